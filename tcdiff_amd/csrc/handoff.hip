// The hand-off between the Dance-Beat Navigator and the sampler (reference TCDiff.py:543-556, the evaluation block of
// TrajDecoder/train_traj.py:239-259), gfx950, one launch: the predicted xy trajectories -> forward Kalman filter
// (TrajDecoder/utils/utils_model.py:10-74) -> zero z channel -> x_0 in the sampler's frame-major token order, optionally
// un-normalised (dataset/preprocess.py:39-43).
//
// One thread per (clip, dancer) trajectory, sequential over the frames.  The covariance recursion of this filter does not depend
// on the data, so the gains K_t come in as a float64 table [frames][4][2] (tcdiff_amd/io.py kalman_gains, cached on the device);
// what is left per frame is the state recursion -- a predict and an update of (x, y, vx, vy) in float64, every product and sum
// rounded on its own like numpy's -- and one rounding of the filtered position to fp32.  A few hundred trajectories of at most
// ~900 frames: no LDS, no MFMA; the gain rows are wave-uniform reads, the trajectory reads are strided by whatever view the caller
// holds.
#include "common.h"
#include "tcdiff_hip.h"

struct HandoffNorm {
    int on;
    float scale[3], mn[3];
};

// Normalizer.unnormalize of one channel: torch.clamp keeps NaN, so no fminf / fmaxf here; two rounded fp32 operations
DEVINL float handoff_unnorm(float v, float mn, float scale) {
#pragma clang fp contract(off)
    v = v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v);
    return (v - mn) / scale;
}

__global__ __launch_bounds__(64) void nav_handoff_kernel(const float* __restrict__ traj, long s_b, long s_dn, long s_f, long s_c,
                                                        int dn, int frames, long n_traj, double dt,
                                                        const double* __restrict__ gains, HandoffNorm nm,
                                                        float* __restrict__ smoothed, float* __restrict__ x0) {
#pragma clang fp contract(off)      // the float64 recursion rounds after every operation, as the numpy form does
    const long tr = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tr >= n_traj) return;
    const long c = tr / dn;
    const int d = (int)(tr - c * dn);
    const float* z = traj + c * s_b + d * s_dn;
    double x = (double)z[0], y = (double)z[s_c], vx = 0.0, vy = 0.0;
    const float zc = nm.on ? handoff_unnorm(0.0f, nm.mn[2], nm.scale[2]) : 0.0f;
    float* sm = smoothed ? smoothed + tr * frames * 2 : nullptr;
    float* xo = x0 ? x0 + (c * frames * dn + d) * 3 : nullptr;          // token f * dn + d of clip c
#pragma unroll 8
    for (int f = 0; f < frames; ++f) {
        const double z0 = (double)z[f * s_f], z1 = (double)z[f * s_f + s_c];
        const double* K = gains + (long)f * 8;
        x = x + dt * vx;                                                  // predict: x = F x
        y = y + dt * vy;
        const double r0 = z0 - x, r1 = z1 - y;                            // update: residual, x += K_t residual
        x = x + (K[0] * r0 + K[1] * r1);
        y = y + (K[2] * r0 + K[3] * r1);
        vx = vx + (K[4] * r0 + K[5] * r1);
        vy = vy + (K[6] * r0 + K[7] * r1);
        float ox = (float)x, oy = (float)y;                               // the one rounding to fp32
        if (nm.on) {
            ox = handoff_unnorm(ox, nm.mn[0], nm.scale[0]);
            oy = handoff_unnorm(oy, nm.mn[1], nm.scale[1]);
        }
        if (sm) {
            sm[2 * f] = ox;
            sm[2 * f + 1] = oy;
        }
        if (xo) {
            float* t = xo + (long)f * dn * 3;
            t[0] = ox;
            t[1] = oy;
            t[2] = zc;
        }
    }
}

extern "C" int tcdiff_nav_handoff(const float* traj, long s_b, long s_dn, long s_f, long s_c, int b, int dn, int frames, double dt,
                                  const double* gains, const float* scale, const float* min_, float* smoothed, float* x0,
                                  hipStream_t stream) {
    if (!traj || !gains || (!smoothed && !x0)) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || frames < 1) return TC_ERR_ARG;
    if ((scale == nullptr) != (min_ == nullptr)) return TC_ERR_ARG;
    HandoffNorm nm;
    nm.on = scale ? 1 : 0;
    for (int k = 0; k < 3; ++k) {
        nm.scale[k] = scale ? scale[k] : 1.0f;
        nm.mn[k] = min_ ? min_[k] : 0.0f;
    }
    const long n_traj = (long)b * dn;
    if ((n_traj + 63) / 64 > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(nav_handoff_kernel, dim3((unsigned)((n_traj + 63) / 64)), dim3(64), 0, stream, traj, s_b, s_dn, s_f, s_c, dn,
                       frames, n_traj, dt, gains, nm, smoothed, x0);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
