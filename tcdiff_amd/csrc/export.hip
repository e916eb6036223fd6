// The pose export of GaussianDiffusion.render_sample (reference model/diffusion.py:811-988), gfx950, fp32, one launch:
// the sampler's normalized rows -> un-normalised SMPL root translations, axis-angle poses, FK joint positions and contacts.
//
//   unnormalize (clip to [-1, 1], then (x - min_) / scale_)   dataset/preprocess.py:39-43, dataset/scaler.py:80-83
//   split contacts / root / 6-D rotations, ax_from_6v          model/diffusion.py:818-838, dataset/quaternion.py:28-32
//   LONG: the window stitch (root cross-fade, slerp)           model/diffusion.py:841-897, dataset/quaternion.py:35-71
//   SMPLSkeleton.forward                                        vis.py:358-406
//
// One thread per output pose (frame, dancer).  A stitched frame reads at most two windows, so the stitch needs no
// communication between threads.  The per-pose arithmetic is csrc/fk_math.h (shared with the training kernels and the host
// build of tests/host).  A few thousand poses per song, off the sampler's hot path: no LDS, no MFMA.
#include "common.h"
#include "fk_math.h"
#include "tcdiff_hip.h"

#define TC_EXPORT_C 151           // 4 contacts, 3 root, 24 x 6 rotation

// un-normalised column c of a sample row: torch.clip keeps NaN, so no fminf / fmaxf here
DEVINL float unnorm(const float* __restrict__ row, const float* __restrict__ scale, const float* __restrict__ mn, int c) {
#pragma clang fp contract(off)
    float x = row[c];
    x = x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x);
    return (x - mn[c]) / scale[c];
}

// axis-angle of rotation j of an un-normalised row (ax_from_6v on the un-normalised 6-D values)
DEVINL V3 row_axis_angle(const float* __restrict__ row, const float* __restrict__ scale, const float* __restrict__ mn, int j) {
    float d6[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d6[k] = unnorm(row, scale, mn, 7 + 6 * j + k);
    return axis_angle_from_quat(quat_from_6d(d6));
}

__global__ __launch_bounds__(64) void pose_export_kernel(const float* __restrict__ x, int b, int S, int dn, int mode,
                                                        const float* __restrict__ scale, const float* __restrict__ mn,
                                                        const float* __restrict__ fade, FkSkel sk, long P,
                                                        float* __restrict__ trans, float* __restrict__ poses,
                                                        float* __restrict__ joints, float* __restrict__ contact) {
#pragma clang fp contract(off)      // the cross-fade is two rounded products and one rounded sum, as in the reference
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    float aa[TC_FK_J * 3], root[3];
    if (mode == TC_EXPORT_NORMAL) {
        // row p of the flattened [b][S * dn] samples is pose p
        const float* row = x + p * TC_EXPORT_C;
        for (int c = 0; c < 4; ++c) contact[p * 4 + c] = unnorm(row, scale, mn, c);
        for (int c = 0; c < 3; ++c) root[c] = unnorm(row, scale, mn, 4 + c);
        for (int j = 0; j < TC_FK_J; ++j) {
            const V3 a = row_axis_angle(row, scale, mn, j);
            aa[3 * j] = a.x; aa[3 * j + 1] = a.y; aa[3 * j + 2] = a.z;
        }
    } else {
        // frame t of the song: window k = t / h owns it from its first half, window k - 1 from its second half
        const int h = S / 2;
        const long t = p / dn;
        const int d = (int)(p - t * dn);
        const int k = (int)(t / h);
        const bool has_l = k >= 1, has_r = k < b;
        const int fl = (int)(t - (long)(k - 1) * h), fr = (int)(t - (long)k * h);      // local frames in windows k - 1, k
        const float* rl = has_l ? x + (((long)(k - 1) * S + fl) * dn + d) * TC_EXPORT_C : nullptr;
        const float* rr = has_r ? x + (((long)k * S + fr) * dn + d) * TC_EXPORT_C : nullptr;
        // fade[0..h) = linspace(0, 1, h) (fade_in and the slerp weight), fade[h..2h) = linspace(1, 0, h) (fade_out)
        const float wl = (has_l && k - 1 < b - 1) ? fade[fl] : 1.0f;          // fl in [h, 2h)
        const float wr = (has_r && k > 0) ? fade[fr] : 1.0f;
        for (int c = 0; c < 3; ++c) {
            float s = 0.0f;
            if (has_l) s = s + unnorm(rl, scale, mn, 4 + c) * wl;
            if (has_r) s = s + unnorm(rr, scale, mn, 4 + c) * wr;
            root[c] = s;
        }
        for (int j = 0; j < TC_FK_J; ++j) {
            V3 a;
            if (has_l && has_r) {
                const Q4 ql = quat_from_axis_angle(row_axis_angle(rl, scale, mn, j));
                const Q4 qr = quat_from_axis_angle(row_axis_angle(rr, scale, mn, j));
                a = axis_angle_from_quat(quat_slerp(ql, qr, fade[fr]));
            } else {
                a = row_axis_angle(has_l ? rl : rr, scale, mn, j);
            }
            aa[3 * j] = a.x; aa[3 * j + 1] = a.y; aa[3 * j + 2] = a.z;
        }
    }
    float jt[TC_FK_J * 3];
    fk_forward(aa, root, sk, jt, nullptr);
    for (int c = 0; c < 3; ++c) trans[p * 3 + c] = root[c];
#pragma unroll
    for (int q = 0; q < TC_FK_J * 3; ++q) {
        poses[p * (TC_FK_J * 3) + q] = aa[q];
        joints[p * (TC_FK_J * 3) + q] = jt[q];
    }
}

extern "C" int tcdiff_pose_export(const float* samples, int b, int S, int dn, int mode, const float* scale,
                                  const float* min_, const float* fade, const int* parents, const float* offsets,
                                  float* smpl_trans, float* smpl_poses, float* full_pose, float* contact,
                                  hipStream_t stream) {
    if (!samples || !scale || !min_ || !parents || !offsets || !smpl_trans || !smpl_poses || !full_pose) return TC_ERR_ARG;
    if (b < 1 || S < 1 || dn < 1) return TC_ERR_ARG;
    if (mode == TC_EXPORT_NORMAL) {
        if (!contact) return TC_ERR_ARG;
    } else if (mode == TC_EXPORT_LONG) {
        if (S % 2 != 0 || !fade) return TC_ERR_ARG;
    } else {
        return TC_ERR_ARG;
    }
    FkSkel sk;
    for (int j = 0; j < TC_FK_J; ++j) sk.has_children[j] = 0;
    for (int j = 0; j < TC_FK_J; ++j) {
        sk.parent[j] = parents[j];
        if (parents[j] >= j) return TC_ERR_ARG;          // a parent must precede its children
        if (parents[j] >= 0) sk.has_children[parents[j]] = 1;
        for (int k = 0; k < 3; ++k) sk.off[j][k] = offsets[3 * j + k];
    }
    const long P = mode == TC_EXPORT_NORMAL ? (long)b * S * dn : ((long)S + (long)(S / 2) * (b - 1)) * dn;
    hipLaunchKernelGGL(pose_export_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, stream, samples, b, S, dn, mode, scale,
                       min_, fade, sk, P, smpl_trans, smpl_poses, full_pose, contact);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
