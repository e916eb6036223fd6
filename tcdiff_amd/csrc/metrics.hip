// Sample-level physical quality metrics of generated group dances, gfx950, float64 arithmetic on the float32 joint positions
// csrc/export.hip leaves on the device.  Two launches for any number of clips, no host synchronisation, no atomics.
//
//   pfc             physical foot contact score, EDGE (Tseng et al., CVPR 2023), eval/eval_pfc.py: root acceleration with its
//                   downward part removed, normalised by its maximum, times min(ankle, toe) flat speed of both feet
//   contact_*       the model's own contact channels against the displacement the dataset labels them from:
//                   dataset/group_dataset.py:204-207 (|feet[t + 1] - feet[t]| < 0.01), model/diffusion.py:719-733
//   collision_rate  same-frame dancer pairs whose roots are closer than `radius` on the floor
//   beat_align      Bailando (Siyao et al., CVPR 2022), utils/metrics_new.py: motion beats = local minima of the
//                   gaussian-smoothed mean joint speed (scipy.ndimage.gaussian_filter1d, mode "reflect";
//                   scipy.signal.argrelextrema(np.less)), scored against the music's beats
//
// metrics_frame_kernel: one thread per (clip, dancer, frame); reads joints / contacts in place through their element strides and
//   writes planes of [b * dn][T] to the workspace:
//     ws  (double): 0 v (mean joint displacement, t < T - 1) | 1 a (root acceleration norm, t < T - 2) |
//                   2..5 fv (flat displacement of feet 7, 10, 8, 11 between t + 1 and t + 2) |
//                   6..9 cd (3-D displacement of feet 7, 8, 10, 11 between t and t + 1) | 10 s (written by the second launch)
//     iws (int):    0 contact flags (bit k: contacts[t][k] > threshold) | 1 pair hits of this dancer with every later one |
//                   2 motion-beat flags (written by the second launch)
// metrics_sequence_kernel: workgroups [0, b * dn) take one (clip, dancer) each: smoothing, minima, the nearest motion beat of
//   every music beat and the sums; workgroups [b * dn, b * dn + b) add one clip's pair hits.  `s` and the beat flags live in the
//   workspace, so a sequence of any length takes the same path.  Every sum: thread i adds elements i, i + 256, ... in index
//   order, then a fixed tree over the 256 threads -- the same bits on every run.
#include "common.h"
#include "tcdiff_hip.h"

#define TC_MET_THREADS 256
#define TC_MET_WS_V 0
#define TC_MET_WS_A 1
#define TC_MET_WS_FV 2
#define TC_MET_WS_CD 6
#define TC_MET_WS_S 10
#define TC_MET_IW_CONTACT 0
#define TC_MET_IW_HITS 1
#define TC_MET_IW_BEAT 2

// squares of the two components that are not `up`, added in axis order
DEVINL double sq_flat(double dx, double dy, double dz, int up) {
#pragma clang fp contract(off)
    const double p = up == 0 ? dy : dx;
    const double q = up == 2 ? dy : dz;
    return p * p + q * q;
}

// a float32 difference is exact in float64
DEVINL void diff3(const float* __restrict__ hi, const float* __restrict__ lo, double& dx, double& dy, double& dz) {
    dx = (double)hi[0] - (double)lo[0];
    dy = (double)hi[1] - (double)lo[1];
    dz = (double)hi[2] - (double)lo[2];
}

__global__ __launch_bounds__(64) void metrics_frame_kernel(const float* __restrict__ joints, long jsb, long jsd, long jst,
                                                          const float* __restrict__ contacts, long csb, long csd, long cst, int dn,
                                                          int T, long P, int up, double dt, double thr, double radius,
                                                          double* __restrict__ ws, int* __restrict__ iws) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const long q = p / T;                                 // sequence = clip * dn + dancer
    const int t = (int)(p - q * T);
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    const float* J0 = joints + c * jsb + d * jsd + (long)t * jst;
    double v = 0.0, a = 0.0, fv[4] = {0.0, 0.0, 0.0, 0.0}, cd[4] = {0.0, 0.0, 0.0, 0.0};
    int flags = 0, hits = 0;
    double dx, dy, dz;
    if (t + 1 < T) {
        const float* J1 = J0 + jst;
        double sum = 0.0;
        for (int j = 0; j < 24; ++j) {
            diff3(J1 + 3 * j, J0 + 3 * j, dx, dy, dz);
            sum += sqrt(dx * dx + dy * dy + dz * dz);
        }
        v = sum / 24.0;
        const int foot[4] = {7, 8, 10, 11};               // the contact channels' order, dataset/group_dataset.py:204
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            diff3(J1 + 3 * foot[k], J0 + 3 * foot[k], dx, dy, dz);
            cd[k] = sqrt(dx * dx + dy * dy + dz * dz);
        }
        if (contacts) {
            const float* C = contacts + c * csb + d * csd + (long)t * cst;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if ((double)C[k] > thr) flags |= 1 << k;
        }
    }
    if (t + 2 < T) {
        const float *J1 = J0 + jst, *J2 = J1 + jst;
        double ux, uy, uz;
        diff3(J1, J0, dx, dy, dz);
        diff3(J2, J1, ux, uy, uz);
        double ax = (ux / dt - dx / dt) / dt, ay = (uy / dt - dy / dt) / dt, az = (uz / dt - dz / dt) / dt;
        if (up == 0) ax = ax < 0.0 ? 0.0 : ax;            // only the upward part of the vertical acceleration counts
        if (up == 1) ay = ay < 0.0 ? 0.0 : ay;
        if (up == 2) az = az < 0.0 ? 0.0 : az;
        a = sqrt(ax * ax + ay * ay + az * az);
        const int foot[4] = {7, 10, 8, 11};               // EDGE's order: left ankle, left toe, right ankle, right toe
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            diff3(J2 + 3 * foot[k], J1 + 3 * foot[k], dx, dy, dz);
            fv[k] = sqrt(sq_flat(dx, dy, dz, up));
        }
    }
    for (int e = d + 1; e < dn; ++e) {
        diff3(joints + c * jsb + e * jsd + (long)t * jst, J0, dx, dy, dz);
        if (sqrt(sq_flat(dx, dy, dz, up)) < radius) ++hits;
    }
    const long QT = P;
    ws[TC_MET_WS_V * QT + p] = v;
    ws[TC_MET_WS_A * QT + p] = a;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ws[(TC_MET_WS_FV + k) * QT + p] = fv[k];
        ws[(TC_MET_WS_CD + k) * QT + p] = cd[k];
    }
    iws[TC_MET_IW_CONTACT * QT + p] = flags;
    iws[TC_MET_IW_HITS * QT + p] = hits;
}

// fixed tree over the workgroup's 256 values; every thread calls it and gets the total
template <typename V>
DEVINL V block_sum(V x, V* red) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    __syncthreads();                                      // the previous total has been read
    red[tid] = x;
    __syncthreads();
    for (int o = TC_MET_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    return red[0];
}

DEVINL double max_nan(double m, double v) { return (v > m || v != v) ? v : m; }          // numpy's max / minimum propagate NaN
DEVINL double min_nan(double m, double v) { return (v < m || v != v) ? v : m; }

DEVINL double block_max(double x, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
    for (int o = TC_MET_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = max_nan(red[tid], red[tid + o]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(TC_MET_THREADS) void metrics_sequence_kernel(
    double* ws, int* iws, const unsigned char* __restrict__ beats, int has_contacts, int b, int dn, int T, double still, int rad,
    double sigma_smooth, double sigma_beat, double* __restrict__ pfc, double* __restrict__ contact_slide,
    double* __restrict__ contact_break, long* __restrict__ contact_frames, double* __restrict__ collision_rate,
    double* __restrict__ beat_align, long* __restrict__ motion_beats) {
#pragma clang fp contract(off)
    __shared__ double s_red[TC_MET_THREADS];
    __shared__ long s_cnt[TC_MET_THREADS];
    __shared__ double s_w[TC_METRICS_MAX_RADIUS + 1];     // the filter's weights 0 .. rad (symmetric)
    const int tid = threadIdx.x;
    const long Q = (long)b * dn, QT = Q * T;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    if (blockIdx.x >= Q) {                                // one clip's pair hits
        const long c = (long)blockIdx.x - Q;
        const int* h = iws + TC_MET_IW_HITS * QT + c * dn * T;
        long n = 0;
        for (long i = tid; i < (long)dn * T; i += TC_MET_THREADS) n += h[i];
        n = block_sum(n, s_cnt);
        if (tid == 0) {
            const long pairs = (long)dn * (dn - 1) / 2;
            collision_rate[c] = pairs ? (double)n / (double)(T * pairs) : 0.0;
        }
        return;
    }

    const long q = blockIdx.x, base = q * T;
    // ---- 1. pfc ----
    {
        double r = nan;
        if (T >= 3) {
            const int n = T - 2;
            const double* a = ws + TC_MET_WS_A * QT + base;
            const double* f = ws + TC_MET_WS_FV * QT + base;
            double m = 0.0;                               // a >= 0
            for (int t = tid; t < n; t += TC_MET_THREADS) m = max_nan(m, a[t]);
            const double A = block_max(m, s_red);
            if (A == 0.0) {
                r = 0.0;
            } else {
                double sum = 0.0;
                for (int t = tid; t < n; t += TC_MET_THREADS) {
                    const double l = min_nan(f[t], f[QT + t]), rr = min_nan(f[2 * QT + t], f[3 * QT + t]);
                    sum += (l * rr) * (a[t] / A);
                }
                r = block_sum(sum, s_red) / (double)n;
            }
        }
        if (tid == 0) pfc[q] = r;
    }
    // ---- 2. the contact channels ----
    if (has_contacts) {
        const double* cd = ws + TC_MET_WS_CD * QT + base;
        const int* fl = iws + TC_MET_IW_CONTACT * QT + base;
        double sum = 0.0;
        long cnt = 0, brk = 0;
        for (int t = tid; t < T - 1; t += TC_MET_THREADS) {
            const int m = fl[t];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (m >> k & 1) {
                    const double dlt = cd[k * QT + t];
                    sum += dlt;
                    ++cnt;
                    if (dlt >= still) ++brk;
                }
        }
        sum = block_sum(sum, s_red);
        cnt = block_sum(cnt, s_cnt);
        brk = block_sum(brk, s_cnt);
        if (tid == 0) {
            contact_slide[q] = cnt ? sum / (double)cnt : 0.0;
            contact_break[q] = cnt ? (double)brk / (double)cnt : 0.0;
            contact_frames[q] = cnt;
        }
    }
    // ---- 4. beat alignment ----
    if (!beats) return;
    const int N = T - 1;
    const double* v = ws + TC_MET_WS_V * QT + base;
    double* s = ws + TC_MET_WS_S * QT + base;
    int* mb = iws + TC_MET_IW_BEAT * QT + base;
    // scipy.ndimage._filters._gaussian_kernel1d: exp(-0.5 / sigma^2 * x^2) / sum
    const double ks = -0.5 / (sigma_smooth * sigma_smooth);
    for (int x = tid; x <= rad; x += TC_MET_THREADS) s_w[x] = exp(ks * ((double)x * (double)x));
    __syncthreads();
    double wsum = 0.0;                                    // every thread, the same order
    for (int x = -rad; x <= rad; ++x) wsum += s_w[x < 0 ? -x : x];
    __syncthreads();
    for (int x = tid; x <= rad; x += TC_MET_THREADS) s_w[x] = s_w[x] / wsum;
    __syncthreads();
    const int per = 2 * N;
    for (int t = tid; t < N; t += TC_MET_THREADS) {
        double acc = 0.0;
        for (int j = -rad; j <= rad; ++j) {
            int i = t + j;
            if (i < 0 || i >= N) {                        // "reflect": (d c b a | a b c d | d c b a), period 2 N
                i %= per;
                if (i < 0) i += per;
                if (i >= N) i = per - 1 - i;
            }
            acc += s_w[j < 0 ? -j : j] * v[i];
        }
        s[t] = acc;
    }
    __syncthreads();                                      // s is complete (workgroup-scope visibility of the global stores)
    long nm = 0;
    for (int t = tid; t < T; t += TC_MET_THREADS) {
        const int is_min = t > 0 && t < N - 1 && s[t] < s[t - 1] && s[t] < s[t + 1];
        mb[t] = is_min;
        nm += is_min;
    }
    nm = block_sum(nm, s_cnt);                            // (its barriers also complete the flags)
    const unsigned char* bt = beats + (q / dn) * T;
    double sum = 0.0;
    long nb = 0;
    const double den = 2.0 * sigma_beat * sigma_beat;
    for (int t = tid; t < T; t += TC_MET_THREADS) {
        if (!bt[t]) continue;
        ++nb;
        if (!nm) continue;
        int k = 0;                                        // distance to the nearest motion beat: there is one, so k < T
        while (!((t - k >= 0 && mb[t - k]) || (t + k < T && mb[t + k])) && k < T) ++k;
        sum += exp(-((double)k * (double)k) / den);
    }
    sum = block_sum(sum, s_red);
    nb = block_sum(nb, s_cnt);
    if (tid == 0) {
        beat_align[q] = (nb && nm) ? sum / (double)nb : nan;
        motion_beats[q] = nm;
    }
}

extern "C" int tcdiff_motion_metrics(const float* joints, const long* joint_strides, const float* contacts,
                                     const long* contact_strides, const unsigned char* beats, int b, int dn, int T, int up, double fps,
                                     double contact_threshold, double still, double radius, double sigma_smooth, double sigma_beat,
                                     double* ws, int* iws, double* pfc, double* contact_slide, double* contact_break,
                                     long* contact_frames, double* collision_rate, double* beat_align, long* motion_beats,
                                     hipStream_t stream) {
    if (!joints || !joint_strides || !ws || !iws || !pfc || !collision_rate) return TC_ERR_ARG;
    if (contacts && (!contact_strides || !contact_slide || !contact_break || !contact_frames)) return TC_ERR_ARG;
    if (beats && (!beat_align || !motion_beats)) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || up < 0 || up > 2) return TC_ERR_ARG;
    if (!(fps > 0.0) || !(sigma_smooth > 0.0) || !(sigma_beat > 0.0)) return TC_ERR_ARG;
    if (!(4.0 * sigma_smooth + 0.5 <= (double)TC_METRICS_MAX_RADIUS)) return TC_ERR_UNSUPPORTED;
    const int rad = (int)(4.0 * sigma_smooth + 0.5);
    const long Q = (long)b * dn, P = Q * T;
    if ((P + 63) / 64 > 0x7fffffffL || Q + b > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    const long cs[3] = {contacts ? contact_strides[0] : 0, contacts ? contact_strides[1] : 0, contacts ? contact_strides[2] : 0};
    hipLaunchKernelGGL(metrics_frame_kernel, dim3((unsigned)((P + 63) / 64)), dim3(64), 0, stream, joints, joint_strides[0],
                       joint_strides[1], joint_strides[2], contacts, cs[0], cs[1], cs[2], dn, T, P, up, 1.0 / fps, contact_threshold,
                       radius, ws, iws);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(metrics_sequence_kernel, dim3((unsigned)(Q + b)), dim3(TC_MET_THREADS), 0, stream, ws, iws, beats,
                       contacts ? 1 : 0, b, dn, T, still, rad, sigma_smooth, sigma_beat, pfc, contact_slide, contact_break,
                       contact_frames, collision_rate, beat_align, motion_beats);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
