// The group metrics (include/tcdiff_group.h), gfx950: body contact of capsule skeletons, crossings of the dancers' floor paths and the
// lagged correlation of their joint speeds, per clip and pair of dancers.  Three launches for any number of clips:
//   1. gap:     one wave per (clip, pair, frame), four frames per workgroup -- both dancers' joints staged in LDS as float64, the 529
//               bone pairs over the lanes in nine rounds, a cross-lane minimum of (gap, code) over a total order
//   2. signals: one workgroup per (clip, dancer) -- the 24 speeds of every frame, then a wave per joint: mean, deviation and the
//               standardised signal, lane l summing l, l + 64, ... and a fixed butterfly over the lanes
//   3. pairs:   one workgroup per (clip, pair) -- the gap plane reduced over the frames, the crossings (a thread per step of a
//               looping over the steps of b inside the window), the correlations (an item per (joint, lag), summed in ascending t)
// No atomics; every floating-point sum has one order, every minimum is over a total order: the same input gives the same bits.
// The arithmetic is csrc/group_math.h (shared with the host build of tests/host).  A few thousand frames per call, off the sampler's
// hot path: no MFMA; LDS holds the staged joints (launch 1) and the table of correlations (launch 3).
#include "common.h"
#include "group_math.h"
#include "tcdiff_group.h"

#define TCG_THREADS 256
#define TCG_MAX_LAGS (2 * TC_GROUP_MAX_LAG + 1)
static_assert(TC_GROUP_LAUNCHES == 3, "three launches");
static_assert(TC_GROUP_WS_PAIR_FRAME == 8 + 4 && TC_GROUP_WS_DANCER_FRAME == 8 * TCG_J && TC_GROUP_WS_DANCER == 8 * TCG_J,
              "the header states the workspace: a gap and a code per (pair, frame), 24 z per (dancer, frame), 24 sigma per dancer");

struct TcgSkel { int parent[TCG_J]; double radius[TCG_J]; };

// pair p of dn dancers in lexicographic order -> (a, b), a < b
DEVINL void pair_of(int p, int dn, int* a, int* b) {
    int first = 0;
    while (p >= dn - 1 - first) {
        p -= dn - 1 - first;
        ++first;
    }
    *a = first;
    *b = first + 1 + p;
}

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCG_THREADS) void group_gap_kernel(const float* __restrict__ joints, long s0, long s1, long s2, int dn, int T,
                                                                int P, int quads, TcgSkel sk, double* __restrict__ gap,
                                                                int* __restrict__ closest) {
    __shared__ double s_j[4][2][TCG_J * 3];
    __shared__ double s_rad[TCG_J];
    __shared__ int s_par[TCG_J];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < TCG_J; ++k) {          // constant indices: the skeleton stays in the kernel's arguments, not in scratch
            s_par[k] = sk.parent[k];
            s_rad[k] = sk.radius[k];
        }
    }
    const long cp = (long)blockIdx.x / quads;                 // clip P + pair
    const int t = (int)((long)blockIdx.x - cp * quads) * 4 + wave;
    const long c = cp / P;
    int a, b;
    pair_of((int)(cp - c * P), dn, &a, &b);
    const bool live = t < T;
    if (live) {
        for (int e = lane; e < 2 * TCG_J * 3; e += 64) {
            const int who = e >= TCG_J * 3, k = e - who * TCG_J * 3;
            s_j[wave][who][k] = (double)joints[c * s0 + (long)(who ? b : a) * s1 + (long)t * s2 + k];
        }
    }
    __syncthreads();
    if (!live) return;
    const double* Ja = s_j[wave][0];
    const double* Jb = s_j[wave][1];
    TcgBest best;
    best.v = 0.0;
    best.code = -1;
    for (int k = lane; k < TCG_BONE_PAIRS; k += 64) {         // ascending codes on a lane
        const int i = 1 + k / 23, j = 1 + k % 23;
        const int pi = s_par[i], pj = s_par[j];
        const double d = tcg_seg_dist(tcg_v(Ja[3 * pi], Ja[3 * pi + 1], Ja[3 * pi + 2]), tcg_v(Ja[3 * i], Ja[3 * i + 1], Ja[3 * i + 2]),
                                      tcg_v(Jb[3 * pj], Jb[3 * pj + 1], Jb[3 * pj + 2]), tcg_v(Jb[3 * j], Jb[3 * j + 1], Jb[3 * j + 2]));
        TcgBest cand;
        cand.v = tcg_gap(d, s_rad[i], s_rad[j]);
        cand.code = TCG_J * i + j;
        if (best.code < 0 || tcg_before(cand, best)) best = cand;
    }
    for (int o = 32; o >= 1; o >>= 1) {                       // every lane holds a candidate: 64 <= 529
        TcgBest other;
        other.v = __shfl_xor(best.v, o);
        other.code = __shfl_xor(best.code, o);
        if (tcg_before(other, best)) best = other;
    }
    if (lane == 0) {
        gap[cp * T + t] = best.v;
        closest[cp * T + t] = best.code;
    }
}

// ---- launch 2 -------------------------------------------------------------------------------------------------------------------------------
DEVINL double wave_sum(double v) {          // bit 5 first, then 4, ... 0; a + b == b + a, so every lane ends with the same bits
#pragma clang fp contract(off)
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(TCG_THREADS) void group_signals_kernel(const float* __restrict__ joints, long s0, long s1, long s2, int dn, int T,
                                                                    double* __restrict__ z, double* __restrict__ sigma) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long q = blockIdx.x;                                // clip dn + dancer
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    const int N = T - 1;
    const float* J = joints + c * s0 + (long)d * s1;
    double* x = z + q * TCG_J * T;                            // [24][T], N of every row used
    for (int t = tid; t < N; t += TCG_THREADS) {
        const float* J0 = J + (long)t * s2;
        const float* J1 = J0 + s2;
        for (int j = 0; j < TCG_J; ++j) x[(long)j * T + t] = tcg_speed(J0, J1, j);
    }
    __syncthreads();                                          // the speeds are complete (workgroup-scope visibility of the global stores)
    for (int j = wave; j < TCG_J; j += 4) {
        double* xj = x + (long)j * T;
        double sum = 0.0;
        for (int t = lane; t < N; t += 64) sum = sum + xj[t];
        const double mu = wave_sum(sum) / (double)N;
        double ss = 0.0;
        for (int t = lane; t < N; t += 64) {
            const double dl = xj[t] - mu;
            ss = ss + dl * dl;
        }
        const double sg = sqrt(wave_sum(ss) / (double)N);
        for (int t = lane; t < N; t += 64) xj[t] = tcg_standard(xj[t], mu, sg);          // a lane rewrites what it alone read
        if (lane == 0) sigma[q * TCG_J + j] = sg;
    }
}

// ---- launch 3 -------------------------------------------------------------------------------------------------------------------------------
DEVINL long block_sum(long x, long* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // the previous total has been read
    red[tid] = x;
    __syncthreads();
    for (int o = TCG_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(TCG_THREADS) void group_pairs_kernel(
    const float* __restrict__ joints, long s0, long s1, long s2, int dn, int T, int P, int up, int window, int max_lag, double sigma_floor,
    const double* __restrict__ gap, const int* __restrict__ closest, const double* __restrict__ z, const double* __restrict__ sigma,
    double* __restrict__ contact_rate, double* __restrict__ gap_min, long* __restrict__ episodes, long* __restrict__ closest_min,
    long* __restrict__ crossings, double* __restrict__ crossing_rate, double* __restrict__ sync, long* __restrict__ sync_lag,
    double* __restrict__ sync_zero) {
#pragma clang fp contract(off)
    __shared__ long s_cnt[TCG_THREADS];
    __shared__ double s_val[TCG_THREADS];
    __shared__ int s_code[TCG_THREADS];
    __shared__ double s_rho[TCG_MAX_LAGS * TCG_J];
    __shared__ double s_R[TCG_MAX_LAGS];
    __shared__ int s_part[TCG_J];
    const int tid = threadIdx.x;
    const long cp = blockIdx.x;
    const long c = cp / P;
    int a, b;
    pair_of((int)(cp - c * P), dn, &a, &b);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int N = T - 1;

    // ---- 1. the gap plane over the frames ----
    {
        const double* g = gap + cp * T;
        long n_neg = 0, n_start = 0;
        TcgBest best;
        best.v = 0.0;
        best.code = -1;
        for (int t = tid; t < T; t += TCG_THREADS) {
            const double v = g[t];
            const bool neg = v < 0.0;
            n_neg += neg;
            n_start += neg && !(t > 0 && g[t - 1] < 0.0);     // a run starts here
            if (tcg_finite(v)) {
                TcgBest cand;
                cand.v = v;
                cand.code = t;
                if (tcg_before_finite(cand, best)) best = cand;
            }
        }
        n_neg = block_sum(n_neg, s_cnt);
        n_start = block_sum(n_start, s_cnt);
        s_val[tid] = best.v;
        s_code[tid] = best.code;
        __syncthreads();
        for (int o = TCG_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) {
                TcgBest mine, other;
                mine.v = s_val[tid]; mine.code = s_code[tid];
                other.v = s_val[tid + o]; other.code = s_code[tid + o];
                if (tcg_before_finite(other, mine)) {
                    s_val[tid] = other.v;
                    s_code[tid] = other.code;
                }
            }
            __syncthreads();
        }
        if (tid == 0) {
            const int t = s_code[0];
            contact_rate[cp] = (double)n_neg / (double)T;
            episodes[cp] = n_start;
            gap_min[cp] = t < 0 ? nan : s_val[0];
            const int code = t < 0 ? 0 : closest[cp * T + t];
            closest_min[3 * cp] = t;
            closest_min[3 * cp + 1] = t < 0 ? -1 : code / TCG_J;
            closest_min[3 * cp + 2] = t < 0 ? -1 : code % TCG_J;
        }
    }

    // ---- 2. crossings of the floor paths ----
    {
        const float* Ra = joints + c * s0 + (long)a * s1;
        const float* Rb = joints + c * s0 + (long)b * s1;
        long n = 0;
        for (int t = tid; t < N; t += TCG_THREADS) {
            double sa[4], sb[4];
            tcg_floor(Ra + (long)t * s2, up, &sa[0], &sa[1]);
            tcg_floor(Ra + (long)(t + 1) * s2, up, &sa[2], &sa[3]);
            const long lo = (long)t - window < 0 ? 0 : (long)t - window;
            const long hi = (long)t + window > N - 1 ? N - 1 : (long)t + window;
            tcg_floor(Rb + lo * s2, up, &sb[2], &sb[3]);
#pragma unroll 4
            for (long s = lo; s <= hi; ++s) {
                sb[0] = sb[2];
                sb[1] = sb[3];
                tcg_floor(Rb + (s + 1) * s2, up, &sb[2], &sb[3]);
                n += tcg_cross(sa, sb);
            }
        }
        n = block_sum(n, s_cnt);
        if (tid == 0) {
            crossings[cp] = n;
            crossing_rate[cp] = N >= 1 ? (double)n / (double)N : 0.0;
        }
    }

    // ---- 3. synchrony ----
    const int L = tcg_lags(T, max_lag);
    if (L < 0) {
        if (tid == 0) {
            sync[cp] = nan;
            sync_zero[cp] = nan;
            sync_lag[cp] = 0;
        }
        return;
    }
    const int nl = 2 * L + 1;
    const long qa = c * dn + a, qb = c * dn + b;
    if (tid < TCG_J) s_part[tid] = sigma[qa * TCG_J + tid] > sigma_floor && sigma[qb * TCG_J + tid] > sigma_floor;
    __syncthreads();
    const double* za = z + qa * TCG_J * T;
    const double* zb = z + qb * TCG_J * T;
    for (int it = tid; it < TCG_J * nl; it += TCG_THREADS) {          // neighbouring threads: one joint, neighbouring lags
        const int j = it / nl, li = it - j * nl, l = li - L;
        double r = 0.0;
        if (s_part[j]) {
            const int lo = l < 0 ? -l : 0, hi = l < 0 ? N : N - l;
            const double* pa = za + (long)j * T;
            const double* pb = zb + (long)j * T + l;
            double sum = 0.0;
#pragma unroll 8
            for (int t = lo; t < hi; ++t) sum = tcg_corr_add(sum, pa[t], pb[t]);          // unrolled: the loads ahead, the sum in its order
            r = sum / (double)(N - (l < 0 ? -l : l));
        }
        s_rho[li * TCG_J + j] = r;
    }
    __syncthreads();
    if (tid < nl) {
        double R = 0.0;
        int n = 0;
        for (int j = 0; j < TCG_J; ++j)
            if (s_part[j]) {
                R = R + s_rho[tid * TCG_J + j];
                ++n;
            }
        s_R[tid] = n ? R / (double)n : nan;
    }
    __syncthreads();
    if (tid == 0) {
        double best = s_R[0];
        int best_lag = -L;
        if (best != best) {                                   // no joint takes part
            sync[cp] = nan;
            sync_zero[cp] = nan;
            sync_lag[cp] = 0;
        } else {
            for (int li = 1; li < nl; ++li)
                if (tcg_better_lag(s_R[li], li - L, best, best_lag)) {
                    best = s_R[li];
                    best_lag = li - L;
                }
            sync[cp] = best;
            sync_zero[cp] = s_R[L];
            sync_lag[cp] = best_lag;
        }
    }
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
struct TcgShape { long P, pair_frames, dancer_frames, dancers; int quads; };

static int tcg_shape(int b, int dn, int T, int max_lag, TcgShape* s) {
    if (b < 1 || dn < 2 || T < 1) return TC_ERR_ARG;
    if (max_lag < 0 || max_lag > TC_GROUP_MAX_LAG) return TC_ERR_ARG;
    s->P = (long)dn * (dn - 1) / 2;
    s->dancers = (long)b * dn;
    if (s->P > 0x7fffffffl || (long)b * s->P > 0x7fffffffl / T || s->dancers * TCG_J > 0x7fffffffl / T) return TC_ERR_UNSUPPORTED;
    s->pair_frames = (long)b * s->P * T;
    s->dancer_frames = s->dancers * T;
    s->quads = (T + 3) / 4;
    return TC_OK;
}

static long tcg_bytes(const TcgShape& s) {
    const long n = s.pair_frames * TC_GROUP_WS_PAIR_FRAME + s.dancer_frames * TC_GROUP_WS_DANCER_FRAME + s.dancers * TC_GROUP_WS_DANCER;
    return (n + 7) / 8 * 8;
}

extern "C" int tcg_group_workspace(int b, int dn, int T, int max_lag, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    TcgShape s;
    const int rc = tcg_shape(b, dn, T, max_lag, &s);
    if (rc != TC_OK) return rc;
    *bytes = tcg_bytes(s);
    return TC_OK;
}

extern "C" int tcg_group_metrics(const float* joints, const long* joint_strides, int b, int dn, int T, int up, double fps,
                                 const int* parents, const double* radii, int window, int max_lag, double sigma_floor,
                                 void* workspace, long workspace_bytes, double* gap, int* closest,
                                 double* contact_rate, double* gap_min, long* episodes, long* closest_min,
                                 long* crossings, double* crossing_rate, double* sync, long* sync_lag, double* sync_zero,
                                 hipStream_t stream) {
    if (!joints || !joint_strides || !parents || !radii || !workspace || !contact_rate || !gap_min || !episodes || !closest_min ||
        !crossings || !crossing_rate || !sync || !sync_lag || !sync_zero)
        return TC_ERR_ARG;
    if (b < 1 || dn < 2 || T < 1 || up < 0 || up > 2 || !(fps > 0.0) || window < 0) return TC_ERR_ARG;
    if (max_lag < 0 || max_lag > TC_GROUP_MAX_LAG || !(sigma_floor >= 0.0)) return TC_ERR_ARG;
    TcgShape s;
    const int rc = tcg_shape(b, dn, T, max_lag, &s);
    if (rc != TC_OK) return rc;
    for (int k = 0; k < 3; ++k)
        if (joint_strides[k] < 0) return TC_ERR_ARG;
    TcgSkel sk;
    sk.parent[0] = 0;
    sk.radius[0] = 0.0;
    for (int j = 1; j < TCG_J; ++j) {
        if (parents[j] < 0 || parents[j] >= j) return TC_ERR_ARG;          // a parent must precede its child
        sk.parent[j] = parents[j];
    }
    for (int j = 1; j < TCG_J; ++j) {
        if (!(radii[j] >= 0.0) || !tcg_finite(radii[j])) return TC_ERR_ARG;
        sk.radius[j] = radii[j];
    }
    if (workspace_bytes < tcg_bytes(s)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)gap % 8 || (uintptr_t)closest % 4) return TC_ERR_ALIGN;
    // the workspace: z [b dn][24][T], sigma [b dn][24], the gap plane [b P][T] (doubles), then the closest plane [b P][T] (ints)
    double* z = (double*)workspace;
    double* sigma = z + s.dancer_frames * TCG_J;
    double* w_gap = sigma + s.dancers * TCG_J;
    int* w_closest = (int*)(w_gap + s.pair_frames);
    double* g = gap ? gap : w_gap;
    int* cl = closest ? closest : w_closest;
    const long s0 = joint_strides[0], s1 = joint_strides[1], s2 = joint_strides[2];
    const int P = (int)s.P;
    hipLaunchKernelGGL(group_gap_kernel, dim3((unsigned)((long)b * P * s.quads)), dim3(TCG_THREADS), 0, stream, joints, s0, s1, s2, dn, T, P,
                       s.quads, sk, g, cl);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(group_signals_kernel, dim3((unsigned)s.dancers), dim3(TCG_THREADS), 0, stream, joints, s0, s1, s2, dn, T, z, sigma);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(group_pairs_kernel, dim3((unsigned)((long)b * P)), dim3(TCG_THREADS), 0, stream, joints, s0, s1, s2, dn, T, P, up, window,
                       max_lag, sigma_floor, (const double*)g, (const int*)cl, (const double*)z, (const double*)sigma, contact_rate,
                       gap_min, episodes, closest_min, crossings, crossing_rate, sync, sync_lag, sync_zero);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
