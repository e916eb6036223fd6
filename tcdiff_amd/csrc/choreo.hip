// The choreography planner and its closing check (include/tcdiff_choreo.h), gfx950.
//   tcc_plan, two launches for any number of clips:
//   1. paths:   one workgroup of 256 per (clip, dancer) -- thread k checks key k and its point, the verdict is one __syncthreads_or;
//               the keys (int32), the points and the PCHIP slopes go to LDS as float64, 9 KiB at 256 keys; then a thread per frame,
//               256 frames at a time, finds its segment by binary search in LDS, evaluates the Hermite form, stores traj and x_0 and
//               leaves the float32 it stored in LDS, from which the steps are formed; the first wave adds the tile's steps so that the
//               order of the path length is the stated one; the maxima are a tree over a total order
//   2. pairs:   one workgroup of 256 per (clip, pair) over the stored traj: the smallest distance over a total order and a count
//   tcc_trajectory_error, one launch: one workgroup of 256 per (clip, dancer), the joints read through their strides; the mean's sum
//               in the same stated order, the maximum and the last counted frame over total orders.
// No atomics; every floating-point sum has one order, every extremum is over a total order: the same input gives the same bits.
// The arithmetic is csrc/choreo_math.h (shared with the host build of tests/host).  A few thousand frames per call, launch latency and
// not work: no MFMA; LDS holds a dancer's spline and one tile of steps.
#include "common.h"
#include "choreo_math.h"
#include "tcdiff_choreo.h"

#define TCC_THREADS 256
static_assert(TC_CHOREO_LAUNCHES == 2 && TC_CHOREO_TILE == TCC_THREADS, "two launches; a tile is one frame a thread");
static_assert(TC_CHOREO_MAX_KEYS <= TCC_THREADS, "a thread per key");
static_assert(TCC_THREADS % 64 == 0, "a tile is whole waves, so that frame t sits on lane t % 64");

struct TccNorm { int on; double scale[2], mn[2]; };

// the tree over a total order and the integer sums that every kernel here ends with; s_v / s_t hold one candidate a thread
template <class Beats>
DEVINL void tcc_reduce_peak(double* s_v, int* s_t, int tid, Beats beats) {
    for (int o = TCC_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            TccPeak mine, other;
            mine.v = s_v[tid]; mine.t = s_t[tid];
            other.v = s_v[tid + o]; other.t = s_t[tid + o];
            if (beats(other, mine)) { s_v[tid] = other.v; s_t[tid] = other.t; }
        }
        __syncthreads();
    }
}
DEVINL void tcc_reduce_count(int* s_n, int tid) {
    for (int o = TCC_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) s_n[tid] += s_n[tid + o];
        __syncthreads();
    }
}

// the terms of one tile are in s_term (NaN: none); lane tid of the first wave adds those of its frames tid, tid + 64, ... in ascending order
DEVINL void tcc_lane_add(const double* s_term, int tid, double& sum) {
#pragma clang fp contract(off)
    for (int w = 0; w < TCC_THREADS / 64; ++w) {
        const double v = s_term[w * 64 + tid];
        if (tcc_finite(v)) sum = sum + v;
    }
}

// ---- tcc_plan, launch 1 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCC_THREADS) void choreo_paths_kernel(const float* __restrict__ points, const int* __restrict__ keys, int keys_per_dancer,
                                                                   const int* __restrict__ counts, int dn, int K, int frames, double fps,
                                                                   TccNorm nm, double max_speed, float* __restrict__ traj, float* __restrict__ x0,
                                                                   int* __restrict__ status, int* __restrict__ clamped, double* __restrict__ speed_max,
                                                                   int* __restrict__ speed_peak, int* __restrict__ too_fast,
                                                                   double* __restrict__ path_length) {
#pragma clang fp contract(off)
    __shared__ int s_key[TC_CHOREO_MAX_KEYS];
    __shared__ double s_y[2][TC_CHOREO_MAX_KEYS], s_d[2][TC_CHOREO_MAX_KEYS];
    __shared__ float s_f[2][TCC_THREADS + 1];                 // the float32 values stored for a tile and for the frame after it
    __shared__ double s_term[TCC_THREADS], s_v[TCC_THREADS];
    __shared__ int s_t[TCC_THREADS], s_n[2][TCC_THREADS];
    const int tid = threadIdx.x;
    const long seq = blockIdx.x;                              // clip dn + dancer
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const float nanf = __int_as_float(0x7fc00000);
    float* tr = traj + seq * frames * 2;
    float* xo = x0 + (c * frames * dn + d) * 3;               // token t dn + d of clip c
    const int count = counts ? counts[seq] : K;
    const int* key = keys + (keys_per_dancer ? seq * K : 0);
    const float* pt = points + seq * K * 2;
    int bad_key = count < 1 || count > K, bad_point = 0;
    if (!bad_key && tid < count) {                            // the padding beyond count is never read
        const int k = key[tid];
        const float px = pt[2 * tid], py = pt[2 * tid + 1];
        bad_key = k < 0 || k >= frames || (tid > 0 && key[tid - 1] >= k);
        bad_point = !(tcc_finite((double)px) && tcc_finite((double)py));
        s_key[tid] = k;
        s_y[0][tid] = (double)px;
        s_y[1][tid] = (double)py;
    }
    bad_key = __syncthreads_or(bad_key);                      // also the barrier after which the keys and points are in LDS
    bad_point = __syncthreads_or(bad_point);
    if (bad_key || bad_point) {
        for (int t = tid; t < frames; t += TCC_THREADS) {
            tr[2 * t] = nanf; tr[2 * t + 1] = nanf;
            float* o = xo + (long)t * dn * 3;
            o[0] = nanf; o[1] = nanf; o[2] = 0.0f;
        }
        if (tid == 0) {
            status[seq] = bad_key ? 1 : 2;
            clamped[seq] = 0; too_fast[seq] = 0; speed_peak[seq] = -1;
            speed_max[seq] = nan; path_length[seq] = nan;
        }
        return;
    }
    if (tid < count) {
        s_d[0][tid] = tcc_slope(s_key, s_y[0], count, tid);
        s_d[1][tid] = tcc_slope(s_key, s_y[1], count, tid);
    }
    __syncthreads();
    double lane_sum = 0.0;                                    // the first wave's: lane l owns the steps of the frames l, l + 64, ...
    TccPeak top;
    top.v = 0.0; top.t = -1;
    int n_clamped = 0, n_fast = 0;
    for (int t0 = 0; t0 < frames; t0 += TCC_THREADS) {
        const int t = t0 + tid;
        if (t < frames) {
            const double vx = tcc_eval(s_key, s_y[0], s_d[0], count, t), vy = tcc_eval(s_key, s_y[1], s_d[1], count, t);
            const float fx = (float)vx, fy = (float)vy;      // the one rounding of traj
            tr[2 * t] = fx; tr[2 * t + 1] = fy;
            s_f[0][tid] = fx; s_f[1][tid] = fy;
            int hit = 0;
            float* o = xo + (long)t * dn * 3;
            if (nm.on) {                                      // the one rounding of x_0, from the float64 value
                o[0] = (float)tcc_x0(vx, nm.scale[0], nm.mn[0], &hit);
                o[1] = (float)tcc_x0(vy, nm.scale[1], nm.mn[1], &hit);
            } else {
                o[0] = fx; o[1] = fy;
            }
            o[2] = 0.0f;
            n_clamped += hit;
        }
        if (tid == 0 && t0 + TCC_THREADS < frames) {          // the frame after the tile, for the tile's last step
            s_f[0][TCC_THREADS] = (float)tcc_eval(s_key, s_y[0], s_d[0], count, t0 + TCC_THREADS);
            s_f[1][TCC_THREADS] = (float)tcc_eval(s_key, s_y[1], s_d[1], count, t0 + TCC_THREADS);
        }
        __syncthreads();
        double step = nan;
        if (t < frames - 1) {
            step = tcc_dist(s_f[0][tid], s_f[1][tid], s_f[0][tid + 1], s_f[1][tid + 1]);
            if (tcc_finite(step)) {
                TccPeak cand;
                cand.v = step * fps; cand.t = t;
                if (tcc_larger(cand, top)) top = cand;
                n_fast += cand.v > max_speed;
            }
        }
        s_term[tid] = step;
        __syncthreads();
        if (tid < 64) tcc_lane_add(s_term, tid, lane_sum);
        __syncthreads();                                      // the tile's floats and steps have been read
    }
    s_v[tid] = top.v; s_t[tid] = top.t;
    s_n[0][tid] = n_clamped; s_n[1][tid] = n_fast;
    if (tid < 64) s_term[tid] = lane_sum;
    __syncthreads();
    tcc_reduce_peak(s_v, s_t, tid, tcc_larger);
    tcc_reduce_count(s_n[0], tid);
    tcc_reduce_count(s_n[1], tid);
    if (tid != 0) return;
    double total = 0.0;
    for (int l = 0; l < 64; ++l) total = total + s_term[l];   // ascending lanes
    status[seq] = 0;
    clamped[seq] = s_n[0][0];
    too_fast[seq] = s_n[1][0];
    speed_peak[seq] = s_t[0];
    speed_max[seq] = s_t[0] < 0 ? nan : s_v[0];
    path_length[seq] = total;
}

// ---- tcc_plan, launch 2 -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCC_THREADS) void choreo_pairs_kernel(const float* __restrict__ traj, int dn, int n_pairs, int frames, double min_distance,
                                                                   double* __restrict__ dist_min, int* __restrict__ dist_min_frame,
                                                                   int* __restrict__ too_close) {
    __shared__ double s_v[TCC_THREADS];
    __shared__ int s_t[TCC_THREADS], s_n[TCC_THREADS];
    const int tid = threadIdx.x;
    const long c = (long)blockIdx.x / n_pairs;
    const int p = (int)((long)blockIdx.x - c * n_pairs);
    int i, j;
    tcc_pair(p, dn, &i, &j);
    const float* A = traj + (c * dn + i) * frames * 2;
    const float* B = traj + (c * dn + j) * frames * 2;
    TccPeak low;
    low.v = 0.0; low.t = -1;
    int n_close = 0;
    for (int t = tid; t < frames; t += TCC_THREADS) {
        TccPeak cand;
        cand.v = tcc_dist(A[2 * t], A[2 * t + 1], B[2 * t], B[2 * t + 1]);
        cand.t = t;
        if (!tcc_finite(cand.v)) continue;                    // a frame with a NaN (a dancer whose status is not 0) is left out
        if (tcc_smaller(cand, low)) low = cand;
        n_close += cand.v < min_distance;
    }
    s_v[tid] = low.v; s_t[tid] = low.t; s_n[tid] = n_close;
    __syncthreads();
    tcc_reduce_peak(s_v, s_t, tid, tcc_smaller);
    tcc_reduce_count(s_n, tid);
    if (tid != 0) return;
    dist_min[blockIdx.x] = s_t[0] < 0 ? __longlong_as_double(0x7ff8000000000000LL) : s_v[0];
    dist_min_frame[blockIdx.x] = s_t[0];
    too_close[blockIdx.x] = s_n[0];
}

// ---- tcc_trajectory_error -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCC_THREADS) void choreo_error_kernel(const float* __restrict__ joints, long s0, long s1, long s2, const float* __restrict__ traj,
                                                                   int dn, int T, int a0, int a1, double* __restrict__ err_mean,
                                                                   double* __restrict__ err_max, double* __restrict__ err_final,
                                                                   int* __restrict__ err_peak, int* __restrict__ counted) {
#pragma clang fp contract(off)
    __shared__ double s_term[TCC_THREADS], s_v[2][TCC_THREADS];
    __shared__ int s_t[2][TCC_THREADS], s_n[TCC_THREADS];
    const int tid = threadIdx.x;
    const long seq = blockIdx.x;                              // clip dn + dancer
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const float* J = joints + c * s0 + (long)d * s1;          // the root is joint 0: the first three floats of a frame
    const float* P = traj + seq * T * 2;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double lane_sum = 0.0;
    TccPeak top, last;
    top.v = last.v = 0.0; top.t = last.t = -1;
    int n = 0;
    for (int t0 = 0; t0 < T; t0 += TCC_THREADS) {
        const int t = t0 + tid;
        double e = nan;
        if (t < T) {
            const float* R = J + (long)t * s2;
            e = tcc_dist(P[2 * t], P[2 * t + 1], R[a0], R[a1]);
            if (tcc_finite(e)) {                              // a non-finite input reaches its distance
                TccPeak cand;
                cand.v = e; cand.t = t;
                if (tcc_larger(cand, top)) top = cand;
                last = cand;                                  // a thread's frames ascend
                ++n;
            }
        }
        s_term[tid] = e;
        __syncthreads();
        if (tid < 64) tcc_lane_add(s_term, tid, lane_sum);
        __syncthreads();
    }
    s_v[0][tid] = top.v; s_t[0][tid] = top.t;
    s_v[1][tid] = last.v; s_t[1][tid] = last.t;
    s_n[tid] = n;
    if (tid < 64) s_term[tid] = lane_sum;
    __syncthreads();
    tcc_reduce_peak(s_v[0], s_t[0], tid, tcc_larger);
    tcc_reduce_peak(s_v[1], s_t[1], tid, tcc_later);
    tcc_reduce_count(s_n, tid);
    if (tid != 0) return;
    double total = 0.0;
    for (int l = 0; l < 64; ++l) total = total + s_term[l];   // ascending lanes
    const int cnt = s_n[0];
    counted[seq] = cnt;
    err_mean[seq] = cnt ? total / (double)cnt : nan;
    err_max[seq] = cnt ? s_v[0][0] : nan;
    err_peak[seq] = s_t[0][0];
    err_final[seq] = cnt ? s_v[1][0] : nan;
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
extern "C" int tcc_plan(const float* points, const int* keys, int keys_per_dancer, const int* counts, int b, int dn, int K, int frames, double fps,
                        const float* scale, const float* min_, double min_distance, double max_speed, float* traj, float* x0, int* status,
                        int* clamped, double* speed_max, int* speed_peak, int* too_fast, double* path_length, double* dist_min,
                        int* dist_min_frame, int* too_close, hipStream_t stream) {
    if (!points || !keys || !traj || !x0 || !status || !clamped || !speed_max || !speed_peak || !too_fast || !path_length) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || K < 1 || K > TC_CHOREO_MAX_KEYS || frames < 1 || !(fps > 0.0 && fps <= 1e6)) return TC_ERR_ARG;
    if (!(min_distance >= 0.0) || !(max_speed >= 0.0) || (scale == nullptr) != (min_ == nullptr)) return TC_ERR_ARG;
    const long dancers = (long)b * dn;
    if (dancers > 0x7fffffffl / frames) return TC_ERR_UNSUPPORTED;
    const long pairs = (long)dn * (dn - 1) / 2;
    if (pairs && (long)b > 0x7fffffffl / pairs) return TC_ERR_UNSUPPORTED;
    if (pairs && (!dist_min || !dist_min_frame || !too_close)) return TC_ERR_ARG;
    if ((uintptr_t)speed_max % 8 || (uintptr_t)path_length % 8 || (pairs && (uintptr_t)dist_min % 8) || (uintptr_t)status % 4 ||
        (uintptr_t)clamped % 4 || (uintptr_t)speed_peak % 4 || (uintptr_t)too_fast % 4 ||
        (pairs && ((uintptr_t)dist_min_frame % 4 || (uintptr_t)too_close % 4)))
        return TC_ERR_ALIGN;
    TccNorm nm;
    nm.on = scale ? 1 : 0;
    for (int k = 0; k < 2; ++k) {
        nm.scale[k] = scale ? (double)scale[k] : 1.0;
        nm.mn[k] = min_ ? (double)min_[k] : 0.0;
    }
    hipLaunchKernelGGL(choreo_paths_kernel, dim3((unsigned)dancers), dim3(TCC_THREADS), 0, stream, points, keys, keys_per_dancer, counts, dn, K, frames,
                       fps, nm, max_speed, traj, x0, status, clamped, speed_max, speed_peak, too_fast, path_length);
    TC_CHECK_LAUNCH();
    if (!pairs) return TC_OK;
    hipLaunchKernelGGL(choreo_pairs_kernel, dim3((unsigned)(b * pairs)), dim3(TCC_THREADS), 0, stream, (const float*)traj, dn, (int)pairs, frames,
                       min_distance, dist_min, dist_min_frame, too_close);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcc_trajectory_error(const float* joints, const long* joint_strides, const float* traj, int b, int dn, int T, int up, double* err_mean,
                                    double* err_max, double* err_final, int* err_peak, int* counted, hipStream_t stream) {
    if (!joints || !joint_strides || !traj || !err_mean || !err_max || !err_final || !err_peak || !counted) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || up < 0 || up > 2) return TC_ERR_ARG;
    const long dancers = (long)b * dn;
    if (dancers > 0x7fffffffl / T) return TC_ERR_UNSUPPORTED;
    for (int k = 0; k < 3; ++k)
        if (joint_strides[k] < 0) return TC_ERR_ARG;
    if ((uintptr_t)err_mean % 8 || (uintptr_t)err_max % 8 || (uintptr_t)err_final % 8 || (uintptr_t)err_peak % 4 || (uintptr_t)counted % 4)
        return TC_ERR_ALIGN;
    const int a0 = up == 0 ? 1 : 0, a1 = up == 2 ? 1 : 2;     // the two components that are not `up`, ascending
    hipLaunchKernelGGL(choreo_error_kernel, dim3((unsigned)dancers), dim3(TCC_THREADS), 0, stream, joints, joint_strides[0], joint_strides[1],
                       joint_strides[2], traj, dn, T, a0, a1, err_mean, err_max, err_final, err_peak, counted);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
