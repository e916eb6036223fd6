// The jitter scores and the rotation filter (include/tcdiff_smooth.h), gfx950.
//   tcw_smoothness, one launch: one workgroup of 256 per (clip, dancer), 64 frames at a time -- every thread forms the second and third
//               differences of six (frame, joint) pairs, world and root-relative, into LDS; then lane l of the first wave adds its
//               frame's terms in joint order and the frame's sum to its lane sum, so the order of every sum is the stated one; lane 0 adds
//               the 64 lane sums in lane order; the maxima are a tree over a total order.
//   tcw_smooth, two launches for any number of clips:
//   1. filter:  one workgroup per (clip, dancer, tile of 64 frames) -- the quaternions of the tile and its halo formed once and staged in
//               LDS as float64, one row per joint and component (lanes on consecutive frames read consecutive words), the root's three
//               rows likewise; wave w filters the joints w, w + 4, ..., lane l the tile's frame l, in ascending tap order, and measures
//               the change of what it stores; the tile's largest changes and its copied outputs go to the workspace
//   2. FK:      one thread per (clip, dancer, frame) for fk_forward of the output if asked, as many again for the input if asked; trailing
//               blocks, a thread per (clip, dancer), reduce launch 1's tiles (they read nothing this launch writes)
// No atomics; every floating-point sum has one order, every maximum is over a total order: the same input gives the same bits.
// The arithmetic is csrc/smooth_math.h on csrc/footlock_math.h and csrc/fk_math.h (shared with the host build of tests/host).  A few
// thousand frames per call, off the sampler's hot path: no MFMA; LDS holds the staged quaternions and the terms of 64 frames.
#include "common.h"
#include "fk_math.h"
#include "smooth_math.h"
#include "tcdiff_smooth.h"

#define TCW_THREADS 256
#define TCW_WAVES (TCW_THREADS / 64)
#define TCW_ROW (TCW_J + 1)               // the terms of a frame in LDS: 25 doubles, so that 64 lanes on 64 frames spread over the banks
static_assert(TC_SMOOTH_LAUNCHES == 2 && TC_SMOOTH_TILE == 64, "two launches; a tile is one wave of frames");
static_assert(TC_SMOOTH_WS_TILE == 2 * sizeof(double) + sizeof(int), "the header states the workspace: two maxima and a count per tile");
static_assert(TCW_J == TC_FK_J && TCW_J % TCW_WAVES == 0, "the joints divide over the waves");
static_assert(TC_SMOOTH_MAX_WINDOW % 2 == 1 && TC_SMOOTH_MAX_WINDOW < 64, "the halo of a tile is shorter than a tile");
static_assert((64 * TCW_J) % TCW_THREADS == 0, "the (frame, joint) pairs of 64 frames divide over the threads");

// ---- tcw_smoothness ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCW_THREADS) void smoothness_kernel(const float* __restrict__ joints, long s0, long s1, long s2, int dn, int T,
                                                                 double f2, double f3, double* __restrict__ accel_mean,
                                                                 double* __restrict__ jitter, double* __restrict__ jitter_local,
                                                                 double* __restrict__ root_jitter, double* __restrict__ accel_max,
                                                                 double* __restrict__ jitter_max, int* __restrict__ accel_peak,
                                                                 int* __restrict__ jitter_peak, int* __restrict__ terms) {
#pragma clang fp contract(off)
    __shared__ double s_term[3][64 * TCW_ROW];                // a, k, kl of 64 frames; NaN: no such term, or a term that is not finite
    __shared__ double s_sum[4][64];
    __shared__ int s_cnt[4][64];
    __shared__ double s_max[2][TCW_THREADS];
    __shared__ int s_at[2][2][TCW_THREADS];
    const int tid = threadIdx.x;
    const long seq = blockIdx.x;                              // clip dn + dancer
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const float* J = joints + c * s0 + (long)d * s1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double sum_a = 0.0, sum_k = 0.0, sum_l = 0.0, sum_r = 0.0;          // the first wave's: lane l owns the frames l, l + 64, ...
    int n_a = 0, n_k = 0, n_l = 0, n_r = 0;
    TcwPeak top_a, top_k;
    top_a.v = top_k.v = 0.0;
    top_a.t = top_k.t = top_a.j = top_k.j = -1;
    for (int t0 = 0; t0 < T - 1; t0 += 64) {
        for (int e = tid; e < 64 * TCW_J; e += TCW_THREADS) {          // consecutive threads on consecutive joints of a frame
            const int l = e / TCW_J, j = e - l * TCW_J, t = t0 + l;
            double a = nan, k = nan, kl = nan;
            if (t >= 1 && t < T - 1) {
                const bool third = t < T - 2;                 // frame t + 2 exists
                const float* Fm = J + (long)(t - 1) * s2;
                const float* F0 = J + (long)t * s2;
                const float* F1 = J + (long)(t + 1) * s2;
                const float* F2 = J + (long)(third ? t + 2 : t + 1) * s2;
                const TckV pm = tcw_point(Fm + 3 * j), p0 = tcw_point(F0 + 3 * j), p1 = tcw_point(F1 + 3 * j), p2 = tcw_point(F2 + 3 * j);
                TcwPeak cand;
                cand.t = t;
                cand.j = j;
                a = cand.v = tcw_accel(pm, p0, p1, f2);
                if (tcw_finite(a) && tcw_beats(cand, top_a)) top_a = cand;
                if (third) {
                    k = cand.v = tcw_jerk(pm, p0, p1, p2, f3);
                    if (tcw_finite(k) && tcw_beats(cand, top_k)) top_k = cand;
                    if (j > 0)
                        kl = tcw_jerk(tck_sub(pm, tcw_point(Fm)), tck_sub(p0, tcw_point(F0)), tck_sub(p1, tcw_point(F1)),
                                      tck_sub(p2, tcw_point(F2)), f3);
                }
            }
            s_term[0][l * TCW_ROW + j] = a;
            s_term[1][l * TCW_ROW + j] = k;
            s_term[2][l * TCW_ROW + j] = kl;
        }
        __syncthreads();
        if (tid < 64) {                                       // lane tid, frame t0 + tid: ascending joints to 0.0, then onto the lane's sum
            double fa = 0.0, fk = 0.0, fl = 0.0;
            for (int j = 0; j < TCW_J; ++j) {
                const double a = s_term[0][tid * TCW_ROW + j], k = s_term[1][tid * TCW_ROW + j], kl = s_term[2][tid * TCW_ROW + j];
                if (tcw_finite(a)) {
                    fa = fa + a;
                    ++n_a;
                }
                if (tcw_finite(k)) {
                    fk = fk + k;
                    ++n_k;
                    if (j == 0) {
                        sum_r = sum_r + k;
                        ++n_r;
                    }
                }
                if (tcw_finite(kl)) {
                    fl = fl + kl;
                    ++n_l;
                }
            }
            sum_a = sum_a + fa;
            sum_k = sum_k + fk;
            sum_l = sum_l + fl;
        }
        __syncthreads();                                      // the terms have been read
    }
    if (tid < 64) {
        s_sum[0][tid] = sum_a; s_sum[1][tid] = sum_k; s_sum[2][tid] = sum_l; s_sum[3][tid] = sum_r;
        s_cnt[0][tid] = n_a; s_cnt[1][tid] = n_k; s_cnt[2][tid] = n_l; s_cnt[3][tid] = n_r;
    }
    s_max[0][tid] = top_a.v; s_at[0][0][tid] = top_a.t; s_at[0][1][tid] = top_a.j;
    s_max[1][tid] = top_k.v; s_at[1][0][tid] = top_k.t; s_at[1][1][tid] = top_k.j;
    __syncthreads();
    for (int o = TCW_THREADS / 2; o > 0; o >>= 1) {           // a total order: the tree's shape does not matter
        if (tid < o) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                TcwPeak mine, other;
                mine.v = s_max[k][tid]; mine.t = s_at[k][0][tid]; mine.j = s_at[k][1][tid];
                other.v = s_max[k][tid + o]; other.t = s_at[k][0][tid + o]; other.j = s_at[k][1][tid + o];
                if (tcw_beats(other, mine)) {
                    s_max[k][tid] = other.v; s_at[k][0][tid] = other.t; s_at[k][1][tid] = other.j;
                }
            }
        }
        __syncthreads();
    }
    if (tid != 0) return;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    int cnt[4] = {0, 0, 0, 0};
    for (int l = 0; l < 64; ++l)                              // ascending lanes
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tot[k] = tot[k] + s_sum[k][l];
            cnt[k] += s_cnt[k][l];
        }
    accel_mean[seq] = cnt[0] ? tot[0] / (double)cnt[0] : nan;
    jitter[seq] = cnt[1] ? tot[1] / (double)cnt[1] : nan;
    jitter_local[seq] = cnt[2] ? tot[2] / (double)cnt[2] : nan;
    root_jitter[seq] = cnt[3] ? tot[3] / (double)cnt[3] : nan;
    terms[seq] = cnt[1];
    accel_max[seq] = s_at[0][0][0] < 0 ? nan : s_max[0][0];
    jitter_max[seq] = s_at[1][0][0] < 0 ? nan : s_max[1][0];
    accel_peak[2 * seq] = s_at[0][0][0]; accel_peak[2 * seq + 1] = s_at[0][1][0];
    jitter_peak[2 * seq] = s_at[1][0][0]; jitter_peak[2 * seq + 1] = s_at[1][1][0];
}

// ---- tcw_smooth, launch 1 -----------------------------------------------------------------------------------------------------------------------
// the frames a tile stages for a window W: from the first frame's window start to the last frame's window end
struct TcwSpan { int lo, n; };
DEVINL TcwSpan span_of(int t0, int t1, int T, int W) {
    TcwSpan s;
    s.lo = tcw_start(t0, T, W);
    s.n = tcw_start(t1, T, W) + W - s.lo;
    return s;
}

// dynamic LDS: sQ [24][4][S] doubles, sP [3][Sr] doubles
__global__ __launch_bounds__(TCW_THREADS) void smooth_filter_kernel(const float* __restrict__ q, const float* __restrict__ pos, int dn, int T,
                                                                    int tiles, int W, const double* __restrict__ taps, int Wr,
                                                                    const double* __restrict__ root_taps, unsigned mask, int S, int Sr,
                                                                    float* __restrict__ q_out, float* __restrict__ pos_out,
                                                                    double* __restrict__ tile_rot, double* __restrict__ tile_pos,
                                                                    int* __restrict__ tile_copied) {
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    __shared__ double s_rot[TCW_THREADS];
    __shared__ double s_shift[64];
    __shared__ int s_cnt[TCW_THREADS];
    double* sQ = s_mem;
    double* sP = sQ + (long)TCW_J * 4 * S;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long seq = (long)blockIdx.x / tiles;                // clip dn + dancer
    const int t0 = (int)((long)blockIdx.x - seq * tiles) * TC_SMOOTH_TILE;
    const int t1 = min(t0 + TC_SMOOTH_TILE, T) - 1;
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const TcwSpan sr = span_of(t0, t1, T, W), sp = span_of(t0, t1, T, Wr);          // sr.n <= 64 + W - 1 = S, sp.n <= Sr
    for (int e = tid; e < sr.n * TCW_J; e += TCW_THREADS) {   // consecutive threads on consecutive frames of a joint: consecutive LDS words
        const int j = e / sr.n, f = e - j * sr.n;
        const long row = (c * T + sr.lo + f) * dn + d;
        const TckQ Q = tck_quat(q + row * (TCW_J * 3) + 3 * j);
        double* dst = sQ + (long)j * 4 * S + f;
        dst[0] = Q.w; dst[S] = Q.x; dst[2 * S] = Q.y; dst[3 * S] = Q.z;
    }
    for (int e = tid; e < sp.n * 3; e += TCW_THREADS) {
        const int k = e / sp.n, f = e - k * sp.n;
        const long row = (c * T + sp.lo + f) * dn + d;
        sP[k * Sr + f] = (double)pos[row * 3 + k];
    }
    __syncthreads();
    const int t = t0 + lane;
    double rot = 0.0, shift = 0.0;
    int copied = 0;
    if (t < T) {
        const long row = (c * T + t) * dn + d;
        const int s = tcw_start(t, T, W);
        const double* tap = taps + (long)(t - s) * W;
        for (int j = wave; j < TCW_J; j += TCW_WAVES) {
            const float* src = q + row * (TCW_J * 3) + 3 * j;
            float* dst = q_out + row * (TCW_J * 3) + 3 * j;
            TcwRot r;
            r.copied = 1;
            if ((mask >> j) & 1u) {
                r = tcw_filter_quat(tap, sQ + (long)j * 4 * S + (s - sr.lo), S, W, t - s);
                copied += r.copied;
            }
            if (r.copied) {                                   // the input's words; its change is exactly 0
                dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
            } else {                                          // the one rounding to float32, and the change of what is stored
                const float o[3] = {(float)r.r.x, (float)r.r.y, (float)r.r.z};
                dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
                const double v = tcw_rot_change(src, o);
                if (tcw_finite(v) && v > rot) rot = v;
            }
        }
        if (wave == 0) {
            const int sroot = tcw_start(t, T, Wr);
            const double* rtap = root_taps + (long)(t - sroot) * Wr;
            const double x = tcw_tap_sum(rtap, sP + (sroot - sp.lo), Wr), y = tcw_tap_sum(rtap, sP + Sr + (sroot - sp.lo), Wr),
                         z = tcw_tap_sum(rtap, sP + 2 * Sr + (sroot - sp.lo), Wr);
            if (tcw_finite(x) && tcw_finite(y) && tcw_finite(z)) {          // a non-finite float in the window reaches its sum
                const float o[3] = {(float)x, (float)y, (float)z};
                pos_out[row * 3] = o[0]; pos_out[row * 3 + 1] = o[1]; pos_out[row * 3 + 2] = o[2];
                const double v = tck_norm(tck_sub(tcw_point(o), tcw_point(pos + row * 3)));
                if (tcw_finite(v)) shift = v;
            } else {
                pos_out[row * 3] = pos[row * 3]; pos_out[row * 3 + 1] = pos[row * 3 + 1]; pos_out[row * 3 + 2] = pos[row * 3 + 2];
                ++copied;
            }
        }
    }
    s_rot[tid] = rot;
    s_cnt[tid] = copied;
    if (wave == 0) s_shift[lane] = shift;
    __syncthreads();
    for (int o = TCW_THREADS / 2; o > 0; o >>= 1) {           // maxima of numbers and an integer sum: any order gives the same bits
        if (tid < o) {
            s_rot[tid] = fmax(s_rot[tid], s_rot[tid + o]);
            s_cnt[tid] += s_cnt[tid + o];
            if (o < 64) s_shift[tid] = fmax(s_shift[tid], s_shift[tid + o]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        tile_rot[blockIdx.x] = s_rot[0];
        tile_pos[blockIdx.x] = s_shift[0];
        tile_copied[blockIdx.x] = s_cnt[0];
    }
}

// ---- tcw_smooth, launch 2 -----------------------------------------------------------------------------------------------------------------------
// blocks [0, out_blocks): the FK of the output; the next in_blocks: of the input (either count is 0 when that side is not asked for); the
// rest: a thread per (clip, dancer) over its tiles.
// fk_forward indexes its joints by a parent read from the skeleton, so its arrays (and the pose handed to it) live in scratch, as in
// csrc/footlock.hip
__global__ __launch_bounds__(64) void smooth_fk_kernel(const float* __restrict__ q, const float* __restrict__ pos, const float* __restrict__ q_out,
                                                       const float* __restrict__ pos_out, int dn, int T, long N, long dancers, int tiles,
                                                       unsigned out_blocks, unsigned in_blocks, FkSkel fk, const double* __restrict__ tile_rot,
                                                       const double* __restrict__ tile_pos, const int* __restrict__ tile_copied,
                                                       float* __restrict__ joints, float* __restrict__ joints_in, double* __restrict__ max_rot,
                                                       double* __restrict__ max_pos, int* __restrict__ copied) {
    if (blockIdx.x >= out_blocks + in_blocks) {
        const long seq = (long)(blockIdx.x - (out_blocks + in_blocks)) * 64 + threadIdx.x;
        if (seq >= dancers) return;
        double rot = 0.0, shift = 0.0;
        int cnt = 0;
        for (int k = 0; k < tiles; ++k) {
            rot = fmax(rot, tile_rot[seq * tiles + k]);
            shift = fmax(shift, tile_pos[seq * tiles + k]);
            cnt += tile_copied[seq * tiles + k];
        }
        max_rot[seq] = rot;
        max_pos[seq] = shift;
        copied[seq] = cnt;
        return;
    }
    const bool input = blockIdx.x >= out_blocks;
    float* __restrict__ out = input ? joints_in : joints;
    const long i = (long)(blockIdx.x - (input ? out_blocks : 0u)) * 64 + threadIdx.x;          // (clip dn + dancer) T + frame
    if (i >= N) return;
    const long seq = i / T;
    const int t = (int)(i - seq * T);
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const long row = (c * T + t) * dn + d;
    const float* a = (input ? q : q_out) + row * (TCW_J * 3);
    const float* p = (input ? pos : pos_out) + row * 3;
    float aa[TCW_J * 3], jt[TCW_J * 3];
#pragma unroll
    for (int k = 0; k < TCW_J * 3; ++k) aa[k] = a[k];
    const float root[3] = {p[0], p[1], p[2]};
    fk_forward(aa, root, fk, jt, nullptr);
#pragma unroll
    for (int k = 0; k < TCW_J * 3; ++k) out[i * (TCW_J * 3) + k] = jt[k];
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
static int tcw_shape(int b, int dn, int T, int t_min, long* dancers) {
    if (b < 1 || dn < 1 || T < t_min) return TC_ERR_ARG;
    *dancers = (long)b * dn;
    if (*dancers > 0x7fffffffl / T) return TC_ERR_UNSUPPORTED;
    return TC_OK;
}

extern "C" int tcw_smoothness(const float* joints, const long* joint_strides, int b, int dn, int T, double fps, double* accel_mean,
                              double* jitter, double* jitter_local, double* root_jitter, double* accel_max, double* jitter_max,
                              int* accel_peak, int* jitter_peak, int* terms, hipStream_t stream) {
    if (!joints || !joint_strides || !accel_mean || !jitter || !jitter_local || !root_jitter || !accel_max || !jitter_max || !accel_peak ||
        !jitter_peak || !terms)
        return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 4 || !(fps > 0.0 && fps <= 1e6)) return TC_ERR_ARG;
    long dancers;
    const int rc = tcw_shape(b, dn, T, 4, &dancers);
    if (rc != TC_OK) return rc;
    for (int k = 0; k < 3; ++k)
        if (joint_strides[k] < 0) return TC_ERR_ARG;
    if ((uintptr_t)accel_mean % 8 || (uintptr_t)jitter % 8 || (uintptr_t)jitter_local % 8 || (uintptr_t)root_jitter % 8 ||
        (uintptr_t)accel_max % 8 || (uintptr_t)jitter_max % 8 || (uintptr_t)accel_peak % 4 || (uintptr_t)jitter_peak % 4 || (uintptr_t)terms % 4)
        return TC_ERR_ALIGN;
    const double f2 = fps * fps;
    hipLaunchKernelGGL(smoothness_kernel, dim3((unsigned)dancers), dim3(TCW_THREADS), 0, stream, joints, joint_strides[0], joint_strides[1],
                       joint_strides[2], dn, T, f2, f2 * fps, accel_mean, jitter, jitter_local, root_jitter, accel_max, jitter_max, accel_peak,
                       jitter_peak, terms);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

static int tcw_tiles(int T) { return (T + TC_SMOOTH_TILE - 1) / TC_SMOOTH_TILE; }
static long tcw_bytes(long dancers, int T) { return (dancers * tcw_tiles(T) * TC_SMOOTH_WS_TILE + 7) / 8 * 8; }          // dancers tiles <= dancers T

extern "C" int tcw_smooth_workspace(int b, int dn, int T, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    long dancers;
    const int rc = tcw_shape(b, dn, T, 1, &dancers);
    if (rc != TC_OK) return rc;
    *bytes = tcw_bytes(dancers, T);
    return TC_OK;
}

static bool tcw_window_ok(int W) { return W >= 3 && W <= TC_SMOOTH_MAX_WINDOW && (W & 1); }
static int tcw_row(int W) { return TC_SMOOTH_TILE + W - 1; }          // a tile and its halo
static size_t tcw_lds(int W, int Wr) { return ((size_t)TCW_J * 4 * tcw_row(W) + 3 * (size_t)tcw_row(Wr)) * sizeof(double); }

extern "C" int tcw_smooth(const float* q, const float* pos, int b, int dn, int T, int window, const double* taps, int root_window,
                          const double* root_taps, unsigned joints_mask, const int* parents, const float* offsets, void* workspace,
                          long workspace_bytes, float* q_out, float* pos_out, float* joints, float* joints_in, double* max_rot_change,
                          double* max_pos_change, int* copied, hipStream_t stream) {
    if (!q || !pos || !taps || !root_taps || !parents || !offsets || !workspace || !q_out || !pos_out || !max_rot_change || !max_pos_change ||
        !copied)
        return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || !tcw_window_ok(window) || !tcw_window_ok(root_window) || T < window || T < root_window) return TC_ERR_ARG;
    if (joints_mask >> TCW_J) return TC_ERR_ARG;
    long dancers;
    const int rc = tcw_shape(b, dn, T, 1, &dancers);
    if (rc != TC_OK) return rc;
    FkSkel fk;
    for (int j = 0; j < TC_FK_J; ++j) fk.has_children[j] = 0;
    for (int j = 0; j < TC_FK_J; ++j) {
        fk.parent[j] = parents[j];
        if (parents[j] >= j) return TC_ERR_ARG;          // a parent must precede its children
        if (parents[j] >= 0) fk.has_children[parents[j]] = 1;
        for (int k = 0; k < 3; ++k) fk.off[j][k] = offsets[3 * j + k];
    }
    if (workspace_bytes < tcw_bytes(dancers, T)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)taps % 8 || (uintptr_t)root_taps % 8 || (uintptr_t)max_rot_change % 8 ||
        (uintptr_t)max_pos_change % 8)
        return TC_ERR_ALIGN;
    static tc_dev_state st;                                   // the largest windows' LDS, allowed once per device
    const int cus = tc_device_once(st, [](int) {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(smooth_filter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)tcw_lds(TC_SMOOTH_MAX_WINDOW, TC_SMOOTH_MAX_WINDOW));
    });
    if (cus < 0) return cus;
    const int tiles = tcw_tiles(T);
    const long n_tiles = dancers * tiles, N = dancers * T;
    // the workspace: the tiles' largest rotation and root changes (doubles), then their copied counts (ints)
    double* tile_rot = (double*)workspace;
    double* tile_pos = tile_rot + n_tiles;
    int* tile_copied = (int*)(tile_pos + n_tiles);
    hipLaunchKernelGGL(smooth_filter_kernel, dim3((unsigned)n_tiles), dim3(TCW_THREADS), tcw_lds(window, root_window), stream, q, pos, dn, T,
                       tiles, window, taps, root_window, root_taps, joints_mask, tcw_row(window), tcw_row(root_window), q_out, pos_out, tile_rot,
                       tile_pos, tile_copied);
    TC_CHECK_LAUNCH();
    const unsigned fk_blocks = (unsigned)((N + 63) / 64), sum_blocks = (unsigned)((dancers + 63) / 64);
    const unsigned out_blocks = joints ? fk_blocks : 0u, in_blocks = joints_in ? fk_blocks : 0u;
    hipLaunchKernelGGL(smooth_fk_kernel, dim3(out_blocks + in_blocks + sum_blocks), dim3(64), 0, stream, q, pos, (const float*)q_out,
                       (const float*)pos_out, dn, T, N, dancers, tiles, out_blocks, in_blocks, fk, (const double*)tile_rot, (const double*)tile_pos,
                       (const int*)tile_copied, joints, joints_in, max_rot_change, max_pos_change, copied);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
