// The self-contact metric (include/tcdiff_selfcontact.h), gfx950: does a capsule of a dancer pass through another capsule of the same
// dancer, per clip and dancer.  Two launches for any number of clips:
//   1. frames:  one wave per (clip, dancer, frame), four frames per workgroup -- the 24 joints staged in LDS as float64, the 253 bone
//               pairs over the lanes in four rounds (a pair that is not listed takes no part), a cross-lane minimum of (gap, code) over
//               a total order, and the four ballots of "deeper than the tolerance" as the frame's penetration words
//   2. dancers: one workgroup per (clip, dancer) -- the gap plane reduced over the frames (counts, episodes, the finite minimum with
//               its frame, the depth sum by the first wave in the stated lane order), then the frames of every bone pair: thread k tests
//               its bit of the frames' words, 64 frames at a time through LDS
// No atomics; the one floating-point sum has one order, every minimum is over a total order: the same input gives the same bits.
// The arithmetic is csrc/group_math.h and csrc/selfcontact_math.h (shared with the host build of tests/host).  A few thousand frames
// per call, off the sampler's hot path: no MFMA; LDS holds the staged joints (launch 1) and a tile of penetration words (launch 2).
#include "common.h"
#include "selfcontact_math.h"
#include "tcdiff_selfcontact.h"

#define TCI_THREADS 256
#define TCI_TILE 64                       // frames of penetration words in LDS at a time (launch 2)
static_assert(TC_SELF_LAUNCHES == 2, "two launches");
static_assert(TC_SELF_PAIRS == TCI_PAIRS && TCI_PAIRS <= TCI_THREADS && TCI_PAIRS <= 64 * TCI_WORDS, "a thread and a bit per pair");
static_assert(TC_SELF_WS_FRAME == 8 * TCI_WORDS + 8 + 4, "the header states the workspace: four words, a gap and a code per frame");
static_assert(TCI_TILE * TCI_WORDS == TCI_THREADS, "a thread loads one word of a tile");

struct TciSkel { int parent[TCG_J]; double radius[TCG_J]; };
struct TciMask { uint64_t word[TCI_WORDS]; };

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCI_THREADS) void selfcontact_frames_kernel(const float* __restrict__ joints, long s0, long s1, long s2, int dn,
                                                                         int T, int quads, TciSkel sk, TciMask mk, double tolerance,
                                                                         double* __restrict__ gap, int* __restrict__ closest,
                                                                         uint64_t* __restrict__ words) {
    __shared__ double s_j[4][TCG_J * 3];
    __shared__ double s_rad[TCG_J];
    __shared__ int s_par[TCG_J];
    __shared__ uint64_t s_mask[TCI_WORDS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < TCG_J; ++k) {          // constant indices: the skeleton stays in the kernel's arguments, not in scratch
            s_par[k] = sk.parent[k];
            s_rad[k] = sk.radius[k];
        }
#pragma unroll
        for (int k = 0; k < TCI_WORDS; ++k) s_mask[k] = mk.word[k];
    }
    const long q = (long)blockIdx.x / quads;                  // clip dn + dancer
    const int t = (int)((long)blockIdx.x - q * quads) * 4 + wave;
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    const bool live = t < T;
    if (live) {
        const float* J = joints + c * s0 + (long)d * s1 + (long)t * s2;
        for (int e = lane; e < TCG_J * 3; e += 64) s_j[wave][e] = (double)J[e];
    }
    __syncthreads();
    if (!live) return;                                        // a frame past the end: masked off, nothing computed
    const double* J = s_j[wave];
    const long row = q * T + t;
    TcgBest best;
    best.v = 0.0;
    best.code = -1;
    for (int r = 0; r < TCI_WORDS; ++r) {                     // ascending codes on a lane
        const int k = lane + 64 * r;
        bool pen = false;
        if (k < TCI_PAIRS && tci_listed(s_mask, k)) {
            int i, j;
            tci_pair_of(k, &i, &j);
            const int pi = s_par[i], pj = s_par[j];
            const double dist = tcg_seg_dist(tcg_v(J[3 * pi], J[3 * pi + 1], J[3 * pi + 2]), tcg_v(J[3 * i], J[3 * i + 1], J[3 * i + 2]),
                                             tcg_v(J[3 * pj], J[3 * pj + 1], J[3 * pj + 2]), tcg_v(J[3 * j], J[3 * j + 1], J[3 * j + 2]));
            TcgBest cand;
            cand.v = tcg_gap(dist, s_rad[i], s_rad[j]);
            cand.code = TCG_J * i + j;
            pen = tci_contact(cand.v, tolerance);
            if (tci_before(cand, best)) best = cand;
        }
        const uint64_t w = __ballot(pen);                     // the wave is whole here: every lane of a live frame takes every round
        if (lane == 0) words[row * TCI_WORDS + r] = w;
    }
    for (int o = 32; o >= 1; o >>= 1) {                       // a lane without a listed pair holds code -1 and loses to every candidate
        TcgBest other;
        other.v = __shfl_xor(best.v, o);
        other.code = __shfl_xor(best.code, o);
        if (tci_before(other, best)) best = other;
    }
    if (lane == 0) {
        gap[row] = best.v;
        closest[row] = best.code;
    }
}

// ---- launch 2 -------------------------------------------------------------------------------------------------------------------------------
DEVINL double wave_sum(double v) {          // bit 5 first, then 4, ... 0; a + b == b + a, so every lane ends with the same bits
#pragma clang fp contract(off)
    for (int o = 32; o >= 1; o >>= 1) v = v + __shfl_xor(v, o);
    return v;
}

DEVINL long block_sum(long x, long* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // the previous total has been read
    red[tid] = x;
    __syncthreads();
    for (int o = TCI_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(TCI_THREADS) void selfcontact_dancers_kernel(int T, double tolerance, const double* __restrict__ gap,
                                                                          const int* __restrict__ closest, const uint64_t* __restrict__ words,
                                                                          double* __restrict__ rate, double* __restrict__ gap_min,
                                                                          long* __restrict__ episodes, long* __restrict__ closest_min,
                                                                          double* __restrict__ depth_mean, long* __restrict__ pair_frames) {
#pragma clang fp contract(off)
    __shared__ long s_cnt[TCI_THREADS];
    __shared__ double s_val[TCI_THREADS];
    __shared__ int s_code[TCI_THREADS];
    __shared__ uint64_t s_w[TCI_TILE * TCI_WORDS];
    __shared__ double s_depth;
    const int tid = threadIdx.x, lane = tid & 63;
    const long q = blockIdx.x;                                // clip dn + dancer
    const double nan = __longlong_as_double(0x7ff8000000000000LL);

    // ---- 1. the gap plane over the frames ----
    const double* g = gap + q * T;
    long n_con = 0, n_start = 0;
    TcgBest best;
    best.v = 0.0;
    best.code = -1;
    for (int t = tid; t < T; t += TCI_THREADS) {
        const double v = g[t];
        const bool con = tci_contact(v, tolerance);
        n_con += con;
        n_start += con && !(t > 0 && tci_contact(g[t - 1], tolerance));          // a run starts here
        if (tcg_finite(v)) {
            TcgBest cand;
            cand.v = v;
            cand.code = t;
            if (tcg_before_finite(cand, best)) best = cand;
        }
    }
    if (tid < 64) {                                           // the depth sum: lane l adds the frames l, l + 64, ... in ascending order
        double sum = 0.0;
        for (int t = lane; t < T; t += 64) {
            const double v = g[t];
            if (tci_contact(v, tolerance)) sum = tci_depth_add(sum, v);
        }
        sum = wave_sum(sum);
        if (tid == 0) s_depth = sum;
    }
    n_con = block_sum(n_con, s_cnt);
    n_start = block_sum(n_start, s_cnt);
    s_val[tid] = best.v;
    s_code[tid] = best.code;
    __syncthreads();
    for (int o = TCI_THREADS / 2; o > 0; o >>= 1) {
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
        rate[q] = (double)n_con / (double)T;
        episodes[q] = n_start;
        gap_min[q] = t < 0 ? nan : s_val[0];
        const int code = t < 0 ? 0 : closest[q * T + t];
        closest_min[3 * q] = t;
        closest_min[3 * q + 1] = t < 0 ? -1 : code / TCG_J;
        closest_min[3 * q + 2] = t < 0 ? -1 : code % TCG_J;
        depth_mean[q] = n_con > 0 ? s_depth / (double)n_con : nan;
    }

    // ---- 2. the frames of every bone pair ----
    const uint64_t* w = words + q * T * TCI_WORDS;
    const long n_words = (long)T * TCI_WORDS;
    long n = 0;
    for (int t0 = 0; t0 < T; t0 += TCI_TILE) {
        __syncthreads();                                      // the previous tile has been read
        const long e = (long)t0 * TCI_WORDS + tid;
        s_w[tid] = e < n_words ? w[e] : 0;                    // frames past the end hold no bit
        __syncthreads();
        if (tid < TCI_PAIRS) {
            const int wi = tid >> 6, bit = tid & 63;
#pragma unroll 8
            for (int tt = 0; tt < TCI_TILE; ++tt) n += (long)((s_w[tt * TCI_WORDS + wi] >> bit) & 1u);
        }
    }
    if (tid < TCI_PAIRS) pair_frames[q * TCI_PAIRS + tid] = n;
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
struct TciShape { long dancers, frames; int quads; };

static int tci_shape(int b, int dn, int T, TciShape* s) {
    if (b < 1 || dn < 1 || T < 1) return TC_ERR_ARG;
    s->dancers = (long)b * dn;
    if (s->dancers > 0x7fffffffl / T) return TC_ERR_UNSUPPORTED;
    s->frames = s->dancers * T;
    s->quads = (T + 3) / 4;
    return TC_OK;
}

static long tci_bytes(const TciShape& s) { return (s.frames * TC_SELF_WS_FRAME + 7) / 8 * 8; }

extern "C" int tci_self_contact_workspace(int b, int dn, int T, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    TciShape s;
    const int rc = tci_shape(b, dn, T, &s);
    if (rc != TC_OK) return rc;
    *bytes = tci_bytes(s);
    return TC_OK;
}

extern "C" int tci_self_contact(const float* joints, const long* joint_strides, int b, int dn, int T, const int* parents, const double* radii,
                                const uint64_t* mask, double tolerance, void* workspace, long workspace_bytes, double* gap, int* closest,
                                double* rate, double* gap_min, long* episodes, long* closest_min, double* depth_mean, long* pair_frames,
                                hipStream_t stream) {
    if (!joints || !joint_strides || !parents || !radii || !mask || !workspace || !rate || !gap_min || !episodes || !closest_min ||
        !depth_mean || !pair_frames)
        return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || !(tolerance >= 0.0) || !tcg_finite(tolerance)) return TC_ERR_ARG;
    TciShape s;
    const int rc = tci_shape(b, dn, T, &s);
    if (rc != TC_OK) return rc;
    for (int k = 0; k < 3; ++k)
        if (joint_strides[k] < 0) return TC_ERR_ARG;
    TciSkel sk;
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
    TciMask mk;
    for (int k = 0; k < TCI_WORDS; ++k) mk.word[k] = mask[k];
    if (mk.word[TCI_WORDS - 1] >> (TCI_PAIRS - 64 * (TCI_WORDS - 1))) return TC_ERR_ARG;          // a bit at k >= 253
    if (!(mk.word[0] | mk.word[1] | mk.word[2] | mk.word[3])) return TC_ERR_ARG;                  // no pair is listed
    if (workspace_bytes < tci_bytes(s)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)gap % 8 || (uintptr_t)closest % 4) return TC_ERR_ALIGN;
    // the workspace: the penetration words [b dn][T][4], the gap plane [b dn][T] (doubles), then the closest plane [b dn][T] (ints)
    uint64_t* words = (uint64_t*)workspace;
    double* w_gap = (double*)(words + s.frames * TCI_WORDS);
    int* w_closest = (int*)(w_gap + s.frames);
    double* g = gap ? gap : w_gap;
    int* cl = closest ? closest : w_closest;
    hipLaunchKernelGGL(selfcontact_frames_kernel, dim3((unsigned)(s.dancers * s.quads)), dim3(TCI_THREADS), 0, stream, joints, joint_strides[0],
                       joint_strides[1], joint_strides[2], dn, T, s.quads, sk, mk, tolerance, g, cl, words);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(selfcontact_dancers_kernel, dim3((unsigned)s.dancers), dim3(TCI_THREADS), 0, stream, T, tolerance, (const double*)g,
                       (const int*)cl, (const uint64_t*)words, rate, gap_min, episodes, closest_min, depth_mean, pair_frames);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
