// The kinematic beats and the monotone time warp (include/tcdiff_beatsync.h), gfx950.  Three launches for any number of clips:
//   1. speed:    tcb_beat_sync -- one workgroup of 64 per (clip, dancer, tile of 63 frames): lane l runs the float32 FK of frame t0 + l into
//                LDS (and joints_in), then forms v of its frame from its own and the next lane's row, and the frame's non-finite mask;
//                tcb_motion_beats -- a thread per (clip, dancer, frame) on the joints it is handed, read in place
//   2. beats:    one workgroup of 256 per warp -- the pooled curve and its filter in LDS, the minima; the kinematic and the music beats
//                compacted into LDS lists by ballot and prefix; a lane per music beat for its nearest kinematic beat (binary search) and
//                for whether it keeps its claim; the serial anchor pass on lane 0 (at most T / 2 items); a lane per anchor for the
//                slopes; a thread per frame for the warp; the reductions, moved and copied of the warp's dancers among them
//   3. resample: one workgroup of 256 per (clip, dancer, tile of 64 frames) -- the 24 slerps and the root of every frame spread over the
//                threads (the transcendental work is here), the result in LDS; then lane l of the first wave runs the FK of frame t0 + l
// No atomics; every floating-point sum has one order, every extremum is over a total order: the same input gives the same bits.
// The arithmetic is csrc/beatsync_math.h on csrc/choreo_math.h, csrc/footlock_math.h and csrc/fk_math.h (shared with the host build of
// tests/host).  A few thousand frames per call, off the sampler's hot path and latency-bound: no MFMA.
#include "common.h"
#include "fk_math.h"
#include "beatsync_math.h"
#include "tcdiff_beatsync.h"

#define TCB_THREADS 256
#define TCB_WAVES (TCB_THREADS / 64)
#define TCB_ROW (TCB_J * 3 + 1)           // a frame's joints in LDS: 73 floats, so that 64 lanes on 64 rows spread over the banks
static_assert(TC_BEATSYNC_LAUNCHES == 3 && TC_BEATSYNC_TILE == 64, "three launches; a tile is one wave of frames");
static_assert(TC_BEATSYNC_WS_FRAME == sizeof(double) + sizeof(int), "the header states the workspace: v and the mask of a frame");
static_assert(TCB_J == TC_FK_J, "one skeleton");

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCB_THREADS) void beat_speed_kernel(const float* __restrict__ joints, long s0, long s1, long s2, int dn, int T, long P,
                                                                 double* __restrict__ ws_v) {
    const long p = (long)blockIdx.x * TCB_THREADS + threadIdx.x;          // (clip dn + dancer) T + frame
    if (p >= P) return;
    const long seq = p / T;
    const int t = (int)(p - seq * T);
    if (t + 1 >= T) return;                                   // v has T - 1 entries; the last slot of a row is never read
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const float* J0 = joints + c * s0 + (long)d * s1 + (long)t * s2;
    ws_v[p] = tcb_speed(J0, J0 + s2);
}

// fk_forward indexes its joints by a parent read from the skeleton, so its arrays (and the pose handed to it) live in scratch, as in
// csrc/smooth.hip
__global__ __launch_bounds__(64) void beat_fk_speed_kernel(const float* __restrict__ q, const float* __restrict__ pos, int dn, int T, int tiles,
                                                           FkSkel fk, float* __restrict__ joints_in, double* __restrict__ ws_v,
                                                           int* __restrict__ ws_mask) {
    __shared__ float sJ[64 * TCB_ROW];
    const int l = threadIdx.x;
    const long seq = (long)blockIdx.x / tiles;                // clip dn + dancer
    const int t0 = (int)((long)blockIdx.x - seq * tiles) * (TC_BEATSYNC_TILE - 1);
    const int t = t0 + l;
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    if (t < T) {
        const long row = (c * T + t) * dn + d;
        float aa[TCB_J * 3], jt[TCB_J * 3];
#pragma unroll
        for (int k = 0; k < TCB_J * 3; ++k) aa[k] = q[row * (TCB_J * 3) + k];
        const float root[3] = {pos[row * 3], pos[row * 3 + 1], pos[row * 3 + 2]};
        fk_forward(aa, root, fk, jt, nullptr);
#pragma unroll
        for (int k = 0; k < TCB_J * 3; ++k) sJ[l * TCB_ROW + k] = jt[k];
        if (l < TC_BEATSYNC_TILE - 1 || t == T - 1) {         // the tile's own frames; lane 63's frame is the next tile's lane 0
            ws_mask[seq * T + t] = (int)tcb_mask(aa, root);
            if (joints_in)
#pragma unroll
                for (int k = 0; k < TCB_J * 3; ++k) joints_in[(seq * T + t) * (TCB_J * 3) + k] = jt[k];
        }
    }
    __syncthreads();
    if (l < TC_BEATSYNC_TILE - 1 && t + 1 < T) ws_v[seq * T + t] = tcb_speed(sJ + l * TCB_ROW, sJ + (l + 1) * TCB_ROW);
}

// ---- launch 2 -------------------------------------------------------------------------------------------------------------------------------
// every thread calls it; flagged threads get their place in the list, every thread the new length
DEVINL int compact(int flag, int base, int* s_cnt, int* place) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    __syncthreads();                                          // the previous counts have been read
    if (lane == 0) s_cnt[wave] = __popcll(m);
    __syncthreads();
    int off = base, total = base;
#pragma unroll
    for (int w = 0; w < TCB_WAVES; ++w) {
        if (w < wave) off += s_cnt[w];
        total += s_cnt[w];
    }
    *place = off + __popcll(m & ((1ull << lane) - 1ull));
    return total;
}

DEVINL int block_sum_int(int x, int* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // the previous total has been read
    red[tid] = x;
    __syncthreads();
    for (int o = TCB_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    return red[0];
}

struct BeatOut {
    double *warp, *speed, *shift_max, *rate_min, *rate_max;
    unsigned char* kin;
    int *status, *kin_count, *music_count, *matched, *dropped, *anchors, *rate_min_frame, *rate_max_frame, *moved, *copied;
};

static size_t tcb_lds(int T) {                                // as the kernel lays it out
    const size_t Tp = ((size_t)T + 1) & ~(size_t)1, h = (size_t)T / 2;
    return (2 * Tp + 8 + h + 4) * sizeof(double) + (2 * (size_t)T + 3 * (h + 2) + (h + 4)) * sizeof(int);
}

// dynamic LDS: A [Tp + 8] doubles (pv; then the anchors' values and slopes), B [Tp] doubles (s; then warp), E [h + 4] doubles (the anchors'
// shifts), kinL [h + 2], musL [T], pick [T], cm [h + 2], ck [h + 2], am [h + 4] ints, Tp = T rounded up to even, h = T / 2
template <bool SYNC>
__global__ __launch_bounds__(TCB_THREADS) void beat_kernel(const double* __restrict__ ws_v, const int* __restrict__ ws_mask,
                                                           const unsigned char* __restrict__ beats, int dn, int T, int share, int max_shift,
                                                           double max_rate, double strength, int rad, const double* __restrict__ weights,
                                                           BeatOut o) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double s_mem[];
    __shared__ int s_cnt[TCB_WAVES];
    __shared__ int s_red[TCB_THREADS];
    __shared__ int s_count;
    __shared__ double s_val[3][TCB_THREADS];
    __shared__ int s_at[2][TCB_THREADS];
    const int tid = threadIdx.x;
    const int Tp = (T + 1) & ~1, h = T / 2, N = T - 1, W = share ? 1 : dn;
    double* A = s_mem;
    double* B = A + Tp + 8;
    double* ae = B + Tp;
    int* kinL = (int*)(ae + h + 4);
    int* musL = kinL + h + 2;
    int* pick = musL + T;
    int* cm = pick + T;
    int* ck = cm + h + 2;
    int* am = ck + h + 2;
    const long wq = blockIdx.x;                               // clip W + warp
    const long c = wq / W;
    const int w = (int)(wq - c * W);
    const int d_first = share ? 0 : w, d_count = share ? dn : 1;
    const double* v0 = ws_v + (c * dn + d_first) * T;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    // a. the warp's curve
    int bad = 0;
    for (int t = tid; t < N; t += TCB_THREADS) {
        double p = v0[t];
        if (share) {
            double sum = 0.0;
            for (int d = 0; d < dn; ++d) sum = sum + v0[(long)d * T + t];
            p = sum / (double)dn;
        }
        A[t] = p;
        bad |= !tcb_finite(p);
    }
    const int status = __syncthreads_or(bad) ? 1 : 0;
    // b. the filter
    for (int t = tid; t < N; t += TCB_THREADS) {
        const double s = tcb_filter(A, N, weights, rad, t);
        B[t] = s;
        o.speed[wq * N + t] = status ? nan : s;
    }
    __syncthreads();
    // c. the minima, and their list
    int nk = 0, place;
    for (int t0 = 0; t0 < T; t0 += TCB_THREADS) {
        const int t = t0 + tid;
        const int flag = t < T && !status && tcb_is_min(B, N, t);
        if (t < T) o.kin[wq * T + t] = (unsigned char)flag;
        nk = compact(flag, nk, s_cnt, &place);
        if (flag) kinL[place] = t;
    }
    if (tid == 0) o.kin_count[wq] = nk;
    if (!SYNC) return;
    // d. the music's beats: the end frames are pinned
    const unsigned char* bt = beats + c * T;
    int nm = 0;
    for (int t0 = 0; t0 < T; t0 += TCB_THREADS) {
        const int t = t0 + tid;
        const int flag = t >= 1 && t <= T - 2 && bt[t] != 0;
        nm = compact(flag, nm, s_cnt, &place);
        if (flag) musL[place] = t;
    }
    __syncthreads();
    // e. every music beat picks its nearest kinematic beat
    for (int i = tid; i < nm; i += TCB_THREADS) {
        const int m = musL[i];
        int p = tcb_nearest(kinL, nk, m);
        if (p >= 0 && (kinL[p] < m ? m - kinL[p] : kinL[p] - m) > max_shift) p = -1;
        pick[i] = p;
    }
    __syncthreads();
    // f. the claims that are kept: the candidates, in ascending m
    int nc = 0;
    for (int i0 = 0; i0 < nm; i0 += TCB_THREADS) {
        const int i = i0 + tid;
        const int flag = i < nm && tcb_keeps(musL, pick, kinL, nm, i);
        nc = compact(flag, nc, s_cnt, &place);
        if (flag) {
            cm[place] = musL[i];
            ck[place] = kinL[pick[i]];
        }
    }
    __syncthreads();                                          // the candidates are complete, and A (pv) has been read
    // g. the anchors: one lane's serial pass
    double* au = A;
    double* ad = A + h + 4;
    if (tid == 0) {
        int dropped = 0;
        const int count = tcb_anchor_pass(cm, ck, nc, T, strength, max_rate, am, au, ae, &dropped);
        s_count = count;
        o.status[wq] = status;
        o.music_count[wq] = nm;
        o.matched[wq] = nc;
        o.dropped[wq] = dropped;
        o.anchors[wq] = count - 2;
    }
    __syncthreads();
    const int count = s_count;
    // h. the slopes
    if (count > 2)
        for (int k = tid; k < count; k += TCB_THREADS) ad[k] = tcc_slope(am, au, count, k) - 1.0;
    __syncthreads();
    // i. the warp (B: s has been read)
    for (int t = tid; t < T; t += TCB_THREADS) {
        const double u = tcb_warp(am, ae, ad, count, T, t);
        B[t] = u;
        o.warp[wq * T + t] = u;
    }
    __syncthreads();
    // j. the reductions
    double shift = 0.0;
    int moved = 0;
    TccPeak lo, hi;
    lo.v = hi.v = 0.0;
    lo.t = hi.t = -1;
    for (int t = tid; t < T; t += TCB_THREADS) {
        const double u = B[t];
        shift = fmax(shift, fabs(u - (double)t));
        moved += u != (double)t;
        if (t < N) {
            TccPeak r;
            r.v = B[t + 1] - u;
            r.t = t;
            if (tcc_smaller(r, lo)) lo = r;
            if (tcc_larger(r, hi)) hi = r;
        }
    }
    s_val[0][tid] = shift; s_val[1][tid] = lo.v; s_val[2][tid] = hi.v;
    s_at[0][tid] = lo.t; s_at[1][tid] = hi.t;
    __syncthreads();
    for (int off = TCB_THREADS / 2; off > 0; off >>= 1) {     // a maximum of numbers and two total orders: the tree's shape does not matter
        if (tid < off) {
            s_val[0][tid] = fmax(s_val[0][tid], s_val[0][tid + off]);
            TccPeak mine, other;
            mine.v = s_val[1][tid]; mine.t = s_at[0][tid]; other.v = s_val[1][tid + off]; other.t = s_at[0][tid + off];
            if (tcc_smaller(other, mine)) { s_val[1][tid] = other.v; s_at[0][tid] = other.t; }
            mine.v = s_val[2][tid]; mine.t = s_at[1][tid]; other.v = s_val[2][tid + off]; other.t = s_at[1][tid + off];
            if (tcc_larger(other, mine)) { s_val[2][tid] = other.v; s_at[1][tid] = other.t; }
        }
        __syncthreads();
    }
    moved = block_sum_int(moved, s_red);
    if (tid == 0) {
        o.shift_max[wq] = s_val[0][0];
        o.rate_min[wq] = s_at[0][0] < 0 ? nan : s_val[1][0];
        o.rate_max[wq] = s_at[1][0] < 0 ? nan : s_val[2][0];
        o.rate_min_frame[wq] = s_at[0][0];
        o.rate_max_frame[wq] = s_at[1][0];
    }
    for (int d = d_first; d < d_first + d_count; ++d) {       // the outputs launch 3 will copy through, from launch 1's masks
        const int* mask = ws_mask + (c * dn + d) * T;
        int copied = 0;
        for (int t = tid; t < T; t += TCB_THREADS) {
            double a;
            const int i = tcb_source(B[t], T, &a);
            if (a != 0.0) copied += __popc((unsigned)(mask[i] | mask[min(i + 1, T - 1)]));
        }
        copied = block_sum_int(copied, s_red);
        if (tid == 0) {
            o.moved[c * dn + d] = moved;
            o.copied[c * dn + d] = copied;
        }
    }
}

// ---- launch 3 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCB_THREADS) void beat_resample_kernel(const float* __restrict__ q, const float* __restrict__ pos,
                                                                    const float* __restrict__ contacts, const double* __restrict__ warp, int dn,
                                                                    int T, int tiles, int share, FkSkel fk, float* __restrict__ q_out,
                                                                    float* __restrict__ pos_out, float* __restrict__ contacts_out,
                                                                    float* __restrict__ joints) {
    __shared__ float sQ[TC_BEATSYNC_TILE * TCB_ROW];
    __shared__ float sP[TC_BEATSYNC_TILE * 3];
    const int tid = threadIdx.x;
    const long seq = (long)blockIdx.x / tiles;                // clip dn + dancer
    const int t0 = (int)((long)blockIdx.x - seq * tiles) * TC_BEATSYNC_TILE;
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const double* wp = warp + (share ? c : seq) * T;
    for (int e = tid; e < TC_BEATSYNC_TILE * (TCB_J + 1); e += TCB_THREADS) {          // consecutive threads on the joints and the root of a frame
        const int l = e / (TCB_J + 1), j = e - l * (TCB_J + 1), t = t0 + l;
        if (t >= T) continue;
        double a;
        const int i = tcb_source(wp[t], T, &a);
        const int i1 = min(i + 1, T - 1);                     // i + 1 wherever a != 0
        const long row = (c * T + t) * dn + d, r0 = (c * T + i) * dn + d, r1 = (c * T + i1) * dn + d;
        if (j < TCB_J) {
            const float *self = q + row * (TCB_J * 3) + 3 * j, *x = q + r0 * (TCB_J * 3) + 3 * j, *y = q + r1 * (TCB_J * 3) + 3 * j;
            float out[3];
            if (a == 0.0) {
                out[0] = x[0]; out[1] = x[1]; out[2] = x[2];
            } else if (tcb_finite3(x) && tcb_finite3(y)) {
                const TckV r = tcb_slerp(x, y, a);
                out[0] = (float)r.x; out[1] = (float)r.y; out[2] = (float)r.z;
            } else {
                out[0] = self[0]; out[1] = self[1]; out[2] = self[2];
            }
            float* dst = q_out + row * (TCB_J * 3) + 3 * j;
            dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
            sQ[l * TCB_ROW + 3 * j] = out[0]; sQ[l * TCB_ROW + 3 * j + 1] = out[1]; sQ[l * TCB_ROW + 3 * j + 2] = out[2];
        } else {
            const float *self = pos + row * 3, *x = pos + r0 * 3, *y = pos + r1 * 3;
            float out[3];
            if (a == 0.0) {
                out[0] = x[0]; out[1] = x[1]; out[2] = x[2];
            } else if (tcb_finite3(x) && tcb_finite3(y)) {
                out[0] = (float)tcb_lerp(x[0], y[0], a); out[1] = (float)tcb_lerp(x[1], y[1], a); out[2] = (float)tcb_lerp(x[2], y[2], a);
            } else {
                out[0] = self[0]; out[1] = self[1]; out[2] = self[2];
            }
            pos_out[row * 3] = out[0]; pos_out[row * 3 + 1] = out[1]; pos_out[row * 3 + 2] = out[2];
            sP[l * 3] = out[0]; sP[l * 3 + 1] = out[1]; sP[l * 3 + 2] = out[2];
            if (contacts) {
                const float* src = contacts + (seq * T + (a < 0.5 ? i : i1)) * 4;
                float* dst = contacts_out + (seq * T + t) * 4;
                dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; dst[3] = src[3];
            }
        }
    }
    __syncthreads();
    const int t = t0 + tid;
    if (tid >= TC_BEATSYNC_TILE || t >= T) return;
    float aa[TCB_J * 3], jt[TCB_J * 3];
#pragma unroll
    for (int k = 0; k < TCB_J * 3; ++k) aa[k] = sQ[tid * TCB_ROW + k];
    const float root[3] = {sP[tid * 3], sP[tid * 3 + 1], sP[tid * 3 + 2]};
    fk_forward(aa, root, fk, jt, nullptr);
#pragma unroll
    for (int k = 0; k < TCB_J * 3; ++k) joints[(seq * T + t) * (TCB_J * 3) + k] = jt[k];
}

// ---- the entry points -----------------------------------------------------------------------------------------------------------------------
static int tcb_shape(int b, int dn, int T, int rad, long* dancers) {
    if (T > TC_BEATSYNC_MAX_FRAMES || rad > TC_BEATSYNC_MAX_RADIUS) return TC_ERR_UNSUPPORTED;
    *dancers = (long)b * dn;
    if (*dancers > 0x7fffffffl / T) return TC_ERR_UNSUPPORTED;
    return TC_OK;
}
static long tcb_bytes(long dancers, int T) { return (dancers * T * TC_BEATSYNC_WS_FRAME + 7) / 8 * 8; }

extern "C" int tcb_beat_sync_workspace(int b, int dn, int T, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1) return TC_ERR_ARG;
    long dancers;
    const int rc = tcb_shape(b, dn, T, 0, &dancers);
    if (rc != TC_OK) return rc;
    *bytes = tcb_bytes(dancers, T);
    return TC_OK;
}

template <bool SYNC>
static int tcb_allow_lds() {                                  // the longest clip's LDS, allowed once per device
    static tc_dev_state st;
    return tc_device_once(st, [](int) {
        return hipFuncSetAttribute(reinterpret_cast<const void*>(beat_kernel<SYNC>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)tcb_lds(TC_BEATSYNC_MAX_FRAMES));
    });
}

extern "C" int tcb_motion_beats(const float* joints, const long* joint_strides, int b, int dn, int T, int share, int rad,
                                const double* weights, void* workspace, long workspace_bytes, double* speed, unsigned char* kin,
                                int* kin_count, hipStream_t stream) {
    if (!joints || !joint_strides || !weights || !workspace || !speed || !kin || !kin_count) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || (share != 0 && share != 1) || rad < 0) return TC_ERR_ARG;
    long dancers;
    const int rc = tcb_shape(b, dn, T, rad, &dancers);
    if (rc != TC_OK) return rc;
    for (int k = 0; k < 3; ++k)
        if (joint_strides[k] < 0) return TC_ERR_ARG;
    if (workspace_bytes < tcb_bytes(dancers, T)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)weights % 8 || (uintptr_t)speed % 8 || (uintptr_t)kin_count % 4) return TC_ERR_ALIGN;
    const int cus = tcb_allow_lds<false>();
    if (cus < 0) return cus;
    const long P = dancers * T;
    double* ws_v = (double*)workspace;
    hipLaunchKernelGGL(beat_speed_kernel, dim3((unsigned)((P + TCB_THREADS - 1) / TCB_THREADS)), dim3(TCB_THREADS), 0, stream, joints,
                       joint_strides[0], joint_strides[1], joint_strides[2], dn, T, P, ws_v);
    TC_CHECK_LAUNCH();
    BeatOut o = {};
    o.speed = speed;
    o.kin = kin;
    o.kin_count = kin_count;
    const long warps = share ? b : dancers;
    hipLaunchKernelGGL(beat_kernel<false>, dim3((unsigned)warps), dim3(TCB_THREADS), tcb_lds(T), stream, (const double*)ws_v, (const int*)nullptr,
                       (const unsigned char*)nullptr, dn, T, share, 0, 1.0, 0.0, rad, weights, o);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcb_beat_sync(const float* q, const float* pos, const float* contacts, const unsigned char* beats, int b, int dn, int T,
                             int share, int max_shift, double max_rate, double strength, int rad, const double* weights, const int* parents,
                             const float* offsets, void* workspace, long workspace_bytes, float* q_out, float* pos_out, float* contacts_out,
                             float* joints, float* joints_in, double* warp, double* speed, unsigned char* kin, int* status, int* kin_count,
                             int* music_count, int* matched, int* dropped, int* anchors, double* shift_max, double* rate_min,
                             double* rate_max, int* rate_min_frame, int* rate_max_frame, int* moved, int* copied, hipStream_t stream) {
    if (!q || !pos || !beats || !weights || !parents || !offsets || !workspace || !q_out || !pos_out || !joints || !warp || !speed || !kin ||
        !status || !kin_count || !music_count || !matched || !dropped || !anchors || !shift_max || !rate_min || !rate_max || !rate_min_frame ||
        !rate_max_frame || !moved || !copied)
        return TC_ERR_ARG;
    if ((contacts == nullptr) != (contacts_out == nullptr)) return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || (share != 0 && share != 1) || rad < 0 || max_shift < 0) return TC_ERR_ARG;
    if (!(max_rate >= 1.0 && max_rate <= 1e6) || !(strength >= 0.0 && strength <= 1.0)) return TC_ERR_ARG;
    long dancers;
    const int rc = tcb_shape(b, dn, T, rad, &dancers);
    if (rc != TC_OK) return rc;
    FkSkel fk;
    for (int j = 0; j < TC_FK_J; ++j) fk.has_children[j] = 0;
    for (int j = 0; j < TC_FK_J; ++j) {
        fk.parent[j] = parents[j];
        if (parents[j] >= j) return TC_ERR_ARG;          // a parent must precede its children
        if (parents[j] >= 0) fk.has_children[parents[j]] = 1;
        for (int k = 0; k < 3; ++k) fk.off[j][k] = offsets[3 * j + k];
    }
    if (workspace_bytes < tcb_bytes(dancers, T)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)weights % 8 || (uintptr_t)warp % 8 || (uintptr_t)speed % 8 || (uintptr_t)shift_max % 8 ||
        (uintptr_t)rate_min % 8 || (uintptr_t)rate_max % 8 || (uintptr_t)status % 4 || (uintptr_t)kin_count % 4 || (uintptr_t)music_count % 4 ||
        (uintptr_t)matched % 4 || (uintptr_t)dropped % 4 || (uintptr_t)anchors % 4 || (uintptr_t)rate_min_frame % 4 ||
        (uintptr_t)rate_max_frame % 4 || (uintptr_t)moved % 4 || (uintptr_t)copied % 4)
        return TC_ERR_ALIGN;
    const int cus = tcb_allow_lds<true>();
    if (cus < 0) return cus;
    const long P = dancers * T;
    double* ws_v = (double*)workspace;                        // the workspace: v of every frame (doubles), then the masks (ints)
    int* ws_mask = (int*)(ws_v + P);
    const int N = T - 1, tiles1 = N < 1 ? 1 : (N + TC_BEATSYNC_TILE - 2) / (TC_BEATSYNC_TILE - 1), tiles3 = (T + TC_BEATSYNC_TILE - 1) / TC_BEATSYNC_TILE;
    hipLaunchKernelGGL(beat_fk_speed_kernel, dim3((unsigned)(dancers * tiles1)), dim3(64), 0, stream, q, pos, dn, T, tiles1, fk, joints_in, ws_v, ws_mask);
    TC_CHECK_LAUNCH();
    BeatOut o = {warp, speed, shift_max, rate_min, rate_max, kin, status, kin_count, music_count, matched, dropped, anchors, rate_min_frame,
                 rate_max_frame, moved, copied};
    const long warps = share ? b : dancers;
    hipLaunchKernelGGL(beat_kernel<true>, dim3((unsigned)warps), dim3(TCB_THREADS), tcb_lds(T), stream, (const double*)ws_v, (const int*)ws_mask, beats,
                       dn, T, share, max_shift, max_rate, strength, rad, weights, o);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(beat_resample_kernel, dim3((unsigned)(dancers * tiles3)), dim3(TCB_THREADS), 0, stream, q, pos, contacts, (const double*)warp, dn, T,
                       tiles3, share, fk, q_out, pos_out, contacts_out, joints);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
