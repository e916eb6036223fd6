// The foot lock (include/tcdiff_footlock.h), gfx950: while a foot is in contact it is held at the mean of where it stood, and hip and
// knee are re-solved by analytic two-bone inverse kinematics.  Three launches for any number of clips:
//   1. frames: one thread per (clip, dancer, frame) -- the float64 chain down both legs and the label, structure-of-arrays workspace
//   2. runs:   one wave per (clip, dancer, leg), lanes over frames in chunks of 64 -- run ends from __ballot, the anchor sums in
//              ascending t, a backward pass (anchors, shifts of the planted frames, the next planted frame) and a forward pass (the
//              previous planted frame, the eased shift, the diagnostics); no atomics, every reduction in a fixed order
//   3. solve:  one thread per (clip, dancer, frame) -- the two-bone solve of both legs, the 24 x 3 pose stored, float32 FK if asked
// The per-frame arithmetic is csrc/footlock_math.h (shared with the host build of tests/host).  A few thousand frames per call, off
// the sampler's hot path: no LDS, no MFMA; the workspace is read and written with consecutive lanes on consecutive frames.
#include "common.h"
#include "fk_math.h"
#include "footlock_math.h"
#include "tcdiff_footlock.h"

// the workspace: TCK_ARRAYS arrays of N doubles, then 4 arrays of N int32 (g and next-planted per leg); N = b dn T frame slots,
// slot = (clip dn + dancer) T + frame
enum { TCK_PH = 0, TCK_PK = 3, TCK_PA = 6, TCK_PE = 9, TCK_RH = 12, TCK_RK = 16, TCK_RA = 20, TCK_D = 24, TCK_LEG = 27, TCK_R0 = 54,
       TCK_ARRAYS = 58 };
static_assert(TCK_ARRAYS * 8 + 16 == TC_FOOTLOCK_WS_PER_FRAME, "the header states the workspace of one frame");
static_assert(TC_FOOTLOCK_CHUNK == 64 && TC_FOOTLOCK_LAUNCHES == 3, "a chunk is one wave of frames; three launches");

struct TckSkel { float off[2][12]; double l1[2], l2[2]; };          // per leg: the offsets of hip, knee, ankle, toe; the bone lengths

DEVINL void put_v(double* __restrict__ w, long N, int arr, long i, TckV v) {
    w[(long)arr * N + i] = v.x; w[(long)(arr + 1) * N + i] = v.y; w[(long)(arr + 2) * N + i] = v.z;
}
DEVINL TckV get_v(const double* __restrict__ w, long N, int arr, long i) {
    return tck_v(w[(long)arr * N + i], w[(long)(arr + 1) * N + i], w[(long)(arr + 2) * N + i]);
}
DEVINL void put_q(double* __restrict__ w, long N, int arr, long i, TckQ q) {
    w[(long)arr * N + i] = q.w; w[(long)(arr + 1) * N + i] = q.x; w[(long)(arr + 2) * N + i] = q.y; w[(long)(arr + 3) * N + i] = q.z;
}
DEVINL TckQ get_q(const double* __restrict__ w, long N, int arr, long i) {
    return tck_q(w[(long)arr * N + i], w[(long)(arr + 1) * N + i], w[(long)(arr + 2) * N + i], w[(long)(arr + 3) * N + i]);
}
DEVINL TckLeg get_leg(const double* __restrict__ w, long N, int leg, long i) {
    TckLeg g;
    const int a = leg * TCK_LEG;
    g.Ph = get_v(w, N, a + TCK_PH, i); g.Pk = get_v(w, N, a + TCK_PK, i); g.Pa = get_v(w, N, a + TCK_PA, i); g.Pe = get_v(w, N, a + TCK_PE, i);
    g.Rh = get_q(w, N, a + TCK_RH, i); g.Rk = get_q(w, N, a + TCK_RK, i); g.Ra = get_q(w, N, a + TCK_RA, i);
    return g;
}
// the input row of slot i: rows are (clip, frame, dancer)
DEVINL long row_of(long i, int dn, int T) {
    const long seq = i / T;
    const int t = (int)(i - seq * T);
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    return (c * T + t) * dn + d;
}
DEVINL TckLeg leg_of_row(const float* __restrict__ q, const float* __restrict__ pos, long row, const TckSkel& sk, int leg, TckQ* R0_out) {
    const float* a = q + row * (TC_FK_J * 3);
    const TckQ R0 = tck_quat(a);
    const TckV P0 = tck_v((double)pos[row * 3], (double)pos[row * 3 + 1], (double)pos[row * 3 + 2]);
    if (R0_out) *R0_out = R0;
    return tck_leg_fk(R0, P0, a + 3 * (1 + leg), a + 3 * (4 + leg), a + 3 * (7 + leg), sk.off[leg]);
}

// ---- launch 1 -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void footlock_frames_kernel(const float* __restrict__ q, const float* __restrict__ pos,
                                                            const float* __restrict__ contacts, long s0, long s1, long s2, long s3, int dn, int T,
                                                            long N, float threshold, double still, TckSkel sk, double* __restrict__ w,
                                                            int* __restrict__ gi) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const long seq = i / T;
    const int t = (int)(i - seq * T);
    const long c = seq / dn;
    const int d = (int)(seq - c * dn);
    const long row = (c * T + t) * dn + d;
#pragma unroll
    for (int leg = 0; leg < 2; ++leg) {
        TckQ R0;
        const TckLeg g = leg_of_row(q, pos, row, sk, leg, &R0);
        const int a = leg * TCK_LEG;
        put_v(w, N, a + TCK_PH, i, g.Ph); put_v(w, N, a + TCK_PK, i, g.Pk); put_v(w, N, a + TCK_PA, i, g.Pa); put_v(w, N, a + TCK_PE, i, g.Pe);
        put_q(w, N, a + TCK_RH, i, g.Rh); put_q(w, N, a + TCK_RK, i, g.Rk); put_q(w, N, a + TCK_RA, i, g.Ra);
        if (leg == 0) put_q(w, N, TCK_R0, i, R0);
        bool ca, ce;
        if (contacts) {
            const float* k = contacts + c * s0 + d * s1 + t * s2;
            ca = k[leg * s3] > threshold;
            ce = k[(2 + leg) * s3] > threshold;
        } else if (t == T - 1) {
            ca = ce = true;
        } else {
            const TckLeg n = leg_of_row(q, pos, row + dn, sk, leg, nullptr);          // frame t + 1, recomputed
            ca = tck_norm(tck_sub(n.Pa, g.Pa)) < still;
            ce = tck_norm(tck_sub(n.Pe, g.Pe)) < still;
        }
        gi[(long)leg * N + i] = ca ? 1 : (ce ? 2 : 0);
    }
}

// ---- launch 2 -------------------------------------------------------------------------------------------------------------------------------
DEVINL double lane_of(double v, int lane) {          // lane is wave-uniform
    const long b = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(b & 0xffffffffl), lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
    return __longlong_as_double((long)(((unsigned long)hi << 32) | lo));
}

__global__ __launch_bounds__(64) void footlock_runs_kernel(int T, long N, int blend, double reach, TckSkel sk, double* __restrict__ w,
                                                          int* __restrict__ gi, int* __restrict__ planted, int* __restrict__ clamped,
                                                          double* __restrict__ max_shift) {
#pragma clang fp contract(off)
    const int leg = blockIdx.x & 1, lane = threadIdx.x;
    const long base = (long)(blockIdx.x >> 1) * T;
    const int* __restrict__ G = gi + (long)leg * N + base;
    int* __restrict__ next = gi + (long)(2 + leg) * N + base;
    const int a = leg * TCK_LEG;
    const int chunks = (T + 63) / 64;

    // pass 1, forward: the anchor of every run, summed in ascending t, left in the d slot of the run's last frame
    int open_g = 0, cnt = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
        const int t = ch * 64 + lane;
        const int g = t < T ? G[t] : 0;
        const int gn = t + 1 < T ? G[t + 1] : 0;
        const TckV P = g ? get_v(w, N, a + (g == 1 ? TCK_PA : TCK_PE), base + t) : tck_v(0.0, 0.0, 0.0);
        const unsigned long ends = __ballot(g != 0 && gn != g);
        unsigned long m = __ballot(g != 0);
        while (m) {
            const int l = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int gl = __builtin_amdgcn_readlane(g, l);
            if (gl != open_g) {          // a run starts; an ankle run that touches a toe run ends where the label changes
                sx = sy = sz = 0.0;
                cnt = 0;
                open_g = gl;
            }
            sx = sx + lane_of(P.x, l);
            sy = sy + lane_of(P.y, l);
            sz = sz + lane_of(P.z, l);
            ++cnt;
            if ((ends >> l) & 1) {
                if (lane == l) put_v(w, N, a + TCK_D, base + t, tck_v(sx / (double)cnt, sy / (double)cnt, sz / (double)cnt));
                open_g = 0;
            }
        }
    }
    __syncthreads();

    // pass 2, backward: the shift of the planted frames and every frame's next planted frame
    double cax = 0.0, cay = 0.0, caz = 0.0;          // the anchor of the first run end beyond this chunk
    int cnext = -1;
    for (int ch = chunks - 1; ch >= 0; --ch) {
        const int t = ch * 64 + lane;
        const int g = t < T ? G[t] : 0;
        const int gn = t + 1 < T ? G[t + 1] : 0;
        const bool end = g != 0 && gn != g;
        const unsigned long ends = __ballot(end), pm = __ballot(g != 0);
        const TckV mine = end ? get_v(w, N, a + TCK_D, base + t) : tck_v(0.0, 0.0, 0.0);
        const unsigned long ahead = ends & (~0ul << lane);
        const int e = ahead ? __ffsll((unsigned long long)ahead) - 1 : lane;
        const double ex = __shfl(mine.x, e), ey = __shfl(mine.y, e), ez = __shfl(mine.z, e);
        if (g) {
            const TckV A = ahead ? tck_v(ex, ey, ez) : tck_v(cax, cay, caz);
            put_v(w, N, a + TCK_D, base + t, tck_sub(A, get_v(w, N, a + (g == 1 ? TCK_PA : TCK_PE), base + t)));
        }
        const unsigned long after = lane == 63 ? 0ul : pm & (~0ul << (lane + 1));
        if (t < T) next[t] = after ? ch * 64 + __ffsll((unsigned long long)after) - 1 : cnext;
        if (ends) {
            const int l = __ffsll((unsigned long long)ends) - 1;
            cax = lane_of(mine.x, l); cay = lane_of(mine.y, l); caz = lane_of(mine.z, l);
        }
        if (pm) cnext = ch * 64 + __ffsll((unsigned long long)pm) - 1;
    }
    __syncthreads();

    // pass 3, forward: the previous planted frame, the eased shift of the frames outside the runs, the diagnostics
    int cprev = -1, n_planted = 0, n_clamped = 0;
    double biggest = 0.0;
    for (int ch = 0; ch < chunks; ++ch) {
        const int t = ch * 64 + lane;
        const int g = t < T ? G[t] : 0;
        const unsigned long pm = __ballot(g != 0);
        const unsigned long before = pm & ((1ul << lane) - 1ul);
        const int t0 = before ? ch * 64 + 63 - __clzll((long long)before) : cprev;
        int st = 0;
        if (t < T) {
            TckV d;
            if (g) {
                d = get_v(w, N, a + TCK_D, base + t);
            } else {
                const int t1 = next[t];
                const TckV d0 = t0 >= 0 ? get_v(w, N, a + TCK_D, base + t0) : tck_v(0.0, 0.0, 0.0);
                const TckV d1 = t1 >= 0 ? get_v(w, N, a + TCK_D, base + t1) : tck_v(0.0, 0.0, 0.0);
                d = tck_ease(t, t0, t1, d0, d1, blend);
                put_v(w, N, a + TCK_D, base + t, d);
            }
            biggest = fmax(biggest, tck_norm(d));
            double rp;
            st = tck_reach(get_v(w, N, a + TCK_PH, base + t), get_v(w, N, a + TCK_PA, base + t), d, sk.l1[leg], sk.l2[leg], reach, &rp);
        }
        n_planted += __popcll(pm);
        n_clamped += __popcll(__ballot(st == 2));
        if (pm) cprev = ch * 64 + 63 - __clzll((long long)pm);
    }
    for (int o = 32; o >= 1; o >>= 1) biggest = fmax(biggest, __shfl_xor(biggest, o));
    if (lane == 0) {
        planted[blockIdx.x] = n_planted;
        clamped[blockIdx.x] = n_clamped;
        max_shift[blockIdx.x] = biggest;
    }
}

// ---- launch 3 -------------------------------------------------------------------------------------------------------------------------------
DEVINL void put_rotvec(float* __restrict__ aa, int j, TckV r) {          // the one rounding to float32
    aa[3 * j] = (float)r.x; aa[3 * j + 1] = (float)r.y; aa[3 * j + 2] = (float)r.z;
}

// WITH_FK: fk_forward indexes its joints by a parent read from the skeleton, so its arrays (and the pose handed to it) live in
// scratch, 1264 bytes a lane, as in csrc/export.hip; the instantiation without it keeps everything in registers
template <bool WITH_FK>
__global__ __launch_bounds__(64) void footlock_solve_kernel(const float* __restrict__ q, const float* __restrict__ pos, int dn, int T, long N,
                                                           double reach, TckSkel sk, FkSkel fk, const double* __restrict__ w,
                                                           float* __restrict__ q_out, float* __restrict__ joints) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const long row = row_of(i, dn, T);
    float aa[TC_FK_J * 3];
#pragma unroll
    for (int k = 0; k < TC_FK_J * 3; ++k) aa[k] = q[row * (TC_FK_J * 3) + k];          // float32 words: what is not solved is not recomputed
    const TckQ R0 = get_q(w, N, TCK_R0, i);
#pragma unroll
    for (int leg = 0; leg < 2; ++leg) {
        const TckV d = get_v(w, N, leg * TCK_LEG + TCK_D, i);
        if (tck_is_zero(d)) continue;
        const TckSolve s = tck_solve(R0, get_leg(w, N, leg, i), d, sk.l1[leg], sk.l2[leg], reach);
        if (s.status == 0) continue;
        put_rotvec(aa, 1 + leg, s.qh);
        put_rotvec(aa, 4 + leg, s.qk);
        put_rotvec(aa, 7 + leg, s.qa);
    }
#pragma unroll
    for (int k = 0; k < TC_FK_J * 3; ++k) q_out[row * (TC_FK_J * 3) + k] = aa[k];
    if (WITH_FK) {
        float jt[TC_FK_J * 3];
        const float root[3] = {pos[row * 3], pos[row * 3 + 1], pos[row * 3 + 2]};
        fk_forward(aa, root, fk, jt, nullptr);
#pragma unroll
        for (int k = 0; k < TC_FK_J * 3; ++k) joints[i * (TC_FK_J * 3) + k] = jt[k];
    }
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
static int tck_shape(int b, int dn, int T, long* N) {
    if (b < 1 || dn < 1 || T < 1) return TC_ERR_ARG;
    const long n = (long)b * dn;
    if (n > 0x3fffffffl || n * T > 0x7fffffffl) return TC_ERR_UNSUPPORTED;          // 2 n blocks in launch 2, int frame slots
    *N = n * T;
    return TC_OK;
}

extern "C" int tck_foot_lock_workspace(int b, int dn, int T, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    long N;
    const int rc = tck_shape(b, dn, T, &N);
    if (rc != TC_OK) return rc;
    *bytes = N * TC_FOOTLOCK_WS_PER_FRAME;
    return TC_OK;
}

extern "C" int tck_foot_lock(const float* q, const float* pos, const float* contacts, const long* contact_strides, int b, int dn, int T,
                             float contact_threshold, double still, int blend, double reach, const int* parents, const float* offsets,
                             void* workspace, long workspace_bytes, float* q_out, float* joints, int* planted, int* clamped,
                             double* max_shift, hipStream_t stream) {
    if (!q || !pos || !parents || !offsets || !workspace || !q_out || !planted || !clamped || !max_shift) return TC_ERR_ARG;
    if (contacts && !contact_strides) return TC_ERR_ARG;
    if (blend < 0 || !(reach > 0.0 && reach < 0.5) || !(still >= 0.0) || contact_threshold != contact_threshold) return TC_ERR_ARG;
    long N;
    const int rc = tck_shape(b, dn, T, &N);
    if (rc != TC_OK) return rc;
    if (blend > 0x3ffffff) return TC_ERR_UNSUPPORTED;
    long s[4] = {0, 0, 0, 0};
    if (contacts)
        for (int k = 0; k < 4; ++k) {
            s[k] = contact_strides[k];
            if (s[k] < 0) return TC_ERR_ARG;
        }
    FkSkel fk;
    for (int j = 0; j < TC_FK_J; ++j) fk.has_children[j] = 0;
    for (int j = 0; j < TC_FK_J; ++j) {
        fk.parent[j] = parents[j];
        if (parents[j] >= j) return TC_ERR_ARG;          // a parent must precede its children
        if (parents[j] >= 0) fk.has_children[parents[j]] = 1;
        for (int k = 0; k < 3; ++k) fk.off[j][k] = offsets[3 * j + k];
    }
    TckSkel sk;
    for (int leg = 0; leg < 2; ++leg) {
        // the legs are hip 1 / 2 under the root, knee 4 / 5, ankle 7 / 8, toe 10 / 11, as in SMPL
        if (parents[0] >= 0 || parents[1 + leg] != 0 || parents[4 + leg] != 1 + leg || parents[7 + leg] != 4 + leg || parents[10 + leg] != 7 + leg)
            return TC_ERR_UNSUPPORTED;
        for (int k = 0; k < 4; ++k)
            for (int c = 0; c < 3; ++c) sk.off[leg][3 * k + c] = offsets[3 * (1 + leg + 3 * k) + c];
        sk.l1[leg] = tck_bone(sk.off[leg] + 3);
        sk.l2[leg] = tck_bone(sk.off[leg] + 6);
        if (!(sk.l1[leg] > 0.0) || !(sk.l2[leg] > 0.0) || !(sk.l1[leg] < 1e30) || !(sk.l2[leg] < 1e30)) return TC_ERR_UNSUPPORTED;
    }
    if (workspace_bytes < N * TC_FOOTLOCK_WS_PER_FRAME) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8) return TC_ERR_ALIGN;
    double* w = (double*)workspace;
    int* gi = (int*)(w + (long)TCK_ARRAYS * N);
    const unsigned blocks = (unsigned)((N + 63) / 64);
    hipLaunchKernelGGL(footlock_frames_kernel, dim3(blocks), dim3(64), 0, stream, q, pos, contacts, s[0], s[1], s[2], s[3], dn, T, N,
                       contact_threshold, still, sk, w, gi);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(footlock_runs_kernel, dim3((unsigned)(2l * b * dn)), dim3(64), 0, stream, T, N, blend, reach, sk, w, gi, planted, clamped,
                       max_shift);
    TC_CHECK_LAUNCH();
    if (joints)
        hipLaunchKernelGGL(footlock_solve_kernel<true>, dim3(blocks), dim3(64), 0, stream, q, pos, dn, T, N, reach, sk, fk, (const double*)w,
                           q_out, joints);
    else
        hipLaunchKernelGGL(footlock_solve_kernel<false>, dim3(blocks), dim3(64), 0, stream, q, pos, dn, T, N, reach, sk, fk, (const double*)w,
                           q_out, joints);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
