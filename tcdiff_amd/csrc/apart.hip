// Keeping the dancers' bodies apart (include/tcdiff_apart.h), gfx950: contact-driven horizontal shifts of the roots, eased in time.
// 2 rounds + 3 launches for any number of clips:
//   demand  (per round): one wave per (clip, pair, frame), four frames per workgroup -- both dancers' shifted joints staged in LDS as
//           float64, every evaluation of g(m) the 529 bone pairs over the lanes in nine rounds and a cross-lane minimum of (gap, code)
//           over a total order; the iteration's exit is wave-uniform (every lane holds the same minimum)
//   combine (per round): one thread per (clip, dancer, frame) -- the envelope of each of its pairs from the m plane, S updated
//   apply:  one thread per (clip, dancer, frame, row of 3 floats): the 24 joints and the row of pos, copied or shifted
//   verify: the demand kernel with zero iterations on joints_out
//   stats:  one workgroup per (clip, pair) and per (clip, dancer): counts, the finite minimum, the maxima over the frames
// No atomics; every minimum is over a total order, every maximum over exact candidates: the same input gives the same bits.
// The arithmetic is csrc/apart_math.h (shared with the host build of tests/host).  A few thousand frames per call, off the sampler's
// hot path: no MFMA; LDS holds the staged joints.
// Departures from the header's plan: the demand kernel ORs the flag byte itself (lane 0 of the wave that owns the (pair, frame) is the
// byte's only writer, so combine need not look for an owner among its dancers); the moved joints of an evaluation are formed in
// registers from the staged ones, not staged again (a second staging would need a barrier inside a loop whose trip count differs
// between the waves of a workgroup).
#include "common.h"
#include "apart_math.h"
#include "tcdiff_apart.h"

#define TCP_THREADS 256
#define TCP_ROWS 25                       // the 24 joints and the row of pos
static_assert(TC_APART_WS_PAIR_FRAME == 8 + 16 + 8 + 8 + 1 && TC_APART_WS_DANCER_FRAME == 16,
              "the header states the workspace: m, u, two gaps and a flag byte per (pair, frame), S per (dancer, frame)");
static_assert(TC_APART_LAUNCHES(3) == 9, "two launches a round and three");

struct TcpSkel { int parent[TCG_J]; double radius[TCG_J]; };
struct TcpMob { double v[TC_APART_MAX_DANCERS]; };

// pair p of dn dancers in lexicographic order -> (a, b), a < b, and back
DEVINL void tcp_pair_of(int p, int dn, int* a, int* b) {
    int first = 0;
    while (p >= dn - 1 - first) {
        p -= dn - 1 - first;
        ++first;
    }
    *a = first;
    *b = first + 1 + p;
}
DEVINL int tcp_pair_index(int a, int b, int dn) { return a * (2 * dn - a - 1) / 2 + (b - a - 1); }

// ---- demand / verify ------------------------------------------------------------------------------------------------------------------------
// S: the shift plane [b dn][T][2] or NULL (all 0: round 1 and verify).  m_out, u_out, flags: NULL for verify.  gap_out: where the entry
// gap goes, or NULL.  first: the flag byte is written, not ORed.
__global__ __launch_bounds__(TCP_THREADS) void apart_demand_kernel(const float* __restrict__ joints, long s0, long s1, long s2,
                                                                   const double* __restrict__ S, int dn, int T, int P, int quads, int up,
                                                                   TcpSkel sk, TcpMob mob, double margin, int iterations, double max_push,
                                                                   double* __restrict__ m_out, double* __restrict__ u_out,
                                                                   double* __restrict__ gap_out, unsigned char* __restrict__ flags,
                                                                   int first) {
    // 72 doubles a dancer: the lanes of a round read 23 joints of b 24 bytes apart (a few two-way bank conflicts) and 3 or 4 joints
    // of a (broadcasts), as csrc/group.hip's gap kernel does
    __shared__ double s_j[4][2][TCG_J * 3];
    __shared__ double s_rad[TCG_J];
    __shared__ int s_par[TCG_J];
    __shared__ double s_mob[TC_APART_MAX_DANCERS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < TCG_J; ++k) {          // constant indices: the tables stay in the kernel's arguments, not in scratch
            s_par[k] = sk.parent[k];
            s_rad[k] = sk.radius[k];
        }
#pragma unroll
        for (int k = 0; k < TC_APART_MAX_DANCERS; ++k) s_mob[k] = mob.v[k];
    }
    const long cp = (long)blockIdx.x / quads;                 // clip P + pair
    const int t = (int)((long)blockIdx.x - cp * quads) * 4 + wave;
    const long c = cp / P;
    int a, b;
    tcp_pair_of((int)(cp - c * P), dn, &a, &b);
    const bool live = t < T;
    if (live) {
        for (int e = lane; e < 2 * TCG_J * 3; e += 64) {
            const int who = e >= TCG_J * 3, k = e - who * TCG_J * 3;
            const int d = who ? b : a;
            double sx = 0.0, sy = 0.0;
            if (S) {
                const double* s = S + ((c * dn + d) * T + t) * 2;
                sx = s[0];
                sy = s[1];
            }
            s_j[wave][who][k] = tcp_stage(joints[c * s0 + (long)d * s1 + (long)t * s2 + k], k % 3, up, sx, sy);
        }
    }
    __syncthreads();                                          // the only barrier: what follows differs between the waves
    if (!live) return;
    const double* Ja = s_j[wave][0];
    const double* Jb = s_j[wave][1];
    const TcpDir u = tcp_direction(tcp_floor(tcp_joint(Ja, 0), up), tcp_floor(tcp_joint(Jb, 0), up));
    double wa, wb;
    const int free_pair = tcp_shares(s_mob[a], s_mob[b], &wa, &wb);
    double m = 0.0, g0 = 0.0;
    int capped = 0;
    const int evaluations = free_pair ? iterations : 0;
    for (int it = 0;; ++it) {                                 // every lane of the wave takes the same way through this loop
        TcgBest best = tcp_gap_range(Ja, Jb, tcp_move(wa, m, u, up), tcp_move(wb, m, u, up), s_par, s_rad, lane, 64);
        for (int o = 32; o >= 1; o >>= 1) {                   // every lane holds a candidate: 64 <= 529; the codes differ, so the
            TcgBest other;                                    // order is strict and every lane ends with the same pair
            other.v = __shfl_xor(best.v, o);
            other.code = __shfl_xor(best.code, o);
            if (tcg_before(other, best)) best = other;
        }
        if (it == 0) g0 = best.v;
        if (it >= evaluations) break;
        const int go = tcp_step(best.v, margin, max_push, &m);
        capped = go == 2;
        if (go != 1 || it + 1 >= evaluations) break;          // the gap at the final m is asked for by nothing: it is not evaluated
    }
    if (lane == 0) {
        const long at = cp * T + t;
        if (gap_out) gap_out[at] = g0;
        if (m_out) {
            m_out[at] = m;
            u_out[2 * at] = u.x;
            u_out[2 * at + 1] = u.y;
            const unsigned char now = (unsigned char)((m > 0.0 ? TC_APART_PUSHED : 0) | (capped ? TC_APART_CAPPED : 0));
            flags[at] = first ? now : (unsigned char)(flags[at] | now);
        }
    }
}

// ---- combine --------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCP_THREADS) void apart_combine_kernel(const double* __restrict__ m, const double* __restrict__ u,
                                                                    double* __restrict__ S, int dn, int T, int P, int blend, TcpMob mob,
                                                                    int first, long total) {
    __shared__ double s_mob[TC_APART_MAX_DANCERS];
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < TC_APART_MAX_DANCERS; ++k) s_mob[k] = mob.v[k];
    }
    __syncthreads();
    const long idx = (long)blockIdx.x * TCP_THREADS + threadIdx.x;          // (clip dn + dancer) T + frame
    if (idx >= total) return;
    const long q = idx / T;
    const int t = (int)(idx - q * T);
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    TcpDir s;
    s.x = first ? 0.0 : S[2 * idx];
    s.y = first ? 0.0 : S[2 * idx + 1];
    const int lo = t - blend < 0 ? 0 : t - blend, hi = t > T - 1 - blend ? T - 1 : t + blend;
    for (int x = 0; x < dn; ++x) {                            // ascending x = ascending pair order among the pairs that hold d
        if (x == d) continue;
        const int a = x < d ? x : d, b = x < d ? d : x;
        double wa, wb;
        if (!tcp_shares(s_mob[a], s_mob[b], &wa, &wb)) continue;          // pinned: its m is 0
        const long row = (c * P + tcp_pair_index(a, b, dn)) * T;
        const double* mp = m + row;
        double e = 0.0;
        for (int k = lo; k <= hi; ++k) {
            const double cand = tcp_tent(mp[k], k < t ? t - k : k - t, blend);
            e = cand > e ? cand : e;
        }
        TcpDir up_;
        up_.x = u[2 * (row + t)];
        up_.y = u[2 * (row + t) + 1];
        s = d == a ? tcp_shift(s, wa, e, up_, -1) : tcp_shift(s, wb, e, up_, +1);
    }
    S[2 * idx] = s.x;
    S[2 * idx + 1] = s.y;
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------------------
// S NULL (no round ran): everything is copied, and zero_shift, if given, is filled with 0
__global__ __launch_bounds__(TCP_THREADS) void apart_apply_kernel(const float* __restrict__ pos, const float* __restrict__ joints, long s0, long s1,
                                                                  long s2, const double* __restrict__ S, double* __restrict__ zero_shift, int dn,
                                                                  int T, int up, float* __restrict__ pos_out, float* __restrict__ joints_out,
                                                                  long total) {
    const long idx = (long)blockIdx.x * TCP_THREADS + threadIdx.x;          // ((clip dn + dancer) T + frame) 25 + row
    if (idx >= total) return;
    const long f = idx / TCP_ROWS;                            // (clip dn + dancer) T + frame
    const int r = (int)(idx - f * TCP_ROWS);
    const long q = f / T;
    const int t = (int)(f - q * T);
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    const float* src;
    float* dst;
    if (r < TCG_J) {
        src = joints + c * s0 + (long)d * s1 + (long)t * s2 + 3 * r;
        dst = joints_out + f * (TCG_J * 3) + 3 * r;
    } else {
        const long at = ((c * T + t) * dn + d) * 3;
        src = pos + at;
        dst = pos_out + at;
    }
    double sx = 0.0, sy = 0.0;
    if (S) {
        sx = S[2 * f];
        sy = S[2 * f + 1];
    } else if (zero_shift && r == 0) {
        zero_shift[2 * f] = 0.0;
        zero_shift[2 * f + 1] = 0.0;
    }
    if (sx == 0.0 && sy == 0.0) {                             // the words, not the values: a NaN keeps its payload
        const uint32_t* w = (const uint32_t*)src;
        uint32_t* o = (uint32_t*)dst;
        o[0] = w[0];
        o[1] = w[1];
        o[2] = w[2];
        return;
    }
    const int f0 = up == 0 ? 1 : 0, f1 = up == 2 ? 1 : 2;
    const uint32_t* w = (const uint32_t*)src;
    ((uint32_t*)dst)[up] = w[up];
    dst[f0] = tcp_out(src[f0], sx);
    dst[f1] = tcp_out(src[f1], sy);
}

// ---- stats ----------------------------------------------------------------------------------------------------------------------------------
DEVINL long tcp_block_sum(long x, long* red) {
    const int tid = threadIdx.x;
    __syncthreads();                                          // the previous total has been read
    red[tid] = x;
    __syncthreads();
    for (int o = TCP_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid] + red[tid + o];
        __syncthreads();
    }
    return red[0];
}
DEVINL double tcp_block_max(double x, double* red) {          // of values >= 0, none NaN
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = x;
    __syncthreads();
    for (int o = TCP_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] = red[tid + o] > red[tid] ? red[tid + o] : red[tid];
        __syncthreads();
    }
    return red[0];
}
// the smallest finite value of g[0 .. T) in tcg_before_finite's order (the earlier frame on a tie), NaN if there is none
DEVINL double tcp_block_finite_min(const double* g, int T, double* s_val, int* s_code) {
    const int tid = threadIdx.x;
    TcgBest best;
    best.v = 0.0;
    best.code = -1;
    for (int t = tid; t < T; t += TCP_THREADS) {
        const double v = g[t];
        if (tcg_finite(v)) {
            TcgBest cand;
            cand.v = v;
            cand.code = t;
            if (tcg_before_finite(cand, best)) best = cand;
        }
    }
    __syncthreads();
    s_val[tid] = best.v;
    s_code[tid] = best.code;
    __syncthreads();
    for (int o = TCP_THREADS / 2; o > 0; o >>= 1) {
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
    return s_code[0] < 0 ? __longlong_as_double(0x7ff8000000000000LL) : s_val[0];
}

// blocks [0, pair_blocks): a (clip, pair); the rest: a (clip, dancer).  flags NULL: no round ran; S NULL likewise.
__global__ __launch_bounds__(TCP_THREADS) void apart_stats_kernel(const double* __restrict__ gap_before, const double* __restrict__ gap_after,
                                                                  const unsigned char* __restrict__ flags, const double* __restrict__ S, int T,
                                                                  long pair_blocks, long* __restrict__ contact_before,
                                                                  long* __restrict__ contact_after, double* __restrict__ gap_min_before,
                                                                  double* __restrict__ gap_min_after, long* __restrict__ pushed,
                                                                  long* __restrict__ capped, double* __restrict__ max_shift,
                                                                  double* __restrict__ max_step) {
    __shared__ long s_cnt[TCP_THREADS];
    __shared__ double s_val[TCP_THREADS];
    __shared__ int s_code[TCP_THREADS];
    const int tid = threadIdx.x;
    if ((long)blockIdx.x < pair_blocks) {
        const long cp = blockIdx.x;
        const double* gb = gap_before + cp * T;
        const double* ga = gap_after + cp * T;
        long nb = 0, na = 0, np = 0, nc = 0;
        for (int t = tid; t < T; t += TCP_THREADS) {
            nb += gb[t] < 0.0;
            na += ga[t] < 0.0;
            if (flags) {
                const unsigned char fl = flags[cp * T + t];
                np += (fl & TC_APART_PUSHED) != 0;
                nc += (fl & TC_APART_CAPPED) != 0;
            }
        }
        nb = tcp_block_sum(nb, s_cnt);
        na = tcp_block_sum(na, s_cnt);
        np = tcp_block_sum(np, s_cnt);
        nc = tcp_block_sum(nc, s_cnt);
        const double mb = tcp_block_finite_min(gb, T, s_val, s_code);
        const double ma = tcp_block_finite_min(ga, T, s_val, s_code);
        if (tid == 0) {
            contact_before[cp] = nb;
            contact_after[cp] = na;
            pushed[cp] = np;
            capped[cp] = nc;
            gap_min_before[cp] = mb;
            gap_min_after[cp] = ma;
        }
        return;
    }
    const long q = (long)blockIdx.x - pair_blocks;            // clip dn + dancer
    double shift = 0.0, step = 0.0;
    if (S) {
        const double* s = S + q * T * 2;
        for (int t = tid; t < T; t += TCP_THREADS) {
            const double len = tcp_length(s[2 * t], s[2 * t + 1]);
            shift = len > shift ? len : shift;
            if (t > 0) {
                const double st = tcp_length(s[2 * t] - s[2 * t - 2], s[2 * t + 1] - s[2 * t - 1]);
                step = st > step ? st : step;
            }
        }
    }
    shift = tcp_block_max(shift, s_val);
    step = tcp_block_max(step, s_val);
    if (tid == 0) {
        max_shift[q] = shift;
        max_step[q] = step;
    }
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
struct TcpShape { long P, pair_frames, dancer_frames, dancers; int quads; };

static int tcp_shape(int b, int dn, int T, TcpShape* s) {
    if (b < 1 || dn < 2 || T < 1) return TC_ERR_ARG;
    if (dn > TC_APART_MAX_DANCERS) return TC_ERR_UNSUPPORTED;
    s->P = (long)dn * (dn - 1) / 2;
    s->dancers = (long)b * dn;
    if ((long)b * s->P > 0x7fffffffl / T || s->dancers * TCP_ROWS > 0x7fffffffl / T) return TC_ERR_UNSUPPORTED;
    s->pair_frames = (long)b * s->P * T;
    s->dancer_frames = s->dancers * T;
    s->quads = (T + 3) / 4;
    if ((long)b * s->P * s->quads > 0x7fffffffl) return TC_ERR_UNSUPPORTED;
    return TC_OK;
}

static long tcp_bytes(const TcpShape& s) {
    const long n = s.pair_frames * TC_APART_WS_PAIR_FRAME + s.dancer_frames * TC_APART_WS_DANCER_FRAME;
    return (n + 7) / 8 * 8;
}

extern "C" int tcp_keep_apart_workspace(int b, int dn, int T, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    TcpShape s;
    const int rc = tcp_shape(b, dn, T, &s);
    if (rc != TC_OK) return rc;
    *bytes = tcp_bytes(s);
    return TC_OK;
}

extern "C" int tcp_keep_apart(const float* pos, const float* joints, const long* joint_strides, int b, int dn, int T, int up,
                              const int* parents, const double* radii, const double* mobility, double margin, int iterations, int rounds,
                              int blend, double max_push, void* workspace, long workspace_bytes, float* pos_out, float* joints_out,
                              double* shift, long* contact_before, long* contact_after, double* gap_min_before, double* gap_min_after,
                              long* pushed, long* capped, double* max_shift, double* max_step, hipStream_t stream) {
    if (!pos || !joints || !joint_strides || !parents || !radii || !mobility || !workspace || !pos_out || !joints_out || !contact_before ||
        !contact_after || !gap_min_before || !gap_min_after || !pushed || !capped || !max_shift || !max_step)
        return TC_ERR_ARG;
    if (b < 1 || dn < 2 || T < 1 || up < 0 || up > 2 || iterations < 0 || rounds < 0 || blend < 0) return TC_ERR_ARG;
    if (!(margin >= 0.0) || !tcg_finite(margin) || !(max_push >= 0.0) || !tcg_finite(max_push)) return TC_ERR_ARG;
    if (dn > TC_APART_MAX_DANCERS || blend > TC_APART_MAX_BLEND || rounds > TC_APART_MAX_ROUNDS) return TC_ERR_UNSUPPORTED;
    TcpShape s;
    const int rc = tcp_shape(b, dn, T, &s);
    if (rc != TC_OK) return rc;
    for (int k = 0; k < 3; ++k)
        if (joint_strides[k] < 0) return TC_ERR_ARG;
    TcpSkel sk;
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
    TcpMob mob;
    for (int d = 0; d < TC_APART_MAX_DANCERS; ++d) {
        if (d < dn && (!(mobility[d] >= 0.0) || !tcg_finite(mobility[d]))) return TC_ERR_ARG;
        mob.v[d] = d < dn ? mobility[d] : 0.0;
    }
    if (workspace_bytes < tcp_bytes(s)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)shift % 8) return TC_ERR_ALIGN;
    // the workspace: m [b P][T], u [b P][T][2], the before and the after gap [b P][T], S [b dn][T][2] (doubles), then the flag bytes [b P][T]
    double* w_m = (double*)workspace;
    double* w_u = w_m + s.pair_frames;
    double* w_before = w_u + 2 * s.pair_frames;
    double* w_after = w_before + s.pair_frames;
    double* w_S = w_after + s.pair_frames;
    unsigned char* w_flags = (unsigned char*)(w_S + 2 * s.dancer_frames);
    double* S = shift ? shift : w_S;
    const long s0 = joint_strides[0], s1 = joint_strides[1], s2 = joint_strides[2];
    const int P = (int)s.P;
    const dim3 frames_grid((unsigned)((long)b * P * s.quads)), threads(TCP_THREADS);
    const dim3 dancer_grid((unsigned)((s.dancer_frames + TCP_THREADS - 1) / TCP_THREADS));
    for (int r = 0; r < rounds; ++r) {
        hipLaunchKernelGGL(apart_demand_kernel, frames_grid, threads, 0, stream, joints, s0, s1, s2, r ? (const double*)S : (const double*)nullptr,
                           dn, T, P, s.quads, up, sk, mob, margin, iterations, max_push, w_m, w_u, r ? (double*)nullptr : w_before, w_flags,
                           r == 0);
        TC_CHECK_LAUNCH();
        hipLaunchKernelGGL(apart_combine_kernel, dancer_grid, threads, 0, stream, (const double*)w_m, (const double*)w_u, S, dn, T, P, blend, mob,
                           r == 0, s.dancer_frames);
        TC_CHECK_LAUNCH();
    }
    const long rows = s.dancer_frames * TCP_ROWS;
    hipLaunchKernelGGL(apart_apply_kernel, dim3((unsigned)((rows + TCP_THREADS - 1) / TCP_THREADS)), threads, 0, stream, pos, joints, s0, s1, s2,
                       rounds ? (const double*)S : (const double*)nullptr, rounds ? (double*)nullptr : shift, dn, T, up, pos_out, joints_out, rows);
    TC_CHECK_LAUNCH();
    const long o2 = (long)TCG_J * 3, o1 = o2 * T, o0 = o1 * dn;          // joints_out is contiguous
    hipLaunchKernelGGL(apart_demand_kernel, frames_grid, threads, 0, stream, (const float*)joints_out, o0, o1, o2, (const double*)nullptr, dn, T, P,
                       s.quads, up, sk, mob, margin, 0, max_push, (double*)nullptr, (double*)nullptr, w_after, (unsigned char*)nullptr, 1);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(apart_stats_kernel, dim3((unsigned)((long)b * P + s.dancers)), threads, 0, stream,
                       (const double*)(rounds ? w_before : w_after), (const double*)w_after,
                       rounds ? (const unsigned char*)w_flags : (const unsigned char*)nullptr, rounds ? (const double*)S : (const double*)nullptr, T,
                       (long)b * P, contact_before, contact_after, gap_min_before, gap_min_after, pushed, capped, max_shift, max_step);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
