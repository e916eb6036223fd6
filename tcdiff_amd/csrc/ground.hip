// Putting the dancers on the floor (include/tcdiff_ground.h), gfx950: a floor measure and contact-driven vertical root shifts.
// Five launches for any number of clips (four with the floor given; three and two for the metrics alone):
//   frames: one thread per (clip, dancer, frame) -- good, the body low L, the two foot lows and the labels
//   median: one workgroup per clip -- the exact median of the planted foot lows (or of L) by a digit-at-a-time selection of the
//           order-preserving 64-bit keys; the digit counts are per-thread registers reduced by wave shuffles, no atomics
//   walk:   one wave per (clip, dancer) -- the runs, their means summed in ascending t through shuffles, the nearest planted frames
//           by ballots, B, e, U and D
//   apply:  one thread per (clip, dancer, frame) -- the copy rule, then L and the foot lows of the float32 output
//   stats:  one wave per (clip, dancer) and evaluation -- counts and maxima over the lanes, the sums in ascending t through shuffles
// No atomics; every sum in one order, every minimum and maximum exact: the same input gives the same bits.  A few thousand frames per
// call, off the sampler's hot path: no MFMA.
// One departure from the header's wording, not from its numbers: L is computed as min over joints j of (z[j] - R[j]), R[j] the
// largest radius of the bones that end at j (the host forms R).  Rounding is monotone, so fl(z - r) over the bones of a joint is
// smallest for the largest r, and this minimum equals the header's minimum over bones to the bit; it keeps the joint table in
// registers with constant indices (no parent lookup into a register array, no scratch).
#include "common.h"
#include "tcdiff_ground.h"

#define TCF_THREADS 256
#define TCF_WAVE 64
#define TCF_J 24
#define TCF_PLANES 9
#define TCF_DIGITS (1 << TC_GROUND_DIGIT_BITS)
static_assert(TC_GROUND_WS_PER_FRAME == 8 * TCF_PLANES + 1, "the header states the workspace: nine float64 planes and a flag byte");
static_assert(TC_GROUND_MEDIAN_KEYS * 8 <= 64 * 1024 && 64 % TC_GROUND_DIGIT_BITS == 0, "the keys staged in LDS; whole digits");
static_assert((TC_GROUND_LEFT | TC_GROUND_RIGHT) == 3 && TC_GROUND_GOOD == 4 && TC_GROUND_CAPPED == 8, "the flag bits");

struct TcfSkel { double reach[TCF_J]; double r_left, r_right; };          // R[j] of the comment above; radii[10], radii[11]

DEVINL int tcf_finite32(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
DEVINL int tcf_finite(double x) { return x - x == 0.0; }
DEVINL double tcf_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
DEVINL double tcf_min(double a, double b) { return b < a ? b : a; }
DEVINL double tcf_pos(double x) { return x > 0.0 ? x : 0.0; }          // max(x, 0): +0 unless x > 0
// w(k) = 1 - k / (blend + 1)
DEVINL double tcf_w(int k, int blend) {
#pragma clang fp contract(off)
    return 1.0 - (double)k / ((double)blend + 1.0);
}
// the lows of one frame from its 24 `up` components
DEVINL void tcf_lows(const double* z, const TcfSkel& sk, double* L, double* lo_l, double* lo_r) {
#pragma clang fp contract(off)
    double m = z[0] - sk.reach[0];
#pragma unroll
    for (int j = 1; j < TCF_J; ++j) m = tcf_min(m, z[j] - sk.reach[j]);
    *L = m;
    *lo_l = tcf_min(z[7], z[10]) - sk.r_left;
    *lo_r = tcf_min(z[8], z[11]) - sk.r_right;
}
// is joint j still between frames t and t + 1 (both given)?
DEVINL int tcf_still(const float* a, const float* b, int j, double still) {
#pragma clang fp contract(off)
    const double dx = (double)b[3 * j] - (double)a[3 * j], dy = (double)b[3 * j + 1] - (double)a[3 * j + 1];
    const double dz = (double)b[3 * j + 2] - (double)a[3 * j + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz) < still;
}

// ---- frames ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCF_THREADS) void ground_frames_kernel(const float* __restrict__ joints, long s0, long s1, long s2,
                                                                    const float* __restrict__ contacts, long k0, long k1, long k2, long k3,
                                                                    int dn, int T, int up, TcfSkel sk, float thr, double still,
                                                                    double* __restrict__ L, double* __restrict__ lo_l,
                                                                    double* __restrict__ lo_r, unsigned char* __restrict__ flags, long total) {
    const long f = (long)blockIdx.x * TCF_THREADS + threadIdx.x;          // (clip dn + dancer) T + frame
    if (f >= total) return;
    const long q = f / T;
    const int t = (int)(f - q * T);
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    const float* J = joints + c * s0 + (long)d * s1 + (long)t * s2;
    int good = 1;
    double z[TCF_J];
#pragma unroll
    for (int j = 0; j < TCF_J; ++j) {
        const float x = J[3 * j], y = J[3 * j + 1], w = J[3 * j + 2];
        good &= tcf_finite32(x) & tcf_finite32(y) & tcf_finite32(w);
        z[j] = (double)(up == 0 ? x : (up == 1 ? y : w));
    }
    double Lv, ll, lr;
    tcf_lows(z, sk, &Lv, &ll, &lr);
    int left = 0, right = 0;
    if (good) {
        if (contacts) {
            const float* k = contacts + c * k0 + (long)d * k1 + (long)t * k2;
            left = k[0] > thr || k[2 * k3] > thr;
            right = k[k3] > thr || k[3 * k3] > thr;
        } else if (t == T - 1) {
            left = right = 1;
        } else {
            const float* N = J + s2;
            left = tcf_still(J, N, 7, still) || tcf_still(J, N, 10, still);
            right = tcf_still(J, N, 8, still) || tcf_still(J, N, 11, still);
        }
    }
    L[f] = Lv;
    lo_l[f] = ll;
    lo_r[f] = lr;
    flags[f] = (unsigned char)((left ? TC_GROUND_LEFT : 0) | (right ? TC_GROUND_RIGHT : 0) | (good ? TC_GROUND_GOOD : 0));
}

// ---- median ---------------------------------------------------------------------------------------------------------------------------------
typedef unsigned long long u64;
DEVINL u64 tcf_key(double v) {                                 // order-preserving: a < b (numbers) <=> key(a) < key(b), -0 before +0
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
DEVINL double tcf_value(u64 k) { return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k)); }
#define TCF_NONE (~0ull)                                        // no candidate: above the key of every number
DEVINL double tcf_mid(double lo, double hi) {                  // numpy's median of an even count: the mean of the two middle values
#pragma clang fp contract(off)
    return (lo + hi) / 2.0;
}

DEVINL long tcf_wave_sum(long x) {
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
// the block's total of x, the same in every thread; red: TCF_THREADS / 64 longs
DEVINL long tcf_block_sum(long x, long* red) {
    const int wave = threadIdx.x >> 6;
    x = tcf_wave_sum(x);
    __syncthreads();                                          // the previous total has been read
    if ((threadIdx.x & 63) == 0) red[wave] = x;
    __syncthreads();
    long s = 0;
#pragma unroll
    for (int w = 0; w < TCF_THREADS / 64; ++w) s += red[w];
    return s;
}

struct TcfCand {
    const double* L;
    const double* lo_l;
    const double* lo_r;
    const unsigned char* flags;
    long base;
    int feet;
    DEVINL u64 key(long e) const {
        if (feet) {
            const long at = base + (e >> 1);
            const int right = (int)(e & 1);
            if (!(flags[at] & (right ? TC_GROUND_RIGHT : TC_GROUND_LEFT))) return TCF_NONE;
            return tcf_key(right ? lo_r[at] : lo_l[at]);
        }
        if (!(flags[base + e] & TC_GROUND_GOOD)) return TCF_NONE;
        return tcf_key(L[base + e]);
    }
};

__global__ __launch_bounds__(TCF_THREADS) void ground_median_kernel(const double* __restrict__ L, const double* __restrict__ lo_l,
                                                                    const double* __restrict__ lo_r, const unsigned char* __restrict__ flags,
                                                                    int dn, int T, double* __restrict__ floor) {
    __shared__ u64 s_key[TC_GROUND_MEDIAN_KEYS];
    __shared__ long s_red[TCF_THREADS / 64];
    __shared__ int s_cnt[TCF_THREADS / 64][TCF_DIGITS];
    __shared__ u64 s_min[TCF_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long c = blockIdx.x, frames = (long)dn * T;
    TcfCand cand;
    cand.L = L;
    cand.lo_l = lo_l;
    cand.lo_r = lo_r;
    cand.flags = flags;
    cand.base = c * frames;
    long n = 0;
    for (long e = tid; e < frames; e += TCF_THREADS) {
        const unsigned char g = flags[cand.base + e];
        n += ((g & TC_GROUND_LEFT) != 0) + ((g & TC_GROUND_RIGHT) != 0);
    }
    n = tcf_block_sum(n, s_red);
    cand.feet = n > 0;
    if (!cand.feet) {
        for (long e = tid; e < frames; e += TCF_THREADS) n += (flags[cand.base + e] & TC_GROUND_GOOD) != 0;
        n = tcf_block_sum(n, s_red);
    }
    if (n == 0) {                                              // the block agrees: n is its total
        if (tid == 0) floor[c] = tcf_nan();
        return;
    }
    const long ne = cand.feet ? 2 * frames : frames;
    const long staged = ne < TC_GROUND_MEDIAN_KEYS ? ne : TC_GROUND_MEDIAN_KEYS;
    for (long e = tid; e < staged; e += TCF_THREADS) s_key[e] = cand.key(e);
    __syncthreads();
    // the key of rank k (from 0) among all ne keys; the n candidates hold ranks 0 .. n - 1, the TCF_NONE keys the rest
    long k = (n - 1) / 2;
    u64 prefix = 0;
    for (int shift = 64 - TC_GROUND_DIGIT_BITS; shift >= 0; shift -= TC_GROUND_DIGIT_BITS) {
        const u64 high = shift + TC_GROUND_DIGIT_BITS >= 64 ? 0ull : ~0ull << (shift + TC_GROUND_DIGIT_BITS);
        int cnt[TCF_DIGITS];
#pragma unroll
        for (int x = 0; x < TCF_DIGITS; ++x) cnt[x] = 0;
        for (long e = tid; e < ne; e += TCF_THREADS) {
            const u64 key = e < staged ? s_key[e] : cand.key(e);
            if ((key & high) == prefix) {
                const int dig = (int)((key >> shift) & (TCF_DIGITS - 1));
#pragma unroll
                for (int x = 0; x < TCF_DIGITS; ++x) cnt[x] += dig == x;
            }
        }
#pragma unroll
        for (int x = 0; x < TCF_DIGITS; ++x)
            for (int o = 32; o >= 1; o >>= 1) cnt[x] += __shfl_xor(cnt[x], o);
        __syncthreads();                                      // the previous pass's counts have been read
        if (lane == 0) {
#pragma unroll
            for (int x = 0; x < TCF_DIGITS; ++x) s_cnt[wave][x] = cnt[x];
        }
        __syncthreads();
        int dig = TCF_DIGITS - 1;
        long below = 0;
        for (int x = 0; x < TCF_DIGITS; ++x) {
            long tot = 0;
#pragma unroll
            for (int w = 0; w < TCF_THREADS / 64; ++w) tot += s_cnt[w][x];
            if (k < below + tot) {
                dig = x;
                break;
            }
            below += tot;
        }
        k -= below;
        prefix |= (u64)dig << shift;
    }
    const u64 lo = prefix;
    double F = tcf_value(lo);
    if ((n & 1) == 0) {                                        // the next rank: lo again if it occurs more than once up to it, else the
        long le = 0;                                           // least key above lo
        u64 above = TCF_NONE;
        for (long e = tid; e < ne; e += TCF_THREADS) {
            const u64 key = e < staged ? s_key[e] : cand.key(e);
            le += key <= lo;
            if (key > lo && key < above) above = key;
        }
        le = tcf_block_sum(le, s_red);
        for (int o = 32; o >= 1; o >>= 1) {
            const u64 other = __shfl_xor(above, o);
            above = other < above ? other : above;
        }
        if (lane == 0) s_min[wave] = above;
        __syncthreads();
        u64 hi = s_min[0];
#pragma unroll
        for (int w = 1; w < TCF_THREADS / 64; ++w) hi = s_min[w] < hi ? s_min[w] : hi;
        if (le >= n / 2 + 1) hi = lo;                          // ranks (n - 1) / 2 and n / 2 both hold lo
        F = tcf_mid(F, tcf_value(hi));
    }
    if (tid == 0) floor[c] = F;
}

// ---- walk -----------------------------------------------------------------------------------------------------------------------------------
DEVINL double tcf_foot(unsigned char g, double ll, double lr) {         // Lf of a planted frame
    const double a = (g & TC_GROUND_LEFT) ? ll : lr;
    return (g & TC_GROUND_LEFT) && (g & TC_GROUND_RIGHT) ? tcf_min(ll, lr) : a;
}

__global__ __launch_bounds__(TCF_WAVE) void ground_walk_kernel(const double* __restrict__ L, const double* __restrict__ lo_l,
                                                               const double* __restrict__ lo_r, unsigned char* __restrict__ flags,
                                                               const double* __restrict__ floor, int dn, int T, int blend, double max_lift,
                                                               double* __restrict__ B, double* __restrict__ E, double* __restrict__ D) {
#pragma clang fp contract(off)
    const long q = blockIdx.x, base = q * T;                  // clip dn + dancer
    const int lane = threadIdx.x;
    const double F = floor[q / dn];
    if (!tcf_finite(F)) {
        for (int t = lane; t < T; t += TCF_WAVE) D[base + t] = 0.0;
        return;
    }
    // the runs: a chunk's a(t) loaded by its lanes, then summed in ascending t by the whole wave through shuffles (every lane holds the
    // same sum: no memory latency in the chain); at a run's end the wave writes its mean over it
    double sum = 0.0;
    int n = 0;
    for (int t0 = 0; t0 < T; t0 += TCF_WAVE) {
        const int t = t0 + lane;
        const unsigned char g = t < T ? flags[base + t] : 0;
        const double a = (g & 3) ? F - tcf_foot(g, lo_l[base + t], lo_r[base + t]) : 0.0;
        const int m = T - t0 < TCF_WAVE ? T - t0 : TCF_WAVE;
        for (int k = 0; k < m; ++k) {
            const int pk = __shfl((int)(g & 3), k);
            const double ak = __shfl(a, k);
            if (pk) {
                sum = sum + ak;
                ++n;
            } else if (n) {                                   // the run ended at t0 + k - 1
                const double mean = sum / (double)n;
                for (int x = lane; x < n; x += TCF_WAVE) B[base + t0 + k - 1 - x] = mean;
                sum = 0.0;
                n = 0;
            }
        }
    }
    if (n) {
        const double mean = sum / (double)n;
        for (int x = lane; x < n; x += TCF_WAVE) B[base + T - 1 - x] = mean;
    }
    __syncthreads();
    // the first planted frame after each frame (backwards, kept in E for now), then the last before it and B of the unplanted frames
    int next = -1;
    for (int t0 = (T - 1) / TCF_WAVE * TCF_WAVE; t0 >= 0; t0 -= TCF_WAVE) {
        const int t = t0 + lane;
        const u64 m = __ballot(t < T && (flags[base + t] & 3));
        const u64 after = lane == 63 ? 0ull : m & (~0ull << (lane + 1));
        if (t < T) E[base + t] = (double)(after ? t0 + __builtin_ctzll(after) : next);
        if (m) next = t0 + __builtin_ctzll(m);
    }
    int last = -1;
    for (int t0 = 0; t0 < T; t0 += TCF_WAVE) {
        const int t = t0 + lane;
        const int p = t < T && (flags[base + t] & 3);
        const u64 m = __ballot(p);
        const u64 before = m & ((1ull << lane) - 1ull);
        const int i = before ? t0 + 63 - __builtin_clzll(before) : last;
        if (t < T && !p) {
            const int j = (int)E[base + t];
            double b = 0.0;
            if (i >= 0 && j >= 0 && j - i - 1 <= 2 * blend) {
                const double bi = B[base + i], bj = B[base + j];
                b = bi + (bj - bi) * ((double)(t - i) / (double)(j - i));
            } else if (i >= 0 && t - i <= blend) {
                b = B[base + i] * tcf_w(t - i, blend);
            } else if (j >= 0 && j - t <= blend) {
                b = B[base + j] * tcf_w(j - t, blend);
            }
            B[base + t] = b;
        }
        if (m) last = t0 + 63 - __builtin_clzll(m);
    }
    __syncthreads();
    for (int t = lane; t < T; t += TCF_WAVE)
        E[base + t] = (flags[base + t] & TC_GROUND_GOOD) ? tcf_pos((F - L[base + t]) - B[base + t]) : 0.0;
    __syncthreads();
    for (int t = lane; t < T; t += TCF_WAVE) {
        const unsigned char g = flags[base + t];
        double Dv = 0.0;
        if (g & TC_GROUND_GOOD) {
            const int lo = t - blend < 0 ? 0 : t - blend, hi = t > T - 1 - blend ? T - 1 : t + blend;
            double U = 0.0;
            for (int s = lo; s <= hi; ++s) {
                const double cand = E[base + s] * tcf_w(s < t ? t - s : s - t, blend);
                U = cand > U ? cand : U;
            }
            Dv = B[base + t] + U;
            if (Dv > max_lift || Dv < -max_lift) {
                Dv = Dv > max_lift ? max_lift : -max_lift;
                flags[base + t] = (unsigned char)(g | TC_GROUND_CAPPED);
            }
        }
        D[base + t] = Dv;
    }
}

// ---- apply ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TCF_THREADS) void ground_apply_kernel(const float* __restrict__ pos, const float* __restrict__ joints, long s0, long s1,
                                                                   long s2, const double* __restrict__ D, int dn, int T, int up, TcfSkel sk,
                                                                   float* __restrict__ pos_out, float* __restrict__ joints_out,
                                                                   double* __restrict__ L, double* __restrict__ lo_l, double* __restrict__ lo_r,
                                                                   long total) {
#pragma clang fp contract(off)
    const long f = (long)blockIdx.x * TCF_THREADS + threadIdx.x;          // (clip dn + dancer) T + frame
    if (f >= total) return;
    const long q = f / T;
    const int t = (int)(f - q * T);
    const long c = q / dn;
    const int d = (int)(q - c * dn);
    const uint32_t* src = (const uint32_t*)(joints + c * s0 + (long)d * s1 + (long)t * s2);
    uint32_t* dst = (uint32_t*)(joints_out + f * (TCF_J * 3));
    const long row = ((c * T + t) * dn + d) * 3;
    const uint32_t* psrc = (const uint32_t*)(pos + row);
    uint32_t* pdst = (uint32_t*)(pos_out + row);
    const double Dv = D[f];
    const int move = Dv != 0.0;                                // the words, not the values, where D is 0: -0.0 and NaN payloads stay
    double z[TCF_J];
#pragma unroll
    for (int j = 0; j < TCF_J; ++j) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint32_t w = src[3 * j + k];
            if (k == up) {
                if (move) w = __float_as_uint((float)((double)__uint_as_float(w) + Dv));
                z[j] = (double)__uint_as_float(w);
            }
            dst[3 * j + k] = w;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t w = psrc[k];
        pdst[k] = k == up && move ? __float_as_uint((float)((double)__uint_as_float(w) + Dv)) : w;
    }
    double Lv, ll, lr;
    tcf_lows(z, sk, &Lv, &ll, &lr);
    L[f] = Lv;
    lo_l[f] = ll;
    lo_r[f] = lr;
}

// ---- stats ----------------------------------------------------------------------------------------------------------------------------------
DEVINL double tcf_wave_max(double x) {                         // of numbers >= 0
    for (int o = 32; o >= 1; o >>= 1) {
        const double y = __shfl_xor(x, o);
        x = y > x ? y : x;
    }
    return x;
}

// blocks [0, dancers): "before" of (clip dn + dancer), from the planes L0 ..; blocks [dancers, 2 dancers): "after", from L1 ..
// counts / values: [3][dancers].  D NULL: no capped, max_shift, max_step.  floor_in: copied to floor by (clip, dancer 0, before).
__global__ __launch_bounds__(TCF_WAVE) void ground_stats_kernel(const double* __restrict__ L0, const double* __restrict__ ll0,
                                                                const double* __restrict__ lr0, const double* __restrict__ L1,
                                                                const double* __restrict__ ll1, const double* __restrict__ lr1,
                                                                const unsigned char* __restrict__ flags, const double* __restrict__ F_of,
                                                                const double* __restrict__ floor_in, double* __restrict__ floor, int dn, int T,
                                                                long dancers, double tolerance, long* __restrict__ counts0,
                                                                double* __restrict__ values0, long* __restrict__ counts1,
                                                                double* __restrict__ values1, const double* __restrict__ D,
                                                                long* __restrict__ capped, double* __restrict__ max_shift,
                                                                double* __restrict__ max_step) {
#pragma clang fp contract(off)
    const int after = (long)blockIdx.x >= dancers;
    const long q = (long)blockIdx.x - (after ? dancers : 0), base = q * T, c = q / dn;
    const int lane = threadIdx.x;
    const double* L = after ? L1 : L0;
    const double* ll = after ? ll1 : ll0;
    const double* lr = after ? lr1 : lr0;
    long* counts = after ? counts1 : counts0;
    double* values = after ? values1 : values0;
    const double F = F_of[c];
    const int finite = tcf_finite(F);
    const double low = F - tolerance, high = F + tolerance;
    long planted = 0, good = 0, pen = 0, flo = 0, ncap = 0;
    double pmax = 0.0, shift = 0.0, step = 0.0;
    for (int t = lane; t < T; t += TCF_WAVE) {
        const unsigned char g = flags[base + t];
        if (g & TC_GROUND_GOOD) {
            const double Lv = L[base + t];
            ++good;
            pen += Lv < low;
            const double x = tcf_pos(F - Lv);
            pmax = x > pmax ? x : pmax;
        }
        if (g & 3) {
            ++planted;
            flo += tcf_foot(g, ll[base + t], lr[base + t]) > high;
        }
        if (D && !after) {
            ncap += (g & TC_GROUND_CAPPED) != 0;
            const double a = fabs(D[base + t]);
            shift = a > shift ? a : shift;
            if (t > 0) {
                const double st = fabs(D[base + t] - D[base + t - 1]);
                step = st > step ? st : step;
            }
        }
    }
    planted = tcf_wave_sum(planted);
    good = tcf_wave_sum(good);
    pen = tcf_wave_sum(pen);
    flo = tcf_wave_sum(flo);
    ncap = tcf_wave_sum(ncap);
    pmax = tcf_wave_max(pmax);
    shift = tcf_wave_max(shift);
    step = tcf_wave_max(step);
    // the sums in ascending t: a chunk's terms loaded by its lanes, added by the whole wave through shuffles; a frame that does not
    // take part adds +0, which leaves a sum of terms >= 0 as it is
    double sp = 0.0, sf = 0.0;
    for (int t0 = 0; t0 < T; t0 += TCF_WAVE) {
        const int t = t0 + lane;
        const unsigned char g = t < T ? flags[base + t] : 0;
        const double x = (g & TC_GROUND_GOOD) ? tcf_pos(F - L[base + t]) : 0.0;
        const double y = (g & 3) ? tcf_pos(tcf_foot(g, ll[base + t], lr[base + t]) - F) : 0.0;
        const int m = T - t0 < TCF_WAVE ? T - t0 : TCF_WAVE;
        for (int k = 0; k < m; ++k) {
            sp = sp + __shfl(x, k);
            sf = sf + __shfl(y, k);
        }
    }
    if (lane != 0) return;
    counts[q] = planted;
    counts[dancers + q] = pen;
    counts[2 * dancers + q] = flo;
    values[q] = finite ? pmax : tcf_nan();
    values[dancers + q] = finite ? sp / (double)good : tcf_nan();
    values[2 * dancers + q] = finite ? sf / (double)planted : tcf_nan();
    if (D && !after) {
        capped[q] = ncap;
        max_shift[q] = shift;
        max_step[q] = step;
    }
    if (floor_in && !after && q - c * dn == 0) floor[c] = floor_in[c];
}

// ---- the entry points ---------------------------------------------------------------------------------------------------------------------
static int tcf_shape(int b, int dn, int T, long* frames) {
    if (b < 1 || dn < 1 || T < 1) return TC_ERR_ARG;
    if (dn > TC_GROUND_MAX_DANCERS) return TC_ERR_UNSUPPORTED;
    if ((long)b * dn > 0x7fffffffl / T) return TC_ERR_UNSUPPORTED;
    *frames = (long)b * dn * T;
    return TC_OK;
}

static long tcf_bytes(long frames) { return (frames * TC_GROUND_WS_PER_FRAME + 7) / 8 * 8; }

extern "C" int tcf_ground_workspace(int b, int dn, int T, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    long frames;
    const int rc = tcf_shape(b, dn, T, &frames);
    if (rc != TC_OK) return rc;
    *bytes = tcf_bytes(frames);
    return TC_OK;
}


static int tcf_finite_host(double x) { return x - x == 0.0; }

// the checks of the tables, in the header's order after the shape's: strides, parents, radii; and the skeleton the kernels read
static int tcf_tables(const long* joint_strides, const float* contacts, const long* contact_strides, const int* parents,
                      const double* radii, TcfSkel* sk) {
    for (int k = 0; k < 3; ++k)
        if (joint_strides[k] < 0) return TC_ERR_ARG;
    if (contacts)
        for (int k = 0; k < 4; ++k)
            if (contact_strides[k] < 0) return TC_ERR_ARG;
    for (int j = 1; j < TCF_J; ++j)
        if (parents[j] < 0 || parents[j] >= j) return TC_ERR_ARG;          // a parent must precede its child
    for (int j = 1; j < TCF_J; ++j)
        if (!(radii[j] >= 0.0) || !tcf_finite_host(radii[j])) return TC_ERR_ARG;
    for (int j = 0; j < TCF_J; ++j) sk->reach[j] = -1.0;
    for (int i = 1; i < TCF_J; ++i) {                          // bone i ends at i and at its parent
        sk->reach[i] = radii[i] > sk->reach[i] ? radii[i] : sk->reach[i];
        sk->reach[parents[i]] = radii[i] > sk->reach[parents[i]] ? radii[i] : sk->reach[parents[i]];
    }
    sk->r_left = radii[10];
    sk->r_right = radii[11];
    return TC_OK;
}

struct TcfWs { double *L0, *ll0, *lr0, *L1, *ll1, *lr1, *B, *E, *D; unsigned char* flags; };
static TcfWs tcf_ws(void* workspace, long frames) {
    TcfWs w;
    double* p = (double*)workspace;
    double** planes[TCF_PLANES] = {&w.L0, &w.ll0, &w.lr0, &w.L1, &w.ll1, &w.lr1, &w.B, &w.E, &w.D};
    for (int k = 0; k < TCF_PLANES; ++k) *planes[k] = p + k * frames;
    w.flags = (unsigned char*)(p + TCF_PLANES * frames);
    return w;
}

static void tcf_frames_launch(const float* joints, const long* js, const float* contacts, const long* cs, int dn, int T, int up,
                              const TcfSkel& sk, float thr, double still, const TcfWs& w, long frames, hipStream_t stream) {
    hipLaunchKernelGGL(ground_frames_kernel, dim3((unsigned)((frames + TCF_THREADS - 1) / TCF_THREADS)), dim3(TCF_THREADS), 0, stream, joints,
                       js[0], js[1], js[2], contacts, contacts ? cs[0] : 0l, contacts ? cs[1] : 0l, contacts ? cs[2] : 0l,
                       contacts ? cs[3] : 0l, dn, T, up, sk, thr, still, w.L0, w.ll0, w.lr0, w.flags, frames);
}

extern "C" int tcf_ground_metrics(const float* joints, const long* joint_strides, const float* contacts, const long* contact_strides, int b,
                                  int dn, int T, int up, const int* parents, const double* radii, const double* floor_in,
                                  float contact_threshold, double still, double tolerance, void* workspace, long workspace_bytes,
                                  double* floor, long* counts, double* values, hipStream_t stream) {
    if (!joints || !joint_strides || (contacts && !contact_strides) || !parents || !radii || !workspace || !floor || !counts || !values)
        return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || up < 0 || up > 2) return TC_ERR_ARG;
    if (contact_threshold != contact_threshold || !(still >= 0.0) || !tcf_finite_host(still) || !(tolerance >= 0.0) ||
        !tcf_finite_host(tolerance))
        return TC_ERR_ARG;
    long frames;
    int rc = tcf_shape(b, dn, T, &frames);
    if (rc != TC_OK) return rc;
    TcfSkel sk;
    rc = tcf_tables(joint_strides, contacts, contact_strides, parents, radii, &sk);
    if (rc != TC_OK) return rc;
    if (workspace_bytes < tcf_bytes(frames)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)floor_in % 8) return TC_ERR_ALIGN;
    const TcfWs w = tcf_ws(workspace, frames);
    tcf_frames_launch(joints, joint_strides, contacts, contact_strides, dn, T, up, sk, contact_threshold, still, w, frames, stream);
    TC_CHECK_LAUNCH();
    if (!floor_in) {
        hipLaunchKernelGGL(ground_median_kernel, dim3((unsigned)b), dim3(TCF_THREADS), 0, stream, (const double*)w.L0, (const double*)w.ll0,
                           (const double*)w.lr0, (const unsigned char*)w.flags, dn, T, floor);
        TC_CHECK_LAUNCH();
    }
    const long dancers = (long)b * dn;
    hipLaunchKernelGGL(ground_stats_kernel, dim3((unsigned)dancers), dim3(TCF_WAVE), 0, stream, (const double*)w.L0, (const double*)w.ll0,
                       (const double*)w.lr0, (const double*)nullptr, (const double*)nullptr, (const double*)nullptr,
                       (const unsigned char*)w.flags, floor_in ? floor_in : (const double*)floor, floor_in, floor, dn, T, dancers, tolerance,
                       counts, values, (long*)nullptr, (double*)nullptr, (const double*)nullptr, (long*)nullptr, (double*)nullptr,
                       (double*)nullptr);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcf_ground(const float* pos, const float* joints, const long* joint_strides, const float* contacts, const long* contact_strides,
                          int b, int dn, int T, int up, const int* parents, const double* radii, const double* floor_in, float contact_threshold,
                          double still, double tolerance, int blend, double max_lift, void* workspace, long workspace_bytes, float* pos_out,
                          float* joints_out, double* shift, double* floor, long* counts_before, double* values_before, long* counts_after,
                          double* values_after, long* capped, double* max_shift, double* max_step, hipStream_t stream) {
    if (!pos || !joints || !joint_strides || (contacts && !contact_strides) || !parents || !radii || !workspace || !pos_out || !joints_out ||
        !floor || !counts_before || !values_before || !counts_after || !values_after || !capped || !max_shift || !max_step)
        return TC_ERR_ARG;
    if (b < 1 || dn < 1 || T < 1 || up < 0 || up > 2 || blend < 0) return TC_ERR_ARG;
    if (contact_threshold != contact_threshold || !(still >= 0.0) || !tcf_finite_host(still) || !(tolerance >= 0.0) ||
        !tcf_finite_host(tolerance) || !(max_lift >= 0.0) || !tcf_finite_host(max_lift))
        return TC_ERR_ARG;
    if (dn > TC_GROUND_MAX_DANCERS || blend > TC_GROUND_MAX_BLEND) return TC_ERR_UNSUPPORTED;
    long frames;
    int rc = tcf_shape(b, dn, T, &frames);
    if (rc != TC_OK) return rc;
    TcfSkel sk;
    rc = tcf_tables(joint_strides, contacts, contact_strides, parents, radii, &sk);
    if (rc != TC_OK) return rc;
    if (workspace_bytes < tcf_bytes(frames)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 || (uintptr_t)floor_in % 8 || (uintptr_t)shift % 8) return TC_ERR_ALIGN;
    const TcfWs w = tcf_ws(workspace, frames);
    double* D = shift ? shift : w.D;
    const double* F = floor_in ? floor_in : (const double*)floor;
    tcf_frames_launch(joints, joint_strides, contacts, contact_strides, dn, T, up, sk, contact_threshold, still, w, frames, stream);
    TC_CHECK_LAUNCH();
    if (!floor_in) {
        hipLaunchKernelGGL(ground_median_kernel, dim3((unsigned)b), dim3(TCF_THREADS), 0, stream, (const double*)w.L0, (const double*)w.ll0,
                           (const double*)w.lr0, (const unsigned char*)w.flags, dn, T, floor);
        TC_CHECK_LAUNCH();
    }
    const long dancers = (long)b * dn;
    hipLaunchKernelGGL(ground_walk_kernel, dim3((unsigned)dancers), dim3(TCF_WAVE), 0, stream, (const double*)w.L0, (const double*)w.ll0,
                       (const double*)w.lr0, w.flags, F, dn, T, blend, max_lift, w.B, w.E, D);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(ground_apply_kernel, dim3((unsigned)((frames + TCF_THREADS - 1) / TCF_THREADS)), dim3(TCF_THREADS), 0, stream, pos, joints,
                       joint_strides[0], joint_strides[1], joint_strides[2], (const double*)D, dn, T, up, sk, pos_out, joints_out, w.L1, w.ll1,
                       w.lr1, frames);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(ground_stats_kernel, dim3((unsigned)(2 * dancers)), dim3(TCF_WAVE), 0, stream, (const double*)w.L0, (const double*)w.ll0,
                       (const double*)w.lr0, (const double*)w.L1, (const double*)w.ll1, (const double*)w.lr1, (const unsigned char*)w.flags, F,
                       floor_in, floor, dn, T, dancers, tolerance, counts_before, values_before, counts_after, values_after, (const double*)D,
                       capped, max_shift, max_step);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
