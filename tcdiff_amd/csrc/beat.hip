// The beat track of the music front end, gfx950: from the onset envelope to column 53 of `cond` (onset_beat) -- the tempo
// estimate and the dynamic-programme beat tracker of librosa 0.9.2 (beat.beat_track, beat.tempo, beat.__beat_tracker) restated for
// one envelope per clip at 60 frames / s.  The definitions: include/tcdiff_hip.h.  Two launches for any number of clips, one when
// the period is given; no float atomics, every sum in a fixed order: a second run, and a clip computed alone, give the same bits.
//
//   beat_tempo_kernel   one workgroup per (clip, chunk of 8 frames), 240 threads: ramp padding and window on load, two lags of the
//                       480-lag autocorrelation per thread (music_acf.h, the tempogram's code), the frame's rows normalised and
//                       summed in float64 in ascending t -> one partial row per workgroup
//   beat_track_kernel   one workgroup per clip, eight waves: the partial rows in ascending chunk order, prior, first argmax ->
//                       period; standard deviation by a fixed tree; local score; the dynamic programme in blocks of h = rint(period / 2)
//                       frames, a wave per frame, the last 2 period cumulative scores in an LDS ring, one barrier per block; flags,
//                       the exact median by radix selection on the ordered bit patterns; backtrace on one lane; trim; one-hot row
//
// Three quirks of librosa 0.9.2 are kept on purpose (someone with librosa can check each):
//   (1) np.round rounds half to even: period = round(3600 / bpm) on the host, h = rint(period / 2) here (12.5 -> 12, 13.5 -> 14);
//   (2) the end of the trim slice is exclusive: beats[v0 : v1] drops the last beat above the threshold;
//   (3) the trim's smoothing window is the SYMMETRIC 5-point Hann, (0, 0.5, 1, 0.5, 0): its end taps are zero, three taps remain.
// The tables w and txwt are built on the host in float64 for every period 1 .. 479 (nothing transcendental runs in float64 here
// but the 480 log1p of the tempo score).
#include <float.h>
#include <limits.h>

#include "common.h"
#include "music_acf.h"
#include "tcdiff_hip.h"

#define BT_WIN TC_BEAT_WIN
#define BT_CHUNK TC_BEAT_CHUNK
#define BT_TABLE TC_BEAT_TABLE
#define BT_THREADS 512
#define BT_WAVES (BT_THREADS / TC_WAVE)
#define BT_RING 2048                                     // >= 2 * 479 + 240: a block's writes never alias the slots it reads
#define BT_TAPS (2 * (BT_WIN - 1) + 1)                   // 959: the longest row of either table

// ---- launch 1: the tempo estimate's autocorrelation ---------------------------------------------------------------------------
// grid (chunks, B), 240 threads.  partial [B][chunks][480] double: the sum over the chunk's frames, in ascending t, of the
// frame's normalised autocorrelation.
__global__ __launch_bounds__(BT_WIN / 2) void beat_tempo_kernel(const float* __restrict__ onset_env, long o_stride, int T, int chunks,
                                                                const float* __restrict__ win, double* __restrict__ partial) {
    __shared__ float s_x[BT_WIN];
    __shared__ float s_red[256];
    const int tid = threadIdx.x, chunk = blockIdx.x;
    const long b = blockIdx.y;
    const float* env = onset_env + b * o_stride;
    const int t0 = chunk * BT_CHUNK, t1 = t0 + BT_CHUNK < T ? t0 + BT_CHUNK : T;
    double ga = 0.0, gc = 0.0;
    for (int t = t0; t < t1; ++t) {
        for (int i = tid; i < BT_WIN; i += BT_WIN / 2) s_x[i] = mu_ramp_sample<BT_WIN>(env, T, t, i) * win[i];
        __syncthreads();
        float a, c;
        mu_acf_pair<BT_WIN>(s_x, tid, a, c);
        const float mx = mu_acf_absmax<BT_WIN>(s_red, a, c, tid);
        ga += (double)(mx < FLT_MIN ? a : a / mx);
        gc += (double)(mx < FLT_MIN ? c : c / mx);
        __syncthreads();                                  // s_x and s_red are rewritten by the next frame
    }
    double* o = partial + (b * chunks + chunk) * BT_WIN;
    o[tid] = ga;
    o[BT_WIN - 1 - tid] = gc;
}

// ---- launch 2: period, local score, dynamic programme, last beat, backtrace, trim -------------------------------------------------
// Fixed-order tree over the 512 threads' values; every thread returns the result.  s_red[512].
template <class Op>
DEVINL double bt_tree(double* s_red, double v, Op op) {
    const int tid = threadIdx.x;
    __syncthreads();                                      // the previous result has been read
    s_red[tid] = v;
    __syncthreads();
    for (int o = BT_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] = op(s_red[tid], s_red[tid + o]);
        __syncthreads();
    }
    return s_red[0];
}

// (value, index) maximum over the wave, ties to the lower index; every lane ends with the result
DEVINL void bt_wave_argmax(double& v, int& k) {
#pragma unroll
    for (int off = TC_WAVE / 2; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int ok = __shfl_xor(k, off);
        if (ov > v || (ov == v && ok < k)) {
            v = ov;
            k = ok;
        }
    }
}

// the bit pattern of a double as an unsigned integer of the same order (negative values reversed, then the sign bit flipped)
DEVINL unsigned long long bt_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
DEVINL double bt_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// m[i]: cum[i] > cum[i - 1] and cum[i] >= cum[i + 1], the ends repeating their edge value (so m[0] is false)
DEVINL bool bt_flag(const double* cum, int T, int i) {
    if (i < 1) return false;
    const double c = cum[i];
    return c > cum[i - 1] && c >= cum[i + 1 < T ? i + 1 : T - 1];
}

// The flagged value of rank `rank` (0 = smallest) by radix selection, eight bits a pass from the top: a histogram of the next
// byte over the values that share the bytes chosen so far (integer LDS atomics: the counts do not depend on the order).
DEVINL double bt_select(const double* cum, int T, int rank, int* s_hist, unsigned long long* s_prefix, int* s_rank) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid == 0) {
        *s_prefix = 0;
        *s_rank = rank;
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        const unsigned long long prefix = *s_prefix;
        for (int i = tid; i < T; i += BT_THREADS) {
            if (!bt_flag(cum, T, i)) continue;
            const unsigned long long key = bt_key(cum[i]);
            if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int r = *s_rank, d = 0;
            while (d < 255 && r >= s_hist[d]) r -= s_hist[d++];
            *s_prefix = prefix | ((unsigned long long)d << shift);
            *s_rank = r;
        }
        __syncthreads();
    }
    return bt_unkey(*s_prefix);
}

// grid (B), 512 threads.  tables [2][BT_TABLE] double: row `period` of w and of txwt starts at period^2 - 1.  partial NULL: the
// period is given in period[b] (and tempo[b] by the caller).  The envelope is finite and non-negative (include/tcdiff_hip.h).
__global__ __launch_bounds__(BT_THREADS) void beat_track_kernel(const float* __restrict__ onset_env, long o_stride, int T, int chunks,
                                                                const double* __restrict__ partial, const double* __restrict__ prior,
                                                                const double* __restrict__ tables, int trim, double* __restrict__ ls_out,
                                                                double* __restrict__ cum_out, int* __restrict__ back_out,
                                                                int* __restrict__ beats_ws, float* __restrict__ onset_beat,
                                                                int* __restrict__ period, int* __restrict__ n_beats,
                                                                double* __restrict__ tempo) {
    __shared__ double s_tab[BT_TAPS + 1];
    __shared__ double s_ring[BT_RING];
    __shared__ double s_red[BT_THREADS];
    __shared__ double s_wv[BT_WAVES];
    __shared__ int s_wk[BT_WAVES];
    __shared__ int s_hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_int[4];
    const int tid = threadIdx.x, lane = tid & (TC_WAVE - 1), wave = tid / TC_WAVE;
    const long b = blockIdx.x;
    const float* env = onset_env + b * o_stride;
    double* ls = ls_out + b * T;
    double* cum = cum_out + b * T;
    int* back = back_out + b * T;
    int* beats = beats_ws + b * T;
    float* row = onset_beat + b * T;
    const auto fmax_op = [](double x, double y) { return x > y ? x : y; };
    const auto fmin_op = [](double x, double y) { return x < y ? x : y; };
    const auto add_op = [](double x, double y) { return x + y; };

    for (int i = tid; i < T; i += BT_THREADS) row[i] = 0.0f;          // the kept beats are set at the very end

    // ---- 0. a silent clip (tempo 0, no beats); a constant one (zero variance: no beats rather than NaNs) -------------------------
    double hi = (double)env[0], lo = hi;
    for (int i = tid; i < T; i += BT_THREADS) {
        const double v = (double)env[i];
        hi = v > hi ? v : hi;
        lo = v < lo ? v : lo;
    }
    hi = bt_tree(s_red, hi, fmax_op);
    lo = bt_tree(s_red, lo, fmin_op);
    const bool silent = hi == 0.0 && lo == 0.0, flat = hi == lo;
    if (flat) {                                                       // (uniform over the workgroup, as every branch around a barrier below)
        for (int i = tid; i < T; i += BT_THREADS) {
            ls[i] = 0.0;
            cum[i] = 0.0;
            back[i] = -1;
        }
        if (tid == 0) n_beats[b] = 0;
    }
    if (silent) {
        if (tid == 0) {
            tempo[b] = 0.0;
            if (partial) period[b] = 0;
        }
        return;
    }

    // ---- 1. the tempo: partial rows in ascending chunk order, prior, first argmax ----------------------------------------------------
    int per;
    if (partial) {
        double v = -INFINITY;
        int k = INT_MAX;
        if (tid < BT_WIN) {
            const double* p = partial + b * chunks * BT_WIN + tid;
            double g = 0.0;
            for (int c = 0; c < chunks; ++c) g += p[(long)c * BT_WIN];
            g /= (double)T;
            v = log1p(1e6 * g) + prior[tid];
            k = tid;
        }
        bt_wave_argmax(v, k);
        if (lane == 0) {
            s_wv[wave] = v;
            s_wk[wave] = k;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < BT_WAVES; ++w)
                if (s_wv[w] > v || (s_wv[w] == v && s_wk[w] < k)) {
                    v = s_wv[w];
                    k = s_wk[w];
                }
            s_int[0] = (k >= 1 && k < BT_WIN) ? k : 0;
        }
        __syncthreads();
        per = s_int[0];
        if (tid == 0) {
            period[b] = per;
            tempo[b] = per ? 3600.0 / (double)per : 0.0;
        }
    } else {
        per = period[b];
    }
    if (flat || per < 1 || per >= BT_WIN) {                           // (the launcher has checked a given period)
        if (tid == 0) n_beats[b] = 0;
        return;
    }

    // ---- 2. x = o / std(o, ddof = 1), kept in cum until the programme overwrites it ---------------------------------------------------
    // (the cum_score output doubles as scratch: x is written here by one thread and read in phase 3 by others, across the
    // barrier below, which orders the workgroup's global stores and loads; phase 4 then overwrites every element with cum)
    double acc = 0.0;
    for (int i = tid; i < T; i += BT_THREADS) acc += (double)env[i];
    const double mean = bt_tree(s_red, acc, add_op) / (double)T;
    acc = 0.0;
    for (int i = tid; i < T; i += BT_THREADS) {
        const double d = (double)env[i] - mean;
        acc += d * d;
    }
    const double sd = sqrt(bt_tree(s_red, acc, add_op) / (double)(T - 1));
    for (int i = tid; i < T; i += BT_THREADS) cum[i] = (double)env[i] / sd;
    for (int j = tid; j < 2 * per + 1; j += BT_THREADS) s_tab[j] = tables[(long)per * per - 1 + j];
    __syncthreads();

    // ---- 3. the local score: ls[i] = sum_j w[j] x[i - j], j = -per .. per ascending, product and sum rounded separately ------------
    double lsmax = -INFINITY;
    for (int i = tid; i < T; i += BT_THREADS) {
#pragma clang fp contract(off)
        double s = 0.0;
        const int j0 = i - (T - 1) > -per ? i - (T - 1) : -per, j1 = i < per ? i : per;      // 0 <= i - j < T
        for (int j = j0; j <= j1; ++j) {
            const double p = s_tab[j + per] * cum[i - j];
            s = s + p;
        }
        ls[i] = s;
        lsmax = s > lsmax ? s : lsmax;
    }
    lsmax = bt_tree(s_red, lsmax, fmax_op);                           // (its barriers: every x has been read, every ls written)
    if (tid == 0) s_int[1] = T;
    __syncthreads();
    {
        const double thr = 0.01 * lsmax;
        int first = T;
        for (int i = tid; i < T && first == T; i += BT_THREADS)
            if (ls[i] >= thr) first = i;
        if (first < T) atomicMin(&s_int[1], first);
    }

    // ---- 4. the dynamic programme --------------------------------------------------------------------------------------------------
    const int h = (int)rint(0.5 * (double)per);                       // half to even
    const int hb = h > 1 ? h : 1;
    int n_cand = 2 * per - h + 1;                                     // offsets d_k = -2 per + k
    n_cand = n_cand > 2 * per ? 2 * per : n_cand;                     // (per = 1: d = 0 scores -inf and is never the first maximum)
    for (int k = tid; k < n_cand; k += BT_THREADS) s_tab[k] = tables[BT_TABLE + (long)per * per - 1 + k];
    __syncthreads();
    const int first = s_int[1];
    for (int i0 = 0; i0 < T; i0 += hb) {
        const int i1 = i0 + hb < T ? i0 + hb : T;
        for (int i = i0 + wave; i < i1; i += BT_WAVES) {
            const double lsi = ls[i];
            double v = -INFINITY;
            int kb = INT_MAX;
            for (int k = lane; k < n_cand; k += TC_WAVE) {
                const int idx = i - 2 * per + k;
                const double c = s_tab[k] + (idx >= 0 ? s_ring[idx & (BT_RING - 1)] : 0.0);
                if (kb == INT_MAX || c > v) {
                    v = c;
                    kb = k;
                }
            }
            bt_wave_argmax(v, kb);
            if (lane == 0) {
                const double cv = lsi + v;
                s_ring[i & (BT_RING - 1)] = cv;
                cum[i] = cv;
                back[i] = i < first ? -1 : i - 2 * per + kb;
            }
        }
        __syncthreads();
    }

    // ---- 5. the last beat: flags, their exact median, the largest flagged i with 2 cum[i] > median --------------------------------------
    if (tid == 0) {
        s_int[2] = 0;
        s_int[3] = -1;
    }
    __syncthreads();
    {
        int n = 0;
        for (int i = tid; i < T; i += BT_THREADS) n += bt_flag(cum, T, i) ? 1 : 0;
        if (n) atomicAdd(&s_int[2], n);
    }
    __syncthreads();
    const int n_flag = s_int[2];
    if (n_flag == 0) {
        if (tid == 0) n_beats[b] = 0;
        return;
    }
    double med = bt_select(cum, T, (n_flag - 1) / 2, s_hist, &s_prefix, &s_int[0]);
    if ((n_flag & 1) == 0) med = (med + bt_select(cum, T, n_flag / 2, s_hist, &s_prefix, &s_int[0])) * 0.5;
    {
        int last = -1;
        for (int i = tid; i < T; i += BT_THREADS)
            if (bt_flag(cum, T, i) && 2.0 * cum[i] > med) last = i;   // (ascending i: the thread's largest)
        if (last >= 0) atomicMax(&s_int[3], last);
    }
    __syncthreads();

    // ---- 6. backtrace on one lane: beats[r], r = 0 the last beat ------------------------------------------------------------------------
    if (tid == 0) {
        int n = 0;
        for (int cur = s_int[3]; cur >= 0; cur = back[cur]) beats[n++] = cur;      // back[cur] < cur: at most T steps
        s_int[0] = n;
        s_int[1] = INT_MAX;
        s_int[2] = -1;
    }
    __syncthreads();
    const int n = s_int[0];
    if (n == 0) {
        if (tid == 0) n_beats[b] = 0;
        return;
    }

    // ---- 7. trim: s[q] = 0.5 ls[beat q - 1] + ls[beat q] + 0.5 ls[beat q + 1], beat q = beats[n - 1 - q] ------------------------------
    const auto smooth = [&](int q) {
        double s = ls[beats[n - 1 - q]];
        if (q >= 1) s = 0.5 * ls[beats[n - q]] + s;
        if (q + 1 < n) s = s + 0.5 * ls[beats[n - 2 - q]];
        return s;
    };
    double thr = 0.0;
    if (trim) {
        acc = 0.0;
        for (int q = tid; q < n; q += BT_THREADS) {
            const double s = smooth(q);
            acc += s * s;
        }
        thr = 0.5 * sqrt(bt_tree(s_red, acc, add_op) / (double)n);
    }
    {
        int v0 = INT_MAX, v1 = -1;
        for (int q = tid; q < n; q += BT_THREADS)
            if (smooth(q) > thr) {
                v0 = q < v0 ? q : v0;
                v1 = q;
            }
        if (v1 >= 0) {
            atomicMin(&s_int[1], v0);
            atomicMax(&s_int[2], v1);
        }
    }
    __syncthreads();

    // ---- 8. the kept beats [v0, v1) (the end is exclusive) -------------------------------------------------------------------------------
    const int v1 = s_int[2], v0 = v1 < 0 ? 0 : s_int[1];             // (no s above the threshold: nothing is kept)
    for (int q = v0 + tid; q < v1; q += BT_THREADS) row[beats[n - 1 - q]] = 1.0f;
    if (tid == 0) n_beats[b] = v1 > v0 ? v1 - v0 : 0;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
#define BT_MAX_CLIPS 65535                               // the clip is a grid coordinate
#define BT_MAX_T (1 << 20)

static int bt_check_shape(int B, int T) {
    if (B < 1 || T < 5) return TC_ERR_ARG;
    if (B > BT_MAX_CLIPS || T > BT_MAX_T) return TC_ERR_UNSUPPORTED;
    return TC_OK;
}

extern "C" int tcdiff_beat_tempo(const float* onset_env, long o_stride, int B, int T, const float* window, double* partial,
                                 hipStream_t stream) {
    if (!onset_env || !window || !partial || o_stride < 0) return TC_ERR_ARG;
    const int rc = bt_check_shape(B, T);
    if (rc != TC_OK) return rc;
    const int chunks = (T + BT_CHUNK - 1) / BT_CHUNK;
    hipLaunchKernelGGL(beat_tempo_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(BT_WIN / 2), 0, stream, onset_env, o_stride, T, chunks,
                       window, partial);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_beat_track(const float* onset_env, long o_stride, int B, int T, const double* partial, const double* prior,
                                 const double* tables, const int* period_host, int trim, double* local_score, double* cum_score,
                                 int* backlink, int* beats_ws, float* onset_beat, int* period, int* n_beats, double* tempo,
                                 hipStream_t stream) {
    if (!onset_env || !tables || !local_score || !cum_score || !backlink || !beats_ws || !onset_beat || !period || !n_beats || !tempo ||
        o_stride < 0)
        return TC_ERR_ARG;
    if ((partial == nullptr) == (period_host == nullptr) || (partial && !prior)) return TC_ERR_ARG;      // estimated or given
    const int rc = bt_check_shape(B, T);
    if (rc != TC_OK) return rc;
    if (period_host) {
        for (int b = 0; b < B; ++b)
            if (period_host[b] < 1 || period_host[b] >= BT_WIN) return TC_ERR_ARG;      // (period already holds the same values)
    }
    const int chunks = (T + BT_CHUNK - 1) / BT_CHUNK;
    hipLaunchKernelGGL(beat_track_kernel, dim3((unsigned)B), dim3(BT_THREADS), 0, stream, onset_env, o_stride, T, chunks, partial, prior,
                       tables, trim, local_score, cum_score, backlink, beats_ws, onset_beat, period, n_beats, tempo);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
