// The chroma columns of the music front end, gfx950: from the harmonic signal to columns 40-51 of `cond` -- librosa 0.9.2's
// chroma_cqt (estimate_tuning = piptrack + pitch_tuning, the seven-octave constant-Q transform with resampy's kaiser_fast
// decimation by two between octaves, the fold to 12 chroma) restated at the reference's arguments: sr 30720, hop 512, 36 bins per
// octave, 7 octaves from C1.  The definitions: include/tcdiff_hip.h.  fp32 arithmetic as librosa's (the tuning residual and its
// histogram in float64), every launch batched over the B clips, no float atomics, every sum in a fixed order: a second run, and a
// clip computed alone, give the same bits.  Nothing comes back to the host: the response kernel reads the clip's tuning index
// on the device and picks that tuning's slab of the basis.
//
//   chroma_pyramid_kernel   one workgroup per (tile of 64 octave-6 samples, clip): the 63-tap decimation run six times over a tile
//                           of the clip and its halo, both resident in LDS; a tile recomputes its halo (1953 + 1890 input samples)
//                           instead of waiting for its neighbour and stores the samples it owns of all six signals
//   chroma_tuning_kernel    one workgroup per clip, eight waves: a wave per STFT frame (frame maximum, piptrack flags, pitch and
//                           magnitude of the flagged bins, packed through an integer LDS counter), the exact median of the
//                           magnitudes by radix selection on the ordered bit patterns (beat.hip's, 32 bits), the float64 residuals
//                           into a 100-cell integer histogram in LDS, the first argmax
//   chroma_response_kernel  one workgroup per (frame, clip): the seven octaves' 1024-sample frames (zero padding, rectangular
//                           window) loaded bit-reversed, seven 1024-point FFTs side by side in LDS (music.hip's radix-2 stages and
//                           float64-computed twiddles), 252 banded complex dot products with the tuning's basis slab, |C| times the
//                           per-bin scale, the fold to 12 and the division by the frame's maximum
#include <float.h>

#include "common.h"
#include "tcdiff_hip.h"

#define CH_NFFT TC_CHROMA_N_FFT
#define CH_HOP TC_MUSIC_HOP
#define CH_OCT TC_CHROMA_OCTAVES
#define CH_BPO TC_CHROMA_BPO
#define CH_BINS TC_CHROMA_BINS
#define CH_BAND TC_CHROMA_BAND
#define CH_TUNINGS TC_CHROMA_TUNINGS
#define CH_TAPS TC_CHROMA_TAPS
#define CH_STFT_BINS (TC_MUSIC_N_FFT / 2 + 1)
#define CH_THREADS 256
#define CH_TILE 64                                       // octave-6 samples per workgroup of the pyramid
#define CH_TUNE_THREADS 512
#define CH_TUNE_WAVES (CH_TUNE_THREADS / TC_WAVE)

// length of signal s of the pyramid (0: the clip itself)
DEVINL int ch_stage_len(int n, int s) { return (int)(((long)n + (1L << s) - 1) >> s); }

// ---- 1. the pyramid --------------------------------------------------------------------------------------------------------------
// Stage s of a tile covers ch_span(s) samples of signal s: the tile's 64 samples of signal 6 need 2 * 64 + 61 of signal 5 (taps
// -31 .. 31 around every second sample), those 2 * 189 + 61 of signal 4, ... 7939 of the clip.
__host__ __device__ constexpr int ch_span(int s) { return s == CH_OCT - 1 ? CH_TILE : 2 * ch_span(s + 1) + (CH_TAPS - 2); }

// grid (ceil(ceil(n / 64) / 64), B).  y: clip b at y + b * y_stride, n samples.  pyramid [B][P]: signals 1 .. 6 one after another.
// Sample g of signal s is sqrt(2) sum_k h[k] x[2 g + k - 31], k ascending, x signal s - 1, zero outside it: adding a zero product
// leaves the sum's bits as they are, so the halo and the clip's ends need no second code path.  Even signals live in s_a, odd
// ones in s_b.
__global__ __launch_bounds__(CH_THREADS) void chroma_pyramid_kernel(const float* __restrict__ y, long y_stride, int n,
                                                                    const float* __restrict__ taps, float* __restrict__ pyramid, long P) {
    __shared__ float s_a[ch_span(0)];
    __shared__ float s_b[ch_span(1)];
    __shared__ float s_h[CH_TAPS + 1];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const long b = blockIdx.y;
    const float* yb = y + b * y_stride;
    float* out = pyramid + b * P;
    constexpr int span[CH_OCT] = {ch_span(0), ch_span(1), ch_span(2), ch_span(3), ch_span(4), ch_span(5), ch_span(6)};
    if (tid < CH_TAPS) s_h[tid] = taps[tid];
    int first = tile * CH_TILE;                           // of the tile's span of signal 6 ...
    for (int s = CH_OCT - 1; s > 0; --s) first = 2 * first - CH_TAPS / 2;      // ... and of the clip: 64^2 tile - 1953
    for (int i = tid; i < span[0]; i += CH_THREADS) {
        const int g = first + i;
        s_a[i] = (g >= 0 && g < n) ? yb[g] : 0.0f;
    }
    __syncthreads();
    const float gain = 1.41421356237309504880f;
    long at = 0;
    for (int s = 1; s < CH_OCT; ++s) {
        const float* src = (s & 1) ? s_a : s_b;
        float* dst = (s & 1) ? s_b : s_a;
        first = (first + CH_TAPS / 2) / 2;                // exact: first + 31 is twice the span's first sample of signal s
        const int len = ch_stage_len(n, s);
        const int own0 = (tile * CH_TILE) << (CH_OCT - 1 - s), own1 = own0 + (CH_TILE << (CH_OCT - 1 - s));
        for (int i = tid; i < span[s]; i += CH_THREADS) {
            float acc = 0.0f;
#pragma unroll 9
            for (int k = 0; k < CH_TAPS; ++k) acc = fmaf(s_h[k], src[2 * i + k], acc);
            const int g = first + i;
            const bool inside = g >= 0 && g < len;
            const float v = inside ? gain * acc : 0.0f;
            dst[i] = v;
            if (inside && g >= own0 && g < own1) out[at + g] = v;
        }
        at += len;
        __syncthreads();
    }
}

// ---- 2. the tuning estimate ---------------------------------------------------------------------------------------------------------
// the bit pattern of a float as an unsigned integer of the same order (negative values reversed, then the sign bit flipped)
DEVINL unsigned ch_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
DEVINL float ch_unkey(unsigned k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

// The magnitude of rank `rank` (0 = smallest) among the clip's n pitches by radix selection, eight bits a pass from the top
// (integer LDS atomics: the counts do not depend on the order).
DEVINL float ch_select(const float* mag, int n, int rank, int* s_hist, unsigned* s_prefix, int* s_rank) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (tid == 0) {
        *s_prefix = 0;
        *s_rank = rank;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        const unsigned prefix = *s_prefix;
        for (int i = tid; i < n; i += CH_TUNE_THREADS) {
            const unsigned key = ch_key(mag[i]);
            if (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(int)((key >> shift) & 255)], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int r = *s_rank, d = 0;
            while (d < 255 && r >= s_hist[d]) r -= s_hist[d++];
            *s_prefix = prefix | ((unsigned)d << shift);
            *s_rank = r;
        }
        __syncthreads();
    }
    return ch_unkey(*s_prefix);
}

// grid (B), 512 threads.  S [B][T][1025]: the magnitude STFT of the clip (tcdiff_music_stft).  pitch_ws / mag_ws [B][T][W],
// W = f_hi - f_lo + 1: the clip's pitches, packed from the front in the order the waves reserve their places (an integer LDS
// counter).  That order differs from run to run and nothing below depends on it: the median is a selection by counting, the
// histogram integer counts.
__global__ __launch_bounds__(CH_TUNE_THREADS) void chroma_tuning_kernel(const float* __restrict__ S, int T, int f_lo, int f_hi, float bin_hz,
                                                                        const double* __restrict__ edges, float* __restrict__ pitch_ws,
                                                                        float* __restrict__ mag_ws, int* __restrict__ tuning_index,
                                                                        int* __restrict__ n_pitches, float* __restrict__ threshold,
                                                                        int* __restrict__ counts) {
    __shared__ double s_edges[CH_TUNINGS + 1];
    __shared__ int s_counts[CH_TUNINGS];
    __shared__ int s_hist[256];
    __shared__ unsigned s_prefix;
    __shared__ int s_int[2];
    const int tid = threadIdx.x, lane = tid & (TC_WAVE - 1), wave = tid / TC_WAVE;
    const long b = blockIdx.x;
    const int W = f_hi - f_lo + 1;
    const long count = (long)T * W;
    const float* Sb = S + b * T * CH_STFT_BINS;
    float* pw = pitch_ws + b * count;
    float* mw = mag_ws + b * count;
    if (tid < CH_TUNINGS + 1) s_edges[tid] = edges[tid];
    if (tid < CH_TUNINGS) s_counts[tid] = 0;
    if (tid == 0) s_int[0] = 0;
    __syncthreads();

    // ---- piptrack: a wave per frame ----
    for (int t = wave; t < T; t += CH_TUNE_WAVES) {
        const float* row = Sb + (long)t * CH_STFT_BINS;
        float mx = 0.0f;                                  // (a maximum does not depend on the order)
        for (int f = lane; f < CH_STFT_BINS; f += TC_WAVE) mx = fmaxf(mx, row[f]);
#pragma unroll
        for (int off = TC_WAVE / 2; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        const float ref = 0.1f * mx;
        for (int f0 = f_lo; f0 <= f_hi; f0 += TC_WAVE) {              // 1 <= f_lo, f_hi <= 1023 (the launcher's check)
#pragma clang fp contract(off)
            const int f = f0 + lane;
            float pitch = 0.0f, mag = 0.0f;
            if (f <= f_hi) {
                const float s0 = row[f - 1], s1 = row[f], s2 = row[f + 1];
                const float m0 = s0 > ref ? s0 : 0.0f, m1 = s1 > ref ? s1 : 0.0f, m2 = s2 > ref ? s2 : 0.0f;
                if (m1 > m0 && m1 >= m2) {
                    const float avg = 0.5f * (s2 - s0);
                    const float den = 2.0f * s1 - s2 - s0;
                    const float shift = avg / (den + (fabsf(den) < FLT_MIN ? 1.0f : 0.0f));
                    const float dskew = 0.5f * avg * shift;
                    pitch = ((float)f + shift) * bin_hz;  // at least (f_lo - 0.5) bin_hz > 0
                    mag = s1 + dskew;
                }
            }
            const bool is_pitch = pitch > 0.0f;
            const unsigned long long votes = __ballot(is_pitch);      // (every lane of the wave is here)
            if (votes == 0) continue;
            int base = 0;
            if (lane == 0) base = atomicAdd(&s_int[0], __popcll(votes));
            base = __shfl(base, 0);
            if (is_pitch) {                               // at most T * W pitches: the workspace cannot overflow
                const int at = base + __popcll(votes & ((1ull << lane) - 1ull));
                pw[at] = pitch;
                mw[at] = mag;
            }
        }
    }
    __syncthreads();                                      // (orders the workgroup's workspace stores before its loads below)
    const int n = s_int[0];
    if (n == 0) {                                         // no pitch: tuning 0.0 (uniform over the workgroup)
        if (tid < CH_TUNINGS) counts[b * CH_TUNINGS + tid] = 0;
        if (tid == 0) {
            tuning_index[b] = CH_TUNINGS / 2;
            n_pitches[b] = 0;
            threshold[b] = 0.0f;
        }
        return;
    }

    // ---- the median of the magnitudes, numpy's: the mean of the two middle values for an even count ----
    float thr = ch_select(mw, n, (n - 1) / 2, s_hist, &s_prefix, &s_int[1]);
    if ((n & 1) == 0) thr = (thr + ch_select(mw, n, n / 2, s_hist, &s_prefix, &s_int[1])) * 0.5f;

    // ---- residuals of the pitches at or above it, in float64 from the float32 pitch; numpy.histogram over the edges ----
    for (int i = tid; i < n; i += CH_TUNE_THREADS) {
        const float p = pw[i];
        if (!(mw[i] >= thr)) continue;
        double r = (double)CH_BPO * log2((double)p / 27.5);
        r -= floor(r);
        if (r >= 0.5) r -= 1.0;
        int k = (int)((r + 0.5) * (double)CH_TUNINGS);
        k = k < 0 ? 0 : (k > CH_TUNINGS - 1 ? CH_TUNINGS - 1 : k);
        while (k > 0 && r < s_edges[k]) --k;              // cell k is [edges[k], edges[k + 1])
        while (k < CH_TUNINGS - 1 && r >= s_edges[k + 1]) ++k;
        atomicAdd(&s_counts[k], 1);
    }
    __syncthreads();
    if (tid < CH_TUNINGS) counts[b * CH_TUNINGS + tid] = s_counts[tid];
    if (tid == 0) {
        int best = 0;
        for (int k = 1; k < CH_TUNINGS; ++k) best = s_counts[k] > s_counts[best] ? k : best;      // the first argmax
        tuning_index[b] = best;
        n_pitches[b] = n;
        threshold[b] = thr;
    }
}

// ---- 3. the response, the fold and the normalisation ------------------------------------------------------------------------------
DEVINL int ch_brev(int i) { return (int)(__brev((unsigned)i) >> 22); }

// grid (T, B).  Octave o (0: the top 36 bins, the clip itself; 6: the bottom 36, signal 6) frames its signal at hop 512 >> o:
// 1024 samples centred on t (512 >> o), zeros outside the signal.  basis [100][36][CH_BAND] complex, row r of tuning k holding
// bins [lo, hi) of band [100][36][2]; scale [100][252], lowest bin first.  cqt_mag (optional) [B][T][252], chroma [B][T][12].
__global__ __launch_bounds__(CH_THREADS) void chroma_response_kernel(const float* __restrict__ y, long y_stride,
                                                                     const float* __restrict__ pyramid, long P, int n, int T,
                                                                     const int* __restrict__ tuning_index, const float2* __restrict__ twiddle,
                                                                     const float2* __restrict__ basis, const int* __restrict__ band,
                                                                     const float* __restrict__ scale, float* __restrict__ chroma,
                                                                     float* __restrict__ cqt_mag) {
    __shared__ float2 s_x[CH_OCT][CH_NFFT];
    __shared__ float2 s_w[CH_NFFT / 2];
    __shared__ float s_mag[CH_BINS];
    __shared__ float s_chr[TC_CHROMA_N];
    const int tid = threadIdx.x, t = blockIdx.x;
    const long b = blockIdx.y;
    int k = tuning_index[b];
    k = k < 0 ? 0 : (k > CH_TUNINGS - 1 ? CH_TUNINGS - 1 : k);        // (a table index: never trusted)
    for (int i = tid; i < CH_NFFT / 2; i += CH_THREADS) s_w[i] = twiddle[i];
    for (int e = tid; e < CH_OCT * CH_NFFT; e += CH_THREADS) {
        const int o = e / CH_NFFT, i = e - o * CH_NFFT;
        const float* src = y + b * y_stride;
        if (o > 0) {
            src = pyramid + b * P;
            for (int s = 1; s < o; ++s) src += ch_stage_len(n, s);
        }
        const int len = ch_stage_len(n, o);
        const int j = t * (CH_HOP >> o) + i - CH_NFFT / 2;            // t (512 >> o) <= n >> o: no overflow
        s_x[o][ch_brev(i)] = float2{(j >= 0 && j < len) ? src[j] : 0.0f, 0.0f};
    }
    // the seven FFTs, stage by stage (music.hip's mu_fft2048 with ten stages): 7 x 512 butterflies between barriers
    for (int s = 0; s < 10; ++s) {
        const int half = 1 << s;
        __syncthreads();
        for (int q = tid; q < CH_OCT * (CH_NFFT / 2); q += CH_THREADS) {
            const int o = q / (CH_NFFT / 2), p = q - o * (CH_NFFT / 2);
            const int j = p & (half - 1);
            const int i0 = ((p >> s) << (s + 1)) + j, i1 = i0 + half;
            const float2 c = s_w[j << (9 - s)];
            const float2 a = s_x[o][i0], d = s_x[o][i1];
            const float2 u = {c.x * d.x - c.y * d.y, c.x * d.y + c.y * d.x};
            s_x[o][i0] = float2{a.x + u.x, a.y + u.y};
            s_x[o][i1] = float2{a.x - u.x, a.y - u.y};
        }
    }
    __syncthreads();
    const long row = b * T + t;
    if (tid < CH_BINS) {
        const int o = tid / CH_BPO, r = tid - o * CH_BPO;
        const long slab = (long)k * CH_BPO + r;
        int lo = band[2 * slab], hi = band[2 * slab + 1];
        lo = lo < 0 ? 0 : (lo > CH_NFFT / 2 + 1 ? CH_NFFT / 2 + 1 : lo);
        hi = hi > CH_NFFT / 2 + 1 ? CH_NFFT / 2 + 1 : hi;
        hi = hi > lo + CH_BAND ? lo + CH_BAND : hi;
        const float2* br = basis + slab * CH_BAND;
        float re = 0.0f, im = 0.0f;
        for (int f = lo; f < hi; ++f) {                   // ascending bins
            const float2 c = br[f - lo], x = s_x[o][f];
            re += c.x * x.x - c.y * x.y;
            im += c.x * x.y + c.y * x.x;
        }
        const int bin = CH_BPO * (CH_OCT - 1 - o) + r;
        const float m = sqrtf(re * re + im * im) * scale[(long)k * CH_BINS + bin];
        s_mag[bin] = m;
        if (cqt_mag) cqt_mag[row * CH_BINS + bin] = m;
    }
    __syncthreads();
    float acc = 0.0f;
    if (tid < TC_CHROMA_N) {                              // chroma c: bins 3 c - 1, 3 c, 3 c + 1 (mod 36) of every octave, lowest first
        for (int o = 0; o < CH_OCT; ++o)
            for (int d = -1; d <= 1; ++d) acc += s_mag[CH_BPO * o + (3 * tid + d + CH_BPO) % CH_BPO];
        s_chr[tid] = acc;
    }
    __syncthreads();
    if (tid < TC_CHROMA_N) {
        float mx = s_chr[0];
        for (int c = 1; c < TC_CHROMA_N; ++c) mx = fmaxf(mx, s_chr[c]);
        chroma[row * TC_CHROMA_N + tid] = mx < FLT_MIN ? acc : acc / mx;
    }
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
#define CH_MAX_CLIPS 65535                               // the clip is a grid y coordinate

static int ch_check_shape(int B, int n) {
    if (B < 1 || n < TC_MUSIC_N_FFT) return TC_ERR_ARG;
    if (B > CH_MAX_CLIPS || n > 0x7fffffff / 4) return TC_ERR_UNSUPPORTED;
    return TC_OK;
}

static long ch_pyramid_len(int n) {
    long P = 0;
    for (int s = 1; s < CH_OCT; ++s) P += ((long)n + (1L << s) - 1) >> s;
    return P;
}

extern "C" int tcdiff_chroma_pyramid(const float* y, long y_stride, int B, int n, const float* taps, float* pyramid, hipStream_t stream) {
    if (!y || !taps || !pyramid || y_stride < 0) return TC_ERR_ARG;
    const int rc = ch_check_shape(B, n);
    if (rc != TC_OK) return rc;
    const int n6 = (int)(((long)n + 63) >> 6);
    hipLaunchKernelGGL(chroma_pyramid_kernel, dim3((unsigned)((n6 + CH_TILE - 1) / CH_TILE), (unsigned)B), dim3(CH_THREADS), 0, stream, y,
                       y_stride, n, taps, pyramid, ch_pyramid_len(n));
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_chroma_tuning(const float* S, int B, int T, int f_lo, int f_hi, float bin_hz, const double* edges, float* pitch_ws,
                                    float* mag_ws, int* tuning_index, int* n_pitches, float* threshold, int* counts, hipStream_t stream) {
    if (!S || !edges || !pitch_ws || !mag_ws || !tuning_index || !n_pitches || !threshold || !counts) return TC_ERR_ARG;
    if (B < 1 || T < 5 || f_lo < 1 || f_hi > CH_STFT_BINS - 2 || f_hi < f_lo || !(bin_hz > 0.0f)) return TC_ERR_ARG;
    if (B > CH_MAX_CLIPS || T > (1 << 20)) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(chroma_tuning_kernel, dim3((unsigned)B), dim3(CH_TUNE_THREADS), 0, stream, S, T, f_lo, f_hi, bin_hz, edges, pitch_ws,
                       mag_ws, tuning_index, n_pitches, threshold, counts);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_chroma_response(const float* y, long y_stride, const float* pyramid, int B, int n, const int* tuning_index,
                                      const float* twiddle, const float* basis, const int* band, const float* scale, float* chroma,
                                      float* cqt_mag, hipStream_t stream) {
    if (!y || !pyramid || !tuning_index || !twiddle || !basis || !band || !scale || !chroma || y_stride < 0) return TC_ERR_ARG;
    const int rc = ch_check_shape(B, n);
    if (rc != TC_OK) return rc;
    const int T = 1 + n / CH_HOP;
    hipLaunchKernelGGL(chroma_response_kernel, dim3((unsigned)T, (unsigned)B), dim3(CH_THREADS), 0, stream, y, y_stride, pyramid,
                       ch_pyramid_len(n), n, T, tuning_index, reinterpret_cast<const float2*>(twiddle), reinterpret_cast<const float2*>(basis),
                       band, scale, chroma, cqt_mag);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
