// The STFT path of the music front end, gfx950: from a waveform to 425 of the 438 columns of `cond` (MFCC, MFCC delta, the onset
// envelope of the percussive part, the tempogram) and the harmonic / percussive separation they hang off.  fp32 arithmetic, every
// launch batched over the B clips (the clip is the last grid dimension), no atomics: every sum runs in a fixed order, so a second
// run and a clip computed alone give the same bits.  The definitions: include/tcdiff_hip.h.
//
//   music_stft_kernel        one frame per workgroup: framing, reflect padding and window on load, 2048-point FFT resident in LDS
//                            (eleven radix-2 stages, twiddles from the host's float64 table), |D|, the 128 mel sums and their maximum
//   music_clip_max_kernel    one workgroup per clip: the largest of its frames' maxima (the launch boundary the clip-wide
//                            maximum needs)
//   music_mfcc_kernel        one frame per workgroup: dB of the frame and of the two frames its delta reads, DCT-II, delta
//   music_median31_kernel    one thread per element and axis: the 31 taps in registers, exact selection by min / max exchanges
//   music_mask_istft_kernel  one frame per workgroup: soft mask, Hermitian extension, inverse FFT, window
//   music_ola_kernel         one thread per output sample: its at most four frames in ascending order (gather, no atomics)
//   music_onset_kernel       one frame per workgroup: dB flux of the percussive mel spectrogram, the median of its 128 values
//   music_tempogram_kernel   one frame per workgroup: ramp padding and window on load, two autocorrelation lags per thread
#include <float.h>

#include "common.h"
#include "music_acf.h"
#include "tcdiff_hip.h"

#define MU_NFFT TC_MUSIC_N_FFT
#define MU_HOP TC_MUSIC_HOP
#define MU_BINS (MU_NFFT / 2 + 1)
#define MU_MELS TC_MUSIC_N_MELS
#define MU_MFCC TC_MUSIC_N_MFCC
#define MU_TEMPO TC_MUSIC_TEMPO_WIN
#define MU_COLS TC_MUSIC_COLS
#define MU_TAPS 31
#define MU_THREADS 256
#define MU_MAX_THREADS 1024

// ---- the 2048-point FFT -----------------------------------------------------------------------------------------------------
// In place over x[2048], which the caller filled in bit-reversed order (element i at mu_brev(i)); decimation in time, stage s
// joins blocks of 2^s; w[k] = exp(-2 pi i k / 2048), k < 1024, conjugated for the inverse (unscaled).  256 threads, four
// butterflies per thread and stage.  Ends with a barrier.
DEVINL int mu_brev(int i) { return (int)(__brev((unsigned)i) >> 21); }

template <bool INV>
DEVINL void mu_fft2048(float2* x, const float2* w) {
    const int tid = threadIdx.x;
    for (int s = 0; s < 11; ++s) {
        const int half = 1 << s;
        __syncthreads();
        for (int q = tid; q < MU_NFFT / 2; q += MU_THREADS) {
            const int j = q & (half - 1);
            const int i0 = ((q >> s) << (s + 1)) + j, i1 = i0 + half;
            float2 c = w[j << (10 - s)];
            if (INV) c.y = -c.y;
            const float2 a = x[i0], b = x[i1];
            const float2 t = {c.x * b.x - c.y * b.y, c.x * b.y + c.y * b.x};
            x[i0] = float2{a.x + t.x, a.y + t.y};
            x[i1] = float2{a.x - t.x, a.y - t.y};
        }
    }
    __syncthreads();
}

// ---- 1. STFT and mel power ----------------------------------------------------------------------------------------------------
// grid (T, B).  y: clip b at y + b * y_stride, n samples.  D / S (both or neither) [B][T][1025], M [B][T][128], frame_max [B][T].
__global__ __launch_bounds__(MU_THREADS) void music_stft_kernel(const float* __restrict__ y, long y_stride, int n, int T,
                                                                const float2* __restrict__ twiddle, const float* __restrict__ win,
                                                                const float* __restrict__ mel_w, const int* __restrict__ mel_range,
                                                                float2* __restrict__ D, float* __restrict__ S, float* __restrict__ M,
                                                                float* __restrict__ frame_max) {
    __shared__ float2 s_x[MU_NFFT];
    __shared__ float2 s_w[MU_NFFT / 2];
    __shared__ float s_pow[MU_BINS];
    const int tid = threadIdx.x, t = blockIdx.x;
    const long b = blockIdx.y;
    const float* yb = y + b * y_stride;
    for (int i = tid; i < MU_NFFT / 2; i += MU_THREADS) s_w[i] = twiddle[i];
    for (int i = tid; i < MU_NFFT; i += MU_THREADS) {
        int j = MU_HOP * t + i - MU_NFFT / 2;             // -1024 <= j <= n + 1023 and n >= 2048: one reflection is enough
        j = j < 0 ? -j : j;
        j = j >= n ? 2 * (n - 1) - j : j;
        s_x[mu_brev(i)] = float2{yb[j] * win[i], 0.0f};
    }
    mu_fft2048<false>(s_x, s_w);
    const long row = b * T + t;
    for (int f = tid; f < MU_BINS; f += MU_THREADS) {
        const float2 v = s_x[f];
        const float a = sqrtf(v.x * v.x + v.y * v.y);
        if (D) {
            D[row * MU_BINS + f] = v;
            S[row * MU_BINS + f] = a;
        }
        s_pow[f] = a * a;
    }
    __syncthreads();
    float* s_mel = reinterpret_cast<float*>(s_x);         // (the spectrum has been read)
    if (tid < MU_MELS) {                                  // filter tid is zero outside bins [lo, hi)
        const int lo = mel_range[2 * tid], hi = mel_range[2 * tid + 1];
        const float* wr = mel_w + (long)tid * MU_BINS;
        float acc = 0.0f;
        for (int f = lo; f < hi; ++f) acc += wr[f] * s_pow[f];
        M[row * MU_MELS + tid] = acc;
        s_mel[tid] = acc;
    }
    __syncthreads();
    for (int o = MU_MELS / 2; o > 0; o >>= 1) {           // the frame's largest mel power, for the clip-wide maximum
        if (tid < o) s_mel[tid] = fmaxf(s_mel[tid], s_mel[tid + o]);
        __syncthreads();
    }
    if (tid == 0) frame_max[row] = s_mel[0];
}

// ---- 2. the largest mel power of a clip ---------------------------------------------------------------------------------------
// grid (B).  M [B][count], the frames' maxima -> mx [B].  A maximum does not depend on the order, so the tree's shape is free.
__global__ __launch_bounds__(MU_MAX_THREADS) void music_clip_max_kernel(const float* __restrict__ M, long count, float* __restrict__ mx) {
    __shared__ float s_red[MU_MAX_THREADS];
    const int tid = threadIdx.x;
    const float* m = M + (long)blockIdx.x * count;
    float v = m[0];
    for (long i = tid; i < count; i += MU_MAX_THREADS) v = fmaxf(v, m[i]);
    s_red[tid] = v;
    __syncthreads();
    for (int o = MU_MAX_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] = fmaxf(s_red[tid], s_red[tid + o]);
        __syncthreads();
    }
    if (tid == 0) mx[blockIdx.x] = s_red[0];
}

// 10 log10(max(1e-10, p)) - ref, floored; contraction off: the clip's largest power must give exactly ref - ref = 0
DEVINL float mu_db(float p, float ref, float floor_) {
#pragma clang fp contract(off)
    const float d = 10.0f * log10f(fmaxf(1e-10f, p)) - ref;
    return fmaxf(d, floor_);
}

// ---- 3. mel dB, MFCC and delta -----------------------------------------------------------------------------------------------
// grid (T, B), 128 threads.  The dB maximum of a clip is 0 (its largest power against itself), so the floor is -80.  Frame t's
// delta is (x[c + 1] - x[c - 1]) / 2 with c = t clamped to [1, T - 2]: the block evaluates the MFCC of the three frames.
__global__ __launch_bounds__(MU_MELS) void music_mfcc_kernel(const float* __restrict__ M, const float* __restrict__ mx, int T,
                                                             const float* __restrict__ dct, float* __restrict__ mel_db,
                                                             float* __restrict__ feats) {
    __shared__ float s_db[3][MU_MELS];
    __shared__ float s_c[3][MU_MFCC];
    const int tid = threadIdx.x, t = blockIdx.x;
    const long b = blockIdx.y;
    const int c = t < 1 ? 1 : (t > T - 2 ? T - 2 : t);
    const int fr[3] = {t, c - 1, c + 1};
    float ref;
    {
#pragma clang fp contract(off)
        ref = 10.0f * log10f(fmaxf(1e-10f, mx[b]));
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) s_db[k][tid] = mu_db(M[(b * T + fr[k]) * MU_MELS + tid], ref, -80.0f);
    mel_db[(b * T + t) * MU_MELS + tid] = s_db[0][tid];
    __syncthreads();
    if (tid < 3 * MU_MFCC) {
        const int k = tid / MU_MFCC, q = tid - k * MU_MFCC;
        const float* dr = dct + q * MU_MELS;
        float acc = 0.0f;
        for (int m = 0; m < MU_MELS; ++m) acc += dr[m] * s_db[k][m];
        s_c[k][q] = acc;
    }
    __syncthreads();
    if (tid < MU_MFCC) {
        float* o = feats + (b * T + t) * MU_COLS;
        o[tid] = s_c[0][tid];
        o[MU_MFCC + tid] = (s_c[2][tid] - s_c[1][tid]) * 0.5f;
    }
}

// ---- 4. the two 31-tap medians ------------------------------------------------------------------------------------------------
// index i of an axis of length L extended as scipy.ndimage's 'reflect' (d c b a | a b c d | d c b a, period 2 L)
DEVINL int mu_reflect(int i, int L) {
    if (i >= 0 && i < L) return i;
    const int p = 2 * L;
    int m = i % p;
    m = m < 0 ? m + p : m;
    return m < L ? m : p - 1 - m;
}

// The exact median of 31 values by forgetful selection: neither the smallest nor the largest of 17 values can be the 16th of
// 31, so both are dropped and the next value is taken in, 16 values lose two again, ... until the middle one of three is left.
// Min / max exchanges only (255 of them), every index a compile-time constant after unrolling: the window stays in registers.
DEVINL void mu_order(float& a, float& b) {
    const float lo = fminf(a, b);
    b = fmaxf(a, b);
    a = lo;
}
DEVINL float mu_median31(float (&v)[MU_TAPS]) {
    constexpr int HI = MU_TAPS / 2 + 1;                   // round j works on v[j .. HI]
#pragma unroll
    for (int j = 0; j < MU_TAPS / 2; ++j) {
#pragma unroll
        for (int i = j; i < HI; ++i) mu_order(v[i], v[i + 1]);              // the largest to v[HI]
#pragma unroll
        for (int i = HI - 1; i > j; --i) mu_order(v[i - 1], v[i]);          // the smallest to v[j]
        if (j + HI + 1 < MU_TAPS) v[HI] = v[j + HI + 1];                    // the next value takes the largest's place
    }
    return v[HI - 1];
}

// grid (ceil(T * 1025 / 256), 2, B): blockIdx.y = 0 the median along time -> H, 1 along frequency -> P.  One thread per element.
__global__ __launch_bounds__(MU_THREADS) void music_median31_kernel(const float* __restrict__ S, int T, float* __restrict__ H,
                                                                    float* __restrict__ P) {
    const int e = blockIdx.x * MU_THREADS + threadIdx.x;
    if (e >= T * MU_BINS) return;
    const int axis = blockIdx.y;
    const long b = blockIdx.z;
    const int t = e / MU_BINS, f = e - t * MU_BINS;
    const float* Sb = S + b * T * MU_BINS;
    float v[MU_TAPS];
#pragma unroll
    for (int k = 0; k < MU_TAPS; ++k) {
        const int d = k - MU_TAPS / 2;
        v[k] = axis == 0 ? Sb[(long)mu_reflect(t + d, T) * MU_BINS + f] : Sb[(long)t * MU_BINS + mu_reflect(f + d, MU_BINS)];
    }
    (axis == 0 ? H : P)[b * T * MU_BINS + e] = mu_median31(v);
}

// ---- 5. / 6. soft masks and the inverse STFT ------------------------------------------------------------------------------------
// grid (T, W, B): blockIdx.y = 0 the percussive part (mask of P against H), 1 the harmonic.  frames [B][W][T][2048].
__global__ __launch_bounds__(MU_THREADS) void music_mask_istft_kernel(const float2* __restrict__ D, const float* __restrict__ H,
                                                                      const float* __restrict__ P, int T,
                                                                      const float2* __restrict__ twiddle, const float* __restrict__ win,
                                                                      float* __restrict__ frames) {
    __shared__ float2 s_x[MU_NFFT];
    __shared__ float2 s_w[MU_NFFT / 2];
    const int tid = threadIdx.x, t = blockIdx.x, part = blockIdx.y, W = gridDim.y;
    const long b = blockIdx.z;
    const long row = (b * T + t) * MU_BINS;
    for (int i = tid; i < MU_NFFT / 2; i += MU_THREADS) s_w[i] = twiddle[i];
    for (int f = tid; f < MU_BINS; f += MU_THREADS) {
        const float h = H[row + f], p = P[row + f];
        const float X = part == 0 ? p : h, R = part == 0 ? h : p;
        const float Z = fmaxf(X, R);
        float m = 0.5f;
        if (!(Z < FLT_MIN)) {
            float xs = X / Z, rs = R / Z;
            xs *= xs;
            rs *= rs;
            m = xs / (xs + rs);
        }
        const float2 d = D[row + f];
        const float2 v = {d.x * m, d.y * m};
        s_x[mu_brev(f)] = v;
        if (f > 0 && f < MU_NFFT / 2) s_x[mu_brev(MU_NFFT - f)] = float2{v.x, -v.y};
    }
    mu_fft2048<true>(s_x, s_w);
    float* o = frames + ((b * W + part) * T + t) * MU_NFFT;
    for (int i = tid; i < MU_NFFT; i += MU_THREADS) o[i] = s_x[i].x * (1.0f / MU_NFFT) * win[i];
}

// grid (ceil(n / 256), W, B).  Output sample i is padded sample p = i + 1024: frames ceil((p - 2047) / 512) .. floor(p / 512),
// ascending.  A sample no frame reaches stays 0 (the zero fill).
__global__ __launch_bounds__(MU_THREADS) void music_ola_kernel(const float* __restrict__ frames, const float* __restrict__ win, int n,
                                                               int T, float* __restrict__ percussive, float* __restrict__ harmonic) {
    const int i = blockIdx.x * MU_THREADS + threadIdx.x;
    if (i >= n) return;
    const int part = blockIdx.y, W = gridDim.y;
    const long b = blockIdx.z;
    const int p = i + MU_NFFT / 2;
    const int lo = p < MU_NFFT ? 0 : (p - MU_NFFT) / MU_HOP + 1;
    const int hi = p / MU_HOP < T - 1 ? p / MU_HOP : T - 1;
    const float* fr = frames + (b * W + part) * T * MU_NFFT;
    float acc = 0.0f, ws = 0.0f;
    for (int t = lo; t <= hi; ++t) {
        const int k = p - MU_HOP * t;
        acc += fr[(long)t * MU_NFFT + k];
        ws += win[k] * win[k];
    }
    (part == 0 ? percussive : harmonic)[b * n + i] = ws > FLT_MIN ? acc / ws : acc;
}

// ---- 7. onset envelope ----------------------------------------------------------------------------------------------------------
// grid (T, B), 128 threads.  M: the mel power of the percussive signal, mx its clip maximum.  onset_env[t] = 0 for t < 3, else
// the median over the bins of max(0, dB[t - 2] - dB[t - 3]): the mean of the values of rank 63 and 64 in (value, bin) order.
__global__ __launch_bounds__(MU_MELS) void music_onset_kernel(const float* __restrict__ M, const float* __restrict__ mx, int T,
                                                              float* __restrict__ onset_env, float* __restrict__ feats) {
    __shared__ float s_v[MU_MELS];
    __shared__ float s_mid[2];
    const int tid = threadIdx.x, t = blockIdx.x;
    const long b = blockIdx.y;
    float out = 0.0f;
    if (t >= 3) {                                         // (uniform over the block)
        float floor_;
        {
#pragma clang fp contract(off)
            floor_ = 10.0f * log10f(fmaxf(1e-10f, mx[b])) - 80.0f;
        }
        const float cur = mu_db(M[(b * T + t - 2) * MU_MELS + tid], 0.0f, floor_);
        const float prev = mu_db(M[(b * T + t - 3) * MU_MELS + tid], 0.0f, floor_);
        const float v = fmaxf(0.0f, cur - prev);
        s_v[tid] = v;
        __syncthreads();
        int r = 0;
        for (int j = 0; j < MU_MELS; ++j) {
            const float u = s_v[j];
            r += (u < v || (u == v && j < tid)) ? 1 : 0;
        }
        if (r == MU_MELS / 2 - 1) s_mid[0] = v;
        if (r == MU_MELS / 2) s_mid[1] = v;
        __syncthreads();
        out = (s_mid[0] + s_mid[1]) * 0.5f;
    }
    if (tid == 0) {
        onset_env[b * T + t] = out;
        feats[(b * T + t) * MU_COLS + 2 * MU_MFCC] = out;
    }
}

// ---- 8. tempogram -----------------------------------------------------------------------------------------------------------------
// grid (T, B), 192 threads.  Frame t is samples [t, t + 384) of onset_env padded by 192 on both sides with a linear ramp to 0
// (numpy.pad: sample j of the left ramp is j * (env[0] / 192), of the right one (191 - j) * (env[T - 1] / 192)), times the window.
// Thread k sums lags k and 383 - k, each in ascending sample order: 385 products per thread.
__global__ __launch_bounds__(MU_TEMPO / 2) void music_tempogram_kernel(const float* __restrict__ onset_env, int T,
                                                                       const float* __restrict__ win, float* __restrict__ feats) {
    __shared__ float s_x[MU_TEMPO];
    __shared__ float s_red[256];
    const int tid = threadIdx.x, t = blockIdx.x;
    const long b = blockIdx.y;
    const float* env = onset_env + b * T;
    for (int i = tid; i < MU_TEMPO; i += MU_TEMPO / 2) s_x[i] = mu_ramp_sample<MU_TEMPO>(env, T, t, i) * win[i];
    __syncthreads();
    const int la = tid, lb = MU_TEMPO - 1 - tid;
    float a, c;
    mu_acf_pair<MU_TEMPO>(s_x, tid, a, c);
    const float mx = mu_acf_absmax<MU_TEMPO>(s_red, a, c, tid);
    float* o = feats + (b * T + t) * MU_COLS + 2 * MU_MFCC + 1;
    o[la] = mx < FLT_MIN ? a : a / mx;
    o[lb] = mx < FLT_MIN ? c : c / mx;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
#define MU_MAX_CLIPS 65535                               // the clip is a grid y / z coordinate

static int mu_check_shape(int B, int n) {
    if (B < 1 || n < MU_NFFT) return TC_ERR_ARG;
    if (B > MU_MAX_CLIPS || n > 0x7fffffff / 4) return TC_ERR_UNSUPPORTED;       // T * 1025 and n + 1024 stay below 2^31
    return TC_OK;
}

extern "C" int tcdiff_music_stft(const float* y, long y_stride, int B, int n, const float* twiddle, const float* window,
                                 const float* mel_w, const int* mel_range, float* D, float* S, float* M, float* frame_max,
                                 hipStream_t stream) {
    if (!y || !twiddle || !window || !mel_w || !mel_range || !M || !frame_max || (D == nullptr) != (S == nullptr)) return TC_ERR_ARG;
    const int rc = mu_check_shape(B, n);
    if (rc != TC_OK) return rc;
    if (y_stride < 0) return TC_ERR_ARG;
    const int T = 1 + n / MU_HOP;
    hipLaunchKernelGGL(music_stft_kernel, dim3((unsigned)T, (unsigned)B), dim3(MU_THREADS), 0, stream, y, y_stride, n, T,
                       reinterpret_cast<const float2*>(twiddle), window, mel_w, mel_range, reinterpret_cast<float2*>(D), S, M, frame_max);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_music_mfcc(const float* M, const float* frame_max, int B, int T, const float* dct, float* mx, float* mel_db,
                                 float* feats, hipStream_t stream) {
    if (!M || !frame_max || !dct || !mx || !mel_db || !feats) return TC_ERR_ARG;
    if (B < 1 || T < 5) return TC_ERR_ARG;
    if (B > MU_MAX_CLIPS) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(music_clip_max_kernel, dim3((unsigned)B), dim3(MU_MAX_THREADS), 0, stream, frame_max, (long)T, mx);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(music_mfcc_kernel, dim3((unsigned)T, (unsigned)B), dim3(MU_MELS), 0, stream, M, mx, T, dct, mel_db, feats);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_music_hpss(const float* D, const float* S, int B, int n, const float* twiddle, const float* window, float* H,
                                 float* P, float* frames, float* percussive, float* harmonic, hipStream_t stream) {
    if (!D || !S || !twiddle || !window || !H || !P || !frames || !percussive) return TC_ERR_ARG;
    const int rc = mu_check_shape(B, n);
    if (rc != TC_OK) return rc;
    const int T = 1 + n / MU_HOP;
    const unsigned W = harmonic ? 2 : 1;
    const unsigned eb = (unsigned)(((long)T * MU_BINS + MU_THREADS - 1) / MU_THREADS);
    hipLaunchKernelGGL(music_median31_kernel, dim3(eb, 2, (unsigned)B), dim3(MU_THREADS), 0, stream, S, T, H, P);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(music_mask_istft_kernel, dim3((unsigned)T, W, (unsigned)B), dim3(MU_THREADS), 0, stream,
                       reinterpret_cast<const float2*>(D), H, P, T, reinterpret_cast<const float2*>(twiddle), window, frames);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(music_ola_kernel, dim3((unsigned)((n + MU_THREADS - 1) / MU_THREADS), W, (unsigned)B), dim3(MU_THREADS), 0, stream,
                       frames, window, n, T, percussive, harmonic);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_music_onset(const float* M, const float* frame_max, int B, int T, const float* window, float* mx,
                                  float* onset_env, float* feats, hipStream_t stream) {
    if (!M || !frame_max || !window || !mx || !onset_env || !feats) return TC_ERR_ARG;
    if (B < 1 || T < 5) return TC_ERR_ARG;
    if (B > MU_MAX_CLIPS) return TC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(music_clip_max_kernel, dim3((unsigned)B), dim3(MU_MAX_THREADS), 0, stream, frame_max, (long)T, mx);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(music_onset_kernel, dim3((unsigned)T, (unsigned)B), dim3(MU_MELS), 0, stream, M, mx, T, onset_env, feats);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(music_tempogram_kernel, dim3((unsigned)T, (unsigned)B), dim3(MU_TEMPO / 2), 0, stream, onset_env, T, window, feats);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
