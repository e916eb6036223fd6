// From a WAV file's bytes to mono samples at 30720 Hz, gfx950: what librosa.load(path, sr=30720) of dataset_utils.py:62 does after
// the container is parsed (tcdiff_amd/audio.py, host) -- soundfile's decode to float32, librosa.to_mono and resampy's kaiser_best
// interpolating resampler -- in two launches for any number of clips.  The definitions: include/tcdiff_hip.h.  No host
// synchronisation, no atomics, every sum in a fixed order: a second run, and a clip computed alone, give the same bits.
//
//   audio_decode_kernel     one thread per frame, grid (frame blocks, clips): the frame's C samples assembled from aligned dword
//                           loads (a 24-bit or 3-channel frame is not dword-aligned; no load is ever misaligned), converted,
//                           summed in channel order and divided by C with a correctly rounded division
//   audio_resample_kernel   one workgroup of 256 per 256 consecutive outputs of one clip: the block's span of the input staged once
//                           in LDS (sized by the launcher from the ratio; positions outside the row are never read), the outputs
//                           dealt to the threads in the order of their table offset, then each thread walks its two wings over the
//                           interleaved (win, delta) table in global memory (262 KB, L2-resident), one 8-byte gather and one LDS
//                           read per tap; the fix_length tail is written as 0 by the same launch
#include "common.h"
#include "tcdiff_hip.h"

#define AU_THREADS 256
#define AU_NWIN (TC_AUDIO_TABLE)                          // 32769 entries of (win, delta)
#define AU_PREC TC_AUDIO_PRECISION                       // 512 table entries per zero crossing
#define AU_MAX_CLIPS 65535                               // the clip is a grid y coordinate

// ---- 1. decode + downmix ----------------------------------------------------------------------------------------------------------
// NB bytes (1 .. 4) at byte offset `at` of the clip, little-endian, from the one or two aligned dwords that hold them.  The second
// dword is read only when the value reaches into it, so no load goes past the dword of the clip's last byte.
template <int NB>
DEVINL uint32_t au_bytes(const uint32_t* __restrict__ words, size_t at) {
    const size_t w = at >> 2;
    const unsigned sh = ((unsigned)at & 3u) * 8u;
    uint64_t v = words[w];
    if (sh + 8u * NB > 32u) v |= (uint64_t)words[w + 1] << 32;
    v >>= sh;
    return NB == 4 ? (uint32_t)v : (uint32_t)v & ((1u << (8 * (NB & 3))) - 1u);
}

template <int FMT>
DEVINL float au_sample(const uint32_t* __restrict__ words, size_t at) {
    if (FMT == TC_AUDIO_U8) return (float)((int)au_bytes<1>(words, at) - 128) * 0.0078125f;
    if (FMT == TC_AUDIO_S16) return (float)(int16_t)au_bytes<2>(words, at) * 0x1p-15f;
    if (FMT == TC_AUDIO_S24) return (float)((int)(au_bytes<3>(words, at) << 8) >> 8) * 0x1p-23f;
    if (FMT == TC_AUDIO_S32) return (float)(int)au_bytes<4>(words, at) * 0x1p-31f;      // v_cvt_f32_i32: nearest even
    if (FMT == TC_AUDIO_F32) return __uint_as_float(au_bytes<4>(words, at));
    const uint64_t lo = au_bytes<4>(words, at), hi = au_bytes<4>(words, at + 4);
    return (float)__longlong_as_double((long long)(lo | (hi << 32)));                   // v_cvt_f32_f64: nearest even
}

template <int FMT>
__global__ __launch_bounds__(AU_THREADS) void audio_decode_kernel(const uint32_t* __restrict__ data, long row_words, int frames, int C,
                                                                  float* __restrict__ out) {
#pragma clang fp contract(off)      // the mean rounds after every addition, as numpy's
    constexpr int SB = FMT == TC_AUDIO_U8 ? 1 : FMT == TC_AUDIO_S16 ? 2 : FMT == TC_AUDIO_S24 ? 3 : FMT == TC_AUDIO_F64 ? 8 : 4;
    const long t = (long)blockIdx.x * AU_THREADS + threadIdx.x;
    if (t >= frames) return;
    const long b = blockIdx.y;
    const uint32_t* words = data + b * row_words;
    size_t at = (size_t)t * (size_t)(C * SB);
    float s = au_sample<FMT>(words, at);
    if (C > 1) {
        for (int c = 1; c < C; ++c) {
            at += SB;
            s = s + au_sample<FMT>(words, at);
        }
        s = __fdiv_rn(s, (float)C);
    }
    out[b * (long)frames + t] = s;
}

// ---- 2. resample ------------------------------------------------------------------------------------------------------------------
// grid (ceil(size / 256), B), dynamic LDS of `span` floats.  y: clip b at y + b * y_stride, n_orig floats.  Output t < n_out reads
// x[n - i], i < min(n + 1, (NWIN - off) / step) <= halo, and x[n + k + 1], k < min(n_orig - n - 1, (NWIN - off') / step) <= halo,
// with n = (int)(t inc) and halo = ceil(NWIN / step).  n does not decrease with t (a rounded product is monotone), so with
// n_lo = (int)(t0 inc) of the block's first output every position read lies in [n_lo - (halo - 1), n_hi + halo], n_hi the block's
// last n; the launcher sizes span = (int)(255 inc) + 3 + 2 halo >= n_hi - n_lo + 2 halo.  Positions outside [0, n_orig) are staged
// as 0 without a load and, by the two min() above, never enter a sum.
__global__ __launch_bounds__(AU_THREADS) void audio_resample_kernel(const float* __restrict__ y, long y_stride, int n_orig,
                                                                    const float2* __restrict__ table, double inc, double scale, int step,
                                                                    int halo, int span, int n_out, int size, float* __restrict__ out) {
#pragma clang fp contract(off)      // the index arithmetic is float64 with one rounding per operation, as the restatement's
    extern __shared__ float s_x[];
    __shared__ int s_key[AU_THREADS];
    __shared__ int s_perm[AU_THREADS];
    const int tid = threadIdx.x, t0 = blockIdx.x * AU_THREADS;
    const long b = blockIdx.y;
    const float* yb = y + b * y_stride;
    const int base = (int)((double)t0 * inc) - (halo - 1);
    for (int i = tid; i < span; i += AU_THREADS) {
        const long g = (long)base + i;
        s_x[i] = (g >= 0 && g < n_orig) ? yb[g] : 0.0f;
    }
    // The block's outputs are dealt to the threads in the order of their left-wing table offset, so that the 64 gathers a wave
    // issues for one tap fall into a quarter of the `step` table entries they would otherwise spread over (the right wing's
    // offsets, step - off, likewise): half the time or less at every rate measured (profiles/audio.txt).  Which thread computes an
    // output does not change its bits.  The rank is counted, not sorted: no atomics, ties in thread order.
    int t = t0 + tid;
    int key = 0x7fffffff;                                 // the fix_length tail goes last
    if (t < n_out) {
        const double tr = (double)t * inc;
        key = (int)(scale * (tr - (double)(int)tr) * (double)AU_PREC);
    }
    s_key[tid] = key;
    __syncthreads();
    int rank = 0;
    for (int j = 0; j < AU_THREADS; ++j) {
        const int kj = s_key[j];
        rank += (kj < key || (kj == key && j < tid)) ? 1 : 0;
    }
    s_perm[rank] = tid;
    __syncthreads();
    t = t0 + s_perm[tid];
    if (t >= size) return;
    float acc = 0.0f;
    if (t < n_out) {
        const double tr = (double)t * inc;
        const int n = (int)tr;
        double frac = scale * (tr - (double)n);
        double f = frac * (double)AU_PREC;
        int off = (int)f;
        float eta = (float)(f - (double)off);
        int cnt = min(n + 1, (AU_NWIN - off) / step);
        const float2* w = table + off;
        const float* x = s_x + (n - base);
#pragma unroll 4
        for (int i = 0; i < cnt; ++i) {
            const float2 wd = w[(long)i * step];
            acc = fmaf(fmaf(eta, wd.y, wd.x), x[-i], acc);
        }
        frac = scale - frac;
        f = frac * (double)AU_PREC;
        off = (int)f;
        eta = (float)(f - (double)off);
        cnt = min(n_orig - n - 1, (AU_NWIN - off) / step);
        w = table + off;
        x += 1;
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const float2 wd = w[(long)k * step];
            acc = fmaf(fmaf(eta, wd.y, wd.x), x[k], acc);
        }
    }
    out[b * (long)size + t] = acc;
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------
extern "C" int tcdiff_audio_decode(const void* data, long row_stride, int B, int frames, int channels, int fmt, float* out,
                                   hipStream_t stream) {
    if (!data || !out || B < 1 || frames < 1 || channels < 1 || fmt < TC_AUDIO_U8 || fmt > TC_AUDIO_F64) return TC_ERR_ARG;
    static const int bytes[6] = {1, 2, 3, 4, 4, 8};
    const long row = (long)frames * channels * bytes[fmt];
    if (row_stride < ((row + 3) & ~3L)) return TC_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(data) & 3u) || (row_stride & 3)) return TC_ERR_ALIGN;
    if (B > AU_MAX_CLIPS || channels > 65535) return TC_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(((long)frames + AU_THREADS - 1) / AU_THREADS), (unsigned)B), block(AU_THREADS);
    const uint32_t* words = static_cast<const uint32_t*>(data);
    const long row_words = row_stride >> 2;
#define AU_DECODE(F) \
    case F: hipLaunchKernelGGL(audio_decode_kernel<F>, grid, block, 0, stream, words, row_words, frames, channels, out); break;
    switch (fmt) {
        AU_DECODE(TC_AUDIO_U8)
        AU_DECODE(TC_AUDIO_S16)
        AU_DECODE(TC_AUDIO_S24)
        AU_DECODE(TC_AUDIO_S32)
        AU_DECODE(TC_AUDIO_F32)
        AU_DECODE(TC_AUDIO_F64)
    }
#undef AU_DECODE
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_audio_resample(const float* y, long y_stride, int B, int n, const float* table, double inc, double scale, int step,
                                     int n_out, int size, float* out, hipStream_t stream) {
    if (!y || !table || !out || y_stride < 0 || B < 1 || n < 1 || n_out < 1 || size < n_out) return TC_ERR_ARG;
    if (!(inc > 0.0) || !(scale > 0.0) || !(scale <= 1.0) || step < 1 || step > AU_PREC) return TC_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(table) & 7u) return TC_ERR_ALIGN;
    // every t < n_out must read inside the row: (n_out - 1) inc < n
    if (!((double)(n_out - 1) * inc < (double)n)) return TC_ERR_ARG;
    if (step < TC_AUDIO_MIN_STEP || B > AU_MAX_CLIPS || n > 0x7fffffff / 4 || size > 0x7fffffff / 4) return TC_ERR_UNSUPPORTED;
    const int halo = (AU_NWIN + step - 1) / step;
    const double reach = 255.0 * inc;
    if (!(reach < 1e8)) return TC_ERR_UNSUPPORTED;
    const int span = (int)reach + 3 + 2 * halo;
    if ((size_t)span * sizeof(float) > 64 * 1024) return TC_ERR_UNSUPPORTED;        // inc <= 8: 3069 floats
    hipLaunchKernelGGL(audio_resample_kernel, dim3((unsigned)((size + AU_THREADS - 1) / AU_THREADS), (unsigned)B), dim3(AU_THREADS),
                       (size_t)span * sizeof(float), stream, y, y_stride, n, reinterpret_cast<const float2*>(table), inc, scale, step, halo,
                       span, n_out, size, out);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
