// Baseline JPEG frames encoded on the device, gfx950: the video stream of a Motion-JPEG AVI.  The bytes are defined in
// include/tcdiff_mjpeg.h; tests/mjpeg_ref.py restates them in numpy integers; the arithmetic is csrc/mjpeg_math.h, which the tests
// also build for the host.  No floating point anywhere, no atomics on global memory, plain C++ and vector stores.
//
// mjpeg_blocks_kernel: one wave per 8 x 8 block, four blocks per workgroup.  Lane (y, x) gathers its sample through the strides
//   with the edge clamp (a 4:2:0 chroma lane gathers its 2 x 2), the two matrix passes go through LDS, the lane quantises
//   coefficient (v, u) = (y, x) and drops it at its zigzag position.  The block's AC bit length comes from one ballot: a non-zero
//   lane finds the previous non-zero lane in the mask, which is its run.
// mjpeg_count_kernel: one workgroup per restart interval = (frame, MCU row); a thread per block, looping when the interval holds
//   more blocks than the workgroup has threads.  Adds the DC difference's bits, scans, leaves each block's bit offset where its
//   length was, then packs the interval window by window in LDS (mjpeg_pack_window) and counts the 0xFF bytes.
// mjpeg_offsets_kernel: one workgroup, a chunked exclusive int64 scan over the intervals in index order.
// mjpeg_write_kernel: one workgroup per interval: packs each window again, scans the 0xFF counts of the threads' byte runs, stuffs
//   into a staging buffer in LDS and copies that to its final place with dword stores between the unaligned ends.
//
// mjpeg_pack_window: every thread walks the symbols of its block if the block's bits meet the window, and ORs each code into the
// window's big-endian dwords (LDS atomics: OR commutes, so the bytes do not depend on the order); a code is clipped to the window
// dword by dword, so a block that straddles two windows is simply walked in both.
#include "common.h"
#include "mjpeg_math.h"

#define MJ_THREADS TC_MJPEG_THREADS
#define MJ_WAVES (MJ_THREADS / 64)
#define MJ_WIN_DWORDS (TC_MJPEG_WINDOW / 4)
static_assert(MJ_THREADS % 64 == 0 && TC_MJPEG_WINDOW % 4 == 0, "whole waves, whole dwords");

struct mj_geom {
    int N, H, W, sub;
    int R, M, bpm, nb;          // MCU rows per frame, MCUs per row, blocks per MCU, blocks per interval
    long sN, sH, sW;
    long nint, nblocks;         // N R,  N R nb
};
struct mj_qt {
    unsigned char t[2][64];
};
struct mj_ws {
    long* ioff;                 // [nint] the interval's first byte in data
    int* ibytes;                // [nint] its bytes after stuffing
    int* ibits;                 // [nint] its bits before padding
    int* bits;                  // [nblocks] the block's AC bits after launch 1, its bit offset in the interval after launch 2
    short* coef;                // [nblocks][64] zigzag order
};

template <class T>
DEVINL T mj_scan_excl(T v, T* lds, int nwaves, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T n = __shfl_up(inc, o);
        if (lane >= o) inc += n;
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < nwaves; ++w) {
        const T x = lds[w];
        if (w < wave) base += x;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

__global__ __launch_bounds__(256) void mjpeg_blocks_kernel(const unsigned char* __restrict__ frames, mj_geom G, mj_qt Q,
                                                           short* __restrict__ coef, int* __restrict__ bits) {
    __shared__ int s_s[4][64], s_t[4][64];
    __shared__ short s_z[4][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, y = lane >> 3, x = lane & 7;
    const long g = (long)blockIdx.x * 4 + wave;
    const bool live = g < G.nblocks;                          // one answer per wave
    const long per = (long)G.R * G.nb, f = live ? g / per : 0, r = live ? g - f * per : 0;
    const int row = (int)(r / G.nb), j = (int)(r - (long)row * G.nb), m = j / G.bpm, k = j - m * G.bpm;
    const int chroma = tcj_block_component(G.sub, k) != 0;
    s_s[wave][lane] = live ? tcj_sample(frames + f * G.sN, G.sH, G.sW, G.H, G.W, G.sub, row, m, k, y, x) : 0;
    __syncthreads();
    s_t[wave][lane] = tcj_dct_pass1(&s_s[wave][y * 8], x);
    __syncthreads();
    int q = tcj_quantise(tcj_dct_pass2(&s_t[wave][x], 8, y), Q.t[chroma][lane]);
    if (lane) q = tcj_clamp(q, 1023);
    s_z[wave][TCJ_UNZIGZAG.v[lane]] = (short)q;
    __syncthreads();
    const int z = s_z[wave][lane];
    const unsigned long long mask = __ballot(lane > 0 && z != 0);
    int b = 0;
    if (lane > 0 && z != 0) {
        const unsigned long long prev = mask & ((1ull << lane) - 1);
        const int p = prev ? 63 - __clzll((long long)prev) : 0;
        b = tcj_ac_bits(chroma, lane - 1 - p, z);
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) b += __shfl_xor(b, o);
    if (!live) return;
    if (!(mask >> 63)) b += (int)(TCJ_AC_CODES[chroma].v[0] >> 16);
    coef[g * 64 + lane] = (short)z;
    if (lane == 0) bits[g] = b;
}

struct mj_putter {
    unsigned* win;
    long w0bits, pos;
    int ndw;
    DEVINL void operator()(unsigned code, int len) {
        const long rel = pos - w0bits, d = rel >> 5;          // floor: a code that starts before the window keeps its tail
        const int sh = (int)(rel & 31);
        pos += len;
        const unsigned long long v = (unsigned long long)code << (64 - len - sh);          // len + sh <= 27 + 31
        const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
        if (hi && d >= 0 && d < ndw) atomicOr(&win[d], hi);
        if (lo && d + 1 >= 0 && d + 1 < ndw) atomicOr(&win[d + 1], lo);
    }
};

// bytes [w0, w0 + nwb) of interval i, before stuffing, into win (big-endian dwords); the interval's 1-padding included
DEVINL void mjpeg_pack_window(const mj_geom& G, const mj_ws& ws, long gb, int tb, int w0, int nwb, unsigned* win) {
    const int ndw = (nwb + 3) >> 2;
    for (int d = threadIdx.x; d < ndw; d += MJ_THREADS) win[d] = 0;
    __syncthreads();
    const long lo = (long)w0 * 8, hi = lo + (long)nwb * 8;
    for (int c0 = 0; c0 < G.nb; c0 += MJ_THREADS) {
        const int j = c0 + threadIdx.x;
        if (j >= G.nb) break;
        const long off = ws.bits[gb + j], end = j + 1 < G.nb ? ws.bits[gb + j + 1] : tb;
        if (end <= lo) continue;                               // the padding shares its byte with the last block's last bit
        if (off >= hi) break;                                  // offsets ascend with j
        const short* zz = ws.coef + (gb + j) * 64;
        const int pj = tcj_pred_block(G.sub, j), k = j % G.bpm;
        const int d = tcj_dc_difference(zz[0], pj < 0 ? 0 : ws.coef[(gb + pj) * 64]);
        mj_putter put{win, lo, off, ndw};
        tcj_block_symbols(zz, d, tcj_block_component(G.sub, k) != 0, put);
        if (j + 1 == G.nb && (tb & 7)) put((1u << (8 - (tb & 7))) - 1, 8 - (tb & 7));
    }
    __syncthreads();
}

DEVINL unsigned mj_byte(const unsigned* win, int b) { return (win[b >> 2] >> (24 - 8 * (b & 3))) & 0xFFu; }

__global__ __launch_bounds__(MJ_THREADS) void mjpeg_count_kernel(mj_geom G, mj_ws ws) {
    __shared__ unsigned win[MJ_WIN_DWORDS];
    __shared__ int s_scan[MJ_WAVES];
    const long i = blockIdx.x, gb = i * G.nb;
    int carry = 0;
    for (int c0 = 0; c0 < G.nb; c0 += MJ_THREADS) {
        const int j = c0 + threadIdx.x;
        int len = 0;
        if (j < G.nb) {
            const int pj = tcj_pred_block(G.sub, j), k = j % G.bpm;
            const int d = tcj_dc_difference(ws.coef[(gb + j) * 64], pj < 0 ? 0 : ws.coef[(gb + pj) * 64]);
            len = ws.bits[gb + j] + tcj_dc_bits(tcj_block_component(G.sub, k) != 0, d);
        }
        int tot;
        const int ex = mj_scan_excl(len, s_scan, MJ_WAVES, &tot);
        if (j < G.nb) ws.bits[gb + j] = carry + ex;
        carry += tot;
    }
    __syncthreads();                                           // the offsets are read by other threads from here on
    const int tb = carry, nbytes = (tb + 7) >> 3;
    int ff = 0;
    for (int w0 = 0; w0 < nbytes; w0 += TC_MJPEG_WINDOW) {
        const int nwb = min(TC_MJPEG_WINDOW, nbytes - w0);
        mjpeg_pack_window(G, ws, gb, tb, w0, nwb, win);
        for (int b = threadIdx.x; b < nwb; b += MJ_THREADS) ff += mj_byte(win, b) == 0xFFu;
        __syncthreads();
    }
    int tot;
    mj_scan_excl(ff, s_scan, MJ_WAVES, &tot);
    if (threadIdx.x == 0) ws.ibits[i] = tb, ws.ibytes[i] = nbytes + tot;
}

__global__ __launch_bounds__(1024) void mjpeg_offsets_kernel(mj_ws ws, long nint, int R, long* __restrict__ offsets) {
    __shared__ long s_scan[16];
    long carry = 0;
    for (long c0 = 0; c0 < nint; c0 += 1024) {
        const long i = c0 + threadIdx.x;
        const bool first = i < nint && i % R == 0;
        const long v = i < nint ? (long)ws.ibytes[i] + 2 + (first ? TC_MJPEG_HEADER_BYTES : 0) : 0;
        long tot;
        const long pos = carry + mj_scan_excl(v, s_scan, 16, &tot);
        if (first) offsets[i / R] = pos;
        if (i < nint) ws.ioff[i] = pos + (first ? TC_MJPEG_HEADER_BYTES : 0);
        carry += tot;
    }
    if (threadIdx.x == 0) offsets[nint / R] = carry;
}

__global__ __launch_bounds__(MJ_THREADS) void mjpeg_write_kernel(mj_geom G, mj_ws ws, tcj_header hd, unsigned char* __restrict__ data,
                                                                 long data_bytes) {
    __shared__ unsigned win[MJ_WIN_DWORDS];
    __shared__ unsigned char stage[2 * TC_MJPEG_WINDOW];
    __shared__ int s_scan[MJ_WAVES];
    const long i = blockIdx.x, gb = i * G.nb;
    const int row = (int)(i % G.R), tb = ws.ibits[i], nbytes = (tb + 7) >> 3;
    const int lead = row == 0 ? TC_MJPEG_HEADER_BYTES : 0;
    long out = ws.ioff[i];
    if (out < lead || ws.ibytes[i] < nbytes || out + ws.ibytes[i] + 2 > data_bytes) return;      // nothing outside data, whatever the workspace holds
    long room = ws.ibytes[i];
    if (row == 0)
        for (int k = threadIdx.x; k < TC_MJPEG_HEADER_BYTES; k += MJ_THREADS) data[out - lead + k] = hd.b[k];
    for (int w0 = 0; w0 < nbytes; w0 += TC_MJPEG_WINDOW) {
        const int nwb = min(TC_MJPEG_WINDOW, nbytes - w0);
        mjpeg_pack_window(G, ws, gb, tb, w0, nwb, win);
        const int seg = (nwb + MJ_THREADS - 1) / MJ_THREADS, b0 = min((int)threadIdx.x * seg, nwb), b1 = min(b0 + seg, nwb);
        int cnt = 0;
        for (int b = b0; b < b1; ++b) cnt += mj_byte(win, b) == 0xFFu;
        int tot;
        int o = b0 + mj_scan_excl(cnt, s_scan, MJ_WAVES, &tot);
        for (int b = b0; b < b1; ++b) {
            const unsigned v = mj_byte(win, b);
            stage[o++] = (unsigned char)v;
            if (v == 0xFFu) stage[o++] = 0;
        }
        __syncthreads();
        const int n = nwb + tot;
        if (n > room) return;                                  // uniform; a workspace that is not launch 2's
        unsigned char* dst = data + out;
        const int head = min(n, (int)((4 - ((uintptr_t)dst & 3)) & 3)), ndw = (n - head) >> 2, tail = head + 4 * ndw;
        for (int k = threadIdx.x; k < head; k += MJ_THREADS) dst[k] = stage[k];
        for (int k = threadIdx.x; k < ndw; k += MJ_THREADS) {
            const unsigned char* s = stage + head + 4 * k;
            reinterpret_cast<unsigned*>(dst + head)[k] = (unsigned)s[0] | (unsigned)s[1] << 8 | (unsigned)s[2] << 16 | (unsigned)s[3] << 24;
        }
        for (int k = tail + threadIdx.x; k < n; k += MJ_THREADS) dst[k] = stage[k];
        out += n, room -= n;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        data[out] = 0xFF;
        data[out + 1] = (unsigned char)(row + 1 < G.R ? 0xD0 + (row & 7) : 0xD9);
    }
}

// the checks every launcher shares, in the header's order; fills G (strides excepted)
static int mj_geometry(int N, int H, int W, int quality, int sub, mj_geom* G) {
    if (N < 1 || W < 1 || H < 1 || quality < 1 || quality > 100 || (sub != TC_MJPEG_444 && sub != TC_MJPEG_420)) return TC_ERR_ARG;
    if (W > TC_MJPEG_MAX_SIDE || H > TC_MJPEG_MAX_SIDE) return TC_ERR_UNSUPPORTED;
    const int side = tcj_mcu_side(sub);
    G->N = N, G->H = H, G->W = W, G->sub = sub;
    G->R = (H + side - 1) / side, G->M = (W + side - 1) / side, G->bpm = tcj_mcu_blocks(sub), G->nb = G->M * G->bpm;
    G->nint = (long)N * G->R;
    G->nblocks = G->nint * G->nb;                              // N R <= 2^31 * 2^13, nb <= 2^16: no overflow of a long
    if (G->nint > 0x7fffffffL || G->nblocks > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    return TC_OK;
}
static long mj_workspace_bytes(const mj_geom& G) { return 16 * G.nint + 132 * G.nblocks; }
static mj_ws mj_carve(void* workspace, const mj_geom& G) {
    mj_ws ws;
    char* p = static_cast<char*>(workspace);
    ws.ioff = reinterpret_cast<long*>(p), p += 8 * G.nint;
    ws.ibytes = reinterpret_cast<int*>(p), p += 4 * G.nint;
    ws.ibits = reinterpret_cast<int*>(p), p += 4 * G.nint;
    ws.bits = reinterpret_cast<int*>(p), p += 4 * G.nblocks;
    ws.coef = reinterpret_cast<short*>(p);
    return ws;
}

extern "C" int tcj_mjpeg_workspace(int N, int H, int W, int subsampling, long* bytes) {
    if (!bytes) return TC_ERR_ARG;
    mj_geom G;
    const int rc = mj_geometry(N, H, W, 50, subsampling, &G);
    if (rc != TC_OK) return rc;
    *bytes = mj_workspace_bytes(G);
    return TC_OK;
}

extern "C" int tcj_mjpeg_plan(const unsigned char* frames, const long* strides, int N, int H, int W, int quality, int subsampling,
                              void* workspace, long workspace_bytes, long* offsets, hipStream_t stream) {
    if (!frames || !strides || !workspace || !offsets) return TC_ERR_ARG;
    mj_geom G;
    int rc = mj_geometry(N, H, W, quality, subsampling, &G);
    if (rc == TC_ERR_ARG) return rc;
    if (strides[0] < 0 || strides[1] < 0 || strides[2] < 0) return TC_ERR_ARG;
    if (rc != TC_OK) return rc;
    if (workspace_bytes < mj_workspace_bytes(G)) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 != 0) return TC_ERR_ALIGN;
    G.sN = strides[0], G.sH = strides[1], G.sW = strides[2];
    const mj_ws ws = mj_carve(workspace, G);
    mj_qt Q;
    tcj_quant_tables(quality, Q.t);
    hipLaunchKernelGGL(mjpeg_blocks_kernel, dim3((unsigned)((G.nblocks + 3) / 4)), dim3(256), 0, stream, frames, G, Q, ws.coef, ws.bits);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(mjpeg_count_kernel, dim3((unsigned)G.nint), dim3(MJ_THREADS), 0, stream, G, ws);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(mjpeg_offsets_kernel, dim3(1), dim3(1024), 0, stream, ws, G.nint, G.R, offsets);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcj_mjpeg_write(int N, int H, int W, int quality, int subsampling, const void* workspace, long workspace_bytes,
                               unsigned char* data, long data_bytes, hipStream_t stream) {
    if (!workspace || !data) return TC_ERR_ARG;
    mj_geom G;
    const int rc = mj_geometry(N, H, W, quality, subsampling, &G);
    if (rc != TC_OK) return rc;
    if (workspace_bytes < mj_workspace_bytes(G) || data_bytes < 0) return TC_ERR_ARG;
    if ((uintptr_t)workspace % 8 != 0) return TC_ERR_ALIGN;
    G.sN = G.sH = G.sW = 0;
    const mj_ws ws = mj_carve(const_cast<void*>(workspace), G);
    mj_qt Q;
    tcj_quant_tables(quality, Q.t);
    tcj_header hd;
    tcj_make_header(&hd, W, H, subsampling, Q.t);
    hipLaunchKernelGGL(mjpeg_write_kernel, dim3((unsigned)G.nint), dim3(MJ_THREADS), 0, stream, G, ws, hd, data, data_bytes);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
