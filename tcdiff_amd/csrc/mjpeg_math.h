// The per-sample and per-block arithmetic of the baseline JPEG encoder (include/tcdiff_mjpeg.h), shared by csrc/mjpeg.hip and by the
// host build tests/host/mjpeg_host.cpp, which tests/test_mjpeg_cpu.py holds to the numpy restatement's bytes.  Integers only.
#pragma once
#include "tcdiff_mjpeg.h"

#if defined(__HIPCC__)
#define TCJ_HD __host__ __device__ __forceinline__
#else
#define TCJ_HD static inline
#endif

// round(s_k cos((2 n + 1) k pi / 16) 2^14), the header's matrix
static constexpr int TCJ_M[8][8] = {{5793, 5793, 5793, 5793, 5793, 5793, 5793, 5793},     {8035, 6811, 4551, 1598, -1598, -4551, -6811, -8035},
                                    {7568, 3135, -3135, -7568, -7568, -3135, 3135, 7568}, {6811, -1598, -8035, -4551, 4551, 8035, 1598, -6811},
                                    {5793, -5793, -5793, 5793, 5793, -5793, -5793, 5793}, {4551, -8035, 1598, 6811, -6811, -1598, 8035, -4551},
                                    {3135, -7568, 7568, -3135, -3135, 7568, -7568, 3135}, {1598, -4551, 6811, -8035, 8035, -6811, 4551, -1598}};
static_assert(TC_MJPEG_DCT_BITS == 14 && TC_MJPEG_COEF_BITS == 2 * TC_MJPEG_DCT_BITS - 8, "pass 1 drops 8 of its 14 fractional bits");

// zigzag position -> natural index 8 v + u, and its inverse
static constexpr unsigned char TCJ_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                                 41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                                 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct tcj_perm {
    unsigned char v[64];
};
constexpr tcj_perm tcj_invert(const unsigned char* p) {
    tcj_perm r{};
    for (int i = 0; i < 64; ++i) r.v[p[i]] = (unsigned char)i;
    return r;
}
static constexpr tcj_perm TCJ_UNZIGZAG = tcj_invert(TCJ_ZIGZAG);          // natural index -> zigzag position

// Annex K.1 and K.2, natural order
static constexpr unsigned char TCJ_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40,  57,  69,  56, 14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3: counts per code length 1 .. 16, then the values in code order.  [0] luminance, [1] chrominance.
static constexpr unsigned char TCJ_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static constexpr unsigned char TCJ_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static constexpr unsigned char TCJ_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
static constexpr unsigned char TCJ_AC_VALS[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// symbol -> length << 16 | code, Annex C's assignment; 0 for a symbol the table lacks
struct tcj_codes {
    unsigned v[256];
};
constexpr tcj_codes tcj_make_codes(const unsigned char* bits, const unsigned char* vals) {
    tcj_codes t{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) t.v[vals[k++]] = (unsigned)len << 16 | code++;
        code <<= 1;
    }
    return t;
}
static constexpr tcj_codes TCJ_DC_CODES[2] = {tcj_make_codes(TCJ_DC_BITS[0], TCJ_DC_VALS), tcj_make_codes(TCJ_DC_BITS[1], TCJ_DC_VALS)};
static constexpr tcj_codes TCJ_AC_CODES[2] = {tcj_make_codes(TCJ_AC_BITS[0], TCJ_AC_VALS[0]), tcj_make_codes(TCJ_AC_BITS[1], TCJ_AC_VALS[1])};

// ---- colour ------------------------------------------------------------------------------------------------------------------------
TCJ_HD int tcj_clamp255(int v) { return v > 255 ? 255 : v; }          // the sums below are never negative
TCJ_HD int tcj_y(int r, int g, int b) { return tcj_clamp255((19595 * r + 38470 * g + 7471 * b + 32768) >> 16); }
TCJ_HD int tcj_cb(int r, int g, int b) { return tcj_clamp255((-11059 * r - 21709 * g + 32768 * b + 8388608 + 32768) >> 16); }
TCJ_HD int tcj_cr(int r, int g, int b) { return tcj_clamp255((32768 * r - 27439 * g - 5329 * b + 8388608 + 32768) >> 16); }
TCJ_HD int tcj_component(const unsigned char* p, int comp) {
    return comp == 0 ? tcj_y(p[0], p[1], p[2]) : comp == 1 ? tcj_cb(p[0], p[1], p[2]) : tcj_cr(p[0], p[1], p[2]);
}

// ---- the geometry of the scan ---------------------------------------------------------------------------------------------------------
TCJ_HD int tcj_mcu_side(int sub) { return sub == TC_MJPEG_420 ? 16 : 8; }
TCJ_HD int tcj_mcu_blocks(int sub) { return sub == TC_MJPEG_420 ? 6 : 3; }
TCJ_HD int tcj_block_component(int sub, int k) { return sub == TC_MJPEG_420 ? (k < 4 ? 0 : k - 3) : k; }
// the block of the same component that precedes block j of an interval, or -1 at the interval's start
TCJ_HD int tcj_pred_block(int sub, int j) {
    const int bpm = tcj_mcu_blocks(sub), m = j / bpm, k = j - m * bpm;
    if (sub == TC_MJPEG_420 && k > 0 && k < 4) return j - 1;
    if (m == 0) return -1;
    return sub == TC_MJPEG_420 && k == 0 ? j - 3 : j - bpm;
}

// sample (y, x) of block k of MCU (row, m) of one frame (its pixel (0, 0) at `frame`), level shifted; sH, sW in bytes
TCJ_HD int tcj_sample(const unsigned char* frame, long sH, long sW, int H, int W, int sub, int row, int m, int k, int y, int x) {
    const int comp = tcj_block_component(sub, k);
    if (sub == TC_MJPEG_420 && comp != 0) {
        int sum = 2;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                int py = row * 16 + 2 * y + dy, px = m * 16 + 2 * x + dx;
                py = py < H ? py : H - 1, px = px < W ? px : W - 1;
                sum += tcj_component(frame + py * sH + px * sW, comp);
            }
        return (sum >> 2) - 128;
    }
    int py, px;
    if (sub == TC_MJPEG_420)
        py = row * 16 + (k >> 1) * 8 + y, px = m * 16 + (k & 1) * 8 + x;
    else
        py = row * 8 + y, px = m * 8 + x;
    py = py < H ? py : H - 1, px = px < W ? px : W - 1;
    return tcj_component(frame + py * sH + px * sW, comp) - 128;
}

// ---- DCT and quantiser ---------------------------------------------------------------------------------------------------------------
// pass 1: t[y][u] from row y of the samples (s[0 .. 7]); pass 2: c[v][u] from column u of t (t[0], t[stride], ...)
TCJ_HD int tcj_dct_pass1(const int* s, int u) {
    int a = 0;
    for (int n = 0; n < 8; ++n) a += TCJ_M[u][n] * s[n];
    return (a + 128) >> 8;
}
TCJ_HD int tcj_dct_pass2(const int* t, int stride, int v) {
    int a = 0;
    for (int m = 0; m < 8; ++m) a += TCJ_M[v][m] * t[m * stride];
    return a;
}
TCJ_HD int tcj_quantise(int c, int t) {
    const int a = c < 0 ? -c : c, q = (a + (t << (TC_MJPEG_COEF_BITS - 1))) / (t << TC_MJPEG_COEF_BITS);
    return c < 0 ? -q : q;
}
TCJ_HD int tcj_clamp(int v, int lim) { return v > lim ? lim : v < -lim ? -lim : v; }
TCJ_HD void tcj_quant_tables(int quality, unsigned char qt[2][64]) {          // natural order
    const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int c = 0; c < 2; ++c)
        for (int i = 0; i < 64; ++i) {
            const int t = (TCJ_BASE[c][i] * scale + 50) / 100;
            qt[c][i] = (unsigned char)(t < 1 ? 1 : t > 255 ? 255 : t);
        }
}

// ---- symbols ---------------------------------------------------------------------------------------------------------------------------
TCJ_HD int tcj_category(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}
TCJ_HD unsigned tcj_amplitude(int v, int s) { return (unsigned)(v < 0 ? v + (1 << s) - 1 : v); }
TCJ_HD int tcj_dc_difference(int dc, int pred) { return tcj_clamp(dc - pred, 2047); }
// the bits of one AC value after `run` zeros (ZRLs included), and of the DC difference
TCJ_HD int tcj_ac_bits(int chroma, int run, int v) {
    const int s = tcj_category(v);
    return (run >> 4) * (int)(TCJ_AC_CODES[chroma].v[0xF0] >> 16) + (int)(TCJ_AC_CODES[chroma].v[(run & 15) << 4 | s] >> 16) + s;
}
TCJ_HD int tcj_dc_bits(int chroma, int d) {
    const int s = tcj_category(d);
    return (int)(TCJ_DC_CODES[chroma].v[s] >> 16) + s;
}
// every code of a block in stream order: put(bits, length), length <= 27.  zz: the quantised, clamped coefficients in zigzag order
template <class Put>
TCJ_HD void tcj_block_symbols(const short* zz, int dcdiff, int chroma, Put& put) {
    int s = tcj_category(dcdiff);
    unsigned h = TCJ_DC_CODES[chroma].v[s];
    put((h & 0xFFFF) << s | tcj_amplitude(dcdiff, s), (int)(h >> 16) + s);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = zz[k];
        if (v == 0) {
            ++run;
            continue;
        }
        for (; run >= 16; run -= 16) put(TCJ_AC_CODES[chroma].v[0xF0] & 0xFFFF, (int)(TCJ_AC_CODES[chroma].v[0xF0] >> 16));
        s = tcj_category(v);
        h = TCJ_AC_CODES[chroma].v[run << 4 | s];
        put((h & 0xFFFF) << s | tcj_amplitude(v, s), (int)(h >> 16) + s);
        run = 0;
    }
    if (run) put(TCJ_AC_CODES[chroma].v[0] & 0xFFFF, (int)(TCJ_AC_CODES[chroma].v[0] >> 16));
}

// ---- the segments before the entropy data -------------------------------------------------------------------------------------------
struct tcj_header {
    unsigned char b[TC_MJPEG_HEADER_BYTES];
};
static inline void tcj_make_header(tcj_header* hd, int W, int H, int sub, const unsigned char qt[2][64]) {
    unsigned char* p = hd->b;
    const unsigned char app0[] = {0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (unsigned char c : app0) *p++ = c;
    *p++ = 0xFF, *p++ = 0xDB, *p++ = 0, *p++ = 132;
    for (int c = 0; c < 2; ++c) {
        *p++ = (unsigned char)c;
        for (int i = 0; i < 64; ++i) *p++ = qt[c][TCJ_ZIGZAG[i]];
    }
    const unsigned char sof[] = {0xFF, 0xC0, 0, 17, 8, (unsigned char)(H >> 8), (unsigned char)H, (unsigned char)(W >> 8), (unsigned char)W, 3,
                                 1, (unsigned char)(sub == TC_MJPEG_420 ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1};
    for (unsigned char c : sof) *p++ = c;
    for (int c = 0; c < 2; ++c) {
        *p++ = 0xFF, *p++ = 0xC4, *p++ = 0, *p++ = 31, *p++ = (unsigned char)c;
        for (int i = 0; i < 16; ++i) *p++ = TCJ_DC_BITS[c][i];
        for (int i = 0; i < 12; ++i) *p++ = TCJ_DC_VALS[i];
        *p++ = 0xFF, *p++ = 0xC4, *p++ = 0, *p++ = 181, *p++ = (unsigned char)(0x10 | c);
        for (int i = 0; i < 16; ++i) *p++ = TCJ_AC_BITS[c][i];
        for (int i = 0; i < 162; ++i) *p++ = TCJ_AC_VALS[c][i];
    }
    const int side = tcj_mcu_side(sub), ri = (W + side - 1) / side;
    const unsigned char tail[] = {0xFF, 0xDD, 0, 4, (unsigned char)(ri >> 8), (unsigned char)ri, 0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0};
    for (unsigned char c : tail) *p++ = c;
}
static_assert(20 + 134 + 19 + 2 * (33 + 183) + 20 == TC_MJPEG_HEADER_BYTES, "the header's segments");
