// Shared pieces of the Dance-Beat Navigator kernels (navigator.hip: inference and the train-mode forward; navigator_train.hip: the
// backward pass): the packed parameter layouts, the 16-row MFMA products and the 16-row LayerNorm.
#pragma once
#include "common.h"
#include "tcdiff_hip.h"

namespace {

constexpr int NV_W = 128;        // transformer width
constexpr int NV_LD = NV_W + 4;  // LDS row stride of a 128-wide block: rows shift by four banks
constexpr int NV_R = 16;         // token rows per workgroup
constexpr int NV_HID = 512;
constexpr int NV_LSTM_S = 2;     // sequences per LSTM workgroup

// packed per-block parameters (floats): tcdiff_amd/navigator.py writes this order
constexpr int BK_LN1G = 0, BK_LN1B = 128, BK_WQ = 256, BK_BQ = BK_WQ + 16384, BK_WK = BK_BQ + 128, BK_BK = BK_WK + 16384,
              BK_WV = BK_BK + 128, BK_BV = BK_WV + 16384, BK_WP = BK_BV + 128, BK_BP = BK_WP + 16384, BK_LN2G = BK_BP + 128,
              BK_LN2B = BK_LN2G + 128, BK_W1 = BK_LN2B + 128, BK_B1 = BK_W1 + 65536, BK_W2 = BK_B1 + 512, BK_B2 = BK_W2 + 65536,
              BK_SIZE = BK_B2 + 128;
// packed Decoder: 192 -> 128 -> 128 -> 64 -> 2 (the last weight padded to 16 rows)
constexpr int DC_W1 = 0, DC_B1 = DC_W1 + 128 * 192, DC_W2 = DC_B1 + 128, DC_B2 = DC_W2 + 16384, DC_W3 = DC_B2 + 128,
              DC_B3 = DC_W3 + 64 * 128, DC_W4 = DC_B3 + 64, DC_B4 = DC_W4 + 16 * 64, DC_SIZE = DC_B4 + 16;
// packed music front: 876 (880) -> 438 (448) -> 438 (448) -> 64, then cond_emb 64 -> 64
constexpr int MU_K0 = 880, MU_N = 448;
constexpr int MU_W1 = 0, MU_B1 = MU_W1 + MU_N * MU_K0, MU_W2 = MU_B1 + MU_N, MU_B2 = MU_W2 + MU_N * MU_N, MU_W3 = MU_B2 + MU_N,
              MU_B3 = MU_W3 + 64 * MU_N, MU_WC = MU_B3 + 64, MU_BC = MU_WC + 64 * 64, MU_SIZE = MU_BC + 64;
static_assert(BK_SIZE == 198272 && DC_SIZE == 50512 && MU_SIZE == 628736, "tcdiff_amd/navigator.py packs these sizes");

DEVINL float leaky(float v) { return v > 0.f ? v : 0.01f * v; }
DEVINL float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }
DEVINL float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// out(row, col, value) for the 16 x (16 ntiles) product of As[16][lda] (LDS) and W[16 ntiles][ldw] (global); K % 16 == 0.
// Wave wv of nw owns pairs of column tiles (two independent accumulator chains).
template <class Epi>
DEVINL void nav_mm16(const float* As, int lda, const float* __restrict__ W, int ldw, int ntiles, int K, int wv, int nw, Epi epi) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const float* a = As + r * lda + 4 * g;
    for (int p = wv; 2 * p < ntiles; p += nw) {
        const int t0 = 2 * p;
        const bool two = t0 + 1 < ntiles;
        const float* w0 = W + (long)(t0 * 16 + r) * ldw + 4 * g;
        const float* w1 = two ? w0 + (long)16 * ldw : w0;
        f32x4_t c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll 4
        for (int k = 0; k < K; k += 16) {
            const f32x4_t av = *reinterpret_cast<const f32x4_t*>(a + k);
            const f32x4_t b0 = *reinterpret_cast<const f32x4_t*>(w0 + k);
            const f32x4_t b1 = *reinterpret_cast<const f32x4_t*>(w1 + k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b0[j], c0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], b1[j], c1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            epi(4 * g + i, t0 * 16 + r, c0[i]);
            if (two) epi(4 * g + i, t0 * 16 + 16 + r, c1[i]);
        }
    }
}

// nn.LayerNorm(128) of the 16 rows of Xs into Ns (biased variance, eps 1e-5): a wave takes four rows, a lane two columns
DEVINL void nav_ln16(const float* Xs, float* Ns, const float* __restrict__ gam, const float* __restrict__ bet) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int r = wv * 4; r < wv * 4 + 4; ++r) {
        const float x0 = Xs[r * NV_LD + lane], x1 = Xs[r * NV_LD + 64 + lane];
        float s = x0 + x1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s * (1.f / NV_W);
        const float d0 = x0 - mean, d1 = x1 - mean;
        float q = d0 * d0 + d1 * d1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
        const float rstd = 1.f / sqrtf(q * (1.f / NV_W) + 1e-5f);
        Ns[r * NV_LD + lane] = d0 * rstd * gam[lane] + bet[lane];
        Ns[r * NV_LD + 64 + lane] = d1 * rstd * gam[64 + lane] + bet[64 + lane];
    }
}

// ---- the same product against W^T: out[r][c] = sum_n As[r][n] W[n][c], W [Kred][ldw] as nn.Linear stores it ([out][in]) -- the
// input gradient of a linear layer without a transposed copy.  Lane (r, g) fetches W[n0 + 4 g + j][c0 + r]: 16 lanes read 64
// consecutive bytes.  nav_mm16t_acc adds one 16-column tile's product to `acc` (lane holds rows 4 g .. 4 g + 3 of column c0 + r),
// so two products that land on the same tile chain their accumulators.  Kred % 16 == 0; columns c0 + r >= ncol read as zero.
DEVINL void nav_mm16t_acc(f32x4_t& acc, const float* As, int lda, const float* __restrict__ W, int ldw, int c0, int ncol, int Kred) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const float* a = As + r * lda + 4 * g;
    const bool ok = c0 + r < ncol;
    const float* w = W + (long)(4 * g) * ldw + (ok ? c0 + r : 0);
#pragma unroll 2
    for (int n = 0; n < Kred; n += 16) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(a + n);
        float bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bv[j] = ok ? w[(long)(n + j) * ldw] : 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
    }
}
// every 16-column tile of the ntiles, one tile per wave and turn
template <class Epi>
DEVINL void nav_mm16t(const float* As, int lda, const float* __restrict__ W, int ldw, int ntiles, int Kred, int wv, int nw, Epi epi) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    for (int t = wv; t < ntiles; t += nw) {
        f32x4_t c = {0.f, 0.f, 0.f, 0.f};
        nav_mm16t_acc(c, As, lda, W, ldw, t * 16, ntiles * 16, Kred);
#pragma unroll
        for (int i = 0; i < 4; ++i) epi(4 * g + i, t * 16 + r, c[i]);
    }
}

// one 16-column tile of nav_mm16 added to `acc`: acc(rows 4 g .. 4 g + 3, column c0 + r) += As[16][K] W[c0 .. c0 + 15][K]^T
DEVINL void nav_mm16_acc(f32x4_t& acc, const float* As, int lda, const float* __restrict__ W, int ldw, int c0, int K) {
    const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const float* a = As + r * lda + 4 * g;
    const float* w = W + (long)(c0 + r) * ldw + 4 * g;
#pragma unroll 4
    for (int k = 0; k < K; k += 16) {
        const f32x4_t av = *reinterpret_cast<const f32x4_t*>(a + k);
        const f32x4_t bv = *reinterpret_cast<const f32x4_t*>(w + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
    }
}

}  // namespace
