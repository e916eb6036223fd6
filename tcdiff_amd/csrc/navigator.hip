// The Dance-Beat Navigator (TrajDecoder/model/traj_model.py:125-200) and its sliding-window rollout (TCDiff.py:526-547) in exact
// fp32: v_mfma_f32_16x16x4_f32 for every product, VALU for the LSTM gates, LayerNorm, softmax and the activations.
//
//   nav_music_kernel  once per rollout: music_projection (876 -> 438 -> 438 -> 64, LeakyReLU) and cond_emb of EVERY frame pair of the
//                     song.  A window's pairs are rows [start/2, start/2 + window + step) of the two tables.
//   nav_lstm_kernel   one launch per window: the 3-layer LSTM(2 -> 64).  The module is built without batch_first, so the recurrence
//                     runs over the CLIP index and the dn*seq positions are independent sequences: a workgroup owns two of them,
//                     keeps one gate row of one layer per thread (768 threads, the 128 weights of a row in registers) and walks the
//                     three layers as a wavefront (layer l handles clip tick - l).  Writes h + PositionalEncoding row.
//   nav_block_kernel  one launch per transformer block, a block of 16 token rows (128 wide) resident in LDS: unmasked head-32
//                     attention over the clip's K / V (one wave per head, scores in LDS), proj + residual, LN2, MLP with erf-GELU,
//                     residual, then the NEXT block's LN1 + Q / K / V (written for the next launch, ping-pong).  layer = -1 is the
//                     front launch (gathers [cond_emb rows | LSTM rows], block 0's LN1 + Q / K / V); the last block's epilogue is
//                     the four-linear Decoder on [x | prediction-side music rows], which writes the window's trajectory and appends
//                     its `step` tail to the rollout.
// So a window is trans_layer + 2 launches in one stream, with no host work between them.
//
// Every product goes through nav_mm16: a 16-row LDS block times W[N][K]^T with W read from global memory in 16-byte pieces along K.
// Lane l (r = l & 15, g = l >> 4) fetches k = k0 + 4 g .. 4 g + 3 of row r (A) / column r (W) and MFMA j of the four pairs element j
// of both: the K order inside a dot product is permuted the same way for A and W, which only changes the fp32 summation order.  An
// output row depends on its own input row only, never on which rows share the block or the launch.
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

// ---- LSTM over the clip axis ---------------------------------------------------------------------------------------------------
// x [b][T][2]; wpk [3][128][256] (k < 64: weight_ih column k, zero beyond the layer's input width; k >= 64: weight_hh column k - 64;
// 256 gate rows in PyTorch's order i, f, g, o); bih / bhh [3][256]; pe [>= T][64]; out [b][T][64] = h + pe; raw (or NULL) = h.
__global__ __launch_bounds__(768) void nav_lstm_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                       const float* __restrict__ bih, const float* __restrict__ bhh,
                                                       const float* __restrict__ pe, float* __restrict__ out,
                                                       float* __restrict__ raw, int b, int T) {
    __shared__ __attribute__((aligned(16))) float hbuf[3][NV_LSTM_S][64];
    __shared__ float gates[3][NV_LSTM_S][256];
    const int l = threadIdx.x >> 8, j = threadIdx.x & 255;
    const int pos0 = blockIdx.x * NV_LSTM_S;
    float w[128];
#pragma unroll
    for (int k = 0; k < 128; ++k) w[k] = wpk[(l * 128 + k) * 256 + j];
    const float bi = bih[l * 256 + j], bh = bhh[l * 256 + j];
    if (j < NV_LSTM_S * 64) hbuf[l][j >> 6][j & 63] = 0.f;
    float c = 0.f;                            // cell state of (sequence j >> 6, unit j & 63) in threads j < 128 of each layer
    float x0[NV_LSTM_S], x1[NV_LSTM_S];       // layer 0: the inputs of the coming tick
#pragma unroll
    for (int s = 0; s < NV_LSTM_S; ++s) {
        const bool ok = l == 0 && pos0 + s < T;
        x0[s] = ok ? x[(long)(pos0 + s) * 2] : 0.f;
        x1[s] = ok ? x[(long)(pos0 + s) * 2 + 1] : 0.f;
    }
    __syncthreads();
    for (int tick = 0; tick < b + 2; ++tick) {
        const int t = tick - l;
        const bool active = t >= 0 && t < b;
        if (active) {
#pragma unroll
            for (int s = 0; s < NV_LSTM_S; ++s) {
                float ai = 0.f, ah = 0.f;
                if (l == 0) {
                    ai = w[0] * x0[s] + w[1] * x1[s];
                } else {
                    const f32x4_t* hp = reinterpret_cast<const f32x4_t*>(hbuf[l - 1][s]);
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const f32x4_t v = hp[k];
                        ai = fmaf(w[4 * k], v[0], ai);
                        ai = fmaf(w[4 * k + 1], v[1], ai);
                        ai = fmaf(w[4 * k + 2], v[2], ai);
                        ai = fmaf(w[4 * k + 3], v[3], ai);
                    }
                }
                const f32x4_t* hh = reinterpret_cast<const f32x4_t*>(hbuf[l][s]);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const f32x4_t v = hh[k];
                    ah = fmaf(w[64 + 4 * k], v[0], ah);
                    ah = fmaf(w[64 + 4 * k + 1], v[1], ah);
                    ah = fmaf(w[64 + 4 * k + 2], v[2], ah);
                    ah = fmaf(w[64 + 4 * k + 3], v[3], ah);
                }
                gates[l][s][j] = (ai + bi) + (ah + bh);
            }
            if (l == 0 && t + 1 < b) {
#pragma unroll
                for (int s = 0; s < NV_LSTM_S; ++s)
                    if (pos0 + s < T) {
                        x0[s] = x[((long)(t + 1) * T + pos0 + s) * 2];
                        x1[s] = x[((long)(t + 1) * T + pos0 + s) * 2 + 1];
                    }
            }
        }
        __syncthreads();
        if (active && j < NV_LSTM_S * 64) {
            const int s = j >> 6, u = j & 63;
            const float* gt = gates[l][s];
            const float gi = sigmoidf(gt[u]), gf = sigmoidf(gt[64 + u]), gg = tanhf(gt[128 + u]), go = sigmoidf(gt[192 + u]);
            c = gf * c + gi * gg;
            const float h = go * tanhf(c);
            hbuf[l][s][u] = h;
            if (l == 2 && pos0 + s < T) {
                const long o = ((long)t * T + pos0 + s) * 64 + u;
                out[o] = h + pe[(pos0 + s) * 64 + u];
                if (raw) raw[o] = h;
            }
        }
        __syncthreads();
    }
}

// ---- music front: every frame pair of the song, once per rollout -----------------------------------------------------------------
// cond [b][n][438]; row m = clip * pairs + p reads frames 2 p, 2 p + 1 (876 consecutive floats)
__global__ __launch_bounds__(256) void nav_music_kernel(const float* __restrict__ cond, int n_frames, int pairs, int rows,
                                                        const float* __restrict__ wm, float* __restrict__ mp,
                                                        float* __restrict__ me) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LA = MU_K0 + 4, LH = MU_N + 4, LO = 68;
    float* As = smem;
    float* H1 = As + NV_R * LA;
    float* H2 = H1 + NV_R * LH;
    float* O3 = H2 + NV_R * LH;
    const int row0 = blockIdx.x * NV_R, wv = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < NV_R * MU_K0; i += 256) {
        const int r = i / MU_K0, k = i - r * MU_K0, m = row0 + r;
        float v = 0.f;
        if (m < rows && k < 876) {
            const int clip = m / pairs, p = m - clip * pairs;
            v = cond[((long)clip * n_frames + 2 * p) * 438 + k];
        }
        As[r * LA + k] = v;
    }
    __syncthreads();
    const float* b1 = wm + MU_B1;
    nav_mm16(As, LA, wm + MU_W1, MU_K0, MU_N / 16, MU_K0, wv, 4, [&](int r, int c, float v) { H1[r * LH + c] = leaky(v + b1[c]); });
    __syncthreads();
    const float* b2 = wm + MU_B2;
    nav_mm16(H1, LH, wm + MU_W2, MU_N, MU_N / 16, MU_N, wv, 4, [&](int r, int c, float v) { H2[r * LH + c] = leaky(v + b2[c]); });
    __syncthreads();
    const float* b3 = wm + MU_B3;
    nav_mm16(H2, LH, wm + MU_W3, MU_N, 4, MU_N, wv, 4, [&](int r, int c, float v) {
        const float y = v + b3[c];
        O3[r * LO + c] = y;
        if (row0 + r < rows) mp[(long)(row0 + r) * 64 + c] = y;
    });
    __syncthreads();
    const float* bc = wm + MU_BC;
    nav_mm16(O3, LO, wm + MU_WC, 64, 4, 64, wv, 4, [&](int r, int c, float v) {
        if (row0 + r < rows) me[(long)(row0 + r) * 64 + c] = v + bc[c];
    });
}

// ---- one transformer block of 16 rows --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nav_block_kernel(tcdiff_nav_args a, int layer, int win) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Xs = smem;
    float* Ns = Xs + NV_R * NV_LD;
    float* Ys = Ns + NV_R * NV_LD;
    float* Big = Ys + NV_R * NV_LD;
    const int T = a.dn * a.seq, Tp = (T + 15) & ~15;
    const int clip = blockIdx.y, row0 = blockIdx.x * NV_R;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const long set = (long)a.b * Tp * NV_W;                  // one ping-pong image of Q, K or V^T
    const int moff = win * a.win_stride;
    float* xg = a.x + (long)clip * T * NV_W;

    if (layer < 0) {
        // [cond_emb(music rows of the conditioning side) repeated per dancer | LSTM output + positional encoding]
        for (int i = tid; i < NV_R * NV_W; i += 256) {
            const int r = i >> 7, c = i & 127, pos = row0 + r;
            float v = 0.f;
            if (pos < T) {
                v = c < 64 ? a.me[((long)clip * a.pairs + a.me_off + moff + pos % a.seq) * 64 + c]
                           : a.lstm_out[((long)clip * T + pos) * 64 + c - 64];
                xg[(long)pos * NV_W + c] = v;
            }
            Xs[r * NV_LD + c] = v;
        }
        __syncthreads();
    } else {
        const float* P = a.blocks + (long)layer * BK_SIZE;
        const long cur = (long)(layer & 1) * set;
        const float* qg = a.q + cur + (long)clip * Tp * NV_W;
        for (int i = tid; i < NV_R * NV_W; i += 256) {
            const int r = i >> 7, c = i & 127, pos = row0 + r;
            Xs[r * NV_LD + c] = pos < T ? xg[(long)pos * NV_W + c] : 0.f;
            Ns[r * NV_LD + c] = pos < T ? qg[(long)pos * NV_W + c] : 0.f;
        }
        __syncthreads();
        // attention, no mask (traj_model.py:37-41): wave = head; scores of the 16 rows against every key of the clip in LDS
        {
            const int ldS = Tp + 4;
            float* Sw = Big + wv * NV_R * ldS;
            const float* kg = a.k + cur + ((long)clip * 4 + wv) * Tp * 32;
            const float* vg = a.vt + cur + ((long)clip * 4 + wv) * 32 * Tp;
            const float scale = 0.17677669529663688f;        // 1 / sqrt(32)
            nav_mm16(Ns + wv * 32, NV_LD, kg, 32, Tp / 16, 32, 0, 1, [&](int r, int c, float v) { Sw[r * ldS + c] = v * scale; });
            __syncthreads();
            {
                float* srow = Sw + (lane >> 2) * ldS;
                const int sub = lane & 3;
                float m = -INFINITY;
                for (int c = sub; c < T; c += 4) m = fmaxf(m, srow[c]);
                m = fmaxf(m, __shfl_xor(m, 1));
                m = fmaxf(m, __shfl_xor(m, 2));
                float s = 0.f;
                for (int c = sub; c < T; c += 4) {
                    const float e = expf(srow[c] - m);
                    srow[c] = e;
                    s += e;
                }
                s += __shfl_xor(s, 1);
                s += __shfl_xor(s, 2);
                for (int c = sub; c < T; c += 4) srow[c] = srow[c] / s;
                for (int c = T + sub; c < Tp; c += 4) srow[c] = 0.f;
            }
            __syncthreads();
            nav_mm16(Sw, ldS, vg, Tp, 2, Tp, 0, 1, [&](int r, int c, float v) { Ys[r * NV_LD + wv * 32 + c] = v; });
            __syncthreads();
        }
        const float* bp = P + BK_BP;
        nav_mm16(Ys, NV_LD, P + BK_WP, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) { Xs[r * NV_LD + c] += v + bp[c]; });
        __syncthreads();
        nav_ln16(Xs, Ns, P + BK_LN2G, P + BK_LN2B);
        __syncthreads();
        constexpr int LH = NV_HID + 4;
        const float* b1 = P + BK_B1;
        nav_mm16(Ns, NV_LD, P + BK_W1, NV_W, NV_HID / 16, NV_W, wv, 4,
                 [&](int r, int c, float v) { Big[r * LH + c] = gelu_erf(v + b1[c]); });
        __syncthreads();
        const float* b2 = P + BK_B2;
        nav_mm16(Big, LH, P + BK_W2, NV_HID, 8, NV_HID, wv, 4, [&](int r, int c, float v) { Xs[r * NV_LD + c] += v + b2[c]; });
        __syncthreads();
        float* tap = a.tap_blocks ? a.tap_blocks + ((long)layer * a.b + clip) * T * NV_W : nullptr;
        for (int i = tid; i < NV_R * NV_W; i += 256) {
            const int r = i >> 7, c = i & 127, pos = row0 + r;
            if (pos < T) {
                const float v = Xs[r * NV_LD + c];
                xg[(long)pos * NV_W + c] = v;
                if (tap) tap[(long)pos * NV_W + c] = v;
            }
        }
    }

    if (layer + 1 < a.n_layers) {
        // the next block's LN1 and Q / K / V: Q [clip][Tp][128], K [clip][head][Tp][32], V^T [clip][head][32][Tp]
        const float* P = a.blocks + (long)(layer + 1) * BK_SIZE;
        const long nxt = (long)((layer + 1) & 1) * set;
        nav_ln16(Xs, Ns, P + BK_LN1G, P + BK_LN1B);
        __syncthreads();
        float* qo = a.q + nxt + (long)clip * Tp * NV_W;
        float* ko = a.k + nxt + (long)clip * 4 * Tp * 32;
        float* vo = a.vt + nxt + (long)clip * 4 * 32 * Tp;
        const float *bq = P + BK_BQ, *bk = P + BK_BK, *bv = P + BK_BV;
        nav_mm16(Ns, NV_LD, P + BK_WQ, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) {
            if (row0 + r < T) qo[(long)(row0 + r) * NV_W + c] = v + bq[c];
        });
        nav_mm16(Ns, NV_LD, P + BK_WK, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) {
            if (row0 + r < T) ko[((long)(c >> 5) * Tp + row0 + r) * 32 + (c & 31)] = v + bk[c];
        });
        nav_mm16(Ns, NV_LD, P + BK_WV, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) {
            if (row0 + r < T) vo[(long)c * Tp + row0 + r] = v + bv[c];
        });
    } else {
        // Decoder on [x | music rows of the prediction side]: 192 -> 128 -> 128 -> 64 -> 2, LeakyReLU between
        constexpr int LD = 196;
        const float* D = a.dec;
        for (int i = tid; i < NV_R * 192; i += 256) {
            const int r = i / 192, c = i - r * 192, pos = row0 + r;
            float v = 0.f;
            if (c < NV_W) v = Xs[r * NV_LD + c];
            else if (pos < T) v = a.mp[((long)clip * a.pairs + a.mp_off + moff + pos % a.seq) * 64 + c - NV_W];
            Big[r * LD + c] = v;
        }
        __syncthreads();
        const float *d1 = D + DC_B1, *d2 = D + DC_B2, *d3 = D + DC_B3, *d4 = D + DC_B4;
        nav_mm16(Big, LD, D + DC_W1, 192, 8, 192, wv, 4, [&](int r, int c, float v) { Ns[r * NV_LD + c] = leaky(v + d1[c]); });
        __syncthreads();
        nav_mm16(Ns, NV_LD, D + DC_W2, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) { Ys[r * NV_LD + c] = leaky(v + d2[c]); });
        __syncthreads();
        nav_mm16(Ys, NV_LD, D + DC_W3, NV_W, 4, NV_W, wv, 4, [&](int r, int c, float v) { Ns[r * NV_LD + c] = leaky(v + d3[c]); });
        __syncthreads();
        nav_mm16(Ns, NV_LD, D + DC_W4, 64, 1, 64, wv, 4, [&](int r, int c, float v) {
            const int pos = row0 + r;
            if (c < 2 && pos < T) {
                const float y = v + d4[c];
                a.traj[((long)clip * T + pos) * 2 + c] = y;
                const int d = pos / a.seq, s = pos - d * a.seq;
                if (a.roll && s >= a.seq - a.step)
                    a.roll[(((long)clip * a.dn + d) * a.roll_frames + a.roll_off + win * a.step + s - (a.seq - a.step)) * 2 + c] = y;
            }
        });
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int tcdiff_nav_music_front(const float* cond, int b, int n_frames, const float* wm, float* mp, float* me,
                                      hipStream_t stream) {
    if (!cond || !wm || !mp || !me || b < 1 || n_frames < 2) return TCDIFF_ERR_ARG;
    if (!al16(wm) || !al16(mp) || !al16(me)) return TCDIFF_ERR_ALIGN;
    const int pairs = n_frames / 2;
    const long rows = (long)b * pairs;
    if (rows > (1 << 24)) return TCDIFF_ERR_ARG;
    const int smem = NV_R * ((MU_K0 + 4) + 2 * (MU_N + 4) + 68) * (int)sizeof(float);
    static bool ready = false;
    if (!ready) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(nav_music_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem) !=
            hipSuccess) {
            (void)hipGetLastError();
            return TCDIFF_ERR_UNSUPPORTED;
        }
        ready = true;
    }
    nav_music_kernel<<<dim3((unsigned)((rows + NV_R - 1) / NV_R)), dim3(256), smem, stream>>>(cond, n_frames, pairs, (int)rows, wm,
                                                                                              mp, me);
    return hipGetLastError() == hipSuccess ? TCDIFF_OK : TCDIFF_ERR_LAUNCH;
}

extern "C" int tcdiff_nav_rollout(const tcdiff_nav_args* a, int n_windows, hipStream_t stream) {
    if (!a || n_windows < 1 || a->b < 1 || a->dn < 1 || a->seq < 1 || a->n_layers < 1 || a->pairs < 1) return TCDIFF_ERR_ARG;
    if (!a->lstm_w || !a->lstm_bih || !a->lstm_bhh || !a->pe || !a->blocks || !a->dec || !a->me || !a->mp || !a->traj ||
        !a->lstm_out || !a->x || !a->q || !a->k || !a->vt)
        return TCDIFF_ERR_ARG;
    const int T = a->dn * a->seq, Tp = (T + 15) & ~15;
    if (T > 500) return TCDIFF_ERR_UNSUPPORTED;              // PositionalEncoding max_len (model/utils.py:12): the reference raises
    // every window's music rows must lie inside the tables
    const int last = (n_windows - 1) * a->win_stride;
    if (a->me_off < 0 || a->mp_off < 0 || a->win_stride < 0 || a->me_off + last + a->seq > a->pairs ||
        a->mp_off + last + a->seq > a->pairs)
        return TCDIFF_ERR_ARG;
    if (a->roll && (a->step < 1 || a->step > a->seq || a->roll_off < 0 || a->roll_off + n_windows * a->step > a->roll_frames))
        return TCDIFF_ERR_ARG;
    if (!al16(a->blocks) || !al16(a->dec) || !al16(a->me) || !al16(a->mp) || !al16(a->lstm_out) || !al16(a->x) || !al16(a->q) ||
        !al16(a->k) || !al16(a->vt) || !al16(a->lstm_w))
        return TCDIFF_ERR_ALIGN;
    const int big = 4 * NV_R * (Tp + 4) > NV_R * (NV_HID + 4) ? 4 * NV_R * (Tp + 4) : NV_R * (NV_HID + 4);
    const int smem = (3 * NV_R * NV_LD + big) * (int)sizeof(float);
    static int ready = 0;
    if (ready < smem) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(nav_block_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, smem) !=
            hipSuccess) {
            (void)hipGetLastError();
            return TCDIFF_ERR_UNSUPPORTED;
        }
        ready = smem;
    }
    const dim3 grid((unsigned)((T + NV_R - 1) / NV_R), (unsigned)a->b);
    tcdiff_nav_args aw = *a;
    for (int w = 0; w < n_windows; ++w) {
        if (w == 1) aw.tap_blocks = nullptr;                 // the per-stage taps record the first window only
        nav_lstm_kernel<<<dim3((unsigned)((T + NV_LSTM_S - 1) / NV_LSTM_S)), dim3(768), 0, stream>>>(
            a->traj, a->lstm_w, a->lstm_bih, a->lstm_bhh, a->pe, a->lstm_out, w == 0 ? a->tap_lstm : nullptr, a->b, T);
        for (int layer = -1; layer < a->n_layers; ++layer) nav_block_kernel<<<grid, dim3(256), smem, stream>>>(aw, layer, w);
        if (hipGetLastError() != hipSuccess) return TCDIFF_ERR_LAUNCH;
    }
    return TCDIFF_OK;
}
