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
#include "nav_common.h"
#include "train_common.h"

namespace {

// ---- LSTM over the clip axis ---------------------------------------------------------------------------------------------------
// x [b][T][2]; wpk [3][128][256] (k < 64: weight_ih column k, zero beyond the layer's input width; k >= 64: weight_hh column k - 64;
// 256 gate rows in PyTorch's order i, f, g, o); bih / bhh [3][256]; pe [>= T][64]; out [b][T][64] = h + pe; raw (or NULL) = h.
// TR (the train-mode forward): pos_embed's dropout on h + pe, and every layer's activated gates, cell and hidden state written out.
template <bool TR>
__global__ __launch_bounds__(768) void nav_lstm_kernel(const float* __restrict__ x, const float* __restrict__ wpk,
                                                       const float* __restrict__ bih, const float* __restrict__ bhh,
                                                       const float* __restrict__ pe, float* __restrict__ out,
                                                       float* __restrict__ raw, int b, int T, tcdiff_nav_train_args tr) {
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
            if constexpr (TR) {
                if (pos0 + s < T) {
                    const long row = ((long)l * b + t) * T + pos0 + s;
                    float* gs = tr.lstm_gates + row * 256 + u;
                    gs[0] = gi, gs[64] = gf, gs[128] = gg, gs[192] = go;
                    tr.lstm_c[row * 64 + u] = c;
                    tr.lstm_h[row * 64 + u] = h;
                }
            }
            if (l == 2 && pos0 + s < T) {
                const long o = ((long)t * T + pos0 + s) * 64 + u;
                if constexpr (TR) {
                    const DropCtx dc = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_POS, tr.drop_thr, tr.drop_scale);
                    out[o] = drop_apply(dc, (uint32_t)o, h + pe[(pos0 + s) * 64 + u]);
                } else {
                    out[o] = h + pe[(pos0 + s) * 64 + u];
                }
                if (raw) raw[o] = h;
            }
        }
        __syncthreads();
    }
}

// ---- music front: every frame pair of the song, once per rollout -----------------------------------------------------------------
// cond [b][n][438]; row m = clip * pairs + p reads frames 2 p, 2 p + 1 (876 consecutive floats)
// zs (the train-mode forward, else NULL): [rows][896] receives the two hidden layers' pre-activations
__global__ __launch_bounds__(256) void nav_music_kernel(const float* __restrict__ cond, int n_frames, int pairs, int rows,
                                                        const float* __restrict__ wm, float* __restrict__ mp,
                                                        float* __restrict__ me, float* __restrict__ zs) {
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
    nav_mm16(As, LA, wm + MU_W1, MU_K0, MU_N / 16, MU_K0, wv, 4, [&](int r, int c, float v) {
        const float z = v + b1[c];
        if (zs && row0 + r < rows) zs[(long)(row0 + r) * (2 * MU_N) + c] = z;
        H1[r * LH + c] = leaky(z);
    });
    __syncthreads();
    const float* b2 = wm + MU_B2;
    nav_mm16(H1, LH, wm + MU_W2, MU_N, MU_N / 16, MU_N, wv, 4, [&](int r, int c, float v) {
        const float z = v + b2[c];
        if (zs && row0 + r < rows) zs[(long)(row0 + r) * (2 * MU_N) + MU_N + c] = z;
        H2[r * LH + c] = leaky(z);
    });
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
// TR (the train-mode forward): the three dropout sites of a block, Q / K / V and the residual stream kept per layer instead of
// ping-pong / in place, and what the backward reads written out (tcdiff_nav_train_args).
template <bool TR>
__global__ __launch_bounds__(256) void nav_block_kernel(tcdiff_nav_args a, int layer, int win, tcdiff_nav_train_args tr) {
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
    const long img = (long)a.b * T * NV_W;                   // TR: one layer's rows
    float* xg = TR ? tr.xs + (layer + 1) * img + (long)clip * T * NV_W : a.x + (long)clip * T * NV_W;
    const float* xin = TR ? xg - img : xg;

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
        const long cur = (long)(TR ? layer : layer & 1) * set;
        const float* qg = a.q + cur + (long)clip * Tp * NV_W;
        for (int i = tid; i < NV_R * NV_W; i += 256) {
            const int r = i >> 7, c = i & 127, pos = row0 + r;
            Xs[r * NV_LD + c] = pos < T ? xin[(long)pos * NV_W + c] : 0.f;
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
                if constexpr (TR) {
                    const int pos = row0 + (lane >> 2);
                    if (sub == 0 && pos < T) tr.lse[(((long)layer * a.b + clip) * 4 + wv) * Tp + pos] = m + logf(s);
                    const DropCtx dc = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_BLOCK(layer, 0), tr.drop_thr, tr.drop_scale);
                    const uint32_t base = (uint32_t)((((long)clip * 4 + wv) * T + pos) * T);
                    for (int c = sub; c < T; c += 4) srow[c] = drop_apply(dc, base + (uint32_t)c, srow[c] / s);
                } else
                for (int c = sub; c < T; c += 4) srow[c] = srow[c] / s;
                for (int c = T + sub; c < Tp; c += 4) srow[c] = 0.f;
            }
            __syncthreads();
            nav_mm16(Sw, ldS, vg, Tp, 2, Tp, 0, 1, [&](int r, int c, float v) { Ys[r * NV_LD + wv * 32 + c] = v; });
            __syncthreads();
        }
        const float* bp = P + BK_BP;
        if constexpr (TR) {
            float* og = tr.att_o + layer * img + (long)clip * T * NV_W;
            for (int i = tid; i < NV_R * NV_W; i += 256)
                if (row0 + (i >> 7) < T) og[(long)(row0 + (i >> 7)) * NV_W + (i & 127)] = Ys[(i >> 7) * NV_LD + (i & 127)];
            const DropCtx dc = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_BLOCK(layer, 1), tr.drop_thr, tr.drop_scale);
            nav_mm16(Ys, NV_LD, P + BK_WP, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) {
                Xs[r * NV_LD + c] += drop_apply(dc, (uint32_t)(((long)clip * T + row0 + r) * NV_W + c), v + bp[c]);
            });
        } else {
            nav_mm16(Ys, NV_LD, P + BK_WP, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) { Xs[r * NV_LD + c] += v + bp[c]; });
        }
        __syncthreads();
        if constexpr (TR) {
            float* mg = tr.xmid + layer * img + (long)clip * T * NV_W;
            for (int i = tid; i < NV_R * NV_W; i += 256)
                if (row0 + (i >> 7) < T) mg[(long)(row0 + (i >> 7)) * NV_W + (i & 127)] = Xs[(i >> 7) * NV_LD + (i & 127)];
        }
        nav_ln16(Xs, Ns, P + BK_LN2G, P + BK_LN2B);
        __syncthreads();
        constexpr int LH = NV_HID + 4;
        const float* b1 = P + BK_B1;
        nav_mm16(Ns, NV_LD, P + BK_W1, NV_W, NV_HID / 16, NV_W, wv, 4,
                 [&](int r, int c, float v) {
                     const float z = v + b1[c];
                     if constexpr (TR)
                         if (row0 + r < T) tr.hid[(((long)layer * a.b + clip) * T + row0 + r) * NV_HID + c] = z;
                     Big[r * LH + c] = gelu_erf(z);
                 });
        __syncthreads();
        const float* b2 = P + BK_B2;
        if constexpr (TR) {
            const DropCtx dc = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_BLOCK(layer, 2), tr.drop_thr, tr.drop_scale);
            nav_mm16(Big, LH, P + BK_W2, NV_HID, 8, NV_HID, wv, 4, [&](int r, int c, float v) {
                Xs[r * NV_LD + c] += drop_apply(dc, (uint32_t)(((long)clip * T + row0 + r) * NV_W + c), v + b2[c]);
            });
        } else {
            nav_mm16(Big, LH, P + BK_W2, NV_HID, 8, NV_HID, wv, 4, [&](int r, int c, float v) { Xs[r * NV_LD + c] += v + b2[c]; });
        }
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
        const long nxt = (long)(TR ? layer + 1 : (layer + 1) & 1) * set;
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
        nav_mm16(Big, LD, D + DC_W1, 192, 8, 192, wv, 4, [&](int r, int c, float v) {
            const float z = v + d1[c];
            if constexpr (TR)
                if (row0 + r < T) tr.dec_z[((long)clip * T + row0 + r) * 320 + c] = z;
            Ns[r * NV_LD + c] = leaky(z);
        });
        __syncthreads();
        nav_mm16(Ns, NV_LD, D + DC_W2, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) {
            const float z = v + d2[c];
            if constexpr (TR)
                if (row0 + r < T) tr.dec_z[((long)clip * T + row0 + r) * 320 + 128 + c] = z;
            Ys[r * NV_LD + c] = leaky(z);
        });
        __syncthreads();
        nav_mm16(Ys, NV_LD, D + DC_W3, NV_W, 4, NV_W, wv, 4, [&](int r, int c, float v) {
            const float z = v + d3[c];
            if constexpr (TR)
                if (row0 + r < T) tr.dec_z[((long)clip * T + row0 + r) * 320 + 256 + c] = z;
            Ns[r * NV_LD + c] = leaky(z);
        });
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

int music_front(const float* cond, int b, int n_frames, const float* wm, float* mp, float* me, float* zs, hipStream_t stream) {
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
                                                                                              mp, me, zs);
    return hipGetLastError() == hipSuccess ? TCDIFF_OK : TCDIFF_ERR_LAUNCH;
}

}  // namespace

extern "C" int tcdiff_nav_music_front(const float* cond, int b, int n_frames, const float* wm, float* mp, float* me,
                                      hipStream_t stream) {
    return music_front(cond, b, n_frames, wm, mp, me, nullptr, stream);
}

namespace {

template <bool TR>
int nav_windows(const tcdiff_nav_args* a, const tcdiff_nav_train_args& tr, int n_windows, hipStream_t stream) {
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
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(nav_block_kernel<TR>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                smem) != hipSuccess) {
            (void)hipGetLastError();
            return TCDIFF_ERR_UNSUPPORTED;
        }
        ready = smem;
    }
    const dim3 grid((unsigned)((T + NV_R - 1) / NV_R), (unsigned)a->b);
    tcdiff_nav_args aw = *a;
    for (int w = 0; w < n_windows; ++w) {
        if (w == 1) aw.tap_blocks = nullptr;                 // the per-stage taps record the first window only
        nav_lstm_kernel<TR><<<dim3((unsigned)((T + NV_LSTM_S - 1) / NV_LSTM_S)), dim3(768), 0, stream>>>(
            a->traj, a->lstm_w, a->lstm_bih, a->lstm_bhh, a->pe, a->lstm_out, w == 0 ? a->tap_lstm : nullptr, a->b, T, tr);
        for (int layer = -1; layer < a->n_layers; ++layer) nav_block_kernel<TR><<<grid, dim3(256), smem, stream>>>(aw, layer, w, tr);
        if (hipGetLastError() != hipSuccess) return TCDIFF_ERR_LAUNCH;
    }
    return TCDIFF_OK;
}

}  // namespace

extern "C" int tcdiff_nav_rollout(const tcdiff_nav_args* a, int n_windows, hipStream_t stream) {
    return nav_windows<false>(a, tcdiff_nav_train_args{}, n_windows, stream);
}

extern "C" int tcdiff_nav_train_fwd(const tcdiff_nav_args* a, const tcdiff_nav_train_args* t, const float* wm, hipStream_t stream) {
    if (!a || !t || !wm || a->roll || a->tap_lstm || a->tap_blocks || a->me_off != 0 || a->mp_off != a->pairs - a->seq)
        return TCDIFF_ERR_ARG;
    if (!t->cond || !t->lstm_gates || !t->lstm_c || !t->lstm_h || !t->xs || !t->xmid || !t->att_o || !t->lse || !t->hid ||
        !t->dec_z || !t->mus_z)
        return TCDIFF_ERR_ARG;
    const int rc = music_front(t->cond, a->b, 2 * a->pairs, wm, const_cast<float*>(a->mp), const_cast<float*>(a->me), t->mus_z, stream);
    if (rc != TCDIFF_OK) return rc;
    return nav_windows<true>(a, *t, 1, stream);
}
