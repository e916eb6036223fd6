// The backward pass of the Dance-Beat Navigator (TrajDecoder/train_traj.py:200, torch autograd over traj_model.py:170-200), exact
// fp32 with v_mfma_f32_16x16x4_f32 products.  The train-mode forward (navigator.hip, TR instantiations) left what is read here.
//
//   navt_dec_bwd     16 token rows: the four Decoder linears backwards, LeakyReLU adjoints in the epilogues; writes every d z (the
//                    weight gradients' left operand), d x and the per-row gradient of the music columns.
//   navt_mlp_bwd     one block, 16 rows: mlp[3] mask -> mlp[2]^T -> erf-GELU' -> mlp[0]^T -> LN2 backward + residual -> resid_drop
//                    mask -> proj^T -> d O and delta = d O . O per head.
//   navt_attn_dq     flash-style, 16 query rows x 4 heads (wave = head): P = exp(s - lse) recomputed from Q, K; d P = d O V^T with
//                    attn_drop's mask regenerated; d S = P (d P - delta) / sqrt(32) in place; d Q = d S K.
//   navt_attn_dkv    the same per 16 key rows: d V = (P mask)^T d O, d K = d S^T Q (the score tile recomputed for each).
//   navt_qkv_bwd     16 rows: d n1 = d Q Wq + d K Wk + d V Wv in one accumulator chain, LN1 backward + residual.
//   navt_front_bwd   16 music rows: cond_emb half summed over dancers, cond_emb^T, + the Decoder's music rows summed over dancers
//                    (the two row ranges overlap when pairs < 2 seq: they add), music_projection's last two linears backwards.
//   navt_lstm_bwd    backward through time over the CLIP axis: 16 positions per workgroup, four waves per layer, the forward's
//                    wavefront reversed (layer l handles clip b - 1 - (tick - (2 - l))); pos_embed's mask on the way in.
//   navt_wgrad / navt_wreduce   d W[n][k] = sum_rows d Y[row][n] act(X[row][k]) and d b[n] = sum_rows d Y[row][n]: stage one sums
//                    fixed row chunks into `partial`, stage two adds the chunks in order.  navt_ln_reduce: the LayerNorm weights.
// No floating-point atomics anywhere: the same inputs and seed give the same bits.
#include "nav_common.h"
#include "train_common.h"

namespace {

DEVINL float leaky_grad(float z) { return z > 0.f ? 1.f : 0.01f; }
// d/dz of 0.5 z (1 + erf(z / sqrt 2)) with libm's erf / exp: the tests hold the gradients to a few fp32 roundings
DEVINL float gelu_erf_grad(float z) {
    return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.3989422804014327f * expf(-0.5f * z * z);
}

constexpr float NV_SCALE = 0.17677669529663688f;             // 1 / sqrt(32)

// LayerNorm(128) backward of 16 rows: Xs the input rows, Ds d(output); Gs += d(input).  The output rows go to n_out (global, rows
// below `valid`), sum_rows d y * xhat and sum_rows d y to part[0 .. 127] / part[128 .. 255] through red [4][256] (waves in order).
DEVINL void nav_ln16_bwd(const float* Xs, const float* Ds, float* Gs, const float* __restrict__ gam, const float* __restrict__ bet,
                         float* __restrict__ n_out, int valid, float* red, float* __restrict__ part) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float sg0 = 0.f, sg1 = 0.f, sb0 = 0.f, sb1 = 0.f;
    const float g0 = gam[lane], g1 = gam[64 + lane];
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
        const float h0 = d0 * rstd, h1 = d1 * rstd;
        const float y0 = Ds[r * NV_LD + lane], y1 = Ds[r * NV_LD + 64 + lane];
        if (r < valid) {
            n_out[(long)r * NV_W + lane] = h0 * g0 + bet[lane];
            n_out[(long)r * NV_W + 64 + lane] = h1 * g1 + bet[64 + lane];
        }
        sg0 += y0 * h0, sg1 += y1 * h1, sb0 += y0, sb1 += y1;
        const float e0 = y0 * g0, e1 = y1 * g1;
        float m1 = e0 + e1, m2 = e0 * h0 + e1 * h1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            m1 += __shfl_xor(m1, o);
            m2 += __shfl_xor(m2, o);
        }
        m1 *= 1.f / NV_W, m2 *= 1.f / NV_W;
        Gs[r * NV_LD + lane] += rstd * (e0 - m1 - h0 * m2);
        Gs[r * NV_LD + 64 + lane] += rstd * (e1 - m1 - h1 * m2);
    }
    red[wv * 256 + lane] = sg0, red[wv * 256 + 64 + lane] = sg1;
    red[wv * 256 + 128 + lane] = sb0, red[wv * 256 + 192 + lane] = sb1;
    __syncthreads();
    part[threadIdx.x] = ((red[threadIdx.x] + red[256 + threadIdx.x]) + red[512 + threadIdx.x]) + red[768 + threadIdx.x];
}

// ---- Decoder -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void navt_dec_bwd(tcdiff_nav_args a, tcdiff_nav_train_args tr) {
    __shared__ __attribute__((aligned(16))) float A[NV_R * NV_LD], B[NV_R * NV_LD];
    const int T = a.dn * a.seq, clip = blockIdx.y, row0 = blockIdx.x * NV_R, tid = threadIdx.x, wv = tid >> 6;
    const long base = (long)clip * T;
    const float* D = a.dec;
    {
        const int r = tid >> 4, c = tid & 15, pos = row0 + r;
        const float v = (c < 2 && pos < T) ? tr.d_out[(base + pos) * 2 + c] : 0.f;
        A[r * NV_LD + c] = v;
        if (pos < T) tr.g_dec[(base + pos) * 336 + 320 + c] = v;
    }
    __syncthreads();
    nav_mm16t(A, NV_LD, D + DC_W4, 64, 4, 16, wv, 4, [&](int r, int c, float v) {
        const int pos = row0 + r;
        float g = 0.f;
        if (pos < T) {
            g = v * leaky_grad(tr.dec_z[(base + pos) * 320 + 256 + c]);
            tr.g_dec[(base + pos) * 336 + 256 + c] = g;
        }
        B[r * NV_LD + c] = g;
    });
    __syncthreads();
    nav_mm16t(B, NV_LD, D + DC_W3, 128, 8, 64, wv, 4, [&](int r, int c, float v) {
        const int pos = row0 + r;
        float g = 0.f;
        if (pos < T) {
            g = v * leaky_grad(tr.dec_z[(base + pos) * 320 + 128 + c]);
            tr.g_dec[(base + pos) * 336 + 128 + c] = g;
        }
        A[r * NV_LD + c] = g;
    });
    __syncthreads();
    nav_mm16t(A, NV_LD, D + DC_W2, 128, 8, 128, wv, 4, [&](int r, int c, float v) {
        const int pos = row0 + r;
        float g = 0.f;
        if (pos < T) {
            g = v * leaky_grad(tr.dec_z[(base + pos) * 320 + c]);
            tr.g_dec[(base + pos) * 336 + c] = g;
        }
        B[r * NV_LD + c] = g;
    });
    __syncthreads();
    nav_mm16t(B, NV_LD, D + DC_W1, 192, 12, 128, wv, 4, [&](int r, int c, float v) {
        const int pos = row0 + r;
        if (pos >= T) return;
        if (c < NV_W) tr.gx[(base + pos) * NV_W + c] = v;
        else tr.g_mpb[(base + pos) * 64 + c - NV_W] = v;
    });
}

// ---- one block: MLP, LN2, proj ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void navt_mlp_bwd(tcdiff_nav_args a, tcdiff_nav_train_args tr, int layer) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LH = NV_HID + 4;
    float* Gs = smem;
    float* Ms = Gs + NV_R * NV_LD;
    float* Ns = Ms + NV_R * NV_LD;
    float* Xs = Ns + NV_R * NV_LD;
    float* Hs = Xs + NV_R * NV_LD;
    float* red = Hs + NV_R * LH;
    const int T = a.dn * a.seq, Tp = (T + 15) & ~15, clip = blockIdx.y, row0 = blockIdx.x * NV_R, tid = threadIdx.x, wv = tid >> 6;
    const long base = (long)clip * T, lrow = ((long)layer * a.b + clip) * T;
    const float* P = a.blocks + (long)layer * BK_SIZE;
    const DropCtx dm = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_BLOCK(layer, 2), tr.drop_thr, tr.drop_scale);
    const DropCtx dr = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_BLOCK(layer, 1), tr.drop_thr, tr.drop_scale);
    for (int i = tid; i < NV_R * NV_W; i += 256) {
        const int r = i >> 7, c = i & 127, pos = row0 + r;
        float g = 0.f, x = 0.f, m = 0.f;
        if (pos < T) {
            g = tr.gx[(base + pos) * NV_W + c];
            x = tr.xmid[(lrow + pos) * NV_W + c];
            m = drop_apply(dm, (uint32_t)((base + pos) * NV_W + c), g);
            tr.g_m[(base + pos) * NV_W + c] = m;
        }
        Gs[r * NV_LD + c] = g, Xs[r * NV_LD + c] = x, Ms[r * NV_LD + c] = m;
    }
    __syncthreads();
    nav_mm16t(Ms, NV_LD, P + BK_W2, NV_HID, NV_HID / 16, NV_W, wv, 4, [&](int r, int c, float v) {
        const int pos = row0 + r;
        float g = 0.f;
        if (pos < T) {
            g = v * gelu_erf_grad(tr.hid[(lrow + pos) * NV_HID + c]);
            tr.g_hid[(base + pos) * NV_HID + c] = g;
        }
        Hs[r * LH + c] = g;
    });
    __syncthreads();
    nav_mm16t(Hs, LH, P + BK_W1, NV_W, 8, NV_HID, wv, 4, [&](int r, int c, float v) { Ns[r * NV_LD + c] = v; });
    __syncthreads();
    const long blk = (long)clip * gridDim.x + blockIdx.x;
    nav_ln16_bwd(Xs, Ns, Gs, P + BK_LN2G, P + BK_LN2B, tr.n2 + (base + row0) * NV_W, T - row0, red, tr.ln_part + blk * 512 + 256);
    __syncthreads();
    for (int i = tid; i < NV_R * NV_W; i += 256) {
        const int r = i >> 7, c = i & 127, pos = row0 + r;
        float m = 0.f;
        if (pos < T) {
            const float g = Gs[r * NV_LD + c];
            tr.gx[(base + pos) * NV_W + c] = g;
            m = drop_apply(dr, (uint32_t)((base + pos) * NV_W + c), g);
            tr.g_a[(base + pos) * NV_W + c] = m;
        }
        Ms[r * NV_LD + c] = m;
    }
    __syncthreads();
    nav_mm16t(Ms, NV_LD, P + BK_WP, NV_W, 8, NV_W, wv, 4, [&](int r, int c, float v) {
        const int pos = row0 + r;
        if (pos < T) tr.g_o[((long)clip * Tp + pos) * NV_W + c] = v;
        Ns[r * NV_LD + c] = v;
    });
    __syncthreads();
    {
        const int r = tid >> 4, h = (tid >> 2) & 3, sub = tid & 3, pos = row0 + r;
        float s = 0.f;
        if (pos < T)
            for (int c = sub; c < 32; c += 4) s += Ns[r * NV_LD + h * 32 + c] * tr.att_o[(lrow + pos) * NV_W + h * 32 + c];
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        if (sub == 0 && pos < T) tr.delta[((long)clip * 4 + h) * Tp + pos] = s;
    }
}

// ---- attention backward, query side ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void navt_attn_dq(tcdiff_nav_args a, tcdiff_nav_train_args tr, int layer) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Qs = smem;
    float* Ds = Qs + NV_R * NV_LD;
    float* Ls = Ds + NV_R * NV_LD;          // [4][16] log-sum-exp, then [4][16] delta
    float* Big = Ls + 128;
    const int T = a.dn * a.seq, Tp = (T + 15) & ~15, clip = blockIdx.y, row0 = blockIdx.x * NV_R, tid = threadIdx.x, wv = tid >> 6;
    const long set = (long)a.b * Tp * NV_W, cur = (long)layer * set;
    const float* qg = a.q + cur + (long)clip * Tp * NV_W;
    const float* kg = a.k + cur + ((long)clip * 4 + wv) * Tp * 32;
    const float* vg = a.vt + cur + ((long)clip * 4 + wv) * 32 * Tp;
    for (int i = tid; i < NV_R * NV_W; i += 256) {
        const int r = i >> 7, c = i & 127, pos = row0 + r;
        Qs[r * NV_LD + c] = pos < T ? qg[(long)pos * NV_W + c] : 0.f;
        Ds[r * NV_LD + c] = pos < T ? tr.g_o[((long)clip * Tp + pos) * NV_W + c] : 0.f;
    }
    if (tid < 128) {
        const int h = (tid & 63) >> 4, r = tid & 15, pos = row0 + r;
        const float* src = tid < 64 ? tr.lse + (((long)layer * a.b + clip) * 4 + h) * Tp : tr.delta + ((long)clip * 4 + h) * Tp;
        Ls[(tid >> 6) * 64 + h * 16 + r] = pos < T ? src[pos] : 0.f;
    }
    __syncthreads();
    const int ldS = Tp + 4;
    float* Sw = Big + wv * NV_R * ldS;
    const float* lse = Ls + wv * 16;
    const float* del = Ls + 64 + wv * 16;
    const DropCtx dc = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_BLOCK(layer, 0), tr.drop_thr, tr.drop_scale);
    nav_mm16(Qs + wv * 32, NV_LD, kg, 32, Tp / 16, 32, 0, 1, [&](int r, int c, float v) {
        Sw[r * ldS + c] = (c < T && row0 + r < T) ? expf(v * NV_SCALE - lse[r]) : 0.f;
    });
    __syncthreads();
    nav_mm16t(Ds + wv * 32, NV_LD, vg, Tp, Tp / 16, 32, 0, 1, [&](int r, int c, float v) {
        const uint32_t idx = (uint32_t)((((long)clip * 4 + wv) * T + row0 + r) * T + c);
        Sw[r * ldS + c] = Sw[r * ldS + c] * (drop_apply(dc, idx, v) - del[r]) * NV_SCALE;
    });
    __syncthreads();
    nav_mm16t(Sw, ldS, kg, 32, 2, Tp, 0, 1, [&](int r, int c, float v) {
        const int pos = row0 + r;
        if (pos < T) tr.g_qkv[((long)clip * T + pos) * 384 + wv * 32 + c] = v;
    });
}

// ---- attention backward, key side -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void navt_attn_dkv(tcdiff_nav_args a, tcdiff_nav_train_args tr, int layer) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;
    float* Vs = Ks + NV_R * NV_LD;
    float* Big = Vs + NV_R * NV_LD;
    const int T = a.dn * a.seq, Tp = (T + 15) & ~15, clip = blockIdx.y, row0 = blockIdx.x * NV_R, tid = threadIdx.x, wv = tid >> 6;
    const long set = (long)a.b * Tp * NV_W, cur = (long)layer * set;
    const float* qg = a.q + cur + (long)clip * Tp * NV_W + wv * 32;
    const float* og = tr.g_o + (long)clip * Tp * NV_W + wv * 32;
    for (int i = tid; i < NV_R * NV_W; i += 256) {
        const int r = i >> 7, c = i & 127, pos = row0 + r, h = c >> 5, d = c & 31;
        Ks[r * NV_LD + c] = pos < T ? a.k[cur + (((long)clip * 4 + h) * Tp + pos) * 32 + d] : 0.f;
        Vs[r * NV_LD + c] = pos < T ? a.vt[cur + (((long)clip * 4 + h) * 32 + d) * Tp + pos] : 0.f;
    }
    __syncthreads();
    const int ldS = Tp + 4;
    float* Sw = Big + wv * NV_R * ldS;
    const float* lse = tr.lse + (((long)layer * a.b + clip) * 4 + wv) * Tp;
    const float* del = tr.delta + ((long)clip * 4 + wv) * Tp;
    const DropCtx dc = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_BLOCK(layer, 0), tr.drop_thr, tr.drop_scale);
    // rows are keys, columns queries: the mask element of (query c, key row0 + r)
    auto midx = [&](int r, int c) { return (uint32_t)((((long)clip * 4 + wv) * T + c) * T + row0 + r); };
    nav_mm16(Ks + wv * 32, NV_LD, qg, NV_W, Tp / 16, 32, 0, 1, [&](int r, int c, float v) {
        Sw[r * ldS + c] = (c < T && row0 + r < T) ? drop_apply(dc, midx(r, c), expf(v * NV_SCALE - lse[c])) : 0.f;
    });
    __syncthreads();
    nav_mm16t(Sw, ldS, og, NV_W, 2, Tp, 0, 1, [&](int r, int c, float v) {
        const int pos = row0 + r;
        if (pos < T) tr.g_qkv[((long)clip * T + pos) * 384 + 256 + wv * 32 + c] = v;
    });
    __syncthreads();
    nav_mm16(Ks + wv * 32, NV_LD, qg, NV_W, Tp / 16, 32, 0, 1, [&](int r, int c, float v) {
        Sw[r * ldS + c] = (c < T && row0 + r < T) ? expf(v * NV_SCALE - lse[c]) : 0.f;
    });
    __syncthreads();
    nav_mm16(Vs + wv * 32, NV_LD, og, NV_W, Tp / 16, 32, 0, 1, [&](int r, int c, float v) {
        const float dl = c < T ? del[c] : 0.f;
        Sw[r * ldS + c] = Sw[r * ldS + c] * (drop_apply(dc, midx(r, c), v) - dl) * NV_SCALE;
    });
    __syncthreads();
    nav_mm16t(Sw, ldS, qg, NV_W, 2, Tp, 0, 1, [&](int r, int c, float v) {
        const int pos = row0 + r;
        if (pos < T) tr.g_qkv[((long)clip * T + pos) * 384 + 128 + wv * 32 + c] = v;
    });
}

// ---- Q / K / V adjoint and LN1 -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void navt_qkv_bwd(tcdiff_nav_args a, tcdiff_nav_train_args tr, int layer) {
    __shared__ __attribute__((aligned(16))) float Qs[NV_R * NV_LD], Ks[NV_R * NV_LD], Vs[NV_R * NV_LD], Ns[NV_R * NV_LD],
        Xs[NV_R * NV_LD], Gs[NV_R * NV_LD], red[1024];
    const int T = a.dn * a.seq, clip = blockIdx.y, row0 = blockIdx.x * NV_R, tid = threadIdx.x, wv = tid >> 6;
    const int lane = tid & 63, lr = lane & 15, lg = lane >> 4;
    const long base = (long)clip * T, lrow = ((long)layer * a.b + clip) * T;
    const float* P = a.blocks + (long)layer * BK_SIZE;
    for (int i = tid; i < NV_R * NV_W; i += 256) {
        const int r = i >> 7, c = i & 127, pos = row0 + r;
        const bool ok = pos < T;
        const float* g = tr.g_qkv + (base + pos) * 384 + c;
        Qs[r * NV_LD + c] = ok ? g[0] : 0.f;
        Ks[r * NV_LD + c] = ok ? g[128] : 0.f;
        Vs[r * NV_LD + c] = ok ? g[256] : 0.f;
        Xs[r * NV_LD + c] = ok ? tr.xs[(lrow + pos) * NV_W + c] : 0.f;
        Gs[r * NV_LD + c] = ok ? tr.gx[(base + pos) * NV_W + c] : 0.f;
    }
    __syncthreads();
    for (int t = wv; t < 8; t += 4) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        nav_mm16t_acc(acc, Qs, NV_LD, P + BK_WQ, NV_W, t * 16, NV_W, NV_W);
        nav_mm16t_acc(acc, Ks, NV_LD, P + BK_WK, NV_W, t * 16, NV_W, NV_W);
        nav_mm16t_acc(acc, Vs, NV_LD, P + BK_WV, NV_W, t * 16, NV_W, NV_W);
#pragma unroll
        for (int i = 0; i < 4; ++i) Ns[(4 * lg + i) * NV_LD + t * 16 + lr] = acc[i];
    }
    __syncthreads();
    const long blk = (long)clip * gridDim.x + blockIdx.x;
    nav_ln16_bwd(Xs, Ns, Gs, P + BK_LN1G, P + BK_LN1B, tr.n1 + (base + row0) * NV_W, T - row0, red, tr.ln_part + blk * 512);
    __syncthreads();
    for (int i = tid; i < NV_R * NV_W; i += 256) {
        const int r = i >> 7, c = i & 127, pos = row0 + r;
        if (pos < T) tr.gx[(base + pos) * NV_W + c] = Gs[r * NV_LD + c];
    }
}

// ---- front: cond_emb and music_projection -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void navt_front_bwd(tcdiff_nav_args a, tcdiff_nav_train_args tr, const float* __restrict__ wm) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr int LO = 68, LH = MU_N + 4;
    float* Es = smem;
    float* Ms = Es + NV_R * LO;
    float* Z2 = Ms + NV_R * LO;
    const int T = a.dn * a.seq, clip = blockIdx.y, row0 = blockIdx.x * NV_R, tid = threadIdx.x, wv = tid >> 6;
    const long tb = (long)clip * T, mb = (long)clip * a.pairs;
    for (int i = tid; i < NV_R * 64; i += 256) {
        const int r = i >> 6, c = i & 63, p = row0 + r;
        float s = 0.f;
        if (p < a.seq)
            for (int d = 0; d < a.dn; ++d) s += tr.gx[(tb + d * a.seq + p) * NV_W + c];
        Es[r * LO + c] = s;
        if (p < a.pairs) tr.g_me[(mb + p) * 64 + c] = s;
    }
    __syncthreads();
    nav_mm16t(Es, LO, wm + MU_WC, 64, 4, 64, wv, 4, [&](int r, int c, float v) {
        const int p = row0 + r, q = p - (a.pairs - a.seq);
        float s = 0.f;
        if (q >= 0 && p < a.pairs)
            for (int d = 0; d < a.dn; ++d) s += tr.g_mpb[(tb + d * a.seq + q) * 64 + c];
        v += s;
        Ms[r * LO + c] = p < a.pairs ? v : 0.f;
        if (p < a.pairs) tr.g_mp[(mb + p) * 64 + c] = v;
    });
    __syncthreads();
    nav_mm16t(Ms, LO, wm + MU_W3, MU_N, MU_N / 16, 64, wv, 4, [&](int r, int c, float v) {
        const int p = row0 + r;
        float g = 0.f;
        if (p < a.pairs) {
            g = v * leaky_grad(tr.mus_z[(mb + p) * (2 * MU_N) + MU_N + c]);
            tr.g_mz[(mb + p) * (2 * MU_N) + MU_N + c] = g;
        }
        Z2[r * LH + c] = g;
    });
    __syncthreads();
    nav_mm16t(Z2, LH, wm + MU_W2, MU_N, MU_N / 16, MU_N, wv, 4, [&](int r, int c, float v) {
        const int p = row0 + r;
        if (p < a.pairs) tr.g_mz[(mb + p) * (2 * MU_N) + c] = v * leaky_grad(tr.mus_z[(mb + p) * (2 * MU_N) + c]);
    });
}

// ---- LSTM backward through time over the clip axis --------------------------------------------------------------------------------------
__global__ __launch_bounds__(768) void navt_lstm_bwd(tcdiff_nav_args a, tcdiff_nav_train_args tr) {
    constexpr int LG = 260, LHH = 68;
    __shared__ __attribute__((aligned(16))) float dGs[3][NV_R][LG];
    __shared__ float dHs[3][NV_R][LHH];
    const int l = threadIdx.x >> 8, j = threadIdx.x & 255, wv = j >> 6, lane = j & 63, lr = lane & 15, lg = lane >> 4;
    const int T = a.dn * a.seq, b = a.b, pos0 = blockIdx.x * NV_R;
    for (int i = j; i < NV_R * LG; i += 256) (&dGs[l][0][0])[i] = 0.f;
    float dcn[4] = {0.f, 0.f, 0.f, 0.f};                     // d c of the clip after this one times its forget gate
    const DropCtx dc = drop_ctx_words(tr.seed0, tr.seed1, TC_SITE_NAV_POS, tr.drop_thr, tr.drop_scale);
    // packed [3][128][256]: row k < 64 = weight_ih column k, row 64 + k = weight_hh column k, both along the 256 gate rows
    const float* w_hh = a.lstm_w + ((long)l * 128 + 64) * 256;
    const float* w_up = a.lstm_w + (long)(l + 1) * 128 * 256;
    __syncthreads();
    for (int tick = 0; tick < b + 2; ++tick) {
        const int t = b - 1 - (tick - (2 - l));
        const bool active = t >= 0 && t < b;
        if (active) {
            f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
            if (l < 2) nav_mm16_acc(acc, &dGs[l + 1][0][0], LG, w_up, 256, wv * 16, 256);
            nav_mm16_acc(acc, &dGs[l][0][0], LG, w_hh, 256, wv * 16, 256);
#pragma unroll
            for (int i = 0; i < 4; ++i) dHs[l][4 * lg + i][wv * 16 + lr] = acc[i];
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = j + 256 * i, r = e >> 6, u = e & 63, pos = pos0 + r;
                if (pos >= T) continue;
                const long row = ((long)l * b + t) * T + pos;
                const float* gs = tr.lstm_gates + row * 256 + u;
                const float gi = gs[0], gf = gs[64], gg = gs[128], go = gs[192];
                const float c = tr.lstm_c[row * 64 + u];
                const float cp = t > 0 ? tr.lstm_c[(row - T) * 64 + u] : 0.f;
                float dh = dHs[l][r][u];
                if (l == 2) {
                    const long o = ((long)t * T + pos) * 64 + u;
                    dh += drop_apply(dc, (uint32_t)o, tr.gx[((long)t * T + pos) * NV_W + 64 + u]);
                }
                const float tc = tanhf(c);
                const float dcell = dh * go * (1.f - tc * tc) + dcn[i];
                dcn[i] = dcell * gf;
                const float di = dcell * gg * gi * (1.f - gi), df = dcell * cp * gf * (1.f - gf);
                const float dg = dcell * gi * (1.f - gg * gg), dO = dh * tc * go * (1.f - go);
                float* ds = &dGs[l][r][u];
                ds[0] = di, ds[64] = df, ds[128] = dg, ds[192] = dO;
                float* gd = tr.g_gates + row * 256 + u;
                gd[0] = di, gd[64] = df, gd[128] = dg, gd[192] = dO;
            }
        }
        __syncthreads();
    }
}

// ---- weight gradients: fixed-order two-stage reductions -----------------------------------------------------------------------------------
struct WgX {                    // X[row][k]: plain (ld), or gathered music rows: row -> (row / gT) * gpairs + goff + (row % gT) % gseq
    const float* X;
    int ld, act;                // act: 0 none, 1 LeakyReLU(0.01), 2 erf-GELU, applied to X while it is read
    int gT, gseq, gpairs, goff;
};

// grid (ceil(Np / 64), ceil(Kv / 64), chunks): wave = one 16-row n tile x 64 columns of k; partial[chunk][Np][Kp] then [Np] bias sums
__global__ __launch_bounds__(256) void navt_wgrad(const float* __restrict__ dY, int ldy, WgX x, long rows, int Nv, int Kv,
                                                  int chunk_rows, float* __restrict__ partial, int Np, int Kp) {
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
    const int nt = blockIdx.x * 4 + wv;
    if (nt * 16 >= Nv) return;
    const int k0 = blockIdx.y * 64, n = nt * 16 + r;
    const long r0 = (long)blockIdx.z * chunk_rows, r1 = r0 + chunk_rows < rows ? r0 + chunk_rows : rows;
    f32x4_t acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float bs = 0.f;
    for (long rb = r0; rb < r1; rb += 4) {
        const long row = rb + g;
        const bool ok = row < r1;
        const float av = (ok && n < Nv) ? dY[row * ldy + n] : 0.f;
        bs += av;
        long xr = row;
        if (x.gT > 0) xr = (row / x.gT) * x.gpairs + x.goff + (int)(row % x.gT) % x.gseq;
        const float* xp = x.X + xr * x.ld;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = k0 + 16 * q + r;
            float xv = (ok && k < Kv) ? xp[k] : 0.f;
            if (x.act == 1) xv = leaky(xv);
            else if (x.act == 2) xv = gelu_erf(xv);
            acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xv, acc[q], 0, 0, 0);
        }
    }
    float* out = partial + (long)blockIdx.z * ((long)Np * Kp + Np);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[(long)(nt * 16 + 4 * g + i) * Kp + k0 + 16 * q + r] = acc[q][i];
    if (blockIdx.y == 0) {
        bs += __shfl_xor(bs, 16);
        bs += __shfl_xor(bs, 32);
        if (g == 0) out[(long)Np * Kp + n] = bs;
    }
}

__global__ __launch_bounds__(256) void navt_wreduce(const float* __restrict__ partial, int chunks, int Nv, int Kv, int Np, int Kp,
                                                    float* __restrict__ gw, int ldo, float* __restrict__ gb,
                                                    float* __restrict__ gb2) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x, nw = (long)Nv * Kv;
    if (i >= nw + Nv) return;
    const long stride = (long)Np * Kp + Np;
    const long src = i < nw ? (i / Kv) * Kp + i % Kv : (long)Np * Kp + (i - nw);
    float s = 0.f;
    for (int c = 0; c < chunks; ++c) s += partial[c * stride + src];
    if (i < nw) gw[(i / Kv) * ldo + i % Kv] = s;
    else {
        if (gb) gb[i - nw] = s;
        if (gb2) gb2[i - nw] = s;
    }
}

// ln_part [nblk][4][128] -> LN1 weight, bias, LN2 weight, bias; a workgroup per 8 columns sums 32 interleaved strands, then those in order
__global__ __launch_bounds__(256) void navt_ln_reduce(const float* __restrict__ part, int nblk, float* __restrict__ g1,
                                                      float* __restrict__ b1, float* __restrict__ g2, float* __restrict__ b2) {
    __shared__ float red[32][8];
    const int c = blockIdx.x * 8 + (threadIdx.x & 7), st = threadIdx.x >> 3;
    float s = 0.f;
    for (int k = st; k < nblk; k += 32) s += part[(long)k * 512 + c];
    red[st][threadIdx.x & 7] = s;
    __syncthreads();
    if (threadIdx.x < 8) {
        float v = 0.f;
        for (int k = 0; k < 32; ++k) v += red[k][threadIdx.x];
        const int col = blockIdx.x * 8 + threadIdx.x, w = col >> 7;
        (w == 0 ? g1 : w == 1 ? b1 : w == 2 ? g2 : b2)[col & 127] = v;
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct Wg {
    const tcdiff_nav_train_args* t;
    hipStream_t stream;
    // d W [Nv][Kv] -> gw, d b -> gb (and gb2) from d Y [rows][ldy] and X
    void operator()(const float* dY, int ldy, WgX x, long rows, int Nv, int Kv, float* gw, float* gb, float* gb2 = nullptr,
                    int ldo = 0) const {
        const int Np = (Nv + 15) & ~15, Kp = (Kv + 63) & ~63;
        int chunks = (int)((rows + 511) / 512);
        chunks = chunks < 1 ? 1 : chunks > TC_NAV_WG_CHUNKS ? TC_NAV_WG_CHUNKS : chunks;
        const int chunk_rows = (int)(((rows + chunks - 1) / chunks + 3) & ~3L);
        navt_wgrad<<<dim3((unsigned)((Np + 63) / 64), (unsigned)(Kp / 64), (unsigned)chunks), dim3(256), 0, stream>>>(
            dY, ldy, x, rows, Nv, Kv, chunk_rows < 4 ? 4 : chunk_rows, t->partial, Np, Kp);
        const long n = (long)Nv * Kv + Nv;
        navt_wreduce<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(t->partial, chunks, Nv, Kv, Np, Kp, gw, ldo ? ldo : Kv, gb,
                                                                                   gb2);
    }
};

template <class Kern>
bool set_smem(Kern k, int bytes, int& ready) {
    if (ready >= bytes) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    ready = bytes;
    return true;
}

}  // namespace

extern "C" int tcdiff_nav_train_bwd(const tcdiff_nav_args* a, const tcdiff_nav_train_args* t, const float* wm, hipStream_t stream) {
    if (!a || !t || !wm || a->b < 1 || a->dn < 1 || a->seq < 1 || a->n_layers < 1 || a->pairs < a->seq) return TCDIFF_ERR_ARG;
    if (a->me_off != 0 || a->mp_off != a->pairs - a->seq) return TCDIFF_ERR_ARG;
    const void* need[] = {a->lstm_w, a->blocks, a->dec, a->mp, a->traj, a->q, a->k, a->vt, t->cond, t->x_in, t->lstm_gates, t->lstm_c,
                          t->lstm_h, t->xs, t->xmid, t->att_o, t->lse, t->hid, t->dec_z, t->mus_z, t->d_out, t->gx, t->g_dec, t->g_mpb,
                          t->g_m, t->g_hid, t->g_a, t->g_o, t->delta, t->g_qkv, t->n1, t->n2, t->ln_part, t->g_me, t->g_mp, t->g_mz,
                          t->g_gates, t->partial, t->grads};
    for (const void* p : need)
        if (!p) return TCDIFF_ERR_ARG;
    if (!al16(a->lstm_w) || !al16(a->blocks) || !al16(a->dec) || !al16(a->q) || !al16(a->k) || !al16(a->vt) || !al16(wm) || !al16(t->g_o))
        return TCDIFF_ERR_ALIGN;
    const int T = a->dn * a->seq, Tp = (T + 15) & ~15, L = a->n_layers, b = a->b;
    if (T > 500) return TCDIFF_ERR_UNSUPPORTED;
    const long R = (long)b * T, P = (long)b * a->pairs;
    static int r_mlp = 0, r_dq = 0, r_dkv = 0, r_front = 0;
    const int s_mlp = (4 * NV_R * NV_LD + NV_R * (NV_HID + 4) + 1024) * 4;
    const int s_dq = (2 * NV_R * NV_LD + 128 + 4 * NV_R * (Tp + 4)) * 4, s_dkv = (2 * NV_R * NV_LD + 4 * NV_R * (Tp + 4)) * 4;
    const int s_front = (2 * NV_R * 68 + NV_R * (MU_N + 4)) * 4;
    if (!set_smem(navt_mlp_bwd, s_mlp, r_mlp) || !set_smem(navt_attn_dq, s_dq, r_dq) || !set_smem(navt_attn_dkv, s_dkv, r_dkv) ||
        !set_smem(navt_front_bwd, s_front, r_front))
        return TCDIFF_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((T + NV_R - 1) / NV_R), (unsigned)b), blk(256);
    const Wg wg{t, stream};
    const WgX none{nullptr, 0, 0, 0, 0, 0, 0};
    auto X = [&](const float* p, int ld, int act) {
        WgX x = none;
        x.X = p, x.ld = ld, x.act = act;
        return x;
    };
    float* G = t->grads;

    // Decoder (traj_model.py:159-167, 194-197)
    navt_dec_bwd<<<grid, blk, 0, stream>>>(*a, *t);
    float* gd = G + TC_NAV_G_DEC(L);
    wg(t->g_dec + 320, 336, X(t->dec_z + 256, 320, 1), R, 2, 64, gd + DC_W4, gd + DC_B4);
    wg(t->g_dec + 256, 336, X(t->dec_z + 128, 320, 1), R, 64, 128, gd + DC_W3, gd + DC_B3);
    wg(t->g_dec + 128, 336, X(t->dec_z, 320, 1), R, 128, 128, gd + DC_W2, gd + DC_B2);
    {
        // the first linear reads [x | music rows of the prediction side]: its weight gradient in two column ranges of row stride 192
        WgX xm = X(a->mp, 64, 0);
        xm.gT = T, xm.gseq = a->seq, xm.gpairs = a->pairs, xm.goff = a->mp_off;
        wg(t->g_dec, 336, X(t->xs + (long)L * R * NV_W, NV_W, 0), R, 128, 128, gd + DC_W1, gd + DC_B1, nullptr, 192);
        wg(t->g_dec, 336, xm, R, 128, 64, gd + DC_W1 + 128, nullptr, nullptr, 192);
    }

    // the blocks, last to first (traj_model.py:62-65, 29-46)
    const int nblk = (int)(grid.x * grid.y);
    for (int l = L - 1; l >= 0; --l) {
        float* gb = G + (long)l * BK_SIZE;
        const long lr = (long)l * R;
        navt_mlp_bwd<<<grid, blk, s_mlp, stream>>>(*a, *t, l);
        wg(t->g_m, NV_W, X(t->hid + lr * NV_HID, NV_HID, 2), R, NV_W, NV_HID, gb + BK_W2, gb + BK_B2);
        wg(t->g_hid, NV_HID, X(t->n2, NV_W, 0), R, NV_HID, NV_W, gb + BK_W1, gb + BK_B1);
        wg(t->g_a, NV_W, X(t->att_o + lr * NV_W, NV_W, 0), R, NV_W, NV_W, gb + BK_WP, gb + BK_BP);
        navt_attn_dq<<<grid, blk, s_dq, stream>>>(*a, *t, l);
        navt_attn_dkv<<<grid, blk, s_dkv, stream>>>(*a, *t, l);
        navt_qkv_bwd<<<grid, blk, 0, stream>>>(*a, *t, l);
        wg(t->g_qkv, 384, X(t->n1, NV_W, 0), R, NV_W, NV_W, gb + BK_WQ, gb + BK_BQ);
        wg(t->g_qkv + 128, 384, X(t->n1, NV_W, 0), R, NV_W, NV_W, gb + BK_WK, gb + BK_BK);
        wg(t->g_qkv + 256, 384, X(t->n1, NV_W, 0), R, NV_W, NV_W, gb + BK_WV, gb + BK_BV);
        navt_ln_reduce<<<dim3(64), blk, 0, stream>>>(t->ln_part, nblk, gb + BK_LN1G, gb + BK_LN1B, gb + BK_LN2G, gb + BK_LN2B);
    }

    // the front: cond_emb (traj_model.py:109-118) and music_projection (:142-148, 184), rows [0, seq) and [pairs - seq, pairs)
    navt_front_bwd<<<dim3((unsigned)((a->pairs + NV_R - 1) / NV_R), (unsigned)b), blk, s_front, stream>>>(*a, *t, wm);
    float* gm = G + TC_NAV_G_MUSIC(L);
    float *gW1 = gm, *gb1 = gW1 + 438 * 876, *gW2 = gb1 + 438, *gb2 = gW2 + 438 * 438, *gW3 = gb2 + 438, *gb3 = gW3 + 64 * 438,
          *gWc = gb3 + 64, *gbc = gWc + 64 * 64;
    wg(t->g_me, 64, X(a->mp, 64, 0), P, 64, 64, gWc, gbc);
    wg(t->g_mp, 64, X(t->mus_z + MU_N, 2 * MU_N, 1), P, 64, 438, gW3, gb3);
    wg(t->g_mz + MU_N, 2 * MU_N, X(t->mus_z, 2 * MU_N, 1), P, 438, 438, gW2, gb2);
    wg(t->g_mz, 2 * MU_N, X(t->cond, 876, 0), P, 438, 876, gW1, gb1);

    // the LSTM (traj_model.py:139, 174), time = the clip axis
    navt_lstm_bwd<<<dim3((unsigned)((T + NV_R - 1) / NV_R)), dim3(768), 0, stream>>>(*a, *t);
    float* gl = G + TC_NAV_G_LSTM(L);
    for (int l = 0; l < 3; ++l) {
        const int in = l == 0 ? 2 : 64;
        float *gih = gl, *ghh = gih + 256 * in, *gbi = ghh + 256 * 64, *gbh = gbi + 256;
        gl = gbh + 256;
        const float* dg = t->g_gates + (long)l * R * 256;
        const WgX xin = l == 0 ? X(t->x_in, 2, 0) : X(t->lstm_h + (long)(l - 1) * R * 64, 64, 0);
        wg(dg, 256, xin, R, 256, in, gih, gbi, gbh);
        // h0 = 0: the first clip contributes nothing, and with one clip the gradient is exactly zero
        wg(dg + (long)T * 256, 256, X(t->lstm_h + (long)l * R * 64, 64, 0), R - T, 256, 64, ghh, nullptr);
    }
    return hipGetLastError() == hipSuccess ? TCDIFF_OK : TCDIFF_ERR_LAUNCH;
}
