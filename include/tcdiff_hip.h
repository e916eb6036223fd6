/* tcdiff_hip.h -- C ABI of libtcdiff_gfx950.so: the MI355X (gfx950) kernels behind TCDiff's denoising hot path.
 *
 * The reference (Da1yuqin/TCDiff) has no FFI: its boundary for this path is the Python class surface
 * `model.model.DanceDecoder` / `model.diffusion.GaussianDiffusion` (TCDiff.py:18-19,76-102).  The host side
 * that mirrors that surface is `tcdiff_amd/{model,diffusion}.py`; every device operation it performs goes
 * through the entry points below (ctypes binding: tcdiff_amd/_lib.py).
 *
 * Conventions
 *   - every function returns 0 (TCDIFF_OK) or a negative error code; nothing is allocated, nothing
 *     synchronises the host; all pointers are caller-owned DEVICE pointers; work is enqueued on `stream`.
 *   - `dtype` selects the arithmetic of GEMM/attention operands: TC_DTYPE_BF16 (bf16 operands,
 *     v_mfma_f32_32x32x16_bf16, fp32 accumulate) or TC_DTYPE_F32 (fp32 operands, v_mfma_f32_32x32x2_f32:
 *     an exact fp32 fma chain -- the parity mode).  "T" below means that element type.  TC_DTYPE_BF16X3 (three GEMM-like
 *     launchers only, see its definition) keeps TC_DTYPE_F32's storage and evaluates products as split-bf16 triples.
 *   - the residual stream, LayerNorm statistics, softmax, FiLM and the diffusion update are always fp32.
 *   - matrices are row-major; `ld*` are leading dimensions in ELEMENTS; operand rows must be 16-byte
 *     aligned and K must be a multiple of 64 (bf16) / 32 (f32) elements (pad with zeros).
 */
#ifndef TCDIFF_HIP_H
#define TCDIFF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define TCDIFF_OK 0
#define TCDIFF_ERR_ARG (-1)
#define TCDIFF_ERR_ALIGN (-2)
#define TCDIFF_ERR_LAUNCH (-3)
#define TCDIFF_ERR_UNSUPPORTED (-4)

#define TC_DTYPE_F32 0
#define TC_DTYPE_BF16 1
#define TC_DTYPE_BF16X3 2 /* tcdiff_gemm_tile (forward epilogues), tcdiff_gemm_rowln, tcdiff_attention only: operands stored as fp32
                             exactly as for TC_DTYPE_F32; every product a b is formed as a_hi b_hi + a_hi b_lo + a_lo b_hi with
                             a_hi = bf16(a), a_lo = bf16(a - a_hi) -- three bf16 MFMAs, fp32 accumulate: ~2^-16 per product, the
                             reference's fp32 path (model/model.py:548-624 runs without autocast) to well inside 1e-3.
                             A 16-byte chunk of four elements is stored as [hi x4 | lo x4], so a T-typed row starts on a
                             chunk: tcdiff_gemm_tile's TC_EPI_STORE_T needs ldc % 4 == 0 (a partial last chunk of N % 4
                             elements is written element by element), tcdiff_convert_pad / tcdiff_step_prologue ld_dst /
                             ld_xin % 4 == 0; TC_ERR_ARG otherwise */

/* activations (fused into GEMM epilogues and elementwise helpers) */
#define TC_ACT_NONE 0
#define TC_ACT_RELU 1
#define TC_ACT_GELU 2 /* exact erf form: F.gelu, TCDiff.py:85 */
#define TC_ACT_MISH 3 /* nn.Mish, model/model.py:157,457 */
#define TC_ACT_SILU 4 /* nn.SiLU, model/model.py:499 */

/* ---- gemm_tile epilogues ------------------------------------------------------------------------ */
#define TC_EPI_STORE_T 0   /* out[m][n] = T(act(acc + bias[n]))                                       */
#define TC_EPI_STORE_F32 1 /* out[m][n] = act(acc + bias[n]) as fp32                                  */
#define TC_EPI_QKV_HEADS 2 /* scatter to the head-major Q / K / V images read by tcdiff_attention     */
#define TC_EPI_ATOMIC_F32 3 /* out[m][n] += acc (fp32 atomics; split-K): only through tcdiff_gemm_splitk */

typedef struct {
    int mode;          /* TC_EPI_* */
    int act;           /* TC_ACT_* */
    float scale_q;     /* QKV: multiplies the Q columns (1/8 = 1/sqrt(d_k), model/model.py:97) */
    const float* bias; /* [N] or NULL */
    void* out;         /* STORE_T: T[M][ldc]; STORE_F32: float[M][ldc]; QKV: Q image */
    void* out_k;       /* QKV: K image    T[n_seq][H][Lp][64]                       */
    void* out_v;       /* QKV: V image    T[n_seq][H][Lp][64]                       */
    int ldc;
    int L, Lp, H;      /* QKV: tokens per sequence (row m -> sequence m / L, token m % L), padded length, heads */
    int n_q, n_k;      /* QKV: columns [0,n_q) are Q, [n_q,n_q+n_k) are K, the rest V (multiples of 128) */
    int tok_off;       /* QKV: added to the token index  */
    int seq_off;       /* QKV: added to the sequence index */
    int k_splits;      /* TC_EPI_ATOMIC_F32: workgroups per output tile (set by tcdiff_gemm_splitk; 0 elsewhere) */
    /* Training step, TC_EPI_STORE_T with act == NONE and N, ldc multiples of the 16-byte chunk: the activation (+ nn.Dropout)
     * that follows / precedes the nn.Linear in the same pass (model/model.py:244,399-400,490-494,522-528 and their autograd).
     *   out2 != NULL   : out = a = T(acc + bias) (kept for the backward), out2[m][n] = T(dropout(act2(a)))
     *   act_src != NULL: the GEMM is the input gradient of the NEXT linear, out = T(T(acc) * mask / (1 - p) * act2'(act_src[m][n]))
     * dropout: counter hash of (drop_seed (DEVICE int[2] or NULL), drop_site, m * N + n); drop_thr = 0 disables it. */
    void* out2; int ldc2;
    const void* act_src; int ld_src;
    int act2;
    const int* drop_seed; int drop_site; uint32_t drop_thr; float drop_scale;
    /* TC_EPI_QKV_HEADS: hgroup > 0 -- the columns of one of Q / K / V hold several images of hgroup heads each (all eight
     * decoder layers' cross-attention K, or V: model/model.py:394-396 evaluated for every layer in one GEMM); image g starts
     * hgroup_stride elements after image g - 1. */
    int hgroup; long hgroup_stride;
    /* small_m != 0: the caller's whole job is small -- tcdiff_gemm_tile may run the product as 32 x 32 tiles with K dealt to the
     * waves (gemm_small_kernel: bf16, TC_EPI_STORE_T / _F32 without out2 / act_src, N % 32 == 0, K % 32 == 0 <= 2048, when the
     * 128 x 128 tiling would leave three quarters of the chip idle).  Another summation order than the 128 x 128 tiling, hence opt-in:
     * with 0 an output element does not depend on how many rows share the launch. */
    int small_m;
} tcdiff_tile_epi;

/* C[M,N] = A[M,K] * W[N,K]^T with epilogue.  If A2 != NULL, output columns >= split_n (a multiple of 128)
 * take their A operand from A2 (same shape/ld as A): one launch computes Q,K from rot(h) and V from h
 * (model/model.py:374-383).  a_mod > 0: A row = m % a_mod.  An operand (rows x ld x element size) must span less than
 * 4 GB: tiles are staged with 32-bit offsets from the operand base (TC_ERR_ARG otherwise; same for tcdiff_gemm_rowln).
 * Replaces: nn.Linear calls model/model.py:78-80,399,454-465,490-494,522-528,560,623,164-166. */
int tcdiff_gemm_tile(int dtype, const void* A, const void* A2, int split_n, const void* W, int M, int N, int K,
                     int lda, int ldw, int a_mod, const tcdiff_tile_epi* epi, hipStream_t stream);

/* ---- gemm_rowln: N = 512, row-complete epilogue ------------------------------------------------- */
#define TC_ROW_BIAS 1       /* v = acc + bias[n]                                                       */
#define TC_ROW_LN_POST 2    /* v = LayerNorm_{ln_eps}(v) * ln_g + ln_b      (SBI_MSA.layer_norm, model/model.py:106) */
#define TC_ROW_FILM 4       /* v = (film[seq][n] + 1) * v + film[seq][512+n] (featurewise_affine, model/model.py:171) */
#define TC_ROW_RES 8        /* v = xres[m][n] + v  (implied by FILM as well)                           */
#define TC_ROW_STORE_X 16   /* xout[m'][n] = v (fp32)                                                  */
#define TC_ROW_NEXT_LN 32   /* u = LayerNorm_{nln_eps}(v) * nln_g + nln_b  (the next block's norm, model/model.py:326,332,338,344) */
#define TC_ROW_STORE_H 64   /* hout[m'][n] = T(u)   (without NEXT_LN: hout[m'][n] = T(v))                      */
#define TC_ROW_STORE_ROT 128 /* rout[m'][n] = T(rotary(u, pos = m' % L))   (model/model.py:375,387)    */

typedef struct {
    int flags;
    const float* bias;
    const float* ln_g;
    const float* ln_b;
    float ln_eps;
    const float* film; /* base of this block's FiLM rows: film[seq * film_ld + n] scale, +512 shift */
    int film_ld;
    const float* xres; /* fp32 [*,512] */
    int xres_mod;      /* > 0: residual row = m % xres_mod */
    float* xout;
    int L;             /* tokens per sequence */
    const float* nln_g;
    const float* nln_b;
    float nln_eps;
    void* hout;
    void* rout;
    const float* rope; /* [Lmax][512]: rope[p][2j] = cos(p*freq_j), rope[p][2j+1] = sin(p*freq_j) */
    int out_mul, out_add; /* output row m' = m * out_mul + out_add (0 -> 1) */
    int groups;           /* > 1: `groups` GEMMs of the same A in one launch; group g takes weight rows
                             [512 g, 512 g + 512), bias[512 g ..] and out_add + g (the per-dancer slices of the last
                             fusion-projection linear, model/model.py:527-528,561) */
} tcdiff_row_epi;

/* out rows[M,512] = epilogue(A[M,K] * W[512,K]^T).  Replaces fc+layer_norm+FiLM+residual
 * (model/model.py:103-106,327,334), linear2+FiLM+residual (:339,399-401), linear3(norm4(x)) (:344) and the
 * last fusion-projection linear (:527), each fused with the LayerNorm(+rotary) that consumes its result. */
int tcdiff_gemm_rowln(int dtype, const void* A, const void* W, int M, int K, int lda, int ldw, int a_mod,
                      const tcdiff_row_epi* epi, hipStream_t stream);

/* ---- training-side rows (forward pieces; csrc/train.hip) -----------------------------------------------------------
 * x_noisy[b][s*dn + d][c] = sqrt_ac[t_b] * x_start[b][d][s][c] + sqrt_1mac[t_b] * noise[b][s][d][c], channels 4 and 5
 * (trajectory) copied from x_start: q_sample + the restore + the (b, dn, S, C) -> (b, S*dn, C) permute of
 * model/diffusion.py:625-634,640-651.  t: int64 [b] on the device. */
int tcdiff_q_sample_traj(const float* x_start, const float* noise, const long* t, const float* sqrt_ac,
                         const float* sqrt_1mac, float* x_noisy, int b, int dn, int S, int C, hipStream_t stream);

/* axis_angle[i * per_row + j][0..2] = matrix_to_axis_angle(rotation_6d_to_matrix(rot6d + i * row_stride + 6 j))
 * (dataset/quaternion.py:28-32; pytorch3d 0.7.1 definitions restated, see oracle/tcdiff_oracle.py): per_row rotations
 * packed in every row of a matrix with `row_stride` floats per row (the 24 x 6 tail of a 151-wide motion row). */
int tcdiff_ax_from_6v(const float* rot6d, long n_rows, int per_row, long row_stride, float* axis_angle,
                      hipStream_t stream);

/* SMPLSkeleton.forward (vis.py:358-406): axis_angle [n][24][3], root [n][3] -> joints [n][24][3].  parents (HOST int[24],
 * a parent precedes its children) and offsets (HOST float[24][3]) are vis.py:48-101's constants or a caller's skeleton. */
int tcdiff_smpl_fk(const float* axis_angle, const float* root, long n, const int* parents, const float* offsets,
                   float* joints, hipStream_t stream);

/* out[b][4] = per-clip means of the reconstruction, velocity, FK and foot-skate terms of model/diffusion.py:668-733
 * (the first three times p2_weight[t_b]); model_out [b][S*dn][C], x_start in the dataset layout [b][dn][S][C],
 * joints_* [b*S*dn][24][3]; l1 != 0 selects F.l1_loss, else F.mse_loss. */
int tcdiff_loss_terms(const float* model_out, const float* x_start, const float* joints_model,
                      const float* joints_target, const float* p2_weight, const long* t, float* out, int b, int dn,
                      int S, int C, int l1, hipStream_t stream);

/* Adan.step (model/adan.py:33-123) over all parameter tensors in one launch: chunks of <= 65536 elements. */
typedef struct {
    float* p;          /* parameter */
    const float* g;    /* gradient */
    float* m;
    float* v;
    float* n_;
    float* pg;         /* prev_grad */
    long n;
} tcdiff_adan_chunk;

typedef struct {       /* Python-side doubles of adan.py rounded to fp32 where they meet a tensor */
    float b1, omb1, b2, omb2, b3, omb3;   /* betas and 1 - beta */
    float cm, cv, cn;                     /* bias corrections 1 / (1 - (1 - beta)^step) */
    float eps, lr, denom;                 /* denom = 1 + weight_decay * lr */
    int first;                            /* bit 0: step == 0 before the call: m, v, n are left untouched (adan.py:71);
                                             bit 1: RESTART of these tensors (adan.py:109-114): m = g, v = 0, n = g^2, then the
                                             parameter update; bit 2: prev_grad is not written (the caller evaluates
                                             restart_cond(state) on the old prev_grad between the two launches) */
} tcdiff_adan_scalars;

int tcdiff_adan_step(const tcdiff_adan_chunk* chunks, int n_chunks, const tcdiff_adan_scalars* scalars,
                     hipStream_t stream);

/* ---- row-block chains (bf16): everything between the two attentions of a decoder layer in ONE launch -------------
 * A block of 64 token rows stays on a CU; only weights stream (tcdiff_amd/csrc/chain.hip).
 *   TC_CHAIN_A      : O_self --fc, LayerNorm(1e-6), FiLM, +x--> x ; norm2, rotary ; w_qs --> Q image (cross-attention)
 *                     replaces model/model.py:103-106,327 and :332,387,78 (+ the 1/sqrt(d_k) of :97)
 *   TC_CHAIN_B      : O_cross --fc, LN, FiLM, +x--> x ; norm3 ; linear1, GELU ; linear2, FiLM, +x ; norm4 ; linear3 --> x' ;
 *                     next layer's norm1 (+rotary) ; w_qs / w_ks / w_vs --> Q, K, V images
 *                     replaces model/model.py:103-106,334,338-339,344,399-401 and the next layer's :326,374-383,78-80
 *   TC_CHAIN_B_LAST : the same up to linear3, whose bf16 rows feed the final projection (model/model.py:623)
 * `wstream`: the chain's weights as ONE linear stream per wave in consumption order, [8 waves][n_stages][4096 B]; a
 * stage is the v_mfma_f32_16x16x32_bf16 A-fragment image of one 32-deep k-step of the 64 (512-wide GEMMs: [n-tile 4][lane
 * group g 4][16 weight rows][16 B], lane group g holding k = 32 ks + 8 PI[g] .. +7 with PI = (0, 3, 1, 2)) or of two k-steps of
 * the 32 (linear1 chunk: [k-step 2][n-tile 2][g][16 rows][16 B]) weight rows wave w consumes; order: fc (16 stages), then for
 * chain A w_qs (16); for chain B four times {linear1 rows 256c+32w.. (8 stages), linear2 k-slice 256c.. (8)}, then
 * linear3 (16), w_qs, w_ks, w_vs of the NEXT layer (16 each).  n_stages = 32 / 144 / 96.  tcdiff_amd/engine.py packs it.
 * Rows: M token rows, L tokens per sequence; FiLM row = m / L, rotary position = m % L; head-major images as
 * TC_EPI_QKV_HEADS (H must be 8).  a_mod / xres_mod > 0: input / residual row = m % mod (layer 0 shares them between
 * the CFG branches).  The fp32 residual stream between chain launches is column-blocked (see the struct).
 *   TC_CHAIN_FULL / TC_CHAIN_FULL_LAST : chain A, then the CROSS-ATTENTION itself (head w on wave w, K / V from the
 *                     fragment-ordered cache images written by tcdiff_pack_kv_frags), then chain B / B_LAST, in one launch:
 *                     per layer the step is  self-attention -> one chain launch.  Stream: chain A's stages followed by
 *                     chain B's (176 / 128 stages); the first fc block uses film, n2_*, the second filmb,
 *                     n3_*; xres / xres_mod feed the first, xout carries x in between. */
#define TC_CHAIN_A 0
#define TC_CHAIN_B 1
#define TC_CHAIN_B_LAST 2
#define TC_CHAIN_FULL 3
#define TC_CHAIN_FULL_LAST 4
#define TC_CHAIN_FRONT 5 /* last fusion linear of one dancer over a block of 64 FRAMES (A = bf16 [M frames][1024], weights
                            rows [512 d, 512 d + 512) of relative_projection_layer.4, K = 1024: 32 stages) -> layer 0's
                            residual input xout (token row = frame dn + d, column-blocked with M dn rows); then layer 0's
                            norm1 (nn_g, nn_b) + rotary and w_qs / w_ks / w_vs (16 stages each) -> Q, K, V images.  M =
                            frames, L = TOKENS per sequence, b3 = all 512 dn biases; wstream = [dn][8 waves][80 stages];
                            grid = blocks x dn.  Replaces model/model.py:526-528,561 and layer 0's :326,374-383,78-80. */

typedef struct {
    int mode, n_stages;
    int M, L, a_mod, xres_mod, H, Lp;
    const void* A;        /* bf16 [*,512]: attention output rows */
    const void* wstream;
    const float* film;    /* FiLM of the attention block, PRE-FOLDED with the post-LayerNorm (SBI_MSA.layer_norm, eps ln_eps)
                             weights g, b in front of it: film[seq * film_ld + n] = g (scale + 1), +512: b (scale + 1) + shift,
                             so that the block's epilogue is x += LN(z) * G + Bv (model/model.py:103-106,171-173,327,334).  The
                             caller folds g, b into the DenseFiLM generator's weights (both rows are linear in its input):
                             tcdiff_amd/engine.py load_weights */
    const float* xres;    /* fp32 residual in: column-blocked (below) with M (xres_mod > 0: xres_mod) rows, or, with
                             xres_rowmajor, plain [*,512] rows (layer 0: written by tcdiff_gemm_rowln) */
    float* xout;          /* fp32 residual out, column-blocked [64][M][8] (chain B: holds x between the blocks, then x') */
    const float* n2_g;    /* the norm that follows: norm2 (chain A) / norm3 (chain B) */
    const float* n2_b;
    const float* rope;    /* cos/sin table of tcdiff_rope_table, column-blocked [64][rope_rows][8] */
    void* q_out;          /* Q image T[n_seq][8][Lp][64] (chain A: cross-attention Q; chain B: next layer's) */
    const float* b1;      /* linear1 bias [1024] */
    const float* film3;   /* FiLM of the feed-forward block, pre-folded with linear2's bias b2: [scale + 1 | b2 (scale + 1) + shift]
                             (model/model.py:339,399-401) */
    const float* n4_g;
    const float* n4_b;
    const float* b3;      /* linear3 bias */
    const float* nn_g;    /* next layer's norm1 */
    const float* nn_b;
    void* k_out;
    void* v_out;
    void* h_out;          /* *_LAST modes: see out_ld */
    int film_ld;
    float ln_eps, n2_eps, n4_eps, nn_eps, scale_q;
    /* TC_CHAIN_FULL*: the cross-attention block */
    const float* filmb;   /* FiLM of the cross-attention block, pre-folded with multihead_attn.layer_norm like `film` */
    const float* n3_g;    /* norm3 */
    const float* n3_b;
    const void* kf;       /* fragment-ordered K cache of this layer: T[n_kv][8 heads][nkt][4][64 lanes][8] */
    const void* vf;       /* fragment-ordered V cache                                                      */
    int n_shared, nkt, Lk; /* kv slot = seq < n_shared ? 0 : seq - n_shared + (n_shared > 0); nkt = ceil(Lk / 32) tiles */
    /* COLUMN-BLOCKED fp32 [rows][512] matrix: element (row, c) at ((c / 8) * rows + row) * 8 + c % 8 -- the 32 rows a
     * wave instruction touches are then one contiguous kilobyte instead of 32 separate 32-byte pieces */
    int xres_rowmajor;     /* 1: xres is a plain row-major [*,512] matrix */
    int rope_rows;         /* rows of the column-blocked rotary table (>= L) */
    int dn;                /* TC_CHAIN_FRONT: dancers */
    int mt;                /* 16-row tiles per row block: 0 = chosen from M and the device's CU count (4 = 64-row blocks when that
                              fills the chip, else 2 or 1: a small job runs on many small blocks), or 1 / 2 / 4 (tests) */
    int out_ld;            /* *_LAST modes: 0 -> h_out = bf16 [M,512] rows of linear3; > 0 -> h_out = fp32 [M][out_ld], the
                              first out_ld columns of linear3 (the caller folded final_layer into its weights and bias:
                              model/model.py:344,623); out_ld % 4 == 0 */
    int nw;                /* waves per workgroup: 0 or 8 = eight waves x 64 output columns; 4 = four waves x 128 columns, one per
                              SIMD (TC_CHAIN_FULL, _FULL_LAST, _FRONT only).  `wstream` must be packed for the same form: per wave
                              stages of 16 nt x 64 lanes x 16 B with nt = 4 (4-KB stages) or 8 (8-KB stages) n-tiles */
    /* ---- round 5: the layer's SELF-attention inside the launch (TC_CHAIN_FULL / _FULL_LAST, nw = 8) ------------------------
     * seq_blocks = 1: row blocks are cut per sequence -- block (s, b) holds rows s L + 16 mt b .. of sequence s only (grid = (M / L)
     * x ceil(L / (16 mt)); no block straddles two sequences, its rows are keys 16 mt b .. of its sequence).
     * sa_q != NULL: instead of reading the attention output `A`, the block computes softmax((Q / 8) K^T) V of its rows itself
     * (model/model.py:97-102; wave = head, online softmax over 32-key tiles as the in-kernel cross-attention) from
     *   sa_q  : the block's Q^T fragments, bf16, as the PREVIOUS launch left them in `qf_out`: [block][8 waves][8 pieces = (row tile
     *           mt < 4, d-step s < 2)][64 lanes][8] -- 8 KB per (block, wave) whatever the launch's rows per block -- scaled by
     *           log2(e) / sqrt(d_k): the in-kernel softmax works in the exp2 domain;
     *   sa_kf, sa_vf : K / V of the layer in the fragment order of tcdiff_pack_kv_frags, bf16 [M / L][8 heads][sa_nkt][4][64][8],
     *           sa_nkt = ceil(L / 32) tiles; keys >= L of the last tile must be finite (the images must start zeroed: a launch
     *           writes the keys it owns, in 16-row blocks one 8-byte half of a V piece per lane).
     * qf_out / kf_out / vf_out != NULL (all three together; requires seq_blocks): the next layer's Q, K, V leave in those formats
     * (written straight from the accumulators: 1-KB pieces per wave instruction) instead of the head-major images q_out / k_out /
     * v_out; out_nkt = the key tiles per (sequence, head) of kf_out / vf_out. */
    int seq_blocks;
    const void* sa_q;
    const void* sa_kf;
    const void* sa_vf;
    int sa_nkt;
    void* qf_out;
    void* kf_out;
    void* vf_out;
    int out_nkt;
} tcdiff_chain_args;

int tcdiff_chain(const tcdiff_chain_args* args, hipStream_t stream);

/* The same decoder layer for SMALL jobs (tcdiff_amd/csrc/chain_split.hip; what TCDiff.py renders: a handful of clips,
 * TCDiff.py:292-303, model/diffusion.py:386-442): FOUR workgroups per 16-row block, each streaming about a third of the layer's
 * weights, as FOUR launches `part` = 1 .. 4 whose boundaries are the exchanges between the four --
 *   1: self-attention of two heads per workgroup (sa_q / sa_kf / sa_vf; without sa_q: the rows of `A`), fc split over K -> p_out
 *   2: sum of p_in; LN, FiLM, +xres -> xout; norm2, rotary; w_qs and cross-attention of two heads; fc split over K   -> p_out
 *   3: sum of p_in; LN, FiLM, +xres -> xout; norm3; linear1 rows 256 c .., GELU, linear2 over those 256              -> p_out
 *   4: sum of p_in; FiLM, +xres; norm4; linear3 (+ the folded final layer) -> xout / h_out; norm1, rotary; Q / K / V fragment images
 * args: as for TC_CHAIN_FULL / TC_CHAIN_FULL_LAST with seq_blocks = 1, nw = 0 / 8, the same 176 / 128-stage `wstream`; the layer's
 * fragment-order outputs (qf_out / kf_out / vf_out) are mandatory unless LAST.  `xres` -> `xout` is NOT in place (parts 2, 3, 4 read
 * whole rows and store quarters: the caller alternates two buffers); p_in / p_out: fp32 [blocks][4][16][512] partial sums, two
 * buffers alternating likewise.  grid = (M / L) * ceil(L / 16) * 4 workgroups: meant for jobs where that fits the chip.
 * part 1 with sa_q and a_mod > 0: sequence s reads the fragment images of sequence s % (a_mod / L) (layer 0 under classifier-free
 * guidance: the stacked branches share x).
 * part = 12: parts 1 and 2 as one launch (no p_in): every member computes the self-attention of all eight heads and the whole fc
 * (more K / V and weight bytes per member, one exchange less: for short sequences).
 * part = 0 (mode TC_CHAIN_FRONT, the 80-stage front stream of any dancer): layer 0's Q / K / V fragment images from the token
 * rows the fusion projection left -- xres: ROW-MAJOR fp32 [M][512] (model/model.py:561 as one [frames][512 dn] product, which is
 * the same memory); nn_g / nn_b / nn_eps: layer 0's norm1; rope; qf_out / kf_out / vf_out / out_nkt; scale_q.  With it a small job
 * runs the fusion projection as plain small products (tcdiff_gemm_tile picks its small-M kernel) and layer 0's self-attention
 * inside part 1, instead of the TC_CHAIN_FRONT launch (9 workgroups for one 3 x 150 clip) and a stand-alone attention. */
int tcdiff_chain_split(const tcdiff_chain_args* args, int part, const float* p_in, float* p_out, hipStream_t stream);

/* Fragment-ordered images of the cross-attention K / V caches for TC_CHAIN_FULL (bf16): for keys key_lo <= key < key_hi
 * of every (slot, head) of Kc / Vc (T[n_slots][H][Lp][64], natural [key][d] rows),
 *   Kf[slot][head][key / 32][(key % 32) / 16][d / 32][16 g + key % 16][jj]  with d % 32 = 16 (jj / 4) + 4 g + jj % 4
 *   Vf[slot][head][key / 32][d / 16][16 g + d % 16][jj]                     with key % 32 = 16 (jj / 4) + 4 g + jj % 4
 * i.e. each 1-KB piece is the 64 lanes' 16-byte v_mfma_f32_16x16x32_bf16 A-operand fragments of one (16-key tile, 32-deep
 * d-step) of K, or (16-d tile, 32-key step) of V^T, in the k order in which the chain kernel's accumulator tiles hold Q^T
 * and P^T (two 16-row tiles, rows 4 g + j of each).  Keys >= Lk inside
 * the last tile must hold finite values (zero).  Run once over [0, Lk) when a cache slot is filled and over the two
 * time-token keys every step. */
int tcdiff_pack_kv_frags(const void* Kc, const void* Vc, void* Kf, void* Vf, int n_slots, int H, int Lp, int nkt,
                         int key_lo, int key_hi, hipStream_t stream);

/* ---- fused attention ------------------------------------------------------------------------------
 * O[(seq*Lq + q)*ldo + head*64 + d] = softmax_k(Q[seq][head][q] . K[kv][head][k]) V[kv][head][k][d]
 * Q  : T[n_seq][H][Lp_q][64]   (already scaled by 1/sqrt(64))
 * K,V: T[n_kv ][H][Lp_k][64]   natural [key][feature] rows (written by TC_EPI_QKV_HEADS / tcdiff_scatter_time_kv)
 * kv = seq < n_shared ? 0 : seq - n_shared + (n_shared > 0)   (the unconditional CFG branch shares one K/V)
 * Lp_q % 128 == 0, Lp_k % 64 == 0, pad rows of Q/K/V must be finite (zero).  Keys >= Lk are masked.
 * ng: query rows per wave of the K/V-resident bf16 kernel in units of 32 (1 or 2); 0 = chosen from the launch size
 * and the device's CU count.  Results do not depend on ng beyond fp32 summation order inside a row.
 * Replaces model/model.py:97-102 (SBI_MSA core) and nn.MultiheadAttention's core (model/model.py:228-236). */
int tcdiff_attention(int dtype, const void* Q, const void* K, const void* V, void* O, int n_seq, int H, int Lq,
                     int Lk, int Lp_q, int Lp_k, int ldo, int n_shared, int ng, hipStream_t stream);

/* ---- LayerNorm (+ rotary) prologue: one wave per 512-wide row ---------------------------------------
 * u = LayerNorm_eps(x[row]) * g + b; optional outputs: h = T(u); rot = T(rotary(u, pos)); y32 = u (fp32).
 * pos = pos_base + (row % pos_mod).  Replaces model/model.py:326 etc. where no producing GEMM can fuse it,
 * norm_cond (:616) and the music encoder's norms (:220-221). */
int tcdiff_ln_rot(int dtype, const float* x, int rows, const float* g, const float* b, float eps, void* h,
                  void* rot, float* y32, const float* rope, int pos_mod, int pos_base, hipStream_t stream);

/* rope[p][2j] = cos(p * freqs[j]), rope[p][2j+1] = sin(p * freqs[j]), p < n_pos, j < 256
 * (model/rotary_embedding_torch.py:115-130 + :58: the table the reference recomputes on every call). */
int tcdiff_rope_table(const float* freqs, float* rope, int n_pos, hipStream_t stream);

/* ---- small elementwise helpers of the step-invariant / per-step conditioning path ----------------- */
/* dst[r][c] = T(src row r)[c] for c < cols, 0 for cols <= c < ld_dst.  Source row r lives at
 * src + (r / rows_per_batch) * batch_stride + (r % rows_per_batch) * row_stride  (strides in floats). */
int tcdiff_convert_pad(int dtype, const float* src, void* dst, int rows, int cols, int ld_dst, int rows_per_batch,
                       long batch_stride, long row_stride, hipStream_t stream);
/* emb[i] = T([sin(t_i * f_k), cos(t_i * f_k)]), k < 256 (SinusoidalPosEmb, model/utils.py:36-48); times int32 */
int tcdiff_sinusoidal(int dtype, const int* times, int n, const float* freq, void* emb, hipStream_t stream);
/* out[b][c] = mean_s x[b][s][c]   (model/model.py:593) */
int tcdiff_mean_pool(const float* x, float* out, int B, int S, int C, hipStream_t stream);
/* out[i][c] = T(act(a[ia[i]][c] + (b ? b[i][c] : 0))), c < 512; ia == NULL -> identity
 * (t = to_time_cond(t_hidden) + cond_hidden; Mish(t): model/model.py:612,157) */
int tcdiff_add_act(int dtype, const float* a, const int* ia, const float* b, int n, int act, void* out,
                   float* out32, hipStream_t stream);
/* per-step: copy the two time-token K/V rows of every layer into the cross-attention caches.
 * tab: T[NL][n_t][2][1024] (K cols 0..511, V cols 512..1023); tidx[seq] selects the row set.
 * Kc, Vc: T[NL][n_kv][H][Lp][64]; rows tok0, tok0+1.  */
int tcdiff_scatter_time_kv(int dtype, const void* tab, int n_t, const int* tidx, void* Kc, void* Vc, int NL,
                           int n_kv, int H, int Lp, int tok0, hipStream_t stream);

/* ---- sampler steps --------------------------------------------------------------------------------
 * step scalars live in DEVICE memory so that one captured hipGraph serves every step:
 *   counter[0] = index of the current step; params[step][8] floats, tseq[step] = timestep index.
 * tcdiff_step_begin: tidx[i] = tseq[counter[0]] for i < n.   tcdiff_step_end: counter[0] += 1.          */
int tcdiff_step_begin(const int* counter, const int* tseq, int* tidx, int n, hipStream_t stream);
int tcdiff_step_end(int* counter, hipStream_t stream);

/* tcdiff_step_prologue: step_begin + add_act(mish) + scatter_time_kv (+ its pack_kv_frags image) + convert_pad of x_t
 * + the counter bump of step_end in ONE launch (model/model.py:606-612 conditioning of a step; model/diffusion.py:245
 * loop variable).  counter is int[4] = {current step, seed0, seed1, next step}; the launch reads counter[3] and writes
 * counter[0] = that step; tcdiff_sampler_update(mode | TC_SAMPLER_ADVANCE) later writes counter[3] = counter[0] + 1,
 * so that no tcdiff_step_end launch is needed.
 * Kc/Vc (row-major caches) or Kf/Vf (fragment images, bf16 only) may be NULL, not both; x may be NULL (no copy); with
 * film_tab the FiLM generator input (film_in) is not produced -- the step needs no FiLM GEMM. */
typedef struct tcdiff_step_prologue_args {
    int* counter;
    const int* tseq;
    int* tidx;            /* [n_seq] <- timestep (kept for the op-by-op kernels) */
    const float* t_base;  /* [n_t][512] time-embedding MLP output per timestep */
    const float* hidden;  /* [n_seq][512] cond hidden rows */
    void* film_in;        /* [n_seq][512] model dtype */
    int n_seq;
    const void* tab;      /* [NL][n_t][2][1024] time-token K|V rows, model dtype */
    int n_t;
    void *Kc, *Vc, *Kf, *Vf;
    int NL, n_kv, H, Lp, nkt, tok0;
    const float* x;       /* [rows][nfeat] fp32 x_t or NULL */
    void* xin;            /* [rows][ld_xin] model dtype, zero padded */
    int rows, nfeat, ld_xin;
    /* FiLM rows from a per-job table instead of a per-step GEMM (NULL: off).  film_tab[n_t][film_rows][nfilm] fp32 holds
     * Linear(Mish(t_base[t] + hidden_j)) of all 24 DenseFiLM blocks (model/model.py:154-168,612) for every timestep row t and
     * every distinct conditioning row j (0 = the null conditioning shared by the unconditional branch, 1 + i = clip i);
     * film_out[seq] <- film_tab[t][seq < n_unc ? 0 : seq - n_unc + 1] for seq < n_seq. */
    const float* film_tab;
    float* film_out;
    int film_rows, nfilm, n_unc;
    /* 0: everything in one launch.  Round 6: the step's first GEMM needs only x_t, the first decoder-layer launch ~110 us later
     * needs the FiLM rows and the time-token rows -- so the captured step launches the prologue in two PARTS, the second on a
     * forked stream beside the input / fusion GEMMs (which leave ~100 CUs idle):
     * TC_PROLOGUE_X    = tidx, the model-dtype copy of x_t, counter[0] <- step;
     * TC_PROLOGUE_COND = the FiLM generator input or the gathered FiLM rows, the time-token K / V rows (it only READS counter[3]). */
    int parts;
} tcdiff_step_prologue_args;
#define TC_PROLOGUE_X 1
#define TC_PROLOGUE_COND 2
int tcdiff_step_prologue(int dtype, const tcdiff_step_prologue_args* a, hipStream_t stream);

/* DDPM: params = {w, coef1, coef2, sigma}  (model/diffusion.py:217-252, model/model.py:546)
 *   x0 = clamp(unc + (cond - unc) * w, -1, 1);  x <- coef1*x0 + coef2*x + sigma*eps
 * DDIM: params = {w, sqrt_recip_ac, sqrt_recipm1_ac, sqrt_ac_next, c, sigma, last}  (model/diffusion.py:195-204,407-431)
 *   x0 = clamp(...); pn = (sqrt_recip_ac*x - x0)/sqrt_recipm1_ac; x <- last ? x0 : sqrt_ac_next*x0 + c*pn + sigma*eps
 * out_unc / out_cond: fp32 [n_rows][ldo] network outputs (out_unc may be NULL when w == 1 is known: x0 = clamp(cond)).
 * eps: fp32 [n_rows][nfeat] or NULL -> Philox4x32-10 normal keyed by (seed, clip0 + row / L, timestep, element);
 *      counter[1], counter[2] are device-side seed words XORed into `seed` (re-seed a captured graph).
 * traj: optional fp32 [n_rows][3]: channels 4,5 of x are overwritten with traj[...,0:2] after the update
 * (model/diffusion.py:427-431).  x is updated in place; x0_out (optional) receives x0. */
#define TC_SAMPLER_DDPM 0
#define TC_SAMPLER_DDIM 1
#define TC_SAMPLER_ADVANCE 0x100 /* OR into mode: also write counter[3] = counter[0] + 1 (pairs with tcdiff_step_prologue) */
int tcdiff_sampler_update(int mode, const float* out_unc, const float* out_cond, int ldo, float* x,
                          const float* eps, const float* traj, float* x0_out, int n_rows, int nfeat, int L,
                          const int* counter, const float* params, const int* tseq, uint64_t seed, int clip0,
                          hipStream_t stream);

/* Constraints re-imposed after a sampler step, as a launch of the captured step (no host callback between steps).
 *   kind 1: x = mask ? value : x unless this is the last step        (ddim_sample_Footwork, model/diffusion.py:341-356)
 *   kind 2: x = (p4 * value + p5 * noise) * mask + (1 - mask) * x    (inpaint_loop's q_sample(value, t-1) blend, :545-551)
 * Bit 1 of (int)params[step][7] enables the step (the host writes "not last" / "t > 0"); columns 4, 5 hold sqrt_ac[t-1],
 * sqrt(1 - ac[t-1]) for kind 2 (DDPM steps, whose own scalars are columns 0..3).  mask: fp32 [mask_rows][nfeat] (row % mask_rows: one [L][nfeat] mask may serve every
 * clip); value, q_eps: fp32 [n_rows][nfeat]; q_eps NULL -> Philox normal (stream word 1, same keying as the step). */
int tcdiff_sampler_constrain(int kind, float* x, const float* mask, int mask_rows, const float* value,
                             const float* q_eps, int n_rows, int nfeat, int L, const int* counter, const float* params,
                             const int* tseq, uint64_t seed, int clip0, hipStream_t stream);

/* tcdiff_window_couple gated by bit 0 of (int)params[step][7] (the reference does not couple after the last step). */
int tcdiff_window_couple_step(float* x, int b, int seq_len, int row_elems, const int* counter, const float* params,
                              hipStream_t stream);

/* y[row][c] = unc + (cond - unc) * w, c < nfeat  (DanceDecoder.guided_forward, model/model.py:546) */
int tcdiff_cfg_combine(const float* out_unc, const float* out_cond, int ldo, float w, float* y, int n_rows,
                       int nfeat, hipStream_t stream);

/* x[1:, :half] = x[:-1, half:] on the (b, seq_len, dn*nfeat) view (model/diffusion.py:502-506,599-601) */
int tcdiff_window_couple(float* x, int b, int seq_len, int row_elems, hipStream_t stream);

/* ---- EMA of the master weights (training-side, model/diffusion.py:61-76 EMA.update_model_average) -------------
 * ma = ma * beta + (1 - beta) * cur over a list of fp32 tensors in ONE launch (the reference issues three elementwise
 * kernels per parameter tensor, 435 tensors).  `chunks` is a DEVICE array: chunk i covers chunks[i].n <= 65536 elements.
 * Rounding as torch's `old * beta + (1 - beta) * new`: two products rounded to fp32, then the sum (no fma). */
typedef struct {
    float* ma;
    const float* cur;
    long n;
} tcdiff_ema_chunk;
int tcdiff_ema_update(const tcdiff_ema_chunk* chunks, int n_chunks, float beta, float one_minus_beta,
                      hipStream_t stream);

/* =====================================================================================================================
 * Training step: train-mode forward pieces and the backward pass (csrc/train_ops.hip, attention_train.hip, gemm.hip).
 * The reference has no backward code: it is torch autograd over model/model.py + model/diffusion.py:636-741, driven by
 * accelerator.backward(total_loss) at TCDiff.py:232.  tcdiff_amd/train_engine.py sequences these launchers as an
 * explicit forward + reverse schedule behind ONE torch.autograd.Function.
 *
 * Gradient dtypes: the gradient of a T-typed activation is T; the gradient of the fp32 residual stream is fp32;
 * parameter gradients are fp32 and ACCUMULATE (+=) into caller-zeroed buffers.
 *
 * Dropout (train mode; model/model.py:98,103,240,244-245,383,396,400-401 and nn.MultiheadAttention's weights) is a
 * counter-based hash of (seed, site, flat element index) -- csrc/train_common.h -- regenerated by the backward kernels.
 * `seed` is a DEVICE int[2] (NULL = {0,0}); drop_thr = floor(p * 2^32) (0 disables), drop_scale = 1 / (1 - p). */
#define TC_SITE_ENC(i, k) (4 * (i) + (k))        /* encoder layer i: k = 0 attention weights, 1 dropout1, 2 inner, 3 dropout2 */
#define TC_SITE_DEC(l, k) (16 + 8 * (l) + (k))   /* decoder layer l: k = 0 self weights, 1 self fc, 2 dropout1, 3 cross
                                                    weights, 4 cross fc, 5 dropout2, 6 inner, 7 dropout3 */

/* dst[r][c] = T(src[r][c]) (c < cols; zeros for cols <= c < cols_pad) and/or dstT[c][r] = T(src[r][c]) (r < rows; zeros
 * for rows <= r < rows_pad), c < cols.  src is fp32 (src_f32 != 0) or T.  colsum (optional, fp32 [cols], caller-zeroed)
 * += sum_r src[r][c]: the bias gradient of an nn.Linear while its dY is being repacked.  Produces the K-contiguous
 * operands tcdiff_gemm_tile needs for dgrad (W^T) and wgrad (dY^T, X^T). */
int tcdiff_cast_transpose(int dtype, int src_f32, const void* src, int rows, int cols, int ld_src, void* dst, int ld_dst,
                          int cols_pad, void* dstT, int ld_dstT, int rows_pad, float* colsum, hipStream_t stream);

/* The same for a table of fp32 matrices in ONE launch -- the operand packs (W as T [N, Kp] and W^T as T [K, Np]) of every
 * nn.Linear, rebuilt from the fp32 master parameters after each optimizer step (the reference's autocast does the
 * equivalent cast per use: accelerate mixed_precision, TCDiff.py:96-104).  `descs_dev` is a DEVICE array; fill each entry's
 * src .. rows_pad, call tcdiff_ct_desc_init (host) for tiles_x / vec and the tile count, and set tile0 to the running sum
 * of the counts; n_tiles = the total. */
typedef struct tcdiff_ct_desc {
    const void* src;                  /* fp32 [rows][ld_src] */
    void* dst;                        /* T [rows][ld_dst], columns cols .. cols_pad zero-filled; or NULL */
    void* dstT;                       /* T [cols][ld_dstT], columns rows .. rows_pad zero-filled; or NULL */
    int rows, cols, ld_src, ld_dst, cols_pad, ld_dstT, rows_pad;
    int tile0, tiles_x, vec;          /* tile0: caller; tiles_x, vec: tcdiff_ct_desc_init */
} tcdiff_ct_desc;
int tcdiff_ct_desc_init(int dtype, tcdiff_ct_desc* d);
int tcdiff_cast_transpose_multi(int dtype, const tcdiff_ct_desc* descs_dev, int n_desc, int n_tiles, hipStream_t stream);

/* ---- row-block GEMM of the training step (bf16; csrc/gemm_rows.hip) -------------------------------------------------
 * C[M, N] = A[M, K] * Wn[N, K]^T with tcdiff_gemm_tile's epilogues, for the tall products inside the decoder layers
 * (K = 512 or 1024, N a multiple of 512): a workgroup keeps 64 / 32 / 16 rows of A in LDS (mt = 4 / 2 / 1; 0 = by M and the
 * CU count) and streams the weights, which arrive as per-wave fragment streams -- the 4-KB stage format of tcdiff_chain:
 * wstream = [8 waves][N / 512 phases x K / 32 stages][4096 B], wave w's stage (p, ks) holding [n-tile 4][lane group 4][16 rows]
 * [8 k] = Wn[512 p + 64 w + 16 nt + c][32 ks + 8 PI(g) + j], PI = (0, 3, 1, 2).  tcdiff_pack_row_streams builds such streams on
 * the device from fp32 matrices: Wn[n][k] = src[n sn + k sk], i.e. (sn, sk) = (ld, 1) for the forward product of an nn.Linear
 * weight [N, K] and (1, ld) for its input gradient (Wn = W^T); an entry may be a piece of the packed matrix (stacked
 * parameters).  descs_dev: DEVICE array; max_elems = the largest N * K in it.
 * A2 / split_n as in tcdiff_gemm_tile (K = 512 only; split_n a multiple of 512).  Epilogue restrictions: act == TC_ACT_NONE,
 * hgroup == 0; TC_EPI_QKV_HEADS: H = 8, n_q and n_k are 0 or 512 and at most 512 columns of V (one phase per image), no
 * tok_off / seq_off, L >= 64; ldc / ldc2 / ld_src multiples of 8 (fp32 output: of 4).  Returns TC_ERR_UNSUPPORTED for shapes it
 * does not take (the caller then uses tcdiff_gemm_tile).
 * Replaces in the training step: nn.Linear forward and input-gradient products of model/model.py:78-80,103,399-401,344. */
typedef struct tcdiff_ws_desc {
    const float* src;
    void* dst;
    long sn, sk;                      /* element strides of Wn's n and k in src */
    int N, K;                         /* this piece: N % 512 == 0, K % 32 == 0 */
    int np_dst, p0, kst_dst, ks0;     /* dst is a stream of np_dst phases x kst_dst stages per wave; the piece's phase p, k-step ks
                                         land at (p0 + p, ks0 + ks).  A whole matrix: np_dst = N / 512, kst_dst = K / 32, p0 = ks0 = 0 */
} tcdiff_ws_desc;
int tcdiff_pack_row_streams(const tcdiff_ws_desc* descs_dev, int n_desc, int max_elems, hipStream_t stream);
int tcdiff_gemm_rows(const void* A, const void* A2, int split_n, const void* wstream, int M, int N, int K, int lda,
                     const tcdiff_tile_epi* epi, int mt, hipStream_t stream);

/* Split-K GEMM with fp32 accumulation into `out`: out[m][n] += sum_k A[m][k] W[n][k] (atomic adds; `splits` workgroups
 * share each 128x128 tile).  The weight gradient dW[N,K] += dY^T X of every nn.Linear, with M = out features, N = in
 * features and the contraction over the token rows. */
int tcdiff_gemm_splitk(int dtype, const void* A, const void* W, int M, int N, int K, int lda, int ldw, float* out,
                       int ldc, int splits, hipStream_t stream);

/* The weight gradient without transposed copies: out[m][n] += sum_k A[k][m] B[k][n], A = dY [tokens][lda], B = X
 * [tokens][ldb] as the forward left them (token-major).  M, N multiples of 128, K (tokens) a multiple of the k-tile (64
 * bf16 / 32 f32), else TC_ERR_UNSUPPORTED and the caller goes through tcdiff_cast_transpose + tcdiff_gemm_splitk.
 * Autograd of nn.Linear's weight in the reference (torch addmm backward; model/model.py:78-80,103,399-401). */
int tcdiff_gemm_tn(int dtype, const void* A, const void* B, int M, int N, int K, int lda, int ldb, float* out, int ldc,
                   int splits, hipStream_t stream);

/* Several weight gradients in ONE launch: out_i[m][n] += sum_k A_i[k][m] B_i[k][n] for i < n_prob <= TC_TN_MAX_PROB, each
 * with tcdiff_gemm_tn's shape rules.  The (tile, k-tile) work units of all problems are cut into equal contiguous shares,
 * one workgroup per CU: every CU runs the same number of k-tiles and a tile is added (fp32 atomics) once per share that
 * touches it.  `probs` is a HOST array (copied into the kernel arguments); fill A .. ldc, the rest is the launcher's.
 * The backward of a decoder layer queues its seven weight gradients and flushes them here (train_engine.py). */
#define TC_TN_MAX_PROB 16
typedef struct {
    const void* A; const void* B; float* out;      /* A [K][lda] (dY), B [K][ldb] (X), out [M][ldc] fp32 */
    int M, N, K, lda, ldb, ldc;
    int nk, unit0;                                  /* set by tcdiff_gemm_tn_grouped */
} tcdiff_tn_problem;
typedef struct {
    int n_prob, total_units, units_per_wg, kc;      /* kc: k-tiles per chunk of the unit order */
    tcdiff_tn_problem p[TC_TN_MAX_PROB];
} tcdiff_tn_group;
int tcdiff_gemm_tn_grouped(int dtype, const tcdiff_tn_problem* probs, int n_prob, hipStream_t stream);

/* x[m][c] = dropout(x[m][c] + pe[m % pos_mod][c]) in place on fp32 rows [rows][cols] (cols % 4 == 0); pe == NULL: dropout only;
 * drop_thr == 0: the addition only.  Hash index = m * cols + c (the index tcdiff_act_drop_bwd uses, which carries the backward).
 * Replaces PositionalEncoding.forward in train mode, model/utils.py:27-32 as called at model/model.py:564,580 (use_rotary=False). */
int tcdiff_pos_drop(float* x, int rows, int cols, const float* pe, int pos_mod, const int* seed, int site, uint32_t drop_thr,
                    float drop_scale, hipStream_t stream);

/* y = T(dropout(act(a)))  /  da = dy * mask / (1 - p) * act'(a).  a, da: fp32 (a_f32 != 0) or T [rows][ld_a]; y, dy:
 * T [rows][ld_y]; columns >= cols of y / da are written as zeros up to the leading dimension.  Hash index = r * cols + c.
 * Replaces the activations + nn.Dropout of model/model.py:244,400 (GELU), :490-494,522-528 (ReLU), :454-458,157 (Mish),
 * :496-501 (SiLU) and their autograd. */
int tcdiff_act_drop(int dtype, int a_f32, const void* a, int ld_a, void* y, int ld_y, int rows, int cols, int act,
                    const int* seed, int site, uint32_t drop_thr, float drop_scale, hipStream_t stream);
int tcdiff_act_drop_bwd(int dtype, int a_f32, const void* a, int ld_a, const void* dy, int ld_y, void* da, int rows,
                        int cols, int act, const int* seed, int site, uint32_t drop_thr, float drop_scale,
                        hipStream_t stream);

/* The row-local glue between two GEMMs of a transformer block, forward and backward, one wave per 512-wide row:
 *   u = dropout_pre(z + bias);  y = dropout_post(LayerNorm_post(u));  v = (scale + 1) y + shift;  xn = xres + v;
 *   hn = LayerNorm_next(xn);  rot = rotary(hn, pos)                      (each stage optional: TC_ROWF_* flags)
 * = model/model.py:103-106 (fc dropout + layer_norm), :327,334,339 (dropout1..3 + featurewise_affine + residual),
 *   :326,332,338,344 (the next norm), :375,387-388 (rotary); encoder :220-221,240,245.
 * Backward (tcdiff_row_bwd) recomputes the forward from (z, xres) and returns d_z (T), d_xres (fp32), per-sequence FiLM
 * gradients (atomic += into d_film) and the LayerNorm / bias gradients -- either per-block partial sums in `partials`
 * ([grid blocks][5][512] fp32: d_bias, d_ln_g, d_ln_b, d_nln_g, d_nln_b), folded by tcdiff_row_param_reduce in a fixed
 * order, or atomic += into g_bias .. g_nln_b. */
#define TC_ROWF_BIAS 1
#define TC_ROWF_DROP_PRE 2
#define TC_ROWF_LN_POST 4
#define TC_ROWF_DROP_POST 8
#define TC_ROWF_FILM 16
#define TC_ROWF_RES 32
#define TC_ROWF_STORE_X 64
#define TC_ROWF_NEXT_LN 128
#define TC_ROWF_STORE_H 256    /* hout = T(hn), or T(xn) without NEXT_LN */
#define TC_ROWF_STORE_ROT 512
typedef struct {
    int flags, M, L;           /* rows; rows per sequence (FiLM row = m / L); M % L == 0 */
    const float* z;            /* fp32 [M][512] */
    const float* bias;
    const float* ln_g; const float* ln_b; float ln_eps;
    const float* film; int film_ld;   /* film[seq * film_ld + c] scale, + 512 shift */
    const float* xres;
    float* xout;
    const float* nln_g; const float* nln_b; float nln_eps;
    void* hout; void* rout;
    const float* rope; int pos_mod, pos_base;   /* rotary position = pos_base + m % pos_mod */
    const int* seed; uint32_t drop_thr; float drop_scale; int site_pre, site_post;
    /* backward only */
    const float* d_xn;         /* fp32 [M][512] or NULL: gradient reaching xn through the residual path of the next block */
    const void* d_h;           /* T [M][512] or NULL */
    const void* d_rot;         /* T [M][512] or NULL */
    void* d_z;                 /* T [M][512] */
    float* d_xres;             /* fp32 [M][512] (TC_ROWF_RES) */
    float* d_film; int dfilm_ld;
    float* partials; int chunks;   /* grid = chunks x (M / L) blocks; partials [chunks * M / L][5][512] */
    int dz_f32;                /* != 0: d_z is fp32 (its consumer is not a GEMM: pooled / memory rows of the conditioning path) */
    /* or, instead of `partials` + tcdiff_row_param_reduce: each block adds its sums straight into the gradients (fp32
     * [512] each, NULL = skip; 512 consecutive atomics per block and vector).  g_bias = column sums of d_z: the bias
     * gradient of the nn.Linear that produced z. */
    float* g_bias; float* g_ln_g; float* g_ln_b; float* g_nln_g; float* g_nln_b;
} tcdiff_row_args;
int tcdiff_row_fwd(int dtype, const tcdiff_row_args* a, hipStream_t stream);
int tcdiff_row_bwd(int dtype, const tcdiff_row_args* a, hipStream_t stream);
/* dst[k][c] += sum_blocks partials[blk][k][c] for the non-NULL dst[k], k < 5 */
int tcdiff_row_param_reduce(const float* partials, int n_blocks, float* d_bias, float* d_ln_g, float* d_ln_b,
                            float* d_nln_g, float* d_nln_b, hipStream_t stream);

/* Train-mode attention: as tcdiff_attention (one K/V per sequence), plus dropout on the softmax weights
 * (model/model.py:98; nn.MultiheadAttention dropout) and lse[seq][H][Lp_q] = log2 sum_k 2^(s log2 e) for the backward. */
/* O_lo (bf16 mode, optional): a second token-major image, bf16(o - float(bf16(o))) of the fp32 output o -- with it the backward's
 * delta_i = sum_d dO_id O_id is taken from O + O_lo (16 bits of O instead of 8).  Round 6 found why it matters: delta enters
 * dS = P (dP - delta), a cancellation, and 8-bit O alone put the decoder's self-attention w_qs / w_ks gradients at twice the error the
 * operand rounding of the step explains (tests/test_train_step_gpu.py, oracle._AttnKernelDelta). */
/* Padding and workspaces of both calls (enforced bit for bit by tests/test_attn_train_f64_gpu.py):
 *   - the pad rows of the Q', K and V images (rows Lq .. Lp_q - 1, Lk .. Lp_k - 1) may hold ANY FINITE values: every key past Lk is
 *     masked by a select and no row past Lq is stored.  Not Inf or NaN: a masked weight of zero times Inf is NaN;
 *   - the pad rows of the dO image must be ZERO (the only padding the backward requires to be zero);
 *   - lse is written at [seq][head][0 .. Lq - 1] only; its pad slots are neither written nor used, whatever they hold;
 *   - delta is a pure workspace: it needs no initialisation (NaN-filled is fine), is written at [0 .. Lq - 1] per (seq, head) before
 *     it is read, and its pad slots are neither written nor used;
 *   - O, O_lo, dQ, dK, dV are written at their Lq (Lk) rows x 64 H columns only: columns up to the leading dimension and rows
 *     beyond the last sequence are left alone.
 * Lp_q % 128 == 0; Lp_k % 64 == 0 for the forward, % 128 for the backward. */
int tcdiff_attention_train(int dtype, const void* Q, const void* K, const void* V, void* O, void* O_lo, float* lse, int n_seq,
                           int H, int Lq, int Lk, int Lp_q, int Lp_k, int ldo, const int* seed, int site, uint32_t drop_thr,
                           float drop_scale, hipStream_t stream);
/* Backward of the above (P is recomputed from Q, K and lse; the dropout bits are regenerated).  dO: head-major image
 * T[n_seq][H][Lp_q][64] (zero pad rows); O: token-major T as written by the forward.  Outputs are token-major T:
 *   dQ[(seq Lq + q) ld_dq + head 64 + d] (times scale_q: the gradient with respect to the UNSCALED projection),
 *   dK[(seq Lk + k) ld_dkv + head 64 + d], dV likewise.   delta: fp32 workspace [n_seq][H][Lp_q].  O_lo: the forward's second
 * image or NULL (delta from the 8-bit O alone).
 * Two launches (query-major for dQ, key-major for dK / dV): no atomics, bitwise reproducible. */
int tcdiff_attention_bwd(int dtype, const void* Q, const void* K, const void* V, const void* O, const void* O_lo,
                         const void* dO,
                         const float* lse, float* delta, void* dQ, int ld_dq, void* dK, void* dV, int ld_dkv, int n_seq,
                         int H, int Lq, int Lk, int Lp_q, int Lp_k, int ldo, float scale_q, const int* seed, int site,
                         uint32_t drop_thr, float drop_scale, hipStream_t stream);

/* small fp32 helpers of the conditioning path and their adjoints */
/* out[r][c] = a[r * ld_a + c] + b[r * ld_b + c], c < cols */
int tcdiff_add_rows(const float* a, int ld_a, const float* b, int ld_b, float* out, int ld_out, int rows, int cols,
                    hipStream_t stream);
/* out[b] = keep[b] ? x[b] : nul (broadcast), rows of `n` floats  (torch.where(keep_mask, ., null_*), model/model.py:585-589,609-610) */
int tcdiff_select_rows(const float* x, const float* nul, const unsigned char* keep, float* out, int B, long n,
                       hipStream_t stream);
/* dx[b] = keep[b] ? g[b] : 0 (dx may be NULL);  dnul += sum over not-kept b of g[b] (caller-zeroed, may be NULL) */
int tcdiff_select_rows_bwd(const float* g, const unsigned char* keep, float* dx, float* dnul, int B, long n,
                           hipStream_t stream);
/* dx[b][s][c] = g_tok[b][s][c] (NULL = 0) + g_pool[b][c] / S: adjoint of {tokens used as they are, tokens.mean(-2)} */
int tcdiff_pool_bwd(const float* g_tok, const float* g_pool, float* dx, int B, int S, int C, hipStream_t stream);

/* out[k] = coef[k] * mean_b terms[b][k] for the four terms of tcdiff_loss_terms (coef = 0.636, 2.964, 0.646, 10.942),
 * out[4] = their sum (model/diffusion.py:735-741). */
int tcdiff_loss_total(const float* terms, int b, float* out, hipStream_t stream);

/* d total / d model_out and d total / d joints_model of the four loss terms (model/diffusion.py:668-741) for
 * total = 0.636 mean_b recon + 2.964 mean_b vel + 0.646 mean_b fk + 10.942 mean_b foot times `gscale` (the incoming
 * gradient of the scalar).  d_out [b][S*dn][C] receives the reconstruction + velocity part (every element written);
 * d_joints [b*S*dn][24][3] the FK + foot part (every element written). */
int tcdiff_loss_terms_bwd(const float* model_out, const float* x_start, const float* joints_model,
                          const float* joints_target, const float* p2_weight, const long* t, const float* gscale,
                          float* d_out, float* d_joints, int b, int dn, int S, int C, int l1, hipStream_t stream);
/* Reverse of tcdiff_ax_from_6v + tcdiff_smpl_fk for the model branch: d_joints -> += d_out[row][4..6] (root) and
 * += d_out[row][7 + 6 j ..] (6-D rotations); motion rows [n][C]. */
int tcdiff_fk_bwd(const float* motion, const float* d_joints, long n, int C, const int* parents, const float* offsets,
                  float* d_out, hipStream_t stream);

/* ---- render-time pose export (csrc/export.hip) ----------------------------------------------------------------------
 * The post-processing of GaussianDiffusion.render_sample (model/diffusion.py:811-988) up to the arrays it pickles:
 * samples [b][S * dn][151] (row = frame * dn + dancer; 4 contacts, 3 root, 24 x 6 rotation) are clipped to [-1, 1] and
 * un-normalised with the min-max scaler's scale_ / min_ [151] (dataset/preprocess.py:39-43, dataset/scaler.py:80-83), the
 * rotations go 6-D -> axis-angle (dataset/quaternion.py:28-32), and SMPLSkeleton.forward (vis.py:358-406) gives the joints.
 *   TC_EXPORT_NORMAL: every clip on its own; P = b * S * dn poses, pose p = sample row p; contact [P][4] is written.
 *   TC_EXPORT_LONG:   b half-overlapping windows of one song stitched as model/diffusion.py:841-897 does: roots
 *                     cross-faded (fade_out * p_i + fade_in * p_{i+1}), rotations slerped (dataset/quaternion.py:35-71)
 *                     with weight linspace(0, 1, S / 2); P = (S + (b - 1) S / 2) * dn poses, frame-major / dancer-minor;
 *                     S even; `fade` (DEVICE float [S]) holds torch.linspace(0, 1, S / 2) then torch.linspace(1, 0, S / 2)
 *                     in float32; contact is not written (the reference drops contacts in this mode) and may be NULL.
 * Outputs (DEVICE fp32): smpl_trans [P][3], smpl_poses [P][24][3] axis-angle, full_pose [P][24][3] joint positions.
 * parents (HOST int[24], a parent precedes its children) / offsets (HOST float[24][3]) as tcdiff_smpl_fk.
 * TC_ERR_ARG for a NULL pointer, b < 1, S < 1, dn < 1, an unknown mode, or a LONG job with an odd S. */
#define TC_EXPORT_NORMAL 0
#define TC_EXPORT_LONG 1
int tcdiff_pose_export(const float* samples, int b, int S, int dn, int mode, const float* scale, const float* min_,
                       const float* fade, const int* parents, const float* offsets, float* smpl_trans, float* smpl_poses,
                       float* full_pose, float* contact, hipStream_t stream);

/* ---- motion ingest (csrc/ingest.hip) -----------------------------------------------------------------------------------
 * The motion side of AIOZDataset.process_dataset (dataset/group_dataset.py:167-238), the inverse of tcdiff_pose_export:
 * pos [clips][dn][sq][3] root positions and q [clips][dn][sq][72] axis-angle rotations (DEVICE fp32, Y-up, never written)
 * -> feats [clips][dn][sq][151] = [contacts 4 | root 3 | 6-D 24 x 6], normalised to [-1, 1].  Two launches, no host
 * synchronisation, for any number of clips:
 *   per pose: joint 0's rotation with 90 degrees about x on the left (:184-191), the root position rotated the same way
 *             (:195-198), SMPLSkeleton.forward (:201, vis.py:358-406), ax_to_6v of all 24 joints (:210,
 *             dataset/quaternion.py:21-25), the four foot joints to `feet` [clips * dn * sq][4][3] (workspace);
 *   per clip: contacts = |feet[t + 1] - feet[t]| < 0.01 along one dancer's frames, 1 on the last frame (:204-207);
 *             fit != 0: a Normalizer fitted on THIS clip's dn * sq rows (:217-218, dataset/scaler.py:50-70) -- stats
 *                       [clips][4][151] receives data_min_, data_max_, scale_ = 2 / range (range < 10 eps -> 1) and
 *                       min_ = -1 - data_min_ * scale_; scale / min_ are not read;
 *             fit == 0: scale / min_ (DEVICE float [151]) are used for every clip (:219-220); stats is not written;
 *             then x * scale_ + min_ as two rounded operations, clipped to [-1, 1] (:221, dataset/scaler.py:73-78).
 * raw (optional, as feats): the un-normalised features.  parents / offsets as tcdiff_smpl_fk.
 * TC_ERR_ARG for a NULL pointer (raw excepted; stats / scale / min_ as the mode needs them), clips, dn or sq < 1, or a
 * parent that does not precede its child. */
int tcdiff_motion_ingest(const float* pos, const float* q, int clips, int dn, int sq, const int* parents, const float* offsets,
                         int fit, const float* scale, const float* min_, float* feats, float* raw, float* feet, float* stats,
                         hipStream_t stream);

/* ---- motion quality metrics (csrc/metrics.hip) -------------------------------------------------------------------------
 * Sample-level physical metrics of joint positions in metres, e.g. tcdiff_pose_export's full_pose.  All arithmetic is float64 on
 * the float32 inputs (a difference of two float32 values is exact), comparisons promote the float32 value; two launches (per
 * frame, per sequence), no host synchronisation, no atomics, every sum in a fixed order: same input, same bits.
 * joints (b, dn, T, 24, 3) fp32 DEVICE, element (c, d, t, j, k) at joints[c * joint_strides[0] + d * joint_strides[1] +
 * t * joint_strides[2] + 3 j + k] (HOST long[3] element strides; the trailing 24 x 3 contiguous; read in place).
 * contacts (optional) (b, dn, T, 4) fp32 DEVICE by contact_strides the same way, feet 7, 8, 10, 11.  beats (optional) [b][T]
 * uint8 DEVICE, non-zero = a music beat on that motion frame.  Per clip c and dancer d, J[t][j] = joint j at frame t:
 *   pfc [b][dn]             EDGE's physical foot contact score, unscaled: rv[t] = (J[t+1][0] - J[t][0]) / D, ra[t] =
 *                           (rv[t+1] - rv[t]) / D (D = 1 / fps, t < T - 2) with its `up` component max(., 0); a = |ra|, A = max_t a;
 *                           fv[t][k] = |(J[t+2][f] - J[t+1][f]) without `up`| for f = 7, 10, 8, 11;
 *                           mean_t min(fv0, fv1) min(fv2, fv3) a[t] / A.  A == 0 -> 0; T < 3 -> NaN.
 *   contact_slide / contact_break [b][dn], contact_frames [b][dn] (long)      only with contacts: over (t < T - 1, foot k) with
 *                           contacts[t][k] > contact_threshold and delta = |J[t+1][f] - J[t][f]|: the mean delta, the share with
 *                           delta >= still, the count.  A zero count gives 0 for both.
 *   collision_rate [b]      share of (frame, unordered dancer pair) with root distance without `up` < radius; dn == 1 -> 0.
 *   beat_align [b][dn], motion_beats [b][dn] (long)      only with beats: v[t] = mean_j |J[t+1][j] - J[t][j]| (t < N = T - 1),
 *                           s = scipy.ndimage.gaussian_filter1d(v, sigma_smooth) (radius int(4 sigma + 0.5), weights
 *                           exp(-x^2 / 2 sigma^2) normalised, mode "reflect" of period 2 N also where the radius exceeds N);
 *                           motion beats M = strict interior local minima of s, |M| to motion_beats; Bailando's score
 *                           mean over music beats m of exp(-min_M (m - .)^2 / (2 sigma_beat^2)); NaN without music or motion beats.
 * Workspaces (DEVICE, contents undefined before and after): ws TC_METRICS_WS_PLANES * b dn T doubles, iws TC_METRICS_IWS_PLANES *
 * b dn T ints.  Outputs DEVICE double / long; those of an absent input are not written and may be NULL.
 * TC_ERR_ARG for a NULL required pointer, b, dn or T < 1, up outside 0..2, fps, sigma_smooth or sigma_beat not > 0;
 * TC_ERR_UNSUPPORTED for a filter radius above TC_METRICS_MAX_RADIUS. */
#define TC_METRICS_WS_PLANES 11
#define TC_METRICS_IWS_PLANES 3
#define TC_METRICS_MAX_RADIUS 512
int tcdiff_motion_metrics(const float* joints, const long* joint_strides, const float* contacts, const long* contact_strides,
                          const unsigned char* beats, int b, int dn, int T, int up, double fps, double contact_threshold,
                          double still, double radius, double sigma_smooth, double sigma_beat, double* ws, int* iws, double* pfc,
                          double* contact_slide, double* contact_break, long* contact_frames, double* collision_rate,
                          double* beat_align, long* motion_beats, hipStream_t stream);

/* ---- set-level metrics (csrc/set_metrics.hip) ------------------------------------------------------------------------------
 * Bailando's kinetic features of joint positions, and FID_k / Div_k of a set of feature rows against a reference set.  float64
 * arithmetic on the inputs, no contraction, no atomics, no host synchronisation (tcdiff_set_check excepted: that is its purpose);
 * every sum over frames or rows is taken as: thread i of 256 adds elements i, i + 256, ... in index order, then a fixed tree;
 * sums over the D columns run in index order.  Same input, same bits.
 *
 * tcdiff_kinetic_features, one launch.  joints (b, dn, T, 24, 3) fp32 DEVICE read in place through joint_strides exactly as
 * tcdiff_motion_metrics reads it.  feats [b][dn][72] double DEVICE, column 3 j + k of joint j.  With D = 1 / fps, w = window,
 * d[t] = J[t][j] - J[t-1][j] (exact in float64), per frame i = 1 .. T - 1:
 *   v_i = (sum of d[s] over s = i - w .. i + w with s - 1 >= 0 and s <= T - 1, ascending) / (count * D)
 *   a_i = (sum of (d[s+1] - d[s]) / D^2 over s = i - w .. i + w with s - 1 >= 0 and s + 1 <= T - 1, ascending) / count
 *   k = 0: mean_i |v_i without its `up` component|^2;  k = 1: mean_i (the `up` component of v_i)^2;  k = 2: mean_i |a_i|,
 * mean_i = the sum over the T - 1 frames divided by T - 1.  T < 3: all 72 values NaN.
 * TC_ERR_ARG for a NULL pointer, b, dn or T < 1, up outside 0..2, window < 1 (an acceleration window would be empty at the last
 * frame) or fps not > 0.
 *
 * tcdiff_set_stats, two launches.  feats [N][D] double DEVICE, N >= 2, 1 <= D <= TC_SET_MAX_D.
 *   fit != 0: mean[c] = sum_n x[n][c] / N and std[c] = sqrt(sum_n (x[n][c] - mean[c])^2 / N) are WRITTEN; fit == 0: they are READ.
 *   z[c][n] = (x[n][c] - mean[c]) / (std[c] + 1e-10);  mu[c] = sum_n z[c][n] / N;  zc[c][n] = z[c][n] - mu[c]  (both [D][N], workspaces
 *   that tcdiff_set_scores does not need);  cov[i][j] = cov[j][i] = sum_n zc[i][n] zc[j][n] / (N - 1), [D][D].
 *   div_rows (optional, [N]): div_rows[i] = sum_{j > i} |z[.][i] - z[.][j]|, the squares added over the columns in index order.
 * TC_ERR_ARG for a NULL pointer (div_rows excepted), N < 2 or D < 1; TC_ERR_UNSUPPORTED for D > TC_SET_MAX_D.
 *
 * tcdiff_set_scores, one launch of one workgroup.  ref_mu [D], ref_cov [D][D] (S1), mu, cov (S2) and div_rows [M] as
 * tcdiff_set_stats leaves them.  div[0] = sum_i div_rows[i] / (M (M - 1) / 2).
 *   fid[0] = |mu - ref_mu|^2 + tr S1 + tr S2 - 2 sum_i r(l_i):  S1 = V diag(w) V^T,  R = V diag(r(w)) V^T,  l = the eigenvalues of
 *   (R S2 R + its transpose) / 2,  r(x) = sqrt(x) if x > D 2^-52 max(x_max, 0) else 0, x_max the largest eigenvalue of that
 *   decomposition.  Both decompositions: Jacobi rotations in round-robin order (D rounded up to even; that many minus one steps of
 *   disjoint pairs per sweep), all angles of a step taken from the matrix before it, column rotations, then row rotations, then the
 *   rotated 2 x 2 blocks in closed form; a pair with |a_pq| <= 2^-60 sqrt(|a_pp a_qq|) is left alone; a sweep without a rotation
 *   ends it.  Three D x (D | 1) double matrices live in LDS: 3 * 72 * 73 * 8 = 126144 bytes at D = 72, the limit TC_SET_MAX_D.
 *   status (DEVICE int[3]): {failed, sweeps of the first decomposition, of the second}, a sweep count -1 where max_sweeps
 *   (1 .. TC_SET_MAX_SWEEPS) sweeps all rotated; then failed = 1 and fid[0] = NaN.
 * TC_ERR_ARG for a NULL pointer, M < 2, D < 1 or max_sweeps outside 1 .. TC_SET_MAX_SWEEPS; TC_ERR_UNSUPPORTED for D > TC_SET_MAX_D.
 *
 * tcdiff_set_check copies status to the host, WAITS for the stream and returns TC_ERR_NOCONVERGE if failed is set. */
#define TC_SET_MAX_D 72
#define TC_SET_MAX_SWEEPS 30
#define TC_ERR_NOCONVERGE (-5)
int tcdiff_kinetic_features(const float* joints, const long* joint_strides, int b, int dn, int T, int up, int window, double fps,
                            double* feats, hipStream_t stream);
int tcdiff_set_stats(const double* feats, long N, int D, int fit, double* mean, double* std_, double* z, double* zc, double* mu,
                     double* cov, double* div_rows, hipStream_t stream);
int tcdiff_set_scores(const double* ref_mu, const double* ref_cov, const double* mu, const double* cov, const double* div_rows,
                      long M, int D, int max_sweeps, double* fid, double* div, int* status, hipStream_t stream);
int tcdiff_set_check(const int* status, hipStream_t stream);

/* ---- music features: the STFT path (csrc/music.hip) ---------------------------------------------------------------------------
 * From a waveform to 425 of the 438 columns of `cond`, as the reference computes them on the CPU with librosa 0.9
 * (data/data_preprocess/dataset_utils.py:45-86), restated here because librosa is not a dependency; parity with librosa's own
 * output is not pinned.  fp32 arithmetic, B clips per launch, no atomics, every sum in a fixed order: a second run, and a clip
 * computed alone, give the same bits.  Eleven launches for a whole feature matrix, whatever B.  Fixed: n_fft 2048, hop 512,
 * periodic Hann windows, 128 mel bands, 20 MFCC, tempogram window 384, HPSS kernel 31, mask power 2, margin 1.
 * A clip has n >= 2048 samples and T = 1 + n / 512 frames.  FLT_MIN below is the smallest normal float.
 *
 * Tables, all DEVICE, computed by the host in float64 and rounded once:
 *   twiddle   [1024][2] float   (cos, -sin)(2 pi k / 2048)
 *   window    [2048] float for the STFT launchers, [384] for tcdiff_music_onset:  0.5 - 0.5 cos(2 pi i / N)
 *   mel_w     [128][1025] float: Slaney mel scale (linear below 1 kHz at 200/3 Hz per mel, logarithmic above with step ln(6.4)/27),
 *             130 points equally spaced in mel over [0, sr/2], triangular filters between them over the bins k sr / 2048, each
 *             scaled by 2 / (f[i+2] - f[i]);  mel_range [128][2] int: filter i is zero outside bins [lo, hi)
 *   dct       [20][128] float: s_k cos(pi (2 m + 1) k / 256), s_0 = sqrt(1/128), s_k = sqrt(2/128)  (orthonormal DCT-II)
 *
 * tcdiff_music_stft, one launch.  y: clip b at y + b * y_stride, n floats.
 *   The clip is padded by 1024 on both sides by reflection (edge sample not repeated); frame t is padded samples
 *   [512 t, 512 t + 2048) times the window; D[b][t][k], k <= 1024, its DFT (interleaved re, im); S = |D|; M[b][t][i] =
 *   sum_k mel_w[i][k] S[b][t][k]^2 in ascending k;  frame_max[b][t] = max_i M[b][t][i].  D and S are both given or both NULL
 *   (the mel power alone).
 *
 * tcdiff_music_mfcc, two launches.  M [B][T][128], frame_max [B][T] -> mx [B] = the largest M of each clip (workspace);
 *   mel_db[b][t][i] = max(-80, 10 log10(max(1e-10, M)) - 10 log10(max(1e-10, mx[b])))  (the largest dB of a clip is 0);
 *   feats[b][t][k] = sum_i dct[k][i] mel_db[b][t][i], k < 20;  feats[b][t][20 + k] = (x[c + 1] - x[c - 1]) / 2 of column k with
 *   c = t clamped to [1, T - 2]  (scipy.signal.savgol_filter, window 3, order 1, mode 'interp').  feats rows have TC_MUSIC_COLS floats.
 *
 * tcdiff_music_hpss, three launches.  H / P [B][T][1025] = the 31-tap median of S along t / along k, the axis extended as
 *   scipy.ndimage's 'reflect' (edge sample repeated, period twice the length): an exact selection per element.
 *   mask(X, R) = 0.5 where Z = max(X, R) < FLT_MIN, else (X/Z)^2 / ((X/Z)^2 + (R/Z)^2).
 *   frames [B][W][T][2048] (workspace, W = 2, or 1 when harmonic is NULL): the inverse real DFT of D mask(P, H) (part 0) and of
 *   D mask(H, P) (part 1), divided by 2048, times the window.  percussive / harmonic [B][n]: sample i is padded sample
 *   p = i + 1024; the sum over the frames t with 512 t <= p < 512 t + 2048 in ascending t of frames[t][p - 512 t], divided by the
 *   sum of window[p - 512 t]^2 over the same frames where that exceeds FLT_MIN; 0 where there is no frame.
 *
 * tcdiff_music_onset, three launches.  M [B][T][128]: the mel power of the PERCUSSIVE signal (tcdiff_music_stft on the whole clip
 *   percussive[b]) and its frame_max; mx [B] workspace.  dB = max(10 log10(max(1e-10, M)), 10 log10(max(1e-10, mx[b])) - 80).
 *   onset_env[b][t] = 0 for t < 3, else the median over i of max(0, dB[t - 2][i] - dB[t - 3][i]) (the mean of the two middle
 *   values); also stored at feats[b][t][40].  Tempogram: onset_env padded by 192 on both sides as numpy.pad's 'linear_ramp' to 0;
 *   x = padded samples [t, t + 384) times the 384-window; a[l] = sum_i x[i] x[i + l] over i + l < 384 in ascending i;
 *   feats[b][t][41 + l] = a[l] / max_l |a[l]|, or a[l] where that maximum is below FLT_MIN.
 *
 * TC_ERR_ARG for a NULL pointer (those named optional excepted), B < 1, n < 2048 or T < 5; TC_ERR_UNSUPPORTED for B > 65535 or
 * n > 2^29. */
#define TC_MUSIC_N_FFT 2048
#define TC_MUSIC_HOP 512
#define TC_MUSIC_N_MELS 128
#define TC_MUSIC_N_MFCC 20
#define TC_MUSIC_TEMPO_WIN 384
#define TC_MUSIC_COLS 425            /* mfcc 0-19, delta 20-39, onset_env 40, tempogram 41-424 */
int tcdiff_music_stft(const float* y, long y_stride, int B, int n, const float* twiddle, const float* window, const float* mel_w,
                      const int* mel_range, float* D, float* S, float* M, float* frame_max, hipStream_t stream);
int tcdiff_music_mfcc(const float* M, const float* frame_max, int B, int T, const float* dct, float* mx, float* mel_db, float* feats,
                      hipStream_t stream);
int tcdiff_music_hpss(const float* D, const float* S, int B, int n, const float* twiddle, const float* window, float* H, float* P,
                      float* frames, float* percussive, float* harmonic, hipStream_t stream);
int tcdiff_music_onset(const float* M, const float* frame_max, int B, int T, const float* window, float* mx, float* onset_env,
                       float* feats, hipStream_t stream);

/* ---- music features: the beat track (csrc/beat.hip) --------------------------------------------------------------------------
 * Column 53 of `cond`, onset_beat: the one-hot output of librosa's beat tracker run on the onset envelope
 * (data/data_preprocess/_preprocess_wav.py:70-83; dataset_utils.py:72 keeps element [0] of the pair, so peak_pick is not built).
 * librosa 0.9.2's beat.beat_track, beat.tempo and beat.__beat_tracker restated for one float envelope o[0 .. T) per clip, T >= 5,
 * at 60 frames / s (the only rate supported); parity with librosa's own output is not pinned.  Precondition: every envelope
 * value is finite and >= 0, as music_features' onset_env is (a negative or NaN value gives NaN scores, which the kernel's
 * maxima skip where numpy's argmax would return the first NaN: the result is then unspecified).  Two launches for any number of
 * clips (tcdiff_beat_tempo, tcdiff_beat_track), one when the period is given; no float atomics, every sum in a fixed order: a
 * second run, and a clip computed alone, give the same bits.  Three quirks of 0.9.2 are kept on purpose: (1) np.round rounds
 * half to even (period = round(3600 / bpm) on the host, h below); (2) the end of the trim slice is exclusive; (3) the trim's
 * symmetric 5-point Hann window has zero end taps.
 *
 * Tables, DEVICE, computed by the host in float64 (nothing is computed in-kernel):
 *   window  [480] float   0.5 - 0.5 cos(2 pi i / 480)
 *   prior   [480] double  -0.5 ((log2(3600 / l) - log2(start_bpm)) / std_bpm)^2;  -inf for l = 0 and wherever 3600 / l >= max_tempo
 *   tables  [2][TC_BEAT_TABLE] double, one row per period p = 1 .. 479 in each half, row p at offset p^2 - 1:
 *           half 0  w[j + p]  = exp(-0.5 (32 j / p)^2), j = -p .. p                          (2 p + 1 values)
 *           half 1  txwt[k]   = -tightness ln(-d_k / p)^2, d_k = -2 p + k, k = 0 .. 2 p - h  (2 p - h + 1 values),
 *                   h = rint(p / 2), half to even
 *
 * tcdiff_beat_tempo, one launch.  onset_env: clip b at onset_env + b * o_stride, T floats.  The envelope is padded by 240 on
 *   both sides as numpy.pad's 'linear_ramp' to 0; for each frame t, x = padded samples [t, t + 480) times the window;
 *   a_t[l] = sum_i x[i] x[i + l] over i + l < 480 in ascending i, in fp32 (the tempogram's form and device code), divided by
 *   max_l |a_t[l]| unless that is below FLT_MIN.  partial[b][c][l], c < ceil(T / TC_BEAT_CHUNK) = the float64 sum of the
 *   normalised a_t[l] over the frames t of chunk c in ascending t.
 *
 * tcdiff_beat_track, one launch, one workgroup per clip.  Float64 from here on.
 *   Period.  partial given (period_host NULL): g[l] = (sum_c partial[b][c][l] in ascending c) / T;
 *     score[l] = log1p(1e6 g[l]) + prior[l];  lag = the first argmax;  period[b] = lag, tempo[b] = 3600 / lag.
 *     partial NULL: the caller has put the periods, ints in [1, 479], into period [B] (DEVICE) and the same values into
 *     period_host [B] (HOST, only read by the launcher's range check); tempo is the caller's (only a silent clip's is set).
 *   A clip whose envelope is all zero gets tempo 0 and no beats; one whose samples are all equal (zero variance) no beats: their
 *     local_score and cum_score rows are 0, their backlink rows -1.
 *   Local score.  x = o / std(o, ddof = 1).  Both sums of the standard deviation (of o, then of (o - mean)^2 with mean = sum / T;
 *     var = sum / (T - 1)) run in this order: partial p < 512 adds its elements p, p + 512, p + 1024, ... in ascending order
 *     (fused multiply-adds allowed), then s[p] += s[p + k] for p < k, k = 256, 128, ... 1; s[0] is the sum.
 *     ls[i] = sum_j w[j] x[i - j], j = -p .. p ascending, x zero outside the clip; each term a rounded product, then a rounded add.
 *   Dynamic programme, i ascending: c[k] = txwt[k] + (cum[i + d_k] if i + d_k >= 0 else 0); k* = the first argmax;
 *     cum[i] = ls[i] + c[k*];  backlink[i] = -1 for i < f, else i + d_k*, f = the first i with ls[i] >= 0.01 max(ls).
 *     Frames i .. i + h - 1 never read one another's cum: the kernel runs blocks of h frames between barriers.
 *   Last beat.  m[i] = cum[i] > cum[i - 1] and cum[i] >= cum[i + 1], the ends repeating their edge value (m[0] is false);
 *     med = the exact median of cum[m] (the mean of the two middle values for an even count);
 *     last = the largest i with m[i] and 2 cum[i] > med.  No flagged frame, or none above the median: no beats.
 *   Backtrace and trim.  beats[0 .. n) = last, backlink[last], ... while >= 0, reversed (beats_ws: workspace, in backtrace order);
 *     s[q] = 0.5 ls[beats[q - 1]] + ls[beats[q]] + 0.5 ls[beats[q + 1]], terms outside the array dropped;
 *     thr = 0.5 sqrt(mean(s^2)) if trim else 0;  v0 / v1 = the first / last q with s[q] > thr;  kept: beats[v0 : v1].
 *     onset_beat[b][t] = 1.0f at the kept beats, 0 elsewhere;  n_beats[b] = their number.
 *
 * TC_ERR_ARG for a NULL pointer (those named optional excepted; exactly one of partial and period_host is given, prior with
 * partial), B < 1, T < 5 or a period outside [1, 479]; TC_ERR_UNSUPPORTED for B > 65535 or T > 2^20. */
#define TC_BEAT_WIN 480
#define TC_BEAT_CHUNK 8              /* frames per workgroup of tcdiff_beat_tempo */
#define TC_BEAT_TABLE (480 * 480 - 1)
int tcdiff_beat_tempo(const float* onset_env, long o_stride, int B, int T, const float* window, double* partial, hipStream_t stream);
int tcdiff_beat_track(const float* onset_env, long o_stride, int B, int T, const double* partial, const double* prior,
                      const double* tables, const int* period_host, int trim, double* local_score, double* cum_score, int* backlink,
                      int* beats_ws, float* onset_beat, int* period, int* n_beats, double* tempo, hipStream_t stream);

/* ---- music features: the chroma columns (csrc/chroma.hip) -----------------------------------------------------------------------
 * Columns 40-51 of `cond`: librosa.feature.chroma_cqt(y=audio_harmonic, sr=30720, n_octaves=7) of
 * data/data_preprocess/_preprocess_wav.py:45-47 and dataset_utils.py:69, that is librosa 0.9.2's estimate_tuning (piptrack +
 * pitch_tuning), its seven-octave constant-Q transform (36 bins per octave from C1, hop 512) with resampy's kaiser_fast decimation
 * by two between octaves, and the fold to 12 chroma.  Everything below restates librosa 0.9.2 and resampy at those arguments FROM
 * KNOWLEDGE OF THOSE VERSIONS, NOT FROM THEIR SOURCE, which is not available where this is built; like the rest of the music path,
 * parity with librosa's own output is not pinned.  The one default this restatement is least sure of is the constant-Q frames'
 * padding (zeros, librosa 0.9's pad_mode='constant' for cqt; see the response).  fp32 arithmetic unless said otherwise, B clips
 * per launch, no float atomics, every sum in a fixed order: a second run, and a clip computed alone, give the same bits.  Four
 * launches for any number of clips (one of them tcdiff_music_stft on the harmonic signal), two when the tuning is given.  A clip
 * has n >= 2048 samples and T = 1 + n / 512 frames.  FLT_MIN is the smallest normal float.
 *
 * Constants: bins_per_octave 36, n_octaves 7, n_bins 252, fmin0 = 32.70319566257483 Hz (C1), alpha = 2^(1/36) - 1, Q = 1 / alpha,
 * Hann window_bandwidth 1.50018310546875, BW_FASTEST 0.85.  A tuning is one of the 100 values
 * EDGES[k] = linspace(-0.5, 0.5, 101)[k], k = 0 .. 99, in fractions of a 1/36-octave bin.
 *
 * Tables, all DEVICE, computed by the host in float64 and rounded once:
 *   taps     [63] float: h[j + 31] = 0.5 win[256 |j|], j = -31 .. 31, of the kaiser_fast table
 *            win[m] = 0.85 sinc(0.85 m / 512) kaiser(2 * 8192 + 1, beta = 8.555504641634386)[8192 + m], m = 0 .. 8192 (sinc(x) =
 *            sin(pi x) / (pi x); m = 8192 is never reached): resampy's interpolating resampler at ratio 1/2 reads only these entries.
 *   twiddle  [512][2] float  (cos, -sin)(2 pi k / 1024)
 *   edges    [101] double    EDGES
 *   basis    [100][36][TC_CHROMA_BAND][2] float, band [100][36][2] int, per tuning k, for the top octave's frequencies
 *            f_r = fmin0 2^(EDGES[k] / 36) 2^(6 + r / 36), r < 36:  len = Q sr / f_r;  the time filter exp(2 pi i f_r a / sr)
 *            over a = arange(-len // 2, len // 2) (floats: floor(len) or ceil(len) points) times the periodic Hann window of
 *            floor(len) points, zero-extended where the filter is one point longer; divided by its L1 norm; centre-padded to
 *            1024 ((1024 - points) // 2 zeros in front); times len / 1024; its 1024-point DFT, bins 0 .. 512; per row, entries
 *            below the magnitude at the first index where the ascending cumulative magnitude reaches 1 % of the row's sum are
 *            set to zero; rounded to complex64.  Row r keeps bins [lo, hi) = band[k][r] (its first to last nonzero, zeros
 *            inside kept, hi - lo <= TC_CHROMA_BAND) at basis[k][r][0 .. hi - lo).  f / sr is the same in every octave up to
 *            exact powers of two, so octave i uses this basis times sqrt(2^i).
 *   scale    [100][252] float, lowest bin first: sqrt(2^i) / sqrt(Q sr / f_bin), i = 6 - bin / 36,
 *            f_bin = fmin0 2^(EDGES[k] / 36) 2^(bin / 36)
 *   At these settings librosa does no early downsampling and handles no top octave apart (the top filter's cutoff, about 4.17 kHz,
 *   is below 0.85 Nyquist, and the downsample count is 0 for every tuning in [-0.5, 0.5)); the host asserts both.
 *
 * tcdiff_chroma_pyramid, one launch.  y: clip b at y + b * y_stride, n floats.  pyramid [B][P], P = sum_{s = 1 .. 6} ceil(n / 2^s):
 *   signals 1 .. 6 one after another, signal s (ceil(n / 2^s) samples) = y_s[t] = sqrt(2) sum_j h[j] y_{s-1}[2 t + j], j = -31 .. 31
 *   ascending (fused multiply-adds), terms outside the signal dropped, t = 0 .. ceil(len / 2) - 1; y_0 = y.  (librosa zero-fills the
 *   last sample of an odd-length signal's half instead of computing it.)
 *
 * tcdiff_chroma_tuning, one launch, one workgroup per clip.  S [B][T][1025]: |STFT| of the clip, n_fft 2048, hop 512, periodic
 *   Hann, centred, reflect padding (S of tcdiff_music_stft).  For bins f_lo <= f <= f_hi (the host's: 150 <= f sr / 2048 < 4000;
 *   1 <= f_lo, f_hi <= 1023):  avg = 0.5 (S[f+1] - S[f-1]);  den = 2 S[f] - S[f+1] - S[f-1];  shift = avg / (den + (|den| < FLT_MIN));
 *   dskew = 0.5 avg shift;  with M = S where S > 0.1 max_f S[t][:] (all 1025 bins) else 0, bin f is a pitch when M[f] > M[f-1]
 *   and M[f] >= M[f+1];  pitch = (f + shift) bin_hz (bin_hz = sr / 2048; float32), mag = S[f] + dskew.  Per clip: thr = the
 *   exact median of mag over the pitches (the mean of the two middle values for an even count, in float32); for the pitches with
 *   mag >= thr, in float64 from the float32 pitch (librosa: float32), r = mod(36 log2(pitch / 27.5), 1), less 1 where r >= 0.5;
 *   counts[b][k] = the number of r in [edges[k], edges[k+1]) (numpy.histogram);  tuning_index[b] = the first argmax;
 *   n_pitches[b], threshold[b] as named.  A clip with no pitch: index 50 (tuning 0.0), threshold 0, counts 0.
 *   pitch_ws / mag_ws [B][T][f_hi - f_lo + 1] workspaces (the clip's pitches, packed in no particular order: every step after
 *   piptrack counts, so the result does not depend on it).
 *
 * tcdiff_chroma_response, one launch, one workgroup per (clip, frame).  Octave i = 0 (the top 36 bins) .. 6 (the bottom 36) reads
 *   y_i at hop 512 / 2^i: frame t holds the 1024 samples centred on t 512 / 2^i, ZEROS outside the signal (see above), rectangular
 *   window; X = its 1024-point DFT;  C[r] = sum_f basis[k][r][f] X[f] over the row's band in ascending f, k = tuning_index[b]
 *   (DEVICE; clamped to 0 .. 99);  cqt_mag[b][t][36 (6 - i) + r] = |C[r]| scale[k][36 (6 - i) + r] (optional output);
 *   raw[c] = sum over the octaves, lowest first, of cqt_mag at bins 3 c - 1, 3 c, 3 c + 1 (mod 36) of the octave;
 *   chroma[b][t][c] = raw[c] / max_c raw, or raw[c] where that maximum is below FLT_MIN.  Every octave has at least T frames
 *   (they disagree when n = 512 k - 1): T is their minimum.
 *
 * TC_ERR_ARG for a NULL pointer (cqt_mag excepted), B < 1, n < 2048, T < 5 or bins outside [1, 1023]; TC_ERR_UNSUPPORTED for
 * B > 65535, n >= 2^29 or T > 2^20. */
#define TC_CHROMA_BPO 36
#define TC_CHROMA_OCTAVES 7
#define TC_CHROMA_BINS 252
#define TC_CHROMA_N 12
#define TC_CHROMA_N_FFT 1024
#define TC_CHROMA_BAND 24            /* the widest band of any row at sr 30720 is 20 bins */
#define TC_CHROMA_TUNINGS 100
#define TC_CHROMA_TAPS 63
int tcdiff_chroma_pyramid(const float* y, long y_stride, int B, int n, const float* taps, float* pyramid, hipStream_t stream);
int tcdiff_chroma_tuning(const float* S, int B, int T, int f_lo, int f_hi, float bin_hz, const double* edges, float* pitch_ws,
                         float* mag_ws, int* tuning_index, int* n_pitches, float* threshold, int* counts, hipStream_t stream);
int tcdiff_chroma_response(const float* y, long y_stride, const float* pyramid, int B, int n, const int* tuning_index,
                           const float* twiddle, const float* basis, const int* band, const float* scale, float* chroma, float* cqt_mag,
                           hipStream_t stream);

/* ---- audio files: decode, downmix, resample (csrc/audio.hip) ---------------------------------------------------------------------
 * What comes before the music features: librosa.load(wav_path, sr=30720) of dataset_utils.py:62, that is soundfile's decode to
 * float32, librosa.to_mono and librosa.resample(res_type="kaiser_best", fix=True, scale=False) over resampy.resample, after
 * data/slice.py:10-26 has cut the song into overlapping windows at the file's own rate (tcdiff_amd.audio.slice_audio, a view).
 * Everything below restates soundfile / libsndfile, librosa 0.9.2 and resampy at those arguments FROM THEIR DEFINITIONS, not from
 * their source, which is not available where this is built; like the rest of the music path, parity with their own output is not
 * pinned.  The RIFF/WAVE container is parsed on the host (tcdiff_amd.audio.read_wav); only the data chunk's bytes reach the
 * device.  Two launches for any number of clips, no host synchronisation, no atomics, every sum in a fixed order: a second run,
 * and a clip computed alone, give the same bits.  Not built: containers other than little-endian RIFF/WAVE, writing the slices
 * back as files, mono=False.
 *
 * tcdiff_audio_decode, one launch, one thread per frame.  data: clip b's data-chunk bytes at data + b * row_stride (row_stride a
 * multiple of 4 and at least frames * channels * bytes rounded up to 4: samples are assembled from aligned dword loads, and the
 * dword that holds a clip's last byte is read whole), interleaved little-endian frames of `channels` samples.  Per sample:
 *   TC_AUDIO_U8   (b - 128) / 128          TC_AUDIO_S16  v / 2^15          TC_AUDIO_S24  v / 2^23        (two's complement v)
 *   TC_AUDIO_S32  float32(v), round to nearest even, times 2^-31
 *   TC_AUDIO_F32  as is                    TC_AUDIO_F64  rounded to float32, nearest even
 * (all but S32 and F64 exact).  The downmix is numpy's float32 mean over the channels: s = x_0, then s = fl32(s + x_c) in channel
 * order, then fl32(s / C), the division correctly rounded; with C = 1 the sample passes through unchanged.
 * out [B][frames] float.
 *
 * tcdiff_audio_resample, one launch, one workgroup of 256 per 256 consecutive outputs of a clip.  y: clip b at y + b * y_stride,
 * n floats (rows may overlap; positions outside a row are never read).  The HOST computes, in float64 with Python's expressions:
 *   ratio = float(sr_new) / sr_orig;  n_out = int(n ratio);  size = int(ceil(n ratio));  inc = 1 / ratio;  scale = min(1, ratio);
 *   step = int(scale 512)
 * (at n = 735, 44100 -> 30720, n_out = 511 and size = 512; step is truncated, which gives down-sampling a DC gain slightly above
 * 1: 1.0006 .. 1.0008 at 44100 -> 30720.  Both are the reference's and stay), and the table, N = 512 * 64, m = 0 .. N,
 *   win[m]   = r sinc(r m / 512) kaiser(2 N + 1, beta = 14.769656459379492)[N + m],  r = 0.9475937167399596 (kaiser_best),
 *              times ratio when ratio < 1;    delta[m] = win[m + 1] - win[m], delta[N] = 0
 * in float64, rounded once to float32: table [N + 1][2] float (win, delta), DEVICE, 8-byte aligned.  Per output t < n_out, with
 * nwin = N + 1:
 *   tr = t inc;  n = (int)tr;  frac = scale (tr - n);  f = 512 frac;  off = (int)f;  eta = f - off
 *   left :  i = 0 .. min(n + 1, (nwin - off) / step) - 1:      out[t] += (win[off + i step] + eta delta[off + i step]) y[n - i]
 *   frac' = scale - frac;  f, off, eta again from frac'
 *   right:  k = 0 .. min(n_orig - n - 1, (nwin - off) / step) - 1: out[t] += (win[off + k step] + eta delta[off + k step]) y[n + k + 1]
 * (n_orig the clip's n).  tr = t inc is the form of resampy >= 0.3 and does not depend on evaluation order; resampy 0.2.2
 * accumulates tr += inc instead.  The index arithmetic from tr to off and eta is float64 with one rounding per operation (no
 * contraction), so n, off and both loop counts are the restatement's by construction; eta is then rounded to float32, and the
 * weights, products and sums are float32 (fused multiply-adds, left wing then right wing, each in ascending i / k).
 * out [B][size] float; out[t] = 0 for n_out <= t < size (librosa's fix_length).  The workgroup stages its span of the input in LDS
 * ((int)(255 inc) + 3 + 2 ceil(nwin / step) floats, sized by the launcher: at most 3069 for sr_orig / sr_new <= 8) and deals its
 * outputs to its threads in the order of off, which narrows a wave's table gathers and changes no output's bits; the table stays
 * in global memory.
 *
 * TC_ERR_ARG for a NULL pointer, B < 1, frames / channels / n / n_out < 1, an unknown format, a row_stride too short, size < n_out,
 * scale outside (0, 1], step outside [1, 512] or (n_out - 1) inc >= n; TC_ERR_ALIGN for data or row_stride not a multiple of 4
 * or a table not 8-byte aligned; TC_ERR_UNSUPPORTED for B > 65535, channels > 65535, n or size >= 2^29, or step <
 * TC_AUDIO_MIN_STEP (sr_orig / sr_new > 8). */
#define TC_AUDIO_U8 0
#define TC_AUDIO_S16 1
#define TC_AUDIO_S24 2
#define TC_AUDIO_S32 3
#define TC_AUDIO_F32 4
#define TC_AUDIO_F64 5
#define TC_AUDIO_PRECISION 512       /* table entries per zero crossing */
#define TC_AUDIO_TABLE (512 * 64 + 1)
#define TC_AUDIO_MIN_STEP 64
int tcdiff_audio_decode(const void* data, long row_stride, int B, int frames, int channels, int fmt, float* out, hipStream_t stream);
int tcdiff_audio_resample(const float* y, long y_stride, int B, int n, const float* table, double inc, double scale, int step, int n_out,
                          int size, float* out, hipStream_t stream);

/* ---- stick-figure frames (csrc/draw.hip)-----------------------------------------------------------------------------------
 * What skeleton_render (vis.py:223-327) shows of a generated dance -- 23 bones per dancer, the root's trail on the floor and
 * four foot markers -- as RGB frames, in two launches for any number of clips: no host synchronisation, no atomics, a fixed
 * paint order, so the same input gives the same bits.
 *
 * tcdiff_draw_project, one workgroup per (clip, frame).  joints (b, dn, T, 24, 3) / contacts (optional, (b, dn, T, 4)) fp32
 * DEVICE, read in place through joint_strides / contact_strides (HOST long[3] element strides, the trailing 24 x 3 / 4
 * contiguous) exactly as tcdiff_motion_metrics reads them.  view (HOST float[12]): a row-major 3 x 4 matrix whose rows give
 * screen x (pixels), screen y (pixels, down) and depth (larger = farther) of (X, Y, Z, 1); every product row . (X, Y, Z, 1) is
 * the float32 chain fma(m2, Z, fma(m1, Y, fma(m0, X, m3))), within 3 * 2^-24 * (|m0 X| + |m1 Y| + |m2 Z| + |m3|) of its exact
 * value.  Outputs (DEVICE):
 *   pts [b][T][dn][24][3] fp32   screen x, screen y and depth of every joint
 *   trail [b][T][dn][2] fp32     screen x, y of the root with its `up` component (0, 1 or 2) replaced by `floor`
 *   order [b][T][dn] int32       painter's order of the frame's dancers: far to near by the root's depth, ties by dancer index;
 *                                dancer d stands at rank #{e : depth_e > depth_d or (depth_e == depth_d and e < d)}; a NaN depth
 *                                counts as +infinity
 *   planted [b][T][dn][4] uint8  feet 7, 8, 10, 11: with contacts, contacts[t][k] > contact_threshold; without,
 *                                |J[t+1][f] - J[t][f]| < still in float64 on the float32 joints and 1 on the last frame -- the rule
 *                                the dataset labels with (dataset/group_dataset.py:204-207) and skeleton_render intends (:272-278)
 * TC_ERR_ARG for a NULL pointer (contacts and contact_strides excepted; contacts without contact_strides is refused), b, dn or
 * T < 1, up outside 0..2; TC_ERR_UNSUPPORTED for b * T above 2^31 - 1.
 *
 * tcdiff_draw_raster, grid (tiles, T, clips), one workgroup per 32 x 32 tile of one frame, writes frames [b][T][H][W][3] uint8
 * RGB and nothing else.  THE PICTURE.  A pixel starts as style->background (c = the 0..255 value per channel) and the frame's
 * primitives are blended over it in this order:
 *   1. static_segs [n_static][4] (DEVICE fp32 ax, ay, bx, by in pixels; may be NULL when n_static == 0), the same in every
 *      frame, in index order, colour static_rgb, half-width static_hw, opacity static_alpha;
 *   2. per dancer d in index order, the trail segments trail[t'-1][d] -> trail[t'][d] for t' = max(1, t - trail_len + 1) .. t
 *      (trail_len <= 0: t' = 1 .. t, every frame so far, as the reference's line 0, vis.py:163-166), colour
 *      colors[d % n_colors], half-width trail_hw, opacity trail_alpha;
 *   3. per dancer d = order[t][0], order[t][1], ...: the 23 bones pts[i] -> pts[parents[i]], i = 1 .. 23 in index order, colour
 *      colors[d % n_colors], half-width line_hw, opacity 1; then, if style->markers, four discs of radius marker_radius at
 *      joints 7, 8, 10, 11, planted_rgb where planted and free_rgb otherwise, opacity 1.
 * A primitive is a segment (a, b) with half-width hw and opacity alpha; a disc is a segment with a == b.  Its coverage at the
 * pixel centre p = (x + 0.5, y + 0.5) is
 *     cov = clamp(hw + 0.5 - dist(p, segment), 0, 1) * alpha,    dist(p, segment) = |p - (a + u (b - a))|,
 *     u = clamp((p - a) . (b - a) / |b - a|^2, 0, 1), and u = 0 for a segment of zero length,
 * a layer blends as c += cov * (src - c) per channel, and the stored byte is (uint8)(c + 0.5).  Only screen x and y of pts are
 * read; depth acts through `order` alone.  A primitive with a non-finite coordinate, or of a dancer index in `order` outside
 * [0, dn), is not drawn.  The kernel evaluates all of this in float64 on the float32 inputs.
 * CULLING.  The workgroup enumerates the primitives 256 at a time, drops those whose bounding box grown by hw + 0.5 (+ 1 / 64
 * pixel) misses the tile's pixel centres -- their coverage is 0 on the whole tile -- and compacts the rest into LDS in paint
 * order; the picture is bit for bit the one without culling, for any number of primitives per frame.  W and H need not be
 * multiples of the tile; joints may lie anywhere off the image.
 * colors (DEVICE uint8 [n_colors][3]); parents (HOST int[24], parents[0] unused); style (HOST).
 * TC_ERR_ARG for a NULL required pointer, b, dn, T, W or H < 1, n_colors < 1, n_static < 0 (or > 0 with NULL static_segs), a
 * parents[i] (i >= 1) outside 0..23, a half-width / radius outside [0, 16384] or an opacity outside [0, 1];
 * TC_ERR_UNSUPPORTED for T or b above 65535 or more than 2^31 primitives in a frame. */
typedef struct {
    unsigned char background[3], static_rgb[3], planted_rgb[3], free_rgb[3];
    float static_hw, static_alpha;       /* the static segments (the floor grid) */
    float line_hw;                       /* bones */
    float trail_hw, trail_alpha;
    int trail_len;                       /* trail segments kept per dancer; <= 0: all */
    int markers;                         /* non-zero: draw the foot discs */
    float marker_radius;
} tcdiff_draw_style;
int tcdiff_draw_project(const float* joints, const long* joint_strides, const float* contacts, const long* contact_strides, int b,
                        int dn, int T, const float* view, float floor, int up, double contact_threshold, double still, float* pts,
                        float* trail, int* order, unsigned char* planted, hipStream_t stream);
int tcdiff_draw_raster(const float* pts, const float* trail, const int* order, const unsigned char* planted, int b, int dn, int T,
                       int W, int H, const int* parents, const float* static_segs, int n_static, const unsigned char* colors,
                       int n_colors, const tcdiff_draw_style* style, unsigned char* frames, hipStream_t stream);

/* ---- Dance-Beat Navigator (csrc/navigator.hip) -----------------------------------------------------------------------
 * TrajDecoder (TrajDecoder/model/traj_model.py:125-200: latent_dim 64, 4 heads, nfeats 2) and the sliding-window rollout of
 * TCDiff.test_loop (TCDiff.py:526-547), exact fp32 throughout (v_mfma_f32_16x16x4_f32 products).  All pointers DEVICE fp32.
 *
 * The music front: `music_projection` (traj_model.py:142-148,177-184: frames paired to 876 features, 876 -> 438 -> 438 -> 64
 * with LeakyReLU(0.01)) and `cond_emb` (:79,109) of EVERY frame pair of cond [b][n_frames][438] (an odd last frame is
 * dropped), once per rollout: mp [b][n_frames / 2][64] = music_projection, me [same] = cond_emb(mp).  A window that starts at
 * the even frame `start` reads rows start / 2 ... of both.  wm: the packed weights, zero-padded to K = 880 / N = 448:
 * W1 [448][880], b1 [448], W2 [448][448], b2 [448], W3 [64][448], b3 [64], Wc [64][64], bc [64] (628736 floats). */
int tcdiff_nav_music_front(const float* cond, int b, int n_frames, const float* wm, float* mp, float* me, hipStream_t stream);

typedef struct {
    int b, dn, seq;      /* clips, dancers, frames per window: T = dn * seq <= 500 token rows per clip */
    int n_layers;        /* transformer blocks */
    int pairs;           /* rows per clip of me / mp */
    int me_off, mp_off;  /* window 0: first row of the conditioning side (music_feat[:, :seq]) / of the prediction side
                            (music_feat[:, -seq:], traj_model.py:187,190) */
    int win_stride;      /* added to both per window (= step) */
    int step;            /* frames appended to `roll` per window */
    int roll_frames, roll_off; /* frames per (clip, dancer) of `roll`; window w's tail goes to frame roll_off + w * step */
    const float* lstm_w;   /* [3][128][256]: k < 64 weight_ih_l (zero beyond the layer's input width), k >= 64 weight_hh_l,
                              transposed; gate rows in PyTorch's order i, f, g, o */
    const float* lstm_bih; /* [3][256] */
    const float* lstm_bhh; /* [3][256] */
    const float* pe;       /* [500][64] PositionalEncoding rows (model/utils.py:18-25) */
    const float* blocks;   /* [n_layers][198272]: ln1 g, b; Wq, bq; Wk, bk; Wv, bv; Wproj, b; ln2 g, b; W1 [512][128], b1;
                              W2 [128][512], b2 -- every W as nn.Linear stores it, [out][in] */
    const float* dec;      /* Decoder (traj_model.py:159-167): W1 [128][192], b1, W2 [128][128], b2, W3 [64][128], b3,
                              W4 [16][64] (rows 2.. zero), b4 [16]: 50512 floats */
    const float* me;       /* tcdiff_nav_music_front's tables */
    const float* mp;
    float* traj;           /* [b][T][2]: in = the conditioning window, out = the prediction (the next window's input) */
    float* lstm_out;       /* [b][T][64] workspace */
    float* x;              /* [b][T][128] workspace (residual stream) */
    float* q;              /* [2][b][Tp][128] workspaces, Tp = T rounded up to 16; ZERO before the first call (the pad rows */
    float* k;              /* [2][b][4][Tp][32]   / columns are read and never written)                                  */
    float* vt;             /* [2][b][4][32][Tp] */
    float* roll;           /* [b][dn][roll_frames][2] or NULL */
    float* tap_lstm;       /* NULL, or [b][T][64]: window 0's LSTM output before the positional encoding */
    float* tap_blocks;     /* NULL, or [n_layers][b][T][128]: window 0's residual stream after every block */
} tcdiff_nav_args;

/* n_windows forwards of TrajDecoder chained as TCDiff.py:540-544 chains them: per window one LSTM launch (traj_model.py:139,174
 * -- built without batch_first, so the recurrence runs over the CLIP index b and the T positions are its batch; the epilogue
 * adds the PositionalEncoding row, :106), one front launch ([cond_emb rows repeated dn times | LSTM rows], :109-118, block 0's
 * LN1 + Q / K / V) and one launch per block (:29-46,62-65: attention WITHOUT mask, heads of 32, proj + residual, LN2, MLP with
 * erf-GELU, residual, the next block's LN1 + Q / K / V; the last one runs the Decoder on [x | prediction-side music rows],
 * :190-200, writes `traj` and the last `step` frames of every dancer to `roll`): n_layers + 2 launches per window, one stream.
 * n_windows = 1 with me_off = 0, mp_off = pairs - seq and roll = NULL is TrajDecoder.forward.
 * TC_ERR_UNSUPPORTED for T > 500 (PositionalEncoding's max_len: the reference raises there too). */
int tcdiff_nav_rollout(const tcdiff_nav_args* a, int n_windows, hipStream_t stream);

/* The hand-off to the sampler (csrc/handoff.hip; TCDiff.py:543-556, TrajDecoder/train_traj.py:245-259): the forward Kalman
 * filter of TrajDecoder/utils/utils_model.py:10-74 over every (clip, dancer) trajectory, the zero z channel and the frame-major
 * token order, one launch, one thread per trajectory.
 * traj: DEVICE fp32, element (clip, dancer, frame, channel) at traj[clip * s_b + dancer * s_dn + frame * s_f + channel * s_c]
 *   (element strides: any view -- the rollout's buffer, x[:, :, :, [4, 5]] -- is read in place); b x dn x frames x 2.
 * State (x, y, vx, vy) in float64, started at the first sample with zero velocity; per frame x = F x (constant velocity over
 * dt), then residual = z - H x, x += K_t residual, every product and sum rounded on its own; the filtered position is rounded
 * once to fp32.
 * gains: DEVICE float64 [frames][4][2], K_t of P = F P F^T + Q, S = H P H^T + R, K = P H^T S^-1 and the Joseph-form update from
 *   P0 = 10 I (data-independent: computed on the host once per (frames, dt, Q, R), tcdiff_amd/io.py kalman_gains).
 * scale / min_: both NULL, or HOST float [3]: the outputs become (clamp(v, -1, 1) - min_[ch]) / scale_[ch] (Normalizer.unnormalize
 *   of the zero-padded triple, dataset/preprocess.py:39-43; clamp keeps NaN), two rounded fp32 operations, z channel included.
 * smoothed (optional): [b][dn][frames][2].  x0 (optional): [b][frames * dn][3], token frame * dn + dancer, channels (x, y, z) with
 *   z = 0 or its un-normalised value, written by the kernel (the buffer need not be zeroed).  At least one of the two.
 * TC_ERR_ARG for a NULL traj / gains, no output, b, dn or frames < 1, or only one of scale / min_; TC_ERR_UNSUPPORTED for more
 * than 2^31 - 1 workgroups of 64 trajectories. */
int tcdiff_nav_handoff(const float* traj, long s_b, long s_dn, long s_f, long s_c, int b, int dn, int frames, double dt,
                       const double* gains, const float* scale, const float* min_, float* smoothed, float* x0, hipStream_t stream);

/* ---- training the Navigator (csrc/navigator.hip train-mode forward, csrc/navigator_train.hip backward) ----------------------
 * TrajDecoder/train_traj.py:179 (`net(x_cond, cond[...])` with net.train()) and :200 (`loss.backward()`: torch autograd over
 * traj_model.py:170-200), fp32 throughout.  Rows are [clip][pos = dancer * seq + frame]; R = b * T token rows, Tp = T rounded up
 * to 16, P = b * pairs music rows, L = n_layers.
 *
 * Dropout (traj_model.py:40 attn_drop, :45 resid_drop, :59 mlp[3]; model/utils.py PositionalEncoding.dropout at :106) uses the
 * counter hash of csrc/train_common.h keyed by (seed, site, flat index in the reference's tensor):
 *   TC_SITE_NAV_POS                      pos_embed.dropout on (b, T, 64)
 *   TC_SITE_NAV_BLOCK(i, 0)              block i attn_drop on the probabilities (b, 4, T, T)
 *   TC_SITE_NAV_BLOCK(i, 1)              block i resid_drop on (b, T, 128)
 *   TC_SITE_NAV_BLOCK(i, 2)              block i mlp[3] on (b, T, 128)
 * The backward regenerates every mask; no mask and no probability is stored.
 * Limits: fp32; T <= 500; the element index is a 32-bit word that wraps, as csrc/train_common.h defines (the oracle wraps alike):
 * attn_drop's b * 4 * T * T stays below 2^32 up to b = 4294 clips at T = 500, beyond which distinct elements share mask bits. */
#define TC_SITE_NAV_POS 256
#define TC_SITE_NAV_BLOCK(i, k) (260 + 4 * (i) + (k))

/* float offsets of the gradients inside `grads`: the transformer blocks and the Decoder as tcdiff_nav_args packs them (the
 * Decoder's last linear in the first 2 of 16 rows), then music_projection + cond_emb UNPADDED (W1 [438][876], b1, W2 [438][438],
 * b2, W3 [64][438], b3, Wc [64][64], bc), then per LSTM layer W_ih [256][in], W_hh [256][64], b_ih, b_hh (in = 2, 64, 64). */
#define TC_NAV_G_DEC(L) ((long)(L) * 198272)
#define TC_NAV_G_MUSIC(L) (TC_NAV_G_DEC(L) + 50512)
#define TC_NAV_G_MUSIC_SIZE (438 * 876 + 438 + 438 * 438 + 438 + 64 * 438 + 64 + 64 * 64 + 64)
#define TC_NAV_G_LSTM(L) (TC_NAV_G_MUSIC(L) + TC_NAV_G_MUSIC_SIZE)
#define TC_NAV_G_LSTM_SIZE (256 * (2 + 64 + 2) + 2 * 256 * (64 + 64 + 2))
#define TC_NAV_G_SIZE(L) (TC_NAV_G_LSTM(L) + TC_NAV_G_LSTM_SIZE)
#define TC_NAV_WG_CHUNKS 32 /* most row chunks of a weight gradient's first stage */
#define TC_NAV_WG_PARTIAL (448 * 896 + 448) /* floats per chunk: the largest [N to 16][K to 64] weight tile plus its bias */

typedef struct {
    unsigned seed0, seed1;  /* the two seed words of this step's masks */
    unsigned drop_thr;      /* floor(p * 2^32); 0 = every site an identity */
    float drop_scale;       /* 1 / (1 - p) */
    const float* cond;      /* [b][2 pairs][438]: the music frames the forward read (an odd last frame already dropped) */
    const float* x_in;      /* [R][2]: the conditioning window (tcdiff_nav_args.traj is overwritten by the prediction) */
    /* written by the forward, read by the backward */
    float* lstm_gates;      /* [3][R][256] the activated gates i, f, g, o */
    float* lstm_c;          /* [3][R][64] cell states */
    float* lstm_h;          /* [3][R][64] hidden states */
    float* xs;              /* [L + 1][R][128] every block's input rows and the last block's output */
    float* xmid;            /* [L][R][128] the rows after the attention residual */
    float* att_o;           /* [L][R][128] the attention's output before proj */
    float* lse;             /* [L][b][4][Tp] log-sum-exp of every score row */
    float* hid;             /* [L][R][512] the MLP's hidden rows before the GELU */
    float* dec_z;           /* [R][320] the Decoder's pre-activations: 128 | 128 | 64 */
    float* mus_z;           /* [P][896] music_projection's pre-activations: 448 | 448 */
    /* tcdiff_nav_args.q / k / vt hold L images instead of 2 */
    /* backward workspaces */
    const float* d_out;     /* [R][2] the loss gradient of the prediction */
    float* gx;              /* [R][128] gradient of the residual stream */
    float* g_dec;           /* [R][336]: d z1 128 | d z2 128 | d z3 64 | d out 16 */
    float* g_mpb;           /* [R][64] gradient of the Decoder's music columns, per token row */
    float* g_m;             /* [R][128] gradient of mlp[2]'s output */
    float* g_hid;           /* [R][512] gradient of mlp[0]'s output */
    float* g_a;             /* [R][128] gradient of proj's output */
    float* g_o;             /* [b][Tp][128] gradient of the attention's output (pad rows stay zero) */
    float* delta;           /* [b][4][Tp] dO . O per row and head */
    float* g_qkv;           /* [R][384] gradients of Q | K | V */
    float* n1;              /* [R][128] LN1's output and */
    float* n2;              /* [R][128] LN2's output of the block in hand: the LayerNorm statistics are deliberately NOT saved by
                               the forward; the backward has the input rows in LDS, recomputes mean / rstd with the forward's
                               expression and writes the normalised rows here for the weight-gradient products */
    float* ln_part;         /* [b * ceil(T / 16)][4][128] per-workgroup sums for the LayerNorm weights */
    float* g_me;            /* [P][64] gradient of cond_emb's output (rows past seq zero) */
    float* g_mp;            /* [P][64] gradient of music_projection's output */
    float* g_mz;            /* [P][896] gradients of music_projection's pre-activations */
    float* g_gates;         /* [3][R][256] gradients of the LSTM's gate pre-activations */
    float* partial;         /* [TC_NAV_WG_CHUNKS][TC_NAV_WG_PARTIAL] first stage of the weight-gradient reductions */
    float* grads;           /* [TC_NAV_G_SIZE(L)] out: every parameter's gradient, assigned */
} tcdiff_nav_train_args;

/* The train-mode forward: tcdiff_nav_music_front + one window of tcdiff_nav_rollout (me_off = 0, mp_off = pairs - seq, no roll,
 * no taps) with the four dropout sites live and the tensors above written out.  With drop_thr = 0 the prediction equals the
 * inference path's bit for bit.  Replaces train_traj.py:179. */
int tcdiff_nav_train_fwd(const tcdiff_nav_args* a, const tcdiff_nav_train_args* t, const float* wm, hipStream_t stream);

/* The reverse pass of that forward, replacing train_traj.py:200 below `pre_traj`: Decoder, the blocks last to first (MLP and proj
 * adjoints with LayerNorm / GELU / residual / dropout fused around the input-gradient products; attention backward flash-style
 * from Q, K, V and the saved log-sum-exp with the mask regenerated; Q / K / V adjoint through LN1), the front (cond_emb half
 * summed over dancers, both music row ranges added where they overlap, music_projection), the LSTM backward through time over
 * the clip axis (the forward's wavefront reversed), and every weight / bias gradient as a fixed-order two-stage reduction: no
 * floating-point atomics, the same bits from the same seed.  Inputs get no gradient. */
int tcdiff_nav_train_bwd(const tcdiff_nav_args* a, const tcdiff_nav_train_args* t, const float* wm, hipStream_t stream);

/* ---- the rest of the Navigator's training step (csrc/navigator_step.hip): loss head and optimizer ----------------------------
 * The loss of TrajDecoder/train_traj.py:183-196 on pre, tgt = (b, dn, seq, 2) fp32 DEVICE views, element (clip, dancer, frame,
 * channel) at p[clip * strides[0] + dancer * strides[1] + frame * strides[2] + channel * strides[3]] (HOST long[4] element
 * strides: `x[:, :, recon_start:recon_end]` is read in place, nothing is copied):
 *   recon = mean((pre - tgt)^2)                                                      train_traj.py:183  over b dn seq 2 elements
 *   dis   = mean(((tgt[:, 1:] - tgt[:, :-1]) - (pre[:, 1:] - pre[:, :-1]))^2)        :186-188           over b (dn - 1) seq 2
 *   v     = mean(((tgt[:, :, 1:] - tgt[:, :, :-1]) - (pre[:, :, 1:] - ...))^2)       :191-193           over b dn (seq - 1) 2
 *   out   = {recon + 2 dis + 2 v, recon, dis, v}                                     :196
 * Rounding points: every difference, the difference of differences, the square and every addition round on their own (no
 * contraction), as the reference's tensor expression; each mean is sum / count (one division); total = (recon + 2 dis) + 2 v.
 * The sums are fixed-order and two-stage, without floating-point atomics: workgroup k sums elements [k, k + 1) *
 * TC_NAV_LOSS_BLOCK (8 per thread in index order, then a fixed tree over the 256 threads) into partial[k][3]; a second launch of
 * one workgroup adds the partials the same way.  Same input, same bits.
 * partial: DEVICE workspace, 3 * ceil(b dn seq 2 / TC_NAV_LOSS_BLOCK) floats.  out: DEVICE float[4].
 * TC_ERR_ARG for a NULL pointer, b < 1, or dn < 2 / seq < 2 (a mean over zero elements: the reference's loss is NaN there). */
#define TC_NAV_LOSS_BLOCK 2048
int tcdiff_nav_loss(const float* pre, const long* pre_strides, const float* tgt, const long* tgt_strides, int b, int dn, int seq,
                    float* partial, float* out, hipStream_t stream);

/* d_pre [b][dn][seq][2] (contiguous) = grad_out[0] * d total / d pre, replacing autograd through train_traj.py:183-196 below
 * `loss.backward()` (:200), one launch, one thread per element:
 *   d_pre = grad_out * ((c_r e + c_d (ed[d - 1] - ed[d])) + c_v (ev[s - 1] - ev[s]))
 * with e, ed, ev the forward's three difference fields (recomputed with the forward's rounding points), the terms past either
 * end absent, and c_r = 2 / (b dn seq 2), c_d = 4 / (b (dn - 1) seq 2), c_v = 4 / (b dn (seq - 1) 2) computed in double and
 * rounded once.  grad_out: DEVICE float, read by the kernel (no host copy).  tgt gets no gradient.  Errors as tcdiff_nav_loss. */
int tcdiff_nav_loss_bwd(const float* pre, const long* pre_strides, const float* tgt, const long* tgt_strides, int b, int dn,
                        int seq, const float* grad_out, float* d_pre, hipStream_t stream);

/* torch.optim.AdamW / Adam (`optimizer.step()`, train_traj.py:201; utils_model.initial_optim) over every parameter in ONE launch:
 * a DEVICE table of chunks of <= 65536 elements, one workgroup each.  A chunk with `dst` also writes each new parameter value to
 * its place in one of TrajDecoder's packed weight images (tcdiff_nav_args.lstm_w / lstm_bih / lstm_bhh / blocks / dec,
 * tcdiff_nav_music_front's wm): element e = e0 + i of the parameter goes to dst[(e / row) * sr + (e % row) * sc] -- row = numel,
 * sc = 1 for a flat copy; row = 876, sr = 880 for a zero-padded matrix; row = in, sr = 1, sc = 256 for the transposed LSTM
 * weights.  The pad elements of an image are never written and stay zero. */
typedef struct {
    float* p;          /* parameter */
    const float* g;    /* gradient */
    float* m;          /* exp_avg */
    float* v;          /* exp_avg_sq */
    float* dst;        /* the parameter's image, or NULL */
    long n;            /* elements of this chunk */
    long e0;           /* index of the chunk's first element inside its parameter */
    long row, sr, sc;  /* the scatter above */
} tcdiff_nav_adamw_chunk;

/* torch/optim/adam.py _single_tensor_adam's Python doubles, rounded to fp32 where they meet a tensor.  Per element:
 *   decoupled: p = p * decay                     else: g = fma(p, wd, g)            [add(alpha=) is one fused multiply-add]
 *   m = fma(w - 1, g - m, g) for w = omb1 >= 0.5, else fma(w, g - m, m)             [at::native::lerp]
 *   v = v * beta2;  v = v + (omb2 * g) * g                                          [mul_, addcmul_: four roundings]
 *   denom = sqrt(v) / bc2_sqrt + eps;  p = p + (neg_step * m) / denom               [IEEE sqrt and divisions, no contraction] */
typedef struct {
    float decay;       /* 1 - lr * weight_decay */
    float wd;          /* weight_decay (the coupled form adds wd * p to the gradient) */
    float omb1;        /* 1 - beta1 */
    float beta2, omb2; /* beta2, 1 - beta2 */
    float neg_step;    /* -(lr / (1 - beta1^step)) */
    float bc2_sqrt;    /* sqrt(1 - beta2^step) */
    float eps;
    int decoupled;     /* 1: AdamW, 0: Adam with L2 weight decay */
} tcdiff_nav_adamw_scalars;

int tcdiff_nav_adamw(const tcdiff_nav_adamw_chunk* chunks, int n_chunks, const tcdiff_nav_adamw_scalars* scalars,
                     hipStream_t stream);

/* library identification */
const char* tcdiff_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TCDIFF_HIP_H */
