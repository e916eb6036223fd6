// What is left of the Dance-Beat Navigator's training step around its forward and backward (TrajDecoder/train_traj.py:183-201),
// gfx950, fp32: the loss head with its gradient, and the Adam / AdamW update that also keeps TrajDecoder's packed weight images
// in step.  All of it is a few hundred thousand to two million elements per call, bandwidth- and latency-bound: one thread per
// element, coalesced 4-byte accesses, no LDS tiling and no MFMA.
//
//   loss (train_traj.py:183-196)           tcdiff_nav_loss       two launches: fixed-order partial sums, then their sum
//   its gradient (autograd of the above)   tcdiff_nav_loss_bwd   one launch, the analytic expression
//   optimizer.step() (train_traj.py:201)   tcdiff_nav_adamw      one launch over a chunk table; scatters into the images
#include "common.h"
#include "tcdiff_hip.h"

struct NavLossView {            // element strides of a (b, dn, seq, 2) view
    const float* p;
    long s_b, s_d, s_s, s_c;
};

// The three difference fields at element (bi, d, s, c), each with the reference's rounding points: e = pre - tgt;
// ed = (pre[d + 1] - pre[d]) - (tgt[d + 1] - tgt[d]) for d < dn - 1; ev alike along the frames for s < seq - 1.  (The reference
// forms target - prediction for the last two; the sign is dropped by the square and fl(a - b) = -fl(b - a).)
struct NavLossTerms {
    float e, ed, ev;
};

DEVINL NavLossTerms nav_loss_terms(const NavLossView& pre, const NavLossView& tgt, long bi, int d, int s, int c, int dn, int seq) {
#pragma clang fp contract(off)
    const float* pp = pre.p + bi * pre.s_b + d * pre.s_d + s * pre.s_s + c * pre.s_c;
    const float* tp = tgt.p + bi * tgt.s_b + d * tgt.s_d + s * tgt.s_s + c * tgt.s_c;
    const float p0 = pp[0], t0 = tp[0];
    NavLossTerms r;
    r.e = p0 - t0;
    r.ed = 0.0f;
    r.ev = 0.0f;
    if (d < dn - 1) {
        const float rd = pp[pre.s_d] - p0, td = tp[tgt.s_d] - t0;
        r.ed = rd - td;
    }
    if (s < seq - 1) {
        const float rv = pp[pre.s_s] - p0, tv = tp[tgt.s_s] - t0;
        r.ev = rv - tv;
    }
    return r;
}

// sum of one value per thread over the 256 threads of a workgroup, always the same tree: same input, same bits
DEVINL float nav_block_sum(float v, float* lds) {
#pragma clang fp contract(off)
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) lds[threadIdx.x] += lds[threadIdx.x + h];
        __syncthreads();
    }
    const float r = lds[0];
    __syncthreads();
    return r;
}

// stage 1: workgroup k sums the squares of elements [k * TC_NAV_LOSS_BLOCK, (k + 1) * TC_NAV_LOSS_BLOCK) into partial[k][3]
__global__ __launch_bounds__(256) void nav_loss_partial_kernel(NavLossView pre, NavLossView tgt, int dn, int seq, long n,
                                                              float* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ float lds[256];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    const long base = (long)blockIdx.x * TC_NAV_LOSS_BLOCK;
    for (int k = 0; k < TC_NAV_LOSS_BLOCK / 256; ++k) {
        const long i = base + k * 256 + threadIdx.x;
        if (i >= n) break;
        const int c = (int)(i & 1);
        long r = i >> 1;
        const int s = (int)(r % seq);
        r /= seq;
        const int d = (int)(r % dn);
        const NavLossTerms t = nav_loss_terms(pre, tgt, r / dn, d, s, c, dn, seq);
        a0 += t.e * t.e;
        a1 += t.ed * t.ed;
        a2 += t.ev * t.ev;
    }
    a0 = nav_block_sum(a0, lds);
    a1 = nav_block_sum(a1, lds);
    a2 = nav_block_sum(a2, lds);
    if (threadIdx.x == 0) {
        partial[blockIdx.x * 3 + 0] = a0;
        partial[blockIdx.x * 3 + 1] = a1;
        partial[blockIdx.x * 3 + 2] = a2;
    }
}

// stage 2, one workgroup: out = {total, recon, dis, v}; the means divide like torch's mean, total = (recon + 2 dis) + 2 v
__global__ __launch_bounds__(256) void nav_loss_final_kernel(const float* __restrict__ partial, int n_blocks, float n_recon,
                                                            float n_dis, float n_v, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float lds[256];
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (int k = threadIdx.x; k < n_blocks; k += 256) {
        a0 += partial[k * 3 + 0];
        a1 += partial[k * 3 + 1];
        a2 += partial[k * 3 + 2];
    }
    a0 = nav_block_sum(a0, lds);
    a1 = nav_block_sum(a1, lds);
    a2 = nav_block_sum(a2, lds);
    if (threadIdx.x == 0) {
        const float recon = a0 / n_recon, dis = a1 / n_dis, v = a2 / n_v;
        out[0] = (recon + 2.0f * dis) + 2.0f * v;
        out[1] = recon;
        out[2] = dis;
        out[3] = v;
    }
}

// d total / d pre, times the incoming gradient: c_r e + c_d (ed[d - 1] - ed[d]) + c_v (ev[s - 1] - ev[s]) with the terms past
// either end absent (the one-sided ends), c_r = 2 / n_recon, c_d = 4 / n_dis, c_v = 4 / n_v
__global__ __launch_bounds__(256) void nav_loss_bwd_kernel(NavLossView pre, NavLossView tgt, int dn, int seq, long n, float c_r,
                                                          float c_d, float c_v, const float* __restrict__ grad_out,
                                                          float* __restrict__ d_pre) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i & 1);
    long r = i >> 1;
    const int s = (int)(r % seq);
    r /= seq;
    const int d = (int)(r % dn);
    const long bi = r / dn;
    const NavLossTerms t = nav_loss_terms(pre, tgt, bi, d, s, c, dn, seq);
    float gd = -t.ed, gv = -t.ev;                     // zero where the element has no neighbour after it
    if (d > 0) gd = nav_loss_terms(pre, tgt, bi, d - 1, s, c, dn, seq).ed + gd;
    if (s > 0) gv = nav_loss_terms(pre, tgt, bi, d, s - 1, c, dn, seq).ev + gv;
    d_pre[i] = grad_out[0] * ((c_r * t.e + c_d * gd) + c_v * gv);
}

static int nav_loss_check(const float* pre, const float* tgt, int b, int dn, int seq, long* n) {
    if (!pre || !tgt || b < 1 || dn < 2 || seq < 2) return TC_ERR_ARG;
    *n = (long)b * dn * seq * 2;
    if ((*n + 255) / 256 > 0x7fffffffL) return TC_ERR_UNSUPPORTED;
    return TC_OK;
}

extern "C" int tcdiff_nav_loss(const float* pre, const long* pre_strides, const float* tgt, const long* tgt_strides, int b, int dn,
                               int seq, float* partial, float* out, hipStream_t stream) {
    long n = 0;
    if (!pre_strides || !tgt_strides || !partial || !out) return TC_ERR_ARG;
    const int rc = nav_loss_check(pre, tgt, b, dn, seq, &n);
    if (rc != TC_OK) return rc;
    const NavLossView pv = {pre, pre_strides[0], pre_strides[1], pre_strides[2], pre_strides[3]};
    const NavLossView tv = {tgt, tgt_strides[0], tgt_strides[1], tgt_strides[2], tgt_strides[3]};
    const int n_blocks = (int)((n + TC_NAV_LOSS_BLOCK - 1) / TC_NAV_LOSS_BLOCK);
    hipLaunchKernelGGL(nav_loss_partial_kernel, dim3(n_blocks), dim3(256), 0, stream, pv, tv, dn, seq, n, partial);
    TC_CHECK_LAUNCH();
    hipLaunchKernelGGL(nav_loss_final_kernel, dim3(1), dim3(256), 0, stream, partial, n_blocks, (float)n,
                       (float)((long)b * (dn - 1) * seq * 2), (float)((long)b * dn * (seq - 1) * 2), out);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

extern "C" int tcdiff_nav_loss_bwd(const float* pre, const long* pre_strides, const float* tgt, const long* tgt_strides, int b,
                                   int dn, int seq, const float* grad_out, float* d_pre, hipStream_t stream) {
    long n = 0;
    if (!pre_strides || !tgt_strides || !grad_out || !d_pre) return TC_ERR_ARG;
    const int rc = nav_loss_check(pre, tgt, b, dn, seq, &n);
    if (rc != TC_OK) return rc;
    const NavLossView pv = {pre, pre_strides[0], pre_strides[1], pre_strides[2], pre_strides[3]};
    const NavLossView tv = {tgt, tgt_strides[0], tgt_strides[1], tgt_strides[2], tgt_strides[3]};
    const float c_r = (float)(2.0 / (double)n), c_d = (float)(4.0 / (double)((long)b * (dn - 1) * seq * 2)),
                c_v = (float)(4.0 / (double)((long)b * dn * (seq - 1) * 2));
    hipLaunchKernelGGL(nav_loss_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, pv, tv, dn, seq, n, c_r, c_d,
                       c_v, grad_out, d_pre);
    TC_CHECK_LAUNCH();
    return TC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// torch.optim.AdamW / Adam, the single-tensor form (torch/optim/adam.py _single_tensor_adam), every parameter in one launch.  One
// workgroup per chunk.  Rounding points per element (tcdiff_hip.h): fused where torch's kernel is one fused multiply-add (add with
// alpha, lerp), two roundings where torch's expression rounds twice (mul_ then addcmul_, addcdiv_'s product, quotient and sum).
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nav_adamw_kernel(const tcdiff_nav_adamw_chunk* __restrict__ chunks,
                                                       tcdiff_nav_adamw_scalars k) {
#pragma clang fp contract(off)
    const tcdiff_nav_adamw_chunk c = chunks[blockIdx.x];
    const bool small_w = fabsf(k.omb1) < 0.5f;                    // at::native::lerp's two branches
    const float coef = small_w ? k.omb1 : k.omb1 - 1.0f;
    for (long i = threadIdx.x; i < c.n; i += 256) {
        float g = c.g[i], p = c.p[i], m = c.m[i], v = c.v[i];
        if (k.decoupled)
            p = p * k.decay;                                      // param.mul_(1 - lr * weight_decay)
        else
            g = __builtin_fmaf(p, k.wd, g);                       // grad.add(param, alpha=weight_decay)
        m = __builtin_fmaf(coef, g - m, small_w ? m : g);         // exp_avg.lerp_(grad, 1 - beta1)
        v = v * k.beta2;                                          // exp_avg_sq.mul_(beta2)
        v = v + (k.omb2 * g) * g;                                 //           .addcmul_(grad, grad, value=1 - beta2)
        const float denom = __fdiv_rn(__fsqrt_rn(v), k.bc2_sqrt) + k.eps;
        p = p + __fdiv_rn(k.neg_step * m, denom);                 // param.addcdiv_(exp_avg, denom, value=-step_size)
        c.p[i] = p;
        c.m[i] = m;
        c.v[i] = v;
        if (c.dst) {
            const long e = c.e0 + i;
            c.dst[(e / c.row) * c.sr + (e % c.row) * c.sc] = p;
        }
    }
}

extern "C" int tcdiff_nav_adamw(const tcdiff_nav_adamw_chunk* chunks, int n_chunks, const tcdiff_nav_adamw_scalars* scalars,
                                hipStream_t stream) {
    if (!chunks || !scalars || n_chunks <= 0) return TC_ERR_ARG;
    hipLaunchKernelGGL(nav_adamw_kernel, dim3(n_chunks), dim3(256), 0, stream, chunks, *scalars);
    TC_CHECK_LAUNCH();
    return TC_OK;
}
