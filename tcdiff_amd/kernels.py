"""Thin tensor-level wrappers over the C ABI (include/tcdiff_hip.h).  torch is used only for device
memory and the current HIP stream; every computation is a launcher of libtcdiff_gfx950.so."""
import ctypes as C

import torch

from . import _lib as L

TORCH_DT = {L.DT_F32: torch.float32, L.DT_BF16: torch.bfloat16, L.DT_BF16X3: torch.float32}


def dtype_id(name_or_dtype) -> int:
    if isinstance(name_or_dtype, str) and name_or_dtype == "bf16x3":
        return L.DT_BF16X3
    if name_or_dtype in ("bf16", torch.bfloat16, L.DT_BF16):
        return L.DT_BF16
    if name_or_dtype in ("f32", "fp32", torch.float32, L.DT_F32):
        return L.DT_F32
    if name_or_dtype == L.DT_BF16X3 and not isinstance(name_or_dtype, bool):
        return L.DT_BF16X3
    raise ValueError(f"unsupported compute dtype {name_or_dtype!r} (bf16, f32 or bf16x3)")


def k_tile(dt: int) -> int:
    return 64 if dt == L.DT_BF16 else 32


def _sdt(dt: int) -> int:
    """the split-bf16 mode (TC_DTYPE_BF16X3) exists on the sampler's path only (GEMM / attention / elementwise launchers of the
    denoiser); the training-step launchers never see it (TrainEngine maps the mode to f32)"""
    return L.DT_F32 if dt == L.DT_BF16X3 else dt


def to_x3(w: torch.Tensor) -> torch.Tensor:
    """fp32 [..., K] (K % 4 == 0) -> the split-bf16 storage of csrc/common.h MmaBF16x3, returned as a float32-typed tensor of the
    same shape holding the bit patterns: every 16-byte chunk of four elements becomes [hi x4 | lo x4] bf16 with hi = bf16(e),
    lo = bf16(e - hi) (round to nearest even, as v_cvt_pk_bf16_f32)."""
    w = w.to(torch.float32).contiguous()
    if w.shape[-1] % 4:
        raise ValueError("to_x3: the last dimension must be a multiple of 4")
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    q = w.shape[:-1] + (w.shape[-1] // 4, 4)
    out = torch.cat([hi.view(torch.int16).reshape(q), lo.view(torch.int16).reshape(q)], -1).contiguous()   # [..., K/4, 8] int16
    return out.view(torch.float32).reshape(w.shape)


def from_x3(t: torch.Tensor) -> torch.Tensor:
    """inverse of to_x3 (tests, diagnostics): hi + lo as fp32"""
    q = t.contiguous().view(torch.int16).reshape(t.shape[:-1] + (t.shape[-1] // 4, 8))
    hi = q[..., :4].contiguous().view(torch.bfloat16).to(torch.float32)
    lo = q[..., 4:].contiguous().view(torch.bfloat16).to(torch.float32)
    return (hi + lo).reshape(t.shape)


def round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    """device address for a c_void_p argument / struct field (a plain int converts as well as a c_void_p object and costs a third)"""
    return None if t is None else t.data_ptr()


def _row_stride(y):
    """row stride of a (B, n) view; a single row counts as contiguous, whatever stride the view carries for it"""
    return y.stride(0) if y.shape[0] > 1 else y.shape[1]


def _skeleton(parents, offsets=()):
    """the FK launchers' HOST skeleton arguments: int[24] parents and float[24][3] offsets"""
    return (C.c_int * 24)(*[int(p) for p in parents]), (C.c_float * 72)(*[float(v) for row in offsets for v in row])


def gemm_tile(dt, A, W, M, N, K, *, lda=None, ldw=None, A2=None, split_n=0, a_mod=0, mode=L.EPI_STORE_T,
              act=L.ACT_NONE, bias=None, out=None, ldc=0, out_k=None, out_v=None, scale_q=1.0, Lseq=0, Lp=0, H=0,
              n_q=0, n_k=0, tok_off=0, seq_off=0, out2=None, ldc2=0, act_src=None, ld_src=0, act2=L.ACT_NONE, seed=None,
              site=0, thr=0, drop_scale=1.0, hgroup=0, hgroup_stride=0, small_m=False):
    """out2 / act_src: the training step's fused activation epilogues; small_m: the launcher may take its small-M kernel
    (include/tcdiff_hip.h tcdiff_tile_epi)."""
    lib = L.load()
    e = L.TileEpi(mode, act, scale_q, _p(bias), _p(out), _p(out_k), _p(out_v), ldc, Lseq, Lp, H, n_q, n_k, tok_off,
                  seq_off, 0, _p(out2), ldc2, _p(act_src), ld_src, act2, _p(seed), site, thr, drop_scale, hgroup, hgroup_stride,
                  int(bool(small_m)))
    rc = lib.tcdiff_gemm_tile(dt, _p(A), _p(A2), split_n, _p(W), M, N, K, lda if lda else K, ldw if ldw else K,
                              a_mod, C.byref(e), stream())
    L.check(rc, "tcdiff_gemm_tile")


def gemm_rows_ok(dt, N, K) -> bool:
    """shapes tcdiff_gemm_rows takes (bf16, K = 512 or 1024, N a multiple of 512)"""
    return dt == L.DT_BF16 and K in (512, 1024) and N > 0 and N % 512 == 0


def gemm_rows(A, wstream, M, N, K, *, lda=None, A2=None, split_n=0, mode=L.EPI_STORE_T, bias=None, out=None, ldc=0,
              out_k=None, out_v=None, scale_q=1.0, Lseq=0, Lp=0, H=0, n_q=0, n_k=0, out2=None, ldc2=0, act_src=None, ld_src=0,
              act2=L.ACT_NONE, seed=None, site=0, thr=0, drop_scale=1.0, mt=0):
    """C[M, N] = A[M, K] Wn^T with gemm_tile's epilogues; wstream = row_streams() of Wn: [8 waves][N/512 * K/32][2048] bf16"""
    if tuple(wstream.shape) != (8, (N // 512) * (K // 32), 2048) or not wstream.is_contiguous():
        raise L.TcdiffError(f"weight stream of a [{N}, {K}] matrix must be contiguous [8, {(N // 512) * (K // 32)}, 2048], got "
                            f"{tuple(wstream.shape)}")
    e = L.TileEpi(mode, L.ACT_NONE, scale_q, _p(bias), _p(out), _p(out_k), _p(out_v), ldc, Lseq, Lp, H, n_q, n_k, 0, 0, 0,
                  _p(out2), ldc2, _p(act_src), ld_src, act2, _p(seed), site, thr, drop_scale, 0, 0)
    rc = L.load().tcdiff_gemm_rows(_p(A), _p(A2), split_n, _p(wstream), M, N, K, lda if lda else K, C.byref(e), mt, stream())
    L.check(rc, "tcdiff_gemm_rows")


def ws_table(entries, device):
    """Device table for pack_row_streams.  entries: dicts with src (fp32 tensor, element (n, k) at src.view(-1)[n sn + k sk]),
    sn, sk, N, K, dst ([8, np_dst * kst_dst, 2048] bf16) and, for a piece of a stacked matrix, np_dst, p0, kst_dst, ks0 (default:
    the whole matrix).  Returns (table tensor, n_desc, max N * K); the table holds raw pointers (the caller keeps the tensors
    alive and rebuilds it when one is reallocated)."""
    n = len(entries)
    arr = (L.WsDesc * n)()
    mx = 0
    for d, e in zip(arr, entries):
        N, K_ = e["N"], e["K"]
        if e["src"].dtype != torch.float32 or N % 512 or K_ % 32:
            raise L.TcdiffError("pack_row_streams takes fp32 sources with N % 512 == 0 and K % 32 == 0")
        npd, p0, kd, ks0 = e.get("np_dst", N // 512), e.get("p0", 0), e.get("kst_dst", K_ // 32), e.get("ks0", 0)
        if p0 + N // 512 > npd or ks0 + K_ // 32 > kd:
            raise L.TcdiffError("pack_row_streams: the piece does not fit the stream")
        if e["dst"].numel() != 8 * npd * kd * 2048 or e["dst"].element_size() != 2 or not e["dst"].is_contiguous():
            raise L.TcdiffError("pack_row_streams: dst must be a contiguous 2-byte tensor of [8, np_dst * kst_dst, 2048]")
        d.src, d.dst, d.sn, d.sk, d.N, d.K = _p(e["src"]), _p(e["dst"]), e["sn"], e["sk"], N, K_
        d.np_dst, d.p0, d.kst_dst, d.ks0 = npd, p0, kd, ks0
        mx = max(mx, N * K_)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
    return raw.to(device), n, mx


def pack_row_streams(table):
    tab, n, mx = table
    L.check(L.load().tcdiff_pack_row_streams(_p(tab), n, mx, stream()), "tcdiff_pack_row_streams")


def row_streams(W, transposed=False):
    """the stream pack of one fp32 matrix W [R, C] (a convenience over ws_table + pack_row_streams): Wn = W (N = R, K = C) or,
    transposed, Wn = W^T (N = C, K = R)"""
    R, Cc = W.shape
    N, K_ = (Cc, R) if transposed else (R, Cc)
    dst = torch.empty(8, (N // 512) * (K_ // 32), 2048, device=W.device, dtype=torch.bfloat16)
    ld = W.stride(0)
    pack_row_streams(ws_table([dict(src=W, sn=1 if transposed else ld, sk=ld if transposed else 1, N=N, K=K_, dst=dst)], W.device))
    return dst


def gemm_rowln(dt, A, W, M, K, *, flags, lda=None, ldw=None, a_mod=0, bias=None, ln_g=None, ln_b=None, ln_eps=1e-6,
               film=None, film_ld=0, xres=None, xres_mod=0, xout=None, Lseq=1, nln_g=None, nln_b=None, nln_eps=1e-5,
               hout=None, rout=None, rope=None, out_mul=1, out_add=0, groups=1):
    lib = L.load()
    e = L.RowEpi(flags, _p(bias), _p(ln_g), _p(ln_b), ln_eps, _p(film), film_ld, _p(xres), xres_mod, _p(xout), Lseq,
                 _p(nln_g), _p(nln_b), nln_eps, _p(hout), _p(rout), _p(rope), out_mul, out_add, groups)
    rc = lib.tcdiff_gemm_rowln(dt, _p(A), _p(W), M, K, lda if lda else K, ldw if ldw else K, a_mod, C.byref(e),
                               stream())
    L.check(rc, "tcdiff_gemm_rowln")


def attention(dt, Q, K, V, O, n_seq, H, Lq, Lk, Lp_q, Lp_k, ldo, n_shared=0, ng=0):
    rc = L.load().tcdiff_attention(dt, _p(Q), _p(K), _p(V), _p(O), n_seq, H, Lq, Lk, Lp_q, Lp_k, ldo, n_shared, ng,
                                   stream())
    L.check(rc, "tcdiff_attention")


def chain(mode, M, Lseq, A, wstream, *, ln_eps=1e-6, film=None, film_ld=0, xres=None,
          xout=None, n2_g=None, n2_b=None, n2_eps=1e-5,
          rope=None, q_out=None, scale_q=0.125, Lp=0, H=8, a_mod=0, xres_mod=0, b1=None, film3=None, n4_g=None,
          n4_b=None, n4_eps=1e-5, b3=None, nn_g=None, nn_b=None, nn_eps=1e-5, k_out=None, v_out=None, h_out=None,
          filmb=None, n3_g=None, n3_b=None, kf=None, vf=None, n_shared=0, nkt=0, Lk=0,
          xres_rowmajor=False, out_ld=0, dn=1, mt=0, seq_blocks=False, sa_q=None, sa_kf=None, sa_vf=None, sa_nkt=0,
          qf_out=None, kf_out=None, vf_out=None, out_nkt=0, split_part=None, p_in=None, p_out=None):
    """rope: the COLUMN-BLOCKED rotary table (to_cb(rope_table)); xres / xout: column-blocked fp32 residual stream
    (xres_rowmajor: xres is a plain [*, 512] matrix); wstream: [(dn,) 8 waves, n_stages, 2048] bf16 (or the 4-wave form
    [(dn,) 4, n_stages, 4096]: tcdiff_chain_args.nw), the stage and wave counts are read from it.  film / filmb / film3 rows are PRE-FOLDED with the LayerNorm weights / linear2 bias around them
    (fold_film below; engine.load_weights folds them into the FiLM generator).  seq_blocks / sa_* / *f_out: row blocks cut per
    sequence, the layer's self-attention inside the launch and the fragment-order Q / K / V outputs that feed it.
    split_part = 1 .. 4: the small-job form of the layer, four workgroups per 16-row block and four launches per layer
    (tcdiff_chain_split: xres -> xout not in place, p_in / p_out the partial-sum buffers); split_part = 0 with CHAIN_FRONT: layer 0's
    Q / K / V fragment images from row-major token rows.
    See include/tcdiff_hip.h tcdiff_chain_args."""
    nw = wstream.shape[-3]
    if (nw, wstream.shape[-1]) not in ((8, 2048), (4, 4096)) or not wstream.is_contiguous():
        raise L.TcdiffError("weight stream must be contiguous [.., 8 waves, n_stages, 2048] or [.., 4 waves, n_stages, 4096] bf16, "
                            f"got {tuple(wstream.shape)}")
    n_stages = wstream.shape[-2]
    a = L.ChainArgs(mode, n_stages, M, Lseq, a_mod, xres_mod, H, Lp, _p(A), _p(wstream), _p(film),
                    _p(xres), _p(xout), _p(n2_g), _p(n2_b), _p(rope), _p(q_out), _p(b1), _p(film3), _p(n4_g),
                    _p(n4_b), _p(b3), _p(nn_g), _p(nn_b), _p(k_out), _p(v_out), _p(h_out), film_ld, ln_eps, n2_eps,
                    n4_eps, nn_eps, scale_q, _p(filmb), _p(n3_g), _p(n3_b), _p(kf), _p(vf), n_shared,
                    nkt, Lk, int(bool(xres_rowmajor)), 0 if rope is None else rope.shape[1], dn, mt, out_ld, nw,
                    int(bool(seq_blocks)), _p(sa_q), _p(sa_kf), _p(sa_vf), sa_nkt, _p(qf_out), _p(kf_out), _p(vf_out), out_nkt)
    if split_part is not None:
        L.check(L.load().tcdiff_chain_split(C.byref(a), split_part, _p(p_in), _p(p_out), stream()), "tcdiff_chain_split")
        return
    L.check(L.load().tcdiff_chain(C.byref(a), stream()), "tcdiff_chain")


def fold_film(film: torch.Tensor, g, b) -> torch.Tensor:
    """[rows, 1024] raw DenseFiLM rows (scale | shift) -> the pre-folded rows the chain kernels take:
    [g (scale + 1) | b (scale + 1) + shift]; g = None stands for 1 (the feed-forward block, b = linear2's bias)."""
    sc1 = film[:, :512] + 1.0
    return torch.cat([sc1 if g is None else g * sc1, b * sc1 + film[:, 512:1024]], 1).contiguous()


def to_cb(x: torch.Tensor) -> torch.Tensor:
    """[rows, 512] -> column-blocked [64, rows, 8] (element (row, c) at ((c // 8) * rows + row) * 8 + c % 8)."""
    rows = x.shape[0]
    return x.reshape(rows, 64, 8).permute(1, 0, 2).contiguous()


def from_cb(x: torch.Tensor, rows: int) -> torch.Tensor:
    """column-blocked [64, rows, 8] (any shape with 512 * rows elements) -> [rows, 512]"""
    return x.reshape(64, rows, 8).permute(1, 0, 2).reshape(rows, 512).contiguous()


def pack_kv_frags(Kc, Vc, Kf, Vf, n_slots, H, Lp, nkt, key_lo, key_hi):
    L.check(L.load().tcdiff_pack_kv_frags(_p(Kc), _p(Vc), _p(Kf), _p(Vf), n_slots, H, Lp, nkt, key_lo, key_hi, stream()),
            "tcdiff_pack_kv_frags")


def ln_rot(dt, x, rows, g, b, eps, *, h=None, rot=None, y32=None, rope=None, pos_mod=0, pos_base=0):
    rc = L.load().tcdiff_ln_rot(dt, _p(x), rows, _p(g), _p(b), eps, _p(h), _p(rot), _p(y32), _p(rope), pos_mod,
                                pos_base, stream())
    L.check(rc, "tcdiff_ln_rot")


def rope_table(freqs, rope, n_pos):
    L.check(L.load().tcdiff_rope_table(_p(freqs), _p(rope), n_pos, stream()), "tcdiff_rope_table")


def convert_pad(dt, src, dst, rows, cols, ld_dst, rows_per_batch=None, batch_stride=0, row_stride=None):
    rpb = rows if rows_per_batch is None else rows_per_batch
    rs = cols if row_stride is None else row_stride
    rc = L.load().tcdiff_convert_pad(dt, _p(src), _p(dst), rows, cols, ld_dst, rpb, batch_stride, rs, stream())
    L.check(rc, "tcdiff_convert_pad")


def sinusoidal(dt, times_i32, n, freq, emb):
    L.check(L.load().tcdiff_sinusoidal(dt, _p(times_i32), n, _p(freq), _p(emb), stream()), "tcdiff_sinusoidal")


def mean_pool(x, out, B, S, Cn):
    L.check(L.load().tcdiff_mean_pool(_p(x), _p(out), B, S, Cn, stream()), "tcdiff_mean_pool")


def add_act(dt, a, ia, b, n, act, out=None, out32=None):
    L.check(L.load().tcdiff_add_act(dt, _p(a), _p(ia), _p(b), n, act, _p(out), _p(out32), stream()),
            "tcdiff_add_act")


def scatter_time_kv(dt, tab, n_t, tidx, Kc, Vc, NL, n_kv, H, Lp, tok0):
    rc = L.load().tcdiff_scatter_time_kv(dt, _p(tab), n_t, _p(tidx), _p(Kc), _p(Vc), NL, n_kv, H, Lp, tok0,
                                         stream())
    L.check(rc, "tcdiff_scatter_time_kv")


def step_begin(counter, tseq, tidx, n):
    L.check(L.load().tcdiff_step_begin(_p(counter), _p(tseq), _p(tidx), n, stream()), "tcdiff_step_begin")


def step_end(counter):
    L.check(L.load().tcdiff_step_end(_p(counter), stream()), "tcdiff_step_end")


def step_prologue(dt, counter, tseq, tidx, t_base, hidden, film_in, n_seq, tab, n_t, Kc, Vc, Kf, Vf, NL, n_kv, H, Lp, nkt,
                  tok0, x=None, xin=None, rows=0, nfeat=0, ld_xin=0, film_tab=None, film_out=None, film_rows=0, nfilm=0,
                  n_unc=0, parts=0):
    a = L.StepPrologueArgs(_p(counter), _p(tseq), _p(tidx), _p(t_base), _p(hidden), _p(film_in), n_seq, _p(tab), n_t,
                           _p(Kc), _p(Vc), _p(Kf), _p(Vf), NL, n_kv, H, Lp, nkt, tok0, _p(x), _p(xin), rows, nfeat,
                           ld_xin, _p(film_tab), _p(film_out), film_rows, nfilm, n_unc, parts)
    L.check(L.load().tcdiff_step_prologue(dt, C.byref(a), stream()), "tcdiff_step_prologue")


def sampler_update(mode, out_unc, out_cond, ldo, x, eps, traj, x0_out, n_rows, nfeat, Lseq, counter, params, tseq,
                   seed=0, clip0=0):
    rc = L.load().tcdiff_sampler_update(mode, _p(out_unc), _p(out_cond), ldo, _p(x), _p(eps), _p(traj), _p(x0_out),
                                        n_rows, nfeat, Lseq, _p(counter), _p(params), _p(tseq), seed, clip0,
                                        stream())
    L.check(rc, "tcdiff_sampler_update")


def window_couple(x, b, seq_len, row_elems):
    L.check(L.load().tcdiff_window_couple(_p(x), b, seq_len, row_elems, stream()), "tcdiff_window_couple")


def sampler_constrain(kind, x, mask, mask_rows, value, q_eps, n_rows, nfeat, Lseq, counter, params, tseq, seed=0, clip0=0):
    rc = L.load().tcdiff_sampler_constrain(kind, _p(x), _p(mask), mask_rows, _p(value), _p(q_eps), n_rows, nfeat, Lseq,
                                           _p(counter), _p(params), _p(tseq), seed, clip0, stream())
    L.check(rc, "tcdiff_sampler_constrain")


def window_couple_step(x, b, seq_len, row_elems, counter, params):
    L.check(L.load().tcdiff_window_couple_step(_p(x), b, seq_len, row_elems, _p(counter), _p(params), stream()),
            "tcdiff_window_couple_step")


def cfg_combine(out_unc, out_cond, ldo, w, y, n_rows, nfeat):
    L.check(L.load().tcdiff_cfg_combine(_p(out_unc), _p(out_cond), ldo, float(w), _p(y), n_rows, nfeat, stream()),
            "tcdiff_cfg_combine")


def ema_chunk_table(ma_tensors, cur_tensors, device):
    """Device table of (ma ptr, cur ptr, n) chunks of <= 65536 elements for tcdiff_ema_update (int64 [n_chunks, 3])."""
    rows = []
    for a, c in zip(ma_tensors, cur_tensors):
        n = a.numel()
        for lo in range(0, n, 65536):
            rows.append((a.data_ptr() + 4 * lo, c.data_ptr() + 4 * lo, min(65536, n - lo)))
    return torch.tensor(rows, dtype=torch.int64, device=device).reshape(-1, 3)


def ema_update(table, beta):
    L.check(L.load().tcdiff_ema_update(_p(table), table.shape[0], float(beta), float(1.0 - beta), stream()),
            "tcdiff_ema_update")



# ---- training-side rows ------------------------------------------------------------------------------------------------
def q_sample_traj(x_start, noise, t, sqrt_ac, sqrt_1mac, x_noisy, b, dn, S, Cn):
    L.check(L.load().tcdiff_q_sample_traj(_p(x_start), _p(noise), _p(t), _p(sqrt_ac), _p(sqrt_1mac), _p(x_noisy), b, dn,
                                          S, Cn, stream()), "tcdiff_q_sample_traj")


def ax_from_6v(rot6d, n_rows, per_row, row_stride, out):
    L.check(L.load().tcdiff_ax_from_6v(_p(rot6d), n_rows, per_row, row_stride, _p(out), stream()), "tcdiff_ax_from_6v")


def smpl_fk(axis_angle, root, n, parents, offsets, joints):
    L.check(L.load().tcdiff_smpl_fk(_p(axis_angle), _p(root), n, *_skeleton(parents, offsets), _p(joints), stream()), "tcdiff_smpl_fk")


def loss_terms(model_out, x_start, joints_model, joints_target, p2_weight, t, out, b, dn, S, Cn, l1):
    L.check(L.load().tcdiff_loss_terms(_p(model_out), _p(x_start), _p(joints_model), _p(joints_target), _p(p2_weight),
                                       _p(t), _p(out), b, dn, S, Cn, int(l1), stream()), "tcdiff_loss_terms")


def adan_chunk_table(params, grads, ms, vs, ns, pgs, device):
    """int64 [n_chunks, 7] device table of (p, g, m, v, n, prev_grad pointers, count) for tcdiff_adan_step."""
    rows = []
    for p, g, m, v, n, pg in zip(params, grads, ms, vs, ns, pgs):
        cnt = p.numel()
        for lo in range(0, cnt, 65536):
            o = 4 * lo
            rows.append((p.data_ptr() + o, g.data_ptr() + o, m.data_ptr() + o, v.data_ptr() + o, n.data_ptr() + o,
                         pg.data_ptr() + o, min(65536, cnt - lo)))
    return torch.tensor(rows, dtype=torch.int64, device=device).reshape(-1, 7)


def adan_step(table, scalars):
    L.check(L.load().tcdiff_adan_step(_p(table), table.shape[0], C.byref(scalars), stream()), "tcdiff_adan_step")


# ---- the Navigator's loss head and optimizer (csrc/navigator_step.hip) -------------------------------------------------
def _strides(t, n):
    """the first n strides of a view as the HOST long[n] a launcher reads them from; no view (None) stays NULL"""
    return None if t is None else (C.c_long * n)(*t.stride()[:n])


def nav_loss_blocks(n_elements: int) -> int:
    """workgroups of tcdiff_nav_loss's first stage = rows of its [n][3] workspace"""
    return (n_elements + L.NAV_LOSS_BLOCK - 1) // L.NAV_LOSS_BLOCK


def nav_loss(pre, tgt, partial, out):
    """pre, tgt: (b, dn, seq, 2) fp32 views, read by their strides; out [4] = total, recon, dis, v"""
    b, dn, seq, _ = pre.shape
    L.check(L.load().tcdiff_nav_loss(_p(pre), _strides(pre, 4), _p(tgt), _strides(tgt, 4), b, dn, seq, _p(partial), _p(out),
                                     stream()), "tcdiff_nav_loss")


def nav_loss_bwd(pre, tgt, grad_out, d_pre):
    b, dn, seq, _ = pre.shape
    L.check(L.load().tcdiff_nav_loss_bwd(_p(pre), _strides(pre, 4), _p(tgt), _strides(tgt, 4), b, dn, seq, _p(grad_out), _p(d_pre),
                                         stream()), "tcdiff_nav_loss_bwd")


def nav_adamw_rows(p, g, m, v, dst=None):
    """tcdiff_nav_adamw_chunk rows of one parameter; dst = (address, row, sr, sc) of its packed image, or None"""
    d, row, sr, sc = dst if dst is not None else (0, 1, 0, 0)
    cnt = p.numel()
    return [(p.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, m.data_ptr() + 4 * lo, v.data_ptr() + 4 * lo, d, min(65536, cnt - lo), lo,
             row, sr, sc) for lo in range(0, cnt, 65536)]


def nav_adamw_table(rows, device):
    """int64 [n_chunks, 10] device table for tcdiff_nav_adamw"""
    return torch.tensor(rows, dtype=torch.int64, device=device).reshape(-1, 10)


def nav_adamw(table, scalars):
    L.check(L.load().tcdiff_nav_adamw(_p(table), table.shape[0], C.byref(scalars), stream()), "tcdiff_nav_adamw")


# ---- training step: train-mode forward pieces and the backward pass ---------------------------------------------------
def drop_params(p: float):
    """(threshold, scale) of the counter-hash dropout (csrc/train_common.h): keep iff hash >= floor(p * 2^32)."""
    if p <= 0.0:
        return 0, 1.0
    return int(p * 4294967296.0), 1.0 / (1.0 - p)


def cast_transpose(dt, src, rows, cols, ld_src, *, dst=None, ld_dst=0, cols_pad=0, dstT=None, ld_dstT=0, rows_pad=0,
                   colsum=None):
    src_f32 = int(src.dtype == torch.float32)           # fp32 source (always, in the f32 mode) or a T-typed one
    rc = L.load().tcdiff_cast_transpose(_sdt(dt), src_f32, _p(src), rows, cols, ld_src, _p(dst), ld_dst, cols_pad, _p(dstT),
                                        ld_dstT, rows_pad, _p(colsum), stream())
    L.check(rc, "tcdiff_cast_transpose")


def gemm_splitk(dt, A, W, M, N, K, lda, ldw, out, ldc, splits):
    L.check(L.load().tcdiff_gemm_splitk(_sdt(dt), _p(A), _p(W), M, N, K, lda, ldw, _p(out), ldc, splits, stream()),
            "tcdiff_gemm_splitk")


def gemm_tn_ok(dt, M, N, K) -> bool:
    """shapes tcdiff_gemm_tn takes (everything else is repacked by cast_transpose and goes through gemm_splitk)"""
    return M % 128 == 0 and N % 128 == 0 and K % k_tile(dt) == 0


def gemm_tn(dt, A, B, M, N, K, lda, ldb, out, ldc, splits):
    """out[m][n] += sum_k A[k][m] B[k][n] (both operands row-major over the contraction index)."""
    L.check(L.load().tcdiff_gemm_tn(_sdt(dt), _p(A), _p(B), M, N, K, lda, ldb, _p(out), ldc, splits, stream()), "tcdiff_gemm_tn")


def gemm_tn_grouped(dt, problems):
    """problems: list of (A, B, M, N, K, lda, ldb, out, ldc) as gemm_tn takes them, at most L.TN_MAX_PROB: all of them in ONE
    launch with the work split evenly over the CUs (the weight gradients a decoder layer's backward has queued)."""
    n = len(problems)
    arr = (L.TnProblem * n)()
    for d, (A, B, M, N, K, lda, ldb, out, ldc) in zip(arr, problems):
        d.A, d.B, d.out = _p(A), _p(B), _p(out)
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, N, K, lda, ldb, ldc
    L.check(L.load().tcdiff_gemm_tn_grouped(_sdt(dt), arr, n, stream()), "tcdiff_gemm_tn_grouped")


def ct_table(dt, entries, device):
    """Device table for cast_transpose_multi.  entries: dicts with src (fp32 tensor view), rows, cols, ld_src and dst /
    ld_dst / cols_pad and / or dstT / ld_dstT / rows_pad.  Returns (table tensor, n_desc, n_tiles); the table holds raw
    pointers, so the caller keeps the tensors alive and rebuilds it when one of them is reallocated."""
    lib = L.load()
    n, tile0 = len(entries), 0
    arr = (L.CtDesc * n)()
    for d, e in zip(arr, entries):
        if e["src"].dtype != torch.float32:
            raise L.TcdiffError("cast_transpose_multi takes fp32 sources")
        d.src, d.dst, d.dstT = _p(e["src"]), _p(e.get("dst")), _p(e.get("dstT"))
        d.rows, d.cols, d.ld_src = e["rows"], e["cols"], e["ld_src"]
        d.ld_dst, d.cols_pad, d.ld_dstT, d.rows_pad = e.get("ld_dst", 0), e.get("cols_pad", 0), e.get("ld_dstT", 0), \
            e.get("rows_pad", 0)
        d.tile0 = tile0
        cnt = lib.tcdiff_ct_desc_init(_sdt(dt), C.byref(d))
        L.check(min(cnt, 0), "tcdiff_ct_desc_init")
        tile0 += cnt
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone()
    return raw.to(device), n, tile0


def cast_transpose_multi(dt, table):
    tab, n, tiles = table
    L.check(L.load().tcdiff_cast_transpose_multi(_sdt(dt), _p(tab), n, tiles, stream()), "tcdiff_cast_transpose_multi")


def pos_drop(x, rows, cols, pe=None, pos_mod=1, seed=None, site=0, thr=0, scale=1.0):
    """x = dropout(x + pe[row % pos_mod]) in place, fp32 rows (PositionalEncoding in train mode, model/utils.py:27-32)"""
    L.check(L.load().tcdiff_pos_drop(_p(x), rows, cols, _p(pe), pos_mod, _p(seed), site, thr, scale, stream()), "tcdiff_pos_drop")


def act_drop(dt, a, ld_a, y, ld_y, rows, cols, act, seed=None, site=0, thr=0, scale=1.0):
    a_f32 = int(a.dtype == torch.float32)
    L.check(L.load().tcdiff_act_drop(_sdt(dt), a_f32, _p(a), ld_a, _p(y), ld_y, rows, cols, act, _p(seed), site, thr, scale,
                                     stream()), "tcdiff_act_drop")


def act_drop_bwd(dt, a, ld_a, dy, ld_y, da, rows, cols, act, seed=None, site=0, thr=0, scale=1.0):
    a_f32 = int(a.dtype == torch.float32)
    L.check(L.load().tcdiff_act_drop_bwd(_sdt(dt), a_f32, _p(a), ld_a, _p(dy), ld_y, _p(da), rows, cols, act, _p(seed), site,
                                         thr, scale, stream()), "tcdiff_act_drop_bwd")


def row_args(**kw) -> "L.RowArgs":
    return L.RowArgs(**{k: (v.data_ptr() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})


def row_fwd(dt, a):
    L.check(L.load().tcdiff_row_fwd(_sdt(dt), C.byref(a), stream()), "tcdiff_row_fwd")


def row_bwd(dt, a):
    L.check(L.load().tcdiff_row_bwd(_sdt(dt), C.byref(a), stream()), "tcdiff_row_bwd")


def row_param_reduce(partials, n_blocks, d_bias=None, d_ln_g=None, d_ln_b=None, d_nln_g=None, d_nln_b=None):
    L.check(L.load().tcdiff_row_param_reduce(_p(partials), n_blocks, _p(d_bias), _p(d_ln_g), _p(d_ln_b), _p(d_nln_g),
                                             _p(d_nln_b), stream()), "tcdiff_row_param_reduce")


def attention_train(dt, Q, K, V, O, lse, n_seq, H, Lq, Lk, Lp_q, Lp_k, ldo, seed, site, thr, scale, O_lo=None):
    """O_lo (bf16 mode): a second image like O that receives what O's 8 bits dropped; hand it to attention_bwd"""
    L.check(L.load().tcdiff_attention_train(_sdt(dt), _p(Q), _p(K), _p(V), _p(O), _p(O_lo), _p(lse), n_seq, H, Lq, Lk, Lp_q, Lp_k,
                                            ldo, _p(seed), site, thr, scale, stream()), "tcdiff_attention_train")


def attention_bwd(dt, Q, K, V, O, dO, lse, delta, dQ, ld_dq, dK, dV, ld_dkv, n_seq, H, Lq, Lk, Lp_q, Lp_k, ldo, scale_q,
                  seed, site, thr, scale, O_lo=None):
    L.check(L.load().tcdiff_attention_bwd(_sdt(dt), _p(Q), _p(K), _p(V), _p(O), _p(O_lo), _p(dO), _p(lse), _p(delta), _p(dQ),
                                          ld_dq, _p(dK), _p(dV), ld_dkv, n_seq, H, Lq, Lk, Lp_q, Lp_k, ldo, scale_q, _p(seed),
                                          site, thr, scale, stream()), "tcdiff_attention_bwd")


def add_rows(a, ld_a, b, ld_b, out, ld_out, rows, cols):
    L.check(L.load().tcdiff_add_rows(_p(a), ld_a, _p(b), ld_b, _p(out), ld_out, rows, cols, stream()), "tcdiff_add_rows")


def select_rows(x, nul, keep_u8, out, B, n):
    L.check(L.load().tcdiff_select_rows(_p(x), _p(nul), _p(keep_u8), _p(out), B, n, stream()), "tcdiff_select_rows")


def select_rows_bwd(g, keep_u8, dx, dnul, B, n):
    L.check(L.load().tcdiff_select_rows_bwd(_p(g), _p(keep_u8), _p(dx), _p(dnul), B, n, stream()),
            "tcdiff_select_rows_bwd")


def pool_bwd(g_tok, g_pool, dx, B, S, Cn):
    L.check(L.load().tcdiff_pool_bwd(_p(g_tok), _p(g_pool), _p(dx), B, S, Cn, stream()), "tcdiff_pool_bwd")


def loss_total(terms, b, out):
    L.check(L.load().tcdiff_loss_total(_p(terms), b, _p(out), stream()), "tcdiff_loss_total")


def loss_terms_bwd(model_out, x_start, joints_model, joints_target, p2_weight, t, gscale, d_out, d_joints, b, dn, S, Cn,
                   l1):
    L.check(L.load().tcdiff_loss_terms_bwd(_p(model_out), _p(x_start), _p(joints_model), _p(joints_target), _p(p2_weight),
                                           _p(t), _p(gscale), _p(d_out), _p(d_joints), b, dn, S, Cn, int(l1), stream()),
            "tcdiff_loss_terms_bwd")


def fk_bwd(motion, d_joints, n, Cn, parents, offsets, d_out):
    L.check(L.load().tcdiff_fk_bwd(_p(motion), _p(d_joints), n, Cn, *_skeleton(parents, offsets), _p(d_out), stream()), "tcdiff_fk_bwd")


# ---- render-time pose export ---------------------------------------------------------------------------------------------
def pose_export(samples, b, S, dn, mode, scale, min_, fade, parents, offsets, smpl_trans, smpl_poses, full_pose, contact):
    L.check(L.load().tcdiff_pose_export(_p(samples), b, S, dn, mode, _p(scale), _p(min_), _p(fade), *_skeleton(parents, offsets), _p(smpl_trans),
                                        _p(smpl_poses), _p(full_pose), _p(contact), stream()), "tcdiff_pose_export")


def gltf_animation(smpl_poses, smpl_trans, clips, T, dn, fps, out):
    """smpl_poses (clips, T, dn, 24, 3) / smpl_trans (clips, T, dn, 3) fp32 contiguous; out (clips, T (1 + 99 dn)) fp32 contiguous"""
    L.check(L.load().tcx_gltf_animation(_p(smpl_poses), _p(smpl_trans), clips, T, dn, fps, _p(out), stream()), "tcx_gltf_animation")


def skin_vertices(smpl_poses, smpl_trans, P, v_shaped, blend, joints, offsets, parents, weights, weight_joints, V, Kw, pose_blend, origin,
                  feat, A, joints_out, out):
    """include/tcdiff_skin.h: smpl_poses (P, 24, 3) / smpl_trans (P, 3) fp32 contiguous; the model's device images; ``parents`` a
    host ctypes array of 24 ints; feat (P, 208) and A (P, 24, 12) fp32 workspaces; joints_out (P, 24, 3) or None; out (P, V, 3)"""
    L.check(L.load().tcs_skin_vertices(_p(smpl_poses), _p(smpl_trans), P, _p(v_shaped), _p(blend), _p(joints), _p(offsets),
                                       C.cast(parents, C.c_void_p), _p(weights), _p(weight_joints), V, Kw, pose_blend, origin,
                                       _p(feat), _p(A), _p(joints_out), _p(out), stream()),
            "tcs_skin_vertices")


# ---- motion ingest -------------------------------------------------------------------------------------------------------
def motion_ingest(pos, q, clips, dn, sq, parents, offsets, fit, scale, min_, feats, raw, feet, stats):
    L.check(L.load().tcdiff_motion_ingest(_p(pos), _p(q), clips, dn, sq, *_skeleton(parents, offsets), int(bool(fit)), _p(scale), _p(min_), _p(feats),
                                          _p(raw), _p(feet), _p(stats), stream()), "tcdiff_motion_ingest")


# ---- motion quality metrics ----------------------------------------------------------------------------------------------
def motion_metrics(joints, contacts, beats, up, fps, contact_threshold, still, radius, sigma_smooth, sigma_beat, ws, iws, pfc,
                   contact_slide, contact_break, contact_frames, collision_rate, beat_align, motion_beats):
    """joints (b, dn, T, 24, 3) / contacts (b, dn, T, 4) fp32 views, read by their strides; beats (b, T) uint8 contiguous"""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcdiff_motion_metrics(_p(joints), _strides(joints, 3), _p(contacts), _strides(contacts, 3), _p(beats), b, dn, T, up, fps,
                                           contact_threshold, still, radius, sigma_smooth, sigma_beat, _p(ws), _p(iws), _p(pfc), _p(contact_slide),
                                           _p(contact_break), _p(contact_frames), _p(collision_rate), _p(beat_align), _p(motion_beats), stream()),
            "tcdiff_motion_metrics")


# ---- set-level metrics -----------------------------------------------------------------------------------------------------
def kinetic_features(joints, up, window, fps, feats):
    """joints (b, dn, T, 24, 3) fp32 view, read by its strides; feats (b, dn, 72) float64 contiguous"""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcdiff_kinetic_features(_p(joints), _strides(joints, 3), b, dn, T, up, window, fps, _p(feats), stream()),
            "tcdiff_kinetic_features")


def geometric_features(joints, up, table, rng, time_per_frame, feats):
    """joints (b, dn, T, 24, 3) fp32 view, read by its strides; table (R, 5) int32 and rng (R, 2) float64 contiguous on the device;
    feats (b, dn, R) float64 contiguous"""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcdiff_geometric_features(_p(joints), _strides(joints, 3), b, dn, T, up, _p(table), _p(rng), table.shape[0],
                                               time_per_frame, _p(feats), stream()), "tcdiff_geometric_features")


def set_stats(feats, fit, mean, std, z, zc, mu, cov, div_rows):
    """feats (N, D) float64 contiguous; fit: mean / std are written, else read; z, zc (D, N) workspaces; div_rows (N,) or None"""
    N, D = feats.shape
    L.check(L.load().tcdiff_set_stats(_p(feats), N, D, int(bool(fit)), _p(mean), _p(std), _p(z), _p(zc), _p(mu), _p(cov),
                                      _p(div_rows), stream()), "tcdiff_set_stats")


def set_scores(ref_mu, ref_cov, mu, cov, div_rows, max_sweeps, fid, div, status):
    L.check(L.load().tcdiff_set_scores(_p(ref_mu), _p(ref_cov), _p(mu), _p(cov), _p(div_rows), div_rows.numel(), mu.numel(),
                                       max_sweeps, _p(fid), _p(div), _p(status), stream()), "tcdiff_set_scores")


def set_check(status):
    """waits for the stream; raises if the eigen-solver of the tcdiff_set_scores call that wrote ``status`` hit its sweep cap"""
    L.check(L.load().tcdiff_set_check(_p(status), stream()), "tcdiff_set_check")


# ---- music features: the STFT path -------------------------------------------------------------------------------------------
def music_stft(y, tab, D, S, M, frame_max):
    """y (B, n) fp32 view read through its row stride; tab: music._tables; D (B, T, 1025, 2) and S (B, T, 1025), both or neither;
    M (B, T, 128) and its maximum per frame, frame_max (B, T)"""
    B, n = y.shape
    L.check(L.load().tcdiff_music_stft(_p(y), _row_stride(y), B, n, _p(tab["twiddle"]), _p(tab["window"]), _p(tab["mel_w"]), _p(tab["mel_range"]),
                                       _p(D), _p(S), _p(M), _p(frame_max), stream()), "tcdiff_music_stft")


def music_mfcc(M, frame_max, tab, mx, mel_db, feats):
    """M (B, T, 128), frame_max (B, T) of music_stft -> mx (B,) workspace, mel_db (B, T, 128), columns 0-39 of feats (B, T, 425)"""
    B, T = M.shape[:2]
    L.check(L.load().tcdiff_music_mfcc(_p(M), _p(frame_max), B, T, _p(tab["dct"]), _p(mx), _p(mel_db), _p(feats), stream()), "tcdiff_music_mfcc")


def music_hpss(D, S, n, tab, H, P, frames, percussive, harmonic):
    """D, S of music_stft -> H, P (B, T, 1025) and frames (B, W, T, 2048) workspaces; percussive and (or None) harmonic (B, n)"""
    B = S.shape[0]
    L.check(L.load().tcdiff_music_hpss(_p(D), _p(S), B, n, _p(tab["twiddle"]), _p(tab["window"]), _p(H), _p(P), _p(frames),
                                       _p(percussive), _p(harmonic), stream()), "tcdiff_music_hpss")


def music_onset(M, frame_max, tab, mx, onset_env, feats):
    """M (B, T, 128), frame_max (B, T): music_stft of the percussive signal -> mx (B,) workspace, onset_env (B, T), columns 40-424 of feats"""
    B, T = M.shape[:2]
    L.check(L.load().tcdiff_music_onset(_p(M), _p(frame_max), B, T, _p(tab["tempo_window"]), _p(mx), _p(onset_env), _p(feats), stream()),
            "tcdiff_music_onset")


# ---- music features: the beat track -------------------------------------------------------------------------------------------
def beat_tempo(o, window, partial):
    """o (B, T) fp32 view read through its row stride; window (480,) fp32 -> partial (B, ceil(T / 8), 480) float64.  One launch."""
    B, T = o.shape
    L.check(L.load().tcdiff_beat_tempo(_p(o), _row_stride(o), B, T, _p(window), _p(partial), stream()), "tcdiff_beat_tempo")


def beat_track(o, partial, prior, tables, period_host, trim, local_score, cum_score, backlink, beats_ws, onset_beat, period, n_beats, tempo):
    """o (B, T) fp32 view; either partial of beat_tempo with prior (480,) float64, or period_host: the B ints the caller has put
    into period (the launcher checks their range on the host); tables: music._beat_tables -> local_score, cum_score (B, T) float64, backlink (B, T) int32, beats_ws (B, T) int32
    workspace, onset_beat (B, T) fp32, period, n_beats (B,) int32, tempo (B,) float64 (the caller's when the period is given).
    One launch."""
    B, T = o.shape
    ph = None if period_host is None else (C.c_int * B)(*[int(p) for p in period_host])
    L.check(L.load().tcdiff_beat_track(_p(o), _row_stride(o), B, T, _p(partial), _p(prior), _p(tables), ph, int(bool(trim)), _p(local_score),
                                       _p(cum_score), _p(backlink), _p(beats_ws), _p(onset_beat), _p(period), _p(n_beats), _p(tempo), stream()),
            "tcdiff_beat_track")


# ---- music features: the chroma columns --------------------------------------------------------------------------------------
def chroma_pyramid(y, taps, pyramid):
    """y (B, n) fp32 view read through its row stride; taps (63,) fp32 -> pyramid (B, sum_s ceil(n / 2^s)), the six decimated
    signals one after another.  One launch."""
    B, n = y.shape
    L.check(L.load().tcdiff_chroma_pyramid(_p(y), _row_stride(y), B, n, _p(taps), _p(pyramid), stream()), "tcdiff_chroma_pyramid")


def chroma_tuning(S, f_lo, f_hi, bin_hz, edges, pitch_ws, mag_ws, tuning_index, n_pitches, threshold, counts):
    """S (B, T, 1025) of music_stft; bins f_lo .. f_hi, bin_hz = sr / 2048; edges (101,) float64; pitch_ws, mag_ws
    (B, T, f_hi - f_lo + 1) workspaces -> tuning_index, n_pitches (B,) int32, threshold (B,) fp32, counts (B, 100) int32.  One launch."""
    B, T = S.shape[:2]
    L.check(L.load().tcdiff_chroma_tuning(_p(S), B, T, f_lo, f_hi, bin_hz, _p(edges), _p(pitch_ws), _p(mag_ws), _p(tuning_index),
                                          _p(n_pitches), _p(threshold), _p(counts), stream()), "tcdiff_chroma_tuning")


def chroma_response(y, pyramid, tuning_index, tab, chroma, cqt_mag):
    """y (B, n) fp32 view, its pyramid, tuning_index (B,) int32 on the device; tab: music._chroma_tables -> chroma (B, T, 12) and
    (or None) cqt_mag (B, T, 252).  One launch."""
    B, n = y.shape
    L.check(L.load().tcdiff_chroma_response(_p(y), _row_stride(y), _p(pyramid), B, n, _p(tuning_index), _p(tab["twiddle"]), _p(tab["basis"]),
                                            _p(tab["band"]), _p(tab["scale"]), _p(chroma), _p(cqt_mag), stream()), "tcdiff_chroma_response")


# ---- audio files: decode, downmix, resample ----------------------------------------------------------------------------------
def audio_decode(data, frames, channels, fmt, out):
    """data (B, row_stride) uint8, each row a file's data-chunk bytes (row_stride a multiple of 4); fmt: a key of _lib.AUDIO_FMT
    -> out (B, frames) fp32 mono.  One launch."""
    B = data.shape[0]
    L.check(L.load().tcdiff_audio_decode(_p(data), data.stride(0), B, frames, channels, L.AUDIO_FMT[fmt], _p(out), stream()),
            "tcdiff_audio_decode")


def audio_resample(y, table, inc, scale, step, n_out, out):
    """y (B, n) fp32 view read through its row stride (rows may overlap); table (32769, 2) fp32 (win, delta); inc, scale float64
    and step as the header defines them -> out (B, size) fp32, samples n_out .. size - 1 zero.  One launch."""
    B, n = y.shape
    L.check(L.load().tcdiff_audio_resample(_p(y), _row_stride(y), B, n, _p(table), inc, scale, step, n_out, out.shape[1], _p(out), stream()),
            "tcdiff_audio_resample")


# ---- stick-figure frames ---------------------------------------------------------------------------------------------------
def draw_project(joints, contacts, view, floor, up, contact_threshold, still, pts, trail, order, planted):
    """joints (b, dn, T, 24, 3) / contacts (b, dn, T, 4) fp32 views, read by their strides; view: 12 floats (row-major 3 x 4)"""
    b, dn, T = joints.shape[:3]
    v = None if view is None else (C.c_float * 12)(*[float(x) for x in view])
    L.check(L.load().tcdiff_draw_project(_p(joints), _strides(joints, 3), _p(contacts), _strides(contacts, 3), b, dn, T, v, floor, up,
                                         contact_threshold, still, _p(pts), _p(trail), _p(order), _p(planted), stream()), "tcdiff_draw_project")


def draw_raster(pts, trail, order, planted, b, dn, T, W, H, parents, static_segs, n_static, colors, n_colors, style, frames):
    """style: an _lib.DrawStyle; frames: a uint8 tensor or a device address (frames placed inside a larger buffer)"""
    par = None if parents is None else _skeleton(parents)[0]
    out = frames if frames is None or isinstance(frames, int) else frames.data_ptr()
    L.check(L.load().tcdiff_draw_raster(_p(pts), _p(trail), _p(order), _p(planted), b, dn, T, W, H, par, _p(static_segs), n_static,
                                        _p(colors), n_colors, None if style is None else C.byref(style), out, stream()),
            "tcdiff_draw_raster")


# ---- shaded meshes (include/tcdiff_shade.h) ----------------------------------------------------------------------------------
def mesh_vertices(vertices, faces, adj_start, adj_faces, P, V, F, view, screen, normals):
    """vertices (P, V, 3) fp32 contiguous; faces (F, 3) int32; the CSR adjacency; view: 12 floats; screen / normals (P, V, 3) or None"""
    v = None if view is None else (C.c_float * 12)(*[float(x) for x in view])
    L.check(L.load().tcr_mesh_vertices(_p(vertices), _p(faces), _p(adj_start), _p(adj_faces), P, V, F, v, _p(screen), _p(normals),
                                       stream()), "tcr_mesh_vertices")


def mesh_raster(screen, normals, faces, b, T, dn, V, F, W, H, colors, n_colors, style, under, scratch, frames):
    """style: an _lib.ShadeStyle; scratch: an int32 tensor; frames: a uint8 tensor or a device address (frames placed inside a
    larger buffer)"""
    out = frames if frames is None or isinstance(frames, int) else frames.data_ptr()
    L.check(L.load().tcr_mesh_raster(_p(screen), _p(normals), _p(faces), b, T, dn, V, F, W, H, _p(colors), n_colors,
                                     None if style is None else C.byref(style), _p(under), _p(scratch),
                                     0 if scratch is None else scratch.numel() * scratch.element_size(), out, stream()),
            "tcr_mesh_raster")


# ---- Motion-JPEG frames (include/tcdiff_mjpeg.h) -------------------------------------------------------------------------------
def mjpeg_workspace(N, H, W, subsampling) -> int:
    """the bytes of workspace mjpeg_plan and mjpeg_write need"""
    n = C.c_long(0)
    L.check(L.load().tcj_mjpeg_workspace(N, H, W, subsampling, C.byref(n)), "tcj_mjpeg_workspace")
    return n.value


def mjpeg_plan(frames, quality, subsampling, workspace, offsets):
    """frames (N, H, W, 3) uint8, read through its strides; workspace: a uint8 tensor; offsets (N + 1,) int64"""
    N, H, W, _ = frames.shape
    strides = (C.c_long * 3)(*frames.stride()[:3])
    L.check(L.load().tcj_mjpeg_plan(_p(frames), strides, N, H, W, quality, subsampling, _p(workspace),
                                    0 if workspace is None else workspace.numel() * workspace.element_size(), _p(offsets), stream()),
            "tcj_mjpeg_plan")


def mjpeg_write(N, H, W, quality, subsampling, workspace, data):
    """data: a uint8 tensor of at least offsets[N] bytes (a view inside a larger buffer is written in place)"""
    L.check(L.load().tcj_mjpeg_write(N, H, W, quality, subsampling, _p(workspace),
                                     0 if workspace is None else workspace.numel() * workspace.element_size(), _p(data),
                                     0 if data is None else data.numel(), stream()), "tcj_mjpeg_write")


# ---- the foot lock (include/tcdiff_footlock.h) ---------------------------------------------------------------------------------
def foot_lock_workspace(b, dn, T) -> int:
    """the bytes of workspace foot_lock needs"""
    n = C.c_long(0)
    L.check(L.load().tck_foot_lock_workspace(b, dn, T, C.byref(n)), "tck_foot_lock_workspace")
    return n.value


def foot_lock(q, pos, contacts, b, dn, T, contact_threshold, still, blend, reach, parents, offsets, workspace, q_out, joints, planted,
              clamped, max_shift):
    """q (b, T dn, 24, 3) / pos (b, T dn, 3) fp32 contiguous; contacts (b, dn, T, 4) fp32 view read by its strides, or None; workspace:
    a uint8 tensor; q_out like q; joints (b, dn, T, 24, 3) or None; planted, clamped (b, dn, 2) int32; max_shift (b, dn, 2) float64.
    Three launches."""
    L.check(L.load().tck_foot_lock(_p(q), _p(pos), _p(contacts), _strides(contacts, 4), b, dn, T, contact_threshold, still, blend, reach,
                                   *_skeleton(parents, offsets), _p(workspace),
                                   0 if workspace is None else workspace.numel() * workspace.element_size(), _p(q_out), _p(joints),
                                   _p(planted), _p(clamped), _p(max_shift), stream()), "tck_foot_lock")


# ---- the group metrics (include/tcdiff_group.h) --------------------------------------------------------------------------------
def group_workspace(b, dn, T, max_lag) -> int:
    """the bytes of workspace group_metrics needs"""
    n = C.c_long(0)
    L.check(L.load().tcg_group_workspace(b, dn, T, max_lag, C.byref(n)), "tcg_group_workspace")
    return n.value


def group_metrics(joints, up, fps, parents, radii, window, max_lag, sigma_floor, workspace, gap, closest, contact_rate, gap_min, episodes,
                  closest_min, crossings, crossing_rate, sync, sync_lag, sync_zero):
    """joints (b, dn, T, 24, 3) fp32 view, read by its strides; parents: 24 ints, radii: 24 floats (host); workspace: a uint8 tensor;
    gap (b, P, T) float64 / closest (b, P, T) int32 contiguous or None; the nine (b, P) outputs, closest_min (b, P, 3).  Three launches."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcg_group_metrics(_p(joints), _strides(joints, 3), b, dn, T, up, fps, (C.c_int * 24)(*parents), (C.c_double * 24)(*radii),
                                       window, max_lag, sigma_floor, _p(workspace),
                                       0 if workspace is None else workspace.numel() * workspace.element_size(), _p(gap), _p(closest),
                                       _p(contact_rate), _p(gap_min), _p(episodes), _p(closest_min), _p(crossings), _p(crossing_rate),
                                       _p(sync), _p(sync_lag), _p(sync_zero), stream()), "tcg_group_metrics")


# ---- keeping the dancers apart (include/tcdiff_apart.h) -------------------------------------------------------------------------
def keep_apart_workspace(b, dn, T) -> int:
    """the bytes of workspace keep_apart needs"""
    n = C.c_long(0)
    L.check(L.load().tcp_keep_apart_workspace(b, dn, T, C.byref(n)), "tcp_keep_apart_workspace")
    return n.value


def keep_apart(pos, joints, up, parents, radii, mobility, margin, iterations, rounds, blend, max_push, workspace, pos_out, joints_out, shift,
               contact_before, contact_after, gap_min_before, gap_min_after, pushed, capped, max_shift, max_step):
    """pos (b, T dn, 3) fp32 contiguous; joints (b, dn, T, 24, 3) fp32 view, read by its strides; parents: 24 ints, radii: 24 floats,
    mobility: dn floats (host); workspace: a uint8 tensor; pos_out / joints_out contiguous; shift (b, dn, T, 2) float64 or None; the
    six (b, P) and two (b, dn) outputs.  2 rounds + 3 launches."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcp_keep_apart(_p(pos), _p(joints), _strides(joints, 3), b, dn, T, up, (C.c_int * 24)(*parents), (C.c_double * 24)(*radii),
                                    (C.c_double * dn)(*mobility), margin, iterations, rounds, blend, max_push, _p(workspace),
                                    0 if workspace is None else workspace.numel() * workspace.element_size(), _p(pos_out), _p(joints_out),
                                    _p(shift), _p(contact_before), _p(contact_after), _p(gap_min_before), _p(gap_min_after), _p(pushed),
                                    _p(capped), _p(max_shift), _p(max_step), stream()), "tcp_keep_apart")


# ---- putting the dancers on the floor (include/tcdiff_ground.h) ----------------------------------------------------------------
def ground_workspace(b, dn, T) -> int:
    """the bytes of workspace ground and ground_metrics need"""
    n = C.c_long(0)
    L.check(L.load().tcf_ground_workspace(b, dn, T, C.byref(n)), "tcf_ground_workspace")
    return n.value


def ground_metrics(joints, contacts, up, parents, radii, floor_in, contact_threshold, still, tolerance, workspace, floor, counts, values):
    """joints (b, dn, T, 24, 3) fp32 view and contacts (b, dn, T, 4) fp32 view or None, read by their strides; parents: 24 ints, radii:
    24 floats (host); floor_in (b,) float64 or None; workspace: a uint8 tensor; floor (b,) float64; counts (3, b, dn) int64, values
    (3, b, dn) float64.  Three launches, two with floor_in."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcf_ground_metrics(_p(joints), _strides(joints, 3), _p(contacts), _strides(contacts, 4), b, dn, T, up,
                                        (C.c_int * 24)(*parents), (C.c_double * 24)(*radii), _p(floor_in), contact_threshold, still, tolerance,
                                        _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(), _p(floor),
                                        _p(counts), _p(values), stream()), "tcf_ground_metrics")


def ground(pos, joints, contacts, up, parents, radii, floor_in, contact_threshold, still, tolerance, blend, max_lift, workspace, pos_out,
           joints_out, shift, floor, counts_before, values_before, counts_after, values_after, capped, max_shift, max_step):
    """pos (b, T dn, 3) fp32 contiguous; joints and contacts as for ground_metrics; pos_out / joints_out contiguous; shift (b, dn, T)
    float64 or None; floor (b,); counts_* (3, b, dn) int64, values_* (3, b, dn) float64; capped (b, dn) int64, max_shift / max_step
    (b, dn) float64.  Five launches, four with floor_in."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcf_ground(_p(pos), _p(joints), _strides(joints, 3), _p(contacts), _strides(contacts, 4), b, dn, T, up,
                                (C.c_int * 24)(*parents), (C.c_double * 24)(*radii), _p(floor_in), contact_threshold, still, tolerance, blend,
                                max_lift, _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(), _p(pos_out),
                                _p(joints_out), _p(shift), _p(floor), _p(counts_before), _p(values_before), _p(counts_after),
                                _p(values_after), _p(capped), _p(max_shift), _p(max_step), stream()), "tcf_ground")


# ---- mesh-level contact between the skinned bodies (include/tcdiff_meshcontact.h) ----------------------------------------------------
def mesh_contact_workspace(b, dn, T, V, F) -> int:
    """the bytes of workspace mesh_contact needs"""
    n = C.c_long(0)
    L.check(L.load().tcm_mesh_contact_workspace(b, dn, T, V, F, C.byref(n)), "tcm_mesh_contact_workspace")
    return n.value


def mesh_contact(vertices, faces, faces_host, dn, up, workspace, inside, depth, rate, episodes, depth_max, deepest, inside_mean):
    """vertices (b, T dn, V, 3) fp32 view, read by its two leading strides; faces (F, 3) int32 on the device and faces_host, the same
    as a contiguous int32 numpy array; workspace: a uint8 tensor; inside (b, P, T, 2) int32 and depth (b, P, T) float64 or None; rate,
    depth_max, inside_mean (b, P) float64; episodes (b, P) and deepest (b, P, 3) int64.  Three launches, none with one dancer."""
    b, rows, V = vertices.shape[:3]
    F = faces_host.shape[0]
    L.check(L.load().tcm_mesh_contact(_p(vertices), _strides(vertices, 2), _p(faces), faces_host.ctypes.data, b, dn, rows // dn,
                                      V, F, up, _p(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size(),
                                      _p(inside), _p(depth), _p(rate), _p(episodes), _p(depth_max), _p(deepest), _p(inside_mean), stream()),
            "tcm_mesh_contact")


# ---- a dancer's contact with itself (include/tcdiff_selfcontact.h) ---------------------------------------------------------------
def self_contact_workspace(b, dn, T) -> int:
    """the bytes of workspace self_contact needs"""
    n = C.c_long(0)
    L.check(L.load().tci_self_contact_workspace(b, dn, T, C.byref(n)), "tci_self_contact_workspace")
    return n.value


def self_contact(joints, parents, radii, mask, tolerance, workspace, gap, closest, rate, gap_min, episodes, closest_min, depth_mean,
                 pair_frames):
    """joints (b, dn, T, 24, 3) fp32 view, read by its strides; parents: 24 ints, radii: 24 floats, mask: four 64-bit words (host);
    workspace: a uint8 tensor; gap (b, dn, T) float64 / closest (b, dn, T) int32 contiguous or None; rate, gap_min, depth_mean (b, dn)
    float64; episodes (b, dn), closest_min (b, dn, 3) and pair_frames (b, dn, 253) int64.  Two launches."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tci_self_contact(_p(joints), _strides(joints, 3), b, dn, T, (C.c_int * 24)(*parents), (C.c_double * 24)(*radii),
                                      (C.c_uint64 * 4)(*mask), tolerance, _p(workspace),
                                      0 if workspace is None else workspace.numel() * workspace.element_size(), _p(gap), _p(closest),
                                      _p(rate), _p(gap_min), _p(episodes), _p(closest_min), _p(depth_mean), _p(pair_frames), stream()),
            "tci_self_contact")


# ---- the jitter scores and the rotation filter (include/tcdiff_smooth.h) -----------------------------------------------------------
def smoothness(joints, fps, accel_mean, jitter, jitter_local, root_jitter, accel_max, jitter_max, accel_peak, jitter_peak, terms):
    """joints (b, dn, T, 24, 3) fp32 view, read by its strides; the six (b, dn) float64 outputs, accel_peak / jitter_peak (b, dn, 2) and
    terms (b, dn) int32.  One launch."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcw_smoothness(_p(joints), _strides(joints, 3), b, dn, T, fps, _p(accel_mean), _p(jitter), _p(jitter_local),
                                    _p(root_jitter), _p(accel_max), _p(jitter_max), _p(accel_peak), _p(jitter_peak), _p(terms), stream()),
            "tcw_smoothness")


def smooth_workspace(b, dn, T) -> int:
    """the bytes of workspace smooth needs"""
    n = C.c_long(0)
    L.check(L.load().tcw_smooth_workspace(b, dn, T, C.byref(n)), "tcw_smooth_workspace")
    return n.value


def smooth(q, pos, b, dn, T, window, taps, root_window, root_taps, joints_mask, parents, offsets, workspace, q_out, pos_out, joints, joints_in,
           max_rot_change, max_pos_change, copied):
    """q (b, T dn, 24, 3) / pos (b, T dn, 3) fp32 contiguous; taps (window, window) / root_taps (root_window, root_window) float64 on the
    device; joints_mask: 24 bits; workspace: a uint8 tensor; q_out / pos_out like q / pos; joints, joints_in (b, dn, T, 24, 3) or None;
    max_rot_change, max_pos_change (b, dn) float64; copied (b, dn) int32.  Two launches."""
    L.check(L.load().tcw_smooth(_p(q), _p(pos), b, dn, T, window, _p(taps), root_window, _p(root_taps), joints_mask,
                                *_skeleton(parents, offsets), _p(workspace),
                                0 if workspace is None else workspace.numel() * workspace.element_size(), _p(q_out), _p(pos_out), _p(joints),
                                _p(joints_in), _p(max_rot_change), _p(max_pos_change), _p(copied), stream()), "tcw_smooth")


# ---- the choreography planner and its closing check (include/tcdiff_choreo.h) -----------------------------------------------------
def choreo_plan(points, keys, counts, frames, fps, scale, min_, min_distance, max_speed, traj, x0, status, clamped, speed_max, speed_peak,
                too_fast, path_length, dist_min, dist_min_frame, too_close):
    """points (b, dn, K, 2) fp32 contiguous; keys (K,) or (b, dn, K) int32; counts (b, dn) int32 or None; scale / min_: two HOST floats
    each or None; traj (b, dn, frames, 2), x0 (b, frames dn, 3) fp32; the per-dancer reports (b, dn), the per-pair reports
    (b, dn (dn - 1) / 2) (None with one dancer).  Two launches, one with one dancer."""
    b, dn, K, _ = points.shape
    norm = (None, None) if scale is None else ((C.c_float * 2)(*scale), (C.c_float * 2)(*min_))
    L.check(L.load().tcc_plan(_p(points), _p(keys), int(keys.dim() == 3), _p(counts), b, dn, K, frames, fps, norm[0], norm[1], min_distance,
                              max_speed, _p(traj), _p(x0), _p(status), _p(clamped), _p(speed_max), _p(speed_peak), _p(too_fast),
                              _p(path_length), _p(dist_min), _p(dist_min_frame), _p(too_close), stream()), "tcc_plan")


def trajectory_error(joints, traj, up, err_mean, err_max, err_final, err_peak, counted):
    """joints (b, dn, T, 24, 3) fp32 view, read by its strides; traj (b, dn, T, 2) fp32 contiguous; err_mean, err_max, err_final (b, dn)
    float64; err_peak, counted (b, dn) int32.  One launch."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcc_trajectory_error(_p(joints), _strides(joints, 3), _p(traj), b, dn, T, up, _p(err_mean), _p(err_max), _p(err_final),
                                          _p(err_peak), _p(counted), stream()), "tcc_trajectory_error")


# ---- the kinematic beats and the time warp onto the music's (include/tcdiff_beatsync.h) ------------------------------------------
def beat_sync_workspace(b, dn, T) -> int:
    """the bytes of workspace motion_beats and beat_sync need"""
    n = C.c_long(0)
    L.check(L.load().tcb_beat_sync_workspace(b, dn, T, C.byref(n)), "tcb_beat_sync_workspace")
    return n.value


def motion_beats(joints, share, rad, weights, workspace, speed, kin, kin_count):
    """joints (b, dn, T, 24, 3) fp32 view, read by its strides; weights (2 rad + 1,) float64 on the device; workspace: a uint8 tensor;
    speed (b, W, T - 1) float64, kin (b, W, T) uint8, kin_count (b, W) int32, W = 1 if share else dn.  Two launches."""
    b, dn, T = joints.shape[:3]
    L.check(L.load().tcb_motion_beats(_p(joints), _strides(joints, 3), b, dn, T, int(share), rad, _p(weights), _p(workspace),
                                      0 if workspace is None else workspace.numel() * workspace.element_size(), _p(speed), _p(kin),
                                      _p(kin_count), stream()), "tcb_motion_beats")


def beat_sync(q, pos, contacts, beats, b, dn, T, share, max_shift, max_rate, strength, rad, weights, parents, offsets, workspace, q_out, pos_out,
              contacts_out, joints, joints_in, warp, speed, kin, status, kin_count, music_count, matched, dropped, anchors, shift_max, rate_min,
              rate_max, rate_min_frame, rate_max_frame, moved, copied):
    """q (b, T dn, 24, 3) / pos (b, T dn, 3) fp32 contiguous; contacts (b, dn, T, 4) fp32 contiguous or None (then contacts_out is None);
    beats (b, T) uint8; weights (2 rad + 1,) float64 on the device; workspace: a uint8 tensor; q_out / pos_out / contacts_out like their
    inputs; joints, joints_in (b, dn, T, 24, 3), joints_in or None; the per-warp outputs (b, W[, T]), moved / copied (b, dn).  Three
    launches."""
    L.check(L.load().tcb_beat_sync(_p(q), _p(pos), _p(contacts), _p(beats), b, dn, T, int(share), max_shift, max_rate, strength, rad, _p(weights),
                                   *_skeleton(parents, offsets), _p(workspace),
                                   0 if workspace is None else workspace.numel() * workspace.element_size(), _p(q_out), _p(pos_out),
                                   _p(contacts_out), _p(joints), _p(joints_in), _p(warp), _p(speed), _p(kin), _p(status), _p(kin_count),
                                   _p(music_count), _p(matched), _p(dropped), _p(anchors), _p(shift_max), _p(rate_min), _p(rate_max),
                                   _p(rate_min_frame), _p(rate_max_frame), _p(moved), _p(copied), stream()), "tcb_beat_sync")
