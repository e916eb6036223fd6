"""The Dance-Beat Navigator on the MI355X: `TrajDecoder` (TrajDecoder/model/traj_model.py:125-200) and the sliding-window
rollout of `TCDiff.test_loop` (TCDiff.py:526-547), as HIP kernels (csrc/navigator.hip); `TrajTrainer` beside the module is the
train-mode forward and the backward pass of TrajDecoder/train_traj.py (csrc/navigator_train.hip); `traj_loss` and `TrajAdamW` are that
step's loss head and optimizer (csrc/navigator_step.hip).

    traj_model = TrajDecoder(nfeats=2, trans_layer=6, window_size=100)
    traj_model.load_state_dict(ckpt["net"], strict=True)                 # the reference's checkpoint, key for key
    traj_model.cuda().eval()
    x_traj = rollout(traj_model, x[:, :, :, [4, 5]], cond, step=25)      # (b, dn, window + n_windows * step, 2)
    x_0 = smooth_x0(x_traj)                                              # Kalman smoothing, zero z, frame-major (csrc/handoff.hip)
    x_0 = rollout_x0(traj_model, x[:, :, :, [4, 5]], cond, step=25)      # both, nothing in between

What the module computes, restated (everything fp32, eval-mode dropouts are identities):

* `lstm`: 3-layer `nn.LSTM(2 -> 64)` on x reshaped to (b, dn * seq, 2).  The reference builds it WITHOUT `batch_first`, so
  **the recurrence runs over the clip index b** and the dn * seq positions are its independent batch: clip i's output depends
  on clips 0 .. i - 1 (one clip alone and the same clip inside a batch differ by ~1e-3).  The checkpoint was trained that
  way; the kernel reproduces it.
* `music_projection`: frames paired to (b, n // 2, 876) (an odd last frame dropped), 876 -> 438 -> 438 -> 64 with
  LeakyReLU(0.01).
* `trans_extractor`: PositionalEncoding rows 0 .. dn * seq - 1 added to the LSTM output (max_len 500: more positions raise, as
  in the reference), [cond_emb(music[:, :seq]) repeated dn times | that] -> width 128, `trans_layer` pre-norm blocks: Q / K / V
  with biases, 4 heads of 32, scale 1 / sqrt(32), **no mask** (the `attn.mask` buffers are registered and never read), proj,
  MLP 128 -> 512 -> 128 with the erf GELU.  `traj_emb` is a parameter forward never uses.  Both are kept for the state_dict.
* `Decoder`: [features | music[:, -seq:] repeated dn times] (192) -> 128 -> 128 -> 64 -> 2 with LeakyReLU, back to
  (b, dn, seq, 2).

`rollout` hoists the music front: window starts are even, so a window's frame pairs are pairs of the whole `cond`; the two
tables are computed once for all cond_len // 2 pairs and every window reads its rows.  A row of the kernel's products depends
on its own input row only, so hoisting changes no bits.
"""
import ctypes as C
import math

import torch
import torch.nn as nn

from . import _lib as L
from . import io as tio
from . import kernels as K

MAX_POS = 500                      # PositionalEncoding max_len (model/utils.py:12)
_BK, _DC, _MU = 198272, 50512, 628736          # packed sizes (csrc/navigator.hip)


class _PositionalEncoding(nn.Module):
    def __init__(self, d_model, dropout, max_len=MAX_POS):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        pos = torch.arange(0, max_len).unsqueeze(1)
        div = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
        pe = torch.zeros(max_len, d_model)
        pe[:, 0::2] = torch.sin(pos * div)
        pe[:, 1::2] = torch.cos(pos * div)
        self.register_buffer("pe", pe.unsqueeze(1))          # (max_len, 1, d_model)


class _Attention(nn.Module):
    def __init__(self, dim, block_size, dropout):
        super().__init__()
        self.key = nn.Linear(dim, dim)
        self.query = nn.Linear(dim, dim)
        self.value = nn.Linear(dim, dim)
        self.attn_drop = nn.Dropout(dropout)
        self.resid_drop = nn.Dropout(dropout)
        self.proj = nn.Linear(dim, dim)
        # part of the reference's state_dict; its forward never applies it
        self.register_buffer("mask", torch.tril(torch.ones(block_size, block_size)).view(1, 1, block_size, block_size))


class _Block(nn.Module):
    def __init__(self, dim, block_size, dropout):
        super().__init__()
        self.ln1 = nn.LayerNorm(dim)
        self.ln2 = nn.LayerNorm(dim)
        self.attn = _Attention(dim, block_size, dropout)
        self.mlp = nn.Sequential(nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim), nn.Dropout(dropout))


class _Extractor(nn.Module):
    def __init__(self, dim, block_size, layers, dropout):
        super().__init__()
        self.cond_emb = nn.Linear(dim, dim)
        self.traj_emb = nn.Linear(3, dim)                    # unused by forward, in the checkpoint
        self.drop = nn.Dropout(dropout)
        self.blocks = nn.Sequential(*[_Block(2 * dim, block_size, dropout) for _ in range(layers)])
        self.pos_embed = _PositionalEncoding(dim, dropout)
        for m in self.modules():                             # the reference's initialisation of this sub-tree
            if isinstance(m, nn.Linear):
                m.weight.data.normal_(mean=0.0, std=0.02)
                m.bias.data.zero_()


class TrajDecoder(nn.Module):
    """Drop-in for `TrajDecoder.model.traj_model.TrajDecoder`: the same constructor, the same 133 state_dict entries (shapes and
    order, incl. `lstm.*_l{0,1,2}`, the `attn.mask` buffers, `trans_extractor.pos_embed.pe`, `trans_extractor.traj_emb.*`), and
    `forward(x (b, dn, seq, 2), music_feat (b, n, 438)) -> (b, dn, seq, 2)` on a HIP device.  Note the LSTM recurrence over the
    clip axis (module docstring): results depend on which clips share a batch, exactly as in the reference.  Inference only."""

    def __init__(self, nfeats, trans_layer=4, window_size=60, latent_dim: int = 64, dropout: float = 0.1, n_head: int = 4,
                 cond_feature_dim: int = 438):
        super().__init__()
        if nfeats != 2 or latent_dim != 64 or n_head != 4 or cond_feature_dim != 438:
            raise L.TcdiffError("TrajDecoder: the kernels are built for nfeats=2, latent_dim=64, n_head=4, cond_feature_dim=438 "
                                f"(got {nfeats}, {latent_dim}, {n_head}, {cond_feature_dim})")
        if trans_layer < 1:
            raise L.TcdiffError("TrajDecoder: trans_layer must be at least 1")
        self.latent_dim, self.window_size, self.trans_layer = latent_dim, window_size, trans_layer
        self.lstm = nn.LSTM(input_size=nfeats, hidden_size=latent_dim, num_layers=3)
        self.music_projection = nn.Sequential(nn.Linear(cond_feature_dim * 2, cond_feature_dim), nn.LeakyReLU(),
                                              nn.Linear(cond_feature_dim, cond_feature_dim), nn.LeakyReLU(),
                                              nn.Linear(cond_feature_dim, latent_dim))
        self.trans_extractor = _Extractor(latent_dim, window_size, trans_layer, dropout)
        self.Decoder = nn.Sequential(nn.Linear(latent_dim * 3, latent_dim * 2), nn.LeakyReLU(),
                                     nn.Linear(latent_dim * 2, latent_dim * 2), nn.LeakyReLU(),
                                     nn.Linear(latent_dim * 2, latent_dim), nn.LeakyReLU(), nn.Linear(latent_dim, nfeats))
        self.__dict__["_packed"] = None
        self.__dict__["_plans"] = {}
        super().train(False)

    def train(self, mode: bool = True):
        if mode:
            raise L.TcdiffError("TrajDecoder stays in eval mode: the training step of TrajDecoder/train_traj.py runs through "
                                "navigator.TrajTrainer(net), not net.train()")
        return super().train(False)

    # ---- weights ------------------------------------------------------------------------------------------------------------------
    def _weights_version(self):
        ts = list(self.parameters()) + [self.trans_extractor.pos_embed.pe]
        return tuple(t._version for t in ts) + (tuple(map(id, ts)), str(ts[0].device))

    def _weights(self):
        """The packed device weights, rebuilt whenever a parameter changed in place or was replaced (as engine.py does)."""
        ver = self._weights_version()
        pk = self.__dict__["_packed"]
        if pk is not None and pk["version"] == ver:
            return pk
        f = lambda t: t.detach().to(torch.float32)
        dev = self.lstm.weight_ih_l0.device
        with torch.no_grad():
            lw = torch.zeros(3, 128, 256, device=dev)
            for l in range(3):
                wi = f(getattr(self.lstm, f"weight_ih_l{l}"))
                lw[l, :wi.shape[1]] = wi.t()
                lw[l, 64:] = f(getattr(self.lstm, f"weight_hh_l{l}")).t()
            bih = torch.stack([f(getattr(self.lstm, f"bias_ih_l{l}")) for l in range(3)]).contiguous()
            bhh = torch.stack([f(getattr(self.lstm, f"bias_hh_l{l}")) for l in range(3)]).contiguous()
            parts = []
            for blk in self.trans_extractor.blocks:
                a = blk.attn
                for t in (blk.ln1.weight, blk.ln1.bias, a.query.weight, a.query.bias, a.key.weight, a.key.bias, a.value.weight,
                          a.value.bias, a.proj.weight, a.proj.bias, blk.ln2.weight, blk.ln2.bias, blk.mlp[0].weight, blk.mlp[0].bias,
                          blk.mlp[2].weight, blk.mlp[2].bias):
                    parts.append(f(t).reshape(-1))
            blocks = torch.cat(parts).contiguous()
            d = self.Decoder
            w4, b4 = torch.zeros(16, 64, device=dev), torch.zeros(16, device=dev)
            w4[:2], b4[:2] = f(d[6].weight), f(d[6].bias)
            dec = torch.cat([f(t).reshape(-1) for t in (d[0].weight, d[0].bias, d[2].weight, d[2].bias, d[4].weight, d[4].bias)] +
                            [w4.reshape(-1), b4]).contiguous()
            m = self.music_projection
            w1, b1 = torch.zeros(448, 880, device=dev), torch.zeros(448, device=dev)
            w2, b2 = torch.zeros(448, 448, device=dev), torch.zeros(448, device=dev)
            w3 = torch.zeros(64, 448, device=dev)
            w1[:438, :876], b1[:438] = f(m[0].weight), f(m[0].bias)
            w2[:438, :438], b2[:438] = f(m[2].weight), f(m[2].bias)
            w3[:, :438] = f(m[4].weight)
            ce = self.trans_extractor.cond_emb
            mus = torch.cat([t.reshape(-1) for t in (w1, b1, w2, b2, w3, f(m[4].bias), f(ce.weight), f(ce.bias))]).contiguous()
            pe = f(self.trans_extractor.pos_embed.pe).reshape(MAX_POS, 64).contiguous()
        assert blocks.numel() == self.trans_layer * _BK and dec.numel() == _DC and mus.numel() == _MU
        pk = dict(version=ver, lstm_w=lw, bih=bih, bhh=bhh, blocks=blocks, dec=dec, music=mus, pe=pe)
        self.__dict__["_packed"] = pk
        return pk

    def _image_slots(self):
        """Where `_weights()` puts every parameter: [(parameter, image, offset, row, sr, sc)] -- element e of the parameter is element
        offset + (e // row) * sr + (e % row) * sc of the image (tcdiff_nav_adamw_chunk, include/tcdiff_hip.h).  `TrajAdamW` writes
        through this map; tests/test_navigator_step_cpu.py holds it against `_weights()` itself."""
        out = []
        flat = lambda t, image, off: out.append((t, image, off, t.numel(), 0, 1))
        for l in range(3):
            wi, wh = getattr(self.lstm, f"weight_ih_l{l}"), getattr(self.lstm, f"weight_hh_l{l}")
            out.append((wi, "lstm_w", l * 128 * 256, wi.shape[1], 1, 256))                 # [256][in] -> rows 0 .. in - 1, transposed
            out.append((wh, "lstm_w", (l * 128 + 64) * 256, 64, 1, 256))                   # [256][64] -> rows 64 .. 127
            flat(getattr(self.lstm, f"bias_ih_l{l}"), "bih", l * 256)
            flat(getattr(self.lstm, f"bias_hh_l{l}"), "bhh", l * 256)
        off = 0
        for blk in self.trans_extractor.blocks:
            a = blk.attn
            for t in (blk.ln1.weight, blk.ln1.bias, a.query.weight, a.query.bias, a.key.weight, a.key.bias, a.value.weight,
                      a.value.bias, a.proj.weight, a.proj.bias, blk.ln2.weight, blk.ln2.bias, blk.mlp[0].weight, blk.mlp[0].bias,
                      blk.mlp[2].weight, blk.mlp[2].bias):
                flat(t, "blocks", off)
                off += t.numel()
        d, off = self.Decoder, 0
        for t in (d[0].weight, d[0].bias, d[2].weight, d[2].bias, d[4].weight, d[4].bias):
            flat(t, "dec", off)
            off += t.numel()
        flat(d[6].weight, "dec", off)                                                      # 2 of 16 rows
        flat(d[6].bias, "dec", off + 16 * 64)
        m, ce, off = self.music_projection, self.trans_extractor.cond_emb, 0
        for t, rows, ld in ((m[0].weight, 448, 880), (m[0].bias, 1, 448), (m[2].weight, 448, 448), (m[2].bias, 1, 448),
                            (m[4].weight, 64, 448), (m[4].bias, 1, 64), (ce.weight, 64, 64), (ce.bias, 1, 64)):
            out.append((t, "music", off, t.shape[-1], ld, 1))
            off += rows * ld
        assert off == _MU
        return out

    # ---- workspaces ---------------------------------------------------------------------------------------------------------------
    def _plan(self, dev, b, dn, seq, pairs, roll_frames, taps):
        key = (str(dev), b, dn, seq, pairs, roll_frames, bool(taps))
        pl = self.__dict__["_plans"].get(key)
        if pl is None:
            T = dn * seq
            Tp = K.round_up(T, 16)
            z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
            pl = dict(traj=z(b, T, 2), lstm_out=z(b, T, 64), x=z(b, T, 128), q=z(2, b, Tp, 128), k=z(2, b, 4, Tp, 32),
                      vt=z(2, b, 4, 32, Tp), mp=z(b, pairs, 64), me=z(b, pairs, 64),
                      roll=z(b, dn, roll_frames, 2) if roll_frames else None,
                      tap_lstm=z(b, T, 64) if taps else None, tap_blocks=z(self.trans_layer, b, T, 128) if taps else None)
            if len(self.__dict__["_plans"]) >= 4:
                self.__dict__["_plans"].clear()
            self.__dict__["_plans"][key] = pl
        return pl

    def _check(self, x, music):
        if self.training:
            raise L.TcdiffError("TrajDecoder stays in eval mode: the training step of TrajDecoder/train_traj.py runs through "
                                "navigator.TrajTrainer(net), not net.train()")
        if torch.is_grad_enabled() and (x.requires_grad or music.requires_grad):
            raise L.TcdiffError("TrajDecoder: inputs get no gradient (TrajDecoder/train_traj.py never asks for one); the parameters' "
                                "gradients come from navigator.TrajTrainer(net)")
        dev = self.lstm.weight_ih_l0.device
        if dev.type != "cuda" or x.device != dev or music.device != dev:
            raise L.TcdiffError("TrajDecoder runs on MI355X only: move the module and its inputs to cuda (no CPU fallback)")
        if x.dim() != 4 or x.shape[-1] != 2:
            raise L.TcdiffError(f"TrajDecoder: x must be (b, dn, seq, 2), got {tuple(x.shape)}")
        if music.dim() != 3 or music.shape[-1] != 438 or music.shape[0] != x.shape[0]:
            raise L.TcdiffError(f"TrajDecoder: music_feat must be ({x.shape[0]}, n, 438), got {tuple(music.shape)}")
        if x.shape[1] * x.shape[2] > MAX_POS:
            raise L.TcdiffError(f"TrajDecoder: dn * seq = {x.shape[1] * x.shape[2]} positions exceed PositionalEncoding's max_len "
                                f"{MAX_POS} (the reference raises here too)")
        if min(x.shape) < 1:
            raise L.TcdiffError(f"TrajDecoder: empty input {tuple(x.shape)}")
        return dev

    def _launch(self, pl, wt, cond, b, dn, seq, pairs, n_windows, me_off, mp_off, stride, step, roll_off):
        lib, st = L.load(), K.stream()
        L.check(lib.tcdiff_nav_music_front(K._p(cond), b, cond.shape[1], K._p(wt["music"]), K._p(pl["mp"]), K._p(pl["me"]), st),
                "tcdiff_nav_music_front")
        roll = pl["roll"]
        a = L.NavArgs(b=b, dn=dn, seq=seq, n_layers=self.trans_layer, pairs=pairs, me_off=me_off, mp_off=mp_off, win_stride=stride,
                      step=step, roll_frames=0 if roll is None else roll.shape[2], roll_off=roll_off, lstm_w=K._p(wt["lstm_w"]),
                      lstm_bih=K._p(wt["bih"]), lstm_bhh=K._p(wt["bhh"]), pe=K._p(wt["pe"]), blocks=K._p(wt["blocks"]),
                      dec=K._p(wt["dec"]), me=K._p(pl["me"]), mp=K._p(pl["mp"]), traj=K._p(pl["traj"]),
                      lstm_out=K._p(pl["lstm_out"]), x=K._p(pl["x"]), q=K._p(pl["q"]), k=K._p(pl["k"]), vt=K._p(pl["vt"]),
                      roll=K._p(roll), tap_lstm=K._p(pl["tap_lstm"]), tap_blocks=K._p(pl["tap_blocks"]))
        L.check(lib.tcdiff_nav_rollout(C.byref(a), n_windows, st), "tcdiff_nav_rollout")

    @staticmethod
    def _fill_taps(taps, pl, b, pairs):
        taps["lstm"] = pl["tap_lstm"].clone()
        taps["music"] = pl["mp"].clone()
        taps["cond_emb"] = pl["me"].clone()
        taps["blocks"] = pl["tap_blocks"].clone()

    def forward(self, x, music_feat, taps=None):
        """One window: `taps` (a dict, tests) receives the LSTM output, the projected music rows and every block's output."""
        dev = self._check(x, music_feat)
        b, dn, seq, _ = x.shape
        pairs = music_feat.shape[1] // 2
        if pairs < seq:
            raise L.TcdiffError(f"TrajDecoder: {music_feat.shape[1]} music frames give {pairs} pairs, fewer than seq = {seq}")
        wt = self._weights()
        pl = self._plan(dev, b, dn, seq, pairs, 0, taps is not None)
        cond = music_feat.detach().to(torch.float32).contiguous()
        pl["traj"].copy_(x.detach().reshape(b, dn * seq, 2))
        self._launch(pl, wt, cond, b, dn, seq, pairs, 1, 0, pairs - seq, 0, 0, 0)
        if taps is not None:
            self._fill_taps(taps, pl, b, pairs)
        return pl["traj"].reshape(b, dn, seq, 2).clone()


def window_starts(cond_len: int, window: int, step: int):
    """The music-frame offsets of the rollout's windows (TCDiff.py:540)."""
    return range(0, cond_len + 1 - (window + step) * 2, step * 2)


def _rollout_check(model, x_traj_xy, cond, step):
    """`rollout`'s argument checks: the first window (a view), the device and the number of windows."""
    window = model.window_size
    if step < 1 or step > window:
        raise L.TcdiffError(f"rollout: step must be in 1 .. window_size = {window}, got {step}")
    if x_traj_xy.dim() != 4 or x_traj_xy.shape[2] < window:
        raise L.TcdiffError(f"rollout: x_traj_xy must be (b, dn, >= {window} frames, 2), got {tuple(x_traj_xy.shape)}")
    first = x_traj_xy[:, :, :window]
    dev = model._check(first, cond)
    return first, dev, len(window_starts(cond.shape[1], window, step))


def _rollout_launch(model, first, dev, cond, step, n_windows, taps):
    """`rollout`'s launches for n_windows >= 1.  Returns the plan: its "roll" buffer holds the trajectories until the next rollout
    of this shape.  Every torch op (the copies into the plan) comes before the first launch."""
    window = model.window_size
    b, dn = first.shape[:2]
    pairs = cond.shape[1] // 2
    wt = model._weights()
    pl = model._plan(dev, b, dn, window, pairs, window + n_windows * step, taps is not None)
    condc = cond.detach().to(torch.float32).contiguous()
    pl["traj"].copy_(first.detach().reshape(b, dn * window, 2))
    pl["roll"][:, :, :window].copy_(first.detach())
    model._launch(pl, wt, condc, b, dn, window, pairs, n_windows, 0, step, step, step, window)
    return pl


def rollout(model: TrajDecoder, x_traj_xy, cond, step: int = 25, taps=None):
    """TCDiff.py:526-547: `x_traj_xy` (b, dn, frames >= window, 2) gives the first window; every window of (window + step) * 2
    music frames, moved by step * 2, predicts the next window from the previous one and contributes its last `step` frames.
    Returns (b, dn, window + n_windows * step, 2) on the device; a `cond` too short for one window returns the initial window (the
    reference's empty range).  The music front runs once for the whole `cond`; between the first and the last launch there is no
    torch op, no allocation and no host synchronisation."""
    first, dev, n_windows = _rollout_check(model, x_traj_xy, cond, step)
    if n_windows == 0:
        return first.detach().to(torch.float32).clone()
    pl = _rollout_launch(model, first, dev, cond, step, n_windows, taps)
    if taps is not None:
        model._fill_taps(taps, pl, first.shape[0], cond.shape[1] // 2)
    return pl["roll"].clone()


# ---- the hand-off to the sampler (TCDiff.py:543-556, TrajDecoder/train_traj.py:245-259) ---------------------------------------------
_GAINS = {}                        # (device, frames, dt, q, r) -> the filter's gains K_t on the device, float64 (frames, 4, 2)


def _gains(dev, frames, dt, q, r):
    """io.kalman_gains on the device: computed on the host and copied once per key, read by every later launch."""
    key = (str(dev), frames, float(dt), float(q), float(r))
    g = _GAINS.get(key)
    if g is None:
        if len(_GAINS) >= 8:
            del _GAINS[next(iter(_GAINS))]                 # the oldest key only: the other tables stay on the device
        g = _GAINS[key] = torch.from_numpy(tio.kalman_gains(frames, *key[2:])).to(dev)
    return g


def _handoff_prepare(shape, dev, dt, q, r, normalizer, out, return_smoothed):
    """Everything the hand-off launch needs besides its input -- the gains, the outputs, the normalizer's six numbers -- so that
    `rollout_x0` can have it ready before the rollout's first launch."""
    b, dn, frames, _ = shape
    L.load()
    gains = _gains(dev, frames, dt, q, r)
    if out is None:
        out = torch.empty(b, frames * dn, 3, device=dev, dtype=torch.float32)
    elif not torch.is_tensor(out) or tuple(out.shape) != (b, frames * dn, 3) or out.dtype != torch.float32 or out.device != dev \
            or not out.is_contiguous():
        raise L.TcdiffError(f"smooth_x0: out must be a contiguous float32 ({b}, {frames * dn}, 3) tensor on {dev}")
    sm = torch.empty(b, dn, frames, 2, device=dev, dtype=torch.float32) if return_smoothed else None
    norm = (None, None)
    if normalizer is not None:
        scale = normalizer.scaler.scale_.detach().to("cpu", torch.float32).reshape(-1).tolist()
        min_ = normalizer.scaler.min_.detach().to("cpu", torch.float32).reshape(-1).tolist()
        if len(scale) != 3 or len(min_) != 3:
            raise L.TcdiffError(f"smooth_x0: the normalizer must be fitted on 3 columns (x, y, z), got {len(scale)}")
        norm = ((C.c_float * 3)(*scale), (C.c_float * 3)(*min_))
    return gains, out, sm, norm


def _handoff_launch(src, dt, gains, norm, sm, out):
    b, dn, frames, _ = src.shape
    s_b, s_dn, s_f, s_c = src.stride()
    lo = src.data_ptr()
    hi = lo + 4 * (1 + (b - 1) * s_b + (dn - 1) * s_dn + (frames - 1) * s_f + s_c)
    if out.data_ptr() < hi and lo < out.data_ptr() + 4 * out.numel():
        raise L.TcdiffError("smooth_x0: out overlaps the trajectories it is computed from")
    L.check(L.load().tcdiff_nav_handoff(K._p(src), s_b, s_dn, s_f, s_c, b, dn, frames, float(dt), K._p(gains), norm[0], norm[1],
                                        K._p(sm), K._p(out), K.stream()), "tcdiff_nav_handoff")
    return out if sm is None else (out, sm)


def _check_traj(x_traj, what):
    if not torch.is_tensor(x_traj) or x_traj.dim() != 4 or x_traj.shape[-1] != 2 or min(x_traj.shape) < 1:
        raise L.TcdiffError(f"{what}: x_traj must be a (b, dn, frames, 2) tensor, got "
                            f"{tuple(x_traj.shape) if torch.is_tensor(x_traj) else type(x_traj).__name__}")
    if x_traj.dtype != torch.float32:
        raise L.TcdiffError(f"{what}: float32 trajectories only, got {x_traj.dtype}")
    if x_traj.device.type != "cuda":
        raise L.TcdiffError(f"{what} runs on MI355X only: move the trajectories to cuda (the CPU form is io.x0_from_navigator)")


def smooth_x0(x_traj, *, dt=1.0, process_noise_std=1e-2, measurement_noise_std=1e-1, normalizer=None, out=None,
              return_smoothed=False):
    """`io.x0_from_navigator` on the device, one launch (csrc/handoff.hip): `x_traj` (b, dn, frames, 2) float32 with ANY strides
    (read in place) -> the forward Kalman filter of `io.kalman_smooth_batch` per (clip, dancer), the state in float64 and the
    result rounded once to float32 -> `x_0` (b, frames * dn, 3), token frame * dn + dancer, channels (x, y, 0): what
    `ddim_sample(x_0=)` / `render_sample(x_0=)` take.  `out=` receives it (every element is written).  `return_smoothed=True`
    returns (x_0, smoothed (b, dn, frames, 2)).  `normalizer=` (an `io.Normalizer` fitted on xyz triples) un-normalises all three
    channels of both outputs -- the evaluation block of TrajDecoder/train_traj.py:245-259.

    The gains come from `io.kalman_gains`, cached on the device per (frames, dt, process_noise_std, measurement_noise_std): from
    the second call with the same key on there is no host-to-device copy, no allocation besides the outputs and no host
    synchronisation.  A normalizer's six numbers are read on the host and travel as kernel arguments: keep its `scale_` / `min_`
    host tensors (as `io.Normalizer` and the dataset make them); device-resident ones cost a copy to the host, and with it a
    host synchronisation, per call.  `out` must not overlap `x_traj`."""
    _check_traj(x_traj, "smooth_x0")
    src = x_traj.detach()
    gains, out, sm, norm = _handoff_prepare(src.shape, src.device, dt, process_noise_std, measurement_noise_std, normalizer, out,
                                            return_smoothed)
    return _handoff_launch(src, dt, gains, norm, sm, out)


def rollout_x0(model: TrajDecoder, x_traj_xy, cond, step: int = 25, *, dt=1.0, process_noise_std=1e-2, measurement_noise_std=1e-1,
               normalizer=None, out=None, return_smoothed=False):
    """`smooth_x0(rollout(model, x_traj_xy, cond, step))` without the copy in between: the hand-off launch follows the rollout's
    on the same stream and reads the rollout's buffer.  The gains and the outputs are made ready first, so between the rollout's
    first launch and the hand-off's there is no clone, no torch op and no host synchronisation.  A `cond` too short for one window
    smooths the initial window (the reference's empty range).  Keywords as `smooth_x0`."""
    first, dev, n_windows = _rollout_check(model, x_traj_xy, cond, step)
    b, dn = first.shape[:2]
    frames = model.window_size + n_windows * step
    gains, out, sm, norm = _handoff_prepare((b, dn, frames, 2), dev, dt, process_noise_std, measurement_noise_std, normalizer, out,
                                            return_smoothed)
    if n_windows == 0:
        src = first.detach().to(torch.float32)
    else:
        src = _rollout_launch(model, first, dev, cond, step, n_windows, None)["roll"]
    return _handoff_launch(src, dt, gains, norm, sm, out)


# ---- training (TrajDecoder/train_traj.py) ------------------------------------------------------------------------------------------
SITE_POS = 256                      # TC_SITE_NAV_POS: pos_embed.dropout on (b, T, 64)


def site_block(i: int, k: int) -> int:
    """TC_SITE_NAV_BLOCK: block i, k = 0 attn_drop on (b, 4, T, T), 1 resid_drop on (b, T, 128), 2 mlp[3] on (b, T, 128)"""
    return 260 + 4 * i + k


_G_MUSIC = 438 * 876 + 438 + 438 * 438 + 438 + 64 * 438 + 64 + 64 * 64 + 64
_G_LSTM = 256 * (2 + 64 + 2) + 2 * 256 * (64 + 64 + 2)


class _TrajTrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, trainer, x, music, seed, *params):
        ctx.trainer, ctx.n = trainer, len(params)
        out = trainer._forward(x, music, seed)
        ctx.gen = trainer._gen
        return out

    @staticmethod
    def backward(ctx, d_out):
        ctx.trainer._backward(d_out, ctx.gen)
        return (None,) * (4 + ctx.n)


class TrajTrainer:
    """The training step of TrajDecoder/train_traj.py:179-201 for a `TrajDecoder`, which itself stays in eval mode:

        trainer = TrajTrainer(net, dropout=0.1)
        pre_traj = trainer(x_cond, cond[:, m0:m1])          # train-mode forward, ONE autograd node
        loss = ...; optimizer.zero_grad(); loss.backward(); optimizer.step()

    `trainer(x, music, seed=None)` is traj_model.py:170-200 in train mode -- the four live dropout sites (pos_embed, and per
    block attn_drop, resid_drop, mlp[3]) with counter-hash masks keyed by (seed, site, flat index of the reference's tensor); a
    `seed` of None draws two words from torch's generator.  Its backward is the HIP reverse pass: it assigns `.grad` of every
    parameter the forward uses (or adds to a `.grad` that is there); `trans_extractor.traj_emb.*` keep None and inputs get no
    gradient.  fp32, the inference path's shape limits, one forward outstanding per trainer.

    Allocation: workspaces are planned per shape and the seed travels as two kernel-argument words, so a step with the usual
    `optimizer.zero_grad()` (set_to_none=True) allocates one tensor between its first and last launch -- the (b, dn, seq, 2)
    prediction handed to autograd, which the caller owns.  With `zero_grad(set_to_none=False)`, or when gradients are accumulated
    over several backwards, every `.grad` still is a view of the gradient buffer, which must not be overwritten: the backward then
    takes a fresh buffer each time."""

    def __init__(self, net: TrajDecoder, dropout: float = 0.1):
        if not isinstance(net, TrajDecoder):
            raise L.TcdiffError("TrajTrainer trains a tcdiff_amd.TrajDecoder")
        if not 0.0 <= float(dropout) < 1.0:
            raise L.TcdiffError(f"TrajTrainer: dropout must be in [0, 1), got {dropout}")
        self.net, self.dropout = net, float(dropout)
        self._plans, self._gen, self._pending, self._flat, self._views = {}, 0, None, None, None

    # ---- the parameters that receive a gradient, with their place in the flat gradient buffer ----------------------------------
    def _slots(self):
        n, out, off = self.net, [], 0
        for blk in n.trans_extractor.blocks:
            a = blk.attn
            for t in (blk.ln1.weight, blk.ln1.bias, a.query.weight, a.query.bias, a.key.weight, a.key.bias, a.value.weight,
                      a.value.bias, a.proj.weight, a.proj.bias, blk.ln2.weight, blk.ln2.bias, blk.mlp[0].weight, blk.mlp[0].bias,
                      blk.mlp[2].weight, blk.mlp[2].bias):
                out.append((t, off))
                off += t.numel()
        assert off == n.trans_layer * _BK
        d = n.Decoder
        for t in (d[0].weight, d[0].bias, d[2].weight, d[2].bias, d[4].weight, d[4].bias):
            out.append((t, off))
            off += t.numel()
        out += [(d[6].weight, off), (d[6].bias, off + 16 * 64)]             # the last linear sits in 2 of 16 padded rows
        off = n.trans_layer * _BK + _DC
        m, ce = n.music_projection, n.trans_extractor.cond_emb
        for t in (m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias, ce.weight, ce.bias):
            out.append((t, off))
            off += t.numel()
        assert off == n.trans_layer * _BK + _DC + _G_MUSIC
        for l in range(3):
            for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                t = getattr(n.lstm, f"{nm}_l{l}")
                out.append((t, off))
                off += t.numel()
        assert off == n.trans_layer * _BK + _DC + _G_MUSIC + _G_LSTM
        return out, off

    def _plan(self, dev, b, dn, seq, pairs):
        key = (str(dev), b, dn, seq, pairs)
        pl = self._plans.get(key)
        if pl is None:
            T, Ly = dn * seq, self.net.trans_layer
            Tp, R, P = K.round_up(T, 16), b * dn * seq, b * pairs
            z = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
            pl = dict(cond=z(b, 2 * pairs, 438), x_in=z(R, 2), traj=z(b, T, 2),
                      lstm_out=z(b, T, 64), x=z(16), q=z(Ly, b, Tp, 128), k=z(Ly, b, 4, Tp, 32), vt=z(Ly, b, 4, 32, Tp),
                      mp=z(b, pairs, 64), me=z(b, pairs, 64), lstm_gates=z(3, R, 256), lstm_c=z(3, R, 64), lstm_h=z(3, R, 64),
                      xs=z(Ly + 1, R, 128), xmid=z(Ly, R, 128), att_o=z(Ly, R, 128), lse=z(Ly, b, 4, Tp), hid=z(Ly, R, 512),
                      dec_z=z(R, 320), mus_z=z(P, 896), d_out=z(R, 2), gx=z(R, 128), g_dec=z(R, 336), g_mpb=z(R, 64),
                      g_m=z(R, 128), g_hid=z(R, 512), g_a=z(R, 128), g_o=z(b, Tp, 128), delta=z(b, 4, Tp), g_qkv=z(R, 384),
                      n1=z(R, 128), n2=z(R, 128), ln_part=z(b * (Tp // 16), 4, 128), g_me=z(P, 64), g_mp=z(P, 64), g_mz=z(P, 896),
                      g_gates=z(3, R, 256), partial=z(L.NAV_WG_CHUNKS, L.NAV_WG_PARTIAL))
            if len(self._plans) >= 2:
                self._plans.clear()
            self._plans[key] = pl
        return pl

    def _args(self, pl, wt, b, dn, seq, pairs, seed):
        a = L.NavArgs(b=b, dn=dn, seq=seq, n_layers=self.net.trans_layer, pairs=pairs, me_off=0, mp_off=pairs - seq, win_stride=0,
                      step=0, roll_frames=0, roll_off=0, lstm_w=K._p(wt["lstm_w"]), lstm_bih=K._p(wt["bih"]),
                      lstm_bhh=K._p(wt["bhh"]), pe=K._p(wt["pe"]), blocks=K._p(wt["blocks"]), dec=K._p(wt["dec"]),
                      me=K._p(pl["me"]), mp=K._p(pl["mp"]), traj=K._p(pl["traj"]), lstm_out=K._p(pl["lstm_out"]), x=K._p(pl["x"]),
                      q=K._p(pl["q"]), k=K._p(pl["k"]), vt=K._p(pl["vt"]), roll=None, tap_lstm=None, tap_blocks=None)
        thr, scale = K.drop_params(self.dropout)
        t = L.NavTrainArgs(seed0=seed[0] & 0xFFFFFFFF, seed1=seed[1] & 0xFFFFFFFF, drop_thr=thr, drop_scale=scale,
                           grads=K._p(self._flat))
        for name, _ in L.NavTrainArgs._fields_:
            if name in pl:
                setattr(t, name, K._p(pl[name]))
        return a, t

    def __call__(self, x, music_feat, seed=None):
        net = self.net
        dev = net._check(x, music_feat)
        if x.requires_grad or music_feat.requires_grad:
            raise L.TcdiffError("TrajTrainer: inputs get no gradient (TrajDecoder/train_traj.py never asks for one)")
        if x.dtype != torch.float32 or music_feat.dtype != torch.float32:
            raise L.TcdiffError("TrajTrainer: fp32 inputs only")
        if x.shape[2] > music_feat.shape[1] // 2:
            raise L.TcdiffError(f"TrajTrainer: {music_feat.shape[1]} music frames give {music_feat.shape[1] // 2} pairs, fewer than "
                                f"seq = {x.shape[2]}")
        if seed is None:
            seed = tuple(int(v) for v in torch.randint(0, 2 ** 31 - 1, (2,)))
        slots, _ = self._slots()
        params = [p for p, _ in slots if p.requires_grad]
        return _TrajTrainFn.apply(self, x, music_feat, (int(seed[0]), int(seed[1])), *params)

    def _forward(self, x, music, seed):
        net = self.net
        dev = x.device
        b, dn, seq, _ = x.shape
        pairs = music.shape[1] // 2
        wt = net._weights()
        pl = self._plan(dev, b, dn, seq, pairs)
        if self._flat is None or self._flat.device != dev:
            self._new_flat(dev)
        pl["cond"].copy_(music.detach()[:, :2 * pairs])
        pl["x_in"].copy_(x.detach().reshape(b * dn * seq, 2))
        pl["traj"].copy_(x.detach().reshape(b, dn * seq, 2))
        a, t = self._args(pl, wt, b, dn, seq, pairs, seed)
        L.check(L.load().tcdiff_nav_train_fwd(C.byref(a), C.byref(t), K._p(wt["music"]), K.stream()), "tcdiff_nav_train_fwd")
        self._gen += 1
        self._pending = dict(gen=self._gen, pl=pl, wt=wt, shape=(b, dn, seq, pairs), seed=seed)
        return pl["traj"].reshape(b, dn, seq, 2).clone()

    def _new_flat(self, dev):
        slots, n = self._slots()
        self._flat = torch.zeros(n, device=dev, dtype=torch.float32)
        self._views = [(p, self._flat[off:off + p.numel()].view(p.shape)) for p, off in slots]

    def _backward(self, d_out, gen):
        pd = self._pending
        if pd is None or pd["gen"] != gen:
            raise L.TcdiffError("TrajTrainer: backward without its forward (one forward may be outstanding per trainer; run forward "
                                "and backward in pairs)")
        self._pending = None
        pl, wt = pd["pl"], pd["wt"]
        b, dn, seq, pairs = pd["shape"]
        # a .grad that still is a view of the buffer (the caller accumulates instead of zero_grad): never overwrite it
        base = self._flat.untyped_storage().data_ptr()
        if any(p.grad is not None and p.grad.untyped_storage().data_ptr() == base for p, _ in self._views):
            self._new_flat(self._flat.device)
        pl["d_out"].copy_(d_out.reshape(b * dn * seq, 2))
        a, t = self._args(pl, wt, b, dn, seq, pairs, pd["seed"])
        L.check(L.load().tcdiff_nav_train_bwd(C.byref(a), C.byref(t), K._p(wt["music"]), K.stream()), "tcdiff_nav_train_bwd")
        with torch.no_grad():
            for p, v in self._views:
                if not p.requires_grad:
                    continue
                if p.grad is None:
                    p.grad = v
                else:
                    p.grad.add_(v)


# ---- the loss head (TrajDecoder/train_traj.py:183-196) -------------------------------------------------------------------------
_LOSS_WS = {}                      # (device, workgroups) -> tcdiff_nav_loss's partial sums


def _loss_ws(dev, n):
    key = (str(dev), K.nav_loss_blocks(n))
    ws = _LOSS_WS.get(key)
    if ws is None:
        if len(_LOSS_WS) >= 8:
            del _LOSS_WS[next(iter(_LOSS_WS))]
        ws = _LOSS_WS[key] = torch.empty(key[1], 3, device=dev, dtype=torch.float32)
    return ws


class _TrajLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pre, tgt):
        out = torch.empty(4, device=pre.device, dtype=torch.float32)
        K.nav_loss(pre, tgt, _loss_ws(pre.device, pre.numel()), out)
        ctx.save_for_backward(pre, tgt)
        ctx.set_materialize_grads(False)
        total, parts = out[0], out[1:]
        ctx.mark_non_differentiable(parts)
        return total, parts

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        if g_total is None or not ctx.needs_input_grad[0]:
            return None, None
        pre, tgt = ctx.saved_tensors
        if g_total.dtype != torch.float32 or g_total.device != pre.device:
            raise L.TcdiffError("traj_loss: the incoming gradient must be a float32 scalar on the loss's device")
        d_pre = torch.empty(pre.shape, device=pre.device, dtype=torch.float32)
        K.nav_loss_bwd(pre, tgt, g_total, d_pre)
        return d_pre, None


def traj_loss(pre_traj, x_target):
    """The loss of TrajDecoder/train_traj.py:183-196 on (b, dn, seq, 2) float32 device tensors:

        total, (recon, dis, v) = traj_loss(pre_traj, x_target)        # total = recon + 2 * dis + 2 * v

    `recon` is the mean squared error of the positions, `dis` that of the differences between neighbouring dancers, `v` that of the
    frame-to-frame differences: four 0-dim views of one device tensor (the shape of `GaussianDiffusion.p_losses`' result).  `total`
    carries ONE autograd node, whose backward is one launch writing the analytic gradient for `pre_traj`, scaled by the incoming
    gradient read on the device; `x_target` gets none.  Both inputs may be views (`x[:, :, recon_start:recon_end]`): they are read
    by their strides, nothing is copied.  The sums are fixed-order: the same input gives the same bits.  No host synchronisation;
    from the second call at a shape on, no allocation besides the four scalars (forward) and the gradient (backward).

    `dn == 1` or `seq == 1` raises: the reference takes a mean over zero elements there and its loss is NaN."""
    for t, what in ((pre_traj, "pre_traj"), (x_target, "x_target")):
        if not torch.is_tensor(t) or t.dim() != 4 or t.shape[-1] != 2 or min(t.shape) < 1:
            raise L.TcdiffError(f"traj_loss: {what} must be a (b, dn, seq, 2) tensor, got "
                                f"{tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if t.dtype != torch.float32:
            raise L.TcdiffError(f"traj_loss: float32 only, {what} is {t.dtype}")
    if pre_traj.shape != x_target.shape:
        raise L.TcdiffError(f"traj_loss: pre_traj {tuple(pre_traj.shape)} and x_target {tuple(x_target.shape)} differ in shape")
    if pre_traj.device.type != "cuda" or x_target.device != pre_traj.device:
        raise L.TcdiffError("traj_loss runs on MI355X only: move both tensors to one cuda device (no CPU fallback)")
    if x_target.requires_grad:
        raise L.TcdiffError("traj_loss: x_target gets no gradient (TrajDecoder/train_traj.py never asks for one)")
    if pre_traj.shape[1] < 2:
        raise L.TcdiffError("traj_loss: the dancer axis (1) has one entry: the reference's dis_loss is a mean over zero elements (NaN)")
    if pre_traj.shape[2] < 2:
        raise L.TcdiffError("traj_loss: the frame axis (2) has one entry: the reference's v_loss is a mean over zero elements (NaN)")
    total, parts = _TrajLossFn.apply(pre_traj, x_target)
    return total, (parts[0], parts[1], parts[2])


# ---- the optimizer (TrajDecoder/train_traj.py:138,201; utils/utils_model.py initial_optim) ---------------------------------------
class TrajAdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW` (`decoupled=False`: `torch.optim.Adam` with L2 weight decay) over the parameters of a `TrajTrainer`'s
    net, as ONE launch per `step()` that also keeps the net's packed weight images in step:

        optimizer = TrajAdamW(trainer)                                   # lr 2e-3, betas (0.5, 0.9), weight_decay 1e-6: option_traj.py
        scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=..., gamma=...)
        optimizer.zero_grad(); total.backward(); optimizer.step(); scheduler.step()

    One parameter group (`add_param_group` raises); `param_groups[0]` carries torch's keys and `state` torch's per-parameter `step`
    (a host float32 scalar), `exp_avg`, `exp_avg_sq`, so `state_dict()` / `load_state_dict()` interchange with `torch.optim.AdamW` /
    `Adam` and a run may move between the two.  `lr`, `betas`, `eps` and `weight_decay` are read from the group at every step.

    `step()` updates every parameter that has a `.grad` and `requires_grad` (the others get no state, as in torch); all of them
    must be contiguous float32 on the GPU with equal step counts.  The scalars are `_single_tensor_adam`'s Python doubles, rounded
    to float32 where they meet a tensor, and travel as kernel arguments.  The device table of chunks points at whatever each
    `.grad` is -- the trainer's views of its flat gradient buffer in the usual step, the caller's own tensors after accumulation
    -- and is rebuilt only when one of its pointers changed.

    The update kernel also scatters each new value into `TrajDecoder._weights()`'s images (transposed LSTM weights, zero-padded
    music matrices, the Decoder's last linear in 2 of 16 rows), so the next forward finds them current without the torch repack.
    `step()` then bumps the parameters' `_version`, as torch's optimizers do (the kernel wrote through raw pointers; autograd's
    saved-tensor check stays honest), and sets the image cache's key to the new versions.  Any other change -- an in-place edit,
    a replaced Parameter, `load_state_dict` -- still misses that key and rebuilds the images through the torch path."""

    def __init__(self, trainer, lr=2e-3, betas=(0.5, 0.9), eps=1e-8, weight_decay=1e-6, decoupled=True):
        if not isinstance(trainer, TrajTrainer):
            raise L.TcdiffError("TrajAdamW updates the net of a navigator.TrajTrainer")
        if not (lr >= 0.0 and eps >= 0.0 and weight_decay >= 0.0 and len(betas) == 2 and all(0.0 <= b < 1.0 for b in betas)):
            raise L.TcdiffError(f"TrajAdamW: invalid lr / betas / eps / weight_decay: {lr}, {betas}, {eps}, {weight_decay}")
        self.trainer, self._table, self._key = trainer, None, None
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled))
        super().__init__(list(trainer.net.parameters()), defaults)

    def add_param_group(self, param_group):
        if self.param_groups:
            raise L.TcdiffError("TrajAdamW: one parameter group only (utils_model.initial_optim's other branch names an attribute "
                                "TrajDecoder does not have)")
        super().add_param_group(param_group)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) != 1:
            raise L.TcdiffError("TrajAdamW: one parameter group only")
        group = self.param_groups[0]
        if group.get("amsgrad") or group.get("maximize") or group.get("capturable") or group.get("differentiable"):
            raise L.TcdiffError("TrajAdamW: amsgrad, maximize, capturable and differentiable are not built")
        ps = [p for p in group["params"] if p.requires_grad and p.grad is not None]
        if not ps:
            return loss
        dev = ps[0].device
        if not all(p.device == dev and dev.type == "cuda" and p.dtype == torch.float32 and p.is_contiguous()
                   and p.grad.device == dev and p.grad.dtype == torch.float32 and not p.grad.is_sparse and p.grad.is_contiguous()
                   for p in ps):
            raise L.TcdiffError("TrajAdamW.step runs on MI355X only, as one launch over contiguous float32 parameters and gradients on "
                                "one cuda device (no CPU / per-tensor fallback)")
        states = []
        for p in ps:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            states.append(st)
        steps = [float(st["step"]) for st in states]
        if any(v != steps[0] for v in steps):
            raise L.TcdiffError("TrajAdamW.step: the parameters' step counts differ (one launch carries one bias correction)")
        if not all(st[k].is_contiguous() and st[k].dtype == torch.float32 and st[k].device == dev for st in states
                   for k in ("exp_avg", "exp_avg_sq")):
            raise L.TcdiffError("TrajAdamW.step: exp_avg / exp_avg_sq must be contiguous float32 tensors on the parameters' device")
        net = self.trainer.net
        wt = net._weights()                                      # current here (or rebuilt by the torch path): the kernel keeps it so
        key = tuple(t.data_ptr() for p, st in zip(ps, states) for t in (p, p.grad, st["exp_avg"], st["exp_avg_sq"])) + \
            tuple(wt[k].data_ptr() for k in ("lstm_w", "bih", "bhh", "blocks", "dec", "music"))
        if key != self._key:
            slot = {id(t): (wt[image].data_ptr() + 4 * off, row, sr, sc) for t, image, off, row, sr, sc in net._image_slots()}
            rows = [r for p, st in zip(ps, states)
                    for r in K.nav_adamw_rows(p, p.grad, st["exp_avg"], st["exp_avg_sq"], slot.get(id(p)))]
            self._table, self._key = K.nav_adamw_table(rows, dev), key
        lr, (beta1, beta2), eps, wd = float(group["lr"]), group["betas"], group["eps"], group["weight_decay"]
        step = steps[0] + 1
        bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
        sc = L.NavAdamWScalars(decay=1 - lr * wd, wd=wd, omb1=1 - beta1, beta2=beta2, omb2=1 - beta2, neg_step=-(lr / bc1),
                               bc2_sqrt=bc2 ** 0.5, eps=eps, decoupled=int(bool(group.get("decoupled_weight_decay", True))))
        K.nav_adamw(self._table, sc)
        torch.autograd.graph.increment_version(ps)
        wt["version"] = net._weights_version()
        torch._foreach_add_([st["step"] for st in states], 1)
        return loss
