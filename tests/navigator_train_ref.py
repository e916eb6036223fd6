"""Reference for the Navigator's training step: tests/navigator_ref.py::forward restated with the four train-mode dropout sites
taking explicit keep masks (traj_model.py:40,45,59 and PositionalEncoding.dropout at :106), plus the loss of
TrajDecoder/train_traj.py:183-196.  Plain differentiable torch, float64 by default.

Masks: oracle.dropout_keep(seed, site, shape, p) with tcdiff_amd.navigator's site numbers -- SITE_POS on (b, T, 64), and per block
site_block(i, 0) on the probabilities (b, 4, T, T), site_block(i, 1) on proj's output (b, T, 128), site_block(i, 2) on the MLP's
output (b, T, 128) -- each in the C order of the reference's tensor.  A kept element is scaled by float32(1 / (1 - p)), the word
the kernels multiply by."""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402

# (name, trans_layer, window, dn, b, music frames, p): the smallest shapes at which each part can still go wrong
CASES = [
    ("A", 2, 20, 2, 4, 50, 0.1),        # pairs 25: music rows 5..19 receive both contributions
    ("B", 2, 20, 5, 3, 51, 0.1),        # odd frame count; T = 100 is not a multiple of 16
    ("C", 2, 20, 2, 1, 40, 0.0),        # one clip: W_hh gradients exactly zero; pairs == seq, full overlap
    ("D", 2, 20, 2, 3, 100, 0.1),       # pairs 50 >= 2 seq: no overlap, rows 20..29 get no gradient
    ("E", 1, 100, 4, 2, 250, 0.1),      # T = 400: many key tiles, the production row count per clip
]
SITE_POS = 256


def site_block(i, k):
    return 260 + 4 * i + k


def masks(seed, p, n_layers, b, T):
    """{site: bool keep mask} for one forward, or None when p == 0"""
    if p <= 0.0:
        return None
    from oracle import tcdiff_oracle as O
    m = {SITE_POS: O.dropout_keep(seed, SITE_POS, (b, T, 64), p)}
    for i in range(n_layers):
        m[site_block(i, 0)] = O.dropout_keep(seed, site_block(i, 0), (b, 4, T, T), p)
        m[site_block(i, 1)] = O.dropout_keep(seed, site_block(i, 1), (b, T, 128), p)
        m[site_block(i, 2)] = O.dropout_keep(seed, site_block(i, 2), (b, T, 128), p)
    return m


def _drop(x, keep, p):
    if keep is None:
        return x
    return x * (keep.to(device=x.device, dtype=x.dtype) * float(np.float32(1.0 / (1.0 - p))))


def forward(sd, x, music, n_layers, keep=None, p=0.0, lstm=None):
    """TrajDecoder.forward in train mode.  keep: masks(...) or None (every site an identity).  lstm: an nn.LSTM to run instead of the
    explicit loop (timing baseline)."""
    b, dn, seq, _ = x.shape
    T = dn * seq
    k = (lambda s: None) if keep is None else (lambda s: keep[s])
    xs = x.reshape(b, T, 2)
    hs = lstm(xs)[0] if lstm is not None else R.lstm_over_clips(sd, xs)
    mp = R.music_front(sd, music)
    pe = sd["trans_extractor.pos_embed.pe"]
    tr = _drop(hs + pe.permute(1, 0, 2)[:, :T], k(SITE_POS), p)
    ce = R._lin(sd, "trans_extractor.cond_emb", mp[:, :seq]).repeat(1, dn, 1)
    h = torch.cat([ce, tr], dim=2)
    for i in range(n_layers):
        q_ = f"trans_extractor.blocks.{i}."
        y = F.layer_norm(h, (128,), sd[q_ + "ln1.weight"], sd[q_ + "ln1.bias"], 1e-5)
        q = R._lin(sd, q_ + "attn.query", y).view(b, T, 4, 32).transpose(1, 2)
        kk = R._lin(sd, q_ + "attn.key", y).view(b, T, 4, 32).transpose(1, 2)
        v = R._lin(sd, q_ + "attn.value", y).view(b, T, 4, 32).transpose(1, 2)
        att = torch.softmax((q @ kk.transpose(-2, -1)) * (1.0 / math.sqrt(32)), dim=-1)
        att = _drop(att, k(site_block(i, 0)), p)
        y = (att @ v).transpose(1, 2).reshape(b, T, 128)
        h = h + _drop(R._lin(sd, q_ + "attn.proj", y), k(site_block(i, 1)), p)
        y = F.layer_norm(h, (128,), sd[q_ + "ln2.weight"], sd[q_ + "ln2.bias"], 1e-5)
        h = h + _drop(R._lin(sd, q_ + "mlp.2", F.gelu(R._lin(sd, q_ + "mlp.0", y))), k(site_block(i, 2)), p)
    f = torch.cat([h, mp[:, -seq:].repeat(1, dn, 1)], dim=2)
    f = F.leaky_relu(R._lin(sd, "Decoder.0", f), 0.01)
    f = F.leaky_relu(R._lin(sd, "Decoder.2", f), 0.01)
    f = F.leaky_relu(R._lin(sd, "Decoder.4", f), 0.01)
    return R._lin(sd, "Decoder.6", f).reshape(b, dn, seq, 2)


def _steps(t, dim):
    """differences of neighbours along `dim`"""
    n = t.shape[dim]
    return t.narrow(dim, 1, n - 1) - t.narrow(dim, 0, n - 1)


def loss_fn(pred, target):
    """The Navigator's training loss (TrajDecoder/train_traj.py:183-196) on (b, dn, seq, 2): mean squared error of the positions,
    plus twice that of the differences between neighbouring dancers, plus twice that of the frame-to-frame velocities."""
    def mse(u, v):
        return ((u - v) ** 2).mean()
    return mse(pred, target) + 2 * mse(_steps(pred, 1), _steps(target, 1)) + 2 * mse(_steps(pred, 2), _steps(target, 2))


def synth_target(name, b, dn, window):
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(("target." + name).encode()))
    return 0.5 * torch.randn(b, dn, window, 2, generator=g)


def is_param(k):
    return not (k.endswith(".mask") or k.endswith(".pe"))


def loss_and_grads(sd, x, music, target, n_layers, keep=None, p=0.0):
    """sd: plain tensors.  Returns (loss, output, {name: grad or None}) of the restatement in sd's dtype."""
    leaf = {k: (v.clone().requires_grad_(True) if is_param(k) else v) for k, v in sd.items()}
    out = forward(leaf, x, music, n_layers, keep, p)
    loss = loss_fn(out, target)
    loss.backward()
    return loss.detach(), out.detach(), {k: v.grad for k, v in leaf.items() if is_param(k)}


GROUPS = ("lstm", "music_projection", "cond_emb", "Decoder")


def group_of(name):
    if name.startswith("trans_extractor.blocks."):
        return "block" + name.split(".")[2]
    if name.startswith("trans_extractor.cond_emb"):
        return "cond_emb"
    return name.split(".")[0]


def group_errors(got, want):
    """{group: max|got - want| / max|want|} over the parameters of each group, plus "all" for the whole flat gradient"""
    num, den = {}, {}
    for k, w in want.items():
        if w is None:
            continue
        g = got[k].detach().cpu().double()
        w = w.detach().cpu().double()
        for grp in (group_of(k), "all"):
            num[grp] = max(num.get(grp, 0.0), float((g - w).abs().max()))
            den[grp] = max(den.get(grp, 0.0), float(w.abs().max()))
    return {k: num[k] / den[k] for k in num}
