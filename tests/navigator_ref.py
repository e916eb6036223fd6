"""Reference for the Dance-Beat Navigator tests: the seeded weight / input recipe, the golden cases, and a plain torch restatement
of TrajDecoder.forward and the test_loop rollout, written from the description in tcdiff_amd/navigator.py (float64 by default).

The restatement is what the GPU tests compare the kernels with; tests/test_navigator_cpu.py holds it to the real reference's
float64 run (tests/golden/navigator.npz, made by tests/golden/make_golden_navigator.py) to 1e-10."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

# (name, trans_layer, window, step, dn, b, cond_len); "forward" cases run one forward on cond_len music frames
CASES = [
    ("prod", 6, 100, 25, 3, 3, 301),        # the production shape: 2 windows
    ("long", 6, 100, 25, 3, 2, 901),        # 14 windows
    ("even", 2, 20, 5, 2, 4, 120),          # even length: 8 windows
    ("odd", 2, 20, 5, 5, 3, 121),           # odd length; dn * seq = 100 is not a multiple of 16
    ("forward_b1", 2, 20, 5, 2, 1, 61),     # one direct forward, one clip
]
STAGE_SAMPLES = 2000


def sample_idx(n: int) -> np.ndarray:
    """the elements of a flattened stage tensor that the golden file keeps"""
    return np.unique(np.linspace(0, n - 1, min(n, STAGE_SAMPLES)).astype(np.int64))


def synth_tensor(name: str, shape) -> torch.Tensor:
    """Seeded by name: LayerNorm weights 1 +- 0.1, biases +-0.1, weights uniform scaled by 1 / sqrt(fan_in)."""
    shape = tuple(shape)
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    u = torch.rand(shape, generator=g) * 2 - 1
    if (".ln1." in name or ".ln2." in name) and name.endswith("weight"):
        return 1.0 + 0.1 * u
    if "bias" in name:
        return 0.1 * u
    return u / math.sqrt(shape[-1])


def synth_state_dict(model: torch.nn.Module):
    """A state dict for `model` (the reference's TrajDecoder or tcdiff_amd's): buffers (`mask`, `pe`) keep their values."""
    buffers = {n for n, _ in model.named_buffers()}
    return {k: (v.clone() if k in buffers else synth_tensor(k, v.shape)) for k, v in model.state_dict().items()}


def synth_inputs(name: str, window: int, dn: int, b: int, cond_len: int):
    g = torch.Generator().manual_seed(zlib.crc32(("inputs." + name).encode()))
    x = 0.5 * torch.randn(b, dn, window, 2, generator=g)
    cond = torch.randn(b, cond_len, 438, generator=g)
    return x, cond


def rel_err(got, want) -> float:
    """max|got - want| / max|want| in float64"""
    got = np.asarray(got.detach().cpu().double() if torch.is_tensor(got) else got, dtype=np.float64)
    want = np.asarray(want.detach().cpu().double() if torch.is_tensor(want) else want, dtype=np.float64)
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def _lin(sd, p, x):
    return x @ sd[p + ".weight"].t() + sd[p + ".bias"]


def lstm_over_clips(sd, x):
    """x (b, N, 2): nn.LSTM without batch_first -- time is the FIRST axis, the clip index; gates in the order i, f, g, o"""
    b, N, _ = x.shape
    h = [x.new_zeros(N, 64) for _ in range(3)]
    c = [x.new_zeros(N, 64) for _ in range(3)]
    out = []
    for t in range(b):
        inp = x[t]
        for l in range(3):
            g = inp @ sd[f"lstm.weight_ih_l{l}"].t() + sd[f"lstm.bias_ih_l{l}"] + h[l] @ sd[f"lstm.weight_hh_l{l}"].t() + \
                sd[f"lstm.bias_hh_l{l}"]
            gi, gf, gg, go = g.chunk(4, dim=-1)
            c[l] = torch.sigmoid(gf) * c[l] + torch.sigmoid(gi) * torch.tanh(gg)
            h[l] = torch.sigmoid(go) * torch.tanh(c[l])
            inp = h[l]
        out.append(inp)
    return torch.stack(out)


def music_front(sd, music):
    """(b, n, 438) -> music_projection of the frame pairs (b, n // 2, 64)"""
    b, n, _ = music.shape
    m = music[:, :n // 2 * 2].reshape(b, n // 2, 876)
    m = F.leaky_relu(_lin(sd, "music_projection.0", m), 0.01)
    m = F.leaky_relu(_lin(sd, "music_projection.2", m), 0.01)
    return _lin(sd, "music_projection.4", m)


def forward(sd, x, music, n_layers, taps=None, lstm=None, projected=None):
    """TrajDecoder.forward.  sd: tensors of x's dtype / device.  lstm: an nn.LSTM to run instead of the explicit loop (timing
    baseline).  projected: music_projection's output if already computed.  taps: dict receiving the stages."""
    b, dn, seq, _ = x.shape
    xs = x.reshape(b, dn * seq, 2)
    hs = lstm(xs)[0] if lstm is not None else lstm_over_clips(sd, xs)
    mp = music_front(sd, music) if projected is None else projected
    pe = sd["trans_extractor.pos_embed.pe"]                                   # (500, 1, 64)
    if dn * seq > pe.shape[0]:
        raise RuntimeError("more positions than PositionalEncoding rows")
    tr = hs + pe.permute(1, 0, 2)[:, :dn * seq]
    ce = _lin(sd, "trans_extractor.cond_emb", mp[:, :seq]).repeat(1, dn, 1)
    h = torch.cat([ce, tr], dim=2)
    T = dn * seq
    blocks = []
    for i in range(n_layers):
        p = f"trans_extractor.blocks.{i}."
        y = F.layer_norm(h, (128,), sd[p + "ln1.weight"], sd[p + "ln1.bias"], 1e-5)
        q = _lin(sd, p + "attn.query", y).view(b, T, 4, 32).transpose(1, 2)
        k = _lin(sd, p + "attn.key", y).view(b, T, 4, 32).transpose(1, 2)
        v = _lin(sd, p + "attn.value", y).view(b, T, 4, 32).transpose(1, 2)
        att = torch.softmax((q @ k.transpose(-2, -1)) * (1.0 / math.sqrt(32)), dim=-1)          # no mask
        y = (att @ v).transpose(1, 2).reshape(b, T, 128)
        h = h + _lin(sd, p + "attn.proj", y)
        y = F.layer_norm(h, (128,), sd[p + "ln2.weight"], sd[p + "ln2.bias"], 1e-5)
        h = h + _lin(sd, p + "mlp.2", F.gelu(_lin(sd, p + "mlp.0", y)))
        blocks.append(h)
    f = torch.cat([h, mp[:, -seq:].repeat(1, dn, 1)], dim=2)
    f = F.leaky_relu(_lin(sd, "Decoder.0", f), 0.01)
    f = F.leaky_relu(_lin(sd, "Decoder.2", f), 0.01)
    f = F.leaky_relu(_lin(sd, "Decoder.4", f), 0.01)
    out = _lin(sd, "Decoder.6", f).reshape(b, dn, seq, 2)
    if taps is not None:
        taps.update(lstm=hs, music=mp, blocks=torch.stack(blocks))
    return out


def window_starts(cond_len, window, step):
    return range(0, cond_len + 1 - (window + step) * 2, step * 2)


def rollout(sd, x_traj_xy, cond, n_layers, window, step, taps=None, lstm=None, per_window=None):
    """TCDiff.py:526-547.  per_window: callable(cond_traj, music) replacing `forward` (a loop over another implementation)."""
    cur = x_traj_xy[:, :, :window]
    pieces = [cur]
    for i, start in enumerate(window_starts(cond.shape[1], window, step)):
        music = cond[:, start:start + (window + step) * 2]
        if per_window is not None:
            cur = per_window(cur, music)
        else:
            cur = forward(sd, cur, music, n_layers, taps=taps if i == 0 else None, lstm=lstm)
        pieces.append(cur[:, :, -step:])
    return torch.cat(pieces, dim=2)


def to(sd, dtype, device="cpu"):
    return {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
