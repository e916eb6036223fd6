"""The Navigator's loss head and optimizer, off the GPU: the float64 restatement of the loss gradient against autograd through
train_traj.py's expression, the NaN that expression gives on a one-entry axis (what `traj_loss` refuses), the refusals off-GPU,
the map `TrajAdamW` scatters through against `TrajDecoder._weights()` itself, and the ctypes mirrors of the new structures."""
import ctypes
import math
import os
import shutil
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402
import navigator_step_ref as SR  # noqa: E402
from tcdiff_amd import TrajAdamW, TrajDecoder, TrajTrainer, navigator, traj_loss  # noqa: E402
from tcdiff_amd import _lib as L  # noqa: E402
from tcdiff_amd import kernels as K  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("shape", SR.LOSS_CASES + [(2, 5, 3)])
def test_restated_gradient_equals_autograd_through_the_literal_expression(shape):
    pre, tgt = (t.double() for t in SR.loss_inputs(*shape))
    _, want = SR.loss_and_grad(pre, tgt, torch.float64)
    got = SR.loss_grad(pre, tgt)
    err = float((got - want).abs().max())
    print(shape, err)
    assert err <= 1e-12
    # and the restated loss of tests/navigator_train_ref.py is the same number
    assert abs(float(SR.literal_loss(pre, tgt)[0] - SR.TR.loss_fn(pre, tgt))) <= 1e-12


@pytest.mark.parametrize("shape", [(3, 1, 5), (3, 4, 1)], ids=["dn1", "seq1"])
def test_the_literal_expression_is_nan_on_a_one_entry_axis(shape):
    pre, tgt = SR.loss_inputs(*shape)
    total, (recon, dis, v) = SR.literal_loss(pre, tgt)
    assert math.isnan(float(total)) and math.isfinite(float(recon))
    assert math.isnan(float(dis if shape[1] == 1 else v))


def test_traj_loss_and_the_fused_step_refuse_to_run_off_gpu():
    pre, tgt = SR.loss_inputs(2, 3, 5)
    with pytest.raises(L.TcdiffError, match="MI355X"):
        traj_loss(pre.requires_grad_(), tgt)
    net = TrajDecoder(nfeats=2, trans_layer=1, window_size=20)
    opt = TrajAdamW(TrajTrainer(net, dropout=0.0))
    assert opt.step() is None                                   # no gradient anywhere: nothing to do, as in torch
    for p in net.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(L.TcdiffError, match="MI355X"):
        opt.step()
    assert len(opt.state) == 0
    with pytest.raises(L.TcdiffError, match="one parameter group"):
        opt.add_param_group({"params": [torch.zeros(3, requires_grad=True)]})
    with pytest.raises(L.TcdiffError, match="TrajTrainer"):
        TrajAdamW(net)


def test_param_group_carries_torch_adamw_keys_and_defaults():
    net = TrajDecoder(nfeats=2, trans_layer=1, window_size=20)
    ours = TrajAdamW(TrajTrainer(net)).param_groups[0]
    theirs = torch.optim.AdamW(net.parameters(), lr=2e-3, betas=(0.5, 0.9), eps=1e-8, weight_decay=1e-6).param_groups[0]
    assert set(ours) == set(theirs)
    for k in theirs:
        if k != "params":
            assert ours[k] == theirs[k], k
    assert all(a is b for a, b in zip(ours["params"], theirs["params"]))
    assert TrajAdamW(TrajTrainer(net), decoupled=False).param_groups[0]["decoupled_weight_decay"] is False


@pytest.mark.parametrize("layers", [1, 3])
def test_the_scatter_map_reproduces_the_packed_images(layers):
    """Every parameter element lands where `_weights()` puts it, inside its image, no two on one place; what the map never writes
    is the zero padding."""
    net = TrajDecoder(nfeats=2, trans_layer=layers, window_size=20)
    net.load_state_dict(R.synth_state_dict(net))
    wt = net._weights()
    images = {k: torch.zeros_like(wt[k]).reshape(-1) for k in ("lstm_w", "bih", "bhh", "blocks", "dec", "music")}
    hits = {k: torch.zeros(v.numel(), dtype=torch.int32) for k, v in images.items()}
    seen = set()
    for p, image, off, row, sr, sc in net._image_slots():
        e = torch.arange(p.numel())
        idx = off + (e // row) * sr + (e % row) * sc
        assert int(idx.min()) >= 0 and int(idx.max()) < images[image].numel(), (image, off)
        images[image][idx] = p.detach().reshape(-1)
        hits[image][idx] += 1
        seen.add(id(p))
    for k, v in images.items():
        assert int(hits[k].max()) == 1
        assert torch.equal(v, wt[k].reshape(-1)), k
        assert float(wt[k].reshape(-1)[hits[k] == 0].abs().max() if bool((hits[k] == 0).any()) else 0.0) == 0.0
    left = [n for n, p in net.named_parameters() if id(p) not in seen]
    assert left == ["trans_extractor.traj_emb.weight", "trans_extractor.traj_emb.bias"]


def test_chunk_rows_cover_every_element_once():
    p, g, m, v = (torch.zeros(3, 65536 + 5) for _ in range(4))
    rows = K.nav_adamw_rows(p, g, m, v, (1 << 20, 7, 8, 1))
    assert [r[5] for r in rows] == [65536, 65536, 65536, 15] and [r[6] for r in rows] == [0, 65536, 131072, 196608]
    assert all(r[0] == p.data_ptr() + 4 * r[6] and r[1] == g.data_ptr() + 4 * r[6] and r[4] == 1 << 20 and r[7:] == (7, 8, 1)
               for r in rows)
    assert K.nav_adamw_rows(p, g, m, v)[0][4] == 0
    assert K.nav_loss_blocks(1) == 1 and K.nav_loss_blocks(2048) == 1 and K.nav_loss_blocks(2049) == 2


def test_new_structures_match_the_header(tmp_path):
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    src = ['#include <stdio.h>', '#include "tcdiff_hip.h"', "int main(void) {",
           '  printf("%zu %zu %d\\n", sizeof(tcdiff_nav_adamw_scalars), sizeof(tcdiff_nav_adamw_chunk), TC_NAV_LOSS_BLOCK);',
           "  return 0;", "}"]
    cfile, exe = tmp_path / "abi.c", tmp_path / "abi"
    cfile.write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", str(cfile),
                    "-o", str(exe)], check=True, capture_output=True)
    scal, chunk, block = (int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert ctypes.sizeof(L.NavAdamWScalars) == scal
    assert chunk == 80                                          # ten 8-byte words: kernels.nav_adamw_table's int64 [n][10]
    assert block == L.NAV_LOSS_BLOCK


def test_launchers_validate_before_any_launch():
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    s4 = (ctypes.c_long * 4)(1, 1, 1, 1)
    buf = ctypes.create_string_buffer(64)
    a = ctypes.c_void_p(ctypes.addressof(buf))
    assert lib.tcdiff_nav_loss(None, s4, a, s4, 1, 2, 2, a, a, None) == -1
    assert lib.tcdiff_nav_loss(a, s4, a, s4, 1, 1, 2, a, a, None) == -1            # dn = 1
    assert lib.tcdiff_nav_loss(a, s4, a, s4, 1, 2, 1, a, a, None) == -1            # seq = 1
    assert lib.tcdiff_nav_loss_bwd(a, s4, a, s4, 1, 2, 2, None, a, None) == -1
    assert lib.tcdiff_nav_loss_bwd(a, s4, a, s4, 0, 2, 2, a, a, None) == -1
    assert lib.tcdiff_nav_adamw(None, 1, ctypes.byref(L.NavAdamWScalars()), None) == -1
    assert lib.tcdiff_nav_adamw(a, 0, ctypes.byref(L.NavAdamWScalars()), None) == -1
    assert navigator.TrajAdamW is TrajAdamW
