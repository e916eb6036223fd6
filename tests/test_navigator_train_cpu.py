"""Training the Dance-Beat Navigator, host side (no GPU): the float64 restatement of tests/navigator_train_ref.py at p = 0 against
the real reference's float64 train-mode run (tests/golden/navigator_train.npz), and the no-fallback rule of TrajTrainer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402
import navigator_train_ref as TR  # noqa: E402

torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
TOL = 1e-10        # two float64 evaluations of the same expression, relative to the tensor's top magnitude


def test_restatement_at_p0_equals_the_reference_loss_output_and_gradients(golden_dir):
    from tcdiff_amd import TrajDecoder
    gold = np.load(os.path.join(golden_dir, "navigator_train.npz"))
    name, layers, window, dn, b, frames, _ = TR.CASES[0]
    m = TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)
    sd = R.to(R.synth_state_dict(m), torch.float64)
    x, cond = R.synth_inputs("train." + name, window, dn, b, frames)
    target = TR.synth_target(name, b, dn, window).double()
    loss, out, grads = TR.loss_and_grads(sd, x.double(), cond.double(), target, layers)
    e = abs(float(loss) - float(gold["loss"])) / abs(float(gold["loss"]))
    print(f"loss {float(loss):.12f} vs {float(gold['loss']):.12f}: {e:.2e}")
    assert e <= TOL
    assert tuple(out.shape) == tuple(gold["out.shape"])
    flat = out.reshape(-1).numpy()
    assert float(np.max(np.abs(flat[R.sample_idx(flat.size)] - gold["out.sample"]))) <= TOL * float(gold["out.top"])
    none = {str(k) for k in gold["none"]}
    assert none == {"trans_extractor.traj_emb.weight", "trans_extractor.traj_emb.bias"}
    assert {k for k, g in grads.items() if g is None} == none
    assert set(grads) == {k for k, _ in m.named_parameters()}
    # attn.key.bias has no influence (it shifts every score of a softmax row alike): its gradient is float64 rounding noise around
    # 1e-17 in both runs, so a tensor's scale is floored at 1e-6 of the largest gradient magnitude of the model
    floor = 1e-6 * max(float(gold[f"grad.{k}.top"]) for k, g in grads.items() if g is not None)
    worst = 0.0
    for k, g in grads.items():
        if g is None:
            continue
        flat = g.reshape(-1).numpy()
        top = max(float(gold[f"grad.{k}.top"]), floor)
        e = float(np.max(np.abs(flat[R.sample_idx(flat.size)] - gold[f"grad.{k}.sample"]))) / top
        worst = max(worst, e)
        assert e <= TOL, (k, e)
        assert abs(float(np.abs(flat).max()) - float(gold[f"grad.{k}.top"])) <= TOL * top, k
    print(f"worst gradient: {worst:.2e}")


def test_masked_restatement_drops_and_scales():
    """with masks the four sites change the result; all-true masks scale by 1 / (1 - p) only"""
    name, layers, window, dn, b, frames, p = TR.CASES[0]
    from tcdiff_amd import TrajDecoder
    sd = R.to(R.synth_state_dict(TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)), torch.float64)
    x, cond = R.synth_inputs("train." + name, window, dn, b, frames)
    keep = TR.masks((3, 4), p, layers, b, dn * window)
    assert set(keep) == {256, 260, 261, 262, 264, 265, 266}
    frac = float(keep[TR.site_block(0, 0)].double().mean())
    assert abs(frac - (1 - p)) < 0.01
    base = TR.forward(sd, x.double(), cond.double(), layers)
    dropped = TR.forward(sd, x.double(), cond.double(), layers, keep, p)
    again = TR.forward(sd, x.double(), cond.double(), layers, TR.masks((3, 4), p, layers, b, dn * window), p)
    assert torch.equal(dropped, again) and not torch.equal(base, dropped)


def test_trainer_has_no_cpu_fallback_and_the_module_surface_stays():
    from tcdiff_amd import TrajDecoder, TrajTrainer, navigator
    from tcdiff_amd._lib import TcdiffError
    net = TrajDecoder(nfeats=2, trans_layer=2, window_size=20)
    assert navigator.TrajTrainer is TrajTrainer
    with pytest.raises(TcdiffError, match="cuda"):
        TrajTrainer(net)(torch.zeros(1, 2, 20, 2), torch.zeros(1, 50, 438))
    with pytest.raises(TcdiffError, match="TrajTrainer"):
        net.train()
    with pytest.raises(TcdiffError, match="TrajTrainer"):
        net(torch.zeros(1, 2, 20, 2, requires_grad=True), torch.zeros(1, 50, 438))
    with pytest.raises(TcdiffError):
        TrajTrainer(net, dropout=1.0)
    with pytest.raises(TcdiffError):
        TrajTrainer(torch.nn.Linear(2, 2))
    assert not net.training
    assert (navigator.SITE_POS, navigator.site_block(1, 2)) == (TR.SITE_POS, TR.site_block(1, 2))
