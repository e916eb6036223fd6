"""One training step of the Dance-Beat Navigator at TrajDecoder/train_traj.py's shape, timed against torch.

    python tools/navigator_train_time.py            # three steps, warm, median of 20, interleaved in this process
    python tools/navigator_train_time.py one        # three fused HIP steps and nothing else (for a kernel trace of the step)
    python tools/navigator_train_time.py one-torch  # the same with torch's loss and torch.optim.AdamW around the HIP passes

A step is forward, loss, backward and AdamW at batch 128, 4 dancers, window 100, step 25, 6 blocks, p = 0.1.  The three legs: the
fused step (TrajTrainer + navigator.traj_loss + navigator.TrajAdamW: no torch kernel between the forward's first launch and the
optimizer's last), the HIP forward and backward with torch's loss and torch.optim.AdamW, and the torch baseline.  The baseline is
torch-ROCm's fp32 autograd of the restatement (tests/navigator_train_ref.py) with nn.LSTM on the same GPU.  The baseline multiplies
by ready-made boolean keep masks drawn once before the timing (about 0.5 GB resident), it does not generate them inside the step:
that favours the baseline slightly.
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import navigator_ref as R  # noqa: E402
import navigator_train_ref as TR  # noqa: E402
from tcdiff_amd import TrajAdamW, TrajDecoder, TrajTrainer, traj_loss  # noqa: E402

DEV = "cuda"
B, DN, WINDOW, STEP, LAYERS, P = 128, 4, 100, 25, 6, 0.1
FRAMES = (WINDOW + STEP) * 2
ADAMW = dict(lr=2e-3, betas=(0.5, 0.9), weight_decay=1e-6)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def make_net(sd=None):
    net = TrajDecoder(nfeats=2, trans_layer=LAYERS, window_size=WINDOW)
    sd = R.synth_state_dict(net) if sd is None else sd
    net.load_state_dict(sd)
    return net.to(DEV).eval(), sd


def main():
    net, sd = make_net()
    x, cond = R.synth_inputs("time", WINDOW, DN, B, FRAMES)
    x, cond = x.to(DEV), cond.to(DEV)
    target = TR.synth_target("time", B, DN, WINDOW).to(DEV)
    trainer = TrajTrainer(net, dropout=P)
    opt = torch.optim.AdamW(net.parameters(), **ADAMW)

    def hip_step():
        loss = TR.loss_fn(trainer(x, cond), target)
        opt.zero_grad()
        loss.backward()
        opt.step()

    fnet, _ = make_net(sd)                       # the fused leg trains its own copy: every leg does the same work per step
    ftrainer = TrajTrainer(fnet, dropout=P)
    fopt = TrajAdamW(ftrainer, **ADAMW)

    def fused_step():
        total, _ = traj_loss(ftrainer(x, cond), target)
        fopt.zero_grad()
        total.backward()
        fopt.step()

    if len(sys.argv) > 1 and sys.argv[1] in ("one", "one-torch"):
        for _ in range(3):
            (fused_step if sys.argv[1] == "one" else hip_step)()
        torch.cuda.synchronize()
        print("three fused HIP steps done" if sys.argv[1] == "one" else "three HIP steps (torch loss and AdamW) done")
        return

    leaf = {k: (v.to(DEV).clone().requires_grad_(True) if TR.is_param(k) else v.to(DEV)) for k, v in sd.items()}
    lstm = torch.nn.LSTM(2, 64, 3).to(DEV)
    lstm.load_state_dict({k[5:]: v for k, v in sd.items() if k.startswith("lstm.")})
    T = DN * WINDOW
    g = torch.Generator(device=DEV).manual_seed(1)
    keep = {TR.SITE_POS: torch.rand(B, T, 64, device=DEV, generator=g) >= P}
    for i in range(LAYERS):
        keep[TR.site_block(i, 0)] = torch.rand(B, 4, T, T, device=DEV, generator=g) >= P
        keep[TR.site_block(i, 1)] = torch.rand(B, T, 128, device=DEV, generator=g) >= P
        keep[TR.site_block(i, 2)] = torch.rand(B, T, 128, device=DEV, generator=g) >= P
    params = [v for k, v in leaf.items() if TR.is_param(k) and not k.startswith("lstm.")] + list(lstm.parameters())
    topt = torch.optim.AdamW(params, **ADAMW)

    def torch_step():
        loss = TR.loss_fn(TR.forward(leaf, x, cond, LAYERS, keep, P, lstm=lstm), target)
        topt.zero_grad()
        loss.backward()
        topt.step()

    for _ in range(3):
        fused_step()
        hip_step()
        torch_step()
    t_fused, t_hip, t_torch = [], [], []
    for _ in range(20):
        t_fused.append(timed(fused_step))
        t_hip.append(timed(hip_step))
        t_torch.append(timed(torch_step))
    mf, mh, mt = statistics.median(t_fused), statistics.median(t_hip), statistics.median(t_torch)
    print(f"shape: batch {B}, {DN} dancers, window {WINDOW}, step {STEP} ({FRAMES} music frames), {LAYERS} blocks, p = {P}")
    print(f"fused step (TrajTrainer, traj_loss, TrajAdamW)  median of 20: {mf:8.2f} ms   (min {min(t_fused):.2f}, max {max(t_fused):.2f})")
    print(f"HIP step   (TrajTrainer, torch loss and AdamW)  median of 20: {mh:8.2f} ms   (min {min(t_hip):.2f}, max {max(t_hip):.2f})")
    print(f"torch step (fp32 autograd, nn.LSTM)             median of 20: {mt:8.2f} ms   (min {min(t_torch):.2f}, max {max(t_torch):.2f})")
    print(f"fused - HIP: {mf - mh:+.2f} ms against a spread of the HIP step's samples of {max(t_hip) - min(t_hip):.2f} ms;   "
          f"torch / fused: {mt / mf:.2f}   torch / HIP: {mt / mh:.2f}")


if __name__ == "__main__":
    main()
