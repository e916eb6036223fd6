"""Dance-Beat Navigator, host side (no GPU): the float64 restatement of tests/navigator_ref.py against the real reference's float64
run (tests/golden/navigator.npz), the drop-in's state_dict surface, the exported launchers, the no-fallback rule and the rollout's
window arithmetic."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import navigator_ref as R  # noqa: E402

torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
RESTATEMENT_TOL = 1e-10        # two float64 evaluations of the same expression, relative to the output's top magnitude


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "navigator.npz"))


def _model(layers, window):
    from tcdiff_amd import TrajDecoder
    return TrajDecoder(nfeats=2, trans_layer=layers, window_size=window)


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_restatement_equals_the_reference_in_float64(gold, case):
    name, layers, window, step, dn, b, cond_len = case
    m = _model(layers, window)
    sd = R.to(R.synth_state_dict(m), torch.float64)
    x, cond = R.synth_inputs(name, window, dn, b, cond_len)
    taps = {}
    if name.startswith("forward"):
        got = R.forward(sd, x.double(), cond.double(), layers, taps=taps)
    else:
        got = R.rollout(sd, x.double(), cond.double(), layers, window, step, taps=taps)
    want = gold[f"{name}.out64"]
    assert tuple(got.shape) == want.shape
    e = R.rel_err(got, want)
    print(f"{name}: restatement vs reference float64, output: {e:.2e} (bound {RESTATEMENT_TOL:.0e})")
    assert e <= RESTATEMENT_TOL
    for st in ("lstm", "music", "blocks"):
        assert tuple(taps[st].shape) == tuple(gold[f"{name}.{st}.shape"])
        flat = taps[st].reshape(-1).numpy()
        e = float(np.max(np.abs(flat[R.sample_idx(flat.size)] - gold[f"{name}.{st}.sample64"])) / gold[f"{name}.{st}.top"])
        print(f"{name}: restatement vs reference float64, {st}: {e:.2e}")
        assert e <= RESTATEMENT_TOL
        assert abs(float(np.abs(flat).max()) - float(gold[f"{name}.{st}.top"])) <= RESTATEMENT_TOL * float(gold[f"{name}.{st}.top"])


def test_state_dict_surface_matches_the_reference(gold):
    m = _model(6, 100)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in gold["keys"]]                  # names AND order
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in gold["shapes"]]
    assert len(sd) == 133 and sum(p.numel() for p in m.parameters()) == int(gold["n_params"]) == 1932122


def test_strict_load_of_a_recipe_state_dict():
    m = _model(6, 100)
    sd = R.synth_state_dict(m)
    m.load_state_dict(sd, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in sd.items() if "traj_emb" not in k}, strict=True)


def test_library_exports_the_navigator_launchers():
    from tcdiff_amd import _lib as L
    from tcdiff_amd import build
    build.build(verbose=False)
    lib = L.load()
    assert hasattr(lib, "tcdiff_nav_music_front") and hasattr(lib, "tcdiff_nav_rollout")
    assert {"tcdiff_nav_music_front", "tcdiff_nav_rollout"} <= set(L.EXPORTS)
    a = L.NavArgs()
    assert lib.tcdiff_nav_rollout(ctypes.byref(a), 1, None) == -1            # validated before any launch
    assert lib.tcdiff_nav_music_front(None, 1, 2, None, None, None, None) == -1


def test_nav_args_mirror_matches_the_header(tmp_path):
    import shutil
    import subprocess
    from tcdiff_amd import _lib as L
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("gcc") is None or not os.path.isdir("/opt/rocm/include"):
        pytest.skip("needs gcc and the HIP headers")
    fields = [f[0] for f in L.NavArgs._fields_]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "tcdiff_hip.h"', "int main(void) {",
           '  printf("%zu\\n", sizeof(tcdiff_nav_args));']
    src += [f'  printf("%zu\\n", offsetof(tcdiff_nav_args, {f}));' for f in fields] + ["  return 0;", "}"]
    (tmp_path / "abi.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__",
                    str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")], check=True, capture_output=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout.split()]
    assert ctypes.sizeof(L.NavArgs) == out[0]
    for f, off in zip(fields, out[1:]):
        assert getattr(L.NavArgs, f).offset == off, f


def test_no_cpu_fallback_and_no_training():
    from tcdiff_amd import navigator as N
    from tcdiff_amd._lib import TcdiffError
    m = _model(2, 20)
    assert not m.training
    with pytest.raises(TcdiffError, match="cuda"):
        m(torch.zeros(1, 2, 20, 2), torch.zeros(1, 50, 438))
    with pytest.raises(TcdiffError, match="cuda"):
        N.rollout(m, torch.zeros(1, 2, 20, 2), torch.zeros(1, 120, 438), step=5)
    with pytest.raises(TcdiffError, match="train_traj"):
        m.train()
    assert m.eval() is m and not m.training
    with pytest.raises(TcdiffError, match="train_traj"):
        m(torch.zeros(1, 2, 20, 2, requires_grad=True), torch.zeros(1, 50, 438))
    for kw in (dict(nfeats=3), dict(nfeats=2, latent_dim=128), dict(nfeats=2, n_head=8)):
        with pytest.raises(TcdiffError):
            N.TrajDecoder(**kw)


def test_window_arithmetic_gives_the_golden_frame_counts(gold):
    from tcdiff_amd import navigator as N
    for name, layers, window, step, dn, b, cond_len in R.CASES:
        if name.startswith("forward"):
            continue
        starts = N.window_starts(cond_len, window, step)
        assert list(starts) == list(R.window_starts(cond_len, window, step))
        assert window + len(starts) * step == gold[f"{name}.out64"].shape[2], name
    assert [len(N.window_starts(n, 100, 25)) for n in (301, 901, 249, 250, 251, 300)] == [2, 14, 0, 1, 1, 2]
