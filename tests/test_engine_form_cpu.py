"""The denoiser's launch form (tcdiff_amd/form.py resolve_form): the truth table of the rules the engine's launch code spelled out
in place before they became one value -- the expected fields are written down from those rules, not computed -- and a source check
that the environment is read nowhere else on the inference path."""
import ast
import os
import re

import pytest

from tcdiff_amd.form import MERGE12_MAX_L, Form, resolve_form

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the default engine: TCDIFF_CHAIN=2, the front launch, in-launch self-attention, 8-wave chain launches, workspaces planned
ON = dict(use_chain=True, use_full=True, front=True, fuse_sa=True, chain_nw=8, n_cu=256, planned=True)


def form(nseq, Lq, env=None, **kw):
    return resolve_form(**{**ON, **kw}, nseq=nseq, Lq=Lq, env=env or {})


def test_default_form_of_one_clip():
    """1 clip of 3 x 150, both guidance branches: 4 * 2 * 29 = 232 workgroups fit 256 CUs"""
    assert form(2, 450) == Form(split=True, merge12=True, frag_front=True, fork_prologue=False, small_m=True, mt=1, fused_sa=True)


@pytest.mark.parametrize("nseq,Lq,n_cu,split", [(2, 450, 256, True), (4, 450, 256, False), (2, 450, 231, False), (2, 450, 232, True),
                                               (1, 15, 256, False), (1, 16, 256, True), (2, 120, 256, True), (4, 74, 256, True)])
def test_split_when_four_workgroups_per_block_fit_the_chip(nseq, Lq, n_cu, split):
    f = form(nseq, Lq, n_cu=n_cu)
    assert (f.split, f.small_m, f.frag_front) == (split, split, split)


def test_split_switched_off_takes_its_dependants_with_it():
    f = form(2, 450, {"TCDIFF_SPLIT": "0", "TCDIFF_SPLIT_MERGE": "1", "TCDIFF_SPLIT_FRONT": "1"})
    assert (f.split, f.merge12, f.frag_front, f.small_m) == (False, False, False, False)
    assert f.fused_sa and f.mt == 1            # the fused launch still cuts its blocks per sequence
    assert form(2, 450, {"TCDIFF_SPLIT": "1"}).split


@pytest.mark.parametrize("value,short,long", [(None, True, False), ("", True, False), ("1", True, True), ("0", False, False)])
def test_merge12_switch(value, short, long):
    assert MERGE12_MAX_L == 512
    env = {} if value is None else {"TCDIFF_SPLIT_MERGE": value}
    # (513 tokens split on a chip of 1024 CUs only: 4 * 1 * 33 = 132 workgroups; 512 tokens: 128)
    assert form(1, 512, env, n_cu=1024).merge12 is short and form(1, 513, env, n_cu=1024).merge12 is long
    assert form(1, 513, env, n_cu=1024).split and form(2, 450, env).merge12 is short


def test_fragment_front_switch():
    f = form(2, 450, {"TCDIFF_SPLIT_FRONT": "0"})
    assert f.split and f.small_m and f.merge12 and not f.frag_front
    assert not form(2, 450, front=False).frag_front and form(2, 450, front=False).split     # TCDIFF_FRONT=0 engines have no front stream


@pytest.mark.parametrize("off", [dict(chain_nw=4), dict(fuse_sa=False), dict(use_full=False), dict(planned=False)])
def test_static_switches_that_rule_the_small_job_form_out(off):
    f = form(2, 450, {"TCDIFF_SPLIT": "1", "TCDIFF_SPLIT_MERGE": "1"}, **off)
    assert (f.split, f.merge12, f.frag_front, f.small_m) == (False, False, False, False)


def test_fused_self_attention_needs_the_eight_wave_form():
    assert form(2, 450, chain_nw=4) == Form(False, False, False, False, False, 0, False)
    assert form(2, 450, fuse_sa=False) == Form(False, False, False, False, False, 0, False)
    assert form(2, 450, planned=False) == Form(False, False, False, False, False, 1, True)


@pytest.mark.parametrize("env,kw,fork", [({}, {}, False), ({"TCDIFF_FORK_PROLOGUE": "1"}, {}, True), ({"TCDIFF_FORK_PROLOGUE": "0"}, {}, False),
                                         ({"TCDIFF_FORK_PROLOGUE": "1"}, dict(front=False), False),
                                         ({"TCDIFF_FORK_PROLOGUE": "1"}, dict(use_chain=False, use_full=False, front=False, fuse_sa=False), False),
                                         ({"TCDIFF_FORK_PROLOGUE": "1", "TCDIFF_SPLIT": "0"}, {}, True)])
def test_fork_prologue_switch(env, kw, fork):
    assert form(2, 450, env, **kw).fork_prologue is fork


@pytest.mark.parametrize("nseq,Lq,mt", [(2, 120, 1), (32, 450, 4), (8, 450, 1), (16, 450, 2), (17, 450, 2), (18, 450, 4)])
def test_block_rows_of_the_fused_launch(nseq, Lq, mt):
    """the smallest of 16 / 32 / 64-row blocks that gives every block its own CU: 29 / 15 / 8 blocks per 450-token sequence"""
    assert form(nseq, Lq).mt == mt


def _environ_lines(path):
    """(line number, name of the enclosing top-level function or Class.method, source line) of every mention of the environment"""
    src = open(path).read()
    owner = {}
    for node in ast.parse(src).body:
        inner = node.body if isinstance(node, ast.ClassDef) else [node]
        for fn in inner:
            if isinstance(fn, (ast.FunctionDef, ast.AsyncFunctionDef)):
                name = f"{node.name}.{fn.name}" if isinstance(node, ast.ClassDef) else fn.name
                owner.update({ln: name for ln in range(fn.lineno, fn.end_lineno + 1)})
    return [(i, owner.get(i), line) for i, line in enumerate(src.splitlines(), 1) if re.search(r"\benviron\b|getenv", line)]


def test_the_inference_switches_are_read_in_the_constructor_and_the_resolver_only():
    pkg = os.path.join(ROOT, "tcdiff_amd")
    eng = _environ_lines(os.path.join(pkg, "engine.py"))
    assert eng and all(fn == "DenoiserEngine.__init__" for _, fn, _ in eng), eng
    res = _environ_lines(os.path.join(pkg, "form.py"))
    assert res and all(fn == "resolve_form" for _, fn, _ in res), res
    dif = _environ_lines(os.path.join(pkg, "diffusion.py"))
    assert len(dif) == 2 and all("TCDIFF_FILM_TABLE" in line or "TCDIFF_GRAPH_STEPS" in line for _, _, line in dif), dif
