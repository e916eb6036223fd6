"""The sampler's captured step graphs (tcdiff_amd/step_graphs.py): how a job's steps are cut into graphs, and the cache's visit policy
-- eager, capture, replay; sixteen graphs; clear() -- driven with fake graph objects, no device.  And three source checks: the step
body closes over nothing, the cache lives in the engine."""
import gc
import weakref

from tcdiff_amd.diffusion import GaussianDiffusion, sampler_steps
from tcdiff_amd.engine import DenoiserEngine
from tcdiff_amd.form import Form
from tcdiff_amd.step_graphs import MAX_GRAPHS, StepGraphs, StepSpec, plan_runs

FORM = Form(split=True, merge12=True, frag_front=True, fork_prologue=False, small_m=True, mt=1, fused_sa=True)
SPEC = StepSpec(mode=0, branches=2, noise=False, traj=False, clip_offset=0, B=1, kind=None, q_noise=False, mask_rows=0, cparams=False,
                couple=None, form=FORM)
# one other value of every field
OTHER = dict(mode=1, branches=1, noise=True, traj=True, clip_offset=3, B=2, kind=2, q_noise=True, mask_rows=450, cparams=True,
             couple=(150, 453), form=FORM._replace(merge12=False))


def test_plan_of_a_job_crossing_the_guidance_boundary():
    plan = plan_runs([2] * 163 + [1] * 100, 20)
    assert plan == [(s, 20) for s in range(0, 160, 20)] + [(160, 1), (161, 1), (162, 1)] + [(s, 20) for s in range(163, 263, 20)]
    assert [s for s, _ in plan] == [0, 20, 40, 60, 80, 100, 120, 140, 160, 161, 162, 163, 183, 203, 223, 243]


def test_plan_of_short_and_undivided_runs():
    assert plan_runs([2] * 50, 20) == [(0, 25), (25, 25)]
    assert plan_runs([2] * 10, 20) == [(i, 1) for i in range(10)]
    assert plan_runs([2] * 7 + [1] * 5, 1) == [(i, 1) for i in range(12)]
    assert plan_runs([], 20) == []


def test_plan_tiles_every_run_and_no_graph_spans_a_change_of_branch_count():
    for n in range(1, 300):
        for branches in ([2] * n, [2] * n + [1] * 100, [1] * 37 + [2] * n):
            plan = plan_runs(branches, 20)
            at = 0
            for start, u in plan:
                assert start == at and u >= 1 and len(set(branches[start:start + u])) == 1, (n, start, u)
                at += u
            assert at == len(branches)
        # whole graphs of the run's own step count first, then single steps
        u_run = GaussianDiffusion._steps_per_graph(n, 20)
        whole = n // u_run if n >= u_run else 0
        assert plan_runs([2] * n, 20) == [(k * u_run, u_run) for k in range(whole)] + [(i, 1) for i in range(whole * u_run, n)]


class FakeGraph:
    def __init__(self, log, key):
        self.log, self.key = log, key

    def replay(self):
        self.log.append(("replay", self.key))


def visit(cache, log, key):
    def capture(body):
        log.append(("capture", key))
        return FakeGraph(log, key)
    cache.visit(key, lambda: log.append(("eager", key)), capture)


def test_eager_then_capture_then_replay_per_key():
    cache, log = StepGraphs(), []
    for _ in range(4):
        visit(cache, log, (SPEC, 5))
    visit(cache, log, (SPEC, 1))
    visit(cache, log, (SPEC, 5))
    a, b = (SPEC, 5), (SPEC, 1)
    assert log == [("eager", a), ("capture", a), ("replay", a), ("replay", a), ("replay", a), ("eager", b), ("replay", a)]
    assert len(cache) == 2 and list(cache.graphs()) == [a]


def test_keys_that_differ_in_one_field_never_share_a_graph():
    assert set(OTHER) == set(StepSpec._fields)
    keys = [(SPEC, 5), (SPEC, 1)] + [(SPEC._replace(**{f: v}), 5) for f, v in OTHER.items()]
    assert len(set(keys)) == len(StepSpec._fields) + 2
    cache, log = StepGraphs(), []
    for k in keys:
        visit(cache, log, k)
    assert log == [("eager", k) for k in keys]              # a captured neighbour is never a hit
    for k in keys:
        visit(cache, log, k)
        visit(cache, log, k)
    graphs = cache.graphs()
    assert len(graphs) == len(keys) <= MAX_GRAPHS and all(graphs[k].key == k for k in keys)
    assert [e for e in log if e[0] == "replay"] == [("replay", k) for k in keys for _ in range(2)]


def test_sixteen_graphs_and_the_oldest_go_first_with_their_marks():
    assert MAX_GRAPHS == 16
    cache, log = StepGraphs(), []
    keys = [(SPEC._replace(clip_offset=i), 5) for i in range(20)]
    for k in keys:
        visit(cache, log, k)
        visit(cache, log, k)
    assert len(cache) == 16 and list(cache.graphs()) == keys[4:]          # 16 marks, 16 graphs
    assert all(k not in cache for k in keys[:4])
    del log[:]
    visit(cache, log, keys[0])
    assert log == [("eager", keys[0])]                                   # the evicted key's mark went with its graph
    visit(cache, log, keys[19])
    assert log[-1] == ("replay", keys[19])


def test_clear_forgets_every_key_and_mark():
    cache, log = StepGraphs(), []
    a, b = (SPEC, 5), (SPEC, 1)
    visit(cache, log, a)
    visit(cache, log, a)
    visit(cache, log, b)
    cache.clear()
    assert len(cache) == 0 and cache.graphs() == {}
    del log[:]
    visit(cache, log, a)
    visit(cache, log, b)
    visit(cache, log, a)
    assert log == [("eager", a), ("eager", b), ("capture", a), ("replay", a)]


def test_retired_graphs_are_released_at_the_next_capture_and_not_before():
    cache, log = StepGraphs(), []
    a, b = (SPEC, 5), (SPEC, 1)
    visit(cache, log, a)
    visit(cache, log, a)
    old = weakref.ref(cache.graphs()[a])
    cache.clear()
    gc.collect()
    assert old() is not None
    visit(cache, log, b)            # eager
    visit(cache, log, a)            # eager
    gc.collect()
    assert old() is not None

    alive_at_capture = []

    def capture(body):
        gc.collect()
        alive_at_capture.append(old() is not None)
        return FakeGraph(log, b)
    cache.visit(b, lambda: None, capture)
    assert alive_at_capture == [False]      # emptied just before the capture


def test_clear_and_new_keys_a_thousand_times_stay_bounded():
    cache, log = StepGraphs(), []
    for r in range(1000):
        for k in [(SPEC._replace(clip_offset=r), u) for u in (1, 5)]:
            visit(cache, log, k)
            visit(cache, log, k)
        visit(cache, log, (SPEC._replace(clip_offset=r), 7))            # a mark without a graph
        cache.clear()
        assert len(cache) == 0 and len(cache._retired) <= 2
    visit(cache, log, (SPEC, 5))
    visit(cache, log, (SPEC, 5))
    assert len(cache) == 1 and cache._retired == []


def test_the_step_body_closes_over_nothing():
    assert sampler_steps.__code__.co_freevars == ()
    assert sampler_steps.__code__.co_varnames[:4] == ("eng", "st", "spec", "u")


def test_the_cache_lives_in_the_engine():
    diff = GaussianDiffusion(None, 150, 151, None, n_timestep=10)
    assert not hasattr(diff, "_graphs") and "_graphs" not in diff.__dict__
    src = open(GaussianDiffusion.__init__.__code__.co_filename).read()
    assert "_graphs" not in src.replace("reset_graphs", "").replace("step_graphs", "")
    assert not hasattr(DenoiserEngine, "generation")
    eng = open(DenoiserEngine.__init__.__code__.co_filename).read()
    assert "generation" not in eng and "graph_warm" not in eng and "self.graphs" not in eng
