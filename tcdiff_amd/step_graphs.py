"""The sampler's captured step graphs (tcdiff_amd/diffusion.py walks them, a DenoiserEngine owns them): what a captured step depends
on, how a job's steps are cut into graphs, and when a graph is captured, replayed and dropped.
Pure host logic: no torch, no device, no environment."""
from __future__ import annotations

from typing import Callable, Hashable, List, NamedTuple, Optional, Sequence, Tuple

from .form import Form

MAX_GRAPHS = 16


class StepSpec(NamedTuple):
    """Everything the captured step body (diffusion.sampler_steps) reads besides the engine and its sampler state, whose buffers a
    graph holds by address (DenoiserEngine.reset_graphs).  (spec, steps per graph) is the graph's key."""
    mode: int                      # TC_SAMPLER_DDPM / _DDIM
    branches: int                  # 2: unconditional | conditional stacked, 1: conditional only (guidance weight 1)
    noise: bool                    # the step's N(0,1) draw is injected (st["eps"]) instead of the in-kernel Philox stream
    traj: bool                     # trajectory channels in-painted from st["traj"]
    clip_offset: int               # global index of the job's first clip (keys the Philox stream)
    B: int                         # clips
    kind: Optional[int]            # the in-painting constraint of tcdiff_sampler_constrain, None: no constraint launch
    q_noise: bool                  # ... with its q_sample draw injected (st["qeps"])
    mask_rows: int                 # ... rows of its mask: one [L, nfeat] mask for every clip, or B * L
    cparams: bool                  # ... reading its own step table st["cparams"] instead of st["params"]
    couple: Optional[Tuple[int, int]]      # (seq_len, row_elems) of tcdiff_window_couple_step, None: no coupling launch
    form: Form                     # the launch form of the denoiser's forward


def steps_per_graph(run_len: int, unroll: int) -> int:
    """steps per captured graph for a run of `run_len` equal steps: `unroll`, or -- when that leaves a tail of single-step replays
    (50 DDIM steps = 20 + 20 + 10 x 1) -- the divisor of the run length nearest above / below it (50 -> 25)"""
    if run_len < unroll or run_len % unroll == 0:
        return unroll                       # (a run shorter than that goes step by step: a graph is captured on its SECOND visit,
                                            # and a whole-run graph would be visited once per job)
    for u in range(unroll + unroll // 2, unroll // 2, -1):
        if run_len % u == 0:
            return u
    return unroll


def plan_runs(branches_per_step: Sequence[int], unroll: int) -> List[Tuple[int, int]]:
    """[(first step, steps)] of the graphs a job replays, in order.  A run of steps with the same branch count is cut into whole graphs
    of steps_per_graph(its length, unroll) steps; what is left of it goes one step at a time (no graph per tail length)."""
    runs, i, n = [], 0, len(branches_per_step)
    while i < n:
        j = i
        while j < n and branches_per_step[j] == branches_per_step[i]:
            j += 1
        u = steps_per_graph(j - i, unroll)
        while i < j:
            if i + u > j:
                u = 1
            runs.append((i, u))
            i += u
    return runs


class StepGraphs:
    """A key's first visit runs its body eagerly (loads code objects, sets kernel attributes), the second captures it and replays the
    graph, later ones replay.  At most MAX_GRAPHS graphs, the oldest dropped first."""

    def __init__(self):
        self._entries = {}       # key -> None (visited once) | its graph; a key's warm-up mark is its presence, so they go together
        self._retired = []       # graphs of cleared keys, kept until the next capture: nothing is destroyed between two replays

    def __len__(self):
        return len(self._entries)

    def __contains__(self, key):
        return key in self._entries

    def graphs(self) -> dict:
        return {k: g for k, g in self._entries.items() if g is not None}

    def clear(self):
        """Forget every key: the buffers the graphs point at may have moved."""
        self._retired.extend(g for g in self._entries.values() if g is not None)
        self._entries = {}

    def visit(self, key: Hashable, body: Callable[[], None], capture: Callable[[Callable[[], None]], object]):
        """Run body() once, the way this visit of `key` asks for.  capture(body) returns a graph of body() with a .replay()."""
        if key not in self._entries:
            body()
            self._entries[key] = None
            return
        graph = self._entries[key]
        if graph is None:
            self._retired.clear()
            live = list(self.graphs())
            for k in live[:max(0, len(live) - (MAX_GRAPHS - 1))]:
                del self._entries[k]
            graph = capture(body)
            del self._entries[key]          # (a graph's age counts from its capture)
            self._entries[key] = graph
        graph.replay()
