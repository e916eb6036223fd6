"""Which launch form one forward of the denoiser takes (tcdiff_amd/engine.py runs it, the sampler keys its captured graphs by it).
Pure host logic: no torch, no device, no library handle."""
from __future__ import annotations

import os
from typing import Mapping, NamedTuple, Optional

MERGE12_MAX_L = 512      # measured: profiles/r06_small_batch_split.txt


class Form(NamedTuple):
    split: bool            # the decoder layers in their small-job form: four workgroups per 16-row block (csrc/chain_split.hip)
    merge12: bool          # ... with parts 1 + 2 as one launch (part 12)
    frag_front: bool       # ... with the fragment front (small products + part 0) instead of the TC_CHAIN_FRONT launch
    fork_prologue: bool    # the sampler's step prologue in two parts, the conditioning part on a forked stream
    small_m: bool          # the input / fusion products through the launcher's small-M kernel (only together with split)
    mt: int                # 16-row units per row block of the layer launch with in-launch self-attention (0: the launcher's own)
    fused_sa: bool         # layers 1.. compute their self-attention inside the chain launch


def resolve_form(*, use_chain: bool, use_full: bool, front: bool, fuse_sa: bool, chain_nw: int, nseq: int, Lq: int, n_cu: int,
                 planned: bool, env: Optional[Mapping[str, str]] = None) -> Form:
    """The form of a forward over nseq sequences of Lq tokens on a chip of n_cu compute units.  use_chain .. chain_nw: the engine's
    switches, read once at its construction; planned: whether the engine holds the small-job workspaces; env: where the four
    per-forward switches are read -- TCDIFF_SPLIT, _SPLIT_MERGE, _SPLIT_FRONT, _FORK_PROLOGUE -- as they are at this call."""
    env = os.environ if env is None else env
    blocks = nseq * ((Lq + 15) // 16)
    fused_sa = fuse_sa and chain_nw == 8
    # small jobs: when the four workgroups of every 16-row block fit the chip at once
    split = bool(use_full and fused_sa and planned and env.get("TCDIFF_SPLIT", "1") != "0" and Lq >= 16 and 4 * blocks <= n_cu)
    # TCDIFF_SPLIT_MERGE=0 never, =1 always, default: sequences of at most MERGE12_MAX_L tokens (every member then streams the
    # sequence's K / V for all eight heads)
    merge = env.get("TCDIFF_SPLIT_MERGE", "")
    # the smallest row blocks that still give every block its own CU (a block streams the layer's weights whatever its rows)
    mt = 0 if not fused_sa else 1 if blocks <= n_cu else 2 if nseq * ((Lq + 31) // 32) <= n_cu else 4
    return Form(split=split, merge12=split and (merge == "1" or (merge != "0" and Lq <= MERGE12_MAX_L)),
                frag_front=bool(split and front and env.get("TCDIFF_SPLIT_FRONT", "1") != "0"),
                fork_prologue=bool(use_chain and front and env.get("TCDIFF_FORK_PROLOGUE", "0") == "1"),
                small_m=split, mt=mt, fused_sa=bool(fused_sa))
