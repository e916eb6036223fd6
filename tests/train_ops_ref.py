"""The training step's row-block, weight-gradient and element-wise kernels in float64: the reference that tcdiff_row_fwd / _bwd /
_param_reduce, tcdiff_act_drop(_bwd), tcdiff_cast_transpose(_multi) (csrc/train_ops.hip) and tcdiff_gemm_splitk / _tn / _tn_grouped
(csrc/gemm.hip) are held to, region by region, by tests/test_train_ops_f64_gpu.py; pinned to torch autograd in float64 by
tests/test_train_ops_reference_cpu.py.

Everything is written as explicit formulas (``Ops``), forward and hand-derived backward, in a dtype of choice:

  * ``Ops()`` is float64 of the operand VALUES as stored.  Each output comes twice (``finish``): "model" is that value rounded once
    to the output's storage type (fp32, or bf16 by round-to-nearest-even), "f64" is unrounded;
  * ``standin(defect)`` is the same arithmetic in float32 torch on the CPU, and for the grouped weight-gradient launch the Python
    restatement of the launcher's split (``grouped_split``: per, kc, and every share walked as (problem, chunk, tile, k-range)).
    ``defect`` emulates one kernel defect (DEFECTS); the CPU module proves that each falls outside BOUNDS somewhere.

Dropout masks are oracle.tcdiff_oracle.dropout_keep: flat index m * 512 + c in the row block, row * cols + c in act_drop.  The
cases, inputs, regions and BOUNDS of the GPU module are defined here so that the CPU module runs the reference and the stand-in on
exactly them.  Not a test module: no test_* name, nothing collected here."""
import functools
import math

import numpy as np
import torch

from bf16_ref import bf, bf16_rne, region_stats, rnd, round_up  # noqa: F401  (re-exported to the test modules)
from x3_ref import rope_f32

D = torch.float64
F32 = torch.float32
SEED = (1234, 5678)
P_DROP = 0.1
ONE_ULP = 2.0 ** -7
TN_MAX_PROB = 16

BIAS, DROP_PRE, LN_POST, DROP_POST, FILM, RES, STORE_X, NEXT_LN, STORE_H, STORE_ROT = (1 << i for i in range(10))
ACT_NONE, ACT_RELU, ACT_GELU, ACT_MISH, ACT_SILU = range(5)
ACT_NAMES = {ACT_RELU: "relu", ACT_GELU: "gelu", ACT_MISH: "mish", ACT_SILU: "silu"}

DEFECTS = (
    "film_row_of_next_sequence",      # the FiLM row is taken at (m + 1) / L
    "rotary_pos_without_mod",         # position = pos_base + m although pos_mod > 0
    "ln_eps_swapped",                 # the post-LayerNorm uses nln_eps and the next one ln_eps
    "drop_post_uses_site_pre",        # the second dropout regenerates the first one's bits
    "bias_grad_before_pre_dropout",   # acc_bias taken in front of the pre-dropout's backward
    "dz_f32_ignored",                 # d_z stored as T although dz_f32 is set
    "film_grad_stored_not_added",     # d_film = sums instead of d_film += sums
    "upper_waves_not_folded",         # rows with (m - lo) % 8 >= 4 missing from the column sums
    "last_chunk_one_row_short",       # the last chunk of a sequence stops one row early
    "splitk_ranges_overlap",          # a split's k-range ends at ceil instead of floor: a k-tile twice when the k-tiles do not divide
    "share_tail_dropped",             # the last k-tile of a share that ends inside a tile is dropped
    "unit_at_problem_boundary",       # the first unit of a problem is looked up in the previous problem (and lost to its own)
    "act_bwd_scale_twice",            # the activation's backward multiplies by 1 / (1 - p) twice
    "drop_index_with_ld",             # the flat dropout index built with the leading dimension in place of cols
)

# Every flag set tcdiff_amd/train_engine.py passes to row_fwd (the backward passes the same without STORE_X): name -> (flags, where)
_BLK = DROP_PRE | LN_POST | DROP_POST | FILM | RES | STORE_X | NEXT_LN
FLAG_SETS = {
    "norm_rot":     (NEXT_LN | STORE_H | STORE_ROT, "train_engine.py:701,773,798,851 / bwd :1043,1098,1113,1184"),
    "pooled_norm":  (NEXT_LN | STORE_H, "train_engine.py:743 / bwd :1139 (L = 1, M = B)"),
    "enc_attn":     (DROP_PRE | RES | STORE_X | NEXT_LN | STORE_H, "train_engine.py:718 / bwd :1167"),
    "enc_ffn_rot":  (DROP_PRE | RES | STORE_X | NEXT_LN | STORE_H | STORE_ROT, "train_engine.py:728 / bwd :1155"),
    "enc_ffn_last": (DROP_PRE | RES | STORE_X, "train_engine.py:732 / bwd :1160"),
    "dec_self":     (_BLK | STORE_ROT, "train_engine.py:819 / bwd :1078"),
    "dec_cross":    (_BLK | STORE_H, "train_engine.py:832 / bwd :1062"),
    "dec_ffn":      (DROP_PRE | FILM | RES | NEXT_LN | STORE_H, "train_engine.py:841 / bwd :1051 (no STORE_X)"),
    "enc_bias":     (BIAS | DROP_PRE | RES | STORE_X, "kernel level only: the encoder block with the nn.Linear bias left to the row block"),
}
SHAPES = ((3, 1, 1), (2, 7, 1), (3, 50, 3), (2, 150, 8), (2, 152, 8), (2, 20, 8), (2, 5, 8))      # (nseq, L, chunks)
GRAD_SETS = {"xhr": ("d_xn", "d_h", "d_rot"), "hr": ("d_h", "d_rot"), "h": ("d_h",), "xh": ("d_xn", "d_h")}
REDUCE_BLOCKS = (1, 3, 4, 13, 16, 17, 29)
LN_EPS, NLN_EPS = 1e-6, 1e-5
SITE_PRE, SITE_POST = 17, 18
ROW_OUT_F = ("xout", "hout", "rout")
ROW_OUT_B = ("d_z", "d_xres", "d_film", "g_bias", "g_ln_g", "g_ln_b", "g_nln_g", "g_nln_b")

# the whole-tensor Frobenius limits of tests/test_train_kernels_gpu.py, which the unit-normal cases here must also meet
FROBENIUS = {
    "f32": {"xout": 2e-6, "hout": 2e-6, "rout": 2e-6, "d_z": 5e-6, "d_z32": 5e-6, "d_xres": 5e-6, "d_film": 1e-5, "g": 1e-5, "gemm": 1e-6,
            "act": 2e-6},
    "bf16": {"xout": 2e-6, "hout": 5e-3, "rout": 5e-3, "d_z": 1.5e-2, "d_z32": 5e-6, "d_xres": 5e-6, "d_film": 1e-5, "g": 1e-5,
             "gemm": 1e-5, "act": 1.5e-2},
}

# Bounds (tests/test_train_ops_f64_gpu.py): (max, mean) of |kernel - reference| / max |reference| per region, for (output, kind,
# against).  "model": the float64 value rounded once to the storage type; "f64": unrounded.  A "_lowvar" / "_offset" output is that of
# a case whose data makes eps a visible part of the LayerNorm denominators / puts the row mean at 30 deviations; "_ext": the row of
# extreme activation arguments; "act_da_f32src": the fp32 da of the (bf16 compute, fp32 source) instantiation.  Set from an MI355X run
# of this suite (profiles/train_ops_f64.txt records the run with these bounds in force; sums added with atomics move in their last
# digits from run to run) at 4x the worst value observed over the output's cases and regions (in brackets: max / mean), with the
# figures that are not measurements: the MAX of a bf16 store (hout, rout, a T-typed d_z, act_y, a bf16 act_da) against the model
# is ONE_ULP = 2^-7, and every fp32 output stays under 1e-5 against float64.  [stand-in max / mean]: 4x the float32 stand-in's
# figure where 4x the kernels' own is less than the stand-in's rounding costs on the CPU.
_BOUNDS = {      # (output, kind): (against the model, against float64)
    ("act_da", "bf16"):              ((ONE_ULP, 1.9e-06), (1.6e-02, 2.6e-03)),    # [1.58e-03 / 4.66e-07] | [3.78e-03 / 6.45e-04]
    ("act_da", "f32"):               ((2.4e-06, 2.5e-07), (2.6e-06, 2.5e-07)),    # [5.88e-07 / 6.04e-08] | [6.11e-07 / 6.06e-08]
    ("act_da_ext", "bf16"):          ((ONE_ULP, 3.3e-08), (1.3e-02, 6.1e-04)),    # [1.10e-04 / 7.83e-09] | [3.05e-03 / 1.46e-04]
    ("act_da_ext", "f32"):           ((2.4e-06, 8.8e-08), (2.6e-06, 8.8e-08)),    # [5.88e-07 / 2.19e-08] | [6.11e-07 / 2.20e-08]
    ("act_da_f32src", "bf16"):       ((2.6e-06, 2.7e-07), (2.5e-06, 2.8e-07)),    # [6.27e-07 / 6.31e-08] | [6.19e-07 / 6.55e-08]
    ("act_da_f32src_ext", "bf16"):   ((2.4e-06, 8.8e-08), (2.5e-06, 9.3e-08)),    # [5.90e-07 / 2.20e-08] | [6.13e-07 / 2.21e-08]
    ("act_y", "bf16"):               ((ONE_ULP, 7.3e-08), (1.5e-02, 2.6e-03)),    # [1.04e-04 / 1.82e-08] | [3.61e-03 / 6.42e-04]
    ("act_y", "f32"):                ((7.0e-07, 2.5e-07), (6.1e-07, 2.4e-07)),    # [1.74e-07 / 6.21e-08] | [1.46e-07 / 5.88e-08]
    ("act_y_ext", "bf16"):           ((ONE_ULP, 2.1e-09), (1.2e-03, 5.0e-05)),    # [2.44e-06 / 5.21e-10] | [2.77e-04 / 1.25e-05]
    ("act_y_ext", "f32"):            ((4.0e-08, 5.9e-09), (3.0e-08, 5.7e-09)),    # [9.54e-09 / 1.41e-09] | [7.04e-09 / 1.42e-09]
    ("colsum", "bf16"):              ((1.0e-06, 2.0e-07), (1.0e-06, 2.1e-07)),    # [2.46e-07 / 4.88e-08] | [2.41e-07 / 5.06e-08]
    ("colsum", "f32"):               ((1.0e-06, 2.1e-07), (1.0e-06, 2.2e-07)),    # [2.46e-07 / 5.20e-08] | [2.41e-07 / 5.31e-08]
    ("d_film", "bf16"):              ((6.4e-07, 9.8e-08), (5.9e-07, 1.0e-07)),    # [1.53e-07 / 2.44e-08] | [1.47e-07 / 2.49e-08]
    ("d_film", "f32"):               ((8.0e-07, 9.7e-08), (8.5e-07, 1.0e-07)),    # [1.91e-07 / 2.42e-08] | [2.03e-07 / 2.46e-08]
    ("d_film_lowvar", "bf16"):       ((5.0e-07, 9.4e-08), (5.3e-07, 9.6e-08)),    # [1.18e-07 / 2.34e-08] | [1.32e-07 / 2.40e-08]
    ("d_film_lowvar", "f32"):        ((5.0e-07, 9.4e-08), (4.9e-07, 9.6e-08)),    # [1.18e-07 / 2.23e-08] | [1.22e-07 / 2.28e-08]
    ("d_film_offset", "bf16"):       ((7.1e-07, 1.3e-07), (6.7e-07, 1.3e-07)),    # [1.68e-07 / 3.15e-08] | [1.67e-07 / 3.18e-08]
    ("d_film_offset", "f32"):        ((8.0e-07, 1.3e-07), (8.3e-07, 1.3e-07)),    # [1.99e-07 / 3.11e-08] | [2.07e-07 / 3.17e-08]
    ("d_xres", "bf16"):              ((7.5e-07, 6.0e-08), (7.1e-07, 6.6e-08)),    # [1.87e-07 / 1.50e-08] | [1.77e-07 / 1.56e-08]
    ("d_xres", "f32"):               ((6.4e-07, 6.1e-08), (7.0e-07, 6.6e-08)),    # [1.60e-07 / 1.46e-08] | [1.74e-07 / 1.58e-08]
    ("d_xres_lowvar", "bf16"):       ((4.5e-07, 4.5e-08), (5.4e-07, 5.0e-08)),    # [1.08e-07 / 1.12e-08] | [1.34e-07 / 1.18e-08]
    ("d_xres_lowvar", "f32"):        ((6.5e-07, 4.4e-08), (5.8e-07, 4.9e-08)),    # [1.62e-07 / 1.10e-08] | [1.38e-07 / 1.16e-08]
    ("d_xres_offset", "bf16"):       ((3.7e-07, 3.7e-08), (4.3e-07, 4.2e-08)),    # [8.81e-08 / 9.17e-09] | [1.03e-07 / 1.01e-08]
    ("d_xres_offset", "f32"):        ((3.7e-07, 3.4e-08), (4.1e-07, 4.1e-08)),    # [8.81e-08 / 8.46e-09] | [9.77e-08 / 9.84e-09]
    ("d_z", "bf16"):                 ((ONE_ULP, 3.6e-06), (1.4e-02, 1.5e-03)),    # [1.18e-03 / 8.54e-07] | [3.38e-03 / 3.65e-04]
    ("d_z", "f32"):                  ((9.7e-07, 5.5e-08), (1.1e-06, 5.8e-08)),    # [2.42e-07 / 1.37e-08] | [2.63e-07 / 1.45e-08]
    ("d_z32", "bf16"):               ((7.2e-07, 4.2e-08), (7.9e-07, 4.7e-08)),    # [1.79e-07 / 1.04e-08] | [1.88e-07 / 1.13e-08]
    ("d_z32", "f32"):                ((9.6e-07, 4.5e-08), (8.8e-07, 4.6e-08)),    # [2.39e-07 / 1.08e-08] | [2.19e-07 / 1.15e-08]
    ("d_z_lowvar", "bf16"):          ((ONE_ULP, 1.1e-07), (1.3e-02, 9.9e-04)),    # [1.10e-04 / 2.69e-08] | [3.19e-03 / 2.47e-04]
    ("d_z_lowvar", "f32"):           ((9.2e-07, 4.3e-08), (8.1e-07, 4.5e-08)),    # [2.30e-07 / 1.03e-08] | [2.02e-07 / 1.08e-08]
    ("d_z_offset", "bf16"):          ((ONE_ULP, 9.3e-07), (1.3e-02, 9.9e-04)),    # [1.57e-03 / 2.21e-07] | [3.13e-03 / 2.36e-04]
    ("d_z_offset", "f32"):           ((4.5e-07, 3.2e-08), (6.0e-07, 3.3e-08)),    # [1.12e-07 / 7.54e-09] | [1.50e-07 / 7.77e-09]
    ("g_bias", "bf16"):              ((1.2e-06, 1.3e-07), (1.1e-06, 1.3e-07)),    # [2.80e-07 / 3.11e-08] | [2.63e-07 / 3.13e-08]
    ("g_bias", "f32"):               ((8.7e-07, 1.3e-07), (9.1e-07, 1.3e-07)),    # [2.06e-07 / 3.08e-08] | [2.27e-07 / 3.17e-08]
    ("g_bias_lowvar", "bf16"):       ((6.4e-07, 1.1e-07), (6.6e-07, 1.1e-07)),    # [1.59e-07 / 2.69e-08] | [1.56e-07 / 2.67e-08]
    ("g_bias_lowvar", "f32"):        ((7.8e-07, 1.1e-07), (7.4e-07, 1.2e-07)),    # [1.94e-07 / 2.74e-08] | [1.84e-07 / 2.82e-08]
    ("g_bias_offset", "bf16"):       ((6.7e-07, 1.0e-07), (6.1e-07, 1.1e-07)),    # [1.67e-07 / 2.43e-08] | [1.46e-07 / 2.56e-08]
    ("g_bias_offset", "f32"):        ((5.5e-07, 9.6e-08), (5.0e-07, 9.7e-08)),    # [1.37e-07 / 2.40e-08] | [1.25e-07 / 2.42e-08]
    ("g_ln_b", "bf16"):              ((8.0e-07, 1.4e-07), (7.4e-07, 1.4e-07)),    # [1.99e-07 / 3.26e-08] | [1.84e-07 / 3.30e-08]
    ("g_ln_b", "f32"):               ((7.3e-07, 1.3e-07), (6.4e-07, 1.3e-07)),    # [1.82e-07 / 3.05e-08] | [1.60e-07 / 3.14e-08]
    ("g_ln_b_lowvar", "bf16"):       ((5.0e-07, 8.7e-08), (4.6e-07, 8.9e-08)),    # [1.25e-07 / 2.17e-08] | [1.14e-07 / 2.22e-08]
    ("g_ln_b_lowvar", "f32"):        ((6.0e-07, 8.8e-08), (6.0e-07, 9.4e-08)),    # [1.49e-07 / 2.19e-08] | [1.50e-07 / 2.23e-08]
    ("g_ln_b_offset", "bf16"):       ((5.4e-07, 9.5e-08), (5.8e-07, 1.0e-07)),    # [1.34e-07 / 2.37e-08] | [1.38e-07 / 2.43e-08]
    ("g_ln_b_offset", "f32"):        ((7.6e-07, 9.6e-08), (7.8e-07, 9.5e-08)),    # [1.89e-07 / 2.40e-08] | [1.86e-07 / 2.37e-08]
    ("g_ln_g", "bf16"):              ((9.3e-07, 1.4e-07), (9.3e-07, 1.4e-07)),    # [2.32e-07 / 3.32e-08] | [2.21e-07 / 3.38e-08]
    ("g_ln_g", "f32"):               ((9.2e-07, 1.4e-07), (8.4e-07, 1.4e-07)),    # [2.29e-07 / 3.43e-08] | [2.01e-07 / 3.47e-08]
    ("g_ln_g_lowvar", "bf16"):       ((5.8e-07, 1.1e-07), (5.1e-07, 1.1e-07)),    # [1.38e-07 / 2.65e-08] | [1.27e-07 / 2.75e-08]
    ("g_ln_g_lowvar", "f32"):        ((5.8e-07, 1.1e-07), (6.3e-07, 1.1e-07)),    # [1.38e-07 / 2.67e-08] | [1.51e-07 / 2.75e-08]
    ("g_ln_g_offset", "bf16"):       ((1.0e-06, 1.6e-07), (9.2e-07, 1.6e-07)),    # [2.43e-07 / 3.82e-08] | [2.30e-07 / 3.87e-08]
    ("g_ln_g_offset", "f32"):        ((7.3e-07, 1.5e-07), (7.2e-07, 1.5e-07)),    # [1.82e-07 / 3.52e-08] | [1.79e-07 / 3.58e-08]
    ("g_nln_b", "bf16"):             ((7.5e-07, 1.1e-07), (6.8e-07, 1.1e-07)),    # [1.87e-07 / 2.54e-08] | [1.63e-07 / 2.53e-08]
    ("g_nln_b", "f32"):              ((1.2e-06, 1.1e-07), (1.2e-06, 1.1e-07)),    # [2.81e-07 / 2.58e-08] | [2.91e-07 / 2.66e-08]
    ("g_nln_b_lowvar", "bf16"):      ((3.9e-07, 8.7e-08), (4.2e-07, 9.0e-08)),    # [9.75e-08 / 2.08e-08] | [1.05e-07 / 2.25e-08]
    ("g_nln_b_lowvar", "f32"):       ((3.9e-07, 9.2e-08), (5.0e-07, 8.8e-08)),    # [9.74e-08 / 2.18e-08] | [1.24e-07 / 2.19e-08]
    ("g_nln_b_offset", "bf16"):      ((3.9e-07, 8.3e-08), (4.8e-07, 9.4e-08)),    # [9.75e-08 / 2.07e-08] | [1.20e-07 / 2.23e-08]
    ("g_nln_b_offset", "f32"):       ((6.1e-07, 9.4e-08), (5.1e-07, 9.0e-08)),    # [1.46e-07 / 2.23e-08] | [1.27e-07 / 2.24e-08]
    ("g_nln_g", "bf16"):             ((9.7e-07, 1.3e-07), (9.2e-07, 1.3e-07)),    # [2.42e-07 / 3.02e-08] | [2.30e-07 / 3.03e-08]
    ("g_nln_g", "f32"):              ((8.9e-07, 1.3e-07), (8.2e-07, 1.2e-07)),    # [2.22e-07 / 3.01e-08] | [1.96e-07 / 2.99e-08]
    ("g_nln_g_lowvar", "bf16"):      ((6.2e-07, 1.1e-07), (6.1e-07, 1.1e-07)),    # [1.55e-07 / 2.53e-08] | [1.46e-07 / 2.57e-08]
    ("g_nln_g_lowvar", "f32"):       ((5.3e-07, 1.1e-07), (5.2e-07, 1.1e-07)),    # [1.26e-07 / 2.55e-08] | [1.23e-07 / 2.53e-08]
    ("g_nln_g_offset", "bf16"):      ((2.3e-06, 6.1e-07), (2.3e-06, 6.1e-07)),    # [5.71e-07 / 1.52e-07] | [5.72e-07 / 1.52e-07]
    ("g_nln_g_offset", "f32"):       ((2.4e-06, 6.2e-07), (2.4e-06, 6.4e-07)),    # [5.92e-07 / 1.54e-07] | [5.82e-07 / 1.53e-07]
    ("hout", "bf16"):                ((ONE_ULP, 1.9e-06), (1.4e-02, 1.4e-03)),    # [1.54e-03 / 4.71e-07] | [3.45e-03 / 3.35e-04]
    ("hout", "f32"):                 ((7.7e-07, 7.9e-08), (7.1e-07, 8.5e-08)),    # [1.92e-07 / 1.97e-08] | [1.77e-07 / 2.03e-08]
    ("hout_lowvar", "bf16"):         ((ONE_ULP, 2.9e-07), (1.5e-02, 1.1e-03)),    # [2.29e-06 / 2.63e-10]  [stand-in 2.93e-04 / 7.16e-08] | [3.52e-03 / 2.59e-04]
    ("hout_lowvar", "f32"):          ((6.6e-07, 4.4e-08), (6.2e-07, 4.6e-08)),    # [1.64e-07 / 1.10e-08] | [1.54e-07 / 1.14e-08]
    ("hout_offset", "bf16"):         ((ONE_ULP, 4.5e-07), (1.4e-02, 7.2e-04)),    # [5.79e-04 / 1.06e-07] | [3.32e-03 / 1.80e-04]
    ("hout_offset", "f32"):          ((2.2e-06, 4.2e-07), (2.2e-06, 4.2e-07)),    # [5.30e-07 / 1.05e-07] | [5.26e-07 / 1.05e-07]
    ("reduce", "f32"):               ((5.9e-07, 4.5e-08), (6.4e-07, 4.9e-08)),    # [1.41e-07 / 1.08e-08] | [1.60e-07 / 1.16e-08]
    ("rout", "bf16"):                ((ONE_ULP, 1.6e-06), (1.3e-02, 1.3e-03)),    # [1.54e-03 / 3.77e-07] | [3.17e-03 / 3.15e-04]
    ("rout", "f32"):                 ((8.0e-07, 8.2e-08), (7.7e-07, 8.2e-08)),    # [1.91e-07 / 2.04e-08] | [1.92e-07 / 2.05e-08]
    ("rout_lowvar", "bf16"):         ((ONE_ULP, 3.6e-08), (9.4e-03, 6.8e-04)),    # [7.34e-05 / 8.96e-09] | [2.34e-03 / 1.70e-04]
    ("rout_lowvar", "f32"):          ((6.0e-07, 3.9e-08), (6.4e-07, 3.9e-08)),    # [1.43e-07 / 9.34e-09] | [1.59e-07 / 9.66e-09]
    ("rout_offset", "bf16"):         ((ONE_ULP, 8.6e-07), (9.7e-03, 6.8e-04)),    # [1.16e-03 / 2.14e-07] | [2.31e-03 / 1.61e-04]
    ("rout_offset", "f32"):          ((2.2e-06, 4.2e-07), (2.1e-06, 4.2e-07)),    # [5.12e-07 / 1.01e-07] | [5.20e-07 / 1.01e-07]
    ("splitk", "bf16"):              ((1.3e-06, 1.3e-07), (1.3e-06, 1.3e-07)),    # [3.13e-07 / 3.05e-08] | [3.17e-07 / 3.04e-08]
    ("splitk", "f32"):               ((4.8e-06, 3.3e-07), (5.2e-06, 3.3e-07)),    # [1.20e-06 / 8.22e-08] | [1.23e-06 / 8.23e-08]
    ("tn", "bf16"):                  ((1.9e-06, 1.3e-07), (2.0e-06, 1.3e-07)),    # [4.69e-07 / 3.01e-08] | [4.90e-07 / 3.03e-08]
    ("tn", "f32"):                   ((5.7e-06, 3.8e-07), (5.8e-06, 3.8e-07)),    # [1.36e-06 / 9.48e-08] | [1.38e-06 / 9.48e-08]
    ("tn_grouped", "bf16"):          ((1.3e-06, 1.2e-07), (1.3e-06, 1.2e-07)),    # [3.11e-07 / 2.81e-08] | [3.05e-07 / 2.84e-08]
    ("tn_grouped", "f32"):           ((3.1e-06, 3.5e-07), (3.1e-06, 3.5e-07)),    # [7.64e-07 / 8.74e-08] | [7.68e-07 / 8.74e-08]
    ("xout", "bf16"):                ((7.4e-07, 4.5e-08), (6.6e-07, 5.2e-08)),    # [1.76e-07 / 1.06e-08] | [1.56e-07 / 1.23e-08]
    ("xout", "f32"):                 ((7.4e-07, 4.5e-08), (6.6e-07, 5.2e-08)),    # [1.76e-07 / 1.06e-08] | [1.56e-07 / 1.23e-08]
    ("xout_lowvar", "bf16"):         ((4.2e-07, 2.7e-08), (4.7e-07, 2.9e-08)),    # [1.04e-07 / 6.35e-09] | [1.17e-07 / 7.21e-09]
    ("xout_lowvar", "f32"):          ((4.2e-07, 2.7e-08), (4.7e-07, 2.9e-08)),    # [1.04e-07 / 6.35e-09] | [1.17e-07 / 7.21e-09]
    ("xout_offset", "bf16"):         ((4.7e-07, 5.7e-08), (3.3e-07, 9.2e-08)),    # [1.11e-07 / 1.36e-08] | [8.22e-08 / 2.18e-08]
    ("xout_offset", "f32"):          ((4.7e-07, 5.7e-08), (3.3e-07, 9.2e-08)),    # [1.11e-07 / 1.36e-08] | [8.22e-08 / 2.18e-08]
}
BOUNDS = {(o, k, ag): v[i] for (o, k), v in _BOUNDS.items() for i, ag in enumerate(("model", "f64"))}


def bf16_store(out, kind):
    """whether a BOUNDS output of a kind is stored as bf16 (everything else is an fp32 store)"""
    if kind != "bf16" or "f32src" in out or out.startswith("d_z32"):
        return False
    return any(out == b or out.startswith(b + "_") for b in ("hout", "rout", "d_z", "act_y", "act_da"))


# ---- rounding ---------------------------------------------------------------------------------------------------------------------
def store(v, typ, how):
    """a computed value as its stored image: how = "f64" (unrounded), "model" (rounded once from float64), "standin" (torch's cast)"""
    if how == "f64":
        return v.to(D)
    if typ == "f32":
        return v.to(F32).to(D)
    if how == "standin":
        return v.to(F32).to(torch.bfloat16).to(D)
    f = v.to(F32)
    return torch.from_numpy(bf16_rne(f).reshape(tuple(f.shape))).to(D)


@functools.lru_cache(maxsize=64)
def keep_mask(site, rows, cols, p=P_DROP):
    from oracle import tcdiff_oracle as O
    return O.dropout_keep(SEED, site, (rows, cols), p)


def drop_scale(p=P_DROP):
    """the fp32 scale the kernels multiply by (kernels.drop_params passes 1 / (1 - p) as a C float)"""
    return float(np.float32(1.0 / (1.0 - p))) if p > 0 else 1.0


# ---- the cases of the row block ---------------------------------------------------------------------------------------------------
def row_case(fs, shape, kind, *, grads=None, dz_f32=False, pos_mod=True, variant=""):
    flags = FLAG_SETS[fs][0]
    if grads is None:
        grads = "".join(k for k, on in (("x", True), ("h", flags & STORE_H), ("r", flags & STORE_ROT)) if on)
    return dict(fs=fs, flags=flags, nseq=shape[0], L=shape[1], chunks=shape[2], kind=kind, grads=grads, dz_f32=dz_f32, pos_mod=pos_mod,
                variant=variant)


def row_case_id(c):
    s = f"{c['fs']}-{c['nseq']}x{c['L']}c{c['chunks']}-{c['kind']}-g{c['grads']}"
    return s + ("-dz32" if c["dz_f32"] else "") + ("" if c["pos_mod"] else "-nomod") + c["variant"]


def row_cases():
    out = []
    for kind in ("f32", "bf16"):
        out += [row_case(fs, shape, kind) for shape in SHAPES for fs in FLAG_SETS]
        out.append(row_case("pooled_norm", (3, 1, 1), kind, grads="h", dz_f32=True))                  # train_engine.py:1139
        out.append(row_case("norm_rot", (2, 152, 8), kind, grads="hr", dz_f32=True))                  # :1113, memory rows, L = S + 2
        out.append(row_case("dec_self", (2, 150, 8), kind, grads="hr", dz_f32=True))                  # every stage in front of an fp32 d_z
        out += [row_case("dec_self", (2, 20, 8), kind, grads=g) for g in ("hr", "h", "xh")]
        out += [row_case("dec_ffn", (2, 150, 8), kind, grads=g) for g in ("xhr", "h")]
        out += [row_case(fs, (2, 7, 1), kind, pos_mod=False) for fs in ("norm_rot", "dec_self")]
        for v in ("_lowvar", "_offset"):
            out += [row_case(fs, (3, 50, 3), kind, variant=v) for fs in ("dec_self", "dec_cross", "enc_attn")]
    return out


def row_groups():
    """[(test id, cases)]: a flag set's plain cases (default gradients, T-typed d_z, pos_mod = L, unit normal) at every shape form one
    test per kind; every other case is a test of its own"""
    groups = {}
    for c in row_cases():
        plain = c == row_case(c["fs"], (c["nseq"], c["L"], c["chunks"]), c["kind"])
        groups.setdefault(f"{c['fs']}-{c['kind']}-every-shape" if plain else row_case_id(c), []).append(c)
    return list(groups.items())


def row_inputs(c, seed=4):
    """float32 CPU tensors of one case; T-typed operands (d_h, d_rot) hold bf16-representable values in a bf16 case.  Accumulating
    outputs' starting values are part of the inputs ("start_*")."""
    nseq, L = c["nseq"], c["L"]
    M = nseq * L
    cast = bf if c["kind"] == "bf16" else (lambda t: t)
    z, xres = rnd(seed, M, 512), rnd(seed + 1, M, 512)
    if c["variant"] == "_lowvar":                         # one sequence at 1e-2: variance 1e-4 against eps 1e-6 / 1e-5
        z[:L] *= 1e-2
        xres[:L] *= 1e-2
    if c["variant"] == "_offset":                         # row mean = 30 deviations
        z = z + 30.0
        xres = xres + 30.0
    x = dict(z=z, xres=xres, bias=0.3 * rnd(seed + 2, 512), ln_g=1 + 0.1 * rnd(seed + 3, 512), ln_b=0.1 * rnd(seed + 4, 512),
             nln_g=1 + 0.1 * rnd(seed + 5, 512), nln_b=0.1 * rnd(seed + 6, 512), film=0.3 * rnd(seed + 7, nseq, 2048),
             rope=rope_f32(M + 8), d_xn=rnd(seed + 8, M, 512), d_h=cast(rnd(seed + 9, M, 512)), d_rot=cast(rnd(seed + 10, M, 512)),
             start_film=rnd(seed + 11, nseq, 2048))
    for i, k in enumerate(ROW_OUT_B[3:]):
        x["start_" + k] = rnd(seed + 12 + i, 512)
    return x


def pos_of(c):
    """(pos_mod, pos_base) of a case: pos_mod = L with pos_base = 3, or pos_mod = 0 with pos_base = 0"""
    return (c["L"], 3) if c["pos_mod"] else (0, 0)


def chunk_of(c):
    """per-row (chunk, index inside the chunk) of tcdiff_row_bwd's grid: per = ceil(L / chunks), lo = chunk * per"""
    per = -(-c["L"] // c["chunks"])
    pos = torch.arange(c["nseq"] * c["L"]) % c["L"]
    return pos // per, pos % per


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
class Ops:
    def __init__(self, dtype=D, defect=None):
        if defect is not None and defect not in DEFECTS:
            raise ValueError(defect)
        self.D, self.defect = dtype, defect
        self.how = "standin" if dtype != D else None

    def c(self, t):
        return torch.as_tensor(t).detach().cpu().to(self.D)

    # -- LayerNorm and rotary ---------------------------------------------------------------------------------------------------
    def ln_norm(self, v, eps):
        """two-pass statistics: x_hat = (v - mean) rstd, rstd = 1 / sqrt(mean((v - mean)^2) + eps)"""
        cen = v - v.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt((cen * cen).mean(-1, keepdim=True) + eps)
        return cen * rstd, rstd

    @staticmethod
    def ln_bwd(xhat, rstd, gy, g):
        """dx of y = x_hat g + b: rstd (gh - mean(gh) - x_hat mean(gh x_hat)), gh = gy g"""
        gh = gy * g
        return (gh - gh.mean(-1, keepdim=True) - xhat * (gh * xhat).mean(-1, keepdim=True)) * rstd

    @staticmethod
    def rot(u, cs, adjoint=False):
        """pairs (2j, 2j + 1) rotated by the angle of cs = (cos, sin); the adjoint is the rotation by the negative angle"""
        up, cp = u.reshape(*u.shape[:-1], 256, 2), cs.reshape(*cs.shape[:-1], 256, 2)
        co, si = cp[..., 0], (-cp[..., 1] if adjoint else cp[..., 1])
        return torch.stack((up[..., 0] * co - up[..., 1] * si, up[..., 1] * co + up[..., 0] * si), -1).reshape(u.shape)

    # -- the row block ----------------------------------------------------------------------------------------------------------
    def row(self, c, x):
        """forward and backward of one case -> unrounded outputs (dtype self.D): xout, hout, rout, d_z, d_xres, d_film [nseq, 1024] and
        the five parameter gradients (sums only: the starting values are added by finish_row)"""
        f, nseq, L, de = c["flags"], c["nseq"], c["L"], self.defect
        M = nseq * L
        t = {k: self.c(v) for k, v in x.items()}
        sc = drop_scale()
        kpre = keep_mask(SITE_PRE, M, 512).to(self.D) * sc
        kpost = kpre if de == "drop_post_uses_site_pre" else keep_mask(SITE_POST, M, 512).to(self.D) * sc
        eps1, eps2 = (NLN_EPS, LN_EPS) if de == "ln_eps_swapped" else (LN_EPS, NLN_EPS)
        seq = torch.arange(M) // L
        fseq = (torch.arange(M) + 1) // L % nseq if de == "film_row_of_next_sequence" else seq
        pm, pb = pos_of(c)
        pos = pb + (torch.arange(M) if (pm == 0 or de == "rotary_pos_without_mod") else torch.arange(M) % pm)
        cs = t["rope"][pos]
        # ---- forward ----
        v = t["z"]
        if f & BIAS:
            v = v + t["bias"]
        if f & DROP_PRE:
            v = v * kpre
        uhat = rstd = None
        if f & LN_POST:
            uhat, rstd = self.ln_norm(v, eps1)
            v = uhat * t["ln_g"] + t["ln_b"]
        if f & DROP_POST:
            v = v * kpost
        y = v
        s1 = None
        if f & FILM:
            s1, sh = t["film"][fseq, 1024:1536] + 1.0, t["film"][fseq, 1536:2048]
            v = s1 * y + sh
        if f & RES:
            v = t["xres"] + v
        xn = v
        u, xh2, rstd2 = xn, None, None
        if f & NEXT_LN:
            xh2, rstd2 = self.ln_norm(xn, eps2)
            u = xh2 * t["nln_g"] + t["nln_b"]
        out = {"xout": xn, "hout": u, "rout": self.rot(u, cs)}
        # ---- backward ----
        zero = torch.zeros(M, 512, dtype=self.D)
        gh = t["d_h"] if "h" in c["grads"] else zero
        if "r" in c["grads"]:
            gh = gh + self.rot(t["d_rot"], cs, adjoint=True)
        gx = t["d_xn"] if "x" in c["grads"] else zero
        per_row = {}
        if f & NEXT_LN:
            per_row["g_nln_g"], per_row["g_nln_b"] = gh * xh2, gh
            gx = gx + self.ln_bwd(xh2, rstd2, gh, t["nln_g"])
        else:
            gx = gx + gh
        out["d_xres"] = gx
        gy = gx
        if f & FILM:
            per_row["film_s"], per_row["film_sh"] = gx * y, gx
            gy = gx * s1
        if f & DROP_POST:
            gy = gy * kpost
        gu = gy
        if f & LN_POST:
            per_row["g_ln_g"], per_row["g_ln_b"] = gy * uhat, gy
            gu = self.ln_bwd(uhat, rstd, gy, t["ln_g"])
        per_row["g_bias"] = gu
        if f & DROP_PRE:
            gu = gu * kpre
        if de != "bias_grad_before_pre_dropout":
            per_row["g_bias"] = gu
        out["d_z"] = gu
        # ---- the column sums: every row of a chunk, whichever wave ran it ----
        w = torch.ones(M, 1, dtype=self.D)
        chunk, idx = chunk_of(c)
        if de == "upper_waves_not_folded":
            w[idx % 8 >= 4] = 0.0
        if de == "last_chunk_one_row_short":
            last = torch.arange(M) % L == L - 1
            w[last] = 0.0
            out["d_z"] = torch.where(last[:, None], zero, out["d_z"])
            out["d_xres"] = torch.where(last[:, None], zero, out["d_xres"])
        for k in ROW_OUT_B[3:]:
            out[k] = (per_row[k] * w).sum(0) if k in per_row else torch.zeros(512, dtype=self.D)
        if f & FILM:
            oh = (seq[None, :] == torch.arange(nseq)[:, None]).to(self.D)
            out["d_film"] = torch.cat([oh @ (per_row["film_s"] * w), oh @ (per_row["film_sh"] * w)], 1)
        else:
            out["d_film"] = torch.zeros(nseq, 1024, dtype=self.D)
        return out

    def finish_row(self, c, x, raw, how):
        """the stored images: accumulating outputs as start + sums, every output rounded to its storage type (how: "model", "f64")"""
        how = self.how or how
        T = c["kind"]
        o = {"xout": store(raw["xout"], "f32", how), "hout": store(raw["hout"], T, how), "rout": store(raw["rout"], T, how),
             "d_xres": store(raw["d_xres"], "f32", how)}
        dz_t = "f32" if (c["dz_f32"] and self.defect != "dz_f32_ignored") else T
        o["d_z"] = store(raw["d_z"], dz_t, how)
        start = torch.zeros_like(raw["d_film"]) if self.defect == "film_grad_stored_not_added" else self.c(x["start_film"][:, 1024:])
        o["d_film"] = store(start + raw["d_film"], "f32", how)
        for k in ROW_OUT_B[3:]:
            o[k] = store(self.c(x["start_" + k]) + raw[k], "f32", how).reshape(1, 512)
        return o

    # -- activation + dropout -----------------------------------------------------------------------------------------------------
    def act(self, a, act):
        if act == ACT_RELU:
            return torch.clamp_min(a, 0.0)
        if act == ACT_GELU:
            return 0.5 * a * (1.0 + torch.erf(a * math.sqrt(0.5)))
        if act == ACT_MISH:
            return a * torch.tanh(torch.clamp_min(a, 0.0) + torch.log1p(torch.exp(-a.abs())))
        if act == ACT_SILU:
            return a * torch.sigmoid(a)
        return a

    def act_grad(self, a, act):
        if act == ACT_RELU:
            return (a > 0).to(a.dtype)
        if act == ACT_GELU:
            return 0.5 * (1.0 + torch.erf(a * math.sqrt(0.5))) + a * torch.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
        sg = torch.sigmoid(a)
        if act == ACT_MISH:
            th = torch.tanh(torch.clamp_min(a, 0.0) + torch.log1p(torch.exp(-a.abs())))
            return th + a * (1.0 - th * th) * sg
        if act == ACT_SILU:
            return sg * (1.0 + a * (1.0 - sg))
        return torch.ones_like(a)

    def act_keep(self, rows, cols, ld, p, site):
        if p <= 0:
            return torch.ones(rows, cols, dtype=self.D)
        if self.defect == "drop_index_with_ld":
            return keep_mask(site, rows, ld, p)[:, :cols].to(self.D)
        return keep_mask(site, rows, cols, p).to(self.D)

    def act_drop(self, a, dy, act, p, site, ld):
        """a, dy [rows, cols] operand values -> (y, da) unrounded"""
        a, dy = self.c(a), self.c(dy)
        k = self.act_keep(a.shape[0], a.shape[1], ld, p, site) * drop_scale(p)
        kb = k * drop_scale(p) if self.defect == "act_bwd_scale_twice" else k
        return self.act(a, act) * k, dy * kb * self.act_grad(a, act)

    # -- cast / transpose ---------------------------------------------------------------------------------------------------------
    def colsum(self, src, start):
        return self.c(start) + self.c(src).sum(0)

    # -- weight gradients ---------------------------------------------------------------------------------------------------------
    def gemm(self, init, A, B):
        """init + A^T B over token-major operands A [rows, n_out], B [rows, n_in]"""
        return self.c(init) + self.c(A).t() @ self.c(B)

    def gemm_split(self, init, A, B, kt, splits):
        """the same as tcdiff_gemm_tile's split-K walks it: split s takes k-tiles [nk s / splits, nk (s + 1) / splits)"""
        A, B = self.c(A), self.c(B)
        nk = A.shape[0] // kt
        splits = max(1, min(splits, nk))
        out = self.c(init).clone()
        for s in range(splits):
            k0, k1 = nk * s // splits, nk * (s + 1) // splits
            if self.defect == "splitk_ranges_overlap":
                k1 = min(nk, -(-nk * (s + 1) // splits))
            out += A[k0 * kt:k1 * kt].t() @ B[k0 * kt:k1 * kt]
        return out

    def gemm_grouped(self, probs, kt, n_cu):
        """probs: [(init, A, B)] -> outputs, accumulated segment by segment in the order of the launcher's shares"""
        shapes = [(A.shape[1], B.shape[1], A.shape[0]) for _, A, B in probs]
        outs = [self.c(i).clone() for i, _, _ in probs]
        ops = [(self.c(A), self.c(B)) for _, A, B in probs]
        for _, pi, tile, k0, nk in grouped_split(shapes, kt, n_cu, self.defect)["segments"]:
            tiles_n = shapes[pi][1] // 128
            m0, n0 = tile // tiles_n * 128, tile % tiles_n * 128
            A, B = ops[pi]
            outs[pi][m0:m0 + 128, n0:n0 + 128] += A[k0 * kt:(k0 + nk) * kt, m0:m0 + 128].t() @ B[k0 * kt:(k0 + nk) * kt, n0:n0 + 128]
        return outs


def standin(defect=None):
    """the kernels' arithmetic in float32 torch on the CPU"""
    return Ops(F32, defect)


# ---- the grouped launcher's split, restated (csrc/gemm.hip tcdiff_gemm_tn_grouped, gemm_tn_grouped_kernel) -------------------------
def grouped_split(shapes, kt, n_cu, defect=None):
    """shapes [(n_out, n_in, tokens)] -> dict(per, kc, grid, units, segments [(share, problem, tile, first k-tile, k-tiles)],
    cross_tile, cross_prob: shares that hold units of more than one tile / problem)"""
    probs, units = [], 0
    for M, N, Kd in shapes:
        probs.append(dict(unit0=units, tiles=(M // 128) * (N // 128), nk=Kd // kt))
        units += probs[-1]["tiles"] * probs[-1]["nk"]
    per = max(4, -(-units // n_cu))
    kc, grid = per, -(-units // per)
    segs, cross_tile, cross_prob = [], 0, 0
    for wg in range(grid):
        u, u_end = wg * per, min(wg * per + per, units)
        seen = []
        while u < u_end:
            pi = 0
            while pi + 1 < len(probs) and probs[pi + 1]["unit0"] <= u:
                pi += 1
            pr = probs[pi]
            lu = u - pr["unit0"]
            nch = -(-pr["nk"] // kc)
            ch = min(lu // (pr["tiles"] * kc), nch - 1)
            clen = min(kc, pr["nk"] - ch * kc)
            local = lu - ch * pr["tiles"] * kc
            tile, kin = local // clen, local % clen
            nk = min(clen - kin, u_end - u)
            nk_run, k0 = nk, ch * kc + kin
            if defect == "share_tail_dropped" and nk < clen - kin:
                nk_run = nk - 1
            if defect == "unit_at_problem_boundary" and pi > 0 and lu == 0:
                nk_run, k0 = nk_run - 1, k0 + 1
            if nk_run > 0:
                segs.append((wg, pi, tile, k0, nk_run))
            seen.append((pi, tile))
            u += nk
        cross_tile += len(set(seen)) > 1
        cross_prob += len({p for p, _ in seen}) > 1
    return dict(per=per, kc=kc, grid=grid, units=units, segments=segs, cross_tile=cross_tile, cross_prob=cross_prob, probs=probs)


def coverage(shapes, kt, n_cu):
    """how often every (problem, tile, k-tile) is visited by the split: a list of int arrays [tiles, k-tiles]"""
    sp = grouped_split(shapes, kt, n_cu)
    cnt = [np.zeros((p["tiles"], p["nk"]), dtype=np.int64) for p in sp["probs"]]
    for _, pi, tile, k0, nk in sp["segments"]:
        cnt[pi][tile, k0:k0 + nk] += 1
    return cnt


def tn_deep(M, N, Kd, kt, splits, n_cu):
    """tcdiff_gemm_tn's four-stage / two-stage choice: about one workgroup per CU and at least 3 k-tiles per split"""
    s = min(splits, Kd // kt)
    return (M // 128) * (N // 128) * s * 4 <= n_cu * 5 and Kd // kt // s >= 3


# ---- GEMM cases: (n_out, n_in, tokens) --------------------------------------------------------------------------------------------
def kt_of(kind):
    return 64 if kind == "bf16" else 32


LONG = [(512, 512, 3392), (1024, 512, 3392)]
GROUPED = {
    # name: (shapes, {kind: per on 256 CUs})
    "short-k": ([(256, 256, 128), (128, 384, 192), (128, 128, 64)], {"bf16": 4, "f32": 4}),
    "long": (LONG, {"bf16": 10, "f32": 20}),
    "mixed": (LONG + [(128, 128, 64), (256, 128, 192), (512, 1536, 1344)], {"bf16": 14, "f32": 28}),
    "one-unit": ([(128, 128, 64)] * TN_MAX_PROB, {"bf16": 4, "f32": 4}),       # tokens = kt of the kind: see grouped_shapes
}
DATA = ("int", "normal")


def grouped_shapes(name, kind):
    shapes = GROUPED[name][0]
    if name == "one-unit":
        shapes = [(128, 128, kt_of(kind))] * TN_MAX_PROB
    return shapes


def grouped_regime(name, kind, n_cu):
    """(reached, text): the predicate of a grouped case restated from the CU count"""
    sp = grouped_split(grouped_shapes(name, kind), kt_of(kind), n_cu)
    want = GROUPED[name][1][kind]
    nks = [p["nk"] for p in sp["probs"]]
    ok = sp["per"] == want
    if name == "short-k":
        ok = ok and all(sp["per"] > nk or sp["per"] == 4 for nk in nks) and sp["cross_tile"] > 0
    if name in ("long", "mixed"):
        ok = ok and sp["per"] > 4 and any(nk % sp["per"] for nk in nks) and sp["cross_tile"] > 0
    if name == "mixed":
        ok = ok and sp["cross_prob"] > 0
    txt = (f"{name} {kind} on {n_cu} CUs: units {sp['units']} per = kc = {sp['per']} (wanted {want}) grid {sp['grid']} k-tiles {nks} "
           f"shares crossing a tile {sp['cross_tile']}, a problem {sp['cross_prob']}")
    return ok, txt


@functools.lru_cache(maxsize=None)
def gemm_operands(shape, kind, data, seed):
    """token-major operands inside wider buffers, as the engine reads them in place: dY [rows, n_out + 128] used from column 64,
    X [rows, n_in + 8]; init [n_out, n_in].  "int": integers in -4 .. 4 (exact in bf16, sums below 2^24, init integers too)."""
    n_out, n_in, rows = shape
    g = torch.Generator().manual_seed(seed)
    if data == "int":
        mk = lambda *s: torch.randint(-4, 5, s, generator=g).to(F32)
    else:
        mk = lambda *s: torch.randn(*s, generator=g)
    dY, X, init = mk(rows, n_out + 128), mk(rows, n_in + 8), mk(n_out, n_in)
    if kind == "bf16":
        dY, X = bf(dY), bf(X)
    return dY, X, init


@functools.lru_cache(maxsize=None)
def gemm_ref(shape, kind, data, seed):
    dY, X, init = gemm_operands(shape, kind, data, seed)
    n_out, n_in, _ = shape
    return Ops().gemm(init, dY[:, 64:64 + n_out], X[:, :n_in])


def tn_cases(kind):
    kt = kt_of(kind)
    return [((128, 128, kt), 1), ((128, 256, 2 * kt), 2)] + [((256, 384, 1344), s) for s in (1, 2, 7, 64)]


def splitk_cases(kind):
    kt = kt_of(kind)
    return [((200, 151, round_up(1000, kt)), 1), ((200, 151, round_up(1000, kt)), 5), ((3, 512, 65 * kt), 64), ((200, 151, 2 * kt), 9)]


# ---- element-wise cases -----------------------------------------------------------------------------------------------------------
ACT_TYPES = (("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"))              # (compute, source)
ACT_SHAPES = ((37, 438, 448, 448, 0), (5, 3, 4, 8, 0), (9, 438, 439, 441, 0), (4, 64, 64, 128, 0), (6, 40, 48, 48, 1))
#             rows, cols, ld_a, ld_y, pointer offset in elements
EXTREME = (0.0, -0.0, 1e-8, -1e-8, 5.0, -5.0, 19.999, -19.999, 20.001, -20.001, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)
ACT_SITE = 22


def act_inputs(rows, cols, kind, src, seed=3, extreme=False):
    """a (the source type's values) and dy (T's values) [rows, cols]; with `extreme` row 0 starts with the extreme arguments"""
    a, dy = 2.0 * rnd(seed, rows, cols), rnd(seed + 1, rows, cols)
    if extreme:
        n = min(cols, len(EXTREME))
        a[0, :n] = torch.tensor(EXTREME[:n])
    if src == "bf16":
        a = bf(a)
    if kind == "bf16":
        dy = bf(dy)
    return a, dy


CAST_SHAPES = ((150, 151, 152), (1, 1, 1), (1000, 70, 71))                  # rows, cols, ld_src


# ---- regions ----------------------------------------------------------------------------------------------------------------------
def row_regions(c):
    """regions of a [M, 512] row-block output: the whole tensor, each sequence, the first and the last row of every sequence, each
    non-empty (sequence, chunk) row range and in it the rows of the upper four waves, the last M % 4 rows"""
    nseq, L = c["nseq"], c["L"]
    M, cols = nseq * L, slice(0, 512)
    m = torch.arange(M)
    chunk, idx = chunk_of(c)
    out = [("all", None, cols)]
    out += [(f"seq{s}", m // L == s, cols) for s in range(nseq)]
    out += [("first", m % L == 0, cols), ("last", m % L == L - 1, cols)]
    for s in range(nseq):
        for k in range(c["chunks"]):
            rows = (m // L == s) & (chunk == k)
            if bool(rows.any()):
                out.append((f"chunk{s}.{k}", rows, cols))
                if bool((rows & (idx % 8 >= 4)).any()):
                    out.append((f"upper{s}.{k}", rows & (idx % 8 >= 4), cols))
    if M % 4:
        out.append(("tail4", m >= M // 4 * 4, cols))
    return out


def vec_regions():
    return [("all", None, slice(0, 512)), ("half0", None, slice(0, 256)), ("half1", None, slice(256, 512))]


def film_regions(nseq):
    out = [("all", None, slice(0, 1024)), ("scale", None, slice(0, 512)), ("shift", None, slice(512, 1024))]
    return out + [(f"seq{s}", torch.arange(nseq) == s, slice(0, 1024)) for s in range(nseq)]


def tile_regions(M, N, tile=128):
    out = [("all", None, slice(0, N))]
    for i in range(-(-M // tile)):
        rows = (torch.arange(M) >= i * tile) & (torch.arange(M) < (i + 1) * tile)
        out += [(f"tile{i}.{j}", rows, slice(j * tile, min(N, (j + 1) * tile))) for j in range(-(-N // tile))]
    return out


def band_regions(rows, cols):
    """cast_transpose: the whole tensor, the last partial 64-row band and the last partial 64-column band"""
    out = [("all", None, slice(0, cols))]
    if rows % 64:
        out.append(("rowband", torch.arange(rows) >= rows // 64 * 64, slice(0, cols)))
    if cols % 64:
        out.append(("colband", None, slice(cols // 64 * 64, cols)))
    return out


def region_class(name):
    return name.split(":")[-1].rstrip("0123456789.")


def row_out_name(out, c):
    return ("d_z32" if out == "d_z" and c["dz_f32"] else out) + c["variant"]


def regions_of_row(out, c):
    if out == "d_film":
        return film_regions(c["nseq"])
    return vec_regions() if out.startswith("g_") else row_regions(c)


def live_outputs(c):
    """the outputs a case's launches write (the others must keep their starting bits)"""
    f = c["flags"]
    live = [o for o, on in (("xout", f & STORE_X), ("hout", f & STORE_H), ("rout", f & STORE_ROT)) if on]
    live += ["d_z", "g_bias"] + (["d_xres"] if f & RES else []) + (["d_film"] if f & FILM else [])
    live += (["g_ln_g", "g_ln_b"] if f & LN_POST else []) + (["g_nln_g", "g_nln_b"] if f & NEXT_LN else [])
    return live


def measure(got, refs, kind, regs_of, name_of=lambda o: o, only=None):
    """[(bounds key, region, max, mean)] of every output in `got` against refs["model"] and refs["f64"], region by region"""
    rows = []
    for out, g in got.items():
        if only is not None and out not in only:
            continue
        for against in ("model", "f64"):
            st = region_stats(g, refs[against][out], regs_of(out))
            rows += [((name_of(out), kind, against), reg, mx, mn) for reg, (mx, mn) in st.items()]
    return rows


def measure_row(c, got, refs):
    return measure(got, refs, c["kind"], lambda o: regions_of_row(o, c), lambda o: row_out_name(o, c), only=live_outputs(c))


def row_refs(c, x):
    ops = Ops()
    raw = ops.row(c, x)
    return {"model": ops.finish_row(c, x, raw, "model"), "f64": ops.finish_row(c, x, raw, "f64")}


def frobenius(got, ref):
    got, ref = torch.as_tensor(got).detach().cpu().double().reshape(-1), torch.as_tensor(ref).detach().cpu().double().reshape(-1)
    return float((got - ref).norm() / (ref.norm() + 1e-300))


def report(rows, worst=None):
    """one printed line: per output the worst max / mean over its regions, against the model | against float64; the worst figure of
    each region class is folded into `worst` when given"""
    line = {}
    for key, reg, mx, mn in rows:
        d = line.get(key, (0.0, 0.0))
        line[key] = (max(d[0], mx), max(d[1], mn))
        if worst is not None:
            w = worst.setdefault(key, {})
            cls = region_class(reg)
            w[cls] = (max(w.get(cls, (0, 0))[0], mx), max(w.get(cls, (0, 0))[1], mn))
    if line:
        print(" ".join(f"{out}[{kind}]={line[(out, kind, 'model')][0]:.1e}/{line[(out, kind, 'model')][1]:.1e}|"
                       f"{line[(out, kind, 'f64')][0]:.1e}/{line[(out, kind, 'f64')][1]:.1e}" for out, kind, ag in line if ag == "model"))


def outside(rows, bounds=None):
    bounds = BOUNDS if bounds is None else bounds
    return [(key, reg, mx, mn, bounds[key]) for key, reg, mx, mn in rows if not (mx <= bounds[key][0] and mn <= bounds[key][1])]
