"""ctypes binding of libtcdiff_gfx950.so (include/tcdiff_hip.h, include/tcdiff_hip_ext.h, include/tcdiff_gltf.h, include/tcdiff_skin.h
include/tcdiff_shade.h, include/tcdiff_mjpeg.h, include/tcdiff_footlock.h, include/tcdiff_group.h, include/tcdiff_apart.h,
include/tcdiff_ground.h, include/tcdiff_meshcontact.h, include/tcdiff_selfcontact.h, include/tcdiff_smooth.h, include/tcdiff_choreo.h and
include/tcdiff_beatsync.h).

The product path has NO fallback: if the shared library is missing or a launcher returns an error, this
module raises.  Nothing here touches ``oracle/``.
"""
import ctypes as C
import os

from . import _abi
from ._abi import TcdiffError  # noqa: F401  (raised here and by the header parser)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TCDIFF_LIB_PATH") or os.path.join(HERE, "libtcdiff_gfx950.so")   # override: diagnostic builds

ABI = _abi.load()
EXT = _abi.load_ext()                                # the second header: ABI stays the first header's
GLTF = _abi.load_gltf()                              # the third: tcx_gltf_animation, bound below, in none of ABI, EXT, EXPORTS
SKIN = _abi.load_skin()                              # the fourth: tcs_skin_vertices and its tile sizes, bound below, in none of the others
SHADE = _abi.load_shade()                            # the fifth: tcr_mesh_vertices, tcr_mesh_raster and their constants, likewise
MJPEG = _abi.load_mjpeg()                            # the sixth: tcj_mjpeg_workspace, tcj_mjpeg_plan, tcj_mjpeg_write and their constants, likewise
FOOTLOCK = _abi.load_footlock()                      # the seventh: tck_foot_lock_workspace, tck_foot_lock and their constants, likewise
GROUP = _abi.load_group()                            # the eighth: tcg_group_workspace, tcg_group_metrics and their constants, likewise
APART = _abi.load_apart()                            # the ninth: tcp_keep_apart_workspace, tcp_keep_apart and their constants, likewise
GROUND = _abi.load_ground()                          # the tenth: tcf_ground_workspace, tcf_ground_metrics, tcf_ground and their constants, likewise
MESH = _abi.load_meshcontact()                       # the eleventh: tcm_mesh_contact_workspace, tcm_mesh_contact and their constants, likewise
SELF = _abi.load_selfcontact()                       # the twelfth: tci_self_contact_workspace, tci_self_contact and their constants, likewise
SMOOTH = _abi.load_smooth()                          # the thirteenth: tcw_smoothness, tcw_smooth_workspace, tcw_smooth and their constants, likewise
CHOREO = _abi.load_choreo()                          # the fourteenth: tcc_plan, tcc_trajectory_error and their constants, likewise
BEATSYNC = _abi.load_beatsync()                      # the fifteenth: tcb_beat_sync_workspace, tcb_motion_beats, tcb_beat_sync and their constants, likewise

for _name, _value in {**ABI.constants, **EXT.constants}.items():          # TC_X -> X, TC_DTYPE_X -> DT_X
    globals()["DT_" + _name[9:] if _name.startswith("TC_DTYPE_") else _name[3:]] = _value
AUDIO_FMT = {f: ABI.constants["TC_AUDIO_" + f.upper()] for f in ("u8", "s16", "s24", "s32", "f32", "f64")}

TileEpi = ABI.structs["tcdiff_tile_epi"]
RowEpi = ABI.structs["tcdiff_row_epi"]
ChainArgs = ABI.structs["tcdiff_chain_args"]
StepPrologueArgs = ABI.structs["tcdiff_step_prologue_args"]
RowArgs = ABI.structs["tcdiff_row_args"]
CtDesc = ABI.structs["tcdiff_ct_desc"]
WsDesc = ABI.structs["tcdiff_ws_desc"]
TnProblem = ABI.structs["tcdiff_tn_problem"]
NavArgs = ABI.structs["tcdiff_nav_args"]
NavTrainArgs = ABI.structs["tcdiff_nav_train_args"]
AdanScalars = ABI.structs["tcdiff_adan_scalars"]
NavAdamWScalars = ABI.structs["tcdiff_nav_adamw_scalars"]
DrawStyle = ABI.structs["tcdiff_draw_style"]
ShadeStyle = SHADE.structs["tcr_shade_style"]

EXPORTS = sorted({**ABI.functions, **EXT.functions})

_lib = None
_rec = None          # a list while train_engine records a command list: every launcher call is appended as (function, arguments)


class _Recorder:
    """Stands in for the library while a step is being recorded: calls go through unchanged and are remembered."""

    def __init__(self, lib, out):
        self._lib, self._out = lib, out

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        out = self._out

        def call(*args):
            rc = fn(*args)
            out.append((fn, args))
            return rc
        return call


def load():
    """Load the HIP library; raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is not None:
        return _lib if _rec is None else _Recorder(_lib, _rec)
    if not os.path.exists(LIB_PATH):
        raise TcdiffError(f"{LIB_PATH} not found: build it with `python -m tcdiff_amd.build` "
                          "(the MI355X path has no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes, _) in {**ABI.functions, **EXT.functions, **GLTF.functions, **SKIN.functions, **SHADE.functions, **MJPEG.functions, **FOOTLOCK.functions,
                                            **GROUP.functions, **APART.functions, **GROUND.functions, **MESH.functions, **SELF.functions,
                                            **SMOOTH.functions, **CHOREO.functions, **BEATSYNC.functions}.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib


_ERR = {-1: "invalid argument", -2: "misaligned pointer / leading dimension", -3: "kernel launch failed",
        -4: "unsupported configuration", -5: "the eigen-solver did not converge"}


def check(rc: int, what: str):
    if rc != 0:
        raise TcdiffError(f"{what}: {_ERR.get(rc, 'error')} (code {rc})")
