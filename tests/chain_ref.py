"""render_sample's corrector chain composed from the five float64 restatements, for the tests: beat_sync -> smooth -> keep_apart ->
ground -> foot_lock in the order and with the threading of tcdiff_amd/diffusion.py (q, pos, joints and contacts handed from stage to
stage as the float32 words the kernels hand over), every stage's result kept.  Nothing is restated here: the stages are
tests/{beatsync,smooth,apart,ground,footlock}_ref.py, imported.  Also the seeded cases N ("normal"), L ("long") and P (poison) as
normalised sample rows, a float32 stand-in of the export for the machines without a GPU, the margins of the decisions the stages
make, and the scores the end-state promises are stated in."""
import functools

import numpy as np
import torch

import apart_ref as AR
import beatsync_ref as BR
import export_ref as XR
import footlock_ref as FR
import ground_ref as GR
import group_ref as G
import metrics_ref as MR
import smooth_ref as SR
from tcdiff_amd import io as tio
from tcdiff_amd.fk import SMPL_OFFSETS

STAGES = ("beat_sync", "smooth", "keep_apart", "ground", "foot_lock")
SUBSETS = [tuple(s for i, s in enumerate(STAGES) if mask >> i & 1) for mask in range(32)]
KIN_GUARD = 1e-9          # tests/metrics_ref.py decisions_clear: neighbouring values of the smoothed speed, relative to its largest
REACH_GUARD = 1e-6        # metres between a leg's target distance and the reach limits at which foot_lock clamps
STILL_GUARD = 1e-6        # tests/test_footlock_cpu.py test_motion_labels_cannot_tie


# ---- one stage: the restatement on a state, and the state it hands on -------------------------------------------------------------------------
def joints_of(q, pos, dn):
    """the float32 joints of poses in rows, by the float64 FK of tests/smooth_ref.py: what stands in for a kernel's fk_forward off the GPU"""
    return BR.joints_of(q, pos, dn)


def stage(name, state, beats, dn, joints_in=None, joints_out=None):
    """one restatement on `state` = dict(q, pos, joints, contacts) of float32 arrays -> (its result, the state handed on).  beat_sync
    takes its speed from `joints_in` (default: the state's joints); the stages whose kernels run an FK of their own hand on
    `joints_out` (the kernel's, in the GPU tests) or joints_of(...)."""
    q, pos, J, C = state["q"], state["pos"], state["joints"], state["contacts"]
    fk = lambda q, pos: joints_of(q, pos, dn) if joints_out is None else np.asarray(joints_out, np.float32)
    if name == "beat_sync":
        ref = BR.beat_sync(q, pos, beats, dn, contacts=C, joints_in=J if joints_in is None else joints_in)
        return ref, dict(q=ref["q"], pos=ref["pos"], joints=fk(ref["q"], ref["pos"]), contacts=ref["contacts"])
    if name == "smooth":
        ref = SR.smooth(q, pos, dn)
        return ref, dict(q=ref["q"], pos=ref["pos"], joints=fk(ref["q"], ref["pos"]), contacts=C)
    if name == "keep_apart":
        ref = AR.keep_apart(pos, J, dn=dn, details=True)
        return ref, dict(q=q, pos=ref["pos"], joints=ref["joints"], contacts=C)
    if name == "ground":
        ref = GR.ground(pos, J, C, dn=dn, details=True)
        return ref, dict(q=q, pos=ref["pos"], joints=ref["joints"], contacts=C)
    if name == "foot_lock":
        ref = FR.foot_lock(q, pos, C, dn=dn)
        return ref, dict(q=ref["q"], pos=pos, joints=fk(ref["q"], pos), contacts=C)
    raise ValueError(name)


def chain(q, pos, contacts, beats, dn, on=STAGES, joints=None):
    """the stages of `on` in render_sample's order on the exported q (b, T dn, 24, 3), pos (b, T dn, 3), contacts (b, dn, T, 4) or None
    and the export's joints (default: joints_of) -> dict: "export" the state before, every stage's name -> (result, state after),
    "final" the last state"""
    q, pos = np.asarray(q, np.float32), np.asarray(pos, np.float32)
    state = dict(q=q, pos=pos, joints=joints_of(q, pos, dn) if joints is None else np.asarray(joints, np.float32),
                 contacts=None if contacts is None else np.asarray(contacts, np.float32))
    out = {"export": state}
    for name in STAGES:
        if name in on:
            ref, state = stage(name, state, beats, dn)
            out[name] = (ref, state)
    out["final"] = state
    return out


# ---- the margins of the decisions, from the restatements' own results -----------------------------------------------------------------------------
def kin_margin(ref):
    """the least difference of neighbouring values of a beat_sync result's smoothed speed curves, relative to each curve's largest: a
    strict minimum (a kinematic beat) cannot appear or vanish under a rounding while this is above KIN_GUARD.  Everything after the
    minima -- the matching, its ties, the rate bound -- is arithmetic on frame numbers, the same on both sides."""
    worst = np.inf
    for s in ref["speed"].reshape(-1, ref["speed"].shape[-1]):
        if np.isfinite(s).all() and s.shape[0] >= 2 and s.max() > 0:
            worst = min(worst, float(np.abs(s[1:] - s[:-1]).min() / s.max()))
    return worst


def reach_margin(ref):
    """the least distance, over the frames a foot_lock result solved, between the target's distance from the hip and the two limits
    at which the target is clamped (include/tcdiff_footlock.h step 4, reach = 1e-3)"""
    off = np.asarray(SMPL_OFFSETS, np.float32).astype(np.float64)
    worst = np.inf
    for (c, d, leg, t), inf in ref["info"].items():
        h, k, a, e = FR.LEGS[leg]
        l1, l2 = float(np.sqrt((off[k] ** 2).sum())), float(np.sqrt((off[a] ** 2).sum()))
        rmax, rmin = (l1 + l2) * (1.0 - 1e-3), abs(l1 - l2) + 1e-3 * (l1 + l2)
        worst = min(worst, abs(rmax - inf["nv"]), abs(inf["nv"] - rmin))
    return worst


def decisions(result, contacts_given):
    """{stage: (clear, what)} of a chain() result: every stage's discontinuous decisions against the guards their own modules set"""
    out = {}
    if "beat_sync" in result:
        m = kin_margin(result["beat_sync"][0])
        out["beat_sync"] = (m > KIN_GUARD, f"neighbouring smoothed speeds {m:.3e} apart (relative)")
    if "keep_apart" in result:
        out["keep_apart"] = AR.judge(result["keep_apart"][0])
    if "ground" in result:
        out["ground"] = GR.judge(result["ground"][0])
    if "foot_lock" in result:
        ref = result["foot_lock"][0]
        r, s = reach_margin(ref), ref["min_margin"]
        out["foot_lock"] = (r > REACH_GUARD and (contacts_given or s > STILL_GUARD), f"reach margin {r:.3e} m, still margin {s:.3e} m")
    return out


def ground_metrics_clear(ref):
    """ground_ref.judge for ground_metrics alone: of a ground(..., details=True) result the margins of the decisions the metrics make
    (the labels and the two tolerance counts), not those of the shift"""
    sub = dict(ref, details={k: (v if k in ("threshold", "still", "tolerance") else []) for k, v in ref["details"].items()})
    return GR.judge(sub)


# ---- the scores of section 3c, by the restatements ------------------------------------------------------------------------------------------------
def runs_of(g):
    """[(first, last, label)] of a (T,) label row of foot_lock's: the maximal runs of one non-zero label"""
    out, t, T = [], 0, len(g)
    while t < T:
        if g[t] == 0:
            t += 1
            continue
        end = t
        while end + 1 < T and g[end + 1] == g[t]:
            end += 1
        out.append((t, end, int(g[t])))
        t = end + 1
    return out


def slide(J64, g):
    """the least, over the planted runs of two frames or more, of the pinned joint's mean step: J64 (b, dn, T, 24, 3), g foot_lock's
    labels (b, dn, 2, T) -> metres a frame (inf without such a run)"""
    worst = np.inf
    for c, d, leg in np.ndindex(g.shape[:3]):
        for first, last, label in runs_of(g[c, d, leg]):
            if last > first:
                j = FR.LEGS[leg][2 if label == 1 else 3]
                worst = min(worst, float(np.linalg.norm(np.diff(J64[c, d, first:last + 1, j], axis=0), axis=-1).mean()))
    return worst


def pin_error(J64, ref):
    """the largest distance of a pinned joint from its run's anchor over the planted, unclamped frames of a foot_lock result; J64 the
    float64 joints of the locked poses"""
    worst, seen = 0.0, 0
    for leg, (h, k, a, e) in enumerate(FR.LEGS):
        g, st = ref["g"][:, :, leg], ref["status"][:, :, leg]
        pin = np.where((g == 2)[..., None], J64[..., e, :], J64[..., a, :])
        free = (g != 0) & (st != 2)
        if free.any():
            worst = max(worst, float(np.linalg.norm(pin - ref["anchor"][:, :, leg], axis=-1)[free].max()))
            seen += int(free.sum())
    return worst, seen


def scores(J32, contacts, beats):
    """what section 3c compares, of float32 joints (b, dn, T, 24, 3): body-contact frames (b, pairs), penetration and float frames
    (b, dn) against the floor estimated from these joints, jitter and accel_mean (b, dn), beat_align (b, dn)"""
    J32 = np.ascontiguousarray(J32, np.float32)
    b, dn, T = J32.shape[:3]
    pos = AR.pos_of(J32)
    contact = AR.keep_apart(pos, J32, rounds=0)["contact_before"] if dn > 1 else np.zeros((b, 0), np.int64)
    gm = GR.ground_metrics(J32, contacts)
    sm = SR.smoothness(J32)
    align = np.array([[MR.beat_one(J32[c, d], beats[c], 5.0, 3.0)[0] for d in range(dn)] for c in range(b)])
    return dict(contact_frames=contact, penetration_frames=gm["penetration_frames"], float_frames=gm["float_frames"],
                planted_frames=gm["planted_frames"], jitter=sm["jitter"], accel_mean=sm["accel_mean"], beat_align=align)


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------------------------
PERIOD = 12                                  # frames between music beats
REST = 24                                    # frames between a dancer's rests: every second beat (see motion)
LEG_JOINTS = [0, 1, 2, 4, 5, 7, 8]           # the pelvis and the two leg chains: what moves a foot
ARM_JOINTS = [13, 14, 16, 17, 18, 19, 20, 21, 22, 23]          # collars to hands: what two dancers side by side touch with
CLOSEST = 0.47                               # metres between the roots of dancers 0 and 1 where they are nearest
ROT_SIGMA, LEG_SIGMA, POS_SIGMA = 0.002, 0.001, 0.0005       # the jitter of tests/smooth_ref.py noisy_case, its sigmas chosen here (see motion)
NAMES = ["data/test/features/gBR_sBM_c01_d04_mBR0_ch01_slice3.npy", "data/test/features/npy_gLO_slice12.npy"]
FAULTS = ("late", "jitter", "overlap", "vertical", "drift")
SEED_N, SEED_L = 2, 2


def lags(dn):
    return np.array([2 + d % 2 for d in range(dn)])


def hill(t, first, last):
    """0 outside [first, last], a cos^2 bump to 1 inside"""
    x = np.clip((t - first) / float(last - first), 0.0, 1.0)
    return np.sin(np.pi * x) ** 2


def plateau(t, mid, flat=5, ramp=5):
    """1 within `flat` frames of mid, a cos^2 ramp to 0 over the next `ramp`"""
    x = np.clip((np.abs(t - mid) - flat) / float(ramp), 0.0, 1.0)
    return np.cos(0.5 * np.pi * x) ** 2


def rests(T, lag):
    return [r for r in range(lag + REST, T - 5, REST)]


def planted_runs(T, dn):
    """runs[dancer][leg] = [(first, last, "a" | "e")]: each dancer plants a foot around every rest (lag + 12 n), legs alternating from
    dancer to dancer, ankle and toe channels alternating"""
    runs = []
    for d, lag in enumerate(lags(dn)):
        per = [[], []]
        for n, r in enumerate(rests(T, lag)):
            per[(n + d) % 2].append((r - 4, min(r + 4, T - 1), "ae"[(n + d) % 3 == 0]))
        runs.append(per)
    return runs


@functools.lru_cache(maxsize=None)
def level_feet():
    """the further flexion of the right knee that brings the two toes of the standing pose of `motion` to one height (SMPL's hips are
    not mirror images: 1.1 cm without it, more than ground's tolerance), by bisection on a float64 FK"""
    def gap(delta):
        pose = np.zeros((24, 3))
        pose[0], pose[[1, 2], 0], pose[[4, 5], 0] = [np.pi / 2, 0.0, 0.0], -0.45, 0.9
        pose[5, 0] += delta
        P = GR.fk64(pose, np.zeros(3))
        return P[11, 2] - P[10, 2]
    lo, hi = -0.3, 0.3
    assert gap(lo) * gap(hi) < 0
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if gap(lo) * gap(mid) > 0 else (lo, mid)
    return 0.5 * (lo + hi)


@functools.lru_cache(maxsize=None)
def motion(b, dn, T, seed, without=()):
    """-> q (b, T dn, 24, 3), pos (b, T dn, 3), contacts (b, dn, T, 4), beats (b, T), float64 / float32 / uint8, z up, read-only.
    Every rotation component and the root's sway move as A cos(pi (t - lag) / 12) about a standing pose with flexed knees (the
    construction of tests/test_beatsync_gpu.py's render_sample test), and the root steps forward between every second pair of their
    rests: the speed is smallest at lag + 24 n, `lag` = 2 or 3 frames (by dancer) after every second of the music's beats at 12 n.  (A
    rest on every beat does not survive the speed curve's Gaussian of sigma 5 frames: it passes 3 % of a 12-frame period and 42 % of a
    24-frame one, and the minima then fall where the rounding and the jitter put them.)  The leg chains move a thirtieth of that, so that a planted foot slides by the root's drift: footlock_ref's
    DRIFT (its components on the floor), slow (6.7 mm a frame) around the rests and up to five times that between them, as a step is.  N(0, sigma) on every rotation
    component and on the root as tests/smooth_ref.py's noisy_case adds it: 2 mrad, but 1 mrad on the leg chains and 0.5 mm on the root, so
    that a foot still rests by the dataset's rule (1 cm a frame) where "long" mode has to label it from the motion.  Dancers
    0 and 1 drift towards each other over the first half of the clip and apart over the second (their capsules overlap around frame
    T / 2: only the sign of a drift component turns there, not the speed); dancer 0 sinks 5 cm below the others around its first
    rest and the last dancer floats 6 cm around its last.  `without`: names of FAULTS left out."""
    g = np.random.default_rng(seed)
    lag = lags(dn) if "late" not in without else np.zeros(dn, int)
    t = np.arange(T)
    ph = np.pi * (t[:, None] - lag[None, :]) / REST                               # (T, dn)
    base = g.normal(0.0, 0.03, (b, 1, dn, 24, 3))
    base[..., 0, :] = [np.pi / 2, 0.0, 0.0]                                        # SMPL's y up made z up
    base[..., [1, 2, 4, 5, 7, 8, 10, 11], :] = 0.0                                  # the legs alike: the feet are level, a planted foot is the body's lowest part
    base[..., [1, 2], 0], base[..., [4, 5], 0] = -0.45, 0.9                         # flexed knees (reach to spare), the toes below the ankles
    base[..., 5, 0] += level_feet()
    base[..., 16, 2], base[..., 17, 2] = -1.45, 1.45                               # the arms down: a body is 0.5 m wide
    amp = g.uniform(0.02, 0.1, (b, 1, dn, 24, 3))
    amp[..., LEG_JOINTS, :] /= 30.0
    amp[..., ARM_JOINTS, :] /= 4.0
    q = base + amp * np.cos(2 * ph)[None, :, :, None, None]
    u = np.sin(ph) ** 2
    speed = 1.0 + 4.0 * u ** 3 if "drift" not in without else np.zeros_like(u)          # (T, dn): 1 at the rests, 5 between them
    drift = np.tile([FR.DRIFT[2], FR.DRIFT[0], 0.0], (T, dn, 1))                   # DRIFT's components on the floor: 6.7 mm a frame
    if "overlap" not in without and dn > 1:
        drift[:T // 2, 1::2, 0] *= -1.0                                            # dancers 0 and 1 close in on each other over the first half
        drift[T // 2:, 0::2, 0] *= -1.0                                            # and part again over the second, at the same speed
    path = speed[:, :, None] * drift
    along = np.concatenate([np.zeros((1, dn, 3)), np.cumsum(path, 0)[:-1]])
    pos = np.zeros((b, T, dn, 3))
    pos += g.uniform(0.002, 0.006, (b, 1, dn, 3)) * [1.0, 1.0, 0.0] * np.cos(2 * ph)[None, :, :, None] + along[None]          # a sway on the floor
    closing = FR.DRIFT[2] * (speed[:T // 2, :2].sum() if "drift" not in without else 4.5 * T // 2)          # what two dancers close over half the clip
    pos[..., 0] += (CLOSEST + closing) * np.arange(dn)                             # dancers 0 and 1 are CLOSEST apart where they turn
    pos[..., 2] += 0.95
    if "vertical" not in without:
        first, last = rests(T, lag[0])[0], rests(T, lag[dn - 1])[-1]
        pos[:, :, 0, 2] -= 0.05 * plateau(t, first)                                # level over the planted run and the frames the retiming may bring into it
        pos[:, :, dn - 1, 2] += 0.06 * plateau(t, last)
    if "jitter" not in without:
        sigma = np.full(24, ROT_SIGMA)
        sigma[LEG_JOINTS] = LEG_SIGMA
        q = q + g.normal(0.0, 1.0, q.shape) * sigma[:, None]
        pos = pos + g.normal(0.0, POS_SIGMA, pos.shape)
    contacts = np.concatenate([FR.contacts_of(T, planted_runs(T, dn), dn)] * b)
    beats = np.zeros((b, T), np.uint8)
    beats[:, PERIOD:T - 1:PERIOD] = 1
    out = (q.reshape(b, T * dn, 24, 3), pos.reshape(b, T * dn, 3), contacts, beats)
    for a in out:
        a.setflags(write=False)
    return out


def normalizer(seed=7):
    """a seeded io.Normalizer of 151 columns: scales in [0.2, 0.3] (a root 2.9 m from the origin stays inside the clip to [-1, 1])"""
    g = np.random.default_rng(seed)
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_ = torch.from_numpy(g.uniform(0.2, 0.3, 151)).float()
    n.scaler.min_ = torch.from_numpy(g.uniform(-0.1, 0.1, 151)).float()
    return n


def rows_of_motion(q, pos, contacts, norm):
    """rotation vectors, roots and contacts -> normalised sample rows (b, T dn, 151) float32: contacts, root, the first two rows of
    every rotation matrix (what rotation_6d_to_matrix reads), scaled as the normalizer scales"""
    b, n = pos.shape[:2]
    R = GR.rodrigues(q)                                                          # (b, n, 24, 3, 3)
    u = np.zeros((b, n, 151))
    if contacts is not None:
        dn = contacts.shape[1]
        u[..., :4] = np.moveaxis(contacts, 1, 2).reshape(b, n, 4)
    u[..., 4:7] = pos
    u[..., 7:] = R[..., :2, :].reshape(b, n, 144)
    x = u * norm.scaler.scale_.double().numpy() + norm.scaler.min_.double().numpy()
    assert np.abs(x).max() < 1.0, "a column leaves the normalizer's range"
    return torch.from_numpy(x.astype(np.float32))


def cond_of(beats, windows=None):
    """cond (b, 2 T, 438) float32 with the beats in column 53; windows = (b, S): the half-overlapping windows of one song's beats (1, T)"""
    if windows is not None:
        b, S = windows
        beats = np.stack([beats[0, k * (S // 2):k * (S // 2) + S] for k in range(b)])
    cond = torch.zeros(beats.shape[0], 2 * beats.shape[1], 438)
    cond[:, 0::2, 53] = torch.from_numpy(beats.astype(np.float32))
    return cond


class Case:
    """a seeded case: x the normalised rows, cond, norm, mode, dn, names, beats (the music's beats on the exported frames)"""
    def __init__(self, mode, without=(), seed=None):
        self.mode, self.norm = mode, normalizer()
        if mode == "normal":
            self.dn, self.T, self.clips = 3, 60, 2
            q, pos, contacts, beats = motion(2, 3, 60, SEED_N if seed is None else seed, tuple(without))
            self.x, self.cond, self.beats, self.names = rows_of_motion(q, pos, contacts, self.norm), cond_of(beats), beats, NAMES
        else:
            self.dn, self.T, self.clips = 2, 80, 1
            S, h, dn = 40, 20, 2
            q, pos, _, beats = motion(1, 2, 80, SEED_L if seed is None else seed, tuple(without))
            cut = lambda a: np.concatenate([a.reshape((80, dn) + a.shape[2:])[k * h:k * h + S].reshape((1, S * dn) + a.shape[2:]) for k in range(3)])
            self.x, self.cond, self.beats, self.names = rows_of_motion(cut(q), cut(pos), None, self.norm), cond_of(beats, (3, S)), beats, NAMES[:1]

    def export(self):
        """the export's float32 results off the GPU: tests/export_ref.py's float64 export of the rows, rounded once"""
        s = self.norm.scaler
        out = XR.export(self.x, s.scale_, s.min_, self.mode, self.dn)
        return tuple(None if t is None else np.ascontiguousarray(t.numpy().astype(np.float32)) for t in out)


@functools.lru_cache(maxsize=None)
def case(which, without=(), seed=None):
    return Case({"N": "normal", "L": "long"}[which], without, seed)


# P: where N's exported poses are poisoned.  The NaN: clip 0, dancer 1, frame 39, the left knee -- mid-clip, the right foot planted, and
# the left leg six frames or more (blend + 1) from every planted run of its own (23-31, 47-55), so that foot_lock's shift of that leg
# is 0 there and the pose is left as it is (include/tcdiff_footlock.h defines nothing for a non-finite target); the +Inf: clip 1,
# dancer 0, frame 3, as far before that dancer's first run (10-18): the filter's edge rows have to cope with it
POISON_Q = (0, 39, 1, 4, 0)          # clip, frame, dancer, joint, component
POISON_POS = (1, 3, 0, 1)            # clip, frame, dancer, component


def poisoned(q, pos, dn):
    q, pos = np.array(q, np.float32), np.array(pos, np.float32)
    c, t, d, j, k = POISON_Q
    q[c, t * dn + d, j, k] = np.nan
    c, t, d, k = POISON_POS
    pos[c, t * dn + d, k] = np.inf
    return q, pos


# ---- section 3c: the promises on the end of the chain -----------------------------------------------------------------------------------------------
def end_state(c, raw, final, lock):
    """raw, final: states (q, pos, contacts as float32 arrays) before and after the whole chain of case `c`; lock: the restatement of
    foot_lock on the lock's own inputs.  Both ends are scored alike: a float64 FK (tests/ground_ref.py's, rotation matrices) of the
    float32 poses, then the restatements.  -> ({promise: kept}, the raw scores, the final scores, the pin error in metres)"""
    fk = lambda s: GR.fk64(SR.frames_of(s["q"], c.dn), SR.frames_of(s["pos"], c.dn))
    J1 = fk(final)
    s0, s1 = scores(fk(raw).astype(np.float32), raw["contacts"], c.beats), scores(J1.astype(np.float32), final["contacts"], c.beats)
    pin, seen = pin_error(J1, lock)
    kept = dict(pin=seen > 0 and pin <= FR.PIN_BOUND, jitter=bool((s1["jitter"] < s0["jitter"]).all()),
                accel_mean=bool((s1["accel_mean"] < s0["accel_mean"]).all()), beat_align=bool((s1["beat_align"] > s0["beat_align"]).all()))
    for k in ("contact_frames", "penetration_frames", "float_frames"):
        kept[k] = bool((s1[k] <= s0[k]).all())
    return kept, s0, s1, pin


def report(s0, s1):
    """the before / after scores as one line per score"""
    flat = lambda a: np.asarray(a).ravel().round(4).tolist()
    return "\n".join(f"    {k}: {flat(s0[k])} -> {flat(s1[k])}" for k in s0)
