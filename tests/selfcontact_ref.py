"""numpy float64 restatement of include/tcdiff_selfcontact.h, written from the header: loops over clips, dancers and frames; the 253
bone pairs of a frame are evaluated elementwise as arrays (every numpy operation rounds once, as the header's arithmetic does).  No
ballots, lanes or tiles, except that ``self_depth_mean`` follows the stated lane order.  Also ``self_pairs`` restated with plain
loops, seeded FK scenes for the GPU test, and the check that no decision the metric makes on them is a near-tie."""
import numpy as np

from group_ref import SMPL_PARENTS, capsule_radii, custom_skeleton, seg_dist

PAIRS = [(i, j) for i in range(1, 24) for j in range(i + 1, 24)]          # k = 0 .. 252, lexicographic
DEFAULTS = dict(radii=None, parents=None, mask=None, rest_joints=None, hops=2, rest_margin=0.05, tolerance=0.03)
MARGIN = 1e-9
FLOATS = ("self_contact_rate", "self_gap_min", "self_depth_mean", "gap")
INTS = ("self_contact_episodes", "self_closest", "self_pair_frames", "closest")
ORDER = ["self_contact_rate", "self_gap_min", "self_contact_episodes", "self_closest", "self_depth_mean", "self_pair_frames"]
# SMPL's rest offsets (joint relative to its parent, metres, y up), as the forward kinematics of the project uses them
OFFSETS = np.array([
    [0.0, 0.0, 0.0], [0.05858135, -0.08228004, -0.01766408], [-0.06030973, -0.09051332, -0.01354254],
    [0.00443945, 0.12440352, -0.03838522], [0.04345142, -0.38646945, 0.008037], [-0.04325663, -0.38368791, -0.00484304],
    [0.00448844, 0.1379564, 0.02682033], [-0.01479032, -0.42687458, -0.037428], [0.01905555, -0.4200455, -0.03456167],
    [-0.00226458, 0.05603239, 0.00285505], [0.04105436, -0.06028581, 0.12204243], [-0.03483987, -0.06210566, 0.13032329],
    [-0.0133902, 0.21163553, -0.03346758], [0.07170245, 0.11399969, -0.01889817], [-0.08295366, 0.11247234, -0.02370739],
    [0.01011321, 0.08893734, 0.05040987], [0.12292141, 0.04520509, -0.019046], [-0.11322832, 0.04685326, -0.00847207],
    [0.2553319, -0.01564902, -0.02294649], [-0.26012748, -0.01436928, -0.03126873], [0.26570925, 0.01269811, -0.00737473],
    [-0.26910836, 0.00679372, -0.00602676], [0.08669055, -0.01063603, -0.01559429], [-0.0887537, -0.00865157, -0.01010708]])


def rest_pose(parents=None):
    parents = SMPL_PARENTS if parents is None else parents
    J = np.zeros((24, 3))
    for j in range(1, 24):
        J[j] = J[parents[j]] + OFFSETS[j]
    return J


def pair_gaps(J, radii, parents):
    """the 253 gaps of one frame: J (24, 3) -> (253,) float64 in the order of PAIRS"""
    J = np.asarray(J).astype(np.float64)
    i, j = np.array(PAIRS).T
    par = np.asarray(parents)
    d = seg_dist(J[par[i]], J[i], J[par[j]], J[j])
    return (d - radii[i]) - radii[j]


def self_pairs(*, radii=None, parents=None, rest_joints=None, hops=2, rest_margin=0.05):
    """the default list, (253,) bool: plain loops.  Bones are neighbours if they share a joint; a pair is left out if its distance
    in the neighbour graph is <= hops or its rest-pose gap is < rest_margin"""
    radii = capsule_radii() if radii is None else np.asarray(radii, np.float64)
    parents = SMPL_PARENTS if parents is None else list(parents)
    rest = rest_pose(parents) if rest_joints is None else np.asarray(rest_joints, np.float64)
    near = np.zeros((24, 24), bool)
    for a in range(1, 24):
        for c in range(1, 24):
            if a != c and (parents[a] == parents[c] or parents[a] == c or parents[c] == a):
                near[a, c] = True
    dist = np.full((24, 24), 99)
    for a in range(1, 24):
        dist[a, a] = 0
    for a in range(1, 24):
        for c in range(1, 24):
            if near[a, c]:
                dist[a, c] = 1
    for m in range(1, 24):                                  # Floyd and Warshall
        for a in range(1, 24):
            for c in range(1, 24):
                if dist[a, m] + dist[m, c] < dist[a, c]:
                    dist[a, c] = dist[a, m] + dist[m, c]
    gaps = pair_gaps(rest, radii, parents)
    out = np.zeros(253, bool)
    for k, (i, j) in enumerate(PAIRS):
        out[k] = dist[i, j] > hops and not gaps[k] < rest_margin
    return out


def depth_sum(gap, contact):
    """the sum of -gap over the contact frames in the header's order: 64 lanes, lane l adds the frames l, l + 64, ...; a butterfly"""
    lanes = [0.0] * 64
    for t in range(len(gap)):
        if contact[t]:
            lanes[t % 64] = lanes[t % 64] + (-float(gap[t]))
    for o in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
    return lanes[0]


def self_contact(joints, *, radii=None, parents=None, mask=None, rest_joints=None, hops=2, rest_margin=0.05, tolerance=0.03, details=False):
    """joints (b, dn, T, 24, 3) float32 -> the dictionary of tcdiff_amd.self_contact.self_contact with return_frames, as numpy arrays;
    ``details`` adds what decisions_clear looks at"""
    joints = np.asarray(joints)
    assert joints.dtype == np.float32 and joints.shape[3:] == (24, 3)
    b, dn, T = joints.shape[:3]
    radii = capsule_radii() if radii is None else np.asarray(radii, np.float64)
    parents = SMPL_PARENTS if parents is None else list(parents)
    if mask is None:
        mask = self_pairs(radii=radii, parents=parents, rest_joints=rest_joints, hops=hops, rest_margin=rest_margin)
    mask = np.asarray(mask, bool)
    assert mask.shape == (253,) and mask.any()
    listed = np.flatnonzero(mask)
    codes = np.array([24 * i + j for i, j in PAIRS])
    out = {"self_contact_rate": np.zeros((b, dn)), "self_gap_min": np.zeros((b, dn)), "self_contact_episodes": np.zeros((b, dn), np.int64),
           "self_closest": np.zeros((b, dn, 3), np.int64), "self_depth_mean": np.zeros((b, dn)),
           "self_pair_frames": np.zeros((b, dn, 253), np.int64), "gap": np.zeros((b, dn, T)), "closest": np.zeros((b, dn, T), np.int32)}
    det = {"tolerance_lead": np.inf, "frame_lead": np.full((b, dn, T), np.inf), "dancer_lead": np.inf}
    for c in range(b):
        for d in range(dn):
            for t in range(T):
                g = pair_gaps(joints[c, d, t], radii, parents)[listed]
                nan = np.isnan(g)
                k = int(np.argmax(nan)) if nan.any() else int(np.argmin(g))          # both give the first such entry: the smallest code
                out["gap"][c, d, t], out["closest"][c, d, t] = g[k], codes[listed[k]]
                with np.errstate(invalid="ignore"):
                    pen = g < -tolerance
                out["self_pair_frames"][c, d, listed[pen]] += 1
                if (~nan).any():
                    det["tolerance_lead"] = min(det["tolerance_lead"], float(np.abs(g[~nan] + tolerance).min()))
                if not nan.any() and g.size > 1:
                    det["frame_lead"][c, d, t] = float(np.partition(g, 1)[1] - g[k])
            gap = out["gap"][c, d]
            with np.errstate(invalid="ignore"):
                con = gap < -tolerance
            n = int(con.sum())
            out["self_contact_rate"][c, d] = n / T
            out["self_contact_episodes"][c, d] = sum(1 for t in range(T) if con[t] and not (t > 0 and con[t - 1]))
            out["self_depth_mean"][c, d] = depth_sum(gap, con) / n if n else np.nan
            best_t = -1
            for t in range(T):
                if np.isfinite(gap[t]) and (best_t < 0 or gap[t] < gap[best_t]):
                    best_t = t
            if best_t < 0:
                out["self_gap_min"][c, d], out["self_closest"][c, d] = np.nan, (-1, -1, -1)
            else:
                code = int(out["closest"][c, d, best_t])
                out["self_gap_min"][c, d], out["self_closest"][c, d] = gap[best_t], (best_t, code // 24, code % 24)
                others = [gap[t] for t in range(T) if t != best_t and np.isfinite(gap[t])]
                if others:
                    det["dancer_lead"] = min(det["dancer_lead"], min(others) - gap[best_t])
    if details:
        out["details"] = det
    return out


def judge(ref):
    """(ok, reasons) from a self_contact(..., details=True) result; see decisions_clear"""
    det = ref["details"]
    why = []
    if det["tolerance_lead"] <= MARGIN:
        why.append(f"a listed gap within {det['tolerance_lead']:.3e} of the tolerance")
    if det["frame_lead"].min() <= MARGIN:
        why.append(f"a frame's smallest gap leads by {det['frame_lead'].min():.3e}")
    if det["dancer_lead"] <= MARGIN:
        why.append(f"a dancer's smallest gap leads by {det['dancer_lead']:.3e}")
    return not why, why


def decisions_clear(joints, **kw):
    """No comparison the metric makes is a near-tie on these inputs, so an implementation that rounds differently in the last places
    still makes every decision the same way: every listed |gap_k + tolerance| above 1e-9; the smallest gap of a frame ahead of its
    runner-up by more than 1e-9; the smallest gap of a dancer over the frames ahead by more than 1e-9.  Returns (ok, reasons)."""
    return judge(self_contact(joints, details=True, **kw))


# ---- bodies that can be checked by hand ------------------------------------------------------------------------------------------------
CHAIN = [-1] + list(range(23))                              # a chain skeleton: bone i runs from joint i - 1 to joint i


def chain_body(T=1):
    """joints 0 .. 23 of a chain laid out far apart along x on dyadic coordinates (joint j at x = 4 j): no two bones near each other
    but the neighbours, which touch at their joint"""
    J = np.zeros((T, 24, 3), np.float32)
    J[:, :, 0] = 4.0 * np.arange(24, dtype=np.float32)
    return J


def bars(a, b=None):
    """the chain folded into three parallel bars, one frame per entry of `a`: bone 1 (joints 0 -> 1) from (0,0,0) to (4,0,0); bone 3
    (joints 2 -> 3) folded back over it at height a, from (4,0,a) to (0,0,a); bone 5 (joints 4 -> 5) beside it at y = b, from (0,b,0)
    to (4,b,0).  For dyadic a and b, dist(bone 1, bone 3) = a and dist(bone 1, bone 5) = b to the bit.  b defaults to 64: far away"""
    a = np.atleast_1d(np.asarray(a, np.float32))
    b = np.full(a.shape, 64.0, np.float32) if b is None else np.atleast_1d(np.asarray(b, np.float32))
    T = a.shape[0]
    J = chain_body(T)
    J[:, 0], J[:, 1] = (0, 0, 0), (4, 0, 0)
    J[:, 2, 0], J[:, 2, 1], J[:, 2, 2] = 4.0, 0.0, a
    J[:, 3, 0], J[:, 3, 1], J[:, 3, 2] = 0.0, 0.0, a
    J[:, 4, 0], J[:, 4, 1], J[:, 4, 2] = 0.0, b, 0.0
    J[:, 5, 0], J[:, 5, 1], J[:, 5, 2] = 4.0, b, 0.0
    J[:, 6:] += np.float32(1000.0)
    return J


def pair_mask(pairs):
    m = np.zeros(253, bool)
    for i, j in pairs:
        m[PAIRS.index((min(i, j), max(i, j)))] = True
    return m


def tie_body(T=2):
    """the exact tie: bones 1 (joints 0 -> 1) and 2 (joints 1 -> 2) of the chain meet at joint 1 = (0, 0, 0), bone 1 along -x and
    bone 2 along -y; bone 5 (joints 4 -> 5) is the segment (1, 1, 1) -> (1, 1, 3), whose nearest point to both is (1, 1, 1) and
    theirs the shared joint: both distances are sqrt(3) to the bit.  Every frame alike"""
    J = chain_body(T)
    J[:, 0], J[:, 1], J[:, 2] = (-2, 0, 0), (0, 0, 0), (0, -2, 0)
    J[:, 3] = (64, 64, 64)
    J[:, 4], J[:, 5] = (1, 1, 1), (1, 1, 3)
    J[:, 6:] += np.float32(100.0)
    return J


# ---- seeded scenes -----------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1), (1, 2, 3), (2, 3, 5), (1, 1, 70), (2, 3, 150), (1, 2, 300)]
SEEDS = {(1, 1, 1): 0, (1, 2, 3): 0, (2, 3, 5): 0, (1, 1, 70): 0, (2, 3, 150): 0, (1, 2, 300): 0}
DEFAULT_RADII_SCENE = ((2, 3, 150), 7)                      # the shape and seed of the scene that is run with radii=None
_cache = {}


def rodrigues(v):
    """axis-angle (..., 3) -> rotation matrices (..., 3, 3)"""
    th = np.linalg.norm(v, axis=-1)[..., None, None]
    k = v / np.maximum(th[..., 0], 1e-12)
    K = np.zeros(v.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def fk(rot, root, parents=None):
    """local axis-angle rotations (T, 24, 3) and root positions (T, 3) -> joints (T, 24, 3): SMPL's offsets down the tree"""
    parents = SMPL_PARENTS if parents is None else parents
    R = rodrigues(rot)
    G = [R[:, 0]]
    J = [root]
    for j in range(1, 24):
        p = parents[j]
        J.append(J[p] + np.einsum("tab,b->ta", G[p], OFFSETS[j]))
        G.append(G[p] @ R[:, j])
    return np.stack(J, 1)


def synth(b, dn, T, seed=None, parents=None):
    """Seeded FK poses at metre scale, (b, dn, T, 24, 3) float32, y up: SMPL's offsets, smooth seeded joint rotations about a pose
    with the arms lowered, lively enough that a forearm or a hand passes through the trunk, the head or a thigh now and then.  With
    three or more dancers the last one of a clip moves little: it never touches itself.  Cached; treat as read-only."""
    seed = SEEDS.get((b, dn, T), 0) if seed is None else seed
    key = (b, dn, T, seed, None if parents is None else tuple(parents))
    if key in _cache:
        return _cache[key]
    g = np.random.default_rng([seed, b, dn, T])
    sec = (np.arange(T, dtype=np.float64) + g.uniform(0, 100)).reshape(T, 1, 1) / 30.0
    out = np.zeros((b, dn, T, 24, 3))
    for c in range(b):
        for d in range(dn):
            calm = dn >= 3 and d == dn - 1
            amp = np.full((24, 1), 0.05 if calm else 0.35)
            if not calm:
                amp[[16, 17, 18, 19]] = 0.9               # shoulders and elbows swing widely
                amp[[1, 2, 4, 5]] = 0.5                   # hips and knees
            k = 3
            f, ph = g.uniform(0.2, 1.2, (k, 1, 24, 3)), g.uniform(0, 2 * np.pi, (k, 1, 24, 3))
            rot = (g.uniform(0.3, 1.0, (k, 1, 24, 3)) * amp / k * np.sin(2 * np.pi * f * sec[None] + ph)).sum(0) * 1.7
            rot[:, 16, 2] -= 1.2                          # the arms lowered: the left one about -z, the right one about +z
            rot[:, 17, 2] += 1.2
            root = np.array([1.5 * d, 0.95, 1.0 * c]) + 0.2 * np.sin(2 * np.pi * 0.3 * sec[:, 0] + g.uniform(0, 6, 3))
            out[c, d] = fk(rot, root, parents)
    _cache[key] = np.ascontiguousarray(out.astype(np.float32))
    _cache[key].setflags(write=False)
    return _cache[key]


def scene_radii(seed=0):
    """the default radii plus a seeded offset within 4 mm per bone: with EQUAL radii on bones that share a joint (the three spine
    bones, the two hips) a limb whose nearest point is that joint gives two gaps equal to the last bit, and the comparison on the
    seeded scenes wants every minimum to lead by a margin; the exact tie is a hand-made case of its own"""
    g = np.random.default_rng([seed, 253])
    r = capsule_radii()
    r[1:] += g.uniform(-0.004, 0.004, 23)
    return r


def parameter_cases():
    """(shape, seed, keyword arguments) of the GPU test's runs with other parameters; tests/test_selfcontact_cpu.py holds each to
    decisions_clear"""
    parents, radii = custom_skeleton()
    shape = (1, 2, 70)
    return [(shape, 0, dict(radii=radii, parents=parents)), (shape, 0, dict(radii=scene_radii(), tolerance=0.0)),
            (shape, 0, dict(radii=scene_radii(), mask=pair_mask([(20, 3), (21, 9), (22, 15)]))),
            (shape, 0, dict(radii=scene_radii(), hops=0, rest_margin=0.0))]
