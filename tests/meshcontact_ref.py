"""numpy float64 restatement of mesh-level contact, written from the definition in include/tcdiff_meshcontact.h (not from
csrc/meshcontact.hip), and the seeded meshes and scenes the CPU and GPU tests share.  Inputs are float32 arrays, promoted to float64
before the first operation; every product, quotient, difference and sum is in the header's order.  There are no boxes, no tiles and no
candidates: every vertex is tested against every face.  The restatement also reports how close every decision it made came to its
boundary (``margins``): |p.x - xe| of every straddling edge, |z_hit - p.z| of every covering face, the lead of the deepest vertex over
the runner-up; ``decisions_clear`` holds them to 1e-9."""
import functools

import numpy as np

CLEAR = 1e-9
METRICS = ("mesh_contact_rate", "mesh_contact_episodes", "mesh_depth_max", "mesh_deepest", "mesh_inside_mean")


# ---- seeded meshes ----------------------------------------------------------------------------------------------------------
def closed_lattice(nu=10, nv=7, seed=None, centre=(0.0, 0.0, 1.0), radius=0.55):
    """shade_ref.lattice's rings -- nv rings of nu vertices between latitudes -+ 70 degrees -- plus the two pole vertices (south
    nu nv, north nu nv + 1) and their fans, every face wound outward: V = nu nv + 2, F = 2 nu nv, closed.  ``seed``: perturb every
    vertex by up to 6 % of the radius.  -> (vertices (V, 3) float32 in metres, z up, centred on ``centre``; faces int32)"""
    lat = np.deg2rad(np.linspace(-70.0, 70.0, nv))
    lon = 2 * np.pi * np.arange(nu) / nu
    v = np.stack([np.cos(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.sin(lon)[None],
                  np.sin(lat)[:, None] * np.ones(nu)[None]], -1).reshape(-1, 3)
    v = np.concatenate([v, [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0]]]) * radius
    if seed is not None:
        v = v + np.random.default_rng([43, seed]).uniform(-0.06, 0.06, v.shape) * radius
    south, north, top = nu * nv, nu * nv + 1, (nv - 1) * nu
    faces = []
    for r in range(nv - 1):
        for k in range(nu):
            a, b, c, d = r * nu + k, r * nu + (k + 1) % nu, (r + 1) * nu + (k + 1) % nu, (r + 1) * nu + k
            faces += [(a, b, c), (a, c, d)]
    for k in range(nu):
        faces += [((k + 1) % nu, k, south), (top + k, top + (k + 1) % nu, north)]
    return (v + np.asarray(centre, np.float64)).astype(np.float32), np.asarray(faces, np.int32)


def box_mesh(n=2):
    """the unit cube [0, 1]^3, every side n x n quads of two triangles, wound outward; with n a power of two every coordinate is
    dyadic.  -> (vertices (6 n^2 + 2, 3) float32, faces (12 n^2, 3) int32)"""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3                 # u x w = +axis
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    def at(di, dj):
                        p = [0, 0, 0]
                        p[axis], p[u], p[w] = side, i + di, j + dj
                        return vid(tuple(p))
                    q = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]          # counter-clockwise seen from +axis
                    if side == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return (np.asarray(verts, np.float64) / n).astype(np.float32), np.asarray(faces, np.int32)


def closed(faces):
    """every directed edge once, its reverse once: a search, not the package's sort"""
    seen = {}
    for f in np.asarray(faces).tolist():
        for i, j in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0])):
            seen[(i, j)] = seen.get((i, j), 0) + 1
    return all(n == 1 and i != j and seen.get((j, i), 0) == 1 for (i, j), n in seen.items())


def pairs(dn):
    return [(a, b) for a in range(dn) for b in range(a + 1, dn)]


def axes(up):
    return (1 if up == 0 else 0), (1 if up == 2 else 2), up


# ---- steps 2 to 6 of the header: one set of points against one body -------------------------------------------------------------------
def _crossed(px, py, u, w):
    """points (n, 1) against the edges u -> w (1, F, 3): (crossed, straddles, |p.x - xe|)"""
    ux, uy, wx, wy = u[..., 0], u[..., 1], w[..., 0], w[..., 1]
    straddle = (uy > py) != (wy > py)
    with np.errstate(all="ignore"):
        xe = ux + ((py - uy) / (wy - uy)) * (wx - ux)
    return straddle & (px < xe), straddle, np.abs(px - xe)


def winding(points, body, faces, up=2):
    """points (n, 3) and body (V, 3) float32 -> w (n,) int64 and the margins (edge, height) of the decisions"""
    ax, ay, az = axes(up)
    P = np.asarray(points, np.float32).astype(np.float64)[:, [ax, ay, az]]
    X = np.asarray(body, np.float32).astype(np.float64)[:, [ax, ay, az]]
    faces = np.asarray(faces, np.int64)
    px, py, pz = P[:, None, 0], P[:, None, 1], P[:, None, 2]
    crossings = np.zeros((P.shape[0], faces.shape[0]), np.int64)
    edge_margin = np.inf
    for i, j in ((0, 1), (1, 2), (2, 0)):
        lo, hi = np.minimum(faces[:, i], faces[:, j]), np.maximum(faces[:, i], faces[:, j])          # always from the lower index
        cr, straddle, gap = _crossed(px, py, X[lo][None], X[hi][None])
        cr &= (lo != hi)[None]
        straddle &= (lo != hi)[None]
        crossings += cr
        if straddle.any():
            edge_margin = min(edge_margin, float(gap[straddle].min()))
    cover = (crossings & 1) == 1
    A, B, C = X[faces[:, 0]][None], X[faces[:, 1]][None], X[faces[:, 2]][None]
    bx, by, cx, cy = B[..., 0] - A[..., 0], B[..., 1] - A[..., 1], C[..., 0] - A[..., 0], C[..., 1] - A[..., 1]
    qx, qy = px - A[..., 0], py - A[..., 1]
    D = bx * cy - by * cx
    with np.errstate(all="ignore"):
        l1 = (qx * cy - qy * cx) / D
        l2 = (bx * qy - by * qx) / D
        z_hit = (A[..., 2] + l1 * (B[..., 2] - A[..., 2])) + l2 * (C[..., 2] - A[..., 2])
    counted = cover & (D != 0.0)
    height_margin = float(np.abs(z_hit - pz)[counted].min()) if counted.any() else np.inf
    with np.errstate(invalid="ignore"):
        above = counted & (z_hit > pz)
    w = np.where(above, np.where(D > 0.0, 1, -1), 0).sum(1)
    return w, (edge_margin, height_margin)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def distances(points, body, faces, up=2):
    """points (n, 3) -> (n, F) float64: the distance of each to every triangle, Ericson's regions in the header's order"""
    ax, ay, az = axes(up)
    p = np.asarray(points, np.float32).astype(np.float64)[:, None, [ax, ay, az]]
    X = np.asarray(body, np.float32).astype(np.float64)[:, [ax, ay, az]]
    faces = np.asarray(faces, np.int64)
    A, B, C = X[faces[:, 0]][None], X[faces[:, 1]][None], X[faces[:, 2]][None]
    ab, ac, ap, bp, cp = B - A, C - A, p - A, p - B, p - C
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va, g, h = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4, d4 - d3, d5 - d6
    with np.errstate(all="ignore"):
        s = (va + vb) + vc
        choices = [A,
                   B,
                   A + (d1 / (d1 - d3))[..., None] * ab,
                   C,
                   A + (d2 / (d2 - d6))[..., None] * ac,
                   B + (g / (g + h))[..., None] * (C - B)]
        inner = (A + (vb / s)[..., None] * ab) + (vc / s)[..., None] * ac
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (g >= 0) & (h >= 0)]
    q = inner
    for cond, choice in zip(conds[::-1], choices[::-1]):          # the first region that applies wins: apply them last to first
        q = np.where(cond[..., None], np.broadcast_to(choice, q.shape), q)
    e = p - q
    with np.errstate(invalid="ignore"):
        return np.sqrt(_dot(e, e))


def inside_of(points, body, faces, up=2):
    """-> (inside (n,) bool, depth (n,) float64 with NaN for the vertices outside, (edge margin, height margin))"""
    w, margins = winding(points, body, faces, up)
    inside = w != 0
    depth = np.full(len(w), np.nan)
    if inside.any():
        which = np.flatnonzero(inside)
        for lo in range(0, len(which), 128):                  # in slices, for the memory's sake
            d = distances(np.asarray(points)[which[lo:lo + 128]], body, faces, up)
            depth[which[lo:lo + 128]] = np.where(np.isnan(d), np.inf, d).min(1)          # a NaN takes no part in the minimum
    return inside, depth, margins


# ---- steps 1, 7 and 8: frames, pairs, clips ---------------------------------------------------------------------------------------------
def mesh_contact(vertices, faces, dn, up=2):
    """vertices (b, T dn, V, 3) float32, faces (F, 3) -> the outputs of tcm_mesh_contact as numpy arrays under the package's names, the
    frame planes ``inside`` (b, P, T, 2) int32 and ``depth`` (b, P, T), and ``margins`` = (edge, height, lead)"""
    vertices = np.asarray(vertices, np.float32)
    b, rows, V = vertices.shape[:3]
    assert rows % dn == 0
    T, pr = rows // dn, pairs(dn)
    P = len(pr)
    out = {"mesh_contact_rate": np.full((b, P), np.nan), "mesh_contact_episodes": np.zeros((b, P), np.int64),
           "mesh_depth_max": np.zeros((b, P)), "mesh_deepest": np.full((b, P, 3), -1, np.int64), "mesh_inside_mean": np.full((b, P), np.nan),
           "inside": np.zeros((b, P, T, 2), np.int32), "depth": np.zeros((b, P, T))}
    edge_m = height_m = lead_m = np.inf
    for c in range(b):
        finite = np.isfinite(vertices[c]).all((1, 2)).reshape(T, dn)
        for k, (a, bb) in enumerate(pr):
            valid = contact = episodes = total = 0
            was = False
            ranked = []                                       # (-depth, frame, dancer, vertex) of every inside vertex: the total order
            for t in range(T):
                if not (finite[t, a] and finite[t, bb]):
                    out["inside"][c, k, t], out["depth"][c, k, t], was = -1, np.nan, False
                    continue
                valid += 1
                frame = []
                for direction, (src, dst) in enumerate(((a, bb), (bb, a))):
                    ins, dep, (em, hm) = inside_of(vertices[c, t * dn + src], vertices[c, t * dn + dst], faces, up)
                    edge_m, height_m = min(edge_m, em), min(height_m, hm)
                    out["inside"][c, k, t, direction] = ins.sum()
                    frame += [(-dep[v], t, src, int(v)) for v in np.flatnonzero(ins)]
                total += len(frame)
                now = len(frame) > 0
                contact += now
                episodes += now and not was
                was = now
                out["depth"][c, k, t] = -min(frame)[0] if frame else 0.0
                ranked += frame
            out["mesh_contact_episodes"][c, k] = episodes
            if valid:
                out["mesh_contact_rate"][c, k] = float(contact) / float(valid)
                out["mesh_inside_mean"][c, k] = float(total) / float(valid)
            if ranked:
                ranked.sort()
                out["mesh_depth_max"][c, k], out["mesh_deepest"][c, k] = -ranked[0][0], ranked[0][1:]
                if len(ranked) > 1:
                    lead_m = min(lead_m, ranked[1][0] - ranked[0][0])
    out["margins"] = (edge_m, height_m, lead_m)
    return out


def decisions_clear(out):
    """-> (ok, why): is every decision of a ``mesh_contact`` result at least CLEAR from its boundary"""
    why = [f"{name} margin {m:.3e} < {CLEAR}" for name, m in zip(("edge", "height", "lead"), out["margins"]) if not m >= CLEAR]
    return not why, why


# ---- seeded scenes --------------------------------------------------------------------------------------------------------------------
def _balls(nu, nv, centres, radii=None, seed=0):
    """centres (b, T, dn, 3) -> vertices (b, T dn, V, 3) float32: every pose a closed lattice of its own seed around its centre"""
    centres = np.asarray(centres, np.float64)
    b, T, dn = centres.shape[:3]
    faces = closed_lattice(nu, nv)[1]
    radii = [0.55] * dn if radii is None else radii
    v = np.stack([np.stack([closed_lattice(nu, nv, seed + 1000 * c + 10 * t + d, centres[c, t, d], radii[d])[0]
                            for t in range(T) for d in range(dn)]) for c in range(b)])
    return v, faces


def _line(b, T, dn, gap, speed=0.0, phase=0.0, fold=False):
    """dancers in a row along x, `gap` apart, dancer d drawn to the middle by speed (d - (dn - 1) / 2) a frame (``fold``: there and
    back, frame t counting as |t mod 6 - 3|); in clip c dancer d stands phase c d further along"""
    c, t, d = np.meshgrid(np.arange(b), np.arange(T), np.arange(dn), indexing="ij")
    if fold:
        t = np.abs(t % 6 - 3)
    x = d * gap - (d - (dn - 1) / 2) * speed * t + phase * c * d
    return np.stack([x, 0.1 * d + 0.0 * x, 1.0 + 0.05 * d + 0.0 * x], -1)


def _build(name):
    if name == "small":                                       # less than one chunk of vertices and one tile of faces
        return _balls(10, 7, _line(2, 5, 3, 0.9, 0.05, 0.03), seed=1) + (3,)
    if name == "ragged":                                      # V = 301: two chunks, the second ragged; F = 598: two tiles, ragged
        return _balls(23, 13, _line(1, 2, 2, 0.9, 0.1), seed=2) + (2,)
    if name == "ontop":                                       # V = 1149 > one batch of candidates; the smaller ball wholly inside
        return _balls(37, 31, _line(1, 1, 2, 0.03), radii=[0.3, 0.55], seed=3) + (2,)
    if name == "single":                                      # dn = 2, T = 1
        return _balls(10, 7, _line(1, 1, 2, 0.8), seed=4) + (2,)
    if name == "alone":                                       # dn = 1: no pair
        return _balls(10, 7, _line(2, 3, 1, 0.0), seed=5) + (1,)
    if name == "disjoint":
        return _balls(10, 7, _line(1, 2, 3, 2.5), seed=6) + (3,)
    if name == "near":                                        # the boxes overlap, nothing is inside: a diagonal offset
        centres = _line(1, 2, 2, 0.0)
        centres[:, :, 1, :2] += 0.86
        return _balls(10, 7, centres, seed=7) + (2,)
    if name == "motion":                                      # dancers that pass through each other: episodes, rate and arg-max move
        return _balls(10, 7, _line(2, 12, 3, 1.3, 0.2, 0.04, fold=True), seed=8) + (3,)
    raise KeyError(name)


CASES = ("small", "ragged", "ontop", "single", "alone", "disjoint", "near", "motion")


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> (vertices (b, T dn, V, 3) float32, faces (F, 3) int32, dn), read-only"""
    v, f, dn = _build(name)
    v.setflags(write=False)
    f.setflags(write=False)
    return v, f, dn


@functools.lru_cache(maxsize=None)
def reference(name, up=2):
    """the restatement's result on a seeded scene, computed once and shared; read-only"""
    v, f, dn = scene(name)
    out = mesh_contact(v, f, dn, up)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def with_nan(name, clip, frame, dancer, vertex=0):
    """a copy of a scene with one non-finite word"""
    v, f, dn = scene(name)
    v = np.array(v)
    v[clip, frame * dn + dancer, vertex, 1] = np.nan
    return v, f, dn
