"""numpy float64 restatement of the shaded mesh frames of tcr_mesh_vertices / tcr_mesh_raster, written from the picture's
definition in include/tcdiff_shade.h (not from csrc/shade.hip), and the seeded meshes the CPU and GPU tests share.  Inputs are
float32 arrays, promoted to float64 before the first operation; every product, difference and sum is in the header's order.  The
raster has no tiles and no chunks: every triangle is evaluated at every pixel."""
import numpy as np

U32 = 2.0 ** -24
U64 = 2.0 ** -53
MAX_COORD = 4096.0           # the margins' derivation (test_shade_gpu.py) is for screen coordinates below this
PALETTE = ((0xE3, 0xBA, 0x8F), (0xFF, 0x6B, 0x6B), (0x0A, 0xBD, 0xE3), (0x57, 0x65, 0x74), (0x01, 0xA3, 0xA4))
STYLE = dict(background=(255, 255, 255), ambient=0.35, light=(0.0, -0.8, 0.6))


# ---- seeded meshes ----------------------------------------------------------------------------------------------------------
def lattice(nu=10, nv=7, seed=None, cx=0.0, radius=0.55, cz=1.0):
    """A sphere-like lattice, closed around: nv rings of nu vertices between latitudes -+ 70 degrees, every vertex shared by its
    quads' triangles (2 nu (nv - 1) faces, wound so that face normals point outward).  ``seed``: perturb every vertex by up to 6 %
    of the radius (None: the exact lattice).  -> (vertices (nu nv, 3) float32 in metres, z up, centred on (cx, 0, cz); faces int32)"""
    lat = np.deg2rad(np.linspace(-70.0, 70.0, nv))
    lon = 2 * np.pi * np.arange(nu) / nu
    v = np.stack([np.cos(lat)[:, None] * np.cos(lon)[None], np.cos(lat)[:, None] * np.sin(lon)[None],
                  np.sin(lat)[:, None] * np.ones(nu)[None]], -1).reshape(-1, 3) * radius
    if seed is not None:
        v = v + np.random.default_rng([41, seed]).uniform(-0.06, 0.06, v.shape) * radius
    faces = []
    for r in range(nv - 1):
        for k in range(nu):
            a, b, c, d = r * nu + k, r * nu + (k + 1) % nu, (r + 1) * nu + (k + 1) % nu, (r + 1) * nu + k
            faces += [(a, b, c), (a, c, d)]
    return (v + np.array([cx, 0.0, cz])).astype(np.float32), np.asarray(faces, np.int32)


def adjacency(faces, V):
    """CSR (start (V + 1,), listed (3F,)): under each vertex the faces that name it, ascending, once per mention; a search"""
    start, listed = [0], []
    for v in range(V):
        for f, tri in enumerate(np.asarray(faces)):
            listed += [f] * int((tri == v).sum())
        start.append(len(listed))
    return np.asarray(start, np.int32), np.asarray(listed, np.int32)


def normals(vertices, faces, adj):
    """vertices (P, V, 3) float32 -> the unrounded float64 vertex normals (P, V, 3): the sum of e1 x e2 over the listed faces in
    the listed order from zero, divided by its length; zero where the length is zero"""
    assert vertices.dtype == np.float32
    X = vertices.astype(np.float64)
    start, listed = adj
    out = np.zeros_like(X)
    for v in range(X.shape[1]):
        s = np.zeros((X.shape[0], 3))
        for f in listed[start[v]:start[v + 1]]:
            i0, i1, i2 = faces[f]
            e1, e2 = X[:, i1] - X[:, i0], X[:, i2] - X[:, i0]
            s[:, 0] += e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
            s[:, 1] += e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
            s[:, 2] += e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        n = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, v] = np.where(n[:, None] == 0, 0.0, s / n[:, None])
    return out


def project(vertices, view):
    """-> (screen (P, V, 3) float64 exact to float64's rounding, the bound 4 * 2^-24 * sum |terms| of a float32 evaluation)"""
    X, m = np.asarray(vertices, np.float64), np.asarray(view, np.float64)
    terms = X[..., None, :] * m[:, :3]
    return terms.sum(-1) + m[:, 3], 4 * U32 * (np.abs(terms).sum(-1) + np.abs(m[:, 3]))


# ---- the picture ------------------------------------------------------------------------------------------------------------
def raster(screen, normal, faces, W, H, colors=PALETTE, style=None, under=None):
    """One frame.  screen, normal (dn, V, 3) float32; faces (F, 3).  Returns a dict:
      values (H, W, 3)   the unrounded channel values (colour * k; under's or the background's bytes where nothing covers)
      winner (H, W)      the visible triangle g = d F + f, or -1
      cand_k (G, H, W)   per triangle the factor k it would shade the pixel with, NaN outside its bounding box grown by one pixel
      edge (H, W)        the smallest distance in pixels from the centre to an edge line (edges of zero length excepted) of any
                         triangle whose grown box holds the pixel; inf where there is none
      zgap (H, W)        the depth gap between the two nearest covering triangles; inf with fewer than two
      level (H, W)       the winner's smallest distance of a channel from a rounding boundary (x.5); inf where nothing covers
      nhat (H, W)        the length of the winner's interpolated normal, sum w_i n_i with weights of sum 1; 1 where nothing covers
      boxed (H, W)       whether any triangle's grown box holds the pixel
      ratio              the largest (longest box side + 1) / (smallest altitude) of a triangle that can cover a clear pixel"""
    assert screen.dtype == np.float32 and normal.dtype == np.float32
    st = dict(STYLE, **(style or {}))
    amb = np.float64(np.float32(st["ambient"]))
    light = np.asarray(st["light"], np.float32).astype(np.float64)
    S, N = screen.astype(np.float64), normal.astype(np.float64)
    dn, V = S.shape[:2]
    F = len(faces)
    PY, PX = np.meshgrid(np.arange(H) + 0.5, np.arange(W) + 0.5, indexing="ij")
    best_z = np.full((H, W), np.inf)
    second_z = np.full((H, W), np.inf)
    winner = np.full((H, W), -1, np.int64)
    best_k = np.zeros((H, W))
    nhat = np.ones((H, W))
    edge = np.full((H, W), np.inf)
    boxed = np.zeros((H, W), bool)
    cand_k = np.full((dn * F, H, W), np.nan)
    ratio = 0.0
    for g in range(dn * F):
        d, f = divmod(g, F)
        idx = np.asarray(faces[f], np.int64)
        if (idx < 0).any() or (idx >= V).any():
            continue
        a, b, c = S[d, idx]
        if not np.isfinite(S[d, idx]).all():
            continue
        xs, ys = S[d, idx, 0], S[d, idx, 1]
        grown = (PX >= xs.min() - 1) & (PX <= xs.max() + 1) & (PY >= ys.min() - 1) & (PY <= ys.max() + 1)
        if not grown.any():
            continue
        inbox = (PX >= xs.min()) & (PX <= xs.max()) & (PY >= ys.min()) & (PY <= ys.max())
        E, lens = [], []
        with np.errstate(all="ignore"):
            for p, q in ((a, b), (b, c), (c, a)):
                dx, dy = q[0] - p[0], q[1] - p[1]
                E.append(dx * (PY - p[1]) - dy * (PX - p[0]))
                lens.append(np.hypot(dx, dy))
            area = (E[0] + E[1]) + E[2]
            for Ei, ln in zip(E, lens):
                if ln > 0:
                    edge = np.where(grown, np.minimum(edge, np.abs(Ei) / ln), edge)
            if min(lens) > 0:
                twice = abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]))
                alt = twice / max(lens)
                if alt > 0:
                    ratio = max(ratio, (max(xs.max() - xs.min(), ys.max() - ys.min()) + 1) / alt)
            covers = (area != 0) & inbox & (((E[0] >= 0) & (E[1] >= 0) & (E[2] >= 0)) | ((E[0] <= 0) & (E[1] <= 0) & (E[2] <= 0)))
            z = ((E[1] * a[2] + E[2] * b[2]) + E[0] * c[2]) / area
            na, nb, nc = N[d, idx]
            n = [(E[1] * na[k] + E[2] * nb[k]) + E[0] * nc[k] for k in range(3)]
            dot = (n[0] * light[0] + n[1] * light[1]) + n[2] * light[2]
            ln = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            k = amb + (1.0 - amb) * (np.abs(dot) / ln)
            k = np.where((ln == 0) | np.isnan(k), amb, k)
            unit = ln / np.abs(area)
        boxed |= grown
        cand_k[g] = np.where(grown, k, np.nan)
        zc = np.where(covers, z, np.inf)
        wins = covers & (zc < best_z)                         # ascending g: an equal depth does not displace the lower g
        second_z = np.where(wins, best_z, np.minimum(second_z, zc))
        best_z = np.where(wins, zc, best_z)
        winner = np.where(wins, g, winner)
        best_k = np.where(wins, k, best_k)
        nhat = np.where(wins, unit, nhat)
    colors = np.asarray(colors, np.float64)
    base = np.empty((H, W, 3))
    base[:] = np.asarray(st["background"], np.float64) if under is None else np.asarray(under, np.float64)
    col = colors[(np.maximum(winner, 0) // F) % len(colors)]
    values = np.where((winner >= 0)[..., None], col * best_k[..., None], base)
    frac = values - np.floor(values)
    level = np.where(winner >= 0, np.abs(frac - 0.5).min(-1), np.inf)
    with np.errstate(invalid="ignore"):
        zgap = second_z - best_z                              # inf - inf where nothing covers: clear_mask reads it as inf
    return dict(values=values, winner=winner, cand_k=cand_k, edge=edge, zgap=zgap, level=level,
                nhat=np.nan_to_num(nhat, nan=0.0), boxed=boxed, ratio=ratio, base=base, colors=colors, F=F)


def to_bytes(values):
    return np.minimum(np.floor(values + 0.5), 255).astype(np.uint8)


def clear_mask(m, delta_edge, delta_z, delta_level):
    """pixels whose every decision is clear of a tie: delta_edge pixels from every edge line near them, delta_z between the two
    nearest covering depths, delta_level (for a unit interpolated normal; divided by the normal's length) from a rounding boundary"""
    with np.errstate(invalid="ignore"):
        zgap = np.where(np.isinf(m["zgap"]) | np.isnan(m["zgap"]), np.inf, m["zgap"])
        return (m["edge"] >= delta_edge) & (zgap >= delta_z) & (m["level"] * m["nhat"] >= delta_level)


def deltas(m, zmax):
    """(delta_edge, delta_z, delta_level) of one raster case, by the rounding count in test_shade_gpu.py's docstring; from the
    inputs and the restatement alone"""
    delta_edge = 1e-10
    r = min(m["ratio"], (2 * MAX_COORD + 1) / delta_edge)
    return delta_edge, 200 * U64 * max(zmax, 1.0) * max(r, 1.0), 255 * 2 * (48 * U64 * max(r, 1.0) + 20 * U64)


def check(got, m, d, what=""):
    """got (H, W, 3) uint8 against one frame of the restatement under the deltas d: every clear pixel equal; every other pixel the
    uncovered value or within one level of one of the restatement's candidates there.  Returns (pixels not clear, pixels that differ)."""
    want = to_bytes(m["values"])
    clear = clear_mask(m, *d)
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64)).max(-1)
    assert got.shape == want.shape and (diff[clear] == 0).all(), (what, "clear pixels differ", int((diff[clear] > 0).sum()))
    for y, x in zip(*np.nonzero(~clear & (diff > 0))):
        if np.array_equal(got[y, x], to_bytes(m["base"][y, x])):
            continue
        ks = m["cand_k"][:, y, x]
        ok = False
        for g in np.flatnonzero(~np.isnan(ks)):
            cand = m["colors"][(g // m["F"]) % len(m["colors"])] * ks[g]
            ok = ok or np.abs(got[y, x].astype(np.float64) - np.floor(cand + 0.5)).max() <= 1
        assert ok, (what, "a pixel that is not clear shows no candidate", int(y), int(x), got[y, x].tolist())
    return int((~clear).sum()), int((diff > 0).sum())


def clear_share(m, d):
    """the share of clear pixels among those inside any triangle's grown box (1.0 when there are none)"""
    n = int(m["boxed"].sum())
    return 1.0 if n == 0 else float((clear_mask(m, *d) & m["boxed"]).sum() / n)


# ---- the seeded scene of the raster tests -----------------------------------------------------------------------------------
_cache = {}


def camera(W, H, span=4.0, elev=40.0, azim=-90.0, center=(0.0, 0.0, 1.0)):
    import draw_ref
    return draw_ref.camera(W, H, elev=elev, azim=azim, center=center, span=span)


def scene(b=2, T=3, dn=3, nu=10, nv=7):
    """(vertices (b, T dn, V, 3) float32, faces): dn perturbed lattices per frame that drift through each other, row = frame * dn +
    dancer.  Cached; read-only."""
    key = (b, T, dn, nu, nv)
    if key not in _cache:
        rows = []
        faces = None
        for c in range(b):
            for t in range(T):
                for d in range(dn):
                    v, faces = lattice(nu, nv, seed=1 + d + 10 * c, cx=(d - (dn - 1) / 2) * (0.7 - 0.25 * t) + 0.1 * c)
                    v = v + np.float32([0.0, 0.35 * (d % 2) - 0.1 * t * (d - 1), 0.05 * t])
                    rows.append(v.astype(np.float32))
        out = np.stack(rows).reshape(b, T * dn, -1, 3)
        out.setflags(write=False)
        _cache[key] = (out, faces)
    return _cache[key]


def projected(W, H, span=4.0, **kw):
    """the scene through the restatement: (view, faces, screen32 (b, T dn, V, 3), normals32, screen64, bound, normals64)"""
    key = ("p", W, H, span, tuple(sorted(kw.items())))
    if key not in _cache:
        verts, faces = scene(**kw)
        view = camera(W, H, span)
        b, n, V, _ = verts.shape
        s64, bound = project(verts.reshape(b * n, V, 3), view)
        n64 = normals(verts.reshape(b * n, V, 3), faces, adjacency(faces, V))
        shape = (b, n, V, 3)
        _cache[key] = (view, faces, s64.astype(np.float32).reshape(shape), n64.astype(np.float32).reshape(shape), s64.reshape(shape),
                       bound.reshape(shape), n64.reshape(shape))
    return _cache[key]


# ---- the raster cases the CPU and GPU tests share ------------------------------------------------------------------------------
CASES = ("33x17", "32x32", "100x76", "crowded", "wild", "one-dancer", "five-dancers", "equal-depth")
CROWD = 640                  # triangles in the crowded tile: more than twice the kernel's chunk of 256


def _unit(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def case(name):
    """-> dict(screen, normals (b, T dn, V, 3) float32, faces (F, 3) int32, b, T, dn, W, H, colors, style, under (b, T, H, W, 3) or
    None).  Cached; read-only."""
    key = ("case", name)
    if key in _cache:
        return _cache[key]
    g = np.random.default_rng([43, CASES.index(name)])
    colors, style, under = PALETTE, {}, None
    if name in ("33x17", "32x32", "100x76", "one-dancer", "five-dancers"):
        W, H = {"33x17": (33, 17), "32x32": (32, 32), "100x76": (100, 76)}.get(name, (33, 17))
        dn = {"one-dancer": 1, "five-dancers": 5}.get(name, 3)
        b, T = (2, 3) if dn == 3 else (1, 2)
        _, faces, screen, normal, _, _, _ = projected(W, H, 2.5, b=b, T=T, dn=dn)
        if name == "33x17":                                   # the picture below the bodies, and a page that is not white
            under = g.integers(0, 256, (b, T, H, W, 3)).astype(np.uint8)
        if name == "32x32":
            style = dict(background=(10, 20, 30), ambient=0.0, light=(0.6, 0.0, 0.8))
        if name == "five-dancers":
            colors = ((200, 100, 0), (10, 220, 130))          # two colours for five dancers: the palette wraps
    elif name == "crowded":
        # CROWD small triangles with vertices of their own, all inside the tile x, y in [32, 64) of a 70 x 66 image
        b, T, dn, W, H = 1, 1, 1, 70, 66
        centre = g.uniform(36.0, 60.0, (CROWD, 1, 2))
        xy = centre + g.uniform(-3.5, 3.5, (CROWD, 3, 2))
        z = g.uniform(-1.0, 1.0, (CROWD, 1, 1)) + g.uniform(-0.1, 0.1, (CROWD, 3, 1))
        screen = np.concatenate([xy, z], -1).reshape(1, 1, 3 * CROWD, 3).astype(np.float32)
        normal = _unit(g.standard_normal((1, 1, 3 * CROWD, 3)))
        faces = np.arange(3 * CROWD, dtype=np.int32).reshape(CROWD, 3)
    elif name == "wild":
        b, T, dn, W, H = 1, 1, 1, 40, 24
        nan, inf = np.nan, np.inf
        tris = [[(-300.0, -200.0, 2.0), (500.0, -150.0, 3.0), (10.0, 700.0, 2.5)],          # larger than the whole image
                [(-30.0, 3.0, 0.0), (-2.0, 9.0, 0.0), (-12.0, 20.0, 0.0)],                  # off the left edge
                [(41.0, 3.0, 0.0), (70.0, 9.0, 0.0), (52.0, 20.0, 0.0)],                    # off the right edge
                [(3.0, -30.0, 0.0), (20.0, -1.0, 0.0), (30.0, -12.0, 0.0)],                 # off the top
                [(3.0, 25.0, 0.0), (20.0, 60.0, 0.0), (30.0, 31.0, 0.0)],                   # off the bottom
                [(4.0, 4.25, 0.0), (10.0, 10.25, 0.0), (20.0, 20.25, 0.0)],                 # zero area: three points of one line
                [(5.0, 3.0, 0.0), (25.0, 8.0, 0.0), (nan, 15.0, 0.0)],                      # a NaN vertex
                [(5.0, 3.0, 0.0), (25.0, 8.0, 0.0), (12.0, inf, 0.0)],                      # an infinite vertex
                [(5.0, 3.0, 0.0), (25.0, 8.0, -inf), (12.0, 15.0, 0.0)],                    # an infinite depth
                [(-5.0, 3.0, 0.0), (-1.0, 20.0, 0.0), (-1e30, -1e30, 0.0)],                 # a vertex 1e30 away, off the left edge
                [(8.0, 5.0, 1.0), (30.0, 7.0, 1.0), (15.0, 21.0, 1.5)]]                     # and one ordinary triangle in front
        screen = np.asarray(tris, np.float32).reshape(1, 1, -1, 3)
        faces = np.arange(screen.shape[2], dtype=np.int32).reshape(-1, 3)
        faces = np.concatenate([faces, np.int32([[30, 31, 31]])])                           # a repeated index
        normal = _unit(g.standard_normal(screen.shape))
    else:
        assert name == "equal-depth"
        # two dancers with the same triangles: equal depth on every pixel, the lower g must show
        b, T, dn, W, H = 1, 1, 2, 20, 12
        tri = np.float32([[(2.25, 1.5, 0.3), (18.5, 3.25, 0.7), (7.75, 11.0, 0.1)], [(18.5, 3.25, 0.7), (19.5, 11.5, 0.2), (7.75, 11.0, 0.1)]])
        screen = np.broadcast_to(tri.reshape(1, 1, 6, 3), (1, 2, 6, 3)).copy()
        normal = _unit(g.standard_normal((1, 2, 6, 3)))
        faces = np.arange(6, dtype=np.int32).reshape(2, 3)
    out = dict(screen=np.ascontiguousarray(screen), normals=np.ascontiguousarray(normal), faces=np.ascontiguousarray(faces), b=b, T=T,
               dn=dn, W=W, H=H, colors=colors, style=style, under=under)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cache[key] = out
    return out


def frames_of(name):
    """the restatement of every frame of a case: [(clip, frame, raster dict, deltas)], cached"""
    key = ("frames", name)
    if key not in _cache:
        c = case(name)
        dn, out = c["dn"], []
        for clip in range(c["b"]):
            for t in range(c["T"]):
                rows = slice(t * dn, (t + 1) * dn)
                m = raster(c["screen"][clip, rows], c["normals"][clip, rows], c["faces"], c["W"], c["H"], c["colors"], c["style"],
                           None if c["under"] is None else c["under"][clip, t])
                z = c["screen"][clip, rows, :, 2]
                z = np.abs(z[np.isfinite(z)])
                d = deltas(m, float(z.max()) if z.size else 1.0)
                if name == "equal-depth":                     # the two depths of a pixel come from the same operations on the same
                    d = (d[0], 0.0, d[2])                     # values: equal bits, no rounding is involved, and the lower g shows
                out.append((clip, t, m, d))
        _cache[key] = out
    return _cache[key]
