"""csrc/skin.hip and tcdiff_amd/body.py on an MI355X against the numpy restatement tests/skin_ref.py, on seeded synthetic models.

The bound on a vertex coordinate is the rule of tests/test_music_gpu.py: 32 times the float32 restatement's own largest error
against the float64 restatement for that case, at least one float32 ulp of the case's largest coordinate; it is computed from the two
restatements on the CPU, never from the kernel's output.  The sizes sit around the kernel's own tile sizes, read from the header."""
import os

import numpy as np
import pytest
import torch

import gltf_ref as G
import skin_ref as S
from tcdiff_amd import _lib as L
from tcdiff_amd import body as B
from tcdiff_amd import export as E
from tcdiff_amd import gltf as X
from tcdiff_amd import io as tio
from tcdiff_amd import kernels as K
from tcdiff_amd.fk import SMPLSkeleton

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PT, VT = L.SKIN.constants["TC_SKIN_POSE_TILE"], L.SKIN.constants["TC_SKIN_VERT_TILE"]


def _splits(n):
    """clips x T x dn with the product n: 1 x n x 1 and, where it exists, a split with more than one clip and dancer"""
    out = [(1, n, 1)]
    for clips in (2, 3):
        for dn in (2, 3):
            if n % (clips * dn) == 0 and n > clips * dn:
                out.append((clips, n // (clips * dn), dn))
                return out
    return out


# 1 pose; one less than a tile, a tile, one more; and, since PT - 1 = 31 is a prime, the nearest counts with a (2, T, 3)-style split
SHAPES = [(1, 1, 1)] + [s for n in (PT - 2, PT - 1, PT, PT + 1, PT + 2) for s in _splits(n)]
VERTS = [1, VT - 1, VT, VT + 1, 2 * VT + 37]


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


@pytest.fixture(scope="module")
def models():
    cache = {}

    def get(V, Kw, seed=0, smpl_tree=False):
        key = (V, Kw, seed, smpl_tree)
        if key not in cache:
            m = S.make_model(V, Kw, seed=1000 * Kw + V + seed, smpl_tree=smpl_tree)
            cache[key] = (m, S.images(m), B.load_body_model(m, device=DEV))
        return cache[key]
    return get


@pytest.mark.parametrize("Kw", [1, 4, 8])
@pytest.mark.parametrize("V", VERTS)
def test_vertices_and_joints_against_the_restatement(models, V, Kw):
    _, im, body = models(V, Kw)
    skel = SMPLSkeleton(offsets=body.offsets, parents=body.parents)
    worst = {}
    for clips, T, dn in SHAPES:
        P = clips * T * dn
        poses, trans = S.poses_of(P)
        q, p = _dev(poses).reshape(clips, T * dn, 24, 3), _dev(trans).reshape(clips, T * dn, 3)
        for pose_blend in (True, False):
            for origin in ("pelvis", "smpl"):
                truth, own, bound = S.bound(im, poses, trans, pose_blend, origin)
                got, joints = B.skin(body, q, p, pose_blend=pose_blend, origin=origin, return_joints=True)
                assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (clips, T * dn, V, 3) and got.is_contiguous()
                assert tuple(joints.shape) == (clips, T * dn, 24, 3) and joints.dtype == torch.float32
                err = float(np.abs(got.cpu().numpy().reshape(P, V, 3).astype(np.float64) - truth).max())
                _, _, jt, _ = S.pose_part(im, poses, trans, origin)
                j_own = float(np.abs(jt.astype(np.float32).astype(np.float64) - jt).max())
                j_bound = max(32 * j_own, float(np.spacing(np.float32(np.abs(jt).max()))))
                j_err = float(np.abs(joints.cpu().numpy().reshape(P, 24, 3).astype(np.float64) - jt).max())
                key = (pose_blend, origin)
                worst[key] = max(worst.get(key, (0, 0, 0, 0)), (err / bound, err, own, j_err))
                assert err <= bound, (clips, T, dn, pose_blend, origin, err, own, bound)
                assert j_err <= j_bound, (clips, T, dn, origin, j_err, j_bound)
                if origin == "pelvis" and pose_blend:                     # code that exists already: the export's forward kinematics
                    fk = skel.forward(q, p)
                    scaled = float(((joints - fk).abs() / fk.abs().clamp(min=1)).max())
                    assert scaled <= 1e-5, (clips, T, dn, scaled)
    for (pose_blend, origin), (ratio, err, own, j_err) in sorted(worst.items()):
        print(f"V = {V}, K = {Kw}, pose_blend {pose_blend}, origin {origin}: largest vertex error {err:.3e} (the float32 restatement's own "
              f"{own:.3e}, {ratio:.3f} of the bound), joints {j_err:.3e}")


# ---- isolation ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [1, 3, 4])
def test_nothing_is_written_outside_out_and_joints(models, lead):
    """out and joints_out between guard floats, 4, 12 and 16 bytes into an allocation; every float inside is written"""
    V, Kw, P = VT + 1, 4, PT + 1
    _, im, body = models(V, Kw)
    poses, trans = S.poses_of(P)
    q, p = _dev(poses), _dev(trans)
    d = body.images(DEV)
    guard = np.float32(-1234.5)
    n, nj = P * V * 3, P * 72
    buf = torch.full((lead + n + 7,), float(guard), device=DEV)
    jbuf = torch.full((lead + nj + 7,), float(guard), device=DEV)
    feat, A = torch.empty(P, 208, device=DEV), torch.empty(P, 24, 12, device=DEV)
    K.skin_vertices(q, p, P, d["v_shaped"], d["blend"], d["J"], d["offsets"], body._parents_c, d["weights"], d["joints"], V, Kw, 1, 0,
                    feat, A, jbuf[lead:lead + nj], buf[lead:lead + n])
    host, jhost = buf.cpu().numpy(), jbuf.cpu().numpy()
    for h, m in ((host, n), (jhost, nj)):
        assert (h[:lead] == guard).all() and (h[lead + m:] == guard).all() and not (h[lead:lead + m] == guard).any()
    plain, joints = B.skin(body, q.reshape(1, P, 24, 3), p.reshape(1, P, 3), return_joints=True)
    assert np.array_equal(host[lead:lead + n], plain.cpu().numpy().reshape(-1)) and np.array_equal(jhost[lead:lead + nj], joints.cpu().numpy().reshape(-1))
    assert (feat[:, 207] == 0).all() and not torch.isnan(feat).any() and not torch.isnan(A).any()
    with pytest.raises(L.TcdiffError, match="misaligned"):                # feat and A are read 16 bytes at a time
        K.skin_vertices(q, p, P, d["v_shaped"], d["blend"], d["J"], d["offsets"], body._parents_c, d["weights"], d["joints"], V, Kw, 1, 0,
                        torch.empty(P * 208 + 1, device=DEV)[1:], A, None, buf[lead:lead + n])


def test_a_nan_pose_stays_in_its_pose(models):
    V, Kw, P = VT + 1, 4, PT + 1
    _, im, body = models(V, Kw)
    poses, trans = (np.array(a) for a in S.poses_of(P))
    clean = B.skin(body, _dev(poses)[None], _dev(trans)[None])[0]
    for bad in (0, 5, PT - 1, PT):
        dirty = poses.copy()
        dirty[bad, 7, 1] = np.nan
        for pose_blend in (True, False):
            got = B.skin(body, _dev(dirty)[None], _dev(trans)[None], pose_blend=pose_blend)[0]
            ref = clean if pose_blend else B.skin(body, _dev(poses)[None], _dev(trans)[None], pose_blend=False)[0]
            others = [i for i in range(P) if i != bad]
            assert torch.equal(got[others].view(torch.int32), ref[others].view(torch.int32)), (bad, pose_blend)
            # every vertex that hangs on joint 7 or below it in the tree, or (with the blend shapes) any vertex at all
            assert torch.isnan(got[bad]).any() and (not pose_blend or torch.isnan(got[bad]).all()), (bad, pose_blend)


def test_a_vertex_on_one_joint_without_blend_shapes_moves_rigidly(models):
    """all weight on one joint and zero posedirs: the vertex is A_j [v; 1] + s, compared in float64"""
    V, P = 40, 9
    m = S.make_model(V, 1, seed=77)
    m["posedirs"] = np.zeros_like(m["posedirs"])
    im, body = S.images(m), B.load_body_model(m, device=DEV)
    poses, trans = S.poses_of(P)
    got = B.skin(body, _dev(poses)[None], _dev(trans)[None])[0].cpu().numpy().astype(np.float64)
    _, A, _, shift = S.pose_part(im, poses, trans, "pelvis")
    A = A.reshape(P, 24, 3, 4)
    j = im["wj"][:, 0]
    assert (im["wv"][:, 0] == 1).all() and len(set(j.tolist())) > 5
    v = im["v_shaped"].astype(np.float64)
    Aj = A[:, j]                                                          # (P, V, 3, 4): each vertex's one joint
    want = np.einsum("pvab,vb->pva", Aj[..., :3], v) + Aj[..., 3] + shift[:, None]
    err = float(np.abs(got - want).max())
    bound = 8 * float(np.spacing(np.float32(np.abs(want).max())))         # three products, four sums and the rounding of A, in float32
    print(f"rigid vertices against A_j v in float64: largest error {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_runs_repeat_on_any_stream_layout_and_buffer(models):
    V, Kw = VT + 1, 4
    clips, T, dn = 3, 11, 2
    _, im, body = models(V, Kw)
    poses, trans = S.poses_of(clips * T * dn)
    q, p = _dev(poses).reshape(clips, T * dn, 24, 3), _dev(trans).reshape(clips, T * dn, 3)
    first, fj = B.skin(body, q, p, return_joints=True)
    again, aj = B.skin(body, q, p, return_joints=True)
    assert torch.equal(_bits(first), _bits(again)) and torch.equal(_bits(fj), _bits(aj))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = B.skin(body, q, p)
    side.synchronize()
    assert torch.equal(_bits(first), _bits(other))
    for c in range(clips):                                                # the pickles' 2-D layout, clip by clip
        flat = B.skin(body, q[c].reshape(T * dn, 72), p[c])
        assert tuple(flat.shape) == (1, T * dn, V, 3) and torch.equal(_bits(flat[0]), _bits(first[c]))
    strided = torch.zeros(clips, T * dn, 25, 3, device=DEV)              # a view that is not contiguous is copied, not misread
    strided[:, :, :24] = q
    assert torch.equal(_bits(B.skin(body, strided[:, :, :24], p)), _bits(first))
    buf = torch.full((clips, T * dn, V, 3), 9.0, device=DEV)
    assert B.skin(body, q, p, out=buf) is buf and torch.equal(_bits(buf), _bits(first))
    for bad in (buf[:, :, :, :2], buf.double(), buf.cpu(), buf[:2], buf.transpose(0, 1)):
        with pytest.raises(L.TcdiffError, match="out must be"):
            B.skin(body, q, p, out=bad)
    with pytest.raises(L.TcdiffError, match="MI355X"):
        B.skin(body, q, p.cpu())


def test_a_pose_alone_has_the_bits_it_has_in_a_batch(models):
    V, Kw, P = VT + 1, 8, PT + 1
    _, im, body = models(V, Kw)
    poses, trans = S.poses_of(P)
    q, p = _dev(poses)[None], _dev(trans)[None]
    for pose_blend in (True, False):
        batch = B.skin(body, q, p, pose_blend=pose_blend)
        for i in (0, 1, PT - 1, PT):
            alone = B.skin(body, q[:, i:i + 1], p[:, i:i + 1], pose_blend=pose_blend)
            assert torch.equal(_bits(alone[0, 0]), _bits(batch[0, i])), (i, pose_blend)


def test_a_vertex_has_the_bits_it_has_in_the_truncated_model():
    V, Kw, P = VT + 1, 4, 5
    m = S.make_model(V, Kw, seed=31)
    cut = {k: (v[:VT] if k in ("v_template", "shapedirs", "posedirs", "weights") else v) for k, v in m.items()}
    cut["J_regressor"], cut["f"] = m["J_regressor"][:, :VT], m["f"][:VT - 2]
    full, short = B.load_body_model(m, device=DEV), B.load_body_model(cut, device=DEV)
    poses, trans = S.poses_of(P)
    q, p = _dev(poses)[None], _dev(trans)[None]
    for origin in ("pelvis", "smpl"):                                     # the truncated regressor moves J: the same joints for both
        a, b = full.images(DEV), short.images(DEV)
        for k in ("J", "offsets"):
            b[k] = a[k]
        got, want = B.skin(full, q, p, origin=origin), B.skin(short, q, p, origin=origin)
        assert tuple(want.shape) == (1, P, VT, 3) and torch.equal(_bits(got[:, :, :VT]), _bits(want)), origin


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------
def _normalizer(scale, min_):
    n = tio.Normalizer.__new__(tio.Normalizer)
    n.scaler = tio.MinMaxScaler((-1, 1), clip=True)
    n.scaler.scale_, n.scaler.min_ = scale.float(), min_.float()
    return n


def test_end_to_end_the_files_skin_is_the_kernels(tmp_path, models):
    """samples -> export_poses -> skin and write_glb(mesh=) -> the reader and evaluator: the file's skinned vertices are
    skin(pose_blend=False) turned to Y-up, for a model of at most four weights per vertex (nothing for glTF to drop).  Bound: the
    CPU .glb test's 1e-5 m widened to the existing GPU end-to-end bound, 2e-5 m."""
    DN, S_ = 2, 5
    norm = _normalizer(torch.ones(151) * 0.5, torch.zeros(151))
    x = torch.rand(2, S_ * DN, 151, generator=torch.Generator().manual_seed(5)) * 2 - 1
    q, pos, _, _ = E.export_poses(x.to(DEV), norm, "normal", DN)
    _, _, body = models(37, 4, smpl_tree=True)
    verts = B.skin(body, q, pos, pose_blend=False).cpu().numpy().astype(np.float64).reshape(2, S_, DN, 37, 3)
    paths = [str(tmp_path / "a.glb"), str(tmp_path / "b.glb")]
    assert X.write_glb(paths, q, pos, DN, mesh=body) == paths
    for c, path in enumerate(paths):
        with open(path, "rb") as f:
            gltf, binary = G.read_glb(f.read())
        got = S.skinned(gltf, binary)
        assert len(got) == DN
        for d in range(DN):
            err = float(np.abs(got[d] - S.to_y_up(verts[c, :, d])).max())
            print(f"clip {c}, dancer {d}: the file's skinned vertices against skin(pose_blend=False), largest difference {err:.3e} m (bound 2e-5)")
            assert got[d].shape == (S_, 37, 3) and err <= 2e-5
    out = X.write_glb_out(str(tmp_path / "glb"), "normal", 7, ["a/x.npy", "a/y.npy"], q, pos, DN, mesh=body)
    assert [open(o, "rb").read() for o in out] == [open(p, "rb").read() for p in paths]
    assert open(paths[0], "rb").read() != open(X.write_glb(str(tmp_path / "stick.glb"), q[:1], pos[:1], DN)[0], "rb").read()
    with pytest.raises(L.TcdiffError, match="mesh="):
        X.write_glb(paths, q, pos, DN, mesh=body, offsets=body.offsets)
    assert sorted(os.listdir(tmp_path)) == ["a.glb", "b.glb", "glb", "stick.glb"]
