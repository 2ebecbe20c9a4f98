"""The mesh extraction on the GPU (include/instantavatar_hip_mesh.h; DESIGN.md section 4, "isosurface"): every new entry
point alone through the C ABI against the float64 references of tests/mesh_refs.py on lattices of 2..65 samples per axis,
then `AvatarModel.extract_mesh` / `pose_mesh` on the synthetic model and the extract_mesh driver.

Tolerances.  Classification is exact (the reference reads the same fp32 lattice), so counts, faces and vertex order are
compared for equality.  Positions: 1e-6 x the largest |box corner coordinate| -- three roundings in t, two each in P_a and
P_b and the final fma pair come to under 16 units of 2^-24 (9.5e-7) of that scale.  Forward skinning: 32 x 2^-24 x the sum of
the absolute values of the terms an output is made of (8 corners x 3 factors of the weights, the blend, two 4-term dot
products: fewer than 32 roundings, each relative to a partial sum that the sum of absolute values bounds)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_refs as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL = 10.0
BOX = mr.DEFAULT_BOX
ANISO = (np.float32([-1.0, -0.5, -2.0]), np.float32([1.5, 0.75, 1.0]))
PAD, MARK = 5, 7.0          # rows behind the counts, and what they are filled with: they must stay untouched


def _L():
    from instantavatar_amd import _lib
    return _lib


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _lattice(N, box):
    from instantavatar_amd import mesh
    return mesh.lattice_desc(N, box[0], box[1])


# ---- 1. lattice points ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,box,first,count", [(9, BOX, 0, 729), (12, ANISO, 0, 1728), (33, ANISO, 1000, 4097), (2, BOX, 3, 5),
                                               (33, BOX, 33 ** 3 - 77, 77)])
def test_lattice_points(N, box, first, count):
    L = _L()
    pts = torch.full((count + PAD, 3), MARK, device=DEV)
    L.call("ia_iso_lattice_points", _lattice(N, box), first, count, pts)
    torch.cuda.synchronize()
    got = _np(pts)
    assert np.array_equal(got[:count].view(np.uint32), mr.lattice_points32(N, box[0], box[1], first, count).view(np.uint32))
    assert (got[count:] == MARK).all()
    with pytest.raises(L.IAError):
        L.call("ia_iso_lattice_points", _lattice(N, box), N ** 3 - 1, 2, pts)


# ---- 2. / 3. count + emit ---------------------------------------------------------------------------------------------
def _nonfinite(N, seed):
    s = mr.noise_lattice(N, seed, LEVEL)
    rng = np.random.RandomState(seed + 100)
    idx = rng.permutation(N ** 3)[:60]
    s[idx[:20]], s[idx[20:40]], s[idx[40:]] = np.nan, np.inf, -np.inf
    return s


def _equal_to_level(N, seed):
    return (LEVEL + np.random.RandomState(seed).randint(-1, 2, N ** 3)).astype(np.float32)      # a third of the samples == level


def _centre(N):
    s = np.zeros((N, N, N), np.float32)
    s[N // 2, N // 2, N // 2] = 50.0
    return s.reshape(-1)


def _corner(N):
    s = np.zeros(N ** 3, np.float32)
    s[0] = 50.0
    return s


#       name          N   lattice                                   cap    box
CASES = {
    "sphere":        (17, lambda: mr.sphere_lattice(17, level=LEVEL), True, BOX),
    "two_spheres":   (20, lambda: mr.two_spheres_lattice(20, LEVEL), True, BOX),      # 19^3 cells: no multiple of the wave size
    "noise9":        (9, lambda: mr.noise_lattice(9, 1, LEVEL), True, BOX),
    "noise12":       (12, lambda: mr.noise_lattice(12, 2, LEVEL), True, ANISO),
    "nonfinite":     (9, lambda: _nonfinite(9, 3), True, BOX),
    "all_inside":    (6, lambda: np.full(6 ** 3, 20.0, np.float32), True, BOX),       # a closed box surface
    "all_outside":   (6, lambda: np.zeros(6 ** 3, np.float32), True, BOX),            # counts 0 0
    "equal_level":   (7, lambda: _equal_to_level(7, 4), True, BOX),
    "n2_capped":     (2, lambda: _centre(2), True, BOX),                              # N = 2 has outer points only: empty with cap
    "n2_open":       (2, lambda: _corner(2), False, BOX),
    "n3_centre":     (3, lambda: _centre(3), True, ANISO),
    "noise9_open":   (9, lambda: mr.noise_lattice(9, 1, LEVEL), False, BOX),          # cap off: an open mesh
    "noise33":       (33, lambda: mr.noise_lattice(33, 5, LEVEL), True, BOX),         # 141 workgroups: the scan over workgroup sums
    # 1 073 workgroups: the scan carries past its first 1 024 sums, and the second sphere lies in the workgroups behind them
    "far_spheres65": (65, lambda: np.maximum(mr.sphere_lattice(65, centre=(-0.7, -0.7, -0.7), radius=0.15),
                                             mr.sphere_lattice(65, centre=(0.9, 0.7, 0.7), radius=0.15)).astype(np.float32), True, BOX),
}
_results = {}


def _extract(sigma, N, cap, box, level=LEVEL):
    """count + emit through the C ABI with marked padding behind both buffers -> (verts [nv,3], faces [nf,3]) numpy"""
    L = _L()
    lat = _lattice(N, box)
    sd = _dev(sigma)
    nb = int(L.call("ia_iso_workspace_bytes", N))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    L.call("ia_iso_count", sd, N, level, int(cap), ws, nb, counts)
    nv, nf = counts.tolist()
    verts = torch.full((nv + PAD, 3), MARK, device=DEV)
    faces = torch.full((nf + PAD, 3), int(MARK), dtype=torch.int32, device=DEV)
    L.call("ia_iso_emit", sd, lat, level, int(cap), ws, nb, verts, nv, faces, nf)
    torch.cuda.synchronize()
    v, f = _np(verts), _np(faces)
    assert (v[nv:] == MARK).all() and (f[nf:] == int(MARK)).all(), "rows past the counts were written"
    return v[:nv], f[:nf]


def _case(name):
    if name not in _results:
        N, make, cap, box = CASES[name]
        sigma = make()
        ref = mr.marching_tets(sigma, N, LEVEL, box[0], box[1], cap)
        _results[name] = (sigma, ref, _extract(sigma, N, cap, box))
    return _results[name]


@pytest.mark.parametrize("name", list(CASES))
def test_count_and_emit_against_reference(name):
    N, _, cap, box = CASES[name]
    if name == "far_spheres65":
        assert (65 ** 3 + 255) // 256 > 1024                 # why 65: more workgroup sums than one trip of the scan over them takes
    sigma, (rv, rf, _), (v, f) = _case(name)
    print("%s: N %d, %d vertices, %d faces (reference %d, %d)" % (name, N, len(v), len(f), len(rv), len(rf)))
    assert (len(v), len(f)) == (len(rv), len(rf))
    if name in ("all_outside", "n2_capped"):
        assert len(v) == 0 and len(f) == 0
        return
    assert len(f) > 0
    got, want = mr.canonical_faces(f), mr.canonical_faces(rf)
    order = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]
    assert np.array_equal(order(got), order(want)), "the face sets differ"
    assert np.array_equal(got, want), "the faces are not in cell / tetrahedron / triangle order"
    tol = 1e-6 * float(np.abs(np.concatenate(box)).max())
    err = np.abs(v.astype(np.float64) - rv).max()            # same index = same edge: the vertex order is compared here
    print("%s: max position error %.3e (bound %.3e)" % (name, err, tol))
    assert err <= tol, (err, tol)
    v2, f2 = _extract(sigma, N, cap, box)
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(f, f2), "two runs differ"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[2] and n not in ("all_outside", "n2_capped")])
def test_capped_meshes_are_closed(name):
    """on the kernel's own output, independent of the reference: every directed edge once, its reverse once"""
    _, _, (v, f) = _case(name)
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    assert mr.is_closed_oriented(f)
    if name == "sphere":
        _, (rv, rf, _), _ = _case(name)
        vol, ref = mr.signed_volume(v, f), mr.signed_volume(rv, rf)
        assert ref > 0 and abs(vol - ref) <= 1e-5 * ref, (vol, ref)
        assert mr.euler_characteristic(len(v), f) == 2


def test_open_mesh_without_cap():
    _, _, (v, f) = _case("noise9_open")
    assert not mr.is_closed_oriented(f)


def test_iso_argument_errors():
    L = _L()
    s = torch.zeros(8, device=DEV)
    ws, counts = torch.empty(1 << 16, dtype=torch.uint8, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(L.IAError):
        L.call("ia_iso_count", s, 1, LEVEL, 1, ws, ws.numel(), counts)
    with pytest.raises(L.IAError):
        L.call("ia_iso_count", s, 565, LEVEL, 1, ws, ws.numel(), counts)
    with pytest.raises(L.IAError, match="workspace"):
        L.call("ia_iso_count", s, 2, LEVEL, 1, ws, 16, counts)


# ---- 4. largest component ---------------------------------------------------------------------------------------------
def _largest(v, f, unit=4.0):
    L = _L()
    nv, nf = len(v), len(f)
    vd, fd = _dev(v), _dev(f)
    nb = int(L.call("ia_mesh_component_workspace_bytes", nv, nf))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    L.call("ia_mesh_largest_count", vd, fd, nv, nf, unit, ws, nb, counts)
    nv2, nf2 = counts.tolist()
    vo = torch.full((nv2 + PAD, 3), MARK, device=DEV)
    fo = torch.full((nf2 + PAD, 3), int(MARK), dtype=torch.int32, device=DEV)
    src = torch.full((nv2 + PAD,), int(MARK), dtype=torch.int32, device=DEV)
    L.call("ia_mesh_largest_emit", vd, fd, nv, nf, ws, nb, vo, nv2, fo, nf2, src)
    torch.cuda.synchronize()
    vo, fo, src = _np(vo), _np(fo), _np(src)
    assert (vo[nv2:] == MARK).all() and (fo[nf2:] == int(MARK)).all() and (src[nv2:] == int(MARK)).all()
    return vo[:nv2], fo[:nf2], src[:nv2]


def test_largest_component():
    _, _, (v, f) = _case("two_spheres")
    label, area = mr.components(v, f)
    assert len(area) == 2
    rv, rf, rsrc = mr.largest_component(v, f)
    vo, fo, src = _largest(v, f)
    assert 0 < len(vo) < len(v) and 0 < len(fo) < len(f)
    assert np.array_equal(src, rsrc) and (np.diff(src) > 0).all(), "vert_src / the order of the kept vertices"
    assert np.array_equal(vo.view(np.uint32), v[src].view(np.uint32))
    assert np.array_equal(fo, rf), "faces: re-indexed, order preserved"
    assert (vo[:, 0] < 0.05).all(), "only the larger sphere (centred at x = -0.45) remains"
    assert mr.is_closed_oriented(fo) and mr.euler_characteristic(len(vo), fo) == 2
    # the smaller sphere first in vertex order, by mirroring the lattice: the winner is decided by area, not by index
    vm = v.copy()
    vm[:, 0] = -vm[:, 0]
    perm = np.argsort(vm[:, 0], kind="stable")
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    vo2, fo2, src2 = _largest(vm[perm], inv[f].astype(np.int32))
    assert len(vo2) == len(vo) and len(fo2) == len(fo) and (vo2[:, 0] > -0.05).all()
    again = _largest(v, f)
    assert all(np.array_equal(a, b) for a, b in zip((vo, fo, src), again)), "two runs differ"


def test_largest_component_of_one_component_and_of_nothing():
    _, _, (v, f) = _case("sphere")
    vo, fo, src = _largest(v, f)
    assert np.array_equal(vo.view(np.uint32), v.view(np.uint32)) and np.array_equal(fo, f) and np.array_equal(src, np.arange(len(v)))
    vo, fo, src = _largest(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert len(vo) == 0 and len(fo) == 0
    # a tie in area: two congruent triangles; the component with the smaller root vertex wins
    tv = np.float32([[5, 0, 0], [6, 0, 0], [5, 1, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]])
    tf = np.int32([[3, 4, 5], [0, 1, 2]])
    vo, fo, src = _largest(tv, tf)
    assert src.tolist() == [0, 1, 2] and fo.tolist() == [[0, 1, 2]]


# ---- 5. forward skinning ----------------------------------------------------------------------------------------------
def _world():
    import world
    return world.build(DEV, 64, 16)


def _grid(model, init):
    fd = model.deformer.deformer
    grid = dict(D=init["D"], H=init["H"], W=init["W"], offset=init["offset_kernel"], scale=init["scale_kernel"])
    vJ = _np(fd.voxel_J_cl).reshape(grid["D"], grid["H"], grid["W"], 12)
    return grid, vJ


def _frame(i):
    import world
    from instantavatar_amd.pipeline import make_batch
    poses, tr = world.poses(8)
    return make_batch(DEV, 8, poses[i], tr[i])


def _skin_check(xc, xd, model, init, what):
    grid, vJ = _grid(model, init)
    s2w = _np(model.deformer.A).reshape(-1, 4, 4)[0]
    ref, mag = mr.forward_skin_ref(xc, vJ, grid, s2w)
    err = np.abs(xd.astype(np.float64) - ref)
    bound = 32 * 2.0 ** -24 * mag
    print("%s: max error / bound %.3f, max |error| %.3e" % (what, float((err / bound).max()), float(err.max())))
    assert (err <= bound).all(), float((err / bound).max())
    return s2w


def test_forward_skin():
    L = _L()
    model, body, fp, init = _world()
    model.deformer.prepare_deformer(_frame(3))
    rng = np.random.RandomState(9)
    n = 4096
    # in and around the body: uniform over 1.3 x the transform grid (normalised coordinate g = scale (x + offset) in [-1.3, 1.3]),
    # so that (1 / 1.3)^3 = 46 % of the points have all corners inside, the rest cross the rim or lie outside
    off, scl = init["offset_kernel"].astype(np.float64), init["scale_kernel"].astype(np.float64)
    xc = (rng.uniform(-1.3, 1.3, (n, 3)) / scl - off).astype(np.float32)
    xc[:64] = (10.0 + rng.uniform(0, 1, (64, 3))).astype(np.float32)          # every corner outside the grid
    xd = torch.full((n + PAD, 3), MARK, device=DEV)
    fd = model.deformer.deformer
    s2w_dev = model.deformer.A.reshape(-1, 4, 4)[0].contiguous()
    L.call("ia_forward_skin", _dev(xc), n, fd.voxel_J_cl, fd.grid_desc(), s2w_dev, xd)
    torch.cuda.synchronize()
    got = _np(xd)
    assert (got[n:] == MARK).all() and np.isfinite(got[:n]).all()
    s2w = _skin_check(xc, got[:n], model, init, "forward skin")
    assert np.array_equal(got[:64], np.broadcast_to(s2w[:3, 3].astype(np.float32), (64, 3))), "J = 0 must give exactly s2w's translation"
    moved = np.abs(got[64:n] - s2w[:3, 3].astype(np.float32)).max(1) > 1e-3
    assert moved.sum() > 1000, "most points lie inside the grid"


# ---- 6. extract_mesh --------------------------------------------------------------------------------------------------
_meshes = {}


def _model_mesh(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _meshes:
        _meshes[key] = _world()[0].extract_mesh(resolution=64, **kw)
    return _meshes[key]


def test_extract_mesh():
    from instantavatar_amd import mesh as M
    model = _world()[0]
    net = model.net_coarse
    one = _model_mesh(largest=False, chunk=1 << 21)
    small = _model_mesh(largest=False, chunk=4096)
    for a, b in ((one.verts, small.verts), (one.faces, small.faces), (one.normals, small.normals), (one.colors, small.colors)):
        assert torch.equal(a, b), "the mesh depends on the chunk size"
    lo, hi = M.field_box(net)
    sigma = _np(M.lattice_sigma(net, M.lattice_desc(64, lo, hi), 4096))
    rv, rf, _ = mr.marching_tets(sigma, 64, 10.0, lo, hi, True)
    v, f = _np(one.verts), _np(one.faces)
    print("extract_mesh(64, all components): %d vertices, %d faces" % (len(v), len(f)))
    assert (len(v), len(f)) == (len(rv), len(rf)) and len(f) > 1000
    assert np.array_equal(mr.canonical_faces(f), mr.canonical_faces(rf))
    assert np.abs(v.astype(np.float64) - rv).max() <= 1e-6 * float(np.abs(np.concatenate([lo, hi])).max())
    assert mr.is_closed_oriented(f)
    big = _model_mesh(largest=True)
    bv, bf = _np(big.verts), _np(big.faces)
    assert 1000 < len(bf) <= len(f) and mr.is_closed_oriented(bf)
    kv, kf, _ = mr.largest_component(v, f)
    assert np.array_equal(bv.view(np.uint32), kv.view(np.uint32)) and np.array_equal(bf, kf)
    for m in (one, big):
        n, c = _np(m.normals).astype(np.float64), _np(m.colors)
        assert np.isfinite(n).all() and np.isfinite(c).all()
        ln = np.linalg.norm(n, axis=1)
        assert ((ln == 0) | (np.abs(ln - 1) <= 1e-6)).all() and (ln > 0).mean() > 0.9
        assert c.min() >= 0 and c.max() <= 1
    # the sign of the normals: -g / |g| points towards falling density, the faces are wound from inside to outside, so a vertex
    # normal lies on the side of the area-weighted normals of its faces; with the sign wrong fewer than half of them would
    tri = bv[bf].astype(np.float64)
    fn = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    vn = np.zeros((len(bv), 3))
    for k in range(3):
        np.add.at(vn, bf[:, k], fn)
    agree = (vn * _np(big.normals)).sum(1) > 0
    print("vertex normals on the side of the face winding: %.4f" % agree.mean())
    assert agree.mean() > 0.5


# ---- 7. pose_mesh -----------------------------------------------------------------------------------------------------
def test_pose_mesh():
    from instantavatar_amd import synthetic as syn
    from instantavatar_amd.pipeline import make_batch
    model, body, fp, init = _world()
    mesh = _model_mesh(largest=True)
    xc = _np(mesh.verts)
    # the canonical pose as the frame's pose, any root orientation and translation: every bone transform is the identity
    pose72 = np.concatenate([np.float32([0.3, -0.2, 0.1]), syn.cano_pose("A_pose")]).astype(np.float32)
    posed = model.pose_mesh(mesh, make_batch(DEV, 8, pose72, np.float32([0.1, 0.15, 5.0])))
    torch.cuda.synchronize()
    assert posed.faces is mesh.faces and posed.colors is mesh.colors
    s2w = _np(model.deformer.A).reshape(-1, 4, 4)[0].astype(np.float64)
    want = xc.astype(np.float64) @ s2w[:3, :3].T + s2w[:3, 3]
    err = np.abs(_np(posed.verts) - want).max()
    print("pose_mesh, canonical pose: max |x_d - s2w x_c| %.3e" % err)
    assert err <= 1e-5 * (1 + np.abs(want).max())
    # rigid: the normals are the canonical ones rotated
    nw = _np(mesh.normals).astype(np.float64) @ s2w[:3, :3].T
    assert np.abs(_np(posed.normals) - nw).max() <= 1e-4
    # a pose of the procedural track: positions against the float64 reference
    posed = model.pose_mesh(mesh, _frame(5))
    torch.cuda.synchronize()
    assert torch.equal(posed.faces, mesh.faces)
    _skin_check(xc, _np(posed.verts), model, init, "pose_mesh, frame 5")
    ln = np.linalg.norm(_np(posed.normals).astype(np.float64), axis=1)
    assert np.isfinite(ln).all() and ((ln == 0) | (np.abs(ln - 1) <= 1e-5)).all() and (ln > 0).mean() > 0.9
    assert np.abs(_np(posed.verts) - want).max() > 0.05, "the pose moved the vertices"


def test_pose_mesh_needs_the_snarf_deformer():
    from instantavatar_amd.deformers.smpl_deformer import SMPLDeformer
    from instantavatar_amd.pipeline import AvatarModel
    m = AvatarModel(SMPLDeformer.__new__(SMPLDeformer), _world()[0].net_coarse, None)
    with pytest.raises(NotImplementedError, match="SNARF"):
        m.pose_mesh(_model_mesh(largest=True), _frame(0))


# ---- 8. driver --------------------------------------------------------------------------------------------------------
def test_extract_mesh_driver(tmp_path):
    import world
    poses, tr = world.poses(8)
    np.savez(tmp_path / "track.npz", poses=poses[:2], trans=tr[:2])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "instantavatar_amd.drivers.extract_mesh", "--synthetic", "--resolution", "48", "--poses",
           str(tmp_path / "track.npz"), "--out", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = {name: mr.read_ply(str(tmp_path / "out" / (name + ".ply"))) for name in ("canonical", "posed_0", "posed_1")}
    for name, p in files.items():
        assert p["payload_bytes"] == p["expected_bytes"] > 0, name
        assert np.array_equal(p["faces"], files["canonical"]["faces"]), name
        assert len(p["vertex"]) == len(files["canonical"]["vertex"])
        assert p["faces"].min() == 0 and p["faces"].max() == len(p["vertex"]) - 1
    assert mr.is_closed_oriented(files["canonical"]["faces"])
    assert not np.array_equal(files["posed_0"]["vertex"]["x"], files["posed_1"]["vertex"]["x"])
    assert not (tmp_path / "out" / "posed_2.ply").exists()
