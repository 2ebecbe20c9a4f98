"""The rasteriser on the GPU (include/instantavatar_hip_raster.h; DESIGN.md section 4, "rasteriser"): every entry point alone
through the C ABI against the numpy references of tests/raster_refs.py, then `rasterize` / `Mesh.render` on the synthetic
model's mesh and the two driver flags.  Image sizes are 37 x 29 and 96 x 80 (no multiples of the wave size); every buffer has
marked padding behind it that must stay untouched.

Tolerances, in units of u = 2^-24 (half an fp32 ulp, relative).
  projection  the kernel evaluates in fp64 and rounds once, so |xy - 256 u_64| <= 0.5 plus float64 noise; the bound asserted is
              the looser one an fp32 evaluation would be entitled to, 0.5 + 256 * 16 u (|fx p.x / p.z| + |cx|).  inv_z: one
              rounding; 8 u asserted.
  coverage    exact integers: face_id is compared for equality wherever the depth order is not a rounding question.
  depth order best and second-best reference inverse depth more than 32 u apart (the device's iz carries 6 roundings: E_i and |A|
              to fp32, the quotient, the product, two fused adds -- all terms positive, so relative errors do not grow).
  depth       16 u: those 6 and the reciprocal.
  attributes  32 u x sum |l_i w_i a_i| / iz: 5 roundings per term, 2 fused adds, the quotient, and iz's own 6."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_refs as rr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
PAD, MARK = 7, 77
SIZES = ((29, 37), (80, 96))          # (H, W)
CASES = rr.hand_cases()


def _L():
    from instantavatar_amd import _lib
    return _lib


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _padded(n, dtype, cols=None):
    """a buffer of n (+ PAD) rows filled with MARK"""
    shape = (n + PAD,) if cols is None else (n + PAD, cols)
    return torch.full(shape, MARK, dtype=dtype, device=DEV)


def _untouched(t, n):
    return bool((t[n:] == MARK).all())


def _project(verts, w2c, fx, fy, cx, cy, near=0.05):
    L = _L()
    nv = len(verts)
    xy, inv_z = _padded(nv, torch.int32, 2), _padded(nv, torch.float32)
    L.call("ia_raster_project", _dev(verts, torch.float32), nv, _dev(w2c, torch.float32), fx, fy, cx, cy, near, xy, inv_z)
    torch.cuda.synchronize()
    assert _untouched(xy, nv) and _untouched(inv_z, nv), "rows past nv were written"
    return _np(xy)[:nv].astype(np.int64), _np(inv_z)[:nv]


def _raster(xy, inv_z, faces, H, W, cull, attrs=None):
    """visibility + resolve through the C ABI with marked padding behind every buffer -> dict of numpy arrays"""
    L = _L()
    nv, nf, R = len(xy), len(faces), H * W
    C = 0 if attrs is None else attrs.shape[1]
    nb = int(L.call("ia_raster_workspace_bytes", nv, nf, H, W))
    assert nb > 0
    ws = torch.full((nb + 256,), MARK, dtype=torch.uint8, device=DEV)
    vis = _padded(R, torch.int64)
    face_id, depth, counts = _padded(R, torch.int32), _padded(R, torch.float32), _padded(2, torch.int32)
    out = _padded(R, torch.float32, C) if C else None
    xy_d, w_d = _dev(xy, torch.int32), _dev(inv_z, torch.float32)
    f_d = _dev(faces, torch.int32) if nf else None
    a_d = _dev(attrs, torch.float32) if C else None
    L.call("ia_raster_visibility", xy_d, w_d, nv, f_d, nf, H, W, int(cull), vis, ws, nb)
    L.call("ia_raster_resolve", xy_d, w_d, nv, f_d, nf, vis, H, W, a_d, C, ws, nb, face_id, depth, out, counts)
    torch.cuda.synchronize()
    assert _untouched(vis, R) and _untouched(face_id, R) and _untouched(depth, R) and _untouched(counts, 2) and _untouched(ws, nb), \
        "bytes past the buffers were written"
    assert out is None or _untouched(out, R)
    return dict(face_id=_np(face_id)[:R].reshape(H, W), depth=_np(depth)[:R].reshape(H, W), vis=_np(vis)[:R].reshape(H, W),
                attrs=None if out is None else _np(out)[:R].reshape(H, W, C), skipped=int(counts[0]), covered=int(counts[1]))


def _check(got, ref, faces, inv_z, attrs, what, sure=None):
    """got (device) against ref (rr.rasterize) on the pixels `sure` (default: all); returns the largest error / bound ratios"""
    sure = np.ones(ref["face_id"].shape, bool) if sure is None else sure
    assert np.array_equal(got["face_id"][sure], ref["face_id"][sure]), "%s: %d face ids differ" % (what, (got["face_id"] != ref["face_id"])[sure].sum())
    hit, empty = sure & (ref["face_id"] >= 0), ref["face_id"] < 0
    assert np.array_equal(got["face_id"] < 0, empty), what              # coverage itself is exact everywhere
    assert (got["depth"][empty] == 0).all() and (got["vis"][empty] == 0).all(), what
    assert got["covered"] == int((~empty).sum()) and got["skipped"] == ref["skipped"], (what, got["covered"], got["skipped"], ref["skipped"])
    ratios = [0.0, 0.0]
    if hit.any():
        want = rr.depth_of(ref)
        ratios[0] = float((np.abs(got["depth"] - want)[hit] / (16 * U * want[hit])).max())
        assert ratios[0] <= 1, (what, ratios[0])
    if attrs is not None:
        want, scale = rr.interpolate(ref, faces, inv_z, attrs)
        assert (got["attrs"][empty] == 0).all(), what
        if hit.any():
            ok = hit[..., None] & (scale > 0)
            ratios[1] = float((np.abs(got["attrs"] - want)[ok] / (32 * U * scale[ok])).max()) if ok.any() else 0.0
            assert ratios[1] <= 1 and (got["attrs"][hit[..., None] & (scale == 0)] == 0).all(), (what, ratios[1])
    return ratios


# ---- 1. projection ----------------------------------------------------------------------------------------------------
def test_project():
    rng = np.random.RandomState(0)
    nv = 3001
    X = rng.uniform(-1, 1, (nv, 3)).astype(np.float32)
    a = 0.4
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, :3] = np.float32([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]) @ np.float32([[1, 0, 0], [0, 0.8, -0.6], [0, 0.6, 0.8]])
    w2c[:3, 3] = [0.1, -0.2, 2.5]
    fx, fy, cx, cy, near = 130.5, 127.25, 47.75, 40.125, 0.75        # (exact in fp32, as the C ABI takes them)
    X[:200, 2] -= 4.0                                         # behind the camera, or in front of it but closer than `near`
    X[200:210] = np.nan
    X[210:215, 0], X[215:220, 1], X[220:225, 2] = np.inf, -np.inf, np.inf
    # in front of `near` and far off screen: placed in camera space (|p.x|, |p.y| of 200 .. 300 at p.z ~ 1: beyond 2^22 / 256 pixels)
    p_far = np.concatenate([rng.uniform(200, 300, (40, 2)) * rng.choice([-1, 1], (40, 2)), rng.uniform(0.8, 1.2, (40, 1))], 1)
    X[300:340] = ((p_far - w2c[:3, 3].astype(np.float64)) @ w2c[:3, :3].astype(np.float64)).astype(np.float32)
    ref = rr.project(X, w2c, fx, fy, cx, cy, near)
    p, valid = ref["p"], ref["valid"]
    fin = np.isfinite(p).all(1)
    # the test's own data: classes are present, and nothing sits on a threshold where the last bit of a float64 sum would decide
    assert (fin & (p[:, 2] < near)).sum() > 100 and (~fin).sum() == 25 and valid.sum() > 2000
    big = fin & (p[:, 2] >= near) & ~valid
    assert big.sum() >= 10
    with np.errstate(all="ignore"):
        assert np.abs(p[fin, 2] - near).min() > 1e-6
        m = np.maximum(np.abs(ref["u"]), np.abs(ref["v"]))[fin & (p[:, 2] >= near)] * 256
        assert np.abs(m - rr.XY_MAX).min() > 1.0
    xy, inv_z = _project(X, w2c, fx, fy, cx, cy, near)
    assert np.array_equal(inv_z != 0, valid), "validity flags"
    assert (xy[~valid] == 0).all() and (inv_z[~valid] == 0).all()
    u, v, z = ref["u"][valid], ref["v"][valid], p[valid, 2]
    bx = 0.5 + 256 * 16 * U * (np.abs(fx * p[valid, 0] / z) + abs(cx))
    by = 0.5 + 256 * 16 * U * (np.abs(fy * p[valid, 1] / z) + abs(cy))
    ex, ey = np.abs(xy[valid, 0] - 256 * u), np.abs(xy[valid, 1] - 256 * v)
    ez = np.abs(inv_z[valid].astype(np.float64) * z - 1)
    print("project: %d valid of %d; max |xy - 256 u| %.4f / %.4f (bound >= 0.5), max inv_z error %.2f u" % (valid.sum(), nv, ex.max(), ey.max(), ez.max() / U))
    assert (ex <= bx).all() and (ey <= by).all() and ez.max() <= 8 * U
    assert np.array_equal(xy[valid], ref["xy"][valid])          # (fp64 on both sides: the same integers)


# ---- 2. visibility + resolve on hand-made input -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_hand_made_cases(name):
    c = CASES[name]
    rng = np.random.RandomState(len(name))
    attrs = rng.uniform(-2, 2, (len(c["xy"]), 3)).astype(np.float32)
    seen = set()
    for H, W in SIZES:
        for cull in (False, True):
            ref = rr.rasterize(c["xy"], c["inv_z"], c["faces"], H, W, cull)
            got = _raster(c["xy"], c["inv_z"], c["faces"], H, W, cull, attrs)
            r = _check(got, ref, c["faces"], c["inv_z"], attrs, "%s %dx%d cull %d" % (name, W, H, cull))
            seen |= set(np.unique(ref["face_id"]))
            print("%s %dx%d cull %d: %d covered, %d skipped, depth %.2f of its bound, attributes %.2f" % (name, W, H, cull, got["covered"], got["skipped"], *r))
    if name in ("sliver", "off_screen", "off_screen_right", "degenerate", "no_faces"):
        assert seen == {-1}
    else:
        assert len(seen) > 1


def test_without_attributes_and_wide_channels():
    """C = 0 (no attribute buffers at all) and C = 8 (the limit) on the case that takes both paths"""
    c = CASES["small_over_large"]
    H, W = SIZES[0]
    ref = rr.rasterize(c["xy"], c["inv_z"], c["faces"], H, W, False)
    _check(_raster(c["xy"], c["inv_z"], c["faces"], H, W, False, None), ref, c["faces"], c["inv_z"], None, "C = 0")
    attrs = np.random.RandomState(8).uniform(-1, 3, (len(c["xy"]), 8)).astype(np.float32)
    _check(_raster(c["xy"], c["inv_z"], c["faces"], H, W, False, attrs), ref, c["faces"], c["inv_z"], attrs, "C = 8")
    L = _L()
    t = torch.zeros(64, dtype=torch.int32, device=DEV)
    with pytest.raises(L.IAError, match="C = 9"):
        L.call("ia_raster_resolve", t, t.float(), 8, t, 4, t.long(), 4, 4, t.float(), 9, t.to(torch.uint8), 64, t, t.float(), t.float(), t)


# ---- 3. depth order: two interpenetrating spheres, projected by the device ------------------------------------------------
@pytest.mark.parametrize("cull", [False, True])
def test_depth_order(cull):
    H, W = 80, 96
    V, F = rr.sphere_pair()
    w2c, fx, fy, cx, cy = rr.pair_camera(H, W)
    xy, inv_z = _project(V, w2c, fx, fy, cx, cy)
    assert (inv_z > 0).all()
    attrs = np.random.RandomState(5).uniform(-1, 1, (len(V), 5)).astype(np.float32)
    ref = rr.rasterize(xy, inv_z, F, H, W, cull)
    cov = ref["face_id"] >= 0
    unsure = cov & (ref["second"] > 0) & (ref["iz"] - ref["second"] <= 32 * U * ref["iz"])
    print("depth order, cull %d: %d covered pixels, %d left out as too close to call, %d faces skipped" % (cull, cov.sum(), unsure.sum(), ref["skipped"]))
    assert cov.sum() == 1576 and unsure.sum() <= 0.005 * cov.sum()
    got = _raster(xy, inv_z, F, H, W, cull, attrs)
    r = _check(got, ref, F, inv_z, attrs, "sphere pair", sure=~unsure)
    print("depth %.2f of its bound (16 u), attributes %.2f of theirs (32 u x scale)" % tuple(r))
    assert len(np.unique(got["face_id"][cov] // 1280)) == 2                   # both spheres are seen
    again = _raster(xy, inv_z, F, H, W, cull, attrs)
    for k in ("face_id", "depth", "vis", "attrs"):
        assert np.array_equal(got[k].view(np.uint8), again[k].view(np.uint8)), "two runs differ in " + k
    assert (got["skipped"], got["covered"]) == (again["skipped"], again["covered"])


# ---- 4. public API ------------------------------------------------------------------------------------------------------
def _world():
    import world
    return world.build(DEV)


def _posed_mesh():
    import world
    from instantavatar_amd.drivers.animate import AnimateSequence
    model = _world()[0]
    poses, tr = world.poses(8)
    seq = AnimateSequence(poses[:3], tr[:3], np.zeros(10, np.float32), torch.device(DEV), size=128)
    mesh = model.extract_mesh(resolution=64)
    return model, seq, model.pose_mesh(mesh, seq.batch(2, rays=False))


def test_mesh_render_against_the_reference():
    from instantavatar_amd import raster
    model, seq, mesh = _posed_mesh()
    cam = seq.camera()
    H, W = cam.H, cam.W
    img = mesh.render(cam)
    frame = raster.rasterize(mesh.verts, mesh.faces, cam, cull=True)
    torch.cuda.synchronize()
    assert torch.equal(frame.face_id, img["face_id"]) and torch.equal(frame.mask, img["mask"]) and frame.attrs is None
    V, F, N, Cc = _np(mesh.verts), _np(mesh.faces), _np(mesh.normals), _np(mesh.colors)
    pr = rr.project(V, _np(cam.w2c), cam.fx, cam.fy, cam.cx, cam.cy, cam.near)
    ref = rr.rasterize(pr["xy"], pr["inv_z"], F, H, W, cull=True)
    cov = ref["face_id"] >= 0
    unsure = cov & (ref["second"] > 0) & (ref["iz"] - ref["second"] <= 32 * U * ref["iz"])
    sure = ~unsure
    fid, mask, depth = _np(img["face_id"]), _np(img["mask"]), _np(img["depth"])
    print("Mesh.render 128 x 128: %d vertices, %d faces, %d covered pixels, %d too close to call, %d faces skipped"
          % (len(V), len(F), cov.sum(), unsure.sum(), int(frame.counts[0])))
    assert cov.sum() > 300 and unsure.sum() <= 0.005 * cov.sum()
    assert np.array_equal(mask, cov) and np.array_equal(fid[sure], ref["face_id"][sure])
    assert frame.counts.tolist() == [ref["skipped"], int(cov.sum())]
    hit = sure & cov
    want = rr.depth_of(ref)
    assert (np.abs(depth - want)[hit] <= 16 * U * want[hit]).all() and (depth[~cov] == 0).all()
    # the 8-bit images: a channel may fall on the other side of a quantisation step, never further
    n_cam = N.astype(np.float64) @ _np(cam.w2c)[:3, :3].astype(np.float64).T
    both, _ = rr.interpolate(ref, F, pr["inv_z"], np.concatenate([Cc.astype(np.float64), n_cam], 1))
    rgba8, normal8, shaded8 = _np(img["rgba8"]), _np(img["normal8"]), _np(img["shaded8"])
    assert np.array_equal(rgba8[..., 3], np.where(cov, 255, 0)) and (rgba8[~cov] == 0).all()
    q = lambda x: np.clip(x, 0, 1) * 255
    assert (np.abs(rgba8[..., :3][hit] - np.floor(q(both[..., :3][hit]))) <= 1).all()
    n = both[..., 3:]
    ln = np.linalg.norm(n, axis=-1)
    lit = hit & (ln > 1e-3)
    assert lit.sum() > 0.9 * hit.sum()
    unit = n[lit] / ln[lit][:, None]
    assert (normal8[lit][:, 3] == 255).all() and (np.abs(normal8[lit][:, :3] - np.floor(q((unit + 1) / 2))) <= 1).all()
    y, x = np.mgrid[0:H, 0:W]
    d = np.stack([(x - cam.cx) / cam.fx, (y - cam.cy) / cam.fy, np.ones((H, W))], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    s = np.maximum(0, -(unit * d[lit]).sum(-1))
    assert (np.abs(shaded8[lit][:, 0] - np.floor(q(s))) <= 1).all() and (shaded8[~cov] == 0).all() and (normal8[~cov] == 0).all()
    assert (s > 0).mean() > 0.8, "the visible normals face the camera"
    # AvatarModel.render_mesh: a Camera renders the mesh as it is
    again = model.render_mesh(mesh, cam)
    assert all(torch.equal(again[k], img[k]) for k in img)


def test_rasterize_refuses_cpu_tensors():
    from instantavatar_amd import raster
    L = _L()
    cam = raster.Camera(np.array([[100.0, 0, 8], [0, 100.0, 8], [0, 0, 1]]), torch.eye(4, device=DEV), 16, 16)
    v, f = torch.zeros(8, 3), torch.zeros(4, 3, dtype=torch.int32)
    with pytest.raises(L.IAError):
        raster.rasterize(v, f.to(DEV), cam)
    with pytest.raises(L.IAError):
        raster.rasterize(v.to(DEV), f, cam)
    with pytest.raises(L.IAError):
        raster.rasterize(v.to(DEV), f.to(DEV), cam, attrs=torch.zeros(8, 2))
    empty = raster.rasterize(v.to(DEV), f.to(DEV), cam)          # 4 degenerate faces: an empty frame
    assert not bool(empty.mask.any()) and empty.counts.tolist() == [4, 0]


def _run_driver(args, timeout=300):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m"] + args, env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_extract_mesh_driver_renders(tmp_path):
    import world
    from PIL import Image
    from instantavatar_amd import mesh as M, raster
    from instantavatar_amd.drivers.animate import AnimateSequence
    poses, tr = world.poses(8)
    np.savez(tmp_path / "track.npz", poses=poses[:2], trans=tr[:2])
    out = tmp_path / "out"
    _run_driver(["instantavatar_amd.drivers.extract_mesh", "--synthetic", "--resolution", "64", "--render", "128", "--poses",
                 str(tmp_path / "track.npz"), "--out", str(out)])
    names = ["canonical_front", "posed_0", "posed_1", "posed_shaded_0", "posed_shaded_1"]
    png = {n: np.asarray(Image.open(out / (n + ".png"))) for n in names}
    assert all(p.shape == (128, 128, 4) and p.dtype == np.uint8 for p in png.values())
    # the raster masks of the same meshes, made here (the driver's model is the synthetic model of the same seed)
    from instantavatar_amd.pipeline import build_synthetic_model
    model = build_synthetic_model(DEV, seed=42)[0]
    model.eval()
    mesh = model.extract_mesh(resolution=64)
    masks = {"canonical_front": mesh.render(raster.look_at_box(*M.field_box(model.net_coarse), 128, torch.device(DEV)))["mask"]}
    seq = AnimateSequence(poses[:2], tr[:2], np.zeros(10, np.float32), torch.device(DEV), size=128)
    for i in range(2):
        masks["posed_%d" % i] = masks["posed_shaded_%d" % i] = model.pose_mesh(mesh, seq.batch(i, rays=False)).render(seq.camera())["mask"]
    for n in names:
        m = _np(masks[n])
        assert m.sum() > 300, n
        assert np.array_equal(png[n][..., 3], np.where(m, 255, 0)), n
    assert not np.array_equal(png["posed_0"], png["posed_1"])
    assert (png["posed_shaded_0"][..., 0] == png["posed_shaded_0"][..., 2]).all()
    assert not (out / "posed_2.png").exists()


def test_animate_mesh_preview(tmp_path):
    from PIL import Image
    out = tmp_path / "out"
    stdout = _run_driver(["instantavatar_amd.drivers.animate", "--synthetic", "--mesh-preview", "64", "--size", "128", "--max-frames", "2",
                          "--out", str(out)])
    assert "frames/s" in stdout
    a, b = (np.asarray(Image.open(out / ("mesh_%d.png" % i))) for i in range(2))
    assert a.shape == b.shape == (128, 128, 4) and (a[..., 3] == 255).sum() > 300 and set(np.unique(a[..., 3])) == {0, 255}
    assert not np.array_equal(a, b) and not (out / "0.png").exists() and not (out / "mesh_2.png").exists()
