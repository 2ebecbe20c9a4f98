"""The surface-normal pass (include/instantavatar_hip_normals.h): every new entry point alone
through the C ABI against the float64 references of tests/normal_refs.py, then the whole pass behind a 64 x 64 frame of the
synthetic model -- eager, graph-replayed and pipelined -- and the `--normals` switch of the animate driver."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import backward_refs as br
import normal_refs as nr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# max |got - ref| / max |ref| of d sigma / d x over the points that are compared, measured on MI355X (printed by the test as
# "MEASURED sigma_grad ..."): SG_MEASURED; asserted at 4 x that -- the margin covers the fp32 accumulation order, which depends on
# the lane mapping.  What the figure consists of: the kernel's features are accumulated in half per level (the forward's
# rounding points), so a hidden unit whose pre-activation is within that rounding of zero is masked differently from the
# float64 reference's own mask, and such a unit shifts the gradient by its W2[0][k] W1[k] row.
SG_MEASURED = {16: 2.812e-3, 8: 1.558e-4, "ragged": 3.242e-3}
SG_MARGIN = 4.0
# (the kernel uses no atomics and a fixed reduction order: the figures are the same in every run.)  The max is made of a few
# mask flips; a wrong derivative of one level would move EVERY point, so the median and the 95th percentile of the per-point
# error / max |ref| are asserted beside it, at the same 4 x what was measured: (median, 95th percentile)
SG_MEASURED_PCT = {16: (3.223e-8, 6.652e-8), 8: (3.250e-8, 6.794e-8), "ragged": (3.224e-8, 6.755e-8)}


def _L():
    from instantavatar_amd import _lib
    return _lib


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


_worlds = {}


def _world(n_levels):
    """(model, field dict with the network's own centre / scale, Levels), built once per level count"""
    if n_levels not in _worlds:
        from instantavatar_amd.pipeline import build_synthetic_model
        model, _, fp = build_synthetic_model(DEV, n_levels=n_levels, seed=42)
        fp = dict(fp, center=_np(model.net_coarse.center).astype(np.float32), scale=_np(model.net_coarse.scale).astype(np.float32))
        _worlds[n_levels] = (model, fp, nr.levels_of(fp))
    return _worlds[n_levels]


# ---- 1. sigma gradient ------------------------------------------------------------------------------------------------
def _sigma_grad_case(n_levels, V, n_live, seed, key):
    L = _L()
    model, fp, lv = _world(n_levels)
    net = model.net_coarse
    x = nr.box_points(fp, n=V, seed=seed)
    xd = _dev(x)
    sig, grad = torch.full((V,), 9.0, device=DEV), torch.full((V, 3), 9.0, device=DEV)
    n_dev = None if n_live is None else torch.tensor([n_live], dtype=torch.int32, device=DEV)
    L.call("ia_field_sigma_grad", xd, V, n_dev, net.field_desc(), sig, grad)
    _, sig_fwd = net(xd)                                  # ia_field_fwd
    torch.cuda.synchronize()
    n = V if n_live is None else n_live
    got_s, got_g = _np(sig), _np(grad)
    assert np.array_equal(got_s[:n].view(np.uint32), _np(sig_fwd)[:n].view(np.uint32)), "sigma differs from ia_field_fwd's"
    assert (got_s[n:] == 9.0).all() and (got_g[n:] == 9.0).all(), "rows past the live count were written"
    assert np.isfinite(got_g[:n]).all()
    ref = nr.sigma_grad_ref(x[:n], fp, lv)
    ex = nr.sigma_grad_excluded(x[:n], fp, lv, ref["h1"])
    assert ex.mean() <= nr.SG_MAX_EXCLUDED, ("too many points left out", float(ex.mean()))
    keep = ~ex
    scale = np.abs(ref["grad"][keep]).max()
    err = np.abs(got_g[:n][keep] - ref["grad"][keep]).max() / scale
    serr = np.abs(got_s[:n][keep] - ref["sigma"][keep]).max() / np.abs(ref["sigma"][keep]).max()
    per_point = np.abs(got_g[:n][keep] - ref["grad"][keep]).max(1) / scale
    med, p95 = float(np.median(per_point)), float(np.percentile(per_point, 95))
    print("MEASURED sigma_grad %-8s left out %.4f  max|ref| %.4g  grad err / max|ref| %.3e (median %.3e, 95th percentile %.3e)  "
          "sigma err / max|ref| %.3e" % (key, ex.mean(), scale, err, med, p95, serr))
    assert SG_MEASURED[key] is not None and SG_MEASURED_PCT[key] is not None, "no measured figure recorded for this case"
    assert err <= SG_MARGIN * SG_MEASURED[key], (key, err, SG_MEASURED[key])
    assert med <= SG_MARGIN * SG_MEASURED_PCT[key][0] and p95 <= SG_MARGIN * SG_MEASURED_PCT[key][1], (key, med, p95, SG_MEASURED_PCT[key])


@pytest.mark.parametrize("n_levels", [16, 8])
def test_sigma_gradient(n_levels):
    _sigma_grad_case(n_levels, nr.SG_POINTS, None, nr.SG_SEED, n_levels)


def test_sigma_gradient_ragged():
    _sigma_grad_case(16, 4097, 4001, nr.SG_SEED + 1, "ragged")


# ---- 2. surface points ------------------------------------------------------------------------------------------------
def test_surface_points():
    L = _L()
    H, W = 40, 48
    R = H * W                         # 7.5 workgroups of 256 rays
    rng = np.random.RandomState(5)
    o = rng.uniform(-1, 1, (R, 3)).astype(np.float32)
    d = rng.normal(size=(R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    alpha = rng.uniform(0, 1, R).astype(np.float32)
    depth = (alpha * rng.uniform(3, 6, R)).astype(np.float32)
    half = np.float32(0.5)
    alpha[[3, 300, 1919]] = np.nextafter(half, np.float32(0))      # just below: no point
    alpha[[4, 301, 1918]] = np.nextafter(half, np.float32(1))      # just above
    alpha[[5, 777]] = half                                          # exactly 0.5: a point
    alpha[[6, 1000]] = 0.0                                          # (0 / 0 is never formed)
    depth[6] = 0.0
    alpha[700], depth[700] = 0.9, np.nan                            # NaN depth: no point
    alpha[701] = np.nan                                             # NaN alpha: no point
    alpha[256 * 3:256 * 4] = 0.0                                    # a workgroup without any point
    ref_pts, ref_idx = nr.surface_points_ref(o, d, depth, alpha)
    for i, want in ((3, False), (4, True), (5, True), (6, False), (700, False), (701, False), (1918, True), (1919, False)):
        assert (i in ref_idx) == want, i
    pts, ray = torch.full((R, 3), 9.0, device=DEV), torch.full((R,), -7, dtype=torch.int32, device=DEV)
    n_pts = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    nb = int(L.call("ia_surface_points_workspace_bytes", R))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    L.call("ia_surface_points", _dev(o), _dev(d), _dev(depth), _dev(alpha), R, pts, ray, n_pts, ws, nb)
    torch.cuda.synchronize()
    n = int(n_pts.item())
    assert n == len(ref_idx) and 500 < n < R
    assert np.array_equal(_np(ray)[:n], ref_idx), "ray indices / order"
    assert (_np(ray)[n:] == -7).all() and (_np(pts)[n:] == 9.0).all(), "rows past the count were written"
    got = _np(pts)[:n].astype(np.float64)
    ulp = np.spacing(np.abs(ref_pts).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - ref_pts) <= ulp).all(), float((np.abs(got - ref_pts) / ulp).max())
    with pytest.raises(L.IAError):
        L.call("ia_surface_points", _dev(o), _dev(d), _dev(depth), _dev(alpha), R, pts, ray, n_pts, ws, 0)


# ---- 3. normals from gradients ----------------------------------------------------------------------------------------
def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_normals_from_gradient():
    L = _L()
    rng = np.random.RandomState(11)
    D, H, W = 4, 8, 8
    vJ = np.zeros((D, H, W, 3, 4), np.float32)
    for idx in np.ndindex(D, H, W):
        vJ[idx][:, :3] = _rotation(rng) + rng.normal(scale=0.05, size=(3, 3))
        vJ[idx][:, 3] = rng.normal(scale=0.3, size=3)
    vJ[1:3, 2:4, 5:7, 0, :3] = 0.0           # the eight corners of cell (x 5, y 2, z 1): first row zero -> the blend is exactly singular
    grid = dict(D=D, H=H, W=W, offset=np.array([0.05, -0.02, 0.01], np.float32), scale=np.array([0.9, 1.1, 1.0], np.float32))
    n = 2000
    root = rng.uniform(-1.8, 1.8, (n, 3)).astype(np.float32)        # grid spans about [-1.1, 1.1]: roots inside, on the rim, far outside
    cell = lambda i, s: -1 + 2 * (i + rng.uniform(0.1, 0.9, 20)) / (s - 1)
    sing = np.stack([cell(5, W), cell(2, H), cell(1, D)], 1)         # normalised coordinates inside the singular cell
    root[:20] = (sing / grid["scale"] - grid["offset"]).astype(np.float32)
    grad = (rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 4, (n, 1))).astype(np.float32)
    grad[20:60] = 0.0                                                # zero gradients
    grad[60:70] *= np.float32(1e-30)                                 # tiny and huge, finite
    grad[70:80] *= np.float32(1e30)
    ray = rng.permutation(3000)[:n].astype(np.int32)                 # scattered into a map of 3001 rays: 9003 words, so the
    R = 3001                                                         # zero-fill's 16-byte body AND its tail of three words run
    w2s = np.eye(4, dtype=np.float32)
    w2s[:3, :3] = _rotation(rng)
    w2s[:3, 3] = [0.3, -0.2, 4.0]
    ref, det = nr.normals_ref(root, grad, vJ.reshape(D, H, W, 12), grid, w2s)
    assert (det[:20] == 0).all() and (ref[:20] == 0).all()
    gd = L.SnarfGrid()
    gd.D, gd.H, gd.W = D, H, W
    gd.offset[:], gd.scale[:] = grid["offset"].tolist(), grid["scale"].tolist()
    out = torch.full((R, 3), float("nan"), device=DEV)               # whatever the call does not write must have been zero-filled
    n_dev = torch.tensor([n - 100], dtype=torch.int32, device=DEV)   # the last 100 points are not live
    L.call("ia_normals_from_gradient", _dev(root), _dev(grad), _dev(ray), n, n_dev, _dev(vJ.reshape(-1)), gd, _dev(w2s), R, out)
    torch.cuda.synchronize()
    got = _np(out).astype(np.float64)
    assert np.isfinite(got).all()
    want = np.zeros((R, 3))
    live = np.arange(n) < n - 100
    want[ray[live]] = ref[live]
    zero = (want == 0).all(1)
    outside = (np.abs((root + grid["offset"]) * grid["scale"]) > 1 + 2.0 / 3).any(1)
    assert zero.sum() > R - n + 100 + 60 and (outside & live).sum() > 100 and (~zero).sum() > 500
    assert (got[zero] == 0).all(), "a pixel without a normal is not exactly zero"
    assert np.abs(got[~zero] - want[~zero]).max() <= 1e-5, float(np.abs(got[~zero] - want[~zero]).max())
    assert np.abs(np.linalg.norm(got[~zero], axis=1) - 1).max() <= 1e-6
    # a small map, far more pixels than points: 301 rays (903 words: less than one workgroup of 16-byte stores, and a tail), 200 points
    R2, n2 = 301, 200
    ray2 = rng.permutation(R2)[:n2].astype(np.int32)
    out2 = torch.full((R2, 3), float("nan"), device=DEV)
    L.call("ia_normals_from_gradient", _dev(root[:n2]), _dev(grad[:n2]), _dev(ray2), n2, None, _dev(vJ.reshape(-1)), gd, _dev(w2s), R2, out2)
    torch.cuda.synchronize()
    got2 = _np(out2).astype(np.float64)
    want2 = np.zeros((R2, 3))
    want2[ray2] = ref[:n2]
    zero2 = (want2 == 0).all(1)
    assert zero2.sum() >= R2 - n2 + 60 and (~zero2).sum() > 10
    assert np.array_equal(got2[zero2], np.zeros((int(zero2.sum()), 3))), "a pixel without a normal is not exactly zero (small map)"
    assert np.abs(got2[~zero2] - want2[~zero2]).max() <= 1e-5


# ---- the 8-bit images -------------------------------------------------------------------------------------------------
def test_pack_normals8():
    L = _L()
    rng = np.random.RandomState(3)
    R = 1000
    nrm = rng.normal(size=(R, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[::7] = 0.0
    d = rng.normal(size=(R, 3)).astype(np.float32)
    q = lambda v: (np.clip(v, np.float32(0), np.float32(1)).astype(np.float32) * np.float32(255)).astype(np.uint8)
    for light in (None, np.array([0.0, 0.0, -2.0], np.float32)):
        a, b = torch.full((R, 4), 7, dtype=torch.uint8, device=DEV), torch.full((R, 4), 7, dtype=torch.uint8, device=DEV)
        L.call("ia_pack_normals8", _dev(nrm), _dev(d), None if light is None else _dev(light), R, a, b)
        torch.cuda.synchronize()
        has = (nrm != 0).any(1)
        l = -d if light is None else np.broadcast_to(light, (R, 3))
        l = l.astype(np.float64) / np.linalg.norm(l.astype(np.float64), axis=1, keepdims=True)
        s = np.maximum((nrm.astype(np.float64) * l).sum(1), 0.0)
        na, sb = _np(a), _np(b)
        assert (na[~has] == 0).all() and (sb[~has] == 0).all()
        assert (na[has, 3] == 255).all() and (sb[has, 3] == 255).all()
        assert np.array_equal(na[has, :3], q((nrm[has] + np.float32(1)) * np.float32(0.5)))
        assert np.abs(sb[has, 0].astype(int) - np.floor(s[has] * 255)).max() <= 1          # (one step: s is formed in fp32)
        assert (sb[has, 0] == sb[has, 1]).all() and (sb[has, 0] == sb[has, 2]).all()


# ---- 4. whole pass ----------------------------------------------------------------------------------------------------
WHOLE_RES, WHOLE_FRAMES = 64, (0, 5)
# angular error (radians) between the product's map and the host reference over the pixels whose winning candidate is the
# oracle's, 99th percentile over the pixels of both frames, measured on MI355X ("MEASURED whole pass ..."); asserted at 2 x.
# The pixels whose arg-max candidate differs from the oracle's are counted and capped, not compared.
WHOLE_P99_MEASURED = 1.306e-3
WHOLE_MAX_MISMATCH = 0.005


def _whole_world():
    import world
    return world.build(DEV, 64, 16)       # (model, body, field dict, the deformer's state for the oracle), shared with the parity tests


def _whole_reference(orc, body, fp, init, pose72, transl, o_cam, d_cam, depth, alpha):
    """the map assembled on the host from the product's own depth / alpha: surface points (normal_refs), `oracle.search` +
    `oracle.field_fwd` + arg-max over the valid candidates for the roots, normal_refs for gradient, blend and rotation.
    -> (normals [R,3] float64, root [R,3] of the pixels with a valid candidate, has [R])"""
    import world
    from instantavatar_amd import synthetic as syn
    W = world.oracle_world(orc, body, fp, init, pose72, transl)
    o2, d2, _, _ = orc.transform_rays_w2s(o_cam, d_cam, W["w2s"])
    pts, idx = nr.surface_points_ref(o2, d2, depth, alpha)
    x, valid, _, _ = orc.search(pts.astype(np.float32), W["voxel_J"], W["tfs"], init, syn.INIT_BONES)
    P, k = valid.shape
    _, sig = orc.field_fwd(W["field"], x.reshape(-1, 3))
    sig = np.where(np.isfinite(sig), sig, np.float32(0)).reshape(P, k)
    sig = np.where(valid != 0, sig, -np.inf)
    arg = sig.argmax(1)                                              # first maximum
    has = (valid != 0).any(1)
    root = np.where(has[:, None], x[np.arange(P), arg], 0).astype(np.float32)
    grad = nr.sigma_grad_ref(root, fp, nr.levels_of(fp))["grad"]
    grad[~has] = 0
    vJ = np.ascontiguousarray(np.transpose(W["voxel_J"], (1, 2, 3, 0)))      # reference layout [12,D,H,W] -> channel-last
    grid = dict(D=init["D"], H=init["H"], W=init["W"], offset=init["offset_kernel"], scale=init["scale_kernel"])
    n, _ = nr.normals_ref(root, grad, vJ, grid, W["w2s"])
    R = len(o_cam)
    out, r_out, h_out = np.zeros((R, 3)), np.zeros((R, 3), np.float32), np.zeros(R, bool)
    out[idx], r_out[idx], h_out[idx] = n, root, has
    return out, r_out, h_out, idx


def test_whole_pass_eager_graph_pipelined(oracle):
    from instantavatar_amd.drivers.animate import fixed_jitter
    from instantavatar_amd.pipeline import GraphedRenderer, PipelinedRenderer, make_batch
    from instantavatar_amd.models.structures.utils import Rays
    import world
    model, body, fp, init = _whole_world()
    res = WHOLE_RES
    poses, tr = world.poses(8)
    batches = [make_batch(DEV, res, poses[i], tr[i]) for i in WHOLE_FRAMES]
    jitter = fixed_jitter(1, DEV)
    eager, angles = [], []
    for f, b in zip(WHOLE_FRAMES, batches):
        four = model.render_image_fast(dict(b), (res, res), jitter=jitter)
        five = model.render_image_fast(dict(b), (res, res), jitter=jitter, normals=True)
        assert len(four) == 4 and len(five) == 5
        for u, v in zip(four, five):
            assert torch.equal(u, v), "the frame changed with normals=True"
        eager.append([t.clone() for t in five])
        # the same pass once more with its roots (the deformer is still prepared for this frame)
        rays = Rays(o=b["rays_o"], d=b["rays_d"], near=b["near"], far=b["far"])
        model.deformer.transform_rays_w2s(rays)
        again, roots = model.deformer.surface_normals(rays.o, rays.d, five[1], five[2], model.net_coarse, want_roots=True)
        assert torch.equal(again.reshape(five[4].shape), five[4])
        torch.cuda.synchronize()
        rgb, depth, alpha, counter, nrm = five
        assert nrm.shape == (1, res, res, 3) and nrm.dtype == torch.float32 and bool(torch.isfinite(nrm).all())
        got = _np(nrm).reshape(-1, 3).astype(np.float64)
        a, dep = _np(alpha).reshape(-1), _np(depth).reshape(-1)
        ref, ref_root, ref_has, idx = _whole_reference(oracle, body, fp, init, poses[f], tr[f], _np(b["rays_o"])[0], _np(b["rays_d"])[0], dep, a)
        n_pts = int(roots["n"].item())
        assert n_pts == len(idx) > 200 and np.array_equal(_np(roots["ray"])[:n_pts], idx), "surface points differ from the reference's"
        got_root = np.zeros_like(ref_root)
        got_root[idx] = _np(roots["root"])[:n_pts]
        ln = np.linalg.norm(got, axis=1)
        hit = np.zeros(len(a), bool)
        hit[idx] = True
        # pixels whose winner is another candidate than the oracle's (or that have a candidate in one of the two only)
        same = hit & ref_has & (np.abs(got_root - ref_root).max(1) <= 1e-3) & (ln > 0)
        agree_none = hit & ~ref_has & (ln == 0)
        mismatch = hit & ~same & ~agree_none
        assert (ln[~hit] == 0).all(), "a normal where alpha < 0.5"
        assert np.abs(ln[ln > 0] - 1).max() <= 1e-6
        assert (ln[same] > 0).all() and (np.linalg.norm(ref[same], axis=1) > 0).all()
        ang = np.arccos(np.clip((got[same] * ref[same]).sum(1), -1, 1))
        p99 = float(np.percentile(ang, 99))
        print("MEASURED whole pass frame %d: %d hit pixels, %d compared, %d without a candidate in both, %d mismatched (cap %.1f); angular "
              "error rad: median %.3e  99th percentile %.3e  max %.3e" % (f, hit.sum(), same.sum(), agree_none.sum(), mismatch.sum(),
                                                                          WHOLE_MAX_MISMATCH * hit.sum(), np.median(ang), p99, ang.max()))
        assert same.sum() > 0.9 * hit.sum()
        assert mismatch.sum() <= WHOLE_MAX_MISMATCH * hit.sum(), (int(mismatch.sum()), int(hit.sum()))
        angles.append(ang)
    p99 = float(np.percentile(np.concatenate(angles), 99))
    print("MEASURED whole pass, both frames: %d pixels compared, angular error 99th percentile %.3e rad" % (sum(map(len, angles)), p99))
    assert WHOLE_P99_MEASURED is not None, "no measured figure recorded"
    assert p99 <= 2 * WHOLE_P99_MEASURED, (p99, WHOLE_P99_MEASURED)
    graphed = GraphedRenderer(model, dict(batches[0]), (res, res), warmup=2, margin=2, sync_check=True, jitter=jitter, normals=True)
    for b, want in zip(batches, eager):
        out = graphed(b)
        torch.cuda.synchronize()
        assert len(out) == 5
        for u, v in zip(out, want):
            assert torch.equal(u, v), "graph replay differs from the eager frame"
    assert graphed.finish() == 0
    piped = PipelinedRenderer(model, dict(batches[0]), (res, res), n_in_flight=2, margin=2, jitter=jitter, normals=True)
    kept = []
    for b in batches + batches:
        piped(b, consume=lambda out, k: kept.append([t.clone() for t in out]))
    piped.synchronize()
    assert piped.finish() == 0
    for got_f, want in zip(kept, eager + eager):
        assert len(got_f) == 5
        for u, v in zip(got_f, want):
            assert torch.equal(u, v), "pipelined frame differs from the eager frame"


def test_smpl_deformer_has_no_normal_pass():
    from instantavatar_amd.deformers.smpl_deformer import SMPLDeformer
    d = SMPLDeformer.__new__(SMPLDeformer)
    with pytest.raises(NotImplementedError, match="SNARF"):
        d.surface_normals(None, None, None, None, None)


# ---- 5. driver --------------------------------------------------------------------------------------------------------
def test_animate_normals_switch(tmp_path):
    from PIL import Image
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "instantavatar_amd.drivers.animate", "--synthetic", "--size", "64", "--max-frames", "3", "--no-gif",
            "--jitter-seed", "1"]
    for name, extra in (("plain", []), ("normals", ["--normals"])):
        r = subprocess.run(base + extra + ["--out", str(tmp_path / name)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    for i in range(3):
        a, b = (tmp_path / "plain" / ("%d.png" % i)).read_bytes(), (tmp_path / "normals" / ("%d.png" % i)).read_bytes()
        assert a == b, "frame %d changed with --normals" % i
        assert not (tmp_path / "plain" / ("normal_%d.png" % i)).exists()
        n_img = np.asarray(Image.open(tmp_path / "normals" / ("normal_%d.png" % i)))
        s_img = np.asarray(Image.open(tmp_path / "normals" / ("shaded_%d.png" % i)))
        assert n_img.shape == (64, 64, 4) and s_img.shape == (64, 64, 4)
        cov = n_img[..., 3] == 255
        assert 200 < cov.sum() < 64 * 64 and np.array_equal(cov, s_img[..., 3] == 255)
        assert (n_img[~cov] == 0).all() and s_img[cov][:, 0].mean() > 64, "the shaded body is lit from the camera"
