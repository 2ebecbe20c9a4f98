"""What the surface-normal pass promises without a GPU: the new prototypes are in the header and exported by the library,
every new call refuses CPU tensors with IAError, `render_image_fast` keeps its four values by default, and the points of the
sigma-gradient test stay under its exclusion cap on the float64 reference alone (tests/normal_refs.py)."""
import numpy as np
import pytest
import torch

import normal_refs as nr

NEW = ("ia_surface_points_workspace_bytes", "ia_surface_points", "ia_field_sigma_grad", "ia_candidate_select",
       "ia_normals_from_gradient", "ia_pack_normals8")


def test_new_prototypes_are_declared_and_exported():
    from instantavatar_amd import _lib
    decl = _lib.declarations("normals")         # a header of their own: include/instantavatar_hip_normals.h
    assert set(decl) == set(NEW)                # (disjoint from every other header's: tests/test_cpu_abi_headers.py)
    for name in NEW:
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
    for name in NEW[1:]:
        assert decl[name].stream, name          # every launching entry point takes a stream
    from instantavatar_amd import build
    import os
    assert "ia_normals.hip" in build.SOURCES
    for unit in ("ia_field.hip", "ia_normals.hip"):      # an edit of the shared device header invalidates both source hashes
        assert "ia_field_dev.h" in [os.path.basename(h) for h in build.includes_of(os.path.join(build.CSRC, unit))], unit
    assert os.path.normpath(_lib.header_path("normals")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]


def test_cpu_tensors_raise():
    from instantavatar_amd import _lib
    f = lambda *s: torch.zeros(s)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    b = lambda *s: torch.zeros(s, dtype=torch.uint8)
    R = 8
    grid, field = _lib.SnarfGrid(), _lib.Field()
    calls = {
        "ia_surface_points": (f(R, 3), f(R, 3), f(R), f(R), R, f(R, 3), i(R), i(1), b(256), 256),
        "ia_field_sigma_grad": (f(R, 3), R, None, field, f(R), f(R, 3)),
        "ia_candidate_select": (f(R), f(R, 3), f(R, 3), R, i(R), b(R), R, None, f(R, 3), f(R, 3), None),
        "ia_normals_from_gradient": (f(R, 3), f(R, 3), i(R), R, None, f(96), grid, f(4, 4), R, f(R, 3)),
        "ia_pack_normals8": (f(R, 3), f(R, 3), None, R, b(R, 4), b(R, 4)),
    }
    assert set(calls) == set(NEW[1:])
    for name, args in calls.items():
        with pytest.raises(_lib.IAError, match="GPU"):
            _lib.call(name, *args, None)      # (explicit NULL stream: asking torch for the current one needs a GPU)


def test_python_entry_points_refuse_cpu_tensors():
    from instantavatar_amd import _lib
    from instantavatar_amd.deformers.snarf_deformer import SNARFDeformer
    from instantavatar_amd.deformers.smpl_deformer import SMPLDeformer
    from instantavatar_amd.models.structures.utils import Rays
    from instantavatar_amd.renderers.raymarcher_acc import Raymarcher
    R = 8
    o, d, dep, alp = torch.zeros(R, 3), torch.zeros(R, 3), torch.zeros(R), torch.zeros(R)
    with pytest.raises(_lib.IAError):
        SNARFDeformer.__new__(SNARFDeformer).surface_normals(o, d, dep, alp, None)
    with pytest.raises(_lib.IAError):
        Raymarcher(8, 64).render_normals(Rays(o=o, d=d, near=dep, far=dep), None, None, dep, alp)
    with pytest.raises(NotImplementedError, match="SNARF"):
        SMPLDeformer.__new__(SMPLDeformer).surface_normals(o, d, dep, alp, None)


def test_render_image_fast_keeps_four_values_by_default():
    """the default path gains nothing: same calls, four outputs; normals=True appends the map"""
    from instantavatar_amd.pipeline import AvatarModel
    calls = []

    class Deformer:
        def prepare_deformer(self, batch): calls.append("prepare")
        def transform_rays_w2s(self, rays): calls.append("w2s")
        def surface_normals(self, o, d, depth, alpha, net):
            calls.append("normals")
            return torch.zeros(o.reshape(-1, 3).shape)

    class Grid:
        def initialize(self, deformer, net, jitter=None): calls.append("grid")

    class Renderer(torch.nn.Module):
        density_grid_test = Grid()
        def forward(self, rays, model, eval_mode=True, noise=0, bg_color=None):
            calls.append("render")
            n = rays.o.reshape(-1, 3).shape[0]
            return dict(rgb_coarse=torch.zeros(1, n, 3), depth_coarse=torch.zeros(1, n), alpha_coarse=torch.zeros(1, n), counter_coarse=torch.zeros(1, n))
        def render_normals(self, rays, deformer, net, depth, alpha):
            return deformer.surface_normals(rays.o, rays.d, depth, alpha, net).reshape(rays.o.shape)

    m = AvatarModel(Deformer(), torch.nn.Identity(), Renderer())
    batch = dict(rays_o=torch.zeros(1, 16, 3), rays_d=torch.zeros(1, 16, 3), near=torch.zeros(1, 16), far=torch.ones(1, 16))
    out = m.render_image_fast(dict(batch), (4, 4))
    assert len(out) == 4 and calls == ["prepare", "grid", "w2s", "render"]
    del calls[:]
    out = m.render_image_fast(dict(batch), (4, 4), normals=True)
    assert len(out) == 5 and out[4].shape == (1, 4, 4, 3) and calls == ["prepare", "grid", "w2s", "render", "normals"]
    d = m.forward(dict(batch))
    assert set(d) == {"rgb_coarse", "depth_coarse", "alpha_coarse", "counter_coarse"}


@pytest.mark.parametrize("n_levels", [16, 8])
def test_sigma_gradient_points_stay_under_the_exclusion_cap(n_levels):
    """the cap of tests/test_gpu_normals.py::test_sigma_gradient is a condition on the chosen points: confirmed here on the
    reference alone; the reference's gradient is checked against central differences of its own sigma inside one cell"""
    fp, lv = nr.synthetic_field(n_levels)
    x = nr.box_points(fp)
    ref = nr.sigma_grad_ref(x, fp, lv)
    ex = nr.sigma_grad_excluded(x, fp, lv, ref["h1"])
    print("left out: %.4f of %d points (%d levels)" % (ex.mean(), len(x), n_levels))
    assert ex.mean() <= nr.SG_MAX_EXCLUDED
    assert np.isfinite(ref["grad"]).all() and np.abs(ref["grad"]).max() > 100
    # central differences with a step far below the finest cell (the reference is piecewise trilinear x piecewise linear):
    # agreement wherever no cell face or ReLU kink lies inside the step
    h = 1e-6
    sub = x[:256].astype(np.float64)
    ok = 0
    for a in range(3):
        e = np.zeros(3); e[a] = h
        # (float64 positions: the reference normalises in fp32, so evaluate its pieces directly in float64 here)
        sp = _sigma64(sub + e, fp, lv)
        sm = _sigma64(sub - e, fp, lv)
        fd = (sp - sm) / (2 * h)
        g = ref["grad"][:256, a]
        close = np.abs(fd - g) <= 1e-3 * np.abs(ref["grad"]).max()
        ok += close.sum()
    assert ok >= 0.9 * 3 * 256, ok


def _sigma64(x, fp, lv):
    """sigma of the reference at float64 positions (no fp32 normalisation), same interpolation and weights"""
    import backward_refs as br
    c, s = fp["center"].astype(np.float64), fp["scale"].astype(np.float64)
    xn = np.clip((x - c) / s + 0.5, 0, 1)
    t = np.asarray(fp["table"]).astype(np.float64)
    feat = np.zeros((len(x), 2 * lv.n_levels))
    for l in range(lv.n_levels):
        pos = xn * np.float64(lv.scale[l]) + 0.5
        fl = np.floor(pos)
        w = pos - fl
        g = fl.astype(np.int64).astype(np.uint32)
        size, res = np.uint32(lv.size[l]), np.uint32(lv.res[l])
        for cnr in range(8):
            cx, cy, cz = g[:, 0] + np.uint32(cnr & 1), g[:, 1] + np.uint32((cnr >> 1) & 1), g[:, 2] + np.uint32((cnr >> 2) & 1)
            if lv.hashed[l]:
                i = (cx ^ (cy * np.uint32(2654435761)) ^ (cz * np.uint32(805459861))) & (size - np.uint32(1))
            else:
                i = cx + cy * res + cz * res * res
                i = np.where(i >= size, i - size, i)
                i = np.minimum(i, size - np.uint32(1))
            wt = (w[:, 0] if cnr & 1 else 1 - w[:, 0]) * (w[:, 1] if cnr & 2 else 1 - w[:, 1]) * (w[:, 2] if cnr & 4 else 1 - w[:, 2])
            feat[:, 2 * l:2 * l + 2] += wt[:, None] * t[i.astype(np.int64) + lv.offset[l]]
    W1 = np.asarray(fp["sig_w1"]).astype(np.float64)
    w2 = np.asarray(fp["sig_w2"]).astype(np.float64)[0]
    return np.maximum(feat @ W1.T, 0) @ w2


def test_surface_and_normal_references():
    """the references on cases with known answers: identity transforms give n = -g / |g|; a rotation by w2s^T; a shear"""
    rng = np.random.RandomState(0)
    D = H = W = 3
    vJ = np.zeros((D, H, W, 3, 4))
    vJ[..., :3] = np.eye(3)
    grid = dict(D=D, H=H, W=W, offset=np.zeros(3, np.float32), scale=np.ones(3, np.float32))
    root = rng.uniform(-0.9, 0.9, (50, 3)).astype(np.float32)
    g = rng.normal(size=(50, 3))
    n, det = nr.normals_ref(root, g, vJ.reshape(D, H, W, 12), grid, np.eye(4))
    assert np.allclose(det, 1) and np.allclose(n, -g / np.linalg.norm(g, axis=1, keepdims=True), atol=1e-12)
    A = np.array([[1.0, 0.4, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 2.0]])
    vJ[..., :3] = A
    Rw = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    w2s = np.eye(4); w2s[:3, :3] = Rw
    n, _ = nr.normals_ref(root, g, vJ.reshape(D, H, W, 12), grid, w2s)
    v = -(np.linalg.inv(A).T @ g.T).T
    want = (Rw.T @ (v / np.linalg.norm(v, axis=1, keepdims=True)).T).T
    assert np.allclose(n, want, atol=1e-12)
    n, _ = nr.normals_ref(root + 5, g, vJ.reshape(D, H, W, 12), grid, w2s)      # far outside the grid
    assert (n == 0).all()
    o, d = rng.normal(size=(6, 3)).astype(np.float32), rng.normal(size=(6, 3)).astype(np.float32)
    alpha = np.float32([0.4, 0.5, 1.0, 0.9, np.nan, 0.0])
    depth = np.float32([1.0, 1.0, 2.0, np.nan, 1.0, 0.0])
    pts, idx = nr.surface_points_ref(o, d, depth, alpha)
    assert idx.tolist() == [1, 2] and np.allclose(pts[0], o[1].astype(np.float64) + 2.0 * d[1]) and np.allclose(pts[1], o[2].astype(np.float64) + 2.0 * d[2])
