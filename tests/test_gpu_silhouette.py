"""The soft-silhouette entries, called through the C ABI (`_lib.call`, plain device tensors) on the seeded cases of
tests/silhouette_refs.py and compared per element with its float64 restatement: ia_sil_project_fwd / _bwd, ia_sil_render_fwd / _bwd
(csrc/ia_silhouette.hip) and ia_sil_body_bwd (csrc/ia_keypoints.hip).  Every stage's reference takes the KERNEL's fp32 output of the
stage before it as exact input.  The bound is derived in silhouette_refs.py; tests/test_cpu_silhouette_refs.py shows on the CPU that
the reference is right, that a second fp32 association stays inside the bound and that eight seeded defects do not.  Every output
buffer carries a sentinel row behind its last row and every workspace a sentinel tail behind NaN bits.  Each comparison prints
"SILREF ..." lines: the figures recorded in silhouette_refs.MEASURED.  Then SoftSilhouette / the autograd function,
`SilhouetteRefiner.refine`, and the driver on a small sequence directory."""
import functools
import os

import numpy as np
import pytest
import torch

import keypoint_refs as kr
import silhouette_refs as sf
import smpl_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.25
WS_TAIL = 64


def _lib():
    from instantavatar_amd import _lib as L
    return L


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _out(rows, *rest):
    return torch.full((rows + 1,) + rest, SENTINEL, device=DEV)


def _take(t, rows, what):
    a = _np(t)
    assert (a[rows:] == SENTINEL).all(), what + ": written behind its last row"
    return a[:rows]


class _Case:
    def __init__(self, name):
        L = _lib()
        self.name, self.i = name, sf.inputs(name)
        i = self.i
        self.nv, self.nf, self.H, self.W = len(i["verts"]), len(i["faces"]), i["H"], i["W"]
        self.verts, self.faces, self.w2c, self.mask = _dev(i["verts"]), _dev(i["faces"].reshape(-1, 3)), _dev(i["w2c"]), _dev(i["mask"])
        self.cam = tuple(float(np.float32(c)) for c in i["cam"])
        self.sigma, self.blur = float(i["sigma"]), float(i["blur"])
        self.need = int(L.call("ia_sil_workspace_bytes", self.nv, self.nf, self.H, self.W))
        self.vf = tuple(_dev(a) for a in sf.vertex_faces(i["faces"], self.nv))
        self.raw = {}

    def workspace(self):
        return torch.full((self.need + WS_TAIL,), 255, dtype=torch.uint8, device=DEV)

    def _ws_ok(self, ws, what):
        torch.cuda.synchronize()
        assert (_np(ws[-WS_TAIL:]) == 255).all(), what + " wrote behind the workspace"

    def project(self):
        screen, inv_z = _out(self.nv, 2), _out(self.nv)
        self.raw = dict(screen=screen, inv_z=inv_z)
        _lib().call("ia_sil_project_fwd", self.verts, self.nv, self.w2c, *self.cam, screen, inv_z)
        return _take(screen, self.nv, "screen"), _take(inv_z, self.nv, "inv_z")

    def project_bwd(self, d_screen):
        d_verts = _out(self.nv, 3)
        self.raw = dict(d_verts=d_verts)
        _lib().call("ia_sil_project_bwd", self.verts, self.nv, self.w2c, *self.cam, _dev(d_screen), d_verts)
        return _take(d_verts, self.nv, "d_verts")

    def render(self, screen, inv_z, ws, mask=True, alpha=True, loss=True, d_alpha=True, ws_bytes=None, **over):
        n = self.H * self.W
        o = dict(alpha=_out(n) if alpha else None, loss=_out(1) if loss else None, d_alpha=_out(n) if d_alpha else None)
        self.raw = o
        a = dict(nv=self.nv, nf=self.nf, H=self.H, W=self.W, sigma=self.sigma, blur=self.blur)
        a.update(over)
        _lib().call("ia_sil_render_fwd", _dev(screen), _dev(inv_z), a["nv"], self.faces, a["nf"], a["H"], a["W"], a["sigma"], a["blur"],
                    self.mask if mask else None, o["alpha"], o["loss"], o["d_alpha"], ws, self.need if ws_bytes is None else ws_bytes)
        self._ws_ok(ws, "render forward")
        return {k: _take(t, 1 if k == "loss" else n, self.name + " " + k) for k, t in o.items() if t is not None}

    def render_bwd(self, screen, inv_z, alpha, d_alpha, ws, ws_bytes=None, **over):
        d_screen = _out(self.nv, 2)
        self.raw = dict(d_screen=d_screen)
        a = dict(nv=self.nv, nf=self.nf, H=self.H, W=self.W, sigma=self.sigma, blur=self.blur)
        a.update(over)
        _lib().call("ia_sil_render_bwd", _dev(screen), _dev(inv_z), a["nv"], self.faces, a["nf"], a["H"], a["W"], a["sigma"], a["blur"], _dev(alpha),
                    _dev(d_alpha), self.vf[0], self.vf[1], d_screen, ws, self.need if ws_bytes is None else ws_bytes)
        self._ws_ok(ws, "render backward")
        return _take(d_screen, self.nv, "d_screen")


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


def _elem(ref, m):
    return (ref, sf.K_BOUND * sf.U * m, sf.U * m, 0 * m)


def _check(got, bound, what):
    over, worst = sf.check(got, bound, what)
    assert not over, (what, "error / allow", over)
    return worst


# ---- every stage against the float64 reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sf.CASES))
def test_every_stage_within_the_bound(name):
    """projection, render (alpha, loss, d_alpha), render backward (d_screen) and projection backward (d_verts), each on the kernel's
    own output of the stage before, each on a workspace freshly filled with NaN bits"""
    c, i = _case(name), sf.inputs(name)
    screen, inv_z = c.project()
    pr = sf.project_ref(i["verts"], i["w2c"], i["cam"])
    assert np.array_equal(inv_z > 0, pr["valid"]) and (screen[~pr["valid"]] == 0).all()
    _check(dict(screen=screen, inv_z=inv_z), {"screen": _elem(pr["screen"], pr["m_screen"]), "inv_z": _elem(pr["inv_z"], pr["m_inv_z"])}, "proj " + name)
    r = c.render(screen, inv_z, c.workspace())
    R = sf.render_ref(screen, inv_z, i["faces"], c.H, c.W, i["sigma"], i["blur"], i["mask"])
    fb, share = sf.fwd_bound(R)
    assert share <= sf.ALLOW_CAP
    _check(r, fb, "fwd " + name)
    d_screen = c.render_bwd(screen, inv_z, r["alpha"], r["d_alpha"], c.workspace())
    B = sf.render_bwd_ref(R, r["alpha"], r["d_alpha"])
    _check(dict(d_screen=d_screen), B["bound"], "bwd " + name)
    d_verts = c.project_bwd(d_screen)
    pb = sf.project_bwd_ref(i["verts"], i["w2c"], i["cam"], d_screen)
    assert (d_verts[~pr["valid"]] == 0).all()
    _check(dict(d_verts=d_verts), {"d_verts": _elem(pb["d_verts"], pb["m_d_verts"])}, "projb " + name)
    if name == "one-triangle":
        assert (r["alpha"] == 1).all() and (d_screen == 0).all()
    if name == "no-faces":
        assert (r["alpha"] == 0).all() and (d_screen == 0).all()


def test_two_calls_give_the_same_bits_and_null_outputs_change_nothing():
    c = _case("tubes-33x70")
    screen, inv_z = c.project()
    s2, z2 = c.project()
    assert np.array_equal(_bits(screen), _bits(s2)) and np.array_equal(_bits(inv_z), _bits(z2))
    first = c.render(screen, inv_z, c.workspace())
    again = c.render(screen, inv_z, c.workspace())
    assert all(np.array_equal(_bits(first[k]), _bits(again[k])) for k in first), "two forward calls differ"
    for null in ("alpha", "loss", "d_alpha"):
        r = c.render(screen, inv_z, c.workspace(), **{null: False})
        assert set(r) == set(first) - {null} and all(np.array_equal(_bits(r[k]), _bits(first[k])) for k in r), null + " = NULL changes the others"
    bare = c.render(screen, inv_z, c.workspace(), mask=False, loss=False, d_alpha=False)
    assert set(bare) == {"alpha"} and np.array_equal(_bits(bare["alpha"]), _bits(first["alpha"]))
    g = c.render_bwd(screen, inv_z, first["alpha"], first["d_alpha"], c.workspace())
    assert np.array_equal(_bits(g), _bits(c.render_bwd(screen, inv_z, first["alpha"], first["d_alpha"], c.workspace()))), "two backward calls differ"
    dv = c.project_bwd(g)
    assert np.array_equal(_bits(dv), _bits(c.project_bwd(g)))


def test_argument_errors_raise_and_write_nothing():
    L = _lib()
    c = _case("tubes-40x48")
    screen, inv_z = c.project()
    ws = c.workspace()
    r = c.render(screen, inv_z, ws)

    def refused(match, **over):
        for call in (lambda **kw: c.render(screen, inv_z, ws, **kw), lambda **kw: c.render_bwd(screen, inv_z, r["alpha"], r["d_alpha"], ws, **kw)):
            ws.fill_(255)
            with pytest.raises(L.IAError, match=match):
                call(**over)
            torch.cuda.synchronize()
            assert all((_np(t) == SENTINEL).all() for t in c.raw.values() if t is not None), match + ": an output was written"
            assert (_np(ws) == 255).all(), match + ": the workspace was written"

    refused("workspace", ws_bytes=c.need - 1)
    refused("outside", H=0)
    refused("outside", W=16385)
    refused("outside", nf=-1)
    refused("sigma", sigma=0.0)
    refused("sigma", sigma=float("nan"))
    refused("blur_radius", blur=-1.0)
    with pytest.raises(L.IAError, match="mask"):
        c.render(screen, inv_z, ws, mask=False)
    with pytest.raises(L.IAError, match="near"):
        L.call("ia_sil_project_fwd", c.verts, c.nv, c.w2c, c.cam[0], c.cam[1], c.cam[2], c.cam[3], 0.0, _out(c.nv, 2), _out(c.nv))
    assert L.call("ia_sil_workspace_bytes", 5, 5, 0, 5) == 0 and L.call("ia_sil_workspace_bytes", 5, 5, 5, 16385) == 0
    assert L.call("ia_sil_workspace_bytes", 5, 1 << 30, 5, 5) == 0 and L.call("ia_sil_workspace_bytes", -1, 5, 5, 5) == 0
    assert L.call("ia_sil_body_workspace_bytes", 0, 5) == 0 and L.call("ia_sil_body_workspace_bytes", 1 << 20, 1 << 10) == 0
    again = c.render(screen, inv_z, c.workspace())
    assert all(np.array_equal(_bits(r[k]), _bits(again[k])) for k in r)


def test_a_damaged_vertex_list_is_ignored_not_dereferenced():
    """offsets and entries outside their range contribute nothing and nothing is read through them"""
    c = _case("tubes-40x48")
    screen, inv_z = c.project()
    r = c.render(screen, inv_z, c.workspace())
    good = c.render_bwd(screen, inv_z, r["alpha"], r["d_alpha"], c.workspace())
    start, corner = (a.copy() for a in sf.vertex_faces(c.i["faces"], c.nv))
    v = 7
    lost = corner[start[v]]
    corner[start[v]] = 3 * c.nf + 5
    start[20], start[21] = start[21], start[20]            # descending: vertex 20 is left empty (and 19, 21 see a changed range)
    keep, c.vf = c.vf, (_dev(start), _dev(corner))
    try:
        bad = c.render_bwd(screen, inv_z, r["alpha"], r["d_alpha"], c.workspace())
    finally:
        c.vf = keep
    assert np.isfinite(bad).all() and (bad[20] == 0).all()
    same = np.ones(c.nv, bool)
    same[[v, 19, 20, 21]] = False
    assert np.array_equal(_bits(bad[same]), _bits(good[same])) and lost >= 0


# ---- the body-model adjoint ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("f1-v257-smpl", "f3-v257-smpl", "f9-v257-star"))
def test_body_adjoint_within_the_bound(name):
    """d_betas, d_pose, d_transl for a seeded vertex cotangent on the bodies of keypoint_refs, in its groups and with its K; twice for the
    same bits; NULL outputs change nothing; arguments outside the limits raise"""
    L = _lib()
    i = kr.inputs(name)
    F, V = i["pose"].shape[0], i["body"]["v_template"].shape[0]
    t = {k: _dev(i["body"][k]) for k in sr.BODY_KEYS}
    body = L.SmplBody()
    for k in sr.BODY_KEYS:
        setattr(body, k, t[k].data_ptr())
    body.n_verts = V
    g = np.random.default_rng(77)
    dv = (g.standard_normal((F, V, 3)) * g.uniform(0, 1, (F, V, 1)) ** 4).astype(np.float32)
    dv[:, ::5] = 0
    d = {k: _dev(i[k]) for k in ("betas", "pose", "transl")}
    need = L.call("ia_sil_body_workspace_bytes", F, V)
    assert need == L.call("ia_kp_workspace_bytes", F, V) > 0
    dvd = _dev(dv)

    def run(d_betas=True, d_pose=True, d_transl=True, ws_bytes=None, n_frames=F):
        ws = torch.full((need + WS_TAIL,), 255, dtype=torch.uint8, device=DEV)
        o = dict(d_betas=_out(10) if d_betas else None, d_pose=_out(F, 72) if d_pose else None, d_transl=_out(F, 3) if d_transl else None)
        run.raw, run.ws = o, ws
        L.call("ia_sil_body_bwd", body, d["betas"], d["pose"], d["transl"], n_frames, dvd, o["d_betas"], o["d_pose"], o["d_transl"], ws,
               need if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        assert (_np(ws[-WS_TAIL:]) == 255).all()
        return {k: _take(v, {"d_betas": 10}.get(k, F), k) for k, v in o.items() if v is not None}

    r = run()
    bound, _ = sf.body_bwd_bound(i["body"], i["betas"], i["pose"], i["transl"], dv)
    over, worst = kr.compare(kr.bwd_groups(r), bound, "SILREF body " + name)
    assert not over, over
    assert all(np.array_equal(_bits(r[k]), _bits(v)) for k, v in run().items()), "two calls differ"
    for null in ("d_betas", "d_pose", "d_transl"):
        q = run(**{null: False})
        assert set(q) == set(r) - {null} and all(np.array_equal(_bits(q[k]), _bits(r[k])) for k in q)
    for kw, match in ((dict(ws_bytes=need - 1), "workspace"), (dict(n_frames=0), "n_frames")):
        with pytest.raises(L.IAError, match=match):
            run(**kw)
        torch.cuda.synchronize()
        assert all((_np(v) == SENTINEL).all() for v in run.raw.values()) and (_np(run.ws) == 255).all()


# ---- SoftSilhouette and the autograd function ----------------------------------------------------------------------------------------
def _camera(i):
    from instantavatar_amd.raster import Camera
    fx, fy, cx, cy, near = i["cam"]
    return Camera(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), _dev(i["w2c"]), i["H"], i["W"], near=near)


def test_module_and_autograd_function_give_the_direct_calls_results():
    from instantavatar_amd.silhouette import SoftSilhouette, soft_silhouette, default_blur_radius
    c, i = _case("tubes-33x70"), sf.inputs("tubes-33x70")
    screen, inv_z = c.project()
    r = c.render(screen, inv_z, c.workspace())
    d_verts = c.project_bwd(c.render_bwd(screen, inv_z, r["alpha"], r["d_alpha"], c.workspace()))
    s = SoftSilhouette(c.faces, _camera(i), sigma=c.sigma, blur_radius=c.blur)
    assert SoftSilhouette(c.faces, _camera(i)).blur_radius == default_blur_radius(1e-4) == sf.default_blur(1e-4)
    alpha = s.render(c.verts)
    assert alpha.shape == (c.H, c.W) and np.array_equal(_bits(_np(alpha).reshape(-1)), _bits(r["alpha"]))
    loss, g = s.loss_and_grad(c.verts, c.mask.view(c.H, c.W))
    assert np.array_equal(_bits(_np(loss).reshape(1)), _bits(r["loss"])) and np.array_equal(_bits(_np(g)), _bits(d_verts))
    v = c.verts.clone().requires_grad_(True)
    a = soft_silhouette(v * 1.0, c.faces, _camera(i), sigma=c.sigma, blur_radius=c.blur)
    ((a - c.mask.view(c.H, c.W)) ** 2).mean().backward()
    # torch forms 2 (alpha - m) / (H W) in its own order: the same d_alpha to a rounding, so the same d_verts to the bound of the
    # backward stages on the perturbed cotangent; with the kernel's own d_alpha handed in, the bits are the direct call's
    assert np.allclose(_np(v.grad), d_verts, rtol=1e-4, atol=1e-4 * np.abs(d_verts).max())
    v2 = c.verts.clone().requires_grad_(True)
    soft_silhouette(v2, c.faces, _camera(i), sigma=c.sigma, renderer=s).backward(_dev(r["d_alpha"]).view(c.H, c.W))
    assert np.array_equal(_bits(_np(v2.grad)), _bits(d_verts))


# ---- SilhouetteRefiner ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refine_case():
    """the smallest make_mesh_body, 3 frames of 48 x 48; masks = the float64 reference's alpha at the true poses, quantised to bytes;
    the start = the true poses with every joint moved by 0.03 rad in a seeded direction and the translation by 1.5 cm"""
    from instantavatar_amd import synthetic
    d = synthetic.make_mesh_body(sides=3, rings=2)
    Jreg = d["J_regressor"].astype(np.float64)
    body = dict(v_template=d["v_template"], shapedirs=d["shapedirs"], posedirs=d["posedirs"], lbs_weights=d["lbs_weights"],
                J0=(Jreg @ d["v_template"]).astype(np.float32), JS=np.einsum("ji,ikl->jkl", Jreg, d["shapedirs"]).astype(np.float32),
                parents=np.asarray(d["parents"]).astype(np.int32))
    body["parents"][0] = -1
    F, H, W, sigma = 3, 48, 48, 1e-3
    pose, transl = synthetic.procedural_pose_track(F)
    transl = transl.copy()
    transl[:, 2] = 3.0
    betas = np.zeros(10, np.float32)
    w2c = np.eye(4, dtype=np.float32)
    cam = (60.0, 60.0, 23.5, 23.5, 0.05)
    g = np.random.default_rng(12)
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    pose0 = (pose.reshape(F, 24, 3) + 0.03 * unit(g.standard_normal((F, 24, 3)))).reshape(F, 72).astype(np.float32)
    transl0 = (transl + 0.015 * unit(g.standard_normal((F, 3)))).astype(np.float32)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    masks = []
    for f in range(F):
        with np.errstate(divide="ignore", invalid="ignore"):
            verts = kr.kp_fwd_ref(body, betas, pose[f:f + 1], transl[f:f + 1], eye, np.zeros((1, 25, 3)), kr.THRESHOLD, np.zeros(11, np.int64))["verts"][0]
        pr = sf.project_ref(verts.astype(np.float32), w2c, cam)
        a = sf.render_ref(pr["screen"].astype(np.float32), pr["inv_z"].astype(np.float32), d["f"], H, W, sigma, sf.default_blur(sigma))["alpha"]
        masks.append(np.round(a * 255).astype(np.uint8).reshape(H, W))
    return dict(body_dict=d, betas=betas, pose=pose0, transl=transl0, masks=np.stack(masks), w2c=w2c, cam=cam, H=H, W=W, sigma=sigma)


def _iou(a, b):
    a, b = a >= 0.5, b >= 0.5
    return float((a & b).sum()) / max(float((a | b).sum()), 1.0)


def test_refine_lowers_every_frames_loss():
    """the first closure evaluation is loss_and_grad; every frame's final loss is strictly below its initial loss (a strong-Wolfe line
    search only accepts a decrease); the IoU of alpha >= 0.5 with the target does not fall; the inputs, betas and the frames that are not
    refined keep their bits.  The reduction is recorded in the docstring of silhouette_refs.py, not gated."""
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.silhouette import SilhouetteRefiner
    i = _refine_case()
    body = SMPL.from_dict(i["body_dict"]).to(DEV)
    cam = _camera(dict(cam=i["cam"], w2c=i["w2c"], H=i["H"], W=i["W"]))
    r = SilhouetteRefiner(body, body.faces_tensor, cam, i["masks"], sigma=i["sigma"])
    b0, p0, t0 = (_dev(i[k]) for k in ("betas", "pose", "transl"))
    keep = [x.clone() for x in (b0, p0, t0)]
    target = i["masks"].astype(np.float32) / 255
    alpha0 = [_np(r.sil.render(r._posed(b0, p0[f].contiguous(), t0[f].contiguous()))) for f in range(3)]
    start = [r.loss_and_grad(p0, t0, b0, f) for f in range(3)]
    start = [(float(l), _np(torch.cat([g["pose"], g["transl"]]))) for l, g in start]
    trace, lines = [], []
    p, t, losses = r.refine(b0, p0, t0, iters=10, log=lines.append, trace=trace)
    losses = _np(losses)
    assert losses.shape == (3, 2) and np.isfinite(losses).all() and len(lines) == 3
    assert all(torch.equal(a, b) for a, b in zip(keep, (b0, p0, t0))), "refine changed its inputs"
    for f in range(3):
        first = next(e for e in trace if e[0] == f)
        assert float(first[1]) == start[f][0] == losses[f, 0] and np.array_equal(_bits(_np(first[2])), _bits(start[f][1])), "the first closure evaluation"
        assert losses[f, 1] < losses[f, 0], "frame %d: %g -> %g" % (f, losses[f, 0], losses[f, 1])
        alpha1 = _np(r.sil.render(r._posed(b0, p[f].contiguous(), t[f].contiguous())))
        iou0, iou1 = _iou(alpha0[f], target[f]), _iou(alpha1, target[f])
        print("SILREF refine frame %d: loss %.6e -> %.6e (x %.2e), IoU %.4f -> %.4f, %d closure evaluations"
              % (f, losses[f, 0], losses[f, 1], losses[f, 1] / losses[f, 0], iou0, iou1, sum(e[0] == f for e in trace)))
        assert iou1 >= iou0
    # one frame alone: the other rows keep their bits
    p1, t1, l1 = r.refine(b0, p0, t0, iters=2, frames=[1])
    assert torch.equal(p1[0], p0[0]) and torch.equal(p1[2], p0[2]) and torch.equal(t1[0], t0[0]) and torch.equal(t1[2], t0[2])
    assert not torch.equal(p1[1], p0[1]) and torch.isnan(l1[0]).all() and torch.isfinite(l1[1]).all()


# ---- the driver ------------------------------------------------------------------------------------------------------------------------
def _sequence(tmp_path, n=2, H=48, W=48, masks=True):
    """a sequence directory of the driver's own files only: cameras.npz, poses.npz, keypoints.npy, masks/*.png"""
    from PIL import Image
    i = _refine_case()
    root = os.path.join(os.fspath(tmp_path), "seq")
    os.makedirs(os.path.join(root, "masks"))
    fx, fy, cx, cy, _ = i["cam"]
    np.savez(os.path.join(root, "cameras.npz"), intrinsic=np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]), extrinsic=np.eye(4), height=H, width=W)
    d = dict(betas=i["betas"], transl=i["transl"][:n], thetas=i["pose"][:n])
    np.savez(os.path.join(root, "poses.npz"), **d)
    rs = np.random.RandomState(3)
    np.save(os.path.join(root, "keypoints.npy"), np.concatenate([rs.rand(n, 25, 2) * [W, H], np.zeros((n, 25, 1))], -1))
    if masks:
        for f in range(n):
            Image.fromarray(i["masks"][f]).save(os.path.join(root, "masks", "%04d.png" % f))
    return root, d


def test_driver_silhouette_stage_writes_a_pose_file_the_loader_reads(tmp_path):
    from instantavatar_amd.datasets.sequence_dir import load_smpl_param
    from instantavatar_amd.drivers import refine_smpl
    root, d = _sequence(tmp_path)
    out_path = os.path.join(root, "poses_optimized.npz")
    assert refine_smpl.main(["--data", root, "--synthetic-mesh-body", "--steps", "0", "--silhouette", "--silhouette-iters", "2"]) == 0
    out = dict(np.load(out_path))
    assert sorted(out) == sorted(d) and all(out[k].shape == np.asarray(d[k]).shape and np.isfinite(out[k]).all() for k in d)
    assert np.array_equal(out["betas"], d["betas"]) and not np.array_equal(out["thetas"], d["thetas"]) and not np.array_equal(out["transl"], d["transl"])
    p = load_smpl_param(out_path)
    assert p["body_pose"].shape == (2, 69) and p["transl"].shape == (2, 3)
    # without --silhouette the driver is the keypoint stage alone, as before: the arrays of read_inputs -> KeypointRefiner.refine ->
    # write_outputs called directly, bit for bit (the masks are not looked at)
    os.remove(out_path)
    assert refine_smpl.main(["--data", root, "--synthetic-body", "--steps", "3"]) == 0
    plain = dict(np.load(out_path))
    os.remove(out_path)
    from instantavatar_amd import synthetic
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.keypoints import KeypointRefiner
    proj, params, pose, betas, transl, kp = refine_smpl.read_inputs(root, 1.0)
    kr_ = KeypointRefiner(SMPL.from_dict(synthetic.make_body()).to(DEV), proj, kp, threshold=0.2)
    b, p_, t_, _ = kr_.refine(_dev(betas), _dev(pose), _dev(transl), steps=3, lr=1e-3)
    refine_smpl.write_outputs(root, params, _np(b), _np(p_), _np(t_))
    direct = dict(np.load(out_path))
    assert sorted(plain) == sorted(direct) and all(plain[k].dtype == direct[k].dtype and np.array_equal(plain[k], direct[k]) for k in plain)


def test_driver_silhouette_errors_name_their_files(tmp_path):
    from instantavatar_amd.drivers import refine_smpl
    root, _ = _sequence(tmp_path)
    args = ["--data", root, "--steps", "0", "--silhouette", "--silhouette-iters", "1"]
    with pytest.raises(SystemExit, match=r"body.*no faces"):
        refine_smpl.main(args + ["--synthetic-body"])
    os.remove(os.path.join(root, "masks", "0001.png"))
    with pytest.raises(SystemExit, match=r"masks.*1 masks? but 2 rows of poses in .*poses\.npz"):
        refine_smpl.main(args + ["--synthetic-mesh-body"])
    os.remove(os.path.join(root, "masks", "0000.png"))
    os.rmdir(os.path.join(root, "masks"))
    with pytest.raises(SystemExit, match=r"masks: is missing"):
        refine_smpl.main(args + ["--synthetic-mesh-body"])
    assert not os.path.exists(os.path.join(root, "poses_optimized.npz"))
