"""The keypoint-refinement entries, called through the C ABI (`_lib.call`, plain device tensors, the ia_smpl_body struct) on the
seeded cases of tests/keypoint_refs.py and compared per output group with its float64 restatement: ia_kp_loss_fwd / ia_kp_loss_bwd
(csrc/ia_keypoints.hip).  The bound is derived in keypoint_refs.py; tests/test_cpu_keypoint_refs.py shows on the CPU that the
reference is right, that a second fp32 association stays inside the bound and that seven seeded defects do not.  Every output
buffer carries a sentinel row behind its last row and every workspace a sentinel tail: nothing may be written there.  Each
comparison prints "KPREF ..." lines: the worst error / (allow / K) per case -- the figures recorded in keypoint_refs.MEASURED.
Then `KeypointRefiner.refine` against the float64 loop, and the driver on a small sequence directory."""
import functools
import os

import numpy as np
import pytest
import torch

import keypoint_refs as kr
import smpl_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 7.25
WS_TAIL = 64
OUT_ROWS = dict(verts=lambda F, V: (F * V, 3), points=lambda F, V: (F * 35, 3), uv=lambda F, V: (F * 25, 2), loss=lambda F, V: (3,),
                d_betas=lambda F, V: (10,), d_pose=lambda F, V: (F, 72), d_transl=lambda F, V: (F, 3))


def _lib():
    from instantavatar_amd import _lib as L
    return L


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a if k in b)


def _out(shape):
    """an output buffer of shape[0] rows and one more behind them, all holding the sentinel"""
    return torch.full((shape[0] + 1,) + tuple(shape[1:]), SENTINEL, device=DEV)


def _take(t, rows, what):
    a = _np(t)
    assert (a[rows:] == SENTINEL).all(), what + ": written behind its last row"
    return a[:rows]


class _Case:
    """the device copies of one case and its ia_smpl_body"""

    def __init__(self, i, name):
        L = _lib()
        self.name, self.i = name, i
        self.F, self.V = i["pose"].shape[0], i["body"]["v_template"].shape[0]
        self.t = {k: _dev(i["body"][k]) for k in sr.BODY_KEYS}
        self.body = L.SmplBody()
        for k in sr.BODY_KEYS:
            setattr(self.body, k, self.t[k].data_ptr())
        self.body.n_verts = self.V
        self.d = {k: _dev(i[k]) for k in ("betas", "pose", "transl", "proj", "keypoints", "kp_vertex")}
        self.thr = float(i["threshold"])
        self.need = L.call("ia_kp_workspace_bytes", self.F, self.V)
        self.n_frames = self.F

    def workspace(self):
        """NaN bits throughout, WS_TAIL bytes more than required"""
        return torch.full((self.need + WS_TAIL,), 255, dtype=torch.uint8, device=DEV)

    def _outs(self, want):
        return {k: (_out(OUT_ROWS[k](self.F, self.V)) if on else None) for k, on in want.items()}

    def _collect(self, o, ws, what):
        torch.cuda.synchronize()
        assert (_np(ws[-WS_TAIL:]) == 255).all(), what + " wrote behind the workspace"
        return {k: _take(t, OUT_ROWS[k](self.F, self.V)[0], self.name + " " + k) for k, t in o.items() if t is not None}

    def fwd(self, ws, verts=True, points=True, uv=True, loss=True, ws_bytes=None, **over):
        o = self._outs(dict(verts=verts, points=points, uv=uv, loss=loss))
        self.raw = o
        d = dict(self.d, **over)
        _lib().call("ia_kp_loss_fwd", self.body, d["betas"], d["pose"], d["transl"], self.n_frames, d["proj"], d["keypoints"], self.thr, d["kp_vertex"],
                    o["verts"], o["points"], o["uv"], o["loss"], ws, self.need if ws_bytes is None else ws_bytes)
        r = self._collect(o, ws, "forward")
        self.verts_dev = None if o["verts"] is None else o["verts"][:self.F * self.V].contiguous()
        return {k: v.reshape({"verts": (self.F, self.V, 3), "points": (self.F, 35, 3), "uv": (self.F, 25, 2), "loss": (3,)}[k]) for k, v in r.items()}

    def bwd(self, ws, verts, d_betas=True, d_pose=True, d_transl=True, ws_bytes=None, **over):
        o = self._outs(dict(d_betas=d_betas, d_pose=d_pose, d_transl=d_transl))
        self.raw = o
        d = dict(self.d, **over)
        _lib().call("ia_kp_loss_bwd", self.body, d["betas"], d["pose"], d["transl"], self.n_frames, d["proj"], d["keypoints"], self.thr, d["kp_vertex"],
                    verts, o["d_betas"], o["d_pose"], o["d_transl"], ws, self.need if ws_bytes is None else ws_bytes)
        return self._collect(o, ws, "backward")


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(kr.inputs(name), name)


def _check(got, bound, what):
    over, worst = kr.compare(got, bound, what)
    assert not over, (what, "error / allow", over)
    return worst


# ---- forward and backward against the float64 reference ------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_loss_and_gradient_within_the_bound(name):
    """verts, points, uv and the three loss terms within allow; then, from the kernel's own verts, d_pose of every frame and joint,
    d_transl of every frame and d_betas within allow -- on a workspace freshly filled with NaN (nothing survives from the forward)"""
    c = _case(name)
    r = c.fwd(c.workspace())
    _check(kr.fwd_groups(r), kr.fwd_bound(name), "fwd " + name)
    if c.F == 1:
        assert r["loss"][2] == 0 and np.array_equal(_bits(r["loss"][0:1]), _bits(r["loss"][1:2])), "F == 1: the temporal term is absent"
    g = c.bwd(c.workspace(), c.verts_dev)
    _check(kr.bwd_groups(g), kr.bwd_bound(name)[0], "bwd " + name)


def test_two_calls_give_the_same_bits_and_null_outputs_change_nothing():
    """the F = 9 case (three frame tiles, two vertex blocks): a second forward and a second backward repeat the first bit for bit
    (fixed-order sums, no atomics); each optional output left NULL leaves the others bit-equal"""
    c = _case("f9-v257-star")
    first = c.fwd(c.workspace())
    verts = c.verts_dev
    assert _same(first, c.fwd(c.workspace())), "two forward calls differ"
    for null in ("verts", "points", "uv", "loss"):
        r = c.fwd(c.workspace(), **{null: False})
        assert set(r) == set(first) - {null} and _same(r, first), null + " = NULL changes the other outputs"
    bare = c.fwd(c.workspace(), verts=False, points=False, uv=False)
    assert set(bare) == {"loss"} and _same(bare, first)
    g = c.bwd(c.workspace(), verts)
    assert _same(g, c.bwd(c.workspace(), verts)), "two backward calls differ"
    for null in ("d_betas", "d_pose", "d_transl"):
        r = c.bwd(c.workspace(), verts, **{null: False})
        assert set(r) == set(g) - {null} and _same(r, g), null + " = NULL changes the other outputs"


def test_identical_frames_and_an_exact_keypoint_hit_follow_the_zero_convention():
    """frames 0 and 1 identical (every vertex distance of that pair is exactly zero) and one keypoint equal to the kernel's own
    projection bit for bit (its error is exactly zero): all outputs finite, the gradients within the bound of the reference that
    takes both norms' derivatives at zero as zero"""
    i = dict(kr.inputs("f3-v257-smpl"))
    i["pose"], i["transl"], i["keypoints"] = i["pose"].copy(), i["transl"].copy(), i["keypoints"].copy()
    i["pose"][1], i["transl"][1] = i["pose"][0], i["transl"][0]
    c = _Case(i, "zero-convention")
    uv = c.fwd(c.workspace())["uv"]
    hit = (0, 3)
    assert i["keypoints"][hit][2] > i["threshold"]
    i["keypoints"][hit][:2] = uv[hit]
    c = _Case(i, "zero-convention")
    r = c.fwd(c.workspace())
    assert np.array_equal(_bits(r["uv"]), _bits(uv)) and np.array_equal(_bits(r["verts"][0]), _bits(r["verts"][1]))
    g = c.bwd(c.workspace(), c.verts_dev)
    assert all(np.isfinite(v).all() for v in list(r.values()) + list(g.values()))
    _check(kr.fwd_groups(r), kr.fwd_bound_of(kr.args(i)), "fwd zero-convention")
    _check(kr.bwd_groups(g), kr.bwd_bound_of(kr.args(i), hit=(hit,))[0], "bwd zero-convention")


def test_argument_errors_raise_and_write_nothing():
    """n_frames = 0, n_verts = 0, n_frames * n_verts * 3 >= 2^31, a workspace one byte short, a kp_vertex entry of V or of -1
    (found on the device by the first kernel, which writes its flag into the workspace and nothing else), NULL verts for the
    backward: IAError from both entries, no output element written, nothing behind the workspace"""
    L = _lib()
    c = _case("f2-v255-chain")
    ws = c.workspace()
    c.fwd(ws)
    verts = c.verts_dev

    def refused(match, head_untouched=True, **over):
        for call in (lambda **kw: c.fwd(ws, **kw), lambda **kw: c.bwd(ws, verts, **kw)):
            ws.fill_(255)
            with pytest.raises(L.IAError, match=match):
                call(**over)
            torch.cuda.synchronize()
            assert all((_np(t) == SENTINEL).all() for t in c.raw.values() if t is not None), match + ": an output was written"
            w = _np(ws)
            assert (w[256:] == 255).all() and (not head_untouched or (w == 255).all()), match + ": the workspace was written"

    refused("workspace", ws_bytes=c.need - 1)
    c.n_frames = 0
    try:
        refused("n_frames")
    finally:
        c.n_frames = c.F
    for nv, match in ((0, "n_verts"), ((1 << 31) // (3 * c.F) + 1, "31 bits")):
        c.body.n_verts = nv
        try:
            refused(match)
        finally:
            c.body.n_verts = c.V
    for bad in (c.V, -1):
        kv = c.i["kp_vertex"].copy()
        kv[7] = bad
        refused("kp_vertex", head_untouched=False, kp_vertex=_dev(kv))
    ws.fill_(255)
    with pytest.raises(L.IAError, match="verts"):
        c.bwd(ws, None)
    assert L.call("ia_kp_workspace_bytes", 0, 5) == 0 and L.call("ia_kp_workspace_bytes", 5, 0) == 0 and L.call("ia_kp_workspace_bytes", 1 << 20, 1 << 10) == 0
    # and the case still computes what it computed before
    assert _same(c.fwd(c.workspace()), c.fwd(c.workspace()))


# ---- KeypointRefiner -------------------------------------------------------------------------------------------------------------
def _pixel_error(uv, kp, thr):
    e = np.linalg.norm(kp[..., :2].astype(np.float64) - uv.astype(np.float64), axis=-1)
    live = np.zeros(e.shape, bool)
    live[:, kr.SELECT] = True
    live &= kp[..., 2] > thr
    return float(e[live].mean())


def test_refine_reduces_the_keypoint_error_like_the_float64_loop():
    """synthetic.make_body(), 6 frames of procedural_pose_track, keypoints from the true poses, start = true poses + 0.05 rad per joint
    + 2 cm, 200 steps: the last loss is below the first, and the mean keypoint pixel error drops by at least half of what
    keypoint_refs.refine_ref (the same loop in float64 numpy) achieves on the same inputs.
    measured (MI355X): 5.4336 -> 0.0747 px (drop 5.3589); the float64 loop: 5.4336 -> 0.0754 px (drop 5.3582)"""
    from instantavatar_amd import synthetic
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.keypoints import KeypointRefiner, SMPL_KP_VERTEX
    i = kr.synthetic_refine_case(synthetic)
    body = SMPL.from_dict(i["body_dict"]).to(DEV)
    r = KeypointRefiner(body, i["proj"], i["keypoints"], threshold=float(i["threshold"]), kp_vertex=SMPL_KP_VERTEX)
    b0, p0, t0 = (_dev(i[k]) for k in ("betas", "pose", "transl"))
    before = _pixel_error(_np(r.loss(b0, p0, t0)["uv"]), i["keypoints"], i["threshold"])
    lines = []
    b, p, t, losses = r.refine(b0, p0, t0, steps=200, lr=1e-3, log=lines.append)
    after = _pixel_error(_np(r.loss(b, p, t)["uv"]), i["keypoints"], i["threshold"])
    losses = _np(losses)
    ref_before, ref_after, ref_losses = kr.refine_ref_drop(synthetic)
    print("KPREF refine: GPU %.4f -> %.4f px (drop %.4f), loss %.5f -> %.5f; float64 loop %.4f -> %.4f px (drop %.4f), loss %.5f -> %.5f"
          % (before, after, before - after, losses[0, 0], losses[-1, 0], ref_before, ref_after, ref_before - ref_after, ref_losses[0, 0], ref_losses[-1, 0]))
    assert losses.shape == (200, 3) and np.isfinite(losses).all() and len(lines) == 1
    assert losses[-1, 0] < losses[0, 0]
    assert before - after >= 0.5 * (ref_before - ref_after)
    out, g = r.loss_and_grad(b0, p0, t0)
    assert g["pose"].shape == (6, 72) and g["transl"].shape == (6, 3) and g["betas"].shape == (10,) and float(out["loss"]) == float(losses[0, 0])


# ---- the driver --------------------------------------------------------------------------------------------------------------------
def _sequence(tmp_path, layout, n=3):
    import sequence_fixture as sf
    root = os.path.join(os.fspath(tmp_path), "seq")
    sf.write_sequence(root, "custom", n=n)
    os.remove(os.path.join(root, "poses_optimized.npz"))
    rs = np.random.RandomState(3)
    cam = np.load(os.path.join(root, "cameras.npz"))
    pose = rs.randn(n, 72) * 0.2
    pose[:, 0] += np.pi
    d = dict(betas=rs.randn(10) * 0.5, transl=rs.randn(n, 3) * 0.05 + [0.0, 0.1, 3.5])
    if layout == "thetas":
        d["thetas"] = pose
    else:
        d["global_orient"], d["body_pose"] = pose[:, :3], pose[:, 3:]
    np.savez(os.path.join(root, "poses.npz"), **d)
    kp = np.concatenate([rs.rand(n, 25, 2) * [cam["width"], cam["height"]], rs.rand(n, 25, 1)], -1)
    np.save(os.path.join(root, "keypoints.npy"), kp)
    return root, d


@pytest.mark.parametrize("layout", ("thetas", "split"))
def test_driver_writes_a_pose_file_the_loader_reads(tmp_path, layout):
    from instantavatar_amd.datasets import sequence_dir as sd
    from instantavatar_amd.drivers import refine_smpl
    root, d = _sequence(tmp_path, layout)
    assert refine_smpl.main(["--data", root, "--synthetic-body", "--steps", "10"]) == 0
    out = dict(np.load(os.path.join(root, "poses_optimized.npz")))
    assert sorted(out) == sorted(d) and all(out[k].shape == np.asarray(d[k]).shape for k in d)
    assert all(np.isfinite(v).all() for v in out.values())
    moved = "thetas" if layout == "thetas" else "body_pose"
    assert not np.array_equal(out[moved], d[moved]) and not np.array_equal(out["transl"], d["transl"])
    if layout == "split":
        assert (out["body_pose"][:, -12:] == 0).all() and (np.asarray(d["body_pose"])[:, -12:] != 0).any()
    else:
        assert (out["thetas"][:, -12:] != 0).any()
    seq = sd.read_sequence(root, "custom", "train", dict(start=0, end=2))
    assert seq.pose_file == os.path.join(root, "poses_optimized.npz") and seq.smpl_params["body_pose"].shape == (3, 69)


def test_driver_errors_name_their_files(tmp_path):
    from instantavatar_amd.drivers import refine_smpl
    root, _ = _sequence(tmp_path, "thetas")
    kp_path = os.path.join(root, "keypoints.npy")
    kp = np.load(kp_path)
    for write, match in ((lambda: np.save(kp_path, kp[:2]), r"keypoints\.npy: 2 rows of keypoints but 3 rows of poses in .*poses\.npz"),
                         (lambda: np.save(kp_path, kp[:, :18]), r"keypoints\.npy: keypoints are \[F,25,3\].*\(3, 18, 3\)"),
                         (lambda: os.remove(kp_path), r"keypoints\.npy: is missing")):
        write()
        with pytest.raises(SystemExit, match=match):
            refine_smpl.main(["--data", root, "--synthetic-body", "--steps", "1"])
        assert not os.path.exists(os.path.join(root, "poses_optimized.npz"))
