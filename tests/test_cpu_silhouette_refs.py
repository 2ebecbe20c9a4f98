"""tests/silhouette_refs.py validated without a GPU: its gradients against central differences of its own loss; a float32 evaluation in
a second association inside the bound; eight seeded defects outside it; the allowance cap on every case; and the registration of the
new header, source and synthetic mesh body."""
import functools
import os

import numpy as np
import pytest

import silhouette_refs as sf

RENDER_CASES = [n for n in sorted(sf.CASES)]


@functools.lru_cache(maxsize=None)
def _chain(name, dtype=np.float64, second=False, defect=None):
    """projection -> render -> render backward -> projection backward of one case, each stage on the fp32 rounding of the stage before
    it (what the kernels are handed); with the float64 bounds"""
    i = sf.inputs(name)
    pr = sf.project_ref(i["verts"], i["w2c"], i["cam"], dtype)
    screen, inv_z = sf.project_ref(i["verts"], i["w2c"], i["cam"])["screen"].astype(np.float32), sf.project_ref(i["verts"], i["w2c"], i["cam"])["inv_z"].astype(np.float32)
    R = sf.render_ref(screen, inv_z, i["faces"], i["H"], i["W"], i["sigma"], i["blur"], i["mask"], dtype, second, defect)
    R64 = sf.render_ref(screen, inv_z, i["faces"], i["H"], i["W"], i["sigma"], i["blur"], i["mask"])
    alpha, d_alpha = R64["alpha"].astype(np.float32), R64["d_alpha"].astype(np.float32)
    B = sf.render_bwd_ref(R, alpha, d_alpha, second, defect, with_bound=dtype is np.float64 and defect is None)
    d_screen = sf.render_bwd_ref(R64, alpha, d_alpha, with_bound=False)["d_screen"].astype(np.float32)
    pb = sf.project_bwd_ref(i["verts"], i["w2c"], i["cam"], d_screen, dtype)
    return dict(i=i, pr=pr, R=R, B=B, pb=pb, screen=screen, inv_z=inv_z, alpha=alpha, d_alpha=d_alpha, d_screen=d_screen)


@functools.lru_cache(maxsize=None)
def _bounds(name):
    c = _chain(name)
    fb, share = sf.fwd_bound(c["R"])
    pr, pb = c["pr"], c["pb"]
    K, U = sf.K_BOUND, sf.U
    proj = {"screen": (pr["screen"], K * U * pr["m_screen"], U * pr["m_screen"], 0 * pr["m_screen"]),
            "inv_z": (pr["inv_z"], K * U * pr["m_inv_z"], U * pr["m_inv_z"], 0 * pr["m_inv_z"])}
    projb = {"d_verts": (pb["d_verts"], K * U * pb["m_d_verts"], U * pb["m_d_verts"], 0 * pb["m_d_verts"])}
    return dict(proj=proj, fwd=fb, bwd=c["B"]["bound"], projb=projb, share=share)


def _loss_of_screen(i, screen):
    R = sf.render_ref(screen.astype(np.float32), np.ones(len(screen), np.float32), i["faces"], i["H"], i["W"], i["sigma"], i["blur"], i["mask"])
    return R["loss"]


def test_gradient_equals_central_differences():
    """d L / d screen of the full chain render -> loss, in float64 on the 40 x 48 case: central differences with h = 2^-10 px (screen
    coordinates are fp32 inputs: a power of two keeps x +- h exact), on 12 seeded coordinates of vertices that carry gradient, to
    1e-5 of the largest gradient entry (truncation ~ h^2 L''' and the cut's jump, which a pair crossing blur_radius adds at p_f ~ 1e-4)"""
    c = _chain("tubes-40x48")
    i, R = c["i"], c["R"]
    # the gradient of the reference's OWN loss: its own alpha and d_alpha, unrounded
    ds = _float64_grad(R)
    rng = np.random.default_rng(11)
    live = np.argwhere(np.abs(ds) > 1e-3 * np.abs(ds).max())
    h = 2.0 ** -10
    worst = 0.0
    for v, a in live[rng.permutation(len(live))[:12]]:
        hi, lo = c["screen"].astype(np.float64).copy(), c["screen"].astype(np.float64).copy()
        hi[v, a] += h
        lo[v, a] -= h
        assert np.float32(hi[v, a]) == hi[v, a] and np.float32(lo[v, a]) == lo[v, a]
        fd = (_loss_of_screen(i, hi) - _loss_of_screen(i, lo)) / (2 * h)
        worst = max(worst, abs(fd - ds[v, a]))
    print("central differences: worst %.3e of %.3e" % (worst, np.abs(ds).max()))
    assert worst <= 1e-5 * np.abs(ds).max()


def _float64_grad(R):
    """render_bwd_ref wants fp32 alpha / d_alpha; here the float64 arrays go in unrounded"""
    al, da = R["alpha"], R["d_alpha"]
    pm = sf._pair_mags(R)
    c = R["scale"] / R["sigma"]
    gd = np.where(R["contrib"], (da * (1 - al))[:, None] * R["pf"] * np.where(R["pos"], c, -c), 0)
    ds = np.zeros((R["nv"], 2))
    idx = R["faces"][R["keep"]]
    for corner in range(3):
        s = np.where(R["kwin"] == corner, -2 * (1 - pm["tw"]) * gd, 0) + np.where((R["kwin"] + 1) % 3 == corner, -2 * pm["tw"] * gd, 0)
        np.add.at(ds, idx[:, corner], (s[..., None] * pm["qw"]).sum(0))
    return ds


def test_projection_gradient_equals_central_differences():
    i = sf.inputs("tubes-40x48")
    g = np.random.default_rng(3)
    d_screen = g.standard_normal((len(i["verts"]), 2)).astype(np.float32)
    pb = sf.project_bwd_ref(i["verts"], i["w2c"], i["cam"], d_screen)
    h = 1e-6
    f = lambda X: (sf.project_ref(X, i["w2c"], i["cam"])["screen"] * d_screen).sum()
    for v, a in ((0, 0), (7, 1), (40, 2), (99, 0)):
        hi, lo = i["verts"].astype(np.float64).copy(), i["verts"].astype(np.float64).copy()
        hi[v, a] += h
        lo[v, a] -= h
        fd = (f(hi) - f(lo)) / (2 * h)
        assert abs(fd - pb["d_verts"][v, a]) <= 1e-6 * np.abs(pb["d_verts"]).max()


def test_body_adjoint_equals_central_differences():
    """<d_verts, verts(pose, transl, betas)> differentiated by central differences equals body_bwd_ref"""
    import keypoint_refs as kr
    i = kr.inputs("f3-v257-smpl")
    g = np.random.default_rng(4)
    dv = g.standard_normal((3, 257, 3)).astype(np.float32)
    r = sf.body_bwd_ref(i["body"], i["betas"], i["pose"], i["transl"], dv)
    f = lambda b, p, t: (sf.body_bwd_ref(i["body"], b, p, t, dv)["verts"] * dv).sum()
    p0 = [np.asarray(i[k], np.float64) for k in ("betas", "pose", "transl")]
    h = 1e-6
    for t, grad in enumerate((r["d_betas"], r["d_pose"], r["d_transl"])):
        for idx in list(np.ndindex(p0[t].shape))[::7]:
            hi, lo = [x.copy() for x in p0], [x.copy() for x in p0]
            hi[t][idx] += h
            lo[t][idx] -= h
            fd = (f(*hi) - f(*lo)) / (2 * h)
            assert abs(fd - grad[idx]) <= 1e-6 * np.abs(grad).max(), (t, idx)


@pytest.mark.parametrize("name", RENDER_CASES)
def test_float32_in_a_second_association_stays_inside_the_bound(name):
    c, b = _chain(name, np.float32, True), _bounds(name)
    for what, got, bound in (("proj", c["pr"], b["proj"]), ("fwd", c["R"], b["fwd"]),
                             ("bwd", c["B"], b["bwd"]), ("projb", c["pb"], b["projb"])):
        got = dict(got, loss=np.array([got["loss"]])) if "loss" in got else got
        over, worst = sf.check(got, bound, "f32 second %s %s" % (what, name))
        assert not over, (what, over)


@pytest.mark.parametrize("defect", sorted(sf.DEFECTS))
def test_seeded_defect_falls_outside_the_bound(defect):
    name = sf.DEFECT_CASE
    c, b = _chain(name, np.float64, False, defect), _bounds(name)
    R = dict(c["R"], loss=np.array([c["R"]["loss"]]))
    over_f, _ = sf.check(R, b["fwd"], "fwd " + defect)
    over_b, _ = sf.check(c["B"], b["bwd"], "bwd " + defect)
    assert (over_f if sf.DEFECTS[defect] == "fwd" else over_b), defect + " is not seen"


@pytest.mark.parametrize("name", RENDER_CASES)
def test_the_allowance_cap_holds(name):
    share = _bounds(name)["share"]
    print("SILREF allowance share %-20s %.4f" % (name, share))
    assert share <= sf.ALLOW_CAP
    assert name not in sf.ALLOW_SHARE or abs(sf.ALLOW_SHARE[name] - share) < 1e-4, "ALLOW_SHARE is out of date"


def test_edge_cases_skip_what_the_definition_skips():
    c = _chain("edge-cases")
    i, R = c["i"], c["R"]
    assert (~c["pr"]["valid"]).sum() == 5 and (c["screen"][~c["pr"]["valid"]] == 0).all() and (c["inv_z"][~c["pr"]["valid"]] == 0).all()
    skipped = set(range(len(i["faces"]))) - set(R["keep"].tolist())
    assert {10, 30, 31} <= skipped and len(skipped) > 3
    assert (c["pb"]["d_verts"][~c["pr"]["valid"]] == 0).all()
    e = _chain("no-faces")
    assert (e["R"]["alpha"] == 0).all() and (e["B"]["d_screen"] == 0).all()
    t = _chain("one-triangle")
    assert (t["R"]["alpha"] == 1).all()


def test_the_new_entries_are_declared_and_registered():
    from instantavatar_amd import _lib, build
    assert sorted(_lib.declarations("silhouette")) == ["ia_sil_body_bwd", "ia_sil_body_workspace_bytes", "ia_sil_project_bwd", "ia_sil_project_fwd",
                                                       "ia_sil_render_bwd", "ia_sil_render_fwd", "ia_sil_workspace_bytes"]
    # (disjoint from every other header's names: tests/test_cpu_abi_headers.py)
    assert os.path.normpath(_lib.header_path("silhouette")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_silhouette.hip" in build.SOURCES


def test_make_mesh_body_faces_index_its_vertices():
    from instantavatar_amd import synthetic
    plain = synthetic.make_body()
    for sides, rings in ((3, 2), (8, 5)):
        b = synthetic.make_mesh_body(sides=sides, rings=rings)
        assert set(b) == set(plain) | {"f"}
        V = b["v_template"].shape[0]
        assert V == 28 * (sides * rings + 2) and b["f"].shape == (28 * 2 * sides * rings, 3) and b["f"].dtype == np.int32
        assert b["f"].min() == 0 and b["f"].max() == V - 1 and len(np.unique(b["f"])) == V
        assert b["lbs_weights"].shape == (V, 24) and np.allclose(b["lbs_weights"].sum(1), 1) and ((b["lbs_weights"] > 0).sum(1) <= 4).all()
        assert np.abs(b["J_regressor"] @ b["v_template"] - b["joints_template"]).max() < 1e-6
        t = b["v_template"][b["f"]].astype(np.float64)
        assert (np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1) > 0).all()
        vol = np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).reshape(28, -1).sum(1)
        assert (vol > 0).all(), "a tube is wound inwards"
    with pytest.raises(ValueError):
        synthetic.make_mesh_body(sides=2)


def test_vertex_faces_lists_every_corner_once():
    i = sf.inputs("edge-cases")
    nv = len(i["verts"])
    start, corner = sf.vertex_faces(i["faces"], nv)
    f = i["faces"].reshape(-1)
    assert start[0] == 0 and start[-1] == len(corner) and (np.diff(start) >= 0).all()
    for v in (0, 5, nv - 1):
        assert sorted(corner[start[v]:start[v + 1]]) == [c for c in np.nonzero(f == v)[0] if c // 3 not in (30, 31)]
