"""The float64 references of tests/smpl_refs.py are right, and the bound built on them can fail: the forward against the
reference's own lbs.py (tests/golden/lbs_golden.npz), the hand-derived backward against central differences of the forward,
seven seeded defects each far outside the bound, a second fp32 association inside it.  No GPU, no product import."""
import os

import numpy as np
import pytest

import smpl_refs as sr

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_LBS = [n for n, c in sr.LBS_CASES.items() if c[0] < 1000]


def _golden_body(g):
    Jr = g["J_regressor"].astype(np.float64)
    return dict(v_template=g["v_template"], shapedirs=g["shapedirs"], posedirs=g["posedirs"], lbs_weights=g["lbs_weights"],
                J0=Jr @ g["v_template"].astype(np.float64), JS=np.einsum("jv,vcl->jcl", Jr, g["shapedirs"].astype(np.float64)),
                parents=g["parents"])


def test_forward_refs_match_the_reference_lbs_golden():
    """lbs_fwd_ref in float64 on the body and the four (betas, pose, transl) cases of lbs_golden.npz -- the reference's lbs.py
    executed in fp32 -- within the tolerances test_smpl_forward_on_device_matches_reference_lbs_golden uses for that file: A,
    the posed vertices, the posed joints and T to 2e-5, the shape and pose offsets to 1e-6; w2s = inv(A_0); and tfs_fwd_ref
    against inv(A_0) . A . tfs_inv_t built from the golden A in float64 (5e-5, as that test, times the row-sum norm of B)."""
    g = np.load(os.path.join(HERE, "golden", "lbs_golden.npz"))
    body = _golden_body(g)
    assert np.array_equal(g["parents"], sr.SMPL_PARENTS)
    pose_t = sr.template_pose()
    po_t = sr.pose_offsets_f32(body, pose_t)
    B = sr.random_affine(np.random.default_rng(5), sr.N_J)
    for i in range(int(g["n_cases"])):
        betas, pose, transl = g["betas%d" % i][0], g["pose%d" % i][0], g["transl%d" % i][0]
        r = sr.lbs_fwd_ref(body, betas, pose, transl, pose_t, po_t)
        for key, ref, tol in (("A", "A", 2e-5), ("x_world", "verts", 2e-5), ("joints_posed", "joints", 2e-5), ("T", "T", 2e-5),
                              ("so", "shape_offsets", 1e-6), ("po", "pose_offsets", 1e-6), ("R", "rot", 2e-6)):
            got = r["rod"]["R"] if key == "R" else r[key]
            err = np.abs(got - g["%s%d" % (ref, i)].reshape(got.shape)).max()
            assert err < tol, (i, key, err)
        A_ref = g["A%d" % i][0].astype(np.float64)
        assert np.abs(r["w2s"] - np.linalg.inv(r["A"][0])).max() < 1e-12
        assert np.abs(r["w2s"] - np.linalg.inv(A_ref[0])).max() < 2e-5
        # T_inv as smpl_deformer.py:66-75 spells it, from this forward's own pieces, with the library inverse
        Minv = np.linalg.inv(r["T"]) @ r["S"]
        Minv[:, :3, 3] += po_t - r["po"]
        assert np.abs(r["T_inv"] - r["Tt"] @ Minv).max() < 1e-10 * np.abs(r["T_inv"]).max()      # (dense golden weights: T is badly conditioned)
        assert np.abs(r["verts"] - (r["x_world"] @ r["w2s"][:3, :3].T + r["w2s"][:3, 3])).max() < 1e-12
        joints = body["J0"] + body["JS"] @ betas.astype(np.float64)
        t = sr.tfs_fwd_ref(joints, g["parents"], pose, transl, B)
        want = np.linalg.inv(A_ref[0])[None] @ A_ref @ B.astype(np.float64)
        assert np.abs(t["tfs"] - want).max() < 5e-5 * np.abs(B).sum(-1).max(), i
        assert np.abs(t["A"] - A_ref).max() < 2e-5 and np.abs(t["w2s"] - np.linalg.inv(A_ref[0])).max() < 2e-5


FD_H = 1e-6
FD_TOL = 5e-8       # 3 x the largest measured (1.6e-8): the forward goes through tensordot / @, whose summation order is the library's
FD_NOISE = 1e-9     # x sum |d . out|: the rounding of L itself, a few 2^-53 sum |terms|, divided by 2 h


def _fd(f, x, h=FD_H):
    x = np.asarray(x, np.float64)
    out = np.zeros_like(x)
    for k in range(x.size):
        e = np.zeros_like(x)
        e[k] = h
        out[k] = (f(x + e) - f(x - e)) / (2 * h)
    return out


def _rel(fd, g):
    return float(np.abs(fd - g).max() / max(np.abs(g).max(), np.abs(fd).max(), 1e-300))


@pytest.mark.parametrize("name", SMALL_LBS)
def test_lbs_backward_ref_equals_central_differences(name):
    """lbs_bwd_ref against central differences (h = 1e-6, float64) of L = sum d_T_inv . T_inv + sum d_w2s . w2s over rows 0..2,
    for all 72 pose entries, the 10 betas and the 3 translations (a NULL transl is differentiated at 0), on every small case:
    the zero-joint poses and the chain and star tables are among them.  Measured: |fd - g| is 2e-11 .. 1.6e-8 of the largest
    entry of a vector that carries signal (d_pose <= 5e-10) and 1e-17 .. 1.4e-10 of sum |d . out| everywhere -- the cancelling d_transl and the
    d_betas of pose == pose_t (|g| 4e-3 under a functional of 16) included, where only the rounding of L itself, a few 2^-53
    sum |terms| divided by 2 h, is left.  Asserted: |fd - g| < 5e-8 max |g| + 1e-9 sum |d . out|."""
    i = sr.lbs_inputs(name)
    D = sr._upstream(i["d_T_inv"], np.float64)
    Dw = None if i["d_w2s"] is None else sr._upstream(i["d_w2s"], np.float64)
    tr0 = np.zeros(3) if i["transl"] is None else i["transl"]

    def L(betas, pose, transl):
        r = sr.lbs_fwd_ref(i["body"], betas, pose, transl, i["pose_t"], i["po_t"])
        return (D * r["T_inv"]).sum() + (0.0 if Dw is None else (Dw * r["w2s"]).sum())

    g = sr.lbs_bwd_ref(*sr.lbs_args(i, True))
    r0 = sr.lbs_fwd_ref(*sr.lbs_args(i))
    Labs = np.abs(D * r0["T_inv"]).sum() + (0.0 if Dw is None else np.abs(Dw * r0["w2s"]).sum())
    fd = dict(d_pose=_fd(lambda x: L(i["betas"], x, tr0), i["pose"]),
              d_betas=_fd(lambda x: L(x, i["pose"], tr0), i["betas"]),
              d_transl=_fd(lambda x: L(i["betas"], i["pose"], x), tr0))
    for k in ("d_pose", "d_betas", "d_transl"):
        err, big = float(np.abs(fd[k] - g[k]).max()), float(np.abs(g[k]).max())
        print("FD %-18s %-8s |g| %.3e  err %.2e  err/|g| %.2e  err/Labs %.2e" % (name, k, big, err, err / max(big, 1e-300), err / Labs))
        assert err < FD_TOL * big + FD_NOISE * Labs, (name, k, err, big, Labs)


@pytest.mark.parametrize("name", sorted(sr.TFS_CASES))
def test_tfs_backward_ref_equals_central_differences(name):
    """tfs_bwd_ref against central differences (h = 1e-6) of L = sum d_tfs . tfs (rows 0..2), 72 pose entries and 3 translations;
    same agreement as the LBS test (measured <= 6e-10 of the largest entry, asserted 5e-8); d_transl is zero up to the rounding of the difference"""
    i = sr.tfs_inputs(name)
    D = sr._upstream(i["d_tfs"], np.float64)
    tr0 = np.zeros(3) if i["transl"] is None else i["transl"]
    L = lambda pose, transl: (D * sr.tfs_fwd_ref(i["joints_rest"], i["parents"], pose, transl, i["tfs_inv_t"])["tfs"]).sum()
    g = sr.tfs_bwd_ref(*sr.tfs_args(i, True))
    fd = _fd(lambda x: L(x, tr0), i["pose"])
    r = _rel(fd, g["d_pose"])
    print("FD tfs %-14s d_pose |g| %.3e  rel %.2e" % (name, np.abs(g["d_pose"]).max(), r))
    assert r < FD_TOL, (name, r)
    fdt = _fd(lambda x: L(i["pose"], x), tr0)
    assert np.abs(fdt).max() < 1e-8 * g["m_d_transl"].max() and np.abs(g["d_transl"]).max() <= 1e-9 * g["m_d_transl"].max()


def test_cancelling_translation_gradients_are_zero_in_float64():
    """d_transl of ia_smpl_tfs_bwd, and of ia_smpl_lbs_bwd without d_w2s, is analytically zero: the float64 reference gives
    |d_transl| <= 1e-9 M on every such case (so u . M alone is the bound there), and with d_w2s it is signal"""
    n = 0
    for name in sr.LBS_CASES:
        bound, R = sr.lbs_bwd_bound(name)
        M = R["m_d_transl"].max()
        if sr.lbs_inputs(name)["d_w2s"] is None:
            n += 1
            assert np.abs(R["d_transl"]).max() <= 1e-9 * M, (name, np.abs(R["d_transl"]).max(), M)
            assert bound["d_transl"][1] == sr.K_BOUND * sr.U * M
        else:
            assert np.abs(R["d_transl"]).max() > 1e-5 * M, name
    assert n >= 3
    for name in sr.TFS_CASES:
        bound, R = sr.tfs_bwd_bound(name)
        assert np.abs(R["d_transl"]).max() <= 1e-9 * R["m_d_transl"].max(), name
        assert bound["d_transl"][1] == sr.K_BOUND * sr.U * R["m_d_transl"].max()


def test_case_lists_cover_what_they_must():
    c = list(sr.LBS_CASES.values())
    assert {x[0] for x in c} == {1, 255, 257, 6890} and sum(x[0] == 6890 for x in c) <= 2
    assert {x[1] for x in c} == {"smpl", "chain", "star"}
    assert {x[2] for x in c} == {"random", "zero", "mixed", "extreme", "same", "bigroot"}
    assert {x[3] for x in c} == {True, False} and {x[4] for x in c} == {None, "small", "large"}
    assert {x[5] for x in c} == {"dense", "onehot", "last"} and {x[6] for x in c} == {True, False}
    assert (sr.parents_table("chain")[1:] == np.arange(23)).all() and (sr.parents_table("star")[1:] == 0).all()
    p = sr.make_pose("extreme", 3).reshape(24, 3)
    assert abs(np.linalg.norm(p[5]) - (np.pi - 1e-3)) < 1e-6 and abs(np.linalg.norm(p[16]) - 4.0) < 1e-6
    assert (sr.make_pose("mixed").reshape(24, 3)[list(sr.ZERO_JOINTS)] == 0).all() and (sr.make_pose("zero") == 0).all()
    i = sr.lbs_inputs("chain-same-257")
    assert np.array_equal(i["pose"], i["pose_t"]) and np.abs(i["pose"]).max() > 0.1
    i = sr.lbs_inputs("smpl-bigroot-6890")
    assert np.linalg.norm(i["transl"]) > 3 and abs(np.linalg.norm(i["pose"][:3]) - 2.5) < 1e-6 and np.abs(i["betas"]).max() > 1
    i = sr.lbs_inputs("star-hand-257")
    assert i["body"]["lbs_weights"][sr.HOT_VERTEX, sr.HAND] == 1.0 and np.abs(i["d_T_inv"][sr.HOT_VERTEX, :3]).min() > 0
    assert (np.delete(i["d_T_inv"], sr.HOT_VERTEX, 0)[:, :3] == 0).all() and (i["d_T_inv"][:, 3] == sr.ROW3_FILL).all()
    i = sr.lbs_inputs("smpl-extreme-255")
    assert (i["d_T_inv"][:-1, :3] == 0).all() and np.abs(i["d_T_inv"][-1, :3]).min() > 0
    b = sr.lbs_inputs("smpl-mixed-6890")["body"]
    assert set(np.unique((b["lbs_weights"] > 0).sum(1))) == {1, 2, 3, 4}
    assert 0.01 < b["shapedirs"].std() < 0.03 and 0.005 < b["posedirs"].std() < 0.015 and (np.abs(b["JS"]) > 0).all()
    d = np.abs(sr.lbs_inputs("smpl-random-257")["d_T_inv"][:, :3])
    assert d.max() / np.median(d) > 64 and (sr.lbs_inputs("smpl-random-257")["d_T_inv"][:, :3] < 0).any()


# ---- the bound can fail --------------------------------------------------------------------------------------------------
def _edit(name, fn, index=None):
    def tap(n, x, idx):
        return fn(x) if n == name and (index is None or idx == index) else x
    return tap


def _zero_col3(x):
    x = x.copy()
    x[:, 3] = 0
    return x


def _zero_last(x):
    x = x.copy()
    x[-1] = 0
    return x


#: defect: (tap, the case that must see it, the groups it must show in)
DEFECTS = {
    "pose-feature share of dR dropped":        (_edit("dpf", np.zeros_like), "smpl-random-257", ["d_pose[%02d]" % j for j in (4, 12, 23)]),
    "d_w2s path dropped":                      (_edit("dS_w2s", np.zeros_like), "smpl-random-257", ["d_pose[00]", "d_transl"]),
    "dg[p] += dg[i] skipped for joint 9":      (_edit("dG_to_parent", _zero_col3, 9), "smpl-random-257", ["d_pose[03]", "d_pose[00]"]),
    "-RG^T dA.t term of dJ dropped":           (_edit("dJ_from_A", np.zeros_like), "smpl-random-257", ["d_betas"]),
    "last vertex left out of the d_A sum":     (_edit("dT", _zero_last), "smpl-extreme-255", ["d_pose[00]"]),
    "+1e-8 in dir's numerator too, as float64": (_edit("dir_numerator", lambda th: th + 1e-8), "chain-zero-255", ["d_pose[01]", "d_pose[23]"]),
    "hand gradient scaled by 1.001":           (None, "star-hand-257", ["d_pose[%02d]" % sr.HAND]),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defects_exceed_the_bound_fifty_times(defect):
    """one edit to an intermediate (or, for the scaled hand, to the result) of the float64 backward: on the named case every
    named group is at least 50 allowances away from the reference -- the condition under which a kernel that passes the GPU
    test cannot carry that defect"""
    tap, name, groups = DEFECTS[defect]
    bound, _ = sr.lbs_bwd_bound(name)
    bad = sr.lbs_bwd_ref(*sr.lbs_args(sr.lbs_inputs(name), True), tap=tap)
    if tap is None:
        bad["d_pose"] = bad["d_pose"].copy()
        bad["d_pose"][3 * sr.HAND:3 * sr.HAND + 3] *= 1.001
    got = sr.bwd_groups(bad)
    for k in groups:
        ref, allow, _, _ = bound[k]
        f = np.abs(got[k] - ref).max() / allow
        print("DEFECT %-42s %-18s %-11s error / allow %.1f" % (defect, name, k, f))
        assert f >= 50, (defect, name, k, f)


@pytest.mark.parametrize("name", [n for n, c in sr.LBS_CASES.items() if c[0] == 6890])
def test_defects_of_one_part_in_a_thousand_are_visible_at_the_product_size(name):
    """at V = 6 890, with dense upstream gradients: d_pose of a hand, of joint 5 (a hip-chain joint with children) and d_betas,
    each scaled by 1.001 -- the size of "a missing term of 1e-3 of the total" -- are at least 50 allowances away.  (Not so
    the root's d_pose: the vertex path cancels there -- the root rotation drops out of T^-1 . s2w -- and its allowance
    is that of the cancelling terms, 3e-3 of what d_w2s leaves.)"""
    bound, R = sr.lbs_bwd_bound(name)
    for k in ("d_pose[%02d]" % sr.HAND, "d_pose[05]", "d_betas"):
        ref, allow, _, _ = bound[k]
        f = np.abs(ref * 1.001 - ref).max() / allow
        print("DEFECT x 1.001  %-18s %-11s error / allow %.1f" % (name, k, f))
        assert f >= 50, (name, k, f)


@pytest.mark.parametrize("name", sorted(sr.LBS_CASES))
def test_second_fp32_association_stays_inside_the_lbs_bound(name):
    """fp32 again with the vertex sums taken in reversed order and every chain product associated from the leaf up: an equally
    valid evaluation, so it must stay within allow, forward and backward, on every case"""
    i = sr.lbs_inputs(name)
    f = sr.fwd_groups(sr.lbs_fwd_ref(*sr.lbs_args(i), dtype=np.float32, assoc="leaf"), "lbs")
    over, _ = sr.compare(f, sr.lbs_fwd_bound(name), "fp32-alt fwd " + name)
    assert not over, over
    b = sr.bwd_groups(sr.lbs_bwd_ref(*sr.lbs_args(i, True), dtype=np.float32, assoc="leaf", reverse=True))
    over, _ = sr.compare(b, sr.lbs_bwd_bound(name)[0], "fp32-alt bwd " + name)
    assert not over, over


@pytest.mark.parametrize("name", sorted(sr.TFS_CASES))
def test_second_fp32_association_stays_inside_the_tfs_bound(name):
    i = sr.tfs_inputs(name)
    f = sr.fwd_groups(sr.tfs_fwd_ref(*sr.tfs_args(i), dtype=np.float32, assoc="leaf"), "tfs")
    over, _ = sr.compare(f, sr.tfs_fwd_bound(name), "fp32-alt fwd " + name)
    assert not over, over
    b = sr.bwd_groups(sr.tfs_bwd_ref(*sr.tfs_args(i, True), dtype=np.float32, assoc="leaf"))
    over, _ = sr.compare(b, sr.tfs_bwd_bound(name)[0], "fp32-alt bwd " + name)
    assert not over, over
