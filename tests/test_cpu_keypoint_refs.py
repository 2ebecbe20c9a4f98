"""tests/keypoint_refs.py validated without a GPU: its gradient against central differences and against autograd through a float64
torch restatement built from the SMPL.forward-style ops of deformers/smplx.py; a float32 evaluation in a second association inside
the bound; seven seeded defects outside it; the float64 refinement loop reduces the keypoint error of the case that
tests/test_gpu_keypoints.py refines on the GPU."""
import functools
import os

import numpy as np
import pytest
import torch

import keypoint_refs as kr

SMALL = "f3-v257-smpl"


@functools.lru_cache(maxsize=None)
def _small():
    return kr.args(kr.inputs(SMALL)), kr.kp_bwd_ref(*kr.args(kr.inputs(SMALL)))


def test_gradient_equals_central_differences():
    """every entry of d_betas, d_transl and of d_pose of frame 1, and a seeded third of the other frames' d_pose: central differences
    in float64 with h = 1e-6, to 1e-6 of the tensor's largest gradient entry (truncation ~h^2, rounding ~1e-16 L / h = 1e-9)"""
    a, g = _small()
    p0 = [np.asarray(x, np.float64) for x in a[1:4]]
    grads = [g["d_betas"], g["d_pose"], g["d_transl"]]
    rng = np.random.default_rng(5)
    h = 1e-6
    for t in range(3):
        idx = list(np.ndindex(p0[t].shape))
        if t == 1:
            idx = [i for i in idx if i[0] == 1 or rng.random() < 1 / 3]
        worst = 0.0
        for i in idx:
            lo, hi = [x.copy() for x in p0], [x.copy() for x in p0]
            hi[t][i] += h
            lo[t][i] -= h
            fd = (kr.kp_fwd_ref(a[0], *hi, *a[4:])["loss"][0] - kr.kp_fwd_ref(a[0], *lo, *a[4:])["loss"][0]) / (2 * h)
            worst = max(worst, abs(fd - grads[t][i]))
        scale = np.abs(grads[t]).max()
        print("central differences, tensor %d: worst %.3e of %.3e" % (t, worst, scale))
        assert worst <= 1e-6 * scale


def _torch_loss(body, betas, pose, transl, proj, kp, thr, kpv):
    """SMPL.forward (body_models.py:289-372 + lbs.py:152-250) and refine-smpl.py:187-208 in torch ops, float64"""
    from instantavatar_amd.deformers.smplx import batch_rodrigues, batch_rigid_transform
    t = lambda k: torch.as_tensor(np.asarray(body[k], np.float64))
    F = pose.shape[0]
    parents = torch.as_tensor(np.asarray(body["parents"], np.int64))
    v_shaped = t("v_template") + torch.einsum("l,mkl->mk", betas, t("shapedirs"))
    J = t("J0") + torch.einsum("jkl,l->jk", t("JS"), betas)
    rot = batch_rodrigues(pose.reshape(-1, 3)).view(F, 24, 3, 3)
    Jt, A = batch_rigid_transform(rot, J[None].expand(F, -1, -1), parents)
    pf = (rot[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(F, 207)
    v_posed = v_shaped[None] + torch.matmul(pf, t("posedirs")).view(F, -1, 3)
    T = torch.matmul(t("lbs_weights")[None].expand(F, -1, -1), A.view(F, 24, 16)).view(F, -1, 4, 4)
    verts = torch.matmul(T[..., :3, :3], v_posed[..., None])[..., 0] + T[..., :3, 3] + transl[:, None]
    joints = torch.cat([Jt + transl[:, None], verts[:, torch.as_tensor(np.asarray(kpv, np.int64))]], 1)
    pts = joints[:, torch.as_tensor(kr.BODY25_TO_POINT)]
    P = torch.as_tensor(np.asarray(proj, np.float64))
    q = torch.einsum("ij,mnj->mni", P[:3, :3], pts) + P[:3, 3]
    uv = q[..., :2] / q[..., 2:3]
    kp = torch.as_tensor(np.asarray(kp, np.float64))
    err = (kp[..., :2] - uv).square().sum(-1).sqrt() * (kp[..., 2] > float(np.float32(thr))).double()
    l_kp = err[:, torch.as_tensor(kr.SELECT)].mean()
    l_t = (verts[1:] - verts[:-1]).square().sum(-1).sqrt().mean()
    return l_kp + l_t, l_kp, l_t, verts, joints, uv


def test_reference_equals_the_torch_restatement_and_its_autograd():
    a, g = _small()
    leaves = [torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in a[1:4]]
    L, l_kp, l_t, verts, joints, uv = _torch_loss(a[0], *leaves, *a[4:])
    L.backward()
    f = g["fwd"]
    for name, ours, theirs in (("loss", f["loss"], np.array([L.item(), l_kp.item(), l_t.item()])), ("verts", f["verts"], verts.detach().numpy()),
                               ("points", f["points"], joints.detach().numpy()), ("uv", f["uv"], uv.detach().numpy()),
                               ("d_betas", g["d_betas"], leaves[0].grad.numpy()), ("d_pose", g["d_pose"], leaves[1].grad.numpy()),
                               ("d_transl", g["d_transl"], leaves[2].grad.numpy())):
        err, scale = np.abs(ours - theirs).max(), np.abs(theirs).max()
        print("torch restatement %-8s err %.3e of %.3e" % (name, err, scale))
        assert err <= 1e-10 * scale, name


def test_single_frame_has_no_temporal_term():
    r = kr.kp_bwd_ref(*kr.args(kr.inputs("f1-v257-smpl")))
    assert r["loss"][2] == 0 and r["loss"][0] == r["loss"][1] and np.isfinite(r["d_pose"]).all()


@pytest.mark.parametrize("name", sorted(kr.CASES))
def test_float32_in_a_second_association_stays_inside_the_bound(name):
    """chain products from the leaf up, every vertex and frame sum in reversed order, float32"""
    a = kr.args(kr.inputs(name))
    r = kr.kp_bwd_ref(*a, dtype=np.float32, assoc="leaf", reverse=True)
    over, _ = kr.compare(kr.fwd_groups(r["fwd"]), kr.fwd_bound(name), "fwd f32 leaf/reversed " + name)
    assert not over, over
    over, _ = kr.compare(kr.bwd_groups(r), kr.bwd_bound(name)[0], "bwd f32 leaf/reversed " + name)
    assert not over, over


@pytest.mark.parametrize("defect", kr.DEFECTS)
def test_seeded_defect_falls_outside_the_bound(defect):
    a = kr.args(kr.inputs(SMALL))
    r = kr.kp_bwd_ref(*a, defect=defect)
    over_f, _ = kr.compare(kr.fwd_groups(r["fwd"]), kr.fwd_bound(SMALL), "fwd " + defect)
    over_b, _ = kr.compare(kr.bwd_groups(r), kr.bwd_bound(SMALL)[0], "bwd " + defect)
    assert over_f, defect + " is not seen in the forward outputs"
    assert over_b, defect + " is not seen in the gradients"


def test_the_zero_convention_gives_finite_gradients():
    """two identical consecutive frames and a keypoint declared an exact hit: finite, and the hit keypoint contributes nothing"""
    i = dict(kr.inputs(SMALL))
    i["pose"], i["transl"] = i["pose"].copy(), i["transl"].copy()
    i["pose"][1], i["transl"][1] = i["pose"][0], i["transl"][0]
    a = kr.args(i)
    r = kr.kp_bwd_ref(*a)
    assert all(np.isfinite(r[k]).all() for k in ("d_betas", "d_pose", "d_transl"))
    h = kr.kp_bwd_ref(*a, hit=((0, 3),))
    i["keypoints"] = i["keypoints"].copy()
    i["keypoints"][0, 3, 2] = 0
    z = kr.kp_bwd_ref(*kr.args(i))
    assert all(np.array_equal(h[k], z[k]) for k in ("d_betas", "d_pose", "d_transl")) and not np.array_equal(h["d_pose"], r["d_pose"])


def test_refine_ref_reduces_the_keypoint_error():
    from instantavatar_amd import synthetic
    before, after, losses = kr.refine_ref_drop(synthetic)
    print("refine_ref: mean keypoint pixel error %.4f -> %.4f, loss %.5f -> %.5f" % (before, after, losses[0, 0], losses[-1, 0]))
    assert after < 0.5 * before and losses[-1, 0] < losses[0, 0]


def test_the_module_constants_are_the_references_own():
    """instantavatar_amd.keypoints carries the same map, selection and vertex list as this reference and as the header's comment"""
    from instantavatar_amd import keypoints as K
    assert tuple(K.BODY25_TO_POINT) == tuple(kr.BODY25_TO_POINT) and tuple(K.SMPL_KP_VERTEX) == kr.SMPL_KP_VERTEX and K.MIDHIP == kr.MIDHIP
    from instantavatar_amd import _lib, build
    assert os.path.normpath(_lib.header_path("keypoints")) in [os.path.normpath(h) for h in build.SHARED_HEADERS] and "ia_keypoints.hip" in build.SOURCES
    assert sorted(_lib.declarations("keypoints")) == ["ia_kp_loss_bwd", "ia_kp_loss_fwd", "ia_kp_workspace_bytes"]
