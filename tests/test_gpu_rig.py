"""csrc/ia_rig.hip against tests/gltf_refs.py (float64 numpy, validated in tests/test_cpu_gltf_refs.py): each entry point alone at the
smallest shapes where it can go wrong, then the invariant the export rests on -- a rig with all 24 influences reproduces
`AvatarModel.pose_mesh`, through `skin_rigged` and through the written file evaluated as a viewer would -- and the extract_mesh driver.
Every bound is derived in gltf_refs' docstring; nothing in them comes from a kernel's output.  A device fault in any of these tests
ends the run: nothing more is started on a GPU that has faulted.

measured (MI355X), error over allowance: full weights 0.10 (2.0e-7 of 2.1e-6), normalised weights 0.014, |sum - 1| 0.35; bones 0.13,
quaternions 0.04, root translation 0.15; skinned positions 0.50, normals 0.13; `full` against query_weights 7.5e-7 of 3.3e-5;
skin_rigged against pose_mesh 1.2e-6 of 3.7e-5; the written file evaluated against pose_mesh 8.1e-7 of 1.0e-3 (that allowance lets
every joint up the chain be off by the quaternion's worst case at the body's full reach)."""
import os

import numpy as np
import pytest
import torch

import gltf_refs as gr
import smpl_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _stop_at_the_first_fault():
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:      # the context is gone: every later GPU test would fail on it, or run into the same fault
        pytest.exit("a rig test left the GPU in a failed state (%s): stopping the run" % repr(e)[:200], returncode=3)


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _grid(dims=gr.WEIGHT_DIMS, offset=gr.WEIGHT_OFFSET, scale=gr.WEIGHT_SCALE):
    from instantavatar_amd import _lib
    g = _lib.SnarfGrid()
    g.D, g.H, g.W = dims
    g.offset[:], g.scale[:] = [float(v) for v in offset], [float(v) for v in scale]
    return g


def _weights(x, vol, channel_last, K, want_full=True, pad=3):
    """ia_rig_weights on n points with `pad` sentinel rows behind every output -> numpy (joints, weights, full), twice"""
    from instantavatar_amd import _lib
    n = len(x)
    v = _dev(np.ascontiguousarray(np.moveaxis(vol, 0, -1)) if channel_last else vol)
    xd = _dev(np.concatenate([x, np.full((pad, 3), np.nan, np.float32)]))
    outs = []
    for _ in range(2):
        j = torch.full((n + pad, K), 77, dtype=torch.uint8, device=DEV)
        w, f = torch.full((n + pad, K), 7.0, device=DEV), torch.full((n + pad, 24), 7.0, device=DEV)
        _lib.call("ia_rig_weights", xd, n, v, int(channel_last), _grid(), K, j, w, f if want_full else None)
        outs.append((j, w, f))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs)), "two calls differ"
    j, w, f = (_np(t) for t in outs[0])
    assert (j[n:] == 77).all() and (w[n:] == 7).all() and (f[n:] == 7).all(), "rows past n were written"
    assert want_full or (f == 7).all()
    return j[:n], w[:n], f[:n]


# ---- ia_rig_weights ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channel_last", [False, True])
@pytest.mark.parametrize("n", gr.WEIGHT_SIZES)
def test_weights_against_reference(n, channel_last):
    vol, x = gr.weight_volume(), gr.weight_points(n)
    E = gr.full_bound(gr.WEIGHT_DIMS)
    for K in gr.WEIGHT_KS:
        rj, rw, rfull, kept, order = gr.rig_weights_ref(x, vol, gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE, K)
        j, w, full = _weights(x, vol, channel_last, K)
        err_full = np.abs(full - rfull).max()
        allow_w = gr.topk_weight_bound(E, kept.sum(1), K)[:, None]
        err_w = (np.abs(w - rw) / allow_w).max()
        sums = np.abs(w.astype(np.float64).sum(1) - 1).max()
        print("RIG weights n=%d %s K=%d: full err %.3e (allow %.3e), weights err / allow %.3f, |sum - 1| %.3e (allow %.3e)"
              % (n, "channel-last" if channel_last else "channel-major", K, err_full, E, err_w, sums, gr.G(K + 1)))
        assert err_full <= E and err_w <= 1 and sums <= gr.G(K + 1)
        assert (np.diff(w, axis=1) <= 0).all() and (w >= 0).all()
        # indices: equal to the reference's, except where two reference weights are too close to order
        skip = gr.index_skips(kept, order, rfull, K, E)
        assert skip.sum() * 100 <= n, (int(skip.sum()), n)
        slot_ref = np.take_along_axis(rfull, j.astype(np.int64), 1)                          # the reference weight of the joint named
        near = np.abs(slot_ref - kept) <= 2 * E
        assert ((j == rj) | near)[~skip].all()
        assert all(len(set(r)) == K for r in j[~skip].tolist())                              # K different joints (no weight is 0 here)
        strict = (np.diff(-np.sort(-rfull, 1)[:, :min(K + 1, 24)], axis=1) < -2 * E).all(1)  # no near tie among the first K + 1
        assert np.array_equal(j[strict], rj[strict])
    # without `full`
    j2, w2, _ = _weights(x, vol, channel_last, 4, want_full=False)
    j4, w4, _ = _weights(x, vol, channel_last, 4)
    assert np.array_equal(j2, j4) and np.array_equal(w2, w4)


@pytest.mark.parametrize("channel_last", [False, True])
def test_weights_exact_tie_zero_slots_and_points_without_weights(channel_last):
    x = gr.weight_points(65)
    j, w, full = _weights(x, gr.tie_volume(), channel_last, 2)
    assert np.array_equal(j, np.tile([3, 7], (65, 1)).astype(np.uint8)) and np.array_equal(w, np.full((65, 2), 0.5, np.float32))
    j, w, full = _weights(x, gr.tie_volume(), channel_last, 6)
    assert np.array_equal(j, np.tile([3, 7, 11, 20, 0, 0], (65, 1))) and np.array_equal(w, np.tile(np.float32([0.25] * 4 + [0, 0]), (65, 1)))
    bad = x.copy()
    bad[0, 1], bad[1, 2], bad[2, 0] = np.nan, np.inf, -np.inf
    j, w, full = _weights(bad, gr.weight_volume(), channel_last, 4)
    assert not j[:3].any() and w[:3].tolist() == [[1, 0, 0, 0]] * 3 and not full[:3].any()
    rj, rw = gr.rig_weights_ref(bad, gr.weight_volume(), gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE, 4)[:2]
    assert np.array_equal(j[3:], rj[3:]) and np.isfinite(w).all()
    j, w, full = _weights(x, np.zeros_like(gr.weight_volume()), channel_last, 4)             # weights that sum to 0
    assert not j.any() and w.tolist() == [[1, 0, 0, 0]] * 65 and not full.any()
    far = np.float32([[3e38, -3e38, 1e30], [1e20, 0, 0]])                                    # finite, far outside: the border voxels
    j, w, full = _weights(far, gr.weight_volume(), channel_last, 24)
    rfull = gr.weights_full_ref(far, gr.weight_volume(), gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE)
    assert np.abs(full - rfull).max() <= gr.full_bound(gr.WEIGHT_DIMS)


def test_weights_refusals():
    from instantavatar_amd import _lib
    x, vol = _dev(gr.weight_points(8)), _dev(gr.weight_volume())
    j, w = torch.zeros((8, 4), dtype=torch.uint8, device=DEV), torch.zeros((8, 4), device=DEV)
    for K in (0, 25):
        with pytest.raises(_lib.IAError, match="K = %d" % K):
            _lib.call("ia_rig_weights", x, 8, vol, 0, _grid(), K, j, w, None)
    with pytest.raises(_lib.IAError, match="GPU"):
        _lib.call("ia_rig_weights", x.cpu(), 8, vol, 0, _grid(), 4, j, w, None)
    with pytest.raises(_lib.IAError, match="uint8"):
        _lib.call("ia_rig_weights", x, 8, vol, 0, _grid(), 4, w, w, None)
    assert _lib.call("ia_rig_weights", x, 0, vol, 0, _grid(), 4, j, w, None) == 0


# ---- the synthetic model -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world32():
    """the synthetic model at skinning resolution 32, its mesh at lattice resolution 32, three frames of the golden track"""
    from instantavatar_amd.pipeline import build_synthetic_model
    model = build_synthetic_model(DEV, resolution=32)[0]
    mesh = model.extract_mesh(resolution=32)
    z = np.load(os.path.join(ROOT, "tests", "golden", "aist_demo_200.npz"))
    frames = [0, 57, 140]
    torch.cuda.synchronize()
    return model, mesh, z["poses"][frames, :72].astype(np.float32), z["trans"][frames].astype(np.float32)


def _deformer_arrays(model):
    d, fd = model.deformer, model.deformer.deformer
    return dict(vol=_np(fd.lbs_voxel_final[0]), offset=_np(fd.offset_kernel.reshape(3)), scale=_np(fd.scale_kernel.reshape(3)),
                joints_rest=_np(d._joints_rest.reshape(24, 3)), parents=_np(d._parents32), tfs_inv_t=_np(d.tfs_inv_t.reshape(24, 4, 4)))


def test_full_weights_equal_query_weights_on_the_synthetic_deformer(world32):
    from instantavatar_amd import rig
    model = world32[0]
    fd = model.deformer.deformer
    a = _deformer_arrays(model)
    rng = np.random.default_rng(11)
    lo, hi = _np(fd.bbox)
    x = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), (2049, 3)).astype(np.float32)          # inside and just outside
    j, w, full = rig.weights(model.deformer, _dev(x), 4, full=True)
    want = fd.query_weights(_dev(x))
    torch.cuda.synchronize()
    dims = a["vol"].shape[1:]
    vmax = float(a["vol"].max())
    each = gr.full_bound(dims, vmax, ops=4)
    err = float((full - want).abs().max())
    err_ref = np.abs(_np(full) - gr.weights_full_ref(x, a["vol"], a["offset"], a["scale"])).max()
    print("RIG full vs query_weights on %s: err %.3e (allow 2 x %.3e), vs float64 %.3e" % (dims, err, each, err_ref))
    assert want.shape == (2049, 24) and err <= 2 * each and err_ref <= each
    assert j.dtype == torch.uint8 and j.shape == (2049, 4) and float((w.sum(1) - 1).abs().max()) <= gr.G(5)


# ---- ia_rig_track ------------------------------------------------------------------------------------------------------------------
def _track_poses(F):
    near_pi = sr.make_pose("random", 21)
    near_pi[9:12] *= (np.pi - 5e-4) / np.linalg.norm(near_pi[9:12])                                       # within 1e-3 of pi
    all5 = [np.zeros(72, np.float32), near_pi, sr.make_pose("mixed", 22), sr.make_pose("extreme", 23), sr.make_pose("bigroot", 24)]
    return np.stack(all5[:F]).astype(np.float32)


@pytest.mark.parametrize("F", [1, 2, 5])
def test_track_against_reference_and_ia_smpl_tfs(F):
    from instantavatar_amd import _lib
    i = sr.tfs_inputs("smpl-random")
    poses = _track_poses(F)
    transl = (np.random.default_rng(F).standard_normal((F, 3)) * 0.5 + [0, 0.15, 5]).astype(np.float32)
    J, par, B = _dev(i["joints_rest"]), _dev(i["parents"]), _dev(i["tfs_inv_t"])
    outs = []
    for _ in range(2):
        bones, quat, root = torch.full((F + 1, 24, 4, 4), 7.0, device=DEV), torch.full((F + 1, 24, 4), 7.0, device=DEV), torch.full((F + 1, 3), 7.0, device=DEV)
        _lib.call("ia_rig_track", J, par, _dev(poses), _dev(transl), B, F, bones, quat, root)
        outs.append((bones, quat, root))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs)), "two calls differ"
    bones, quat, root = (_np(t) for t in outs[0])
    assert (bones[F] == 7).all() and (quat[F] == 7).all() and (root[F] == 7).all(), "frames past F were written"
    bound = gr.track_bound(i["joints_rest"], i["parents"], poses, transl, i["tfs_inv_t"])
    got = {"bones.R": bones[:F, :, :3, :3], "bones.t": bones[:F, :, :3, 3], "bones.row3": bones[:F, :, 3, :], "quat": quat[:F], "root_t": root[:F]}
    for k, (ref, allow) in bound.items():
        err = float(np.abs(got[k].astype(np.float64) - ref).max())
        print("RIG track F=%d %-10s err %.3e  allow %.3e" % (F, k, err, allow))
        assert err <= allow, k
    assert np.abs(np.linalg.norm(quat[:F].astype(np.float64), axis=-1) - 1).max() <= 4 * gr.U
    # the same frames through ia_smpl_tfs: bones = its A times tfs_inv_t
    for f in range(F):
        tfs, w2s, A = torch.empty((24, 4, 4), device=DEV), torch.empty((4, 4), device=DEV), torch.empty((24, 4, 4), device=DEV)
        _lib.call("ia_smpl_tfs", J, par, _dev(poses[f]), _dev(transl[f]), B, tfs, w2s, A)
        prod = _np(A).astype(np.float64) @ i["tfs_inv_t"].astype(np.float64)
        a = sr._fwd_case("tfs", sr.tfs_fwd_ref, (i["joints_rest"], i["parents"], poses[f], transl[f], i["tfs_inv_t"]))
        absB = np.abs(i["tfs_inv_t"].astype(np.float64))
        # A within its allowance of the exact A, times |tfs_inv_t|; bones within theirs
        thru = (a["A.R"][1] * absB[:, :3, :].sum(1) + a["A.t"][1] * absB[:, 3:, :].sum(1)).max()
        err = np.abs(prod - bones[f].astype(np.float64)).max()
        allow = thru + max(bound["bones.R"][1], bound["bones.t"][1])
        print("RIG track F=%d frame %d bones vs ia_smpl_tfs: err %.3e  allow %.3e" % (F, f, err, allow))
        assert err <= allow
    # quat and root_t are optional, transl too
    b2 = torch.empty((F, 24, 4, 4), device=DEV)
    _lib.call("ia_rig_track", J, par, _dev(poses), _dev(transl), B, F, b2, None, None)
    b3, r3 = torch.empty((F, 24, 4, 4), device=DEV), torch.empty((F, 3), device=DEV)
    _lib.call("ia_rig_track", J, par, _dev(poses), None, B, F, b3, None, r3)
    torch.cuda.synchronize()
    assert torch.equal(b2, outs[0][0][:F]) and np.array_equal(_np(r3), np.tile(i["joints_rest"][0], (F, 1)))
    assert np.abs(_np(b3)[:, :, :3, :3] - bones[:F, :, :3, :3]).max() == 0


# ---- ia_rig_skin -------------------------------------------------------------------------------------------------------------------
def _skin_inputs(n, K, F, seed):
    rng = np.random.default_rng(seed)
    x, nn = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    nn[0] = 0                                                                  # a zero normal stays zero
    j = rng.integers(0, 24, (n, K)).astype(np.uint8)
    w = rng.random((n, K)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    i = sr.tfs_inputs("smpl-random")
    poses = np.stack([sr.make_pose("random", 30 + f) for f in range(F)])
    transl = (rng.standard_normal((F, 3)) + [0, 0, 5]).astype(np.float32)
    bones = gr.track_ref(i["joints_rest"], i["parents"], poses, transl, i["tfs_inv_t"])["bones"].astype(np.float32)
    return x, nn, j, w, bones


@pytest.mark.parametrize("K", [1, 4, 5, 8, 24])
@pytest.mark.parametrize("n", [1, 65, 300])
def test_skin_against_reference(n, K):
    from instantavatar_amd import _lib
    for F in (1, 3, 35):                                                       # 35 frames: a launch split over the frames (one range per frame at these sizes)
        x, nn, j, w, bones = _skin_inputs(n, K, F, 1000 * n + 10 * K + F)
        if n > 1:
            j[1, 0] = 200                                                      # an index above 23 is read as 23
        p_ref, n_ref = gr.lbs_ref(x, nn, j, w, bones)
        p_allow, n_allow = gr.skin_bound(x, nn, j, w, bones)
        xd, nd, jd, wd, bd = _dev(x), _dev(nn), _dev(j), _dev(w), _dev(bones)
        for with_normals in (True, False):
            outs = []
            for _ in range(2):
                pv, pn = torch.full((F + 1, n, 3), 7.0, device=DEV), torch.full((F + 1, n, 3), 7.0, device=DEV)
                _lib.call("ia_rig_skin", xd, nd if with_normals else None, n, jd, wd, K, bd, F, pv, pn if with_normals else None)
                outs.append((pv, pn))
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(*outs)), "two calls differ"
            pv, pn = (_np(t) for t in outs[0])
            assert (pv[F] == 7).all() and (pn[F] == 7).all() and (with_normals or (pn == 7).all()), "rows past F frames were written"
            ratio = float((np.abs(pv[:F] - p_ref) / p_allow).max())
            assert ratio <= 1, (n, K, F, ratio)
            if with_normals:
                ratio_n = float((np.abs(pn[:F] - n_ref) / n_allow).max())
                assert ratio_n <= 1 and (pn[:F, 0] == 0).all(), (n, K, F, ratio_n)
                assert np.abs(np.linalg.norm(pn[:F, 1:].astype(np.float64), axis=-1) - 1).max(initial=0.0) <= 4 * gr.U
                print("RIG skin n=%d K=%d F=%d: position err / allow %.3f, normal err / allow %.3f" % (n, K, F, ratio, ratio_n))


def test_skin_walks_several_lds_stages_per_workgroup():
    """one vertex tile and 17 * 8192 frames: the launch is split into 8192 frame ranges of 17 frames, two LDS stages (16 + 1) each;
    the bones repeat with period 37, so every frame must equal, bit for bit, that frame of a 37-frame call"""
    from instantavatar_amd import _lib
    n, K, P = 3, 2, 37
    F = 17 * 8192
    x, nn, j, w, bones = (_dev(a) for a in _skin_inputs(n, K, P, 5))
    small_v, small_n = torch.empty((P, n, 3), device=DEV), torch.empty((P, n, 3), device=DEV)
    _lib.call("ia_rig_skin", x, nn, n, j, w, K, bones, P, small_v, small_n)
    idx = torch.arange(F, device=DEV) % P
    big_v, big_n = torch.full((F + 1, n, 3), 7.0, device=DEV), torch.full((F + 1, n, 3), 7.0, device=DEV)
    _lib.call("ia_rig_skin", x, nn, n, j, w, K, bones[idx].contiguous(), F, big_v, big_n)
    torch.cuda.synchronize()
    assert torch.equal(big_v[:F], small_v[idx]) and torch.equal(big_n[:F], small_n[idx])
    assert bool((big_v[F] == 7).all()) and bool((big_n[F] == 7).all())


def test_skin_refusals():
    from instantavatar_amd import _lib
    x, nn, j, w, bones = (_dev(a) for a in _skin_inputs(8, 4, 2, 1))
    out = torch.empty((2, 8, 3), device=DEV)
    for K in (0, 25):
        with pytest.raises(_lib.IAError, match="K = %d" % K):
            _lib.call("ia_rig_skin", x, None, 8, j, w, K, bones, 2, out, None)
    with pytest.raises(_lib.IAError, match="GPU"):
        _lib.call("ia_rig_skin", x.cpu(), None, 8, j, w, 4, bones, 2, out, None)
    with pytest.raises(_lib.IAError, match="together"):
        _lib.call("ia_rig_skin", x, nn, 8, j, w, 4, bones, 2, out, None)
    assert _lib.call("ia_rig_skin", x, None, 0, j, w, 4, bones, 2, out, None) == 0


# ---- the invariant -----------------------------------------------------------------------------------------------------------------
def test_a_rig_with_all_influences_reproduces_pose_mesh_and_so_does_the_written_file(world32, tmp_path):
    from instantavatar_amd import rig as rig_mod
    from instantavatar_amd.pipeline import make_batch
    model, mesh, poses, trans = world32
    a = _deformer_arrays(model)
    n = mesh.verts.shape[0]
    assert n > 500
    r24 = model.rig_mesh(mesh, influences=24)
    assert r24.joints.shape == (n, 24) and r24.weights.dtype == torch.float32 and r24.inverse_bind.shape == (24, 4, 4)
    xv, xn = model.skin_rigged(mesh, r24, _dev(poses), _dev(trans))
    posed = [model.pose_mesh(mesh, make_batch(DEV, 8, poses[f], trans[f])) for f in range(3)]
    want = np.stack([_np(p.verts) for p in posed]).astype(np.float64)
    torch.cuda.synchronize()
    assert xv.shape == (3, n, 3) and xn.shape == (3, n, 3)
    # the vertices inside the weight volume: outside it the transform grid is padded with zeros, the weights with the border
    x = _np(mesh.verts).astype(np.float64)
    g = a["scale"].astype(np.float64) * (x + a["offset"].astype(np.float64))
    inside = (np.abs(g) < 1 - 1e-4).all(1)
    print("RIG invariant: %d vertices, %d inside the weight volume" % (n, int(inside.sum())))
    assert inside.mean() > 0.5
    full = gr.weights_full_ref(x[inside], a["vol"], a["offset"], a["scale"])
    fps = 30.0
    path = str(tmp_path / "avatar.glb")
    bones, quat, root_t = rig_mod.track(model.deformer, _dev(poses), _dev(trans))
    mesh.to_glb(path, r24, (quat, root_t), fps)
    doc, binary = gr.read_glb(path)
    glb = gr.glb_terms(x[inside], _np(r24.joints)[inside], _np(r24.weights)[inside], r24.inverse_bind, r24.rest_translation, r24.parents, poses)
    got = _np(xv).astype(np.float64)
    for f in range(3):
        t = gr.invariant_terms(x[inside], full, a["joints_rest"], a["parents"], poses[f], trans[f], a["tfs_inv_t"])
        allow = t["pose"] + t["renorm"] + t["rig"]
        err = float(np.abs(got[f][inside] - want[f][inside]).max())
        print("RIG invariant frame %d: skin_rigged vs pose_mesh max %.3e, allow %.3e (pose %.2e, renorm %.2e, rig %.2e)"
              % (f, err, allow, t["pose"], t["renorm"], t["rig"]))
        assert err <= allow
        ev = gr.skinned(doc, binary, f / fps)[0]
        allow_file = t["pose"] + t["renorm"] + gr.G(36) * t["mag_world"] + glb[f]
        err_file = float(np.abs(ev[inside] - want[f][inside]).max())
        print("RIG invariant frame %d: file evaluated vs pose_mesh max %.3e, allow %.3e (file terms %.2e)" % (f, err_file, allow_file, glb[f]))
        assert err_file <= allow_file
    # the default pose of the file is the canonical mesh; fewer influences deviate, and the report says by how much
    assert np.abs(gr.skinned(doc, binary)[0] - x).max() < 1e-5
    devs = []
    for K in (4, 8):
        rk = model.rig_mesh(mesh, influences=K)
        mx, mean = rig_mod.deviation(model.skin_rigged(mesh, rk, _dev(poses), _dev(trans))[0], torch.as_tensor(want, device=DEV))
        devs.append(float(mx.max()))
        print("RIG deviation of %d influences from pose_mesh: max %.3e, mean %.3e" % (K, float(mx.max()), float(mean.mean())))
    assert np.isfinite(devs).all()
    # chunked skinning returns the same values from the host
    cv, cn = rig_mod.skin(r24, mesh, bones, chunk=2)
    assert not cv.is_cuda and torch.equal(cv, xv.cpu()) and torch.equal(cn, xn.cpu())


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_extract_mesh_driver_with_a_rig(tmp_path, capsys):
    import io
    import re
    from PIL import Image
    from instantavatar_amd.drivers import extract_mesh as drv
    z = np.load(os.path.join(ROOT, "tests", "golden", "aist_demo_200.npz"))
    np.savez(tmp_path / "track.npz", poses=z["poses"][[0, 57, 140]], trans=z["trans"][[0, 57, 140]])
    common = ["--synthetic", "--resolution", "32", "--texture", "4", "--poses", str(tmp_path / "track.npz")]
    assert drv.main(common + ["--out", str(tmp_path / "plain")]) == 0
    said = capsys.readouterr().out
    assert "rig:" not in said and "avatar.glb" not in os.listdir(tmp_path / "plain")
    assert drv.main(common + ["--rig", "4", "--out", str(tmp_path / "rig")]) == 0
    said = capsys.readouterr().out
    before = sorted(os.listdir(tmp_path / "plain"))
    assert sorted(os.listdir(tmp_path / "rig")) == sorted(before + ["avatar.glb"])
    for name in before:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "rig" / name, "rb").read(), name
    m = re.search(r"rig: 4 influences per vertex deviate from the posed meshes by at most ([\d.e+-]+), ([\d.e+-]+) on average over 3 frames", said)
    assert m and 0 <= float(m.group(2)) <= float(m.group(1)) < 1.0, said[-2000:]
    doc, binary = gr.read_glb(str(tmp_path / "rig" / "avatar.glb"))
    at = gr.primitive(doc, binary)
    nf = sum(1 for line in open(tmp_path / "rig" / "canonical_textured.obj") if line.startswith("f "))
    assert len(doc["skins"][0]["joints"]) == 24 and len(at["POSITION"]) == 3 * nf and "TEXCOORD_0" in at and "JOINTS_0" in at and "JOINTS_1" not in at
    times = gr.accessor(doc, binary, doc["animations"][0]["samplers"][0]["input"])[:, 0]
    assert np.array_equal(times, (np.arange(3) / 30.0).astype(np.float32))
    v = doc["bufferViews"][doc["images"][0]["bufferView"]]
    png = Image.open(io.BytesIO(binary[v["byteOffset"]:v["byteOffset"] + v["byteLength"]]))
    assert np.array_equal(np.asarray(png), np.asarray(Image.open(tmp_path / "rig" / "canonical_textured.png")))
