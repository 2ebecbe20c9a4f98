"""Pins tests/deformer_refs.py itself (no GPU).  (a) The float64 restatements equal float64 torch on the CPU --
grid_sample(align_corners=True, padding_mode="border") on the 5-D volume for the weights, autograd through the reference's
formulation for the two gradients -- and the project's oracle lies within the K u M bounds of the same inputs.  (b) The
same expressions in plain numpy fp32, in sequential and in pairwise association, stay inside the bounds on every input set
of tests/test_gpu_deformer_kernels.py.  (c) Eleven seeded defects, applied to the restatement, each exceed the bound in at
least one element on the same inputs."""
import numpy as np
import pytest
import torch

import deformer_refs as dr

F64 = torch.float64


def _ratio(got, ref, bound, what, expect_inside=True):
    """worst |got - ref| / bound; where the bound is 0 the value must be exactly the reference's"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    err[np.isnan(err)] = np.inf
    z = bound == 0
    r = float((err[~z] / bound[~z]).max()) if (~z).any() else 0.0
    if z.any() and (err[z] != 0).any():
        r = np.inf
    if expect_inside:
        print("RATIO cpu %-56s %.4f" % (what, r))
        assert r <= 1.0, (what, r)
    return r


def _close(a, b, scale, what, rel=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b)
    tol = rel * np.maximum(np.asarray(scale, np.float64), 1e-300)
    assert (err <= tol).all(), (what, float((err / tol).max()))


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _tfs_torch(tfs):
    t = np.asarray(tfs, np.float64).copy()
    t[:, 3, :] = (0, 0, 0, 1)          # (the inputs hold NaN there; autograd must find no gradient for it either)
    return _t(t).requires_grad_()


def _grid_sample(inp, x):
    """query_weights (deformer_torch.py:190-202) in float64 torch: [n,24]"""
    g = inp["grid"]
    vol = _t(inp["cm"])[None]
    q = (_t(x) + _t(g.offset)) * _t(g.scale)
    return torch.nn.functional.grid_sample(vol, q[None, None, None], align_corners=True, mode="bilinear", padding_mode="border")[0, :, 0, 0].T


CASES = [(dims, n, layout) for n in dr.ENTRY_COUNTS for dims, layout in zip(dr.SAMPLE_VOLUMES, ("dense", "compact"))] + \
        [(dims, n, layout) for n in dr.ENTRY_COUNTS[1:3] for dims, layout in zip(dr.SAMPLE_VOLUMES, ("compact", "dense"))]
SPECIAL = [(dr.SAMPLE_VOLUMES[0], 257, "compact", "over"), (dr.SAMPLE_VOLUMES[1], 257, "compact", "zero")]


def _inputs(dims, n, layout, rule="default", n_init=13):
    return dr.sampling_inputs(dims, n, layout, n_init, rule)


def _implicit(inp, **kw):
    return dr.implicit_bwd_ref(inp["xc"], inp["J_inv"], inp["live"], inp["grad"], kw.pop("vol", inp["cm"]), inp["grid"], inp["prefill"], **kw)


def _inverse(inp, **kw):
    return dr.inverse_skinning_ref(inp["xc"], inp["xd"], inp["pt"], inp["live"], kw.pop("vol", inp["cl"]), inp["grid"], inp["tfs"], inp["grad"],
                                   inp["prefill"], **kw)


# ---- the input sets hold what they promise ----------------------------------------------------------------------------
def test_input_sets_reach_the_paths_they_name():
    for (dims, want) in dr.PRECOMPUTE_GRIDS:
        n_thr, blocks, variant = dr.precompute_variant(*dims)
        assert variant == want and dims[2] % 4 == 0, (dims, n_thr, blocks, variant)
    assert dr.precompute_variant(3, 5, 12)[0] == 45 and dr.precompute_variant(4, 8, 40)[:2] == (320, 2)
    assert dr.precompute_variant(5, 16, 20)[0] % 64 != 0 and dr.precompute_variant(4, 8, 64)[:2] == (512, 2)
    # the large case: the smallest count above 1024 full tiles; two workgroups take a second trip
    assert dr.implicit_blocks(dr.BIG_N) == 1024 and dr.implicit_blocks(dr.BIG_N - 300) == 1024 and dr.BIG_N == 262444
    assert (dr.BIG_N + dr.TILE - 1) // dr.TILE == 1026
    for dims in dr.SAMPLE_VOLUMES:
        inp = _inputs(dims, 785, "dense")
        g, x, live = inp["grid"], inp["xc"], inp["live"]
        assert 0.2 < (~live).mean() < 0.4 and np.isnan(x[~live]).all() and np.isnan(inp["J_inv"][~live]).all() and np.isnan(inp["grad"][~live]).all()
        gn, c = dr.voxel_index(g, x[live], np.float32)
        top = np.array(g.sizes, np.float32) - 1
        for a in range(3):
            assert (c[:, a] == 0).any() and (c[:, a] == top[a]).any(), "a face is missing"
            inner = (c[:, a] > 0) & (c[:, a] < top[a])
            assert (inner & (c[:, a] == np.floor(c[:, a]))).any(), "no interior node"
        assert ((c == np.floor(c)) & (c >= 0) & (c <= top)).all(1).any(), "no point on a node along all axes"
        assert (np.abs(gn) > 1).any(1).sum() >= 8 and np.abs(gn).max() > 2 and inner.sum() > 300
        assert (inp["grad"][live] == 0).all(1).any() and ((inp["grad"][live] == 0).sum(1) == 1).any()
        mag = np.abs(inp["J_inv"][live]).max(1)
        assert mag.max() / mag.min() > 30 and (inp["J_inv"][live] < 0).any() and (inp["J_inv"][live] > 0).any()
        cm, cl = inp["cm"], inp["cl"]
        assert np.array_equal(np.moveaxis(cm, 0, -1), cl) and (cm >= 0).all() and (cl.max(-1) == 1).sum() >= 2
        assert np.abs(cl.astype(np.float64).sum(-1) - 1).max() < 4e-7
        assert np.isnan(inp["tfs"][:, 3]).all() and g.scale[2] == g.scale[0] * 4 and (inp["prefill"] != 0).all()
    c = _inputs(dr.SAMPLE_VOLUMES[1], 785, "compact")
    assert c["n_cand"] < 0.7 * c["n"] and (c["pt_cnt"] == 0).any() and (c["pt_cnt"] == 13).any() and int(c["pt_cnt"].sum()) == 785


# ---- (a) the references are right -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", dr.SAMPLE_VOLUMES)
def test_sampled_weights_equal_grid_sample(dims):
    inp = _inputs(dims, 785, "dense")
    x = inp["xc"][inp["live"]]
    w_cm, dw, allow = dr.sample_weights_ref(inp["cm"], inp["grid"], x)
    w_cl, _, _ = dr.sample_weights_ref(inp["cl"], inp["grid"], x)
    assert np.array_equal(w_cm, w_cl)
    _close(w_cm, _grid_sample(inp, x).numpy(), 1.0, "weights vs grid_sample")
    # the derivative is the slope of the sample: central differences in the voxel index, away from the nodes and the clamp
    g, c = dr.voxel_index(inp["grid"], x)
    top = np.array(inp["grid"].sizes) - 1.0
    h = 1e-6
    V = dr.channel_last(inp["cl"], inp["grid"]).astype(np.float64)
    ok = ((c - np.floor(c) > 1e-3) & (np.ceil(c) - c > 1e-3) & (c > 0) & (c < top)).all(1)
    assert ok.sum() > 200
    for a in range(3):
        e = np.zeros(3)
        e[a] = h
        num = (dr._trilinear(V, c[ok] + e, inp["grid"].sizes)[0] - dr._trilinear(V, c[ok] - e, inp["grid"].sizes)[0]) / (2 * h)
        _close(dw[ok][:, a], num, 1.0, "dw/dc axis %d" % a, rel=1e-8)


@pytest.mark.parametrize("dims,n,layout", CASES[2:6])
def test_gradient_references_equal_autograd(dims, n, layout):
    inp = _inputs(dims, n, layout)
    live = inp["live"]
    x, J, g = _t(inp["xc"][live]), _t(inp["J_inv"][live].reshape(-1, 3, 3)), _t(inp["grad"][live])
    w = _grid_sample(inp, inp["xc"][live])
    # version 1 (deformer_torch.py:50-67): x_c* - J_inv (d(x_c*) - sg[d(x_c*)])
    tfs = _tfs_torch(inp["tfs"])
    T = torch.einsum("pn,nij->pij", w, tfs)
    d = torch.einsum("pij,pj->pi", T, torch.cat([x, torch.ones(len(x), 1, dtype=F64)], 1))[:, :3]
    xc = x - torch.einsum("pij,pj->pi", J, d - d.detach())
    (xc * g).sum().backward()
    ref = _implicit(inp)
    want = tfs.grad.numpy() + inp["prefill"].astype(np.float64)
    _close(ref["d_tfs"], want, ref["M"] + 1e-30, "implicit d_tfs vs autograd")
    assert np.array_equal(ref["d_tfs"][:, 3], inp["prefill"][:, 3].astype(np.float64))
    assert np.array_equal(_implicit(inp, vol=inp["cl"])["d_tfs"], ref["d_tfs"])
    # version 2 (deformer_torch.py:68-75): (x_d - t) @ R
    tfs = _tfs_torch(inp["tfs"])
    xd = _t(inp["xd"][inp["pt"][live]]).requires_grad_()
    T = torch.einsum("pn,nij->pij", w, tfs)
    out = torch.einsum("pi,pij->pj", xd - T[:, :3, 3], T[:, :3, :3])
    (out * g).sum().backward()
    r2 = _inverse(inp)
    _close(r2["out"][live], out.detach().numpy(), 4.0, "inverse skinning value vs torch")
    assert (r2["out"][~live] == 0).all() and (r2["d_xd"][~live] == 0).all()
    _close(r2["d_tfs"], tfs.grad.numpy() + inp["prefill"].astype(np.float64), r2["M"] + 1e-30, "inverse skinning d_tfs vs autograd")
    _close(r2["d_xd"][live], xd.grad.numpy(), 4.0 * np.abs(inp["grad"][live]).max(), "d_xd_entry vs autograd")


@pytest.mark.parametrize("dims,n,layout", CASES[2:6])
def test_oracle_lies_within_the_bounds(oracle, dims, n, layout):
    inp = _inputs(dims, n, layout)
    g, live = inp["grid"], inp["live"]
    init = dict(lbs_voxel=inp["cm"], offset_kernel=g.offset, scale_kernel=g.scale, D=g.D, H=g.H, W=g.W)
    tfs = np.nan_to_num(inp["tfs"], nan=0.0)
    z = lambda a: np.where(np.isnan(a), np.float32(0), a)           # (the oracle masks AFTER reading: finite fill in the dead rows)
    w, _, allow = dr.sample_weights_ref(inp["cm"], g, inp["xc"][live])
    _ratio(oracle.query_weights(init, inp["xc"][live]), w, dr.weight_error(w, allow) + dr.U * w, "oracle weights %d %s" % (n, layout))
    ref = _implicit(inp)
    got = oracle.implicit_diff_grad(init, z(inp["xc"]), z(inp["J_inv"]), live, z(inp["grad"])).astype(np.float64) + inp["prefill"]
    got[:, 3] = inp["prefill"][:, 3]
    _ratio(got, ref["d_tfs"], dr.bound_implicit(ref, n), "oracle implicit d_tfs %d %s" % (n, layout))
    if layout == "dense":
        ni = inp["n_init"]
        P = inp["P"]
        pad = P * ni - n
        xc = np.concatenate([z(inp["xc"]), np.zeros((pad, 3), np.float32)]).reshape(P, ni, 3)
        go = np.concatenate([z(inp["grad"]), np.zeros((pad, 3), np.float32)]).reshape(P, ni, 3)
        m = np.concatenate([live, np.zeros(pad, bool)]).reshape(P, ni)
        val, d_tfs = oracle.inverse_skinning(init, xc, inp["xd"], m, tfs, go)
        r2 = _inverse(inp)
        _ratio(val.reshape(-1, 3)[:n], r2["out"], r2["b_out"] + dr.U * np.abs(r2["out"]), "oracle inverse skinning value %d" % n)
        got = d_tfs.astype(np.float64) + inp["prefill"]
        got[:, 3] = inp["prefill"][:, 3]
        _ratio(got, r2["d_tfs"], dr.bound_inverse_bwd(r2, n), "oracle inverse skinning d_tfs %d" % n)


@pytest.mark.parametrize("dims,want", dr.PRECOMPUTE_GRIDS)
def test_precompute_reference(oracle, dims, want):
    grid = dr.make_grid(*dims)
    cm, cl = dr.make_volume(grid)
    tfs = dr.make_tfs()
    ref = dr.precompute_ref(cm, tfs, grid)
    assert np.array_equal(dr.precompute_ref(cl, tfs, grid)["voxel_J"], ref["voxel_J"])
    # float64 torch: einsum of the weights with the transforms, the centres from linspace
    T = np.nan_to_num(tfs.astype(np.float64), nan=0.0)
    J = torch.einsum("dhwn,nq->dhwq", _t(cl), _t(T.reshape(24, 16)[:, :12])).numpy()
    _close(ref["voxel_J"], J, 4.0, "voxel_J vs einsum")
    lin = [(np.linspace(-1, 1, s) / float(grid.scale[a]) - float(grid.offset[a])) for a, s in enumerate(grid.sizes)]
    cz, cy, cx = np.meshgrid(lin[2], lin[1], lin[0], indexing="ij")
    h = np.stack([cx, cy, cz, np.ones_like(cx)], -1)
    d = np.einsum("dhwck,dhwk->cdhw", J.reshape(*dims, 3, 4), h)
    _close(ref["voxel_d"], d, 8.0, "voxel_d vs einsum", rel=1e-10)
    assert np.array_equal(ref["bbox"], np.concatenate([ref["voxel_d"].reshape(3, -1).min(1), ref["voxel_d"].reshape(3, -1).max(1)]))
    # the oracle (the reference's kernel restated, pinned to it by tests/test_ref_pin.py)
    init = dict(lbs_voxel=cm, offset_kernel=grid.offset, scale_kernel=grid.scale, D=grid.D, H=grid.H, W=grid.W)
    vJ, vd = oracle.precompute(init, np.nan_to_num(tfs, nan=0.0))
    _ratio(np.moveaxis(vJ, 0, -1), ref["voxel_J"], ref["b_J"], "oracle voxel_J %s" % (dims,))
    _ratio(vd, ref["voxel_d"], ref["b_d"], "oracle voxel_d %s" % (dims,))
    # (b) plain fp32 in two association orders
    for order in ("seq", "pair"):
        f = dr.precompute_ref(cm, tfs, grid, np.float32, order)
        assert f["voxel_J"].dtype == np.float32 and f["voxel_d"].dtype == np.float32
        _ratio(f["voxel_J"], ref["voxel_J"], ref["b_J"], "fp32 %s voxel_J %s" % (order, dims))
        _ratio(f["voxel_d"], ref["voxel_d"], ref["b_d"], "fp32 %s voxel_d %s" % (order, dims))
        _ratio(f["bbox"], ref["bbox"], ref["b_box"], "fp32 %s bbox %s" % (order, dims))
    # (c) the box without the lanes of a ragged wave
    if dr.precompute_variant(*dims)[0] % 64:
        bad = dr.precompute_ref(cm, tfs, grid, defect="box_ragged_wave")
        assert _ratio(bad["bbox"], ref["bbox"], ref["b_box"], "", expect_inside=False) > 1, dims


def test_expand_candidate_points_reference():
    for P in (1, 255, 257):
        e = dr.expand_inputs(P)
        assert (e["pt_cnt"] == 13).any() and (P == 1 or (e["pt_cnt"] == 0).any()) and e["cap"] < e["total"]
        full = dr.expand_candidate_points_ref(e["pt_off"], e["pt_cnt"], P, None, e["total"], np.full(e["total"] + 8, -7, np.int32))
        assert np.array_equal(full[:e["total"]], np.repeat(np.arange(P), e["pt_cnt"])) and (full[e["total"]:] == -7).all()
        cut = dr.expand_candidate_points_ref(e["pt_off"], e["pt_cnt"], P, e["n_pts"], e["cap"], np.full(e["total"] + 8, -7, np.int32))
        lim = min(e["cap"], int(e["pt_cnt"][:e["n_pts"]].sum()))
        assert np.array_equal(cut[:lim], full[:lim]) and (cut[lim:] == -7).all()


# ---- (b) plain fp32 attains the bounds --------------------------------------------------------------------------------
def _fp32_inside(inp, n, tag):
    ref, r2 = _implicit(inp), _inverse(inp)
    for order in ("seq", "pair"):
        for vol in ("cm", "cl"):
            f = _implicit(inp, vol=inp[vol], dtype=np.float32, order=order)
            assert f["d_tfs"].dtype == np.float32
            _ratio(f["d_tfs"], ref["d_tfs"], dr.bound_implicit(ref, n), "fp32 %s %s implicit d_tfs %s" % (order, vol, tag))
        f = _inverse(inp, dtype=np.float32, order=order)
        _ratio(f["out"], r2["out"], r2["b_out"], "fp32 %s inverse skinning value %s" % (order, tag))
        _ratio(f["d_tfs"], r2["d_tfs"], dr.bound_inverse_bwd(r2, n), "fp32 %s inverse skinning d_tfs %s" % (order, tag))
        _ratio(f["d_xd"], r2["d_xd"], r2["b_d_xd"], "fp32 %s inverse skinning d_xd %s" % (order, tag))
    return ref, r2


@pytest.mark.parametrize("dims,n,layout", CASES)
def test_plain_fp32_stays_inside(dims, n, layout):
    _fp32_inside(_inputs(dims, n, layout), n, "%d %s" % (n, layout))


@pytest.mark.parametrize("dims,n,layout,rule", SPECIAL)
def test_plain_fp32_stays_inside_special_counts(dims, n, layout, rule):
    inp = _inputs(dims, n, layout, rule)
    ref, r2 = _fp32_inside(inp, n, "%d %s" % (n, rule))
    if rule == "zero":
        assert np.array_equal(ref["d_tfs"], inp["prefill"].astype(np.float64)) and (r2["out"] == 0).all() and (r2["d_xd"] == 0).all()
    else:
        assert inp["live"].all()


# ---- (c) the bounds are sharp: every seeded defect leaves them --------------------------------------------------------
SAMPLING_DEFECTS = ("zero_padding", "align_corners_false", "shift_bone_plane")
V1_DEFECTS = SAMPLING_DEFECTS + ("J_not_transposed", "h_without_one", "drop_last_partial_block", "read_past_live", "overwrite")
V2_DEFECTS = SAMPLING_DEFECTS + ("v2_translation_sign", "drop_last_partial_block", "read_past_live", "overwrite")


@pytest.mark.parametrize("dims,n,layout", [CASES[4], CASES[7]])
def test_seeded_defects_break_the_bounds(dims, n, layout):
    inp = _inputs(dims, n, layout)
    ref, r2 = _implicit(inp), _inverse(inp)
    b1, b2 = dr.bound_implicit(ref, n), dr.bound_inverse_bwd(r2, n)
    x = inp["xc"][inp["live"]]
    w, _, allow = dr.sample_weights_ref(inp["cm"], inp["grid"], x)
    for defect in SAMPLING_DEFECTS:
        bad = dr.sample_weights_ref(inp["cm"], inp["grid"], x, defect=defect, want_allow=False)[0]
        assert _ratio(bad, w, dr.weight_error(w, allow), "", expect_inside=False) > 1, defect
    for defect in V1_DEFECTS:
        r = _ratio(_implicit(inp, defect=defect)["d_tfs"], ref["d_tfs"], b1, "", expect_inside=False)
        print("DEFECT implicit %-28s error / bound %.3g" % (defect, r))
        assert r > 1, defect
    for defect in V2_DEFECTS:
        bad = _inverse(inp, defect=defect)
        r = _ratio(bad["d_tfs"], r2["d_tfs"], b2, "", expect_inside=False)
        print("DEFECT inverse skinning %-20s error / bound %.3g" % (defect, r))
        assert r > 1, defect
        if defect in SAMPLING_DEFECTS:
            assert _ratio(bad["out"], r2["out"], r2["b_out"], "", expect_inside=False) > 1, defect
    assert _ratio(_inverse(inp, defect="v2_translation_sign")["d_xd"], r2["d_xd"], r2["b_d_xd"], "", expect_inside=False) == 0   # (its d_xd is R g all the same)


def test_large_case_second_trip():
    """262 444 entries: plain fp32 stays inside in both orders, and a second tile that overwrites the first does not"""
    inp = _inputs(dr.SAMPLE_VOLUMES[1], dr.BIG_N, "compact", "nearly_all")
    assert inp["n_cand"] > dr.MAX_BLOCKS * dr.TILE + dr.TILE
    ref = _implicit(inp, vol=inp["cl"])
    b = dr.bound_implicit(ref, dr.BIG_N)
    for order in ("seq", "pair"):
        _ratio(_implicit(inp, vol=inp["cl"], dtype=np.float32, order=order)["d_tfs"], ref["d_tfs"], b, "fp32 %s implicit d_tfs large" % order)
    for defect in ("second_tile_overwrites", "drop_last_partial_block"):
        r = _ratio(_implicit(inp, vol=inp["cl"], defect=defect)["d_tfs"], ref["d_tfs"], b, "", expect_inside=False)
        print("DEFECT implicit large %-24s error / bound %.3g" % (defect, r))
        assert r > 1, defect
    dense = _inputs(dr.SAMPLE_VOLUMES[0], dr.BIG_N, "dense", "nearly_all")
    r2 = _inverse(dense)
    b2 = dr.bound_inverse_bwd(r2, dr.BIG_N)
    _ratio(_inverse(dense, dtype=np.float32, order="pair")["d_tfs"], r2["d_tfs"], b2, "fp32 pair inverse skinning d_tfs large")
    r = _ratio(_inverse(dense, defect="second_tile_overwrites")["d_tfs"], r2["d_tfs"], b2, "", expect_inside=False)
    print("DEFECT inverse skinning large second_tile_overwrites error / bound %.3g" % r)
    assert r > 1
