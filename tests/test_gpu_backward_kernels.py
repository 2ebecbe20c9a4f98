"""The kernels that produce the gradients of a training step, each called alone through the C ABI on seeded host-built inputs
and compared with the float64 restatements of tests/backward_refs.py: the compositor (forward and backward), the candidate
selection, the hash-grid backward (and once its forward) and the two fit-stage scatters.  No training, no rendering, no
state produced by atomics.  Every bound is |got - ref| <= K u M (K counted from the kernel source, next to its definition in
backward_refs.py) or, for the compositor's recurrences, the plain-fp32 yardstick of `composite_bounds` (per ray and output:
a margin times the host's fp32 error in two association orders, plus a floor of a few u of the ray's magnitude);
tests/test_cpu_backward_refs.py shows on the same inputs that plain fp32 attains them.  Where the bound is zero the output
is exactly the reference's.  Each check prints the worst error / bound it saw ("RATIO ..." lines, recorded in NOTES.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_refs as br

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _ratio(got, ref, bound, what):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), (what, "non-finite output")
    err = np.abs(got - ref)
    z = bound == 0
    assert (err[z] == 0).all(), (what, "differs where the bound is zero", int((err[z] != 0).sum()), float(err[z].max()))
    r = err[~z] / bound[~z]
    worst = float(r.max()) if r.size else 0.0
    print("RATIO %-52s %.3f" % (what, worst))
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(np.where(z, 0, err / np.where(z, 1, bound)))), err.shape)
        raise AssertionError((what, "error / bound", worst, "at", i, "got", float(got[i]), "ref", float(ref[i]), "bound", float(bound[i])))
    return worst


def _lib():
    from instantavatar_amd import _lib as L
    return L


# ---- compositor ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", br.COMPOSITE_CASES, ids=lambda c: c[0])
def test_composite_train_forward_and_backward(case):
    name, n_init, with_noise, with_bg, grads = case
    L = _lib()
    inp = br.composite_inputs(n_init, with_noise, with_bg, grads)
    R, B, ray_of, _, _ = br.composite_bounds(inp)
    n, ms, S, nc = inp["n_rays"], inp["max_samples"], len(inp["pt_off"]), inp["cand_cap"]
    d = {k: _dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=DEV)
    color, depth, alpha, wd = z(n, 3) + 9, z(n) + 9, z(n) + 9, z(n, ms)
    s_arg, s_sigma, s_alpha, s_T = z(S, dt=torch.int32) + 12345, z(S) + 9, z(S) + 9, z(S) + 9
    L.check(L.lib().ia_composite_train_fwd(L.ptr(d["cand_rgb"]), L.ptr(d["cand_sigma"]), nc, L.ptr(d["pt_off"]), L.ptr(d["pt_cnt"]), n_init,
                                           L.ptr(d["ray_off"]), L.ptr(d["ray_cnt"]), L.ptr(d["s_z"]), L.ptr(d["nears"]), L.ptr(d["fars"]), n, ms,
                                           L.ptr(d.get("noise")), float(inp["noise_scale"]), L.ptr(d.get("bg")), L.ptr(color), L.ptr(depth),
                                           L.ptr(alpha), L.ptr(wd), L.ptr(d["s_slot"]), L.ptr(s_arg), L.ptr(s_sigma), L.ptr(s_alpha),
                                           L.ptr(s_T), L.stream()), "ia_composite_train_fwd")
    d_rgb, d_sig = z(nc, 3), z(nc)
    L.check(L.lib().ia_composite_train_bwd(L.ptr(d.get("d_color")), L.ptr(d.get("d_depth")), L.ptr(d.get("d_alpha")), L.ptr(d.get("d_weights")),
                                           L.ptr(d["cand_rgb"]), L.ptr(d["ray_off"]), L.ptr(d["ray_cnt"]), L.ptr(d["s_z"]), L.ptr(d["nears"]),
                                           L.ptr(d["fars"]), n, ms, L.ptr(d.get("bg")), L.ptr(d["s_slot"]), L.ptr(s_arg), L.ptr(s_sigma),
                                           L.ptr(s_alpha), L.ptr(s_T), L.ptr(d_rgb), L.ptr(d_sig), L.stream()), "ia_composite_train_bwd")
    torch.cuda.synchronize()
    assert np.array_equal(_np(s_arg), R["s_arg"]), "saved winners differ"
    got = dict(color=color, depth=depth, alpha=alpha, weights_dense=wd, s_sigma=s_sigma, s_alpha=s_alpha, s_T=s_T,
               d_cand_rgb=d_rgb, d_cand_sigma=d_sig)
    for k, v in got.items():
        # per ray and output: MARGIN x the worst plain-fp32 error of that ray + FLOOR u x the ray's magnitude (backward_refs.py);
        # a candidate that won no sample has bound 0
        bound = np.where(ray_of[k] >= 0, B[k][np.maximum(ray_of[k], 0)], 0.0)
        _ratio(_np(v), R[k], bound, "composite %s %s" % (name, k))
    # candidates that are no sample's winner keep the caller's zero (their bound is zero above; said once more in the open)
    won = np.zeros(nc, bool)
    won[R["s_arg"][R["s_arg"] >= 0]] = True
    assert (~won).sum() > 100 and (_np(d_sig)[~won] == 0).all() and (_np(d_rgb)[~won] == 0).all()
    # the relu: no gradient at sigma <= 0 (exact zeros included)
    s_of = np.full(nc, np.nan)
    s_of[R["s_arg"][R["s_arg"] >= 0]] = R["s_sigma"][R["s_arg"] >= 0]
    assert (s_of == 0).any() and (_np(d_sig)[s_of <= 0] == 0).all()


# ---- candidate selection ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_init", [1, 9])
def test_candidate_argmax_and_gather(n_init):
    L = _lib()
    inp = br.candidate_inputs(n_init)
    P, nc = len(inp["pt_off"]), inp["cand_cap"]
    d = {k: _dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    arg = torch.full((P,), 777, dtype=torch.int32, device=DEV)
    L.check(L.lib().ia_candidate_argmax(L.ptr(d["cand_sigma"]), nc, L.ptr(d["pt_off"]), L.ptr(d["pt_cnt"]), P, n_init, L.ptr(arg), L.stream()),
            "ia_candidate_argmax")
    a_ref, _ = br.candidate_argmax_ref(inp["cand_sigma"], nc, inp["pt_off"], inp["pt_cnt"], n_init)
    assert np.array_equal(_np(arg), a_ref)
    assert (a_ref < 0).sum() > 50 and (a_ref >= 0).sum() > 1000
    rgb, sigma = torch.full((P, 3), 9.0, device=DEV), torch.full((P,), 9.0, device=DEV)
    L.check(L.lib().ia_candidate_gather_fwd(L.ptr(d["cand_rgb"]), L.ptr(d["cand_sigma"]), L.ptr(arg), P, -1e5, L.ptr(rgb), L.ptr(sigma),
                                            L.stream()), "ia_candidate_gather_fwd")
    r_ref, s_ref = br.candidate_gather_ref(inp["cand_rgb"], inp["cand_sigma"], a_ref, -1e5)
    assert np.array_equal(_np(rgb).view(np.uint32), r_ref.view(np.uint32)) and np.array_equal(_np(sigma).view(np.uint32), s_ref.view(np.uint32))
    for use_rgb, use_sigma in ((True, True), (False, True), (True, False)):
        d_cr, d_cs = torch.zeros((nc, 3), device=DEV), torch.zeros(nc, device=DEV)
        L.check(L.lib().ia_candidate_gather_bwd(L.ptr(d["d_rgb"]) if use_rgb else None, L.ptr(d["d_sigma"]) if use_sigma else None, L.ptr(arg), P,
                                                L.ptr(d_cr), L.ptr(d_cs), L.stream()), "ia_candidate_gather_bwd")
        r_b, s_b = br.candidate_gather_bwd_ref(inp["d_rgb"] if use_rgb else None, inp["d_sigma"] if use_sigma else None, a_ref, nc)
        assert np.array_equal(_np(d_cr).view(np.uint32), r_b.view(np.uint32)) and np.array_equal(_np(d_cs).view(np.uint32), s_b.view(np.uint32))


# ---- hash grid -------------------------------------------------------------------------------------------------------
def _field(n_levels, inp):
    """a field descriptor over a host-built table (the MLP weights are not read by the encoding kernels)"""
    L = _lib()
    hd = L.make_hash_desc(n_levels)
    lv = br.Levels(hd.scale[:n_levels], hd.res[:n_levels], hd.offset[:n_levels + 1])
    return hd, lv


def _field_desc(hd, inp, keep):
    L = _lib()
    f = L.Field()
    f.center[:], f.scale[:] = [float(v) for v in inp["center"]], [float(v) for v in inp["fscale"]]
    f.hash = hd
    table = _dev(inp["table"].view(np.int16))
    dummy = torch.zeros(64 * 64, dtype=torch.float16, device=DEV)
    keep += [table, dummy]
    f.table = table.data_ptr()
    f.sig_w1 = f.sig_w2 = f.col_w1 = f.col_w2 = f.col_w3 = dummy.data_ptr()
    f.mlp_frags, f.enc_ws, f.enc_ws_samples, f.enc_split = None, None, 0, 0
    return f


def _hashgrid_bwd(fd, lv, x, dfeat, n_dev, want_dx, levels=None, dtable=None):
    L = _lib()
    V = x.shape[0]
    dtable = torch.zeros((lv.n_entries, 2), device=DEV) if dtable is None else dtable
    dx = torch.full((V, 3), 7.0, device=DEV) if want_dx else None
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    if levels is None:
        L.check(L.lib().ia_hashgrid_bwd(L.ptr(x), V, L.ptr(nd), C.byref(fd), L.ptr(dfeat), L.ptr(dtable), L.ptr(dx), L.stream()), "ia_hashgrid_bwd")
    else:
        L.check(L.lib().ia_hashgrid_bwd_levels(L.ptr(x), V, L.ptr(nd), C.byref(fd), L.ptr(dfeat), L.ptr(dtable), levels[0], levels[1], L.stream()),
                "ia_hashgrid_bwd_levels")
    torch.cuda.synchronize()
    return dtable, dx


@pytest.mark.parametrize("n_levels,V", br.HASH_CASES)
def test_hashgrid_backward_on_the_lattice(n_levels, V):
    """centre 0, scale 1, coordinates on the 2^-12 lattice: the reference forms bit for bit the `pos` of the kernel"""
    keep = []
    hd, lv = _field(n_levels, None)
    inp = br.hashgrid_lattice_inputs(lv, V)
    fd = _field_desc(hd, inp, keep)
    x, dfeat = _dev(inp["x"]), _dev(inp["dfeat"])
    n_dev = V if V < 257 else V - 29                 # rows past *n_dev: no contribution, dx untouched
    ref = br.hashgrid_bwd_ref(inp["x"], n_dev, inp["center"], inp["fscale"], lv, inp["dfeat"], table=inp["table"])
    what = "hashgrid L%d V%d " % (n_levels, V)
    for want_dx in (True, False):
        dtable, dx = _hashgrid_bwd(fd, lv, x, dfeat, None if n_dev == V else n_dev, want_dx)
        _ratio(_np(dtable), ref["dtable"], br.bound_table(ref), what + ("dtable" if want_dx else "dtable (no dx)"))
        if want_dx:
            dx = _np(dx)
            assert (dx[n_dev:] == 7.0).all(), "rows past *n_dev were written"
            _ratio(dx[:n_dev], ref["dx"][:n_dev], br.bound_dx(ref, n_levels)[:n_dev], what + "dx")
            raw = br.normalise32(inp["x"][:n_dev], inp["center"], inp["fscale"])[0]
            outside = (raw <= 0) | (raw >= 1)
            assert (dx[:n_dev][outside] == 0).all() and (V < 60 or outside.any())
    # three level ranges add up to the full table
    parts = torch.zeros((lv.n_entries, 2), device=DEV)
    cuts = (0, n_levels // 3, n_levels - 3, n_levels)
    for a, b in ((cuts[1], cuts[2]), (cuts[2], cuts[3]), (cuts[0], cuts[1])):
        _hashgrid_bwd(fd, lv, x, dfeat, None if n_dev == V else n_dev, False, levels=(a, b), dtable=parts)
    _ratio(_np(parts), ref["dtable"], br.bound_table(ref), what + "dtable by level ranges")
    if V == 6000:
        # the forward once: float64 interpolation at the reference's indices against the kernel that is pinned bit for bit
        # to the oracle -- ties the reference's indexing to it
        L = _lib()
        feat = torch.zeros((V, 2 * n_levels), dtype=torch.float16, device=DEV)
        L.check(L.lib().ia_hashgrid_fwd(L.ptr(x), V, C.byref(fd), L.ptr(feat), L.stream()), "ia_hashgrid_fwd")
        torch.cuda.synchronize()
        f64, mag = br.hashgrid_fwd_ref(inp["x"], inp["center"], inp["fscale"], lv, inp["table"])
        _ratio(_np(feat.float()), f64, br.bound_feat(mag), what + "forward features")


@pytest.mark.parametrize("n_levels", [8, 16])
def test_hashgrid_input_gradient_with_a_real_centre_and_scale(n_levels):
    """dx with a non-dyadic centre / scale, per point; a row within 2 ulp of a cell face may be left out (the input set is
    drawn away from them: at most 1 in 10^4, checked on the CPU)"""
    keep = []
    hd, lv = _field(n_levels, None)
    inp = br.hashgrid_real_inputs(lv)
    fd = _field_desc(hd, inp, keep)
    bad = br.near_cell_face(inp["x"], inp["center"], inp["fscale"], lv)
    assert bad.sum() <= 1e-4 * len(bad)
    ref = br.hashgrid_bwd_ref(inp["x"], None, inp["center"], inp["fscale"], lv, inp["dfeat"], table=inp["table"])
    _, dx = _hashgrid_bwd(fd, lv, _dev(inp["x"]), _dev(inp["dfeat"]), None, True)
    _ratio(_np(dx)[~bad], ref["dx"][~bad], br.bound_dx(ref, n_levels)[~bad], "hashgrid L%d real centre/scale dx" % n_levels)


# ---- fit-stage scatters ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("over_cap", [False, True], ids=["n_cand_below_cap", "n_cand_above_cap"])
def test_smpl_nn_compact_backward(over_cap):
    L = _lib()
    inp = br.smpl_nn_inputs(over_cap)
    ref = br.smpl_nn_compact_bwd_ref(**inp)
    d = {k: _dev(v) for k, v in inp.items() if isinstance(v, np.ndarray)}
    P, V = len(inp["pts"]), len(inp["T_inv"])
    n_cand = torch.tensor([inp["n_cand"]], dtype=torch.int32, device=DEV)
    for want_T, want_pts in ((True, True), (True, False), (False, True)):
        d_T = torch.full((V, 4, 4), 5.0, device=DEV) if want_T else None      # (zero-filled by the call)
        d_pts = torch.full((P, 3), 5.0, device=DEV) if want_pts else None
        L.check(L.lib().ia_smpl_nn_compact_bwd(L.ptr(d["pts"]), P, L.ptr(d["cand_pt"]), L.ptr(d["idx"]), L.ptr(n_cand), inp["cap"], L.ptr(d["T_inv"]),
                                               V, L.ptr(d["d_cand_xc"]), L.ptr(d_T), L.ptr(d_pts), L.stream()), "ia_smpl_nn_compact_bwd")
        torch.cuda.synchronize()
        tag = "smpl_nn %s T=%d pts=%d " % ("over" if over_cap else "under", want_T, want_pts)
        if want_T:
            _ratio(_np(d_T), ref["d_T_inv"], br.bound_T_inv(ref), tag + "d_T_inv")
        if want_pts:
            _ratio(_np(d_pts), ref["d_pts"], br.bound_pts(ref), tag + "d_pts")


def test_ray_samples_backward():
    L = _lib()
    inp = br.ray_samples_inputs()
    ref = br.ray_samples_bwd_ref(**inp)
    d = {k: _dev(v) for k, v in inp.items()}
    n = len(inp["ray_cnt"])
    d_o, d_d = torch.full((n, 3), 5.0, device=DEV), torch.full((n, 3), 5.0, device=DEV)
    L.check(L.lib().ia_ray_samples_bwd(L.ptr(d["ray_off"]), L.ptr(d["ray_cnt"]), L.ptr(d["s_z"]), L.ptr(d["d_pts"]), n, L.ptr(d_o), L.ptr(d_d),
                                       L.stream()), "ia_ray_samples_bwd")
    torch.cuda.synchronize()
    b_o, b_d = br.bound_rays(ref, inp["ray_cnt"])
    _ratio(_np(d_o), ref["d_o"], b_o, "ray_samples d_o")
    _ratio(_np(d_d), ref["d_d"], b_d, "ray_samples d_d")
