"""The deformer precompute and gradient entries of csrc/ia_snarf.hip, each called alone through the C ABI (`_lib.call`, plain
device tensors, the SnarfGrid struct) on the seeded input sets of tests/deformer_refs.py and compared element by element with
its float64 restatements: ia_precompute / ia_precompute_ws (k_precompute<4,true|false>, k_bbox_init, k_bbox_reduce),
ia_snarf_implicit_bwd / ia_snarf_implicit_bwd_compact (k_implicit_bwd<CL,0>, k_implicit_bwd_reduce), ia_snarf_inverse_skinning /
ia_snarf_inverse_skinning_bwd (k_inverse_skinning<CL>, k_implicit_bwd<CL,1>) and ia_expand_candidate_points.  No deformer
object, no autograd, no state the product builds.  Every bound is |got - ref| <= K u M + A, derived in deformer_refs.py;
tests/test_cpu_deformer_refs.py shows on the CPU that the references are right, that plain fp32 stays inside the bounds in two
association orders and that eleven seeded defects do not.  Nothing is excluded: every element of every output is compared;
where the bound is zero (row 3 of d_tfs, entries that are not live) the output equals the reference exactly.  Every output
buffer carries a sentinel row behind its last row and every workspace a sentinel tail, and a repeated call must give the same
bits.  Each comparison prints one "RATIO <what> <worst error / bound>" line (recorded in NOTES.md).

Which variant a precompute grid reaches follows from the host rule of ia_precompute_ws (deformer_refs.precompute_variant,
asserted on the CPU), not from device state.  NOT covered: the second grid-stride trip of k_precompute, which needs more than
8192 x 256 x 4 voxels (about 800 MB of weights)."""
import numpy as np
import pytest
import torch

import deformer_refs as dr

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
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ratio(got, ref, bound, what):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), (what, "non-finite output", int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    z = bound == 0
    assert (err[z] == 0).all(), (what, "differs where the bound is zero", int((err[z] != 0).sum()), float(err[z].max()))
    r = err[~z] / bound[~z]
    worst = float(r.max()) if r.size else 0.0
    print("RATIO %-64s %.4f" % (what, worst))
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(np.where(z, 0, err / np.where(z, 1, bound)))), err.shape)
        raise AssertionError((what, "error / bound", worst, "at", i, "got", float(got[i]), "ref", float(ref[i]), "bound", float(bound[i])))
    return worst


def _out(rows, *shape, fill=None):
    """an output buffer of `rows` rows and one more behind them that holds the sentinel"""
    t = torch.full((rows + 1,) + shape, SENTINEL, device=DEV)
    if fill is not None:
        t[:rows] = _dev(fill)
    return t


def _take(t, rows, what):
    a = _np(t)
    assert (a[rows:] == SENTINEL).all(), what + ": written behind its last row"
    return a[:rows]


def _ws(nbytes):
    """NaN bits throughout, WS_TAIL bytes more than required"""
    return torch.full((int(nbytes) + WS_TAIL,), 255, dtype=torch.uint8, device=DEV)


def _ws_intact(ws, what):
    assert (_np(ws[-WS_TAIL:]) == 255).all(), what + ": wrote behind the workspace"


def _grid(g):
    s = _lib().SnarfGrid()
    s.D, s.H, s.W = g.D, g.H, g.W
    s.offset[:], s.scale[:] = [float(v) for v in g.offset], [float(v) for v in g.scale]
    return s


# ---- a3: precompute --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,variant", dr.PRECOMPUTE_GRIDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_precompute(dims, variant):
    L = _lib()
    grid = dr.make_grid(*dims)
    cm, _ = dr.make_volume(grid)
    tfs = dr.make_tfs()
    ref = dr.precompute_ref(cm, tfs, grid)
    gs, n = _grid(grid), grid.n
    vol, t = _dev(cm), _dev(tfs)
    need = int(L.call("ia_precompute_workspace_bytes", gs))
    assert need == dr.precompute_variant(*dims)[1] * 24

    def run(form):
        J = _out(n, 12)
        d = None if form == "no_d" else _out(3 * n)
        box = None if form == "no_box" else _out(6)
        if form == "atomics" or form == "no_box":
            L.call("ia_precompute", vol, t, J, d, box, gs)
        else:
            ws = _ws(need)
            L.call("ia_precompute_ws", vol, t, J, d, box, gs, ws, need)
        torch.cuda.synchronize()
        if form not in ("atomics", "no_box"):
            _ws_intact(ws, "precompute " + form)
        what = "precompute %s %s " % (dims, form)
        return dict(J=_take(J, n, what + "voxel_J").reshape(dims + (12,)), d=None if d is None else _take(d, 3 * n, what + "voxel_d").reshape((3,) + dims),
                    box=None if box is None else _take(box, 6, what + "bbox"))

    got = {f: run(f) for f in ("atomics", "ws", "no_d", "no_box")}
    a = got["atomics"]
    tag = "precompute %dx%dx%d %s " % (dims + (variant,))
    _ratio(a["J"], ref["voxel_J"], ref["b_J"], tag + "voxel_J")
    _ratio(a["d"], ref["voxel_d"], ref["b_d"], tag + "voxel_d")
    _ratio(a["box"], ref["bbox"], ref["b_box"], tag + "bbox")
    # a min / max, not a sum: exactly the extrema of the kernel's own voxel_d
    own = np.concatenate([a["d"].reshape(3, -1).min(1), a["d"].reshape(3, -1).max(1)])
    assert _same(a["box"], own), (a["box"], own)
    for f in ("ws", "no_d", "no_box"):
        assert _same(got[f]["J"], a["J"]), f
        assert got[f]["d"] is None or _same(got[f]["d"], a["d"]), f
        assert got[f]["box"] is None or _same(got[f]["box"], a["box"]), (f, got[f]["box"], a["box"])
    again = run("ws")
    assert _same(again["J"], a["J"]) and _same(again["d"], a["d"]) and _same(again["box"], a["box"]), "a repeated call differs"


# ---- a7: the sampling kernels ----------------------------------------------------------------------------------------
class _Case:
    """device copies of one input set of deformer_refs.sampling_inputs"""

    def __init__(self, dims, n, layout, rule="default", n_init=13):
        self.inp = i = dr.sampling_inputs(dims, n, layout, n_init, rule)
        self.n, self.tag = n, "%s n=%d%s" % (layout, n, "" if rule == "default" else " " + rule)
        self.grid = _grid(i["grid"])
        self.vol = {0: _dev(i["cm"]), 1: _dev(i["cl"])}
        self.d = {k: _dev(i[k]) for k in ("xc", "J_inv", "grad", "valid", "xd", "tfs", "cand_pt")}
        self.n_dev = None if i["n_cand"] is None else torch.tensor([i["n_cand"]], dtype=torch.int32, device=DEV)
        self.need = int(_lib().call("ia_snarf_implicit_bwd_workspace_bytes", n))
        assert self.need == dr.implicit_blocks(n) * 288 * 4

    def implicit(self, cl, dense_entry):
        L, d = _lib(), self.d
        d_tfs, ws = _out(24, 4, 4, fill=self.inp["prefill"]), _ws(self.need)
        if dense_entry:
            L.call("ia_snarf_implicit_bwd", d["xc"], d["J_inv"], d["valid"], d["grad"], self.n, self.vol[0], self.grid, d_tfs, ws, self.need)
        else:
            L.call("ia_snarf_implicit_bwd_compact", d["xc"], d["J_inv"], d["grad"], self.n, self.n_dev, self.vol[cl], cl, self.grid, d_tfs, ws, self.need)
        torch.cuda.synchronize()
        _ws_intact(ws, "implicit " + self.tag)
        return _take(d_tfs, 24, "implicit d_tfs " + self.tag)

    def inverse(self, cl):
        L, d, i = _lib(), self.d, self.inp
        out = _out(self.n, 3)
        L.call("ia_snarf_inverse_skinning", d["xc"], d["xd"], d["cand_pt"], i["n_init"], d["valid"], self.n, self.n_dev, self.vol[cl], cl, self.grid,
               d["tfs"], out)
        torch.cuda.synchronize()
        return _take(out, self.n, "inverse skinning out " + self.tag)

    def inverse_bwd(self, cl, want_dxd):
        L, d, i = _lib(), self.d, self.inp
        d_tfs, ws = _out(24, 4, 4, fill=i["prefill"]), _ws(self.need)
        d_xd = _out(self.n, 3) if want_dxd else None
        L.call("ia_snarf_inverse_skinning_bwd", d["xc"], d["xd"], d["cand_pt"], i["n_init"], d["valid"], d["grad"], self.n, self.n_dev, self.vol[cl], cl,
               self.grid, d["tfs"], d_tfs, d_xd, ws, self.need)
        torch.cuda.synchronize()
        _ws_intact(ws, "inverse skinning bwd " + self.tag)
        return _take(d_tfs, 24, "inverse skinning d_tfs " + self.tag), (_take(d_xd, self.n, "d_xd_entry " + self.tag) if want_dxd else None)


def _check_row3(got, inp, what):
    assert _same(got[:, 3], inp["prefill"][:, 3]), what + ": row 3 of d_tfs lost its pre-fill"


def _implicit_ref(inp, cl):
    return dr.implicit_bwd_ref(inp["xc"], inp["J_inv"], inp["live"], inp["grad"], inp["cl" if cl else "cm"], inp["grid"], inp["prefill"])


def _inverse_ref(inp, cl):
    return dr.inverse_skinning_ref(inp["xc"], inp["xd"], inp["pt"], inp["live"], inp["cl" if cl else "cm"], inp["grid"], inp["tfs"], inp["grad"],
                                   inp["prefill"])


DIMS = {1: dr.SAMPLE_VOLUMES[0], 255: dr.SAMPLE_VOLUMES[1], 257: dr.SAMPLE_VOLUMES[0], 785: dr.SAMPLE_VOLUMES[1]}


@pytest.mark.parametrize("n", dr.ENTRY_COUNTS)
def test_implicit_bwd_dense(n):
    """ia_snarf_implicit_bwd: validity mask, channel-major weights; d_tfs is accumulated onto its pre-fill"""
    c = _Case(DIMS[n], n, "dense")
    ref = _implicit_ref(c.inp, 0)
    got = c.implicit(0, True)
    _ratio(got, ref["d_tfs"], dr.bound_implicit(ref, n), "implicit_bwd dense n=%d d_tfs" % n)
    _check_row3(got, c.inp, "implicit_bwd dense")
    assert _same(c.implicit(0, True), got), "a repeated call differs"


@pytest.mark.parametrize("n,rule", [(m, "default") for m in dr.ENTRY_COUNTS] + [(257, "over"), (257, "zero")])
def test_implicit_bwd_compact(n, rule):
    """ia_snarf_implicit_bwd_compact in both weight layouts: *n_cand below, above and at zero against cap"""
    c = _Case(DIMS[n] if rule != "zero" else dr.SAMPLE_VOLUMES[1], n, "compact", rule)
    for cl in (0, 1):
        ref = _implicit_ref(c.inp, cl)
        got = c.implicit(cl, False)
        _ratio(got, ref["d_tfs"], dr.bound_implicit(ref, n), "implicit_bwd compact n=%d %s %s d_tfs" % (n, rule, "channel-last" if cl else "channel-major"))
        _check_row3(got, c.inp, "implicit_bwd compact")
        assert _same(c.implicit(cl, False), got), "a repeated call differs"
        if rule == "zero":
            assert _same(got, c.inp["prefill"])


def test_implicit_bwd_compact_second_trip():
    """262 444 candidates, channel-last: two workgroups take a second trip through the LDS tile"""
    n = dr.BIG_N
    c = _Case(dr.SAMPLE_VOLUMES[1], n, "compact", "nearly_all")
    assert c.inp["n_cand"] > dr.MAX_BLOCKS * dr.TILE + dr.TILE
    ref = _implicit_ref(c.inp, 1)
    got = c.implicit(1, False)
    _ratio(got, ref["d_tfs"], dr.bound_implicit(ref, n), "implicit_bwd compact n=%d channel-last d_tfs" % n)
    _check_row3(got, c.inp, "implicit_bwd compact large")
    assert _same(c.implicit(1, False), got), "a repeated call differs"


def _check_inverse(c, cl, n, tag):
    ref = _inverse_ref(c.inp, cl)
    live = c.inp["live"]
    out = c.inverse(cl)
    _ratio(out, ref["out"], ref["b_out"], "inverse_skinning %s out" % tag)
    assert (out[~live] == 0).all()
    d_tfs, d_xd = c.inverse_bwd(cl, True)
    _ratio(d_tfs, ref["d_tfs"], dr.bound_inverse_bwd(ref, n), "inverse_skinning_bwd %s d_tfs" % tag)
    _ratio(d_xd, ref["d_xd"], ref["b_d_xd"], "inverse_skinning_bwd %s d_xd_entry" % tag)
    assert (d_xd[~live] == 0).all()
    _check_row3(d_tfs, c.inp, "inverse_skinning_bwd " + tag)
    plain, none = c.inverse_bwd(cl, False)
    assert none is None and _same(plain, d_tfs), "d_tfs depends on whether d_xd_entry is asked for"
    return out, d_tfs


@pytest.mark.parametrize("n,n_init", [(1, 1), (255, 13), (257, 1), (785, 13)])
def test_inverse_skinning_dense(n, n_init):
    """version 2 in the dense [P, n_init] layout, both weight layouts, d_xd_entry given and NULL"""
    c = _Case(DIMS[n], n, "dense", n_init=n_init)
    for cl in (0, 1):
        _check_inverse(c, cl, n, "dense n=%d n_init=%d %s" % (n, n_init, "channel-last" if cl else "channel-major"))


@pytest.mark.parametrize("n,rule", [(m, "default") for m in dr.ENTRY_COUNTS] + [(257, "over"), (257, "zero")])
def test_inverse_skinning_compact(n, rule):
    """version 2 over compact candidate lists: cand_pt written by ia_expand_candidate_points itself, then given directly"""
    L = _lib()
    c = _Case(DIMS[n] if rule != "zero" else dr.SAMPLE_VOLUMES[1], n, "compact", rule)
    i = c.inp
    direct = c.d["cand_pt"]
    made = torch.full((n + 8,), -7, dtype=torch.int32, device=DEV)
    L.call("ia_expand_candidate_points", _dev(i["pt_off"]), _dev(i["pt_cnt"]), i["P"], None, made, n)
    torch.cuda.synchronize()
    assert np.array_equal(_np(made)[:n], i["cand_pt"]) and (_np(made)[n:] == -7).all()
    results = []
    for src in (made[:n].clone(), direct):
        c.d["cand_pt"] = src
        for cl in (0, 1):
            results.append(_check_inverse(c, cl, n, "compact n=%d %s %s" % (n, rule, "channel-last" if cl else "channel-major")))
    for (o_a, t_a), (o_b, t_b) in zip(results[:2], results[2:]):
        assert _same(o_a, o_b) and _same(t_a, t_b), "the two sources of cand_pt differ"
    if rule == "zero":
        assert _same(results[0][1], i["prefill"]) and (results[0][0] == 0).all()


def test_inverse_skinning_bwd_second_trip():
    """262 444 entries of the dense layout (n_init = 13): the second trip of k_implicit_bwd<CL,1>, d_xd_entry given"""
    n = dr.BIG_N
    c = _Case(dr.SAMPLE_VOLUMES[0], n, "dense", "nearly_all")
    ref = _inverse_ref(c.inp, 1)
    d_tfs, d_xd = c.inverse_bwd(1, True)
    _ratio(d_tfs, ref["d_tfs"], dr.bound_inverse_bwd(ref, n), "inverse_skinning_bwd dense n=%d channel-last d_tfs" % n)
    _ratio(d_xd, ref["d_xd"], ref["b_d_xd"], "inverse_skinning_bwd dense n=%d channel-last d_xd_entry" % n)
    _check_row3(d_tfs, c.inp, "inverse_skinning_bwd large")
    again, _ = c.inverse_bwd(1, True)
    assert _same(again, d_tfs), "a repeated call differs"


# ---- candidate -> sample point ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 255, 257])
def test_expand_candidate_points(P):
    L = _lib()
    e = dr.expand_inputs(P)
    off, cnt = _dev(e["pt_off"]), _dev(e["pt_cnt"])
    for n_pts, cap in ((None, e["total"]), (e["n_pts"], e["cap"]), (None, e["cap"]), (e["n_pts"], e["total"])):
        buf = torch.full((e["total"] + 8,), -7, dtype=torch.int32, device=DEV)
        nd = None if n_pts is None else torch.tensor([n_pts], dtype=torch.int32, device=DEV)
        L.call("ia_expand_candidate_points", off, cnt, P, nd, buf, cap)
        torch.cuda.synchronize()
        want = dr.expand_candidate_points_ref(e["pt_off"], e["pt_cnt"], P, n_pts, cap, np.full(e["total"] + 8, -7, np.int32))
        assert np.array_equal(_np(buf), want), (P, n_pts, cap)
        assert (want[e["total"]:] == -7).all() and (want[:min(cap, e["total"])] >= 0).sum() > 0
