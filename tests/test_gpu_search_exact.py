"""k_search against the CPU oracle's search + filter, BIT FOR BIT, at the smallest shapes at which the solver loop can go
wrong (-m gpu).

Both sides get the same voxel_J (the oracle's precompute of an 8 x 16 x 16 transform grid under a bent pose of the test
world), the same transforms and the same points, so nothing but the kernel differs: every solve executes the arithmetic
sequence of the reference (fuse_cuda_kernel_fast.cu:252-413) and the oracle restates that sequence with the same fused
multiply-adds.  Checked: the dense layout (`ia_snarf_search`: xc, valid, valid_raw, J_inv), the compacted roots
(`ia_snarf_search_compact`, `_compact_jinv`: per point the candidates and their J_inv in init order; the ranges of different
points may be permuted), each once with the in-library profiling off and once on (two instantiations of the kernel), and the
solve / fetch counters of the profiling mode against the oracle's own counts.

Shapes: n_init 1 and 13; 1, 3, 63, 64, 65 and 200 points -- quads with one to three live lanes, a ragged last tile, more than
one workgroup (64 points each).  The points mix roots inside the grid, points every init of which is trivial, nodes of the
grid's six faces (the last cell of each axis: the far corners fall outside with weight 0), NaN and +-1e30 coordinates.  One
more world is the same scene scaled by 4096: Broyden steps of hundreds of units leave the exponent range of the shared
reciprocal (`div_shared_range`, ia_search_dev.h), so its waves take the compiler's divisions."""
import ctypes as C

import numpy as np
import pytest
import torch

from instantavatar_amd import _lib, synthetic as syn

import world as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_MAX = 200
SCALED = 4096.0


def _points(vd, rng):
    """P_MAX points, kinds interleaved so that every prefix (P = 1, 3, 63, ...) holds a mixture; the first one has a root."""
    D, H, Wd = vd.shape[1:]
    flat = vd.reshape(3, -1).T
    inside = flat[rng.randint(0, len(flat), P_MAX)] + (rng.randn(P_MAX, 3) * 0.01).astype(np.float32)
    faces = []
    for _ in range(P_MAX):
        z, y, x = rng.randint(0, D), rng.randint(0, H), rng.randint(0, Wd)
        ax, end = rng.randint(0, 3), rng.randint(0, 2)
        if ax == 0: x = (Wd - 1) * end
        if ax == 1: y = (H - 1) * end
        if ax == 2: z = (D - 1) * end
        faces.append(vd[:, z, y, x])
    faces = np.asarray(faces, np.float32)
    far = (rng.rand(P_MAX, 3).astype(np.float32) + 40.0) * np.where(rng.rand(P_MAX, 3) < 0.5, -1, 1).astype(np.float32)
    odd = np.array([[np.nan, 0, 0], [0, 1e30, 0], [0, 0, -1e30], [np.nan, np.nan, np.nan], [1e30, -1e30, 0.1]], np.float32)
    pts = np.empty((P_MAX, 3), np.float32)
    for i in range(P_MAX):
        kind = i % 8
        if kind in (0, 3, 5, 6): pts[i] = inside[i]
        elif kind in (2, 7): pts[i] = faces[i]
        elif kind == 1: pts[i] = far[i]
        else: pts[i] = odd[(i // 8) % len(odd)]
    return pts


def _fma32(a, b, c):
    # fmaf on float32 arrays: the product of two floats is exact in double, one rounding to double, one to float
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _queued(pts, tfs, bones, off, scl, dims):
    """which (point, init) solves k_search queues: those whose INITIAL fetch has a corner inside the grid (ia_common.h,
    ia_solve_is_trivial; the others are invalid by construction and never enter the solver loop)"""
    T = tfs[list(bones)]                                           # [n, 4, 4]
    with np.errstate(all="ignore"):
        d = pts[:, None, :] - T[None, :, :3, 3]                    # [P, n, 3]
        x0 = np.stack([_fma32(d[..., 2], T[None, :, 2, c], _fma32(d[..., 1], T[None, :, 1, c], d[..., 0] * T[None, :, 0, c]))
                       for c in range(3)], -1)
        g = scl[None, None] * (x0 + off[None, None])
        idx = ((g + np.float32(1)) / np.float32(2)) * (dims[None, None] - 1).astype(np.float32)
        idx = np.where(np.abs(idx) <= np.float32(2147483648.0), idx, np.float32(-100))
        f0 = np.floor(idx)
    return ~((f0 < -1) | (f0 >= dims[None, None])).any(-1)


@pytest.fixture(scope="module")
def cases(oracle):
    """the two worlds with their points and the oracle's results for n_init = 1 and 13 at P_MAX points (a prefix of the
    points is a prefix of the results: solves are independent), computed once"""
    body = syn.make_body()
    init32 = oracle.deformer_initialize(body, np.zeros(10, np.float32), syn.cano_pose("A_pose"), resolution=32, n_smooth=30)
    wv = np.ascontiguousarray(init32["lbs_voxel"][:, :, ::2, ::2])             # 8 x 16 x 16, still convex weights
    wv /= wv.sum(0, keepdims=True)
    poses, tr = W.poses()
    tfs, _ = oracle.prepare_deformer(body, init32, np.zeros(10, np.float32), poses[5, 3:], poses[5, :3], tr[5])
    out = {}
    for name, k in (("unit", 1.0), ("scaled", SCALED)):
        t = np.ascontiguousarray(tfs, np.float32).copy()
        t[:, :3, 3] *= np.float32(k)
        init = dict(lbs_voxel=wv, offset_kernel=(init32["offset_kernel"] * np.float32(k)).astype(np.float32),
                    scale_kernel=(init32["scale_kernel"] / np.float32(k)).astype(np.float32), D=8, H=16, W=16)
        vJ, vd = oracle.precompute(init, t)
        pts = _points(vd, np.random.RandomState(3))
        # thresholds scale with the world; the scaled one must not stop at the first divergence test, or no update runs
        cvg, dvg = (1e-5, 1e-1) if k == 1.0 else (1e-5 * k, 1e15)
        ref = {}
        for n in (1, 13):
            bones = syn.INIT_BONES[:n]
            x, Ji, raw, it = oracle.broyden(pts, vJ, t, init, bones, cvg, dvg, want_iters=True)
            keep = oracle.filter_dup(x, raw)
            q = _queued(pts, t, bones, init["offset_kernel"], init["scale_kernel"], np.array([16, 16, 8]))
            ref[n] = dict(x=x, Ji=Ji.reshape(len(pts), n, 9), raw=raw, keep=keep, it=it, queued=q)
        out[name] = dict(init=init, tfs=t, vJ_cl=np.ascontiguousarray(np.transpose(vJ, (1, 2, 3, 0))), pts=pts, ref=ref, cvg=cvg, dvg=dvg)
    return out


def test_the_points_exercise_what_they_should(cases):
    """properties of the inputs, from the oracle alone: roots, trivial points, long solves, the fallback's magnitudes"""
    u, s = cases["unit"], cases["scaled"]
    r = u["ref"][13]
    assert r["raw"][:1].any() and r["raw"].sum() > 100 and (r["keep"] != r["raw"]).any()       # roots, and duplicates to filter
    assert (~r["queued"]).all(1).sum() >= 20 and r["queued"].all(1).sum() >= 1                   # points with every init trivial
    assert (r["it"][r["queued"]] >= 4).sum() > 100 and u["ref"][1]["raw"].sum() > 10
    assert not np.isfinite(u["pts"]).all() and np.abs(u["pts"][np.isfinite(u["pts"])]).max() >= 1e30
    # scaled world: solves that run at least two updates and end more than 2^9 units from their start -- a first step of that
    # length puts c = J_inv^T u beyond the 2^8 bound of div_shared_range
    rs = s["ref"][13]
    T = s["tfs"][list(syn.INIT_BONES)]
    x0 = np.einsum("nji,pnj->pni", T[:, :3, :3], s["pts"][:, None, :] - T[None, :, :3, 3])
    with np.errstate(all="ignore"):
        moved = np.abs(rs["x"] - x0).max(-1)
    assert ((rs["it"] >= 4) & rs["raw"].astype(bool) & (moved > 512)).sum() > 20


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grid(init):
    g = _lib.SnarfGrid()
    g.D, g.H, g.W = init["D"], init["H"], init["W"]
    g.offset[:] = init["offset_kernel"].tolist()
    g.scale[:] = init["scale_kernel"].tolist()
    return g


def _run_dense(c, P, n):
    xd, vJ, tfs = _t(c["pts"][:P]), _t(c["vJ_cl"]), _t(c["tfs"])
    xc = torch.full((P, n, 3), 7.0, device=DEV); Ji = torch.full((P, n, 9), 7.0, device=DEV)
    keep = torch.full((P, n), 9, device=DEV, dtype=torch.uint8); raw = torch.full((P, n), 9, device=DEV, dtype=torch.uint8)
    _lib.call("ia_snarf_search", xd, P, vJ, tfs, _lib.bone_array(syn.INIT_BONES[:n]), n, _grid(c["init"]), c["cvg"], c["dvg"], xc, keep, raw, Ji)
    torch.cuda.synchronize()
    return xc.cpu().numpy(), keep.cpu().numpy(), raw.cpu().numpy(), Ji.cpu().numpy()


def _run_compact(c, P, n, jinv):
    xd, vJ, tfs = _t(c["pts"][:P]), _t(c["vJ_cl"]), _t(c["tfs"])
    cap = P * n
    cand = torch.full((cap, 3), 7.0, device=DEV); cJ = torch.full((cap, 9), 7.0, device=DEV)
    off = torch.full((P,), -1, device=DEV, dtype=torch.int32); cnt = torch.full((P,), 99, device=DEV, dtype=torch.uint8)
    n_cand = torch.full((1,), 123, device=DEV, dtype=torch.int32)
    head = (xd, P, None, vJ, tfs, _lib.bone_array(syn.INIT_BONES[:n]), n, _grid(c["init"]), c["cvg"], c["dvg"], cand)
    if jinv:
        nb = int(_lib.call("ia_snarf_search_jinv_workspace_bytes", P, n))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        _lib.call("ia_snarf_search_compact_jinv", *head, cJ, cap, off, cnt, n_cand, 1, ws, nb)
    else:
        _lib.call("ia_snarf_search_compact", *head, cap, off, cnt, n_cand, 1)
    torch.cuda.synchronize()
    return cand.cpu().numpy(), cJ.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy(), int(n_cand.item())


def _check_compact(got, r, P, jinv, what):
    cand, cJ, off, cnt, n_cand = got
    keep = r["keep"][:P].astype(bool)
    assert np.array_equal(cnt, keep.sum(1)), what
    assert n_cand == keep.sum(), what
    live = np.nonzero(cnt)[0]
    order = live[np.argsort(off[live], kind="stable")]
    assert len(live) == 0 or np.array_equal(off[order], np.concatenate([[0], np.cumsum(cnt[order])[:-1]]).astype(np.int64)), (what, "ranges are not a partition")
    for p in live:
        sl = slice(off[p], off[p] + cnt[p])
        assert np.array_equal(_bits(cand[sl]), _bits(r["x"][p][keep[p]])), (what, p)
        if jinv:
            assert np.array_equal(_bits(cJ[sl]), _bits(r["Ji"][p][keep[p]])), (what, p)


def _units():
    u = (C.c_uint64 * 3)()
    _lib.call("ia_profile_get_units", 0, u, 3)
    return [int(v) for v in u]


def _check_case(c, P, n):
    r = c["ref"][n]
    xc, keep, raw, Ji = _run_dense(c, P, n)
    what = "P=%d n_init=%d" % (P, n)
    assert np.array_equal(raw, r["raw"][:P]), what
    assert np.array_equal(keep, r["keep"][:P]), what
    assert np.array_equal(_bits(xc), _bits(r["x"][:P])), what
    assert np.array_equal(_bits(Ji), _bits(r["Ji"][:P])), what
    plain = [_run_compact(c, P, n, False), _run_compact(c, P, n, True)]
    _check_compact(plain[0], r, P, False, what + " compact")
    _check_compact(plain[1], r, P, True, what + " compact_jinv")
    # the counting instantiation: same outputs, and the counters of the launch are the oracle's
    q = r["queued"][:P]
    want = [int(q.sum()), int(r["it"][:P][q].sum())]
    _lib.call("ia_profile_enable", 1)
    try:
        for j, jinv in enumerate((False, True)):
            _lib.call("ia_profile_reset")
            got = _run_compact(c, P, n, jinv)
            u = _units()
            print("%s profile(jinv=%d): solves %d fetches %d loaded %d, oracle %s" % (what, jinv, u[0], u[1], u[2], want))
            assert u[:2] == want and u[2] <= u[1], (what, u, want)
            _check_compact(got, r, P, jinv, what + " profiled")
            # (offsets come from an atomic: compare what is order independent, and the payload through the offsets above)
            assert np.array_equal(got[3], plain[j][3]) and got[4] == plain[j][4]
    finally:
        _lib.call("ia_profile_reset")
        _lib.call("ia_profile_enable", 0)


@pytest.mark.parametrize("n_init", [1, 13])
@pytest.mark.parametrize("P", [1, 3, 63, 64, 65, 200])
def test_search_is_the_oracle_bit_for_bit(cases, P, n_init):
    _check_case(cases["unit"], P, n_init)


def test_search_with_the_fallback_divisions_is_the_oracle_bit_for_bit(cases):
    _check_case(cases["scaled"], P_MAX, 13)
