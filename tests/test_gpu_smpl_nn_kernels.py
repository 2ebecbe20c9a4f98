"""The forward entries of csrc/ia_smpl_nn.hip, each called alone through the C ABI on the seeded bodies and point sets of
tests/smpl_nn_refs.py, on buffers prefilled with a sentinel, on the library's stream: `ia_smpl_nn_deform` (k_smpl_nn),
`ia_smpl_nn_compact` on the brute-force route and on the grid route (k_smpl_nn_grid on a grid of `ia_smpl_nn_grid_build`),
and `ia_smpl_deform_query` on both routes.  No deformer object, no autograd, no state the product builds.

Index, validity, canonical point and the compact lists are compared BIT FOR BIT with the exact layer of smpl_nn_refs (NaN as
NaN), for every live point, invalid ones included; the float64 comparator then runs on the kernel's own outputs and prints
"RATIO ..." lines (recorded in NOTES.md).  tests/test_cpu_smpl_nn_refs.py shows on the CPU that the exact layer equals the
oracle's loop, satisfies the float64 layer and that the seeded defects do not pass.  No point is excluded from any comparison.
The grid is a black box: no test interprets the buffer (a refused build is only checked to have left its prefill).
The body `margin` is the directed case for the cell width of ia_smpl_nn_grid_build: a vertex whose cell coordinate rounds up
across a cell boundary, with valid points pred(thr) and further below it; cells exactly `thr` wide would lose them.

The fused query is expected to equal, bit for bit, the pinned pieces it fuses: the reference's compact canonical list through
`ia_field_fwd`, then render_iter_refs.candidate_max with n_init = 1; (0, fill) on invalid points."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_refs as mr
import render_iter_refs as rr
import smpl_nn_refs as nr
from test_gpu_mlp_kernels import _Field, _real_field

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IA_OK, IA_ERR_ARG, IA_ERR_WORKSPACE = 0, -1, -3
PAD = 3          # rows behind the last row of every output


def _lib():
    from instantavatar_amd import _lib as L
    return L


def _dev(a):
    return None if a is None else torch.as_tensor(np.array(a, order="C")).to(DEV)       # (a copy: the cases are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def _raw(name, *args):
    """the entry's own status (no exception on a refusal), on the library's stream"""
    L = _lib()
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else C.byref(a) if isinstance(a, C.Structure) else a for a in args]
    rc = getattr(L.lib(), name)(*conv, L.stream())
    torch.cuda.synchronize()
    return rc


def _full(rows, shape, sent, dtype):
    return torch.full((rows,) + shape, sent, dtype=dtype, device=DEV)


class _Body:
    """device copies of one case of smpl_nn_refs"""

    def __init__(self, c):
        self.c, self.V, self.thr = c, len(c["verts"]), float(c["thr"])
        self.verts, self.T_inv, self.pts = _dev(c["verts"]), _dev(c["T_inv"]), _dev(c["pts"])

    def n_dev(self, n):
        return None if n is None else torch.tensor([n], dtype=torch.int32, device=DEV)

    def deform(self, P, n_live=None, want_idx=True, verts=None, n_verts=None, cano=True, valid=True):
        rows = max(P, 0) + PAD
        out = dict(cano=_full(rows, (3,), float(nr.SENT_F), torch.float32), valid=_full(rows, (), int(nr.SENT_B), torch.uint8),
                   idx=_full(rows, (), int(nr.SENT_I), torch.int32))
        rc = _raw("ia_smpl_nn_deform", self.pts, P, self.n_dev(n_live), self.verts if verts is None else verts, self.T_inv,
                  self.V if n_verts is None else n_verts, self.thr, out["cano"] if cano else None, out["valid"] if valid else None,
                  out["idx"] if want_idx else None)
        return rc, {k: _np(v) for k, v in out.items()}

    def compact(self, P, n_live=None, grid=None, thr=None):
        rows = max(P, 0) + PAD
        out = dict(cand_xc=_full(rows, (3,), float(nr.SENT_F), torch.float32), cand_pt=_full(rows, (), int(nr.SENT_I), torch.int32),
                   idx=_full(rows, (), int(nr.SENT_I), torch.int32), pt_off=_full(rows, (), int(nr.SENT_I), torch.int32),
                   pt_cnt=_full(rows, (), int(nr.SENT_B), torch.uint8), n_cand=_full(1, (), int(nr.SENT_I), torch.int32))
        rc = _raw("ia_smpl_nn_compact", self.pts, P, self.n_dev(n_live), self.verts, self.T_inv, self.V, self.thr if thr is None else float(thr),
                  out["cand_xc"], out["cand_pt"], out["idx"], out["pt_off"], out["pt_cnt"], out["n_cand"], grid)
        out = {k: _np(v) for k, v in out.items()}
        out["n_cand"] = int(out["n_cand"][0])
        return rc, out

    def build_grid(self, buf=None, thr=None, nbytes=None):
        need = int(_lib().call("ia_smpl_nn_grid_bytes", self.V))
        if buf is None:
            buf = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
        rc = _raw("ia_smpl_nn_grid_build", self.verts, self.V, self.thr if thr is None else float(thr), buf, need if nbytes is None else nbytes)
        return rc, buf


@functools.lru_cache(maxsize=None)
def _body(name):
    return _Body(nr.staging_case(int(name[7:])) if name.startswith("staging") else nr.case(name))


def _live(P, n_live):
    return P if n_live is None else min(P, n_live)


def _check_deform(out, ref, P, live, what, idx=True):
    got = dict(idx=out["idx"][:live] if idx else ref["idx"][:live], valid=out["valid"][:live], cano=out["cano"][:live])
    exp = {k: ref[k][:live] for k in ("idx", "valid", "cano")}
    assert set(np.unique(out["valid"][:live])) <= {0, 1}
    bad = nr.agree_exact(got, exp)
    assert bad == 0, (what, "points that differ from the exact layer", bad)
    assert (out["cano"][live:] == nr.SENT_F).all() and (out["valid"][live:] == nr.SENT_B).all() and (out["idx"][live if idx else 0:] == nr.SENT_I).all(), \
        what + ": a row at or past the live count was written"


def _ratios(c, out, n, what):
    r = nr.check64(c["pts"][:n], c["verts"], c["T_inv"], c["thr"], out["idx"][:n], out["valid"][:n], out["cano"][:n])
    print("RATIO %-40s nearest %.4f  cano %.4f  validity decided on %d of %d" % (what, r["nn"], r["cano"], r["decided"], n))
    assert nr.passes64(r), (what, r)


STAGING = tuple("staging%d" % n for n in nr.STAGING_SIZES)
N_DEV_RULES = (("null", None), ("equal", 1000), ("above", 1500), ("zero", 0), ("below", 300))


# ---- ia_smpl_nn_deform -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nr.BODIES + STAGING)
def test_deform(name):
    """every body, and the staging loop at n_verts 1, 3, 5, 64, either side of 64 KB of dynamic LDS, 6 890 and the largest the
    entry accepts (156 KB): bit for bit, then the float64 comparator on the kernel's outputs; idx NULL; a repeated call"""
    b = _body(name)
    c, P = b.c, len(b.c["pts"])
    rc, out = b.deform(P)
    assert rc == IA_OK, (name, rc, _lib().lib().ia_last_error())
    _check_deform(out, c["ref"], P, P, "deform " + name)
    _ratios(c, out, P, "deform " + name)
    rc, again = b.deform(P)
    assert rc == IA_OK and all(out[k].tobytes() == again[k].tobytes() for k in out), "a repeated call differs"
    rc, no_idx = b.deform(P, want_idx=False)
    assert rc == IA_OK
    _check_deform(no_idx, c["ref"], P, P, "deform idx NULL " + name, idx=False)


@pytest.mark.parametrize("P", nr.P_PREFIXES)
def test_deform_prefixes(P):
    b = _body("lattice400")
    rc, out = b.deform(P)
    assert rc == IA_OK
    _check_deform(out, b.c["ref"], P, P, "deform P=%d" % P)


@pytest.mark.parametrize("rule,n", N_DEV_RULES)
def test_deform_device_count(rule, n):
    b, P = _body("cloud257"), 1000
    rc, out = b.deform(P, n_live=n)
    assert rc == IA_OK
    _check_deform(out, b.c["ref"], P, _live(P, n), "deform *n_pts_dev " + rule)


def test_deform_refusals():
    """13 313 vertices, n_verts 0, NULL outputs and P < 0 are refused and leave every output untouched; P = 0 is OK"""
    b, P = _body("cloud257"), 300
    big = torch.zeros((nr.MAX_VERTS + 1, 3), device=DEV)
    for what, kw in (("13313 vertices", dict(verts=big, n_verts=nr.MAX_VERTS + 1)), ("n_verts 0", dict(n_verts=0)), ("pts_cano NULL", dict(cano=False)),
                     ("valid NULL", dict(valid=False))):
        rc, out = b.deform(P, **kw)
        assert rc == IA_ERR_ARG, (what, rc)
        _check_deform(out, b.c["ref"], P, 0, what)
    rc, out = b.deform(-1)
    assert rc == IA_ERR_ARG
    _check_deform(out, b.c["ref"], 0, 0, "P < 0")
    rc, out = b.deform(0)
    assert rc == IA_OK
    _check_deform(out, b.c["ref"], 0, 0, "P = 0")


# ---- ia_smpl_nn_compact ----------------------------------------------------------------------------------------------
def _grid_for(b):
    rc, buf = b.build_grid()
    assert rc == IA_OK
    return buf


@pytest.mark.parametrize("route", ["brute", "grid"])
@pytest.mark.parametrize("name", nr.BODIES + STAGING)
def test_compact(name, route):
    b = _body(name)
    P = len(b.c["pts"])
    grid = _grid_for(b) if route == "grid" else None
    rc, out = b.compact(P, grid=grid)
    assert rc == IA_OK, (name, route, rc, _lib().lib().ia_last_error())
    nr.check_compact(out, b.c["ref"], P, route)
    assert 0 < out["n_cand"] < P
    rc, again = b.compact(P, grid=grid)
    assert rc == IA_OK
    nr.check_compact(again, b.c["ref"], P, route)
    assert all(np.array_equal(out[k], again[k]) for k in ("idx", "pt_cnt")) and out["n_cand"] == again["n_cand"]


@pytest.mark.parametrize("route", ["brute", "grid"])
def test_compact_prefixes_and_device_count(route):
    """P = 1 ... 1000 as prefixes of the interleaved point list; *n_pts_dev NULL, equal to P, above, zero and 300 of 1000;
    P = 0 leaves *n_cand == 0 and writes nothing else"""
    b = _body("doubled100")
    grid = _grid_for(b) if route == "grid" else None
    for P in nr.P_PREFIXES:
        rc, out = b.compact(P, grid=grid)
        assert rc == IA_OK
        nr.check_compact(out, b.c["ref"], P, route)
    for rule, n in N_DEV_RULES:
        rc, out = b.compact(1000, n_live=n, grid=grid)
        assert rc == IA_OK, rule
        nr.check_compact(out, b.c["ref"], _live(1000, n), route)
        if rule == "zero":
            assert out["n_cand"] == 0
    rc, out = b.compact(0, grid=grid)
    assert rc == IA_OK and out["n_cand"] == 0
    nr.check_compact(out, b.c["ref"], 0, route)


# ---- the grid route --------------------------------------------------------------------------------------------------
def test_grid_rebuilt_in_a_used_buffer():
    """the line body (64 cells along x), then the one-vertex body and the 257-vertex cloud built into the SAME buffer"""
    L = _lib()
    line = _body("line500")
    rc, buf = line.build_grid()
    assert rc == IA_OK
    for name in ("line500", "one", "cloud257", "line500"):
        b = _body(name)
        assert int(L.call("ia_smpl_nn_grid_bytes", b.V)) <= buf.numel()
        rc, _ = b.build_grid(buf=buf)
        assert rc == IA_OK
        P = len(b.c["pts"])
        rc, out = b.compact(P, grid=buf)
        assert rc == IA_OK
        nr.check_compact(out, b.c["ref"], P, "grid")


@pytest.mark.parametrize("name", ["cloud257", "lattice400", "line500", "far", "margin"])
def test_grid_serves_smaller_query_thresholds(name):
    """a grid built with threshold t, queried with t, t / 2 and t / 16"""
    b = _body(name)
    c, P = b.c, len(b.c["pts"])
    grid = _grid_for(b)
    for div in (1, 2, 16):
        t = c["thr"] / div
        ref = c["ref"] if div == 1 else nr.nn_exact(c["pts"], c["verts"], c["T_inv"], t)
        assert ref["valid"].any()
        for route, g in (("grid", grid), ("brute", None)):
            rc, out = b.compact(P, grid=g, thr=t)
            assert rc == IA_OK
            nr.check_compact(out, ref, P, route)


def test_grid_build_refusals():
    """a buffer one byte short, n_verts 0 and threshold 0 are refused; the buffer keeps its prefill"""
    b = _body("cloud257")
    need = int(_lib().call("ia_smpl_nn_grid_bytes", b.V))
    for what, kw in (("one byte short", dict(nbytes=need - 1)), ("threshold 0", dict(thr=0.0))):
        rc, buf = b.build_grid(**kw)
        assert rc == IA_ERR_ARG, (what, rc)
        assert bool((buf == 255).all()), what + ": the refused build wrote into the buffer"
    buf = torch.full((need,), 255, dtype=torch.uint8, device=DEV)
    rc = _raw("ia_smpl_nn_grid_build", b.verts, 0, b.thr, buf, need)
    assert rc == IA_ERR_ARG and bool((buf == 255).all())


# ---- ia_smpl_deform_query --------------------------------------------------------------------------------------------
def _field(enc_ws_samples=0):
    W, table = _real_field(8)
    fd = _Field(8, W, table, mr.REAL_CENTER, mr.REAL_SCALE)
    return fd.with_enc_ws(enc_ws_samples) if enc_ws_samples else fd


def _expected_query(fd, ref, n_live, fill):
    """the pinned pieces: compact canonical list of the exact layer -> ia_field_fwd -> candidate_max(n_init = 1)"""
    k = nr.compact_ref(ref, n_live)
    n = k["n_cand"]
    sig, col = np.zeros(n_live, np.float32), np.zeros((n_live, 3), np.float32)
    if n:
        rgb, sigma = torch.full((n, 3), 9.0, device=DEV), torch.full((n,), 9.0, device=DEV)
        _lib().call("ia_field_fwd", _dev(k["cand_xc"]), n, None, fd.f, rgb, sigma)
        torch.cuda.synchronize()
        rgb, sigma = _np(rgb), _np(sigma)
        assert np.isfinite(rgb).all() and np.isfinite(sigma).all()
        sig, col = rr.candidate_max(k["pt_off"], k["pt_cnt"], sigma, rgb, 1, dtype=np.float32)
    v = ref["valid"][:n_live]
    return np.where(v, sig, np.float32(fill)).astype(np.float32), np.where(v[:, None], col, np.float32(0)).astype(np.float32)


def _query(b, fd, P, n_live, fill, nan_to_num, grid, want_rgb=True, ws_short=0):
    need = int(_lib().call("ia_smpl_query_workspace_bytes", P))
    ws = torch.full((need + 64,), 255, dtype=torch.uint8, device=DEV)
    rows = P + PAD
    rgb, sigma = _full(rows, (3,), float(nr.SENT_F), torch.float32), _full(rows, (), float(nr.SENT_F), torch.float32)
    rc = _raw("ia_smpl_deform_query", b.pts, P, b.n_dev(n_live), b.verts, b.T_inv, b.V, b.thr, fd.f, float(fill), int(nan_to_num),
              rgb if want_rgb else None, sigma, ws, need - ws_short, grid)
    assert bool((ws[need:] == 255).all()), "wrote behind the workspace"
    return rc, _np(rgb), _np(sigma), ws


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("route", ["brute", "grid"])
@pytest.mark.parametrize("name", ["cloud257", "lattice400", "line500"])
def test_deform_query(name, route):
    b = _body(name)
    fd = _field()
    grid = _grid_for(b) if route == "grid" else None
    P_full = len(b.c["pts"])
    for fill, nan_to_num in ((0.0, 0), (-1e5, 1)):
        for P, n in ((P_full, None), (1000, 1000), (1000, 1500), (1000, 300), (1000, 0), (257, None), (1, None)):
            live = _live(P, n)
            rc, rgb, sigma, _ = _query(b, fd, P, n, fill, nan_to_num, grid)
            assert rc == IA_OK
            want_s, want_c = _expected_query(fd, b.c["ref"], live, fill)
            what = "%s %s fill %g P %d n %s" % (name, route, fill, P, n)
            assert _bits_equal(sigma[:live], want_s), what + ": sigma"
            assert _bits_equal(rgb[:live], want_c), what + ": rgb"
            assert (sigma[live:] == nr.SENT_F).all() and (rgb[live:] == nr.SENT_F).all(), what + ": a row at or past the live count was written"
            inv = ~b.c["ref"]["valid"][:live]
            assert (sigma[:live][inv] == np.float32(fill)).all() and (rgb[:live][inv] == 0).all()
        # rgb NULL: the same sigma
        rc, rgb, sigma, _ = _query(b, fd, 1000, 300, fill, nan_to_num, grid, want_rgb=False)
        assert rc == IA_OK and (rgb == nr.SENT_F).all()
        assert _bits_equal(sigma[:300], _expected_query(fd, b.c["ref"], 300, fill)[0]) and (sigma[300:] == nr.SENT_F).all()
    # a workspace one byte short: the workspace error, nothing written
    rc, rgb, sigma, ws = _query(b, fd, 1000, None, 0.0, 0, grid, ws_short=1)
    assert rc == IA_ERR_WORKSPACE and (rgb == nr.SENT_F).all() and (sigma == nr.SENT_F).all() and bool((ws == 255).all())


@pytest.mark.parametrize("route", ["brute", "grid"])
def test_deform_query_sharded_encoder(route):
    """P = 9 000 with a descriptor that carries enc_ws: the valid count reaches the sharded encoder as a device count"""
    P = 9000
    b = _Body(nr.big_case("cloud257", P))
    grid = _grid_for(b) if route == "grid" else None
    plain, sharded = _field(), _field(P + 11)
    rc, rgb0, sig0, _ = _query(b, plain, P, None, 0.0, 0, grid)
    assert rc == IA_OK
    rc, rgb1, sig1, _ = _query(b, sharded, P, None, 0.0, 0, grid)
    assert rc == IA_OK
    assert _bits_equal(sig0, sig1) and _bits_equal(rgb0, rgb1), "the sharded encoding changes the result"
    want_s, want_c = _expected_query(plain, b.c["ref"], P, 0.0)
    assert _bits_equal(sig1[:P], want_s) and _bits_equal(rgb1[:P], want_c)
    assert 0.3 < b.c["ref"]["valid"].mean() < 0.95
