"""The SMPL body-model entries, each called alone through the C ABI (`_lib.call`, plain device tensors, the ia_smpl_body struct)
on the seeded cases of tests/smpl_refs.py and compared per output group with its float64 restatements: ia_smpl_lbs_fwd /
ia_smpl_lbs_bwd (the five kernels of csrc/ia_smpl_lbs.hip) and ia_smpl_tfs / ia_smpl_tfs_bwd (k_smpl_tfs, k_smpl_tfs_bwd of
csrc/ia_snarf.hip).  No SMPLDeformer, no autograd.  The bound is derived in smpl_refs.py; tests/test_cpu_smpl_refs.py shows
on the CPU that the references are right, that a second fp32 association stays inside the bound and that seven seeded defects
do not.  Every output buffer carries a sentinel row behind its last row and every workspace a sentinel tail: nothing may be
written there.  Each comparison prints one "SMPLREF ..." line per case and group: max error, allowance, error / (allow / K)
-- the figures recorded in smpl_refs.MEASURED."""
import functools

import numpy as np
import pytest
import torch

import smpl_refs as sr

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
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a if k in b)


def _out(rows, *shape):
    """an output buffer of `rows` rows and one more behind them, all holding the sentinel"""
    return torch.full((rows + 1,) + shape, SENTINEL, device=DEV)


def _take(t, rows, what):
    a = _np(t)
    assert (a[rows:] == SENTINEL).all(), what + ": written behind its last row"
    return a[:rows]


class _Case:
    """the device copies of one LBS case and its ia_smpl_body"""

    def __init__(self, name):
        L = _lib()
        self.name, self.i = name, sr.lbs_inputs(name)
        self.V = self.i["body"]["v_template"].shape[0]
        self.t = {k: _dev(self.i["body"][k]) for k in sr.BODY_KEYS}
        self.body = L.SmplBody()
        for k in sr.BODY_KEYS:
            setattr(self.body, k, self.t[k].data_ptr())
        self.body.n_verts = self.V
        self.d = {k: _dev(self.i[k]) for k in ("betas", "pose", "transl", "pose_t", "po_t", "d_T_inv", "d_w2s")}
        self.need = L.call("ia_smpl_lbs_workspace_bytes", self.V)

    def workspace(self, need=None):
        """NaN bits throughout, WS_TAIL bytes more than required"""
        return torch.full(((self.need if need is None else need) + WS_TAIL,), 255, dtype=torch.uint8, device=DEV)

    def fwd(self, ws, transl="case", verts=True, verts_t=True, w2s=True, ws_bytes=None):
        V = self.V
        o = dict(T_inv=_out(V, 4, 4), verts=_out(V, 3) if verts else None, verts_t=_out(V, 3) if verts_t else None,
                 w2s=_out(1, 4, 4) if w2s else None)
        tr = self.d["transl"] if isinstance(transl, str) else transl
        self.raw = o
        _lib().call("ia_smpl_lbs_fwd", self.body, self.d["betas"], self.d["pose"], tr, self.d["pose_t"], self.d["po_t"], o["T_inv"], o["verts"],
                    o["verts_t"], o["w2s"], ws, self.need if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        assert (_np(ws[-WS_TAIL:]) == 255).all(), "forward wrote behind the workspace"
        r = {k: _take(t, 1 if k == "w2s" else V, self.name + " " + k) for k, t in o.items() if t is not None}
        if "w2s" in r:
            r["w2s"] = r["w2s"][0]
        return r

    def bwd(self, ws, d_w2s=True, d_betas=True, d_transl=True, d_pose=True, ws_bytes=None):
        o = dict(d_betas=_out(10) if d_betas else None, d_pose=_out(72) if d_pose else None, d_transl=_out(3) if d_transl else None)
        self.raw = o
        _lib().call("ia_smpl_lbs_bwd", self.body, self.d["betas"], self.d["pose"], self.d["transl"], self.d["pose_t"], self.d["po_t"],
                    self.d["d_T_inv"], self.d["d_w2s"] if d_w2s else None, o["d_betas"], o["d_pose"], o["d_transl"], ws,
                    self.need if ws_bytes is None else ws_bytes)
        torch.cuda.synchronize()
        assert (_np(ws[-WS_TAIL:]) == 255).all(), "backward wrote behind the workspace"
        return {k: _take(t, {"d_betas": 10, "d_pose": 72, "d_transl": 3}[k], self.name + " " + k) for k, t in o.items() if t is not None}


@functools.lru_cache(maxsize=None)
def _case(name):
    return _Case(name)


def _check(got, bound, what):
    over, worst = sr.compare(got, bound, what)
    assert not over, (what, "error / allow", over)
    return worst


# ---- ia_smpl_lbs_fwd -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sr.LBS_CASES))
def test_lbs_fwd_within_the_bound(name):
    """T_inv (rotation and translation block), verts, verts_t, w2s within allow; the fourth rows exactly 0 0 0 1; nothing behind
    row V; with verts, verts_t, w2s and transl all NULL, T_inv keeps the bits of the call that has them (transl = 0 there)"""
    c = _case(name)
    r = c.fwd(c.workspace())
    _check(sr.fwd_groups(r, "lbs"), sr.lbs_fwd_bound(name), "lbs_fwd " + name)
    full = c.fwd(c.workspace(), transl=torch.zeros(3, device=DEV))
    bare = c.fwd(c.workspace(), transl=None, verts=False, verts_t=False, w2s=False)
    assert set(bare) == {"T_inv"} and np.array_equal(_bits(bare["T_inv"]), _bits(full["T_inv"])), "T_inv depends on the optional pointers"
    if c.i["transl"] is None:
        assert _same(r, full), "NULL transl is not transl = 0"


# ---- ia_smpl_lbs_bwd -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bound_without_d_w2s(name):
    i = dict(sr.lbs_inputs(name), d_w2s=None)
    return sr._bwd_case(sr.lbs_bwd_ref, sr.lbs_args(i, True), ("d_transl",))[0]


@pytest.mark.parametrize("name", sorted(sr.LBS_CASES))
def test_lbs_bwd_within_the_bound(name):
    """d_pose of every joint, d_betas and d_transl within allow, after the case's own forward on the same workspace; then, all
    bit-equal to that: a second call (fixed-order sums, no atomics), a call on a workspace freshly filled with NaN with no
    forward before it, d_betas NULL, d_transl NULL.  Cases with d_w2s run once more without it: the bound of that reference,
    d_transl held to the cancellation floor K u M."""
    c = _case(name)
    ws = c.workspace()
    c.fwd(ws)
    first = c.bwd(ws)
    _check(sr.bwd_groups(first), sr.lbs_bwd_bound(name)[0], "lbs_bwd " + name)
    assert _same(first, c.bwd(ws)), "two backward calls differ"
    assert _same(first, c.bwd(c.workspace())), "the backward depends on what the forward left in the workspace"
    for null in ("d_betas", "d_transl"):
        r = c.bwd(c.workspace(), **{null: False})
        assert set(r) == {"d_betas", "d_pose", "d_transl"} - {null} and _same(r, first), null + " = NULL changes the other outputs"
    if c.i["d_w2s"] is not None:
        r = c.bwd(c.workspace(), d_w2s=False)
        _check(sr.bwd_groups(r), _bound_without_d_w2s(name), "lbs_bwd -d_w2s " + name)
        assert not np.array_equal(r["d_pose"][:3], first["d_pose"][:3]), "d_w2s is not read"


def test_lbs_bwd_on_a_workspace_last_used_by_a_larger_body():
    """the backward recomputes what it needs: on a workspace that the forward and backward of a larger body (V = 257, other
    pose, other parent table) used last, the V = 255 case gives the bits it gives after its own forward"""
    big, small = _case("smpl-random-257"), _case("chain-zero-255")
    ws = small.workspace()
    small.fwd(ws)
    own = small.bwd(ws)
    ws = big.workspace()
    big.fwd(ws)
    big.bwd(ws)
    assert _same(own, small.bwd(ws, ws_bytes=big.need)), "stale workspace contents reach the result"


def test_lbs_argument_errors_raise_and_launch_nothing():
    """a workspace one byte short (both entries), n_verts = 0, NULL d_pose: IAError, and no output element is written"""
    L = _lib()
    c = _case("star-mixed-1")
    ws = c.workspace()

    def untouched():
        torch.cuda.synchronize()
        assert all((_np(t) == SENTINEL).all() for t in c.raw.values() if t is not None) and (_np(ws) == 255).all()

    for call in (c.fwd, c.bwd):
        with pytest.raises(L.IAError, match="workspace"):
            call(ws, ws_bytes=c.need - 1)
        untouched()
    c.body.n_verts = 0
    try:
        for call in (c.fwd, c.bwd):
            with pytest.raises(L.IAError, match="body"):
                call(ws)
            untouched()
    finally:
        c.body.n_verts = c.V
    with pytest.raises(L.IAError, match="null"):
        c.bwd(ws, d_pose=False)
    untouched()


# ---- ia_smpl_tfs / ia_smpl_tfs_bwd -------------------------------------------------------------------------------------
def _tfs_dev(name):
    i = sr.tfs_inputs(name)
    return i, {k: _dev(v) for k, v in i.items()}


def _tfs(d, transl="case", A=True, w2s=True):
    o = dict(tfs=_out(24, 4, 4), w2s=_out(1, 4, 4) if w2s else None, A=_out(24, 4, 4) if A else None)
    _lib().call("ia_smpl_tfs", d["joints_rest"], d["parents"], d["pose"], d["transl"] if isinstance(transl, str) else transl, d["tfs_inv_t"],
                o["tfs"], o["w2s"], o["A"])
    torch.cuda.synchronize()
    r = {k: _take(t, 1 if k == "w2s" else 24, "tfs " + k) for k, t in o.items() if t is not None}
    if "w2s" in r:
        r["w2s"] = r["w2s"][0]
    return r


def _tfs_bwd(d, d_transl=True):
    o = dict(d_pose=_out(72), d_transl=_out(3) if d_transl else None)
    _lib().call("ia_smpl_tfs_bwd", d["joints_rest"], d["parents"], d["pose"], d["transl"], d["tfs_inv_t"], d["d_tfs"], o["d_pose"], o["d_transl"])
    torch.cuda.synchronize()
    return {k: _take(t, {"d_pose": 72, "d_transl": 3}[k], "tfs_bwd " + k) for k, t in o.items() if t is not None}


@pytest.mark.parametrize("name", sorted(sr.TFS_CASES))
def test_tfs_fwd_and_bwd_within_the_bound(name):
    """tfs, w2s and A (rotation and translation blocks; fourth rows exactly 0 0 0 1) with a general affine tfs_inv_t; A NULL
    leaves tfs and w2s bit-equal; a NULL transl is transl = 0.  d_pose per joint within allow, d_transl -- analytically zero --
    within the floor K u M; d_transl NULL leaves d_pose bit-equal; two calls give the same bits; the fourth row of d_tfs,
    filled with 1e30, is not read."""
    i, d = _tfs_dev(name)
    r = _tfs(d)
    _check(sr.fwd_groups(r, "tfs"), sr.tfs_fwd_bound(name), "tfs " + name)
    bare = _tfs(d, A=False)
    assert set(bare) == {"tfs", "w2s"} and _same(bare, r), "A = NULL changes tfs / w2s"
    if i["transl"] is None:
        assert _same(r, _tfs(d, transl=torch.zeros(3, device=DEV))), "NULL transl is not transl = 0"
    g = _tfs_bwd(d)
    _check(sr.bwd_groups(g), sr.tfs_bwd_bound(name)[0], "tfs_bwd " + name)
    assert _same(g, _tfs_bwd(d)), "two backward calls differ"
    bare = _tfs_bwd(d, d_transl=False)
    assert set(bare) == {"d_pose"} and _same(bare, g), "d_transl = NULL changes d_pose"
