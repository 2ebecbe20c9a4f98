"""The three fused-MLP entries, each called alone through the C ABI on seeded host-built inputs and compared with the float64
restatements of tests/mlp_refs.py: ia_field_bwd (on integer lattices bit for bit, and real-valued against the per-element
bound propagated through the reference), ia_field_grad_scale (bit for bit) and the activation record of ia_field_fwd_train
(stage by stage from the kernel's own previous stage).  No training, no autograd wrapper.  The bounds are derived in
mlp_refs.py; tests/test_cpu_mlp_refs.py shows on the CPU that plain fp32 attains them and that six mutants do not.  Each
check prints the worst error / bound it saw ("RATIO ..." lines, recorded in NOTES.md)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_refs as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IA_OK, IA_ERR_WORKSPACE = 0, -3


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _ratio(got, ref, bound, what):
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert np.isfinite(got).all(), (what, "non-finite output")
    err = np.abs(got - ref)
    z = bound == 0
    assert (err[z] == 0).all(), (what, "differs where the bound is zero", int((err[z] != 0).sum()), float(err[z].max()))
    r = err[~z] / bound[~z]
    worst = float(r.max()) if r.size else 0.0
    print("RATIO %-52s %.3f  (bound zero on %d of %d)" % (what, worst, int(z.sum()), z.size))
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(np.where(z, 0, err / np.where(z, 1, bound)))), err.shape)
        raise AssertionError((what, "error / bound", worst, "at", i, "got", float(got[i]), "ref", float(ref[i]), "bound", float(bound[i])))
    return worst


def _lib():
    from instantavatar_amd import _lib as L
    return L


class _Field:
    """a field descriptor over host-built weights (and table), with the tensors it points to"""

    def __init__(self, n_levels, W, table=None, center=(0, 0, 0), fscale=(1, 1, 1), frags=True):
        L = _lib()
        self.n_levels = n_levels
        self.hd = L.make_hash_desc(n_levels)
        self.t = {k: _dev(np.asarray(W[k], np.float16)) for k in mr.WEIGHT_NAMES}
        self.t["table"] = torch.zeros(64, dtype=torch.float16, device=DEV) if table is None else table
        f = self.f = L.Field()
        f.center[:], f.scale[:] = [float(v) for v in center], [float(v) for v in fscale]
        f.hash = self.hd
        f.table = self.t["table"].data_ptr()
        f.sig_w1, f.sig_w2 = self.t["W1"].data_ptr(), self.t["W2"].data_ptr()
        f.col_w1, f.col_w2, f.col_w3 = self.t["Wc1"].data_ptr(), self.t["Wc2"].data_ptr(), self.t["Wc3"].data_ptr()
        f.mlp_frags, f.enc_ws, f.enc_ws_samples, f.enc_split = None, None, 0, 0
        if frags:
            self.t["frags"] = torch.zeros(L.lib().ia_field_frags_bytes() // 2, dtype=torch.float16, device=DEV)
            L.check(L.lib().ia_field_prepare(C.byref(f), L.ptr(self.t["frags"]), L.stream()), "ia_field_prepare")
            f.mlp_frags = self.t["frags"].data_ptr()

    def with_enc_ws(self, samples):
        self.t["enc_ws"] = torch.zeros(self.n_levels * samples, dtype=torch.int32, device=DEV)
        self.f.enc_ws, self.f.enc_ws_samples = self.t["enc_ws"].data_ptr(), samples
        return self


# ---- ia_field_bwd ----------------------------------------------------------------------------------------------------
def _bwd(fd, inp, S_dev, prefill, ws_extra=0, ws_short=0, V=None):
    """one call of ia_field_bwd alone: -> (status, dfeat, {g_*}); dfeat is pre-filled with 7.0, the workspace with NaN bits"""
    L = _lib()
    nl = fd.n_levels
    V = len(inp["acts"]) if V is None else V
    d = inp["_dev"]
    dfeat = torch.full((len(inp["acts"]), 2 * nl), 7.0, device=DEV)
    g = {k: _dev(prefill[k]) for k in mr.GRADS}
    need = L.lib().ia_field_bwd_workspace_bytes(V, nl)
    ws = torch.full((need + ws_extra + 16,), 255, dtype=torch.uint8, device=DEV)
    nd = None if inp["n_live"] is None else torch.tensor([inp["n_live"]], dtype=torch.int32, device=DEV)
    rc = L.lib().ia_field_bwd(L.ptr(d["acts"]), L.ptr(d["rgb"]), L.ptr(d["d_rgb"]), L.ptr(d["d_sigma"]), V, L.ptr(nd), L.ptr(S_dev),
                              C.byref(fd.f), L.ptr(dfeat), L.ptr(g["w1"]), L.ptr(g["w2"]), L.ptr(g["c1"]), L.ptr(g["c2"]), L.ptr(g["c3"]),
                              L.ptr(ws), need + ws_extra - ws_short, L.stream())
    torch.cuda.synchronize()
    return rc, _np(dfeat), {k: _np(v) for k, v in g.items()}


def _to_dev(inp):
    inp["_dev"] = {k: _dev(inp[k]) for k in ("acts", "rgb", "d_rgb", "d_sigma")}
    return inp


def _same_bits(a, b):
    return np.array_equal(_bits(a[1]), _bits(b[1])) and all(np.array_equal(_bits(a[2][k]), _bits(b[2][k])) for k in mr.GRADS)


@pytest.mark.parametrize("n_levels,V,n_live", mr.LATTICE_CASES)
def test_field_bwd_on_the_lattice_is_exact(n_levels, V, n_live):
    """integer inputs on which every operation of the backward is exact in half and fp32 (asserted by the builder): the
    kernel equals the float64 reference bit for bit -- dfeat, and prefill + gradient in the five g_* buffers"""
    L = _lib()
    assert L.lib().ia_field_bwd_workspace_bytes(V, n_levels) == mr.bwd_workspace_bytes(V, n_levels)
    pre = mr.lattice_prefill(n_levels)
    for S in mr.lattice_scales(V):
        inp, R = mr.lattice_inputs(n_levels, V, S, n_live)
        _to_dev(inp)
        fd = _Field(n_levels, inp)
        S_dev = torch.tensor([S], dtype=torch.float32, device=DEV)
        n = R["n"]
        what = "lattice L%d V%d%s S%g " % (n_levels, V, "" if n_live is None else " n_dev%d" % n_live, S)
        first = _bwd(fd, inp, S_dev, pre)
        rc, dfeat, g = first
        assert rc == IA_OK
        assert (dfeat[n:] == 7.0).all(), "dfeat rows at or past *n_dev were written"
        _ratio(dfeat[:n], R["dfeat"], np.zeros_like(R["dfeat"]), what + "dfeat")
        for k in mr.GRADS:
            _ratio(g[k], pre[k] + R["g_" + k], np.zeros(g[k].shape), what + "g_" + k)
        # identical bits from a second call, and with a workspace larger than required
        assert _same_bits(first, _bwd(fd, inp, S_dev, pre)), "two back-to-back calls differ"
        assert _same_bits(first, _bwd(fd, inp, S_dev, pre, ws_extra=4096 + 64)), "a larger workspace changes the result"
        if S != mr.LATTICE_SCALES[-1]:
            continue
        # a workspace that is too small: the workspace error, nothing written
        rc, dfeat, g = _bwd(fd, inp, S_dev, pre, ws_short=4)
        assert rc == IA_ERR_WORKSPACE and (dfeat == 7.0).all() and all(np.array_equal(g[k], pre[k]) for k in mr.GRADS)
        # no samples: OK, nothing written
        rc, dfeat, g = _bwd(fd, inp, S_dev, pre, V=0)
        assert rc == IA_OK and (dfeat == 7.0).all() and all(np.array_equal(g[k], pre[k]) for k in mr.GRADS)


@functools.lru_cache(maxsize=None)
def _real_field(n_levels):
    """xavier weights and a random table in a body-sized box, shared by the real-valued tests"""
    W = mr.xavier_weights(n_levels)
    n_entries = int(_lib().make_hash_desc(n_levels).offset[n_levels])
    return W, _dev(mr.real_table(n_entries))


def _fwd_train(fd, x, n_dev=None, fill=True):
    """one call of ia_field_fwd_train alone -> (rgb, sigma, acts) on the host; rows the call does not write keep 9.0 / 0x1234"""
    L = _lib()
    V = len(x)
    rgb, sigma = torch.full((V, 3), 9.0, device=DEV), torch.full((V,), 9.0, device=DEV)
    acts = torch.full((V, mr.act_stride(fd.n_levels)), 0x1234, dtype=torch.int16, device=DEV).view(torch.float16)
    assert L.lib().ia_field_act_stride(fd.n_levels) == acts.shape[1]
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    L.check(L.lib().ia_field_fwd_train(L.ptr(x), V, L.ptr(nd), C.byref(fd.f), L.ptr(rgb), L.ptr(sigma), L.ptr(acts), L.stream()), "ia_field_fwd_train")
    torch.cuda.synchronize()
    return _np(rgb), _np(sigma), _np(acts)


@pytest.mark.parametrize("n_levels", [8, 16])
def test_field_bwd_real_valued_within_the_propagated_bound(n_levels):
    """fp16 weights of the synthetic field's magnitude, the record and rgb of ia_field_fwd_train, gradients over 24 binades
    (some rows land in the subnormal halves), *scale from ia_field_grad_scale: every element of dfeat and of the five
    weight gradients within the bound propagated through the float64 reference (mlp_refs.py: derivation)"""
    L = _lib()
    W, table = _real_field(n_levels)
    fd = _Field(n_levels, W, table, mr.REAL_CENTER, mr.REAL_SCALE)
    V = mr.REAL_V
    rgb, _, acts = _fwd_train(fd, _dev(mr.real_points(V)))
    d_rgb, d_sigma = mr.real_gradients(V)
    inp = _to_dev(dict(acts=acts, rgb=rgb, d_rgb=d_rgb, d_sigma=d_sigma, n_live=None, **W))
    state, S_dev = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(1, device=DEV)
    d = inp["_dev"]
    L.check(L.lib().ia_field_grad_scale(L.ptr(d["rgb"]), L.ptr(d["d_rgb"]), L.ptr(d["d_sigma"]), V, None, L.ptr(state), L.ptr(S_dev), L.stream()),
            "ia_field_grad_scale")
    S = _np(S_dev)[0]
    assert _bits(np.array([S]))[0] == _bits(np.array([mr.grad_scale_ref(rgb, d_rgb, d_sigma, None)]))[0] and (_np(state) == 0).all()
    R = mr.mlp_bwd_ref(acts, rgb, d_rgb, d_sigma, None, S, **W)
    mr.assert_real_case_is_hard(R)
    zero = {k: np.zeros(s, np.float32) for k, s in mr.GRAD_SHAPES(n_levels).items()}
    rc, dfeat, g = _bwd(fd, inp, S_dev, zero)
    assert rc == IA_OK
    what = "real L%d V%d " % (n_levels, V)
    _ratio(dfeat, R["dfeat"], R["b_dfeat"], what + "dfeat")
    for k in mr.GRADS:
        _ratio(g[k], R["g_" + k], R["b_" + k], what + "g_" + k)


# ---- ia_field_grad_scale ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", (0,) + mr.SCALE_V)
def test_grad_scale_is_exact(V):
    """*scale against the numpy fp32 reference, bit for bit (a maximum has no summation order); the ticket state is left zero
    by every call, NaN and Inf give NaN, and the call after a NaN call is clean"""
    L = _lib()
    rgb, d_rgb, d_sigma = mr.grad_scale_inputs(V)
    state, scale = torch.zeros(2, dtype=torch.int32, device=DEV), torch.full((1,), 123.0, device=DEV)
    rgb_d = _dev(rgb)

    def run(g, s, n_dev=None):
        nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
        g_d, s_d = _dev(g), _dev(s)
        scale.fill_(123.0)
        L.check(L.lib().ia_field_grad_scale(L.ptr(rgb_d), L.ptr(g_d), L.ptr(s_d), V, L.ptr(nd), L.ptr(state), L.ptr(scale), L.stream()),
                "ia_field_grad_scale")
        torch.cuda.synchronize()
        assert (_np(state) == 0).all(), "state2 is not left zero"
        return _np(scale)[0], mr.grad_scale_ref(rgb, g, s, n_dev)

    def same(got_ref, what):
        got, ref = got_ref
        assert _bits(np.array([got]))[0] == _bits(np.array([ref]))[0], (what, V, got, ref)
        return got

    first = same(run(d_rgb, d_sigma), "plain")
    assert same(run(0 * d_rgb, 0 * d_sigma), "all gradients zero") == mr.SCALE_EMPTY
    if V == 0:
        assert first == mr.SCALE_EMPTY
        return
    assert same(run(d_rgb, d_sigma), "again") == first and np.isfinite(first)
    yy = rgb * (1 - rgb)
    i, c = np.unravel_index(int(np.argmax(yy)), yy.shape)          # (any sample will do; this one has the largest y (1 - y))
    s = d_sigma.copy()
    s[i] = -57.3
    assert same(run(d_rgb, s), "maximum in d_sigma") == np.float32(1024) / np.float32(57.3)
    g = d_rgb.copy()
    g[i, c] = 1234.5
    assert same(run(g, d_sigma), "maximum in the rgb term") == np.float32(1024) / ((g[i, c] * rgb[i, c]) * (np.float32(1) - rgb[i, c]))
    # a huge value only past *n_dev is ignored (with it the scale would be 1024 / 1e30)
    n_dev = V - 1 - (V > 300) * 77
    s, g = d_sigma.copy(), d_rgb.copy()
    s[n_dev:], g[n_dev:] = 1e30, -1e30
    assert same(run(g, s, n_dev), "huge past n_dev") > 1.0
    # NaN and Inf anywhere among the live samples give NaN; the next finite call gives the finite answer
    for bad, in_sigma in ((np.nan, False), (np.inf, True), (-np.inf, False), (np.nan, True)):
        s, g = d_sigma.copy(), d_rgb.copy()
        if in_sigma:
            s[i] = bad
        else:
            g[i, c] = bad
        got, ref = run(g, s)
        assert np.isnan(got) and np.isnan(ref), (bad, in_sigma, got)
        same(run(d_rgb, d_sigma), "finite after a non-finite call")


# ---- ia_field_fwd_train ----------------------------------------------------------------------------------------------
FWD_CASES = tuple((L, V, None) for L in (8, 16) for V in mr.FWD_V[:-1]) + ((8, 769, 700), (16, 769, 700), (16, mr.SHARD_V, mr.SHARD_V - 100),
                                                                           (8, mr.SHARD_V, None), (16, mr.FWD_V[-1], None))


@pytest.mark.parametrize("n_levels,V,n_dev", FWD_CASES)
def test_fwd_train_record_stage_by_stage(n_levels, V, n_dev):
    """rgb / sigma equal ia_field_fwd and the record's features equal ia_hashgrid_fwd bit for bit; the same bits without
    mlp_frags and (V >= 8192) with the sharded encoding; every MLP stage of the record against the float64 product of the
    record's own previous stage: exact wherever the value is clear of a rounding boundary, else the neighbouring half.
    The largest V is 256 workgroups x 12 waves x 64 samples, one more full tile and 5 samples: a second round of the wave loop."""
    L = _lib()
    W, table = _real_field(n_levels)
    fd = _Field(n_levels, W, table, mr.REAL_CENTER, mr.REAL_SCALE)
    x = _dev(mr.real_points(V))
    n = V if n_dev is None else n_dev
    rgb, sigma, acts = _fwd_train(fd, x, n_dev)
    what = "fwd_train L%d V%d " % (n_levels, V)
    # rows at or past *n_dev keep their prefill
    assert (rgb[n:] == 9.0).all() and (sigma[n:] == 9.0).all() and (_bits(acts[n:]) == 0x1234).all()
    # the inference kernel and the encoding alone
    rgb0, sigma0 = torch.full((V, 3), 9.0, device=DEV), torch.full((V,), 9.0, device=DEV)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    L.check(L.lib().ia_field_fwd(L.ptr(x), V, L.ptr(nd), C.byref(fd.f), L.ptr(rgb0), L.ptr(sigma0), L.stream()), "ia_field_fwd")
    feat = torch.zeros((V, 2 * n_levels), dtype=torch.float16, device=DEV)
    L.check(L.lib().ia_hashgrid_fwd(L.ptr(x), V, C.byref(fd.f), L.ptr(feat), L.stream()), "ia_hashgrid_fwd")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(rgb), _bits(_np(rgb0))) and np.array_equal(_bits(sigma), _bits(_np(sigma0))), "differs from ia_field_fwd"
    assert np.array_equal(_bits(acts[:n, :2 * n_levels]), _bits(_np(feat)[:n])), "record features differ from ia_hashgrid_fwd"
    # other routes, same bits
    routes = [("no mlp_frags", _Field(n_levels, W, table, mr.REAL_CENTER, mr.REAL_SCALE, frags=False))]
    if V >= 8192:
        routes.append(("sharded encoding", _Field(n_levels, W, table, mr.REAL_CENTER, mr.REAL_SCALE).with_enc_ws(V + 11)))
    for name, other in routes:
        r2, s2, a2 = _fwd_train(other, x, n_dev)
        assert np.array_equal(_bits(rgb), _bits(r2)) and np.array_equal(_bits(sigma), _bits(s2)) and np.array_equal(_bits(acts), _bits(a2)), name
    # the MLP, stage by stage
    rec = mr.split_record(acts[:n])
    checks = mr.fwd_record_checks(rec, **W)
    for k in ("h1", "out", "c1", "c2"):
        _ratio(rec[k], *checks[k], what + k)
    _ratio(rgb[:n], *checks["rgb"], what + "rgb")
    assert np.array_equal(_bits(sigma[:n]), _bits(rec["out"][:, 0].astype(np.float32))), "sigma is not out[0]"
    assert np.isfinite(acts[:n].astype(np.float32)).all()
