"""The kernels of the forward half of a training step, each called alone through the C ABI on seeded host-built inputs
(tests/train_step_refs.py; no model, no world, no training):

  ia_march_train_compact   BIT FOR BIT against the oracle's dense march compacted in plain float32, on every input set (ten
                           max_samples around the steps-per-lane boundaries x 1 ... 203 rays x two grid sizes x three
                           occupancy grids x jitter / NULL); the dense ia_raymarch_train on the same inputs; sample_cap; arguments
  ia_nerf_loss             float64, |got - ref| <= K u M, all sizes x the poison / overflow matrix, both weight paths
  ia_transform_rays_w2s, ia_frame_stats   float64, K u M

tests/test_cpu_train_step_refs.py shows on the same inputs that a numpy restatement of the marcher equals the reference,
that plain fp32 attains every bound, and which mutants the comparisons reject.  Each bounded check prints the worst error /
bound it saw ("RATIO ..." lines, recorded in NOTES.md)."""
import numpy as np
import pytest
import torch

import train_step_refs as tr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.as_tensor(np.array(a, order="C")).to(DEV)       # (a copy: the shared inputs are read-only)


def _np(t):
    return t.detach().cpu().numpy()


def _ratio(got, ref, bound, what):
    """as in test_gpu_backward_kernels.py, and NaN exactly where the reference has NaN (a poisoned step)"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN where none is due or none where it is", int(np.isnan(got).sum()), int(nan.sum()))
    assert np.isfinite(got[~nan]).all(), (what, "non-finite output")
    err = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, ref)))
    z = (bound == 0) & ~nan
    assert (err[z] == 0).all(), (what, "differs where the bound is zero", int((err[z] != 0).sum()), float(err[z].max()))
    ok = ~z & ~nan
    r = err[ok] / bound[ok]
    worst = float(r.max()) if r.size else 0.0
    print("RATIO %-52s %.3f" % (what, worst))
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(np.where(ok, err / np.where(ok, bound, 1), 0))), err.shape)
        raise AssertionError((what, "error / bound", worst, "at", i, "got", float(got[i]), "ref", float(ref[i]), "bound", float(bound[i])))
    return worst


def _lib():
    from instantavatar_amd import _lib as L
    return L


# ---- marcher ---------------------------------------------------------------------------------------------------------
_BITS, _RAYS = {}, {}


def _occ(G, grid):
    if (G, grid) not in _BITS:
        L = _lib()
        desc = L.OccGrid()
        desc.G = G
        desc.aabb_min[:] = [float(v) for v in tr.MARCH_AABB[0]]
        desc.aabb_max[:] = [float(v) for v in tr.MARCH_AABB[1]]
        _BITS[(G, grid)] = (_dev(tr.pack_occupancy(tr.march_occupancy(G, grid))), desc)
    return _BITS[(G, grid)]


def _rays(ms, n):
    if (ms, n) not in _RAYS:
        r = tr.march_rays(ms, n)
        _RAYS[(ms, n)] = {k: _dev(r[k]) for k in ("o", "d", "near", "far", "jitter")}
        _RAYS[(ms, n)]["step"] = _dev(tr.step_size(r["near"], r["far"], ms))
    return _RAYS[(ms, n)]


def _march(ms, n, G, grid, jit, size, cap):
    """one call of ia_march_train_compact into sentinel-filled buffers of `size` samples; returns the outputs as numpy"""
    L = _lib()
    bits, desc = _occ(G, grid)
    r = _rays(ms, n)
    s_pts = torch.full((size, 3), float(tr.SENT_F), device=DEV)
    s_z = torch.full((size,), float(tr.SENT_F), device=DEV)
    s_slot = torch.full((size,), int(tr.SENT_I), dtype=torch.int32, device=DEV)
    ray_off, ray_cnt = torch.full((n,), -1, dtype=torch.int32, device=DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV)
    n_samples = torch.full((1,), 999, dtype=torch.int32, device=DEV)       # (zeroed inside)
    L.call("ia_march_train_compact", r["o"], r["d"], r["near"], r["far"], n, bits, desc, ms, r["jitter"] if jit else None, s_pts, s_z, s_slot,
           ray_off, ray_cnt, n_samples, cap)
    torch.cuda.synchronize()
    return dict(s_pts=_np(s_pts), s_z=_np(s_z), s_slot=_np(s_slot), ray_off=_np(ray_off), ray_cnt=_np(ray_cnt), n_samples=int(n_samples.item()))


@pytest.mark.parametrize("ms", tr.MARCH_MS)
def test_march_train_compact_bit_for_bit(oracle, ms):
    L = _lib()
    n_sets = n_total = 0
    for case in tr.march_cases(ms):
        n, G, grid, jit = case
        ref = tr.march_reference(ms, *case)
        size = ref["n_samples"] + 64
        got = _march(ms, n, G, grid, jit, size, size)
        try:
            tr.march_compare(got, ref)          # n_samples, ray_cnt, tiling, every sample's bits, sentinels behind n_samples
        except AssertionError as e:
            raise AssertionError(("max_samples %d, %d rays, G %d, grid %s, jitter %s" % (ms, n, G, grid, jit),) + e.args) from None
        if jit:
            continue
        # the dense marcher on the same inputs: the oracle's depths, bit for bit; the compact result is its compaction
        bits, desc = _occ(G, grid)
        r = _rays(ms, n)
        depths = torch.full((n, ms), float(tr.SENT_F), device=DEV)
        L.call("ia_raymarch_train", r["o"], r["d"], r["near"], r["far"], n, bits, desc, r["step"], ms, depths)
        torch.cuda.synchronize()
        z = _np(depths)
        assert np.array_equal(z.view(np.uint32), ref["dense"].view(np.uint32)), ("dense depths", ms, case)
        q = tr.march_rays(ms, n)
        tr.march_compare(got, tr.compact_from_dense(z, q["o"], q["d"], q["near"], q["far"], ms, None))
        n_sets += 1
        n_total += ref["n_samples"]
    assert n_sets == len(tr.march_cases(ms)) // 2 and n_total > 0


def test_march_train_compact_sample_cap(oracle):
    ms, case = 126, (203, 24, "block", True)
    ref = tr.march_reference(ms, *case)
    total = ref["n_samples"]
    assert total > 400
    tr.march_compare(_march(ms, *case, total, total), ref, sample_cap=total)
    # half the capacity, buffers of the full size: n_samples still reports the total, positions below the cap hold the sample
    # their ray_off assigns, everything from the cap on keeps the sentinel
    got = _march(ms, *case, total, total // 2)
    assert got["n_samples"] == total
    tr.march_compare(got, ref, sample_cap=total // 2)
    assert (got["s_z"][total // 2:] == tr.SENT_F).all() and (got["s_slot"][total // 2:] == tr.SENT_I).all() and (got["s_pts"][total // 2:] == tr.SENT_F).all()
    assert (got["s_z"][:total // 2] != tr.SENT_F).all()


def test_march_train_compact_arguments(oracle):
    L = _lib()
    ms_ok, case = 64, (9, 24, "full", True)
    bits, desc = _occ(24, "full")
    r = _rays(ms_ok, 9)
    for bad in (511, 0):
        bufs = [torch.full((64, 3), 5.0, device=DEV), torch.full((64,), 5.0, device=DEV), torch.full((64,), 5, dtype=torch.int32, device=DEV),
                torch.full((9,), 5, dtype=torch.int32, device=DEV), torch.full((9,), 5, dtype=torch.int32, device=DEV),
                torch.full((1,), 5, dtype=torch.int32, device=DEV)]
        with pytest.raises(L.IAError, match="ia_march_train_compact: bad sizes"):
            L.call("ia_march_train_compact", r["o"], r["d"], r["near"], r["far"], 9, bits, desc, bad, None, *bufs, 64)
        assert b"bad sizes" in L.lib().ia_last_error()
        torch.cuda.synchronize()
        assert all((_np(b) == 5).all() for b in bufs), "something was launched"
    n_samples = torch.full((1,), 999, dtype=torch.int32, device=DEV)
    assert L.call("ia_march_train_compact", None, None, None, None, 0, None, None, ms_ok, None, None, None, None, None, None, n_samples, 0) == 0
    torch.cuda.synchronize()
    assert int(n_samples.item()) == 0


# ---- loss ------------------------------------------------------------------------------------------------------------
def _loss_call(call, misalign=False):
    """one call of ia_nerf_loss; gradients into buffers prefilled with 5; returns outputs (numpy), the reference, the bounds"""
    L = _lib()
    N, M, w, p, c, pre, vec = call
    inp = tr.loss_inputs(N, M)
    ref = tr.nerf_loss_ref(**inp, w_rgb=w[0], w_alpha=w[1], w_reg=w[2], poison=p, overflow_count=c, overflow_cap=tr.LOSS_CAP, out_pre=pre)
    d = {k: _dev(v) for k, v in inp.items()}
    off = 1 if misalign else 0
    wbuf, dwbuf = torch.zeros(M + 8, device=DEV), torch.full((M + 8,), 5.0, device=DEV)
    wbuf[off:off + M] = d["weight"]
    weight, d_weight = wbuf[off:off + M], dwbuf[off:off + M]
    assert M == 0 or (weight.data_ptr() % 16 == 0) == (not misalign)
    out = torch.zeros(6, device=DEV) if pre is None else _dev(np.asarray(pre, np.float32))
    d_rgb, d_alpha = torch.full((N, 3), 5.0, device=DEV), torch.full((N,), 5.0, device=DEV)
    poison = None if p is None else torch.tensor([p], dtype=torch.float32, device=DEV)
    count = None if c is None else torch.tensor([c], dtype=torch.int32, device=DEV)
    L.call("ia_nerf_loss", d["rgb"], d["tgt_rgb"], d["alpha"], d["tgt_alpha"], weight if M else None, N, M, w[0], w[1], w[2], poison, count,
           tr.LOSS_CAP, out, d_rgb, d_alpha, d_weight if M else None)
    torch.cuda.synchronize()
    assert (_np(dwbuf)[:off] == 5).all() and (_np(dwbuf)[off + M:] == 5).all(), "d_weight written outside its range"
    got = dict(out=_np(out), d_rgb=_np(d_rgb).reshape(-1), d_alpha=_np(d_alpha), d_weight=_np(d_weight).copy())
    return got, ref, tr.nerf_loss_bounds(ref, vec)


@pytest.mark.parametrize("size", tr.LOSS_SIZES, ids=lambda s: "%dx%d" % s)
def test_nerf_loss_values_and_gradients(size):
    calls = [c for c in tr.loss_calls() if (c[0], c[1]) == size]
    assert len(calls) >= 12
    worst = {}
    for call in calls:
        N, M, w, p, c, pre, vec = call
        misalign = (M % 4 == 0) and not vec
        got, ref, bounds = _loss_call(call, misalign)
        tag = "loss %dx%d w%s p=%s c=%s%s%s " % (N, M, w[1], p, c, " pre" if pre else "", " off-16" if misalign else "")
        for k in ("out", "d_rgb", "d_alpha", "d_weight"):
            worst[k] = max(worst.get(k, 0.0), _ratio(got[k], ref[k], bounds[k], tag + k))
        poisoned = (p is not None and p > 0) or (c is not None and c > tr.LOSS_CAP)
        assert np.isnan(got["out"][0]) == poisoned and np.isfinite(got["out"][1:5]).all()
        for k in ("d_rgb", "d_alpha", "d_weight"):
            assert np.isnan(got[k]).all() if poisoned else np.isfinite(got[k]).all(), k
        assert got["out"][5] == ((tr.LOSS_PRE[5] if pre else 0.0) if c is None else float(c > tr.LOSS_CAP))
    for k, v in worst.items():
        print("RATIO loss %dx%d worst %-39s %.3f" % (size + (k, v)))


@pytest.mark.parametrize("size", [(64, 64 * 256), (300, 128 * 1024 * 2 + 4)], ids=lambda s: "%dx%d" % s)
def test_nerf_loss_weight_paths_agree_bit_for_bit(size):
    """the same data through the 16-byte path and, given one float off alignment, through the scalar path: the same per-element
    arithmetic, so the same gradient bits (the values differ in summation order only and are bounded above)"""
    call = (size[0], size[1], tr.LOSS_WEIGHTS[0], None, None, None, True)
    a, _, _ = _loss_call(call, misalign=False)
    b, _, _ = _loss_call(call[:6] + (False,), misalign=True)
    for k in ("d_weight", "d_rgb", "d_alpha"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.isfinite(a["d_weight"]).all() and (a["d_weight"] != 5).all()


# ---- ray set-up and frame statistics ---------------------------------------------------------------------------------
@pytest.mark.parametrize("R", tr.RAYS_R)
def test_transform_rays_w2s(R):
    L = _lib()
    inp = tr.transform_inputs(R)
    ref, bound = tr.transform_rays_w2s_ref(**inp)
    o2, d2 = torch.full((R + 3, 3), 5.0, device=DEV), torch.full((R + 3, 3), 5.0, device=DEV)
    near, far = torch.full((R + 3,), 5.0, device=DEV), torch.full((R + 3,), 5.0, device=DEV)
    L.call("ia_transform_rays_w2s", _dev(inp["o"]), _dev(inp["d"]), _dev(inp["w2s"]), R, o2, d2, near, far)
    torch.cuda.synchronize()
    got = dict(o=_np(o2), d=_np(d2), near=_np(near), far=_np(far))
    assert (ref["near"] < 0).any()
    for k in ("o", "d", "near", "far"):
        assert (got[k][R:] == 5).all(), (k, "written past R")
        _ratio(got[k][:R], ref[k], bound[k], "transform_rays R %d %s" % (R, k))


@pytest.mark.parametrize("R", tr.STATS_R)
def test_frame_stats(R):
    L = _lib()
    inp = tr.stats_inputs(R)
    ref, bound = tr.frame_stats_ref(inp["counter"], inp["alpha"], tr.STATS_PRE)
    acc = _dev(np.asarray(tr.STATS_PRE + (9.0,), np.float32))
    L.call("ia_frame_stats", _dev(inp["counter"]), _dev(inp["alpha"]), R, acc)
    torch.cuda.synchronize()
    got = _np(acc)
    assert got[2] == 9.0
    _ratio(got[:2], ref, bound, "frame_stats R %d" % R)
