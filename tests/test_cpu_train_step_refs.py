"""Pins tests/train_step_refs.py itself (no GPU): the numpy restatement of the marcher KERNEL equals the oracle-based
reference bit for bit on every input set of tests/test_gpu_train_step_kernels.py; the input sets contain what they claim
(slot-cap rays, masked leading slots, t == 0 slots, rays that miss the box and still sample, empty rays); one-line
mutants of the emulation are each rejected by the comparison the GPU test makes; and for the loss, the ray set-up and the
frame statistics a plain float32 evaluation in the kernel's order stays inside every bound while six mutants of the loss do
not."""
import numpy as np
import pytest

import train_step_refs as tr


def _ratio(got, ref, bound, what, quiet=False):
    """worst |got - ref| / bound; NaN exactly where the reference has NaN; exact where the bound is 0.  Returns the ratio
    (inf for a NaN mismatch or a difference at a zero bound) -- the callers assert."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    nan = np.isnan(ref)
    if (np.isnan(got) != nan).any():
        return np.inf
    err = np.abs(got - ref)[~nan]
    b = bound[~nan]
    z = b == 0
    if (err[z] != 0).any():
        return np.inf
    r = float((err[~z] / b[~z]).max()) if (~z).any() else 0.0
    if not quiet:
        print("RATIO cpu-fp32 %-50s %.3f" % (what, r))
    return r


# ---- marcher ---------------------------------------------------------------------------------------------------------
def _emulate(ms, n, G, grid, jit, **kw):
    r = tr.march_rays(ms, n)
    return tr.march_train_compact_emulated(r["o"], r["d"], r["near"], r["far"], tr.march_occupancy(G, grid), tr.MARCH_AABB, ms,
                                           r["jitter"] if jit else None, **kw)


@pytest.mark.parametrize("ms", tr.MARCH_MS)
def test_march_emulation_equals_reference_bit_for_bit(oracle, ms):
    total = 0
    for case in tr.march_cases(ms):
        ref = tr.march_reference(ms, *case)
        tr.march_compare(_emulate(ms, *case, size=ref["n_samples"] + 64), ref)
        total += ref["n_samples"]
    assert total > 0


@pytest.mark.parametrize("ms", tr.MARCH_MS)
def test_march_input_sets_contain_what_they_claim(oracle, ms):
    r = tr.march_rays(ms, 203)
    kinds = np.array(r["kinds"])
    steps = tr.loop_steps(r["near"], r["far"], ms)
    # the kernel's `+ 2`: no reference loop runs past max_samples + 1 steps (counted to max_samples + 8)
    for n in tr.MARCH_NRAYS:
        q = tr.march_rays(ms, n)
        assert tr.loop_steps(q["near"], q["far"], ms).max() <= ms + 1
        if n >= 7:
            have = set(q["kinds"])
            assert {"block", "miss", "inner", "zero", "large"} <= have and have & {"eq", "lt"} and have & {"nan_near", "nan_far"}
        if n >= 9:
            assert {"eq", "lt", "nan_near", "nan_far"} <= set(q["kinds"])
    # slot cap: a ray of the training form (near / far = |o| -+ 1) whose loop takes max_samples + 1 steps; in the fully occupied
    # grid every step takes a slot, so the last one is past the cap.  The reference does this at every max_samples that is no
    # power of two and (for these rays) at none that is: not forced there.
    train_form = np.isin(kinds, ("block", "miss", "inner", "large"))
    share = float((steps[train_form] == ms + 1).mean())
    print("SLOTCAP max_samples %3d: %5.1f %% of %d rays with near / far = |o| -+ 1 take max_samples + 1 steps" % (ms, 100 * share, train_form.sum()))
    if ms & (ms - 1):
        assert share > 0
        full = tr.march_reference(ms, 203, 64, "full", True)
        capped = train_form & (steps == ms + 1) & (r["near"] > 0)
        assert capped.any() and (full["ray_cnt"][capped] == ms).all()
    # masked leading slots followed by kept ones: the first kept sample's slot is > 0
    for grid in ("block", "full"):
        ref = tr.march_reference(ms, 203, 64, grid, True)
        first = ref["s_slot"][np.minimum(ref["ray_start"], max(ref["n_samples"] - 1, 0))]
        masked_then_kept = (ref["ray_cnt"] > 0) & (first > 0) & (kinds == "inner")
        assert masked_then_kept.any() or ms == 1, grid          # (one step: it is masked or kept, not both)
    # a t == 0 slot: an occupied step at depth exactly 0 takes a slot and is masked
    full = tr.march_reference(ms, 203, 64, "full", True)
    z0 = np.nonzero(kinds == "zero0")[0]
    assert z0.size and (r["near"][z0] == 0).all()
    if ms > 1:      # step 0 took slot 0 and is masked: the first kept sample sits in slot 1
        assert (full["ray_cnt"][z0] > 0).all() and (full["s_slot"][full["ray_start"][z0]] == 1).all()
    else:
        assert (full["ray_cnt"][z0] == 0).all()
    if ms in (2, 64, 256):
        i = int(np.nonzero(kinds == "zero")[0][0])
        ts = tr.running_sum(r["near"][i:i + 1], tr.step_size(r["near"][i:i + 1], r["far"][i:i + 1], ms), ms)[0]
        assert ts[ms // 2] == 0 and full["ray_cnt"][i] == ms // 2 - 1
        assert ms == 2 or full["s_slot"][full["ray_start"][i]] == ms // 2 + 1      # (at 2 the steps are -1 and 0: nothing is kept)
    # rays that miss the box sample through the border cells; the same rays are empty in the block of the other grids' interior
    for G in tr.MARCH_G:
        border = tr.march_reference(ms, 203, G, "border", True)
        assert (border["ray_cnt"][kinds == "miss"] > 0).all()
    # empty rays: the degenerate ones in every grid
    for grid in tr.MARCH_GRIDS:
        ref = tr.march_reference(ms, 203, 24, grid, False)
        assert (ref["ray_cnt"][np.isin(kinds, ("eq", "lt", "nan_near", "nan_far"))] == 0).all()
    # jitter rows: exact zeros and the largest float below 1 sit on rays that sample
    assert (r["jitter"][1] == 0).all() and (r["jitter"][2] == tr.ONE_BELOW).all()
    assert full["ray_cnt"][1] > 0 and (full["ray_cnt"][2] > 0 or ms == 1)      # (row 2 is an `inner` ray: its one step at 1 is masked)


@pytest.mark.parametrize("mutant", tr.MARCH_MUTANTS)
def test_march_mutants_are_rejected(oracle, mutant):
    rejected = []
    for ms in tr.MARCH_MS:
        for case in tr.march_cases(ms):
            if case[0] != 203:
                continue
            ref = tr.march_reference(ms, *case)
            try:
                tr.march_compare(_emulate(ms, *case, size=ref["n_samples"] + 64 + 203, mutant=mutant), ref)
            except AssertionError:
                rejected.append((ms,) + case)
    print("MUTANT %-15s rejected on %3d of %d sets of 203 rays, max_samples %s" % (mutant, len(rejected), len(tr.MARCH_MS) * 12,
                                                                                 sorted({c[0] for c in rejected})))
    assert rejected


def test_march_sample_cap_in_the_emulation(oracle):
    ms, case = 126, (203, 24, "block", True)
    ref = tr.march_reference(ms, *case)
    total = ref["n_samples"]
    assert total > 400
    tr.march_compare(_emulate(ms, *case, size=total, sample_cap=total), ref, sample_cap=total)
    tr.march_compare(_emulate(ms, *case, size=total, sample_cap=total // 2), ref, sample_cap=total // 2)
    with pytest.raises(AssertionError):      # the comparison sees a buffer written past the cap
        tr.march_compare(_emulate(ms, *case, size=total, sample_cap=total // 2 + 1), ref, sample_cap=total // 2)


def test_fma32_rounds_once():
    from fractions import Fraction
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal(4000).astype(np.float32), rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.standard_normal(4000) * 2.0 ** rng.integers(-30, 0, 4000))).astype(np.float32)
    got = tr.fma32(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        e = abs(Fraction(float(got[i])) - exact)
        assert e <= abs(Fraction(float(lo)) - exact) and e <= abs(Fraction(float(hi)) - exact), i


# ---- loss ------------------------------------------------------------------------------------------------------------
def _loss_worst(call, mutant=None):
    N, M, w, p, c, pre, vec = call
    inp = tr.loss_inputs(N, M)
    ref = tr.nerf_loss_ref(**inp, w_rgb=w[0], w_alpha=w[1], w_reg=w[2], poison=p, overflow_count=c, overflow_cap=tr.LOSS_CAP, out_pre=pre)
    bounds = tr.nerf_loss_bounds(ref, vec)
    got = tr.nerf_loss_fp32(**inp, w_rgb=w[0], w_alpha=w[1], w_reg=w[2], poison=p, overflow_count=c, overflow_cap=tr.LOSS_CAP, out_pre=pre,
                            vec=vec, mutant=mutant)
    return {k: _ratio(got[k], ref[k], bounds[k], k, quiet=True) for k in ("out", "d_rgb", "d_alpha", "d_weight")}, ref


def test_loss_plain_fp32_attains_every_bound():
    worst = {}
    for call in tr.loss_calls():
        r, ref = _loss_worst(call)
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert max(r.values()) <= 1.0, (call[:2], call[3:], r)
        # the poison rule itself
        N, M, w, p, c, pre, vec = call
        want = (p is not None and p > 0) or (c is not None and c > tr.LOSS_CAP)
        assert ref["poisoned"] == want and np.isnan(ref["out"][0]) == want and np.isfinite(ref["out"][1:5]).all()
        assert all(np.isnan(ref[k]).all() == want or ref[k].size == 0 for k in ("d_rgb", "d_alpha", "d_weight"))
        assert ref["out"][5] == ((7.0 if pre else 0.0) if c is None else float(c > tr.LOSS_CAP))
    for k, v in worst.items():
        print("RATIO cpu-fp32 loss %-45s %.3f" % (k, v))


@pytest.mark.parametrize("mutant", tr.LOSS_MUTANTS)
def test_loss_mutants_miss_a_bound(mutant):
    worst = max(max(_loss_worst(call, mutant)[0].values()) for call in tr.loss_calls())
    print("MUTANT loss %-15s worst error / bound %.3g" % (mutant, worst))
    assert worst > 1.0


def test_loss_edges_are_in_the_inputs():
    inp = tr.loss_inputs(1000, 7000)
    w, a = inp["weight"], inp["alpha"]
    assert (w == 0).any() and (w == 1).any() and np.median(w) < 0.1
    assert (a == 0).any() and (a == 0.5).any() and (a == 1).any()
    assert (inp["tgt_rgb"] == 0).any() and (inp["tgt_rgb"] == 1).any() and set(np.unique(inp["tgt_alpha"])) == {0.0, 1.0}
    g = tr.loss_geometry(300, 128 * 1024 * 2 + 4, True), tr.loss_geometry(300, 128 * 1024 * 2 + 5, False)
    assert g[0]["B"] == g[1]["B"] == 128 and g[0]["L_w"] - 2 > 1 and g[1]["L_w"] > 1        # more than one grid-stride trip


# ---- ray set-up and frame statistics ---------------------------------------------------------------------------------
@pytest.mark.parametrize("R", tr.RAYS_R)
def test_transform_rays_plain_fp32_attains_the_bounds(R):
    inp = tr.transform_inputs(R)
    ref, bound = tr.transform_rays_w2s_ref(**inp)
    got = tr.transform_rays_w2s_fp32(**inp)
    assert (ref["near"] < 0).any() and (R < 4 or (ref["near"] > 0).any())
    assert np.abs(inp["w2s"][:3, 3]).min() > 0 and np.abs(inp["w2s"][:3, :3]).min() > 1e-3
    for k in ("o", "d", "near", "far"):
        assert _ratio(got[k], ref[k], bound[k], "transform_rays R %d %s" % (R, k)) <= 1.0


@pytest.mark.parametrize("R", tr.STATS_R)
def test_frame_stats_plain_fp32_attains_the_bounds(R):
    inp = tr.stats_inputs(R)
    ref, bound = tr.frame_stats_ref(inp["counter"], inp["alpha"], tr.STATS_PRE)
    got = tr.frame_stats_fp32(inp["counter"], inp["alpha"], tr.STATS_PRE)
    assert (inp["alpha"] == 0.5).any() and (R < 4 or np.isnan(inp["alpha"]).any())
    assert _ratio(got, ref, bound, "frame_stats R %d" % R) <= 1.0
    # counting 0.5 or NaN as covered is seen
    wrong = ref[1] - tr.STATS_PRE[1] + float(((inp["alpha"] == 0.5) | np.isnan(inp["alpha"])).mean())
    assert abs(wrong - (ref[1] - tr.STATS_PRE[1])) > bound[1]
