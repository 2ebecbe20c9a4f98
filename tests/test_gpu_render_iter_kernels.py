"""The four kernels of ia_render_test's wave-front loop, each called alone through the C ABI (ia_render_init_rays,
ia_render_march_compact, ia_render_composite_compact, ia_render_finalize) on seeded host-built inputs
(tests/render_iter_refs.py; no model, no world):

  march       BIT FOR BIT against the plain reference loop, on eleven schedules (N_step 1 ... 9, max_samples, max_batch < n_alive,
              k_before >= max_samples) x eleven occupancy grids x four routes (G = 64 from LDS, the same bits 4 bytes off 16-byte
              alignment from memory, G = 32, G = 16), tails from ia_occupancy_pack; the exact skip forced off on the interior
              grids; the two searched sets (near == t_hi, |o| = 1000); sample_cap; a repeated call
  composite   float64 with bounds, and bit for bit against ia_candidate_max -> ia_composite_test on the same samples
  chain       three iterations march -> composite -> next alive
  init / finalize   bit for bit; arguments

tests/test_cpu_render_iter_refs.py shows on the same inputs that a numpy restatement of the kernels equals the references and
which one-line mutants the comparisons reject.  Each bounded check prints the worst error / bound ("RATIO ...", NOTES.md)."""
import numpy as np
import pytest
import torch

import render_iter_refs as rr
from train_step_refs import F, MARCH_AABB

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_NAMES = [c[0] for c in rr.CASES]


def _dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _lib():
    from instantavatar_amd import _lib as L
    return L


_BITS = {}
_AABB = []


def _aabb():
    if not _AABB:
        _AABB.append(_dev(MARCH_AABB.astype(F).reshape(6)))
    return _AABB[0]


def _bits(G, grid, route="aligned", flag=None):
    """the bit grid of (G, grid) from ia_occupancy_pack (its tails checked against the numpy tails); route 'offset': the same
    words at an address 4 bytes behind a 16-byte boundary; flag: the border flag overwritten"""
    key = (G, grid, route, flag)
    if key not in _BITS:
        occ = rr.iter_occupancy(G, grid)
        n_words = G ** 3 // 32
        bits = torch.zeros(n_words + 8, dtype=torch.int32, device=DEV)
        _lib().call("ia_occupancy_pack", _dev(occ.astype(np.uint8).reshape(-1)), G, bits)
        torch.cuda.synchronize()
        got = _np(bits)
        want = rr.pack_with_tail(occ)
        assert np.array_equal(got[:n_words], want[:n_words]), ("bit words", G, grid)
        assert np.array_equal(got[n_words:n_words + 7], want[n_words:n_words + 7]), ("tail words", G, grid, got[n_words:].tolist(), want[n_words:].tolist())
        assert bits.data_ptr() % 16 == 0
        if flag is not None:
            bits = bits.clone()
            bits[n_words] = flag
        if route == "offset":
            buf = torch.zeros(n_words + 8 + 4, dtype=torch.int32, device=DEV)
            buf[1:1 + n_words + 8] = bits
            bits = buf[1:1 + n_words + 8]
            assert bits.data_ptr() % 16 == 4 and bits.is_contiguous()
        _BITS[key] = bits
    return _BITS[key]


def _state0(inp):
    return np.array([[inp["n_alive"], 0, 0, inp["k_before"], inp["iters0"], 0, 0, 0], rr.STATE1_PRE], np.int32)


def _march(inp, bits, size, cap):
    """one call of ia_render_march_compact into sentinel-filled buffers; returns the outputs as numpy (and the device tensors)"""
    R = inp["R"]
    t = dict(o=_dev(inp["o"]), d=_dev(inp["d"]), near_w=_dev(inp.get("near_w", inp["near"])), far=_dev(inp["far"]), step=_dev(inp["step"]),
             alive=_dev(inp["alive"]), state=_dev(_state0(inp)), s_pts=torch.full((size, 3), float(rr.SENT_F), device=DEV),
             s_t=torch.full((size,), float(rr.SENT_F), device=DEV), ray_off=torch.full((R,), int(rr.SENT_I), dtype=torch.int32, device=DEV),
             ray_cnt=torch.full((R,), int(rr.SENT_I), dtype=torch.int32, device=DEV), counter=_dev(inp["counter0"]))
    assert inp["n_alive"] <= R and cap <= size and len(inp["alive"]) == R and int(inp["alive"].max()) < R
    _lib().call("ia_render_march_compact", t["o"], t["d"], t["near_w"], t["far"], t["step"], t["alive"], R, bits, inp["G"], _aabb(), t["state"],
                t["s_pts"], t["s_t"], t["ray_off"], t["ray_cnt"], t["counter"], cap, inp["max_samples"], inp["max_batch"])
    torch.cuda.synchronize()
    return {k: _np(t[k]) for k in ("s_pts", "s_t", "ray_off", "ray_cnt", "near_w", "counter", "state")}, t


def _check_march(inp, ref, bits, what):
    size = ref["n_samples"] + 64
    got, _ = _march(inp, bits, size, size)
    try:
        rr.march_iter_compare(got, ref, inp)
    except AssertionError as e:
        raise AssertionError((what,) + e.args) from None
    return got


@pytest.mark.parametrize("case", CASE_NAMES)
def test_march_compact_bit_for_bit_every_route(case):
    n_sets = n_total = 0
    for grid in rr.GRIDS:
        for G in rr.GS:
            inp = rr.iter_inputs(case, G, grid)
            ref = rr.march_iter_ref(inp)
            assert ref["n_step"] == rr.CASE_NSTEP[case]
            _check_march(inp, ref, _bits(G, grid), "%s G %d %s" % (case, G, grid))
            n_sets += 1
            n_total += ref["n_samples"]
            if G == 64:
                _check_march(inp, ref, _bits(G, grid, "offset"), "%s G 64 %s, bits off alignment (global route)" % (case, grid))
            if grid in rr.INTERIOR_GRIDS:        # the exact skip off: the same result
                _check_march(inp, ref, _bits(G, grid, flag=0), "%s G %d %s, flag forced 0" % (case, G, grid))
    assert n_sets == len(rr.GRIDS) * len(rr.GS) and (n_total > 0) == (case != "done")
    if case == "done":                           # nothing processed, nothing written (march_iter_compare: every buffer keeps its sentinel)
        assert ref["n_eff"] == 0


@pytest.mark.parametrize("which", ["stage", "margin"])
def test_march_compact_searched_sets(which):
    inp = rr.special_inputs(which)
    ref = rr.march_iter_ref(inp)
    for route in ("aligned", "offset"):
        _check_march(inp, ref, _bits(64, "block", route), "%s %s" % (which, route))


def test_march_compact_sample_cap_and_repeat():
    inp = rr.iter_inputs("n9", 64, "block")
    ref = rr.march_iter_ref(inp)
    total = ref["n_samples"]
    assert total > 400
    bits = _bits(64, "block")
    a, _ = _march(inp, bits, total, total)
    rr.march_iter_compare(a, ref, inp, sample_cap=total)
    # half the capacity: n_samples and the counts are complete, positions below the cap hold their samples, nothing at or past it
    cap = total // 2
    got, _ = _march(inp, bits, total, cap)
    rr.march_iter_compare(got, ref, inp, sample_cap=cap)
    assert (got["s_t"][cap:] == rr.SENT_F).all() and (got["s_pts"][cap:] == rr.SENT_F).all() and (got["s_t"][:cap] != rr.SENT_F).all()
    assert got["state"][0, 1] == total
    # a repeated call: the same bits up to the waves' permutation, which the ranges undo
    b, _ = _march(inp, bits, total, total)
    rr.march_iter_compare(b, ref, inp)
    for k in ("ray_cnt", "near_w", "counter", "state"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    na = ref["n_eff"]
    for i in np.nonzero(a["ray_cnt"][:na] > 0)[0][::7]:
        c = a["ray_cnt"][i]
        assert np.array_equal(a["s_t"][a["ray_off"][i]:a["ray_off"][i] + c].view(np.uint32), b["s_t"][b["ray_off"][i]:b["ray_off"][i] + c].view(np.uint32))


# ---- compositor ------------------------------------------------------------------------------------------------------
def _composite(cs, march=None, layout=None, prior=None):
    """one call of ia_render_composite_compact on the samples of `march` laid out as `layout` (ray_off per alive slot; default:
    alive order); returns color, depth, T, alive_next, n_next (numpy) and the candidate tables on the device in that layout"""
    L = _lib()
    inp = cs["inp"]
    march = cs["march"] if march is None else march
    na, N, R, P = march["n_eff"], march["n_step"], inp["R"], march["n_samples"]
    off = march["ray_start"] if layout is None else np.asarray(layout, np.int64)[:na]
    cnt = march["ray_cnt"][:na].astype(np.int64)
    slot = np.repeat(np.arange(na), cnt)
    pos = off[slot] + (np.arange(P) - march["ray_start"][slot])
    size = P + 8
    s_t, pt_off, pt_cnt = np.full(size, rr.SENT_F, F), np.zeros(size, np.int32), np.zeros(size, np.uint8)
    s_t[pos], pt_off[pos], pt_cnt[pos] = march["s_t"], cs["pt_off"], cs["pt_cnt"]
    ray_off, ray_cnt = np.full(R, rr.SENT_I, np.int32), np.full(R, rr.SENT_I, np.int32)
    ray_off[:na], ray_cnt[:na] = off, cnt
    C = len(cs["cand_sigma"])
    sig, col = np.zeros(C + 8, F), np.zeros((C + 8, 3), F)
    sig[:C], col[:C] = cs["cand_sigma"], cs["cand_rgb"]
    state = np.array([[inp["n_alive"], P, 0, inp["k_before"], inp["iters0"], N, na, 0], [0] * 8], np.int32)
    prior = prior or dict(color=cs["color0"], depth=cs["depth0"], T=cs["T0"])
    t = dict(alive=_dev(inp["alive"]), nxt=torch.full((R,), int(rr.SENT_I), dtype=torch.int32, device=DEV), state=_dev(state), ray_off=_dev(ray_off),
             ray_cnt=_dev(ray_cnt), s_t=_dev(s_t), step=_dev(inp["step"]), pt_off=_dev(pt_off), pt_cnt=_dev(pt_cnt), col=_dev(col), sig=_dev(sig),
             color=_dev(prior["color"]), depth=_dev(prior["depth"]), T=_dev(prior["T"]))
    assert na <= R and (pos < size).all() and (cs["pt_off"].astype(np.int64) + cs["pt_cnt"] <= C).all()
    L.call("ia_render_composite_compact", t["alive"], t["nxt"], t["state"], t["ray_off"], t["ray_cnt"], t["s_t"], t["step"], t["pt_off"], t["pt_cnt"],
           t["col"], t["sig"], cs["n_init"], R, t["color"], t["depth"], t["T"], cs["thresh"])
    torch.cuda.synchronize()
    st = _np(t["state"])
    assert np.array_equal(st[0], state[0]) and (st[1, 1:] == 0).all(), ("state", st.tolist())
    return dict(color=_np(t["color"]), depth=_np(t["depth"]), T=_np(t["T"]), alive_next=_np(t["nxt"]), n_next=int(st[1, 0])), t, pos


def _dense_pair(cs, t, pos, prior=None):
    """ia_candidate_max -> ia_composite_test on the same samples in the dense layout"""
    L = _lib()
    inp, march = cs["inp"], cs["march"]
    na, N, P = march["n_eff"], march["n_step"], march["n_samples"]
    size = t["s_t"].numel()
    rgb, sig = torch.zeros((size, 3), device=DEV), torch.zeros(size, device=DEV)
    L.call("ia_candidate_max", t["col"], t["sig"], t["pt_off"], t["pt_cnt"], size, None, cs["n_init"], 0.0, 1, rgb, sig)
    torch.cuda.synchronize()
    d_rgb, d_sig, d_delta, d_depth = rr.dense_layout(cs, _np(sig)[pos], _np(rgb)[pos])
    prior = prior or dict(color=cs["color0"], depth=cs["depth0"], T=cs["T0"])
    color, depth, T = _dev(prior["color"]), _dev(prior["depth"]), _dev(prior["T"])
    L.call("ia_composite_test", _dev(d_rgb), _dev(d_sig), _dev(d_delta), _dev(d_depth), _dev(inp["alive"][:na].astype(np.int64)), na, N, color, depth, T,
           cs["thresh"])
    torch.cuda.synchronize()
    return dict(color=_np(color), depth=_np(depth), T=_np(T)), d_depth


COMPOSITE_SETS = [(case, 64, grid, n_init, th) for case in CASE_NAMES for grid in ("block", "full", "rand3")
                  for n_init, th in ((1, rr.THRESH), (13, rr.THRESH), (13, -0.5))]


@pytest.mark.parametrize("case", CASE_NAMES)
def test_composite_compact_float64_and_dense_pair(case):
    worst = {}
    for cset in [s for s in COMPOSITE_SETS if s[0] == case]:
        cs = rr.composite_inputs(*cset)
        ref = rr.composite_ref(cs)
        march = cs["march"]
        na = march["n_eff"]
        # the ranges of the waves in reverse order: a layout the atomics may produce, and not the reference's own
        cnt = march["ray_cnt"][:na].astype(np.int64)
        wave_tot = np.add.reduceat(cnt, np.arange(0, na, rr.WAVE)) if na else np.zeros(0, np.int64)
        base = (np.cumsum(wave_tot[::-1]) - wave_tot[::-1])[::-1]
        layout = np.concatenate([base[w] + np.cumsum(cnt[w * 64:(w + 1) * 64]) - cnt[w * 64:(w + 1) * 64] for w in range(len(wave_tot))]) if na else cnt
        got, t, pos = _composite(cs, layout=layout)
        w = rr.composite_compare(got, ref, cs, "composite %s G %d %s n_init %d thresh %.2f" % cset)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if na:
            dense, d_depth = _dense_pair(cs, t, pos)
            for k in ("color", "depth", "T"):
                assert np.array_equal(got[k].view(np.uint32), dense[k].view(np.uint32)), (cset, k, "differs from ia_candidate_max -> ia_composite_test")
            ray = cs["inp"]["alive"][:na]
            keep = (dense["T"][ray].astype(np.float64) > 1e-4) & (d_depth[:, -1] > 0)
            assert sorted(got["alive_next"][:got["n_next"]].tolist()) == sorted(ray[keep].tolist()), (cset, "survivors differ from the dense rule")
        # a repeated call: the same bits
        again, _, _ = _composite(cs, layout=layout)
        for k in ("color", "depth", "T"):
            assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), (cset, k, "not repeatable")
        assert sorted(got["alive_next"][:got["n_next"]].tolist()) == sorted(again["alive_next"][:again["n_next"]].tolist())
    print("RATIO composite %-43s %s" % (case, " ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_three_chained_iterations():
    """march -> composite -> next alive, three times, every buffer handed on by the kernels themselves; the reference loop runs
    beside it in float64 on the kernel's own alive order (checked first), its bounds growing with the errors it inherits"""
    L = _lib()
    G, grid, R, ms, mb, n_init = 64, "block", 300, 64, 257 * 3, 13
    r = rr.iter_rays(ms, R, G, grid)
    alive = np.random.default_rng(11).permutation(R).astype(np.int32)
    inp = dict(r, occ=rr.iter_occupancy(G, grid), G=G, grid=grid, alive=alive, n_alive=257, R=R, max_samples=ms, max_batch=mb, k_before=0,
               counter0=np.zeros(R, F), iters0=0, case="chain")
    bits = _bits(G, grid)
    state = torch.zeros((8, 8), dtype=torch.int32, device=DEV)
    state[0, 0] = 257
    dev = dict(near_w=_dev(r["near"]), counter=torch.zeros(R, device=DEV))
    color, depth, T = torch.zeros((R, 3), device=DEV), torch.zeros(R, device=DEV), torch.ones(R, device=DEV)
    ref_prior, bound_prior = dict(color=np.zeros((R, 3)), depth=np.zeros(R), T=np.ones(R)), None
    cur = _dev(alive)
    n_steps = []
    for it in range(3):
        na, N = rr.schedule(inp["n_alive"], inp["k_before"], ms, mb)
        assert na > 0, "the chain ran out of rays"
        ref_m = rr.march_iter_ref(inp)
        size = ref_m["n_samples"] + 64
        t = dict(o=_dev(inp["o"]), d=_dev(inp["d"]), far=_dev(inp["far"]), step=_dev(inp["step"]), s_pts=torch.full((size, 3), float(rr.SENT_F), device=DEV),
                 s_t=torch.full((size,), float(rr.SENT_F), device=DEV), ray_off=torch.full((R,), int(rr.SENT_I), dtype=torch.int32, device=DEV),
                 ray_cnt=torch.full((R,), int(rr.SENT_I), dtype=torch.int32, device=DEV))
        st = state[it:it + 2]
        L.call("ia_render_march_compact", t["o"], t["d"], dev["near_w"], t["far"], t["step"], cur, R, bits, G, _aabb(), st.view(-1), t["s_pts"], t["s_t"],
               t["ray_off"], t["ray_cnt"], dev["counter"], size, ms, mb)
        torch.cuda.synchronize()
        got_m = dict(s_pts=_np(t["s_pts"]), s_t=_np(t["s_t"]), ray_off=_np(t["ray_off"]), ray_cnt=_np(t["ray_cnt"]), near_w=_np(dev["near_w"]),
                     counter=_np(dev["counter"]))
        got_state = _np(st)
        want = ref_m["state"].copy()
        want[1] = [0, 0, 0, want[1, 3], want[1, 4], 0, 0, 0]
        got_m["state"], ref_m["state"] = got_state, want
        rr.march_iter_compare(got_m, ref_m, inp)
        n_steps.append(N)
        # candidates of this iteration's samples, in the kernel's compact layout
        cs = rr.composite_tables(inp, ref_m, n_init, rr.THRESH, 4000 + it, fresh=True, kill_rate=0.02)
        P = ref_m["n_samples"]
        cnt = ref_m["ray_cnt"][:na].astype(np.int64)
        slot = np.repeat(np.arange(na), cnt)
        pos = got_m["ray_off"][:na].astype(np.int64)[slot] + (np.arange(P) - ref_m["ray_start"][slot])
        pt_off, pt_cnt = np.zeros(size, np.int32), np.zeros(size, np.uint8)
        pt_off[pos], pt_cnt[pos] = cs["pt_off"], cs["pt_cnt"]
        C = len(cs["cand_sigma"])
        sig, col = np.zeros(C + 8, F), np.zeros((C + 8, 3), F)
        sig[:C], col[:C] = cs["cand_sigma"], cs["cand_rgb"]
        nxt = torch.full((R,), int(rr.SENT_I), dtype=torch.int32, device=DEV)
        before = dict(prior_color=_np(color).copy(), prior_depth=_np(depth).copy(), prior_T=_np(T).copy())
        L.call("ia_render_composite_compact", cur, nxt, st.view(-1), t["ray_off"], t["ray_cnt"], t["s_t"], t["step"], _dev(pt_off), _dev(pt_cnt), _dev(col),
               _dev(sig), n_init, R, color, depth, T, rr.THRESH)
        torch.cuda.synchronize()
        ref_c = rr.composite_ref(cs, T0=ref_prior["T"], color0=ref_prior["color"], depth0=ref_prior["depth"], prior=bound_prior)
        assert not ref_c["undecidable"].any(), "a ray of the chain sits on a threshold"
        n_next = int(state[it + 1, 0].item())
        got_c = dict(color=_np(color), depth=_np(depth), T=_np(T), alive_next=_np(nxt), n_next=n_next)
        ref_c.update(before)                     # (rays that are not processed keep the bits the chain gave them, not the set's priors)
        rr.composite_compare(got_c, ref_c, cs, "chain iteration %d (N_step %d, %d rays)" % (it, N, na))
        ref_prior = dict(color=ref_c["color"], depth=ref_c["depth"], T=ref_c["T"])
        bound_prior = dict(b_color=ref_c["b_color"], b_depth=ref_c["b_depth"], rel_T=ref_c["rel_T"])
        nxt_np = got_c["alive_next"].copy()
        rest = np.setdiff1d(np.arange(R, dtype=np.int32), nxt_np[:n_next])
        nxt_np[n_next:] = rest                   # (the slots behind the alive rays: other rays, untouched)
        inp = dict(inp, alive=nxt_np, n_alive=n_next, k_before=inp["k_before"] + N, near_w=ref_m["near_w"], counter0=ref_m["counter"],
                   iters0=inp["iters0"] + 1)
        cur = _dev(nxt_np)
    assert len(set(n_steps)) > 1, n_steps       # the schedule moved as rays died
    final = _np(state)
    assert final[3, 3] == sum(n_steps) and final[3, 4] == 3


# ---- init, finalize, arguments ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 255, 256, 257, 513])
def test_init_rays_and_finalize_bit_for_bit(R):
    L = _lib()
    rng = np.random.default_rng(R)
    near, far = rng.uniform(0.5, 3, R).astype(F), rng.uniform(2, 5, R).astype(F)
    if R > 4:
        near[1], far[2], far[3] = np.nan, np.nan, near[3]
    ms = 37
    ref = rr.init_rays_ref(near, far, ms)
    bufs = dict(near_w=torch.full((R,), 5.0, device=DEV), step=torch.full((R,), 5.0, device=DEV), color=torch.full((R, 3), 5.0, device=DEV),
                depth=torch.full((R,), 5.0, device=DEV), nohit=torch.full((R,), 5.0, device=DEV), counter=torch.full((R,), 5.0, device=DEV),
                alive=torch.full((R,), 5, dtype=torch.int32, device=DEV))
    state = torch.full((1024 * 8 + 8,), 9, dtype=torch.int32, device=DEV)
    L.call("ia_render_init_rays", R, _dev(near), _dev(far), bufs["near_w"], bufs["step"], bufs["color"], bufs["depth"], bufs["nohit"], bufs["counter"],
           bufs["alive"], ms, state)
    torch.cuda.synchronize()
    for k, v in bufs.items():
        g = _np(v)
        if k == "step":                          # (the bits of a NaN quotient are the hardware's choice: NaN where NaN is due)
            assert np.array_equal(np.isnan(g), np.isnan(ref[k])) and np.isnan(g).sum() == (2 if R > 4 else 0)
            g = np.where(np.isnan(g), ref[k], g)
        assert np.array_equal(g.view(np.uint32), ref[k].view(np.uint32)), k
    st = _np(state)
    assert st[0] == R and (st[1:1024 * 8] == 0).all() and (st[1024 * 8:] == 9).all()
    # finalize: with bg and without, the n_alive_out rule on both sides of k_before == max_samples
    color, depth = rng.random((R, 3)).astype(F), rng.random(R).astype(F)
    nohit, counter, bg = rng.random(R).astype(F), rng.integers(0, 99, R).astype(F), rng.random((R, 3)).astype(F)
    nohit[0] = 1.0
    for bgv in (None, bg):
        for st_end in ([7, 1, 2, ms - 1, 4, 5, 6, 0], [7, 1, 2, ms, 4, 5, 6, 0], [0, 0, 0, 3, 9, 0, 0, 0]):
            want = rr.finalize_ref(color, depth, nohit, counter, bgv, st_end, ms)
            out = dict(rgb=torch.full((R, 3), 5.0, device=DEV), depth=torch.full((R,), 5.0, device=DEV), alpha=torch.full((R,), 5.0, device=DEV),
                       counter=torch.full((R,), 5.0, device=DEV), n_alive_out=torch.full((2,), 5, dtype=torch.int32, device=DEV))
            L.call("ia_render_finalize", R, _dev(color), _dev(depth), _dev(nohit), _dev(counter), None if bgv is None else _dev(bgv),
                   _dev(np.array(st_end, np.int32)), ms, out["n_alive_out"], out["rgb"], out["depth"], out["alpha"], out["counter"])
            torch.cuda.synchronize()
            for k, v in out.items():
                assert np.array_equal(_np(v).view(np.uint32), want[k].view(np.uint32)), (k, bgv is None, st_end)
    # n_alive_out may be NULL
    L.call("ia_render_finalize", R, _dev(color), _dev(depth), _dev(nohit), _dev(counter), None, _dev(np.zeros(8, np.int32)), ms, None, out["rgb"], out["depth"],
           out["alpha"], out["counter"])
    torch.cuda.synchronize()


def test_the_entries_refuse_bad_arguments():
    L = _lib()
    R = 8
    f = lambda *s: torch.full(s, 5.0, device=DEV)
    i = lambda *s: torch.full(s, 5, dtype=torch.int32, device=DEV)
    bits = _bits(16, "block")
    bufs = [f(R), f(R), f(R, 3), f(R), f(R), f(R), i(R), i(16), f(64, 3), f(64), i(R), i(R), torch.full((64,), 5, dtype=torch.uint8, device=DEV)]
    near_w, step, color, depth, nohit, counter, alive, state, s_pts, s_t, ray_off, ray_cnt, pt_cnt = bufs
    calls = [
        ("ia_render_init_rays: bad sizes", ("ia_render_init_rays", 0, near_w, near_w, near_w, step, color, depth, nohit, counter, alive, 4, state)),
        ("ia_render_init_rays: bad sizes", ("ia_render_init_rays", R, near_w, near_w, near_w, step, color, depth, nohit, counter, alive, 0, state)),
        ("ia_render_init_rays: null pointer", ("ia_render_init_rays", R, near_w, near_w, near_w, step, color, depth, nohit, counter, alive, 4, None)),
        ("ia_render_march_compact: bad sizes", ("ia_render_march_compact", color, color, near_w, step, step, alive, R, bits, 16, _aabb(), state, s_pts, s_t,
                                                ray_off, ray_cnt, counter, 64, 0, 8)),
        ("ia_render_march_compact: bad sizes", ("ia_render_march_compact", color, color, near_w, step, step, alive, R, bits, 16, _aabb(), state, s_pts, s_t,
                                                ray_off, ray_cnt, counter, -1, 4, 8)),
        ("ia_render_march_compact: unsupported G", ("ia_render_march_compact", color, color, near_w, step, step, alive, R, bits, 6, _aabb(), state, s_pts,
                                                    s_t, ray_off, ray_cnt, counter, 64, 4, 8)),
        ("ia_render_march_compact: null pointer", ("ia_render_march_compact", color, color, near_w, step, step, alive, R, None, 16, _aabb(), state, s_pts,
                                                   s_t, ray_off, ray_cnt, counter, 64, 4, 8)),
        ("ia_render_march_compact: occ_bits must be 4-byte aligned", ("ia_render_march_compact", color, color, near_w, step, step, alive, R,
                                                                      bits.data_ptr() + 2, 16, _aabb(), state, s_pts, s_t, ray_off, ray_cnt, counter, 64, 4, 8)),
        ("ia_render_composite_compact: bad sizes", ("ia_render_composite_compact", alive, alive, state, ray_off, ray_cnt, s_t, step, ray_off, pt_cnt, s_pts,
                                                    s_t, 0, R, color, depth, nohit, 0.01)),
        ("ia_render_composite_compact: null pointer", ("ia_render_composite_compact", alive, alive, state, ray_off, ray_cnt, s_t, step, ray_off, None, s_pts,
                                                       s_t, 1, R, color, depth, nohit, 0.01)),
        ("ia_render_finalize: bad sizes", ("ia_render_finalize", 0, color, depth, nohit, counter, None, state, 4, None, color, depth, nohit, counter)),
        ("ia_render_finalize: null pointer", ("ia_render_finalize", R, color, depth, nohit, counter, None, None, 4, None, color, depth, nohit, counter)),
    ]
    for msg, c in calls:
        with pytest.raises(L.IAError, match=msg):
            L.call(*c)
        assert msg.split(":")[0].encode() in L.lib().ia_last_error()
    torch.cuda.synchronize()
    assert all((_np(b) == 5).all() for b in bufs), "something was launched"
