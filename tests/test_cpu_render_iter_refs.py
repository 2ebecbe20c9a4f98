"""tests/render_iter_refs.py on the CPU: what the references of the inference wave-front loop are worth, shown without a GPU.

On every input set (eleven schedules x three grid sizes x eleven occupancy grids, and the two searched sets):
  * the march reference equals the oracle's `orc_raymarch_test` (depths, positions and near bit for bit),
  * the numpy restatement of k_march_compact (`march_iter_emulated`, LDS and global route) equals the reference under
    `march_iter_compare`, the comparison the GPU test makes,
  * every mutant of MARCH_MUTANTS is rejected by that comparison on at least one set (the sets that kill it are counted), and
    the three changes that provably cannot alter an output (MARCH_EQUIVALENT) are shown to pass on every set;
for the compositor
  * the float64 reference agrees with the oracle's `orc_candidate_max` -> `orc_composite_test` inside its bound,
  * plain float32 compositing in the kernel's order (`composite_emulated`) stays inside the bound,
  * the reference alone leaves at most 2 % of a set's rays undecidable,
  * every mutant of COMPOSITE_MUTANTS is rejected by `composite_compare`."""
import ctypes as C

import numpy as np
import pytest

import render_iter_refs as rr
from train_step_refs import F, MARCH_AABB

CASE_NAMES = [c[0] for c in rr.CASES]
_KILLS = {}


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _oracle_march(orc, inp, tab):
    """orc_raymarch_test on the rays of a set that have a positive step (the reference loop does not end on the others)"""
    na, N = tab["n_eff"], tab["n_step"]
    with np.errstate(invalid="ignore"):
        sel = np.nonzero(tab["dt"] > 0)[0]
    alive = np.ascontiguousarray(tab["ray"][sel], np.int64)
    o, d = np.ascontiguousarray(inp["o"], F), np.ascontiguousarray(inp["d"], F)
    near, far, step = np.array(inp["near"], F), np.ascontiguousarray(inp["far"], F), np.ascontiguousarray(inp["step"], F)
    aabb = MARCH_AABB.astype(F)
    offset, scale = np.ascontiguousarray(aabb[0]), np.ascontiguousarray(aabb[1] - aabb[0])
    occ8 = np.ascontiguousarray(inp["occ"], np.uint8)
    n = len(alive)
    pts, dl, z = np.zeros((n, max(N, 1), 3), F), np.zeros((n, max(N, 1)), F), np.zeros((n, max(N, 1)), F)
    if n and N:
        orc.lib().orc_raymarch_test(_p(o), _p(d), _p(near), _p(far), _p(alive), C.c_long(n), _p(occ8), int(inp["G"]), _p(scale), _p(offset),
                                    _p(step), int(N), _p(pts), _p(dl), _p(z))
    return sel, pts, dl, z, near


def _check_against_oracle(orc, inp, tab, ref):
    sel, pts, dl, z, near = _oracle_march(orc, inp, tab)
    na = tab["n_eff"]
    assert np.array_equal(near.view(np.uint32), ref["near_w"].view(np.uint32)), "near after the march"
    cnt = ref["ray_cnt"][:na]
    assert np.array_equal((dl > 0).sum(1) if tab["n_step"] else np.zeros(len(sel), int), cnt[sel])
    with np.errstate(invalid="ignore"):
        assert (cnt[~(tab["dt"] > 0)] == 0).all()
    for i, s in enumerate(sel):
        a, c = ref["ray_start"][s], cnt[s]
        assert np.array_equal(z[i, :c].view(np.uint32), ref["s_t"][a:a + c].view(np.uint32))
        assert np.array_equal(pts[i, :c].view(np.uint32), ref["s_pts"][a:a + c].view(np.uint32))
        assert (dl[i, :c] == inp["step"][tab["ray"][s]]).all()


def _rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", CASE_NAMES)
def test_march_reference_oracle_emulation_and_mutants(oracle, case):
    for G in rr.GS:
        for grid in rr.GRIDS:
            inp = rr.iter_inputs(case, G, grid)
            tab = rr.step_table(inp)
            ref = rr.march_iter_ref(inp, tab)
            assert (ref["n_eff"], ref["n_step"]) == rr.schedule(inp["n_alive"], inp["k_before"], inp["max_samples"], inp["max_batch"])
            assert ref["n_step"] == rr.CASE_NSTEP[case]
            _check_against_oracle(oracle, inp, tab, ref)
            for lds in (True, False):
                rr.march_iter_compare(rr.march_iter_emulated(inp, tab, lds=lds), ref, inp)
            for m in rr.MARCH_MUTANTS:
                if _rejected(lambda: rr.march_iter_compare(rr.march_iter_emulated(inp, tab, m), ref, inp)):
                    _KILLS.setdefault(m, []).append((case, G, grid))
            for m in rr.MARCH_EQUIVALENT:
                rr.march_iter_compare(rr.march_iter_emulated(inp, tab, m), ref, inp)
    if case == "done":
        assert ref["n_samples"] == 0 and ref["n_eff"] == 0


@pytest.mark.parametrize("which", ["stage", "margin"])
def test_march_searched_sets(oracle, which):
    inp = rr.special_inputs(which)
    tab = rr.step_table(inp)
    ref = rr.march_iter_ref(inp, tab)
    _check_against_oracle(oracle, inp, tab, ref)
    for lds in (True, False):
        rr.march_iter_compare(rr.march_iter_emulated(inp, tab, lds=lds), ref, inp)
    killer = dict(stage="stage_lt", margin="margin0")[which]
    assert _rejected(lambda: rr.march_iter_compare(rr.march_iter_emulated(inp, tab, killer), ref, inp)), killer
    _KILLS.setdefault(killer, []).append((which,))
    for m in rr.MARCH_EQUIVALENT:
        rr.march_iter_compare(rr.march_iter_emulated(inp, tab, m), ref, inp)


def test_every_march_mutant_is_rejected(oracle):
    """(runs behind the two tests above: they fill the table)"""
    if not _KILLS:
        for case in ("n5", "n7"):
            test_march_reference_oracle_emulation_and_mutants(oracle, case)
        for which in ("stage", "margin"):
            test_march_searched_sets(oracle, which)
    for m in rr.MARCH_MUTANTS:
        print("KILLED %-18s on %d sets, e.g. %s" % (m, len(_KILLS.get(m, [])), _KILLS.get(m, [None])[0]))
    assert all(_KILLS.get(m) for m in rr.MARCH_MUTANTS), {m: len(_KILLS.get(m, [])) for m in rr.MARCH_MUTANTS}


def test_ray_sets_hold_every_kind():
    r = rr.iter_rays(64, 130, 64, "block")
    assert set(rr.EXTRA_KINDS) <= set(r["kinds"]) and {"miss", "lt", "eq", "nan_near", "nan_far", "large", "fmaedge", "inner"} <= set(r["kinds"])
    inp = rr.iter_inputs("n5", 64, "block")
    assert not np.array_equal(inp["alive"][:65], np.arange(65)) and len(set(inp["alive"].tolist())) == inp["R"]
    assert sorted(set(rr.CASE_NSTEP.values())) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert sorted(c[1] for c in rr.CASES if c[0].startswith("n") and c[0] != "nms") == [1, 3, 63, 64, 65, 200, 257, 513]
    for G in rr.GS:
        for grid in rr.GRIDS:
            t = rr.tail_words(rr.iter_occupancy(G, grid)).view(np.int32)
            assert (t[0] == 1) == (grid in rr.INTERIOR_GRIDS + ("empty",)), (G, grid)
            assert (t[1] > t[2]) == (grid == "empty")


# ---- compositor ------------------------------------------------------------------------------------------------------
COMPOSITE_SETS = [(case, 64, grid, n_init, th) for case in CASE_NAMES for grid in ("block", "full", "rand3")
                  for n_init, th in ((1, rr.THRESH), (13, rr.THRESH), (13, -0.5))]


def _oracle_composite(orc, cs):
    """orc_candidate_max (fill 0, nan_to_num) -> orc_composite_test on the dense layout of the set's samples"""
    inp, march, n_init = cs["inp"], cs["march"], cs["n_init"]
    P = march["n_samples"]
    pc, po = cs["pt_cnt"].astype(np.int64), cs["pt_off"].astype(np.int64)
    rgb_c, sig_c, valid = np.zeros((P, n_init, 3), F), np.zeros((P, n_init), F), np.zeros((P, n_init), np.uint8)
    for c in range(n_init):                      # valid candidates sit in the leading slots (the order of the compact lists)
        on = c < pc
        valid[on, c] = 1
        sig_c[on, c], rgb_c[on, c] = cs["cand_sigma"][po[on] + c], cs["cand_rgb"][po[on] + c]
    rgb, sig = np.zeros((max(P, 1), 3), F), np.zeros(max(P, 1), F)
    if P:
        orc.lib().orc_candidate_max(_p(rgb_c), _p(sig_c), _p(valid), C.c_long(P), int(n_init), C.c_float(0.0), 1, _p(rgb), _p(sig))
    d_rgb, d_sig, d_delta, d_depth = rr.dense_layout(cs, sig[:P], rgb[:P])
    na, N = march["n_eff"], march["n_step"]
    color, depth, T = np.array(cs["color0"], F), np.array(cs["depth0"], F), np.array(cs["T0"], F)
    alive = np.ascontiguousarray(inp["alive"][:na], np.int64)
    if na:
        orc.lib().orc_composite_test(_p(d_rgb), _p(d_sig), _p(d_delta), _p(d_depth), _p(alive), C.c_long(na), int(N), _p(color), _p(depth), _p(T),
                                     C.c_float(cs["thresh"]))
    last = d_depth[:, -1] if na else np.zeros(0, F)
    surv = alive[(T[alive].astype(np.float64) > 1e-4) & (last > 0)].astype(np.int32)      # raymarcher_acc.py:126
    nxt = np.full(inp["R"], rr.SENT_I, np.int32)
    nxt[:len(surv)] = surv
    return dict(color=color, depth=depth, T=T, alive_next=nxt, n_next=len(surv))


@pytest.mark.parametrize("case", CASE_NAMES)
def test_composite_reference_oracle_fp32_and_mutants(oracle, case):
    quiet = lambda *a: None
    for cset in [s for s in COMPOSITE_SETS if s[0] == case]:
        cs = rr.composite_inputs(*cset)
        ref = rr.composite_ref(cs)
        na = ref["n_eff"]
        assert ref["undecidable"].sum() <= rr.MAX_UNDECIDABLE * max(na, 1), (cset, int(ref["undecidable"].sum()))
        w = rr.composite_compare(rr.composite_emulated(cs), ref, cs, "fp32 %s" % (cset,), report=quiet)
        if cs["thresh"] > 0:                     # (the oracle's dense layout marks empty slots by delta = 0 as the kernel does)
            rr.composite_compare(_oracle_composite(oracle, cs), ref, cs, "oracle %s" % (cset,), report=quiet)
        for m in rr.COMPOSITE_MUTANTS:
            if _rejected(lambda: rr.composite_compare(rr.composite_emulated(cs, m), ref, cs, m, report=quiet)):
                _KILLS.setdefault(m, []).append(cset)
        if case == "n9" and cset[2] == "block":
            print("RATIO fp32 emulation %s" % (cset,), w)


def test_every_composite_mutant_is_rejected(oracle):
    if not any(m in _KILLS for m in rr.COMPOSITE_MUTANTS):
        for case in ("n5", "n9", "n3"):
            test_composite_reference_oracle_fp32_and_mutants(oracle, case)
    for m in rr.COMPOSITE_MUTANTS:
        print("KILLED %-18s on %d sets, e.g. %s" % (m, len(_KILLS.get(m, [])), _KILLS.get(m, [None])[0]))
    assert all(_KILLS.get(m) for m in rr.COMPOSITE_MUTANTS), {m: len(_KILLS.get(m, [])) for m in rr.COMPOSITE_MUTANTS}


def test_composite_sets_end_rays_at_every_group_position():
    """the terminating densities land on every position of a trip of four, and on tails m = 1, 2, 3"""
    cs = rr.composite_inputs("n9", 64, "full", 13)
    ref, march = rr.composite_ref(cs), cs["march"]
    cnt = march["ray_cnt"][:march["n_eff"]]
    assert {1, 2, 3, 0} <= set((cnt[cnt > 0] % 4).tolist()) or len(set(cnt.tolist())) > 1
    cs5 = rr.composite_inputs("n5", 64, "block", 13)
    assert {int(c) % 4 for c in cs5["march"]["ray_cnt"][:65] if c > 0} >= {1}
    ended = np.zeros(4, int)
    for kill_pos in range(4):
        ended[kill_pos] = ((cs["slot"] % 10 == kill_pos) & (cs["j"] == kill_pos)).sum()
    assert (ended > 0).all()
    assert ref["keep"].any() and (~ref["keep"]).any()
    assert (cs["pt_cnt"] == 0).any() and (cs["pt_cnt"] == 13).any() and ((cs["pt_cnt"] > 0) & (cs["pt_cnt"] < 13)).any()
    assert np.isnan(cs["cand_sigma"]).any() and np.isinf(cs["cand_sigma"]).any() and (~np.isfinite(cs["cand_rgb"])).any()


def test_init_and_finalize_references():
    near, far = np.array([1.0, 2.0, np.nan], F), np.array([3.0, 1.0, 4.0], F)
    r = rr.init_rays_ref(near, far, 64)
    assert r["step"][0] == F(2.0 / 64) and r["step"][1] < 0 and np.isnan(r["step"][2]) and r["nohit"].tolist() == [1, 1, 1]
    f = rr.finalize_ref(np.zeros((2, 3), F), np.zeros(2, F), np.array([0.25, 1.0], F), np.zeros(2, F), None, [5, 0, 0, 64, 7, 0, 0, 0], 64)
    assert f["n_alive_out"].tolist() == [0, 7] and f["rgb"][0].tolist() == [0.25] * 3 and f["alpha"].tolist() == [0.75, 0.0]
    assert rr.finalize_ref(np.zeros((2, 3), F), np.zeros(2, F), np.ones(2, F), np.zeros(2, F), None, [5, 0, 0, 63, 7, 0, 0, 0], 64)["n_alive_out"].tolist() == [5, 7]


def test_render_iter_header_is_bound():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    import os
    from instantavatar_amd import _lib, build
    d = _lib.declarations("render_iter")
    assert sorted(d) == ["ia_render_composite_compact", "ia_render_finalize", "ia_render_init_rays", "ia_render_march_compact"]
    assert all(v.stream for v in d.values())
    assert [p.name for p in d["ia_render_finalize"].params] == ["R", "color", "depth", "nohit", "counter", "bg", "state_end", "max_samples", "n_alive_out",
                                                                "rgb", "depth_out", "alpha", "counter_out", "stream"]
    assert os.path.normpath(_lib.header_path("render_iter")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    L = _lib.lib()
    assert all(n in _lib._bound for n in d)
    # the argument checks run before anything touches the GPU
    assert L.ia_render_finalize(0, None, None, None, None, None, None, 4, None, None, None, None, None, None) != 0
    assert b"ia_render_finalize: bad sizes" in L.ia_last_error()
    assert L.ia_render_init_rays(4, None, None, None, None, None, None, None, None, None, 4, None, None) != 0
    assert b"ia_render_init_rays: null pointer" in L.ia_last_error()
