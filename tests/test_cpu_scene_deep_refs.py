"""tests/scene_deep_refs.py -- the yardstick of tests/test_gpu_scene_deep.py -- held to facts that can be verified by hand, to the
project's other references (render_iter_refs' dense compositing for K = 1, scene_refs' layered composite on disjoint blocks), and
the conditions the inputs of tests/scene_deep_cases.py must meet for the GPU comparison to mean something; then the binding table of
include/instantavatar_hip_scene_deep.h and what the entry point decides before any launch.  No GPU."""
import math
import os

import numpy as np
import pytest

import render_iter_refs as rir
import scene_deep_cases as cases
import scene_deep_refs as sdr
import scene_refs as sr

F = np.float32


def _case(z, dl, sg, rgb, **kw):
    """lists given as [K][S] python lists for ONE pixel"""
    a = lambda x: np.asarray(x, F)[:, :, None]
    return dict(z=a(z), delta=a(dl), sigma=a(sg), rgb=np.asarray(rgb, F)[:, :, None, :], factor=kw.get("factor"), ground=kw.get("ground"),
                bg=kw.get("bg"), thresh=sdr.THRESH)


def _tau(sg, dl):
    return math.exp(-float(F(sg)) * float(F(dl)))


def test_two_samples_by_hand():
    """B lies in front of A although A is the lower list: C = a_B c_B + tau_B a_A c_A"""
    cA, cB = [0.25, 0.5, 1.0], [1.0, 0.5, 0.125]
    case = _case([[3.0], [2.0]], [[0.5], [0.25]], [[2.0], [4.0]], [[cA], [cB]])
    ref = sdr.deep_ref(case)
    tA, tB = _tau(2.0, 0.5), _tau(4.0, 0.25)
    want = (1 - tB) * np.array(cB) + tB * (1 - tA) * np.array(cA)
    assert np.allclose(ref["rgb"][0], want, rtol=0, atol=1e-15)
    assert abs(ref["depth"][0] - ((1 - tB) * 2.0 + tB * (1 - tA) * 3.0)) <= 1e-15
    assert abs(ref["alpha"][0] - (1 - tA * tB)) <= 1e-15
    assert ref["owners"][0] == [1, 0] and ref["interleaved"] == 0 and not ref["undecidable"][0]
    emu = sdr.deep_emulated(case)
    assert not sdr.differs(emu, ref) and emu["interleaved"] == 0
    assert (ref["b_rgb"] > 0).all() and (ref["b_rgb"] < 1e-6).all()


def test_three_samples_by_hand_interleaved_with_ground_factor_and_background():
    """A B A along the ray, the ground between B and the second A, a factor per list and a background"""
    c = dict(a1=[1.0, 0.0, 0.5], a2=[0.0, 1.0, 0.5], b=[0.5, 0.5, 0.0])
    fac = np.array([[0.5], [0.75]], F)
    ground = (np.array([2.75], F), np.array([0.5], F), np.array([[1.0, 0.5, 0.25]], F), np.array([0.5], F))
    bg = np.array([0.125, 0.25, 0.5], F)
    case = _case([[2.0, 3.0], [2.5, 0.0]], [[0.5, 0.5], [0.5, 0.0]], [[1.0, 2.0], [3.0, 0.0]], [[c["a1"], c["a2"]], [c["b"], [0, 0, 0]]],
                 factor=fac, ground=ground, bg=bg)
    ref = sdr.deep_ref(case)
    t1, t2, tb = _tau(1.0, 0.5), _tau(2.0, 0.5), _tau(3.0, 0.5)
    T, C, D = 1.0, np.zeros(3), 0.0
    for alpha, col, z, tau in ((1 - t1, np.array(c["a1"]) * 0.5, 2.0, t1), (1 - tb, np.array(c["b"]) * 0.75, 2.5, tb)):
        C, D, T = C + alpha * T * col, D + alpha * T * z, T * tau
    C, D, T = C + T * (np.array([1.0, 0.5, 0.25]) * 0.5 * 0.5), D + T * (0.5 * 2.75), T * 0.5
    C, D, T = C + (1 - t2) * T * np.array(c["a2"]) * 0.5, D + (1 - t2) * T * 3.0, T * t2
    assert np.allclose(ref["rgb"][0], C + T * bg.astype(np.float64), rtol=0, atol=1e-15)
    assert abs(ref["depth"][0] - D) <= 1e-15 and ref["alpha"][0] == 1.0 and ref["b_alpha"][0] == 0.0
    assert ref["owners"][0] == [0, 1, 2, 0] and ref["interleaved"] == 1
    # without the B sample the ground alone splits A's run: still interleaved, the layered order is not the merged one
    alone = _case([[2.0, 3.0]], [[0.5, 0.5]], [[1.0, 2.0]], [[c["a1"], c["a2"]]], ground=ground)
    assert sdr.deep_ref(alone)["owners"][0] == [0, 1, 0] and sdr.deep_ref(alone)["interleaved"] == 1
    assert not sdr.differs(sdr.deep_emulated(case), ref) and sdr.deep_emulated(case)["interleaved"] == 1
    assert sdr.deep_emulated(alone)["interleaved"] == 1


def test_ties_skips_stops_and_bad_values_by_hand():
    # an exact tie goes to the lower list, the ground comes last
    ground = (np.array([2.0], F), np.array([1.0], F), np.array([[1.0, 1.0, 1.0]], F), np.array([1.0], F))
    tie = _case([[2.0], [2.0]], [[1.0], [1.0]], [[50.0], [50.0]], [[[1, 0, 0]], [[0, 1, 0]]], ground=ground)
    ref = sdr.deep_ref(tie)
    assert ref["owners"][0] == [0, 1, 2] and ref["rgb"][0][0] > 0.999 and ref["rgb"][0][1] < 1e-6
    # a sample under the threshold changes nothing, not even T; its owner does not count
    faint = _case([[2.0, 3.0], [2.5, 0.0]], [[1.0, 1.0], [1.0, 0.0]], [[1.0, 1.0], [0.005, 0.0]], [[[1, 0, 0], [1, 0, 0]], [[0, 1, 0], [0, 0, 0]]])
    ref = sdr.deep_ref(faint)
    assert ref["owners"][0] == [0] and ref["interleaved"] == 0 and ref["rgb"][0][1] == 0.0
    assert abs(ref["alpha"][0] - (1 - _tau(1.0, 1.0) ** 2)) <= 1e-15
    # a list ends at its own stop: the third sample of A is never seen, B behind it is (at the joint T)
    t = _tau(5.0, 1.0)
    stop = _case([[2.0, 3.0, 4.0], [5.0, 0.0, 0.0]], [[1.0] * 3, [1.0, 0, 0]], [[5.0] * 3, [5.0, 0, 0]],
                 [[[1, 0, 0]] * 3, [[0, 1, 0], [0, 0, 0], [0, 0, 0]]])
    ref = sdr.deep_ref(stop)
    assert t * t < 1e-4 < t
    assert ref["n_composited"][0] == 3 and abs(ref["rgb"][0][1] - (1 - t) * t * t) <= 1e-18
    assert abs(ref["rgb"][0][0] - ((1 - t) + t * (1 - t))) <= 1e-15
    # non-finite sigma and colour count as 0; a non-finite z or delta ends its list
    bad = _case([[2.0, 3.0], [2.5, np.nan], [np.inf, 2.6]], [[1.0, 1.0], [1.0, 1.0], [1.0, 1.0]], [[np.nan, 1.0], [1.0, 9.0], [9.0, 9.0]],
                [[[1, 1, 1], [np.inf, 0.5, np.nan]], [[0, 1, 0], [1, 1, 1]], [[1, 1, 1], [1, 1, 1]]])
    ref = sdr.deep_ref(bad)
    assert ref["owners"][0] == [1, 0] and np.isfinite(ref["rgb"]).all()
    t1 = _tau(1.0, 1.0)
    assert np.allclose(ref["rgb"][0], [0.0, (1 - t1) + t1 * (1 - t1) * 0.5, 0.0], rtol=0, atol=1e-15)


def _dense_set(case):
    """a one-list case as a compact set of render_iter_refs.composite_ref: one candidate per sample, priors (0, 0, 1)"""
    z, dl = case["z"][0], case["delta"][0]                        # [S,n]
    S, n = z.shape
    with np.errstate(invalid="ignore"):
        filled = np.cumprod((dl > 0) & np.isfinite(z), axis=0).astype(bool)
    cnt = filled.sum(0)
    start = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    pick = lambda a: np.concatenate([a[:cnt[p], p] for p in range(n)]) if cnt.sum() else a[:0, 0]
    P = int(cnt.sum())
    step = np.array([dl[0, p] if cnt[p] else 0 for p in range(n)], F)
    assert all((dl[:cnt[p], p] == step[p]).all() for p in range(n))           # one step per ray, as the renderer has it
    return dict(inp=dict(R=n, alive=np.arange(n, dtype=np.int32), step=step),
                march=dict(n_eff=n, n_step=S, ray_cnt=cnt.astype(np.int32), ray_start=start, s_t=pick(z).astype(F), n_samples=P),
                thresh=sdr.THRESH, T0=np.ones(n, F), color0=np.zeros((n, 3), F), depth0=np.zeros(n, F), pt_off=np.arange(P, dtype=np.int32),
                pt_cnt=np.ones(P, np.int32), cand_sigma=pick(case["sigma"][0]).astype(F), cand_rgb=pick(case["rgb"][0]).astype(F), n_init=0)


@pytest.mark.parametrize("name", ["k1_n1_s1", "k1_n70_s37"])
def test_one_list_is_the_dense_compositing_of_render_iter_refs(name):
    case, ref = cases.case_and_ref(name)
    want = rir.composite_ref(_dense_set(case))
    assert np.abs(ref["rgb"] - want["color"]).max() <= 1e-15 and np.abs(ref["depth"] - want["depth"]).max() <= 1e-15
    assert np.abs(ref["T"] - want["T"]).max() <= 1e-15 and np.abs(ref["alpha"] - (1 - want["T"])).max() <= 1e-15
    assert np.allclose(ref["b_rgb"], want["b_color"], rtol=1e-9, atol=0) and np.allclose(ref["b_depth"], want["b_depth"], rtol=1e-9, atol=0)
    assert ref["interleaved"] == 0
    # and of its fp32 emulation, bit for bit
    emu, emu_want = sdr.deep_emulated(case), rir.composite_emulated(_dense_set(case))
    assert emu["rgb"].tobytes() == emu_want["color"].tobytes() and emu["depth"].tobytes() == emu_want["depth"].tobytes()
    assert emu["alpha"].tobytes() == (F(1) - emu_want["T"]).astype(F).tobytes()


def _layered64(c, a, d, ground, bg):
    """scene_refs.composite's step 3 on float64 layers (scene_refs rounds its inputs to fp32 first, which the per-layer sums of a
    float64 reference are not): take part iff a > 0, key d / a, order (key, index), C += T c, D += T d, T *= 1 - a; the ground with
    colour (c_g shade) a_g, term a_g t_g, key t_g and index K"""
    K, n = a.shape
    rgb, alpha, depth = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    for p in range(n):
        items = [(d[k, p] / a[k, p], k, c[k, p], a[k, p], d[k, p]) for k in range(K) if a[k, p] > 0]
        if ground is not None and ground[1][p] > 0:
            t_g, a_g, c_g, sh = (np.asarray(x[p], np.float64) for x in ground)
            items.append((float(t_g), K, (c_g * sh) * a_g, float(a_g), float(a_g * t_g)))
        items.sort(key=lambda it: (it[0], it[1]))
        C, D, T = np.zeros(3), 0.0, 1.0
        for _, _, col, op, term in items:
            C, D, T = C + T * col, D + T * term, T * (1.0 - op)
        rgb[p], alpha[p], depth[p] = (C, 1.0 - T, D) if bg is None else (C + T * bg[p], 1.0, D)
    return rgb, alpha, depth


def test_layered64_is_scene_refs_composite():
    """on layers that ARE fp32 values the restatement above and tests/scene_refs.py agree"""
    rng = np.random.default_rng(3)
    K, n = 3, 40
    a = rng.uniform(0, 1, (K, n)).astype(F) * (rng.uniform(size=(K, n)) < 0.8)
    c, d = rng.uniform(0, 1, (K, n, 3)).astype(F), (a * rng.uniform(2, 4, (K, n))).astype(F)
    ground = (rng.uniform(2, 4, n).astype(F), (rng.uniform(0, 1, n) * (np.arange(n) % 3 > 0)).astype(F), rng.uniform(0, 1, (n, 3)).astype(F),
              rng.uniform(0.4, 1, n).astype(F))
    bg = rng.uniform(0, 1, (n, 3)).astype(F)
    for g, b in ((None, None), (ground, None), (ground, bg)):
        want = sr.composite(c, a, d, ground=g, background=b)
        got = _layered64(c.astype(np.float64), a.astype(np.float64), d.astype(np.float64), g, None if b is None else b.astype(np.float64))
        for x, key in zip(got, ("rgb", "alpha", "depth")):
            assert np.abs(x - want[key]).max() <= 1e-15, key


@pytest.mark.parametrize("name", cases.DISJOINT)
def test_disjoint_blocks_equal_the_layered_composite_of_the_per_layer_sums(name):
    case, ref = cases.case_and_ref(name)
    K, n = case["K"], case["n"]
    assert ref["interleaved"] == 0
    c, a, d = np.zeros((K, n, 3)), np.zeros((K, n)), np.zeros((K, n))
    for k in range(K):
        one = sdr.deep_ref(cases.single(case, k))
        c[k], a[k], d[k] = one["rgb"], one["alpha"], one["depth"]
        if case["factor"] is not None:
            c[k] = c[k] * case["factor"][k].astype(np.float64)[:, None]
    assert (a > 0).sum(0).max() >= 2 and ((a > 0) & (a < 0.999)).any()
    bg = None if case["bg"] is None else np.broadcast_to(np.asarray(case["bg"], np.float64).reshape(-1, 3), (n, 3))
    rgb, alpha, depth = _layered64(c, a, d, case["ground"], bg)
    assert np.abs(ref["rgb"] - rgb).max() <= 1e-12 and np.abs(ref["alpha"] - alpha).max() <= 1e-12 and np.abs(ref["depth"] - depth).max() <= 1e-12
    # the blocks are met in another order than the lists' at some pixel: the merge sorts
    assert any(o != sorted(o) for o in ref["owners"]) or K == 1


@pytest.mark.parametrize("name", cases.NAMES)
def test_emulation_within_bound_and_few_undecidable_pixels(name):
    case, ref = cases.case_and_ref(name)
    und = int(ref["undecidable"].sum())
    print("%s: %d of %d pixels undecidable, %d interleaved" % (name, und, case["n"], ref["interleaved"]))
    assert und <= sdr.MAX_UNDECIDABLE * case["n"]
    emu = sdr.deep_emulated(case)
    assert not sdr.differs(emu, ref)
    assert emu["interleaved"] == ref["interleaved"] or und
    fin = np.isfinite(case["rgb"]).all() and np.isfinite(case["sigma"]).all()
    assert np.isfinite(ref["rgb"]).all() and np.isfinite(ref["depth"]).all() and np.isfinite(ref["alpha"]).all(), fin
    sdr.deep_compare(emu, ref, name + " (fp32 emulation)")


@pytest.mark.parametrize("mutant", sdr.MUTANTS)
def test_every_mutant_is_caught(mutant):
    caught = [name for name in cases.NAMES if sdr.differs(sdr.deep_emulated(cases.case_and_ref(name)[0], mutant), cases.case_and_ref(name)[1])]
    print("%s: caught by %s" % (mutant, ", ".join(caught)))
    assert caught


def test_the_cases_contain_what_they_claim():
    Ks, ns, Ss = set(), set(), set()
    kinds, wheres, bgs, facs = set(), set(), set(), set()
    for name in cases.NAMES:
        case, ref = cases.case_and_ref(name)
        Ks.add(case["K"]); ns.add(case["n"]); Ss.add(case["S"])
        kinds |= set(case["kinds"].reshape(-1).tolist())
        if case["ground"] is not None:
            wheres |= set(case["ground_where"].tolist())
        bgs.add(None if case["bg"] is None else case["bg"].size == 3)
        facs.add(case["factor"] is not None)
        z, dl = case["z"], case["delta"]
        with np.errstate(invalid="ignore"):
            live = (dl > 0) & np.isfinite(z)
        if case["mode"] == "ties" and case["K"] > 1 and case["n"] > 1:
            both = live[0] & live[1]
            assert (z[0][:, None][..., :] == z[1][None]).any() and both.any(), name        # equal keys across lists
            assert any(len(o) >= 2 for o in ref["owners"])
        if case["mode"] == "interleaved" and case["K"] > 1 and case["n"] > 1 and case["S"] > 1:
            assert ref["interleaved"] > case["n"] // 4, name
        if case["mode"] == "disjoint":
            assert ref["interleaved"] == 0, name
        if case["ground"] is not None and case["n"] > 1:
            assert any(case["K"] in o and o[0] != case["K"] and o[-1] != case["K"] for o in ref["owners"]), name    # the ground between samples
    assert Ks == {1, 2, 3, 8} and ns == {1, 70} and Ss == {1, 4, 37}
    assert kinds == {"empty", "full", "part", "stop", "faint", "mixed"} and wheres == {"front", "between", "behind", "absent"}
    assert bgs == {None, True, False} and facs == {True, False}
    # a list cut by its own stop: filled slots behind the last composited sample of a "stop" list
    case, ref = cases.case_and_ref("k2_inter")
    stops = np.argwhere(case["kinds"] == "stop")
    assert len(stops) and case["S"] > 8
    bad = [n for n in cases.NAMES if not all(np.isfinite(cases.make(n)[k]).all() for k in ("z", "delta", "sigma", "rgb"))]
    assert bad == ["k3_inter_bad", "k8_ties_bad"]
    for n in bad:
        c = cases.make(n)
        assert all((~np.isfinite(c[k])).any() for k in ("z", "delta", "sigma", "rgb")), n


def test_binding_table():
    from instantavatar_amd import _lib, build
    d = _lib.declarations("scene_deep")
    assert sorted(d) == ["ia_scene_deep_composite"] and d["ia_scene_deep_composite"].stream and len(d["ia_scene_deep_composite"].params) == 20
    assert hasattr(_lib.lib(), "ia_scene_deep_composite") and "ia_scene_deep_composite" in _lib._bound
    assert "ia_scene_deep.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_scene_deep.hip"))
    assert os.path.normpath(_lib.header_path("scene_deep")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_scene_deep.hip" in build.source_manifest() and "ia_scene_deep.hip" in build.library_manifest()
    with pytest.raises(_lib.IAError, match=r"instantavatar_hip_scene_deep\.h"):
        _lib.call("ia_scene_nothing")
    with open(_lib.header_path("scene_deep")) as f:
        assert "#define IA_SCENE_DEEP_MAX_SLOTS %d" % sdr.MAX_SLOTS in f.read()


def test_host_side_argument_errors():
    """what the entry point decides before any launch"""
    from instantavatar_amd import _lib
    P = 4096                                                  # (a non-null address that is never read: every call below is refused)

    def deep(K=2, S=4, n=4, ground=(None,) * 4, thresh=0.01, z=P, out=P):
        return _lib.call("ia_scene_deep_composite", z, P, P, P, K, S, n, None, *ground, None, 0, thresh, out, P, P, P, None)
    for K in (0, 9, -1):
        with pytest.raises(_lib.IAError, match="K = %d outside" % K):
            deep(K=K)
    for S in (0, 1025):
        with pytest.raises(_lib.IAError, match="S = %d outside" % S):
            deep(S=S)
    with pytest.raises(_lib.IAError, match="n = -1"):
        deep(n=-1)
    for t in (-0.1, float("nan"), float("inf")):
        with pytest.raises(_lib.IAError, match="thresh"):
            deep(thresh=t)
    with pytest.raises(_lib.IAError, match="or none of them"):
        deep(ground=(P, P, None, P))
    with pytest.raises(_lib.IAError, match="null pointer"):
        deep(z=None)
    assert deep(n=0, z=None, out=None) == 0                    # nothing to do: nothing is read
