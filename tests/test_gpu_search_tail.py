"""k_search with sparse waves against the CPU oracle, BIT FOR BIT (-m gpu): the slot-aware refill of a short pull and the tail
compaction (instantavatar_amd/csrc/ia_search_tail.h) change which LANE runs a solve, never what a solve computes.

World, points and checks are those of test_gpu_search_exact.py (the 8 x 16 x 16 grid of tests/world.py; the dense layout, the
compacted roots, the J_inv route, each with the in-library profiling off and on, the solve / fetch counters against the
oracle's own counts).  What differs is the shapes, chosen so that waves start in, and decay through, each placement class:

  * P = 1, 5, 16, 17, 32, 33, 64, 200 points x n_init = 1, 2, 13: queues of fewer than 16, 17..32, 33..64 and several hundred
    items -- a wave's FIRST pull is short (slot-aware refill into slot 0, then 3, 1, 2), exactly fills it, or is one of many;
  * the points mix roots of different trip counts, two-trip divergers, trivial points and NaN / +-1e30 (`_points`), so a wave
    that starts with 33..64 live solves loses most of them after two trips and crosses both thresholds (32, 16) while the
    long solves go on -- with 200 points while other waves of the workgroup are still pulling.

Plus placement invariance: the same 200 points in three random orders give, per point, identical candidates and J_inv, and
the same solve / fetch / loaded totals."""
import numpy as np
import pytest

from instantavatar_amd import _lib, synthetic as syn

import test_gpu_search_exact as E
import world as W

pytestmark = pytest.mark.gpu
P_LIST = [1, 5, 16, 17, 32, 33, 64, 200]
N_LIST = [1, 2, 13]


@pytest.fixture(scope="module")
def case(oracle):
    """the unit world of test_gpu_search_exact with the oracle's results for n_init = 1, 2, 13 at 200 points, computed once (a
    prefix of the points is a prefix of the results: solves are independent)"""
    body = syn.make_body()
    init32 = oracle.deformer_initialize(body, np.zeros(10, np.float32), syn.cano_pose("A_pose"), resolution=32, n_smooth=30)
    wv = np.ascontiguousarray(init32["lbs_voxel"][:, :, ::2, ::2])
    wv /= wv.sum(0, keepdims=True)
    poses, tr = W.poses()
    tfs, _ = oracle.prepare_deformer(body, init32, np.zeros(10, np.float32), poses[5, 3:], poses[5, :3], tr[5])
    t = np.ascontiguousarray(tfs, np.float32)
    init = dict(lbs_voxel=wv, offset_kernel=init32["offset_kernel"].astype(np.float32), scale_kernel=init32["scale_kernel"].astype(np.float32),
                D=8, H=16, W=16)
    vJ, vd = oracle.precompute(init, t)
    pts = E._points(vd, np.random.RandomState(3))
    ref = {}
    for n in N_LIST:
        bones = syn.INIT_BONES[:n]
        x, Ji, raw, it = oracle.broyden(pts, vJ, t, init, bones, 1e-5, 1e-1, want_iters=True)
        q = E._queued(pts, t, bones, init["offset_kernel"], init["scale_kernel"], np.array([16, 16, 8]))
        ref[n] = dict(x=x, Ji=Ji.reshape(len(pts), n, 9), raw=raw, keep=oracle.filter_dup(x, raw), it=it, queued=q)
    return dict(init=init, tfs=t, vJ_cl=np.ascontiguousarray(np.transpose(vJ, (1, 2, 3, 0))), pts=pts, ref=ref, cvg=1e-5, dvg=1e-1)


def test_the_shapes_reach_every_placement_class(case):
    """from the oracle alone: queue lengths on both sides of 16, 32 and 64, and trip counts uneven enough that a full wave
    thins out below 32 and below 16 while long solves remain"""
    live = {(P, n): int(case["ref"][n]["queued"][:P].sum()) for P in P_LIST for n in N_LIST}
    print("queued solves per shape:", live)
    assert any(0 < v <= 16 for v in live.values()) and any(16 < v <= 32 for v in live.values())
    assert any(32 < v <= 64 for v in live.values()) and any(v > 256 for v in live.values())
    for n in (2, 13):
        r = case["ref"][n]
        it = r["it"][r["queued"]]                       # fetches of every queued solve
        print("n_init %d: %d queued, fetches per solve: %s" % (n, it.size, np.bincount(it)))
        assert (it <= 2).mean() > 0.3 and (it >= 4).sum() >= 17 and (it >= 6).sum() >= 1
    # P = 64, n_init = 2: the queue (33..64 items) is ONE short pull of one wave, which then thins out past 32 and past 16
    q = case["ref"][2]["queued"][:64]
    it = case["ref"][2]["it"][:64][q]
    print("P 64, n_init 2: fetches per solve:", np.bincount(it))
    assert 32 < it.size <= 64 and 16 < (it >= 3).sum() <= 32 and 0 < (it >= 7).sum() <= 16


@pytest.mark.parametrize("n_init", N_LIST)
@pytest.mark.parametrize("P", P_LIST)
def test_sparse_waves_are_the_oracle_bit_for_bit(case, P, n_init):
    E._check_case(case, P, n_init)


def _by_point(got, P):
    cand, cJ, off, cnt, n_cand = got
    return [(E._bits(cand[off[p]:off[p] + cnt[p]]).tobytes(), E._bits(cJ[off[p]:off[p] + cnt[p]]).tobytes()) for p in range(P)], n_cand


def test_the_order_of_the_points_does_not_change_a_point(case):
    P, n = 200, 13
    r = case["ref"][n]
    want = [(E._bits(r["x"][p][r["keep"][p].astype(bool)]).tobytes(), E._bits(r["Ji"][p][r["keep"][p].astype(bool)]).tobytes()) for p in range(P)]
    rng = np.random.RandomState(5)
    totals = []
    try:
        for k in range(4):
            perm = np.arange(P) if k == 0 else rng.permutation(P)
            c = dict(case, pts=np.ascontiguousarray(case["pts"][perm]))
            for prof in (0, 1):                       # the product kernel, then the counting instantiation
                _lib.call("ia_profile_enable", prof)
                _lib.call("ia_profile_reset")
                got, n_cand = _by_point(E._run_compact(c, P, n, True), P)
                if prof:
                    totals.append(E._units())
                assert n_cand == int(r["keep"].sum())
                for j, p in enumerate(perm):
                    assert got[j] == want[p], (k, prof, j, p)
    finally:
        _lib.call("ia_profile_reset")
        _lib.call("ia_profile_enable", 0)
    print("solves / fetches / loaded per order:", totals)
    assert all(t == totals[0] for t in totals)
    assert totals[0][:2] == [int(r["queued"].sum()), int(r["it"][r["queued"]].sum())]
