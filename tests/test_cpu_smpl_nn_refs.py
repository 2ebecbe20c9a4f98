"""Pins tests/smpl_nn_refs.py itself (no GPU).  (a) The exact layer equals the oracle's `smpl_nn_deform` -- a C loop with
fmaf -- bit for bit (index, validity, canonical point) on every body and staging size.  (b) The exact layer satisfies the
float64 comparator on every body: the chosen vertex is a true nearest up to rounding, validity agrees outside the band
around thr^2, the canonical point is inside its bound.  (c) The float32 restatement of the vertex grid (header, clamped
binning, 27-cell query) equals the exact layer on every body.  (d) Ten seeded defects are each rejected by at least one
body, and the test says by which ("DEFECT ..." lines); the unfused distance is rejected by the bit-exact comparison while
it stays inside the float64 bounds, which is what the exact layer is for.  Cells exactly `thr` wide instead of 1.001 thr
are rejected by the directed body `margin` alone, where a vertex's cell coordinate rounds up across a cell boundary."""
import numpy as np
import pytest

import smpl_nn_refs as nr

ALL = nr.BODIES


def _grid_result(c, defect=None):
    return nr.GridEmu(c["verts"], c["thr"], defect).query(c["pts"], c["T_inv"], c["thr"])


@pytest.mark.parametrize("name", ALL)
def test_bodies_discriminate(name):
    """the assertions of `case` (valid and invalid points, exact ties, exact threshold hits) hold; print what each body holds"""
    c = nr.case(name)
    r = c["ref"]
    g = nr.GridEmu(c["verts"], c["thr"])
    print("BODY %-12s V %4d  P %4d  valid %.2f  tied valid %4d  dist == thr2 %3d  grid %s  h %.5f" % (
        name, len(c["verts"]), len(c["pts"]), r["valid"].mean(), int((r["valid"] & (r["ties"] > 1)).sum()),
        int((r["best"] == nr.thr2_of(c["thr"])).sum()), "x".join(map(str, g.dims)), g.h))
    assert len(c["pts"]) <= nr.P_CAP and not np.isfinite(c["pts"]).all()
    if name == "line500":
        assert g.dims[0] == nr.MAX_DIM and g.h > np.float32(c["thr"]) * np.float32(1.001), "the extent does not set the cell"
    if name == "margin":
        assert g.h == np.float32(c["thr"] * np.float32(1.001)) and g.dims[0] == 6
    if name in ("sheet", "coincident5", "one"):
        assert g.dims.min() <= 3
    if name == "cloud257":
        assert g.h == np.float32(np.float32(c["thr"]) * np.float32(1.001)) and g.dims.max() <= 10


@pytest.mark.parametrize("name", ALL + tuple("staging%d" % n for n in nr.STAGING_SIZES))
def test_exact_layer_equals_the_oracle(oracle, name):
    c = nr.staging_case(int(name[7:])) if name.startswith("staging") else nr.case(name)
    cano, valid, idx = oracle.smpl_nn_deform(c["pts"], c["verts"], c["T_inv"], c["thr"])
    got = dict(idx=idx, valid=valid, cano=cano)
    assert nr.agree_exact(got, c["ref"]) == 0


@pytest.mark.parametrize("name", ALL + tuple("staging%d" % n for n in nr.STAGING_SIZES))
def test_exact_layer_passes_float64(name):
    c = nr.staging_case(int(name[7:])) if name.startswith("staging") else nr.case(name)
    r = nr.check64(c["pts"], c["verts"], c["T_inv"], c["thr"], c["ref"]["idx"], c["ref"]["valid"], c["ref"]["cano"])
    print("RATIO cpu %-24s nearest %.4f  cano %.4f  validity decided on %d of %d" % (name, r["nn"], r["cano"], r["decided"], len(c["pts"])))
    assert nr.passes64(r), r
    assert r["decided"] > 0


@pytest.mark.parametrize("name", ALL)
def test_grid_emulation_equals_exact_layer(name):
    c = nr.case(name)
    assert nr.agree_grid(_grid_result(c), c["ref"]) == 0


def test_grid_emulation_with_a_smaller_query_threshold():
    """a grid built for t serves every query threshold up to t"""
    for name in ("cloud257", "lattice400", "line500"):
        c = nr.case(name)
        g = nr.GridEmu(c["verts"], c["thr"])
        for div in (2, 16):
            t = c["thr"] / div
            ref = nr.nn_exact(c["pts"], c["verts"], c["T_inv"], t)
            assert ref["valid"].any()
            assert nr.agree_grid(g.query(c["pts"], c["T_inv"], t), ref) == 0


GRID_DEFECTS = ("cell_thr", "cell_half", "own_cell", "corner", "slot_ties", "upper_face")
EXACT_DEFECTS = ("le", "no_translation", "skip_tail")


@pytest.mark.parametrize("defect", GRID_DEFECTS)
def test_grid_defect_is_rejected(defect):
    hit = {n: nr.agree_grid(_grid_result(nr.case(n), defect), nr.case(n)["ref"]) for n in ALL}
    print("DEFECT %-16s rejected by %s" % (defect, ", ".join("%s (%d points)" % kv for kv in hit.items() if kv[1]) or "NOTHING"))
    assert any(hit.values()), defect
    if defect == "cell_thr":
        # the margin 1.001 exists for the rounding of the cell coordinates; only the directed body reaches it
        assert hit["margin"] > 0


@pytest.mark.parametrize("defect", EXACT_DEFECTS)
def test_exact_defect_is_rejected(defect):
    """a defect of the brute-force kernel: rejected bit for bit, and by the float64 comparator where it is more than rounding"""
    hit, hit64 = {}, {}
    for n in ALL:
        c = nr.case(n)
        bad = nr.nn_exact(c["pts"], c["verts"], c["T_inv"], c["thr"], mutant=defect)
        hit[n] = nr.agree_exact(bad, c["ref"])
        hit64[n] = not nr.passes64(nr.check64(c["pts"], c["verts"], c["T_inv"], c["thr"], bad["idx"], bad["valid"], bad["cano"]))
    print("DEFECT %-16s rejected by %s; by float64 alone on %s" % (defect, ", ".join("%s (%d points)" % kv for kv in hit.items() if kv[1]) or "NOTHING",
                                                                  ", ".join(k for k, v in hit64.items() if v) or "nothing"))
    assert any(hit.values()), defect
    if defect == "le":
        # dist == thr^2 lies inside the band the float64 layer leaves open: only the exact layer decides it
        assert hit["lattice400"] and not any(hit64.values())
    else:
        assert any(hit64.values()), defect


def test_unfused_distance_is_rejected_only_bit_for_bit():
    """plain products and sums instead of the two fused operations: within rounding of float64, so the float64 comparator
    accepts it on every body; the exact layer does not"""
    hit = {}
    for n in ALL:
        c = nr.case(n)
        bad = nr.nn_exact(c["pts"], c["verts"], c["T_inv"], c["thr"], mutant="unfused")
        hit[n] = nr.agree_exact(bad, c["ref"])
        r = nr.check64(c["pts"], c["verts"], c["T_inv"], c["thr"], bad["idx"], bad["valid"], bad["cano"])
        assert nr.passes64(r), (n, r)
    print("DEFECT %-16s rejected by %s" % ("unfused", ", ".join("%s (%d points)" % kv for kv in hit.items() if kv[1]) or "NOTHING"))
    assert any(hit.values())


def test_compact_comparator_rejects_seeded_outputs():
    """check_compact accepts the compaction in point order and with two blocks' ranges exchanged, and rejects an offset that
    repeats, a block out of order, a candidate of the wrong point and a written slot past n_cand"""
    c = nr.case("cloud257")
    ref, n_live, P = c["ref"], 1000, 1003
    k = nr.compact_ref(ref, n_live)

    def buffers(pt_off=None, idx=None):
        off = k["pt_off"] if pt_off is None else pt_off
        o = dict(n_cand=k["n_cand"], pt_cnt=np.full(P, nr.SENT_B, np.uint8), pt_off=np.full(P, nr.SENT_I, np.int32), idx=np.full(P, nr.SENT_I, np.int32),
                 cand_pt=np.full(P, nr.SENT_I, np.int32), cand_xc=np.full((P, 3), nr.SENT_F, np.float32))
        o["pt_cnt"][:n_live], o["pt_off"][:n_live] = k["pt_cnt"], off
        o["idx"][:n_live] = ref["idx"][:n_live] if idx is None else idx
        v = ref["valid"][:n_live]
        o["cand_pt"][off[v]] = np.flatnonzero(v)
        o["cand_xc"][off[v]] = ref["cano"][:n_live][v]
        return o

    nr.check_compact(buffers(), ref, n_live, "brute")
    v = ref["valid"][:n_live]
    n0, n1 = int(v[:256].sum()), int(v[256:512].sum())
    swapped = k["pt_off"].copy()
    swapped[:256] += n1
    swapped[256:512] -= n0
    nr.check_compact(buffers(swapped), ref, n_live, "brute")
    grid_idx = np.where(v, ref["idx"][:n_live], -1)
    nr.check_compact(buffers(idx=grid_idx), ref, n_live, "grid")

    def rejected(o, route="brute"):
        with pytest.raises(AssertionError):
            nr.check_compact(o, ref, n_live, route)

    rejected(buffers(idx=grid_idx), "brute")
    rejected(buffers(), "grid")
    first = np.flatnonzero(v)[:2]
    rev = k["pt_off"].copy()
    rev[first] = rev[first[::-1]]
    rejected(buffers(rev))                                  # a bijection, but not increasing inside the block
    o = buffers()
    o["cand_pt"][0] += 1
    rejected(o)
    o = buffers()
    o["cand_xc"][k["n_cand"]] = 0
    rejected(o)
    o = buffers()
    o["pt_cnt"][n_live] = 0
    rejected(o)
    o = buffers()
    o["n_cand"] += 1
    rejected(o)
