"""tests/meshray_refs.py, the float64 brute-force reference of the ray queries ("ray queries"), is itself checked here
against analysis: spheres, the slab test, a dyadic triangle, parity.  Then the conditions the GPU tests rely on, asserted on those tests'
own inputs (which rays are clear, how many hit), the binding table of include/instantavatar_hip_meshray.h, what the entry points refuse
before anything is launched, and the drivers' refusals.  No GPU."""
import os

import numpy as np
import pytest

import meshray_refs as mr

NAMES = ["ia_meshray_closest", "ia_meshray_count"]


def _header():
    from instantavatar_amd import _lib
    with open(_lib.header_path("meshray")) as f:
        return f.read()


# ---- the reference against analysis ----------------------------------------------------------------------------------------------------
def test_rd32_ru32():
    x = np.array([0.1, -0.1, 1.0, 1e-50, -1e-50, 1e77, -1e77, 0.0, np.inf, -np.inf])
    lo, hi = mr.rd32(x), mr.ru32(x)
    assert lo.dtype == np.float32 and hi.dtype == np.float32
    assert (lo.astype(np.float64) <= x).all() and (hi.astype(np.float64) >= x).all()
    exact = np.array([False, False, True, False, False, False, False, True, True, True])
    assert np.array_equal(lo == hi, exact)
    with np.errstate(over="ignore"):
        assert (np.nextafter(lo, np.float32(np.inf))[~exact] == hi[~exact]).all()              # neighbours: nothing lies between
    assert lo[5] == np.finfo(np.float32).max and np.isposinf(hi[5]) and np.isneginf(lo[6]) and hi[6] == -np.finfo(np.float32).max
    assert lo[3] == 0 and hi[3] == np.float32(1e-45) and hi[4] == 0 and lo[4] == -np.float32(1e-45)


def test_icosphere_first_hit_lies_between_the_two_spheres():
    v, f = mr.icosphere(2)
    o, d = mr.probe_rays()
    ref = mr.closest(o, d, v, f)
    r_in = np.linalg.norm(v.astype(np.float64)[f].mean(1), axis=1).min()                       # the face centres are the closest points of a face
    r_out = np.linalg.norm(v.astype(np.float64), axis=1).max()
    assert 0.97 < r_in < r_out < 1 + 1e-6
    outside = np.linalg.norm(o, axis=1) > 2
    t_far, t_near = mr.sphere_hit(o, d, r_in), mr.sphere_hit(o, d, r_out)
    hit = ref["face"] >= 0
    assert (hit[np.isfinite(t_far)]).all() and not hit[~np.isfinite(t_near)].any()               # through the inner sphere: hit; past the outer: miss
    # from outside the first hit lies between the spheres' entries, from inside between their exits
    both = hit & np.isfinite(t_far)
    lo = np.where(outside, t_near, t_far)[both]
    hi = np.where(outside, t_far, t_near)[both]
    assert (lo - 1e-12 <= ref["t"][both]).all() and (ref["t"][both] <= hi + 1e-12).all()
    b = ref["bary"][hit]
    assert (b >= 0).all() and np.abs(b.sum(1) - 1).max() < 1e-15
    p = (b[:, :, None] * v.astype(np.float64)[f[ref["face"][hit]]]).sum(1)
    at = o[hit].astype(np.float64) + ref["t"][hit, None] * d[hit].astype(np.float64)
    assert np.abs(p - at).max() < 1e-14                                                          # bary = (w, u, v) weighs (p0, p1, p2)
    n = mr.count(o, d, v, f)
    assert (n[outside & hit] == 2).all() and (n[~outside] == 1).all() and (n[~hit] == 0).all()
    assert np.array_equal(mr.count(o, d, v, f, limit=1), np.minimum(n, 1))


def test_cube_agrees_with_the_slab_test():
    v, f = mr.cube(8, half=1.0)
    rng = np.random.default_rng(11)
    o = rng.uniform(-2.5, 2.5, (1500, 3)).astype(np.float32)
    d = rng.uniform(-1, 1, (1500, 3)).astype(np.float32)
    ref = mr.closest(o, d, v, f)
    want = mr.slab_hit(o, d, 1.0)
    assert np.array_equal(np.isfinite(ref["t"]), np.isfinite(want)) and 0.1 < np.isfinite(want).mean() < 0.9      # hits and misses both
    k = np.isfinite(want)
    assert np.abs(ref["t"][k] - want[k]).max() < 1e-13
    # on the lattice itself every number is dyadic: exactly the slab test, ties at edges and vertices included
    o, d = mr.cube_rays()
    H = mr.hits(o, d, v, f)
    ref = mr.closest(o, d, v, f, H=H)
    assert len(o) < 5000 and np.array_equal(ref["t"], mr.slab_hit(o, d, 1.0))
    tied = (H["hit"] & (H["t"] == ref["t"][:, None])).sum(1)
    assert (tied >= 2).sum() > 400 and (tied >= 4).sum() > 50
    k = np.where(tied >= 2)[0]
    assert (ref["face"][k] == np.argmax(H["hit"][k] & (H["t"][k] == ref["t"][k, None]), 1)).all()       # the smallest index among the tied


def test_one_dyadic_triangle_is_exact():
    v, f = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.int32([[0, 1, 2]])
    o = np.float32([[0.25, 0.25, 1], [0.5, 0, 1], [0, 0, -1], [0.75, 0.75, 1], [0.25, 0.25, 0.5], [0.25, 0.25, 1], [0.25, 0.25, 1]])
    d = np.float32([[0, 0, -1], [0, 0, -1], [0, 0, 2], [0, 0, -1], [1, 0, 0], [0, 0, 1], [0, 0, 0]])
    ref = mr.closest(o, d, v, f)
    assert ref["t"].tolist() == [1.0, 1.0, 0.5, np.inf, np.inf, np.inf, np.inf] and ref["face"].tolist() == [0, 0, 0, -1, -1, -1, -1]
    assert ref["bary"][:3].tolist() == [[0.5, 0.25, 0.25], [0.5, 0.5, 0.0], [1.0, 0.0, 0.0]]
    up, down = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))
    one = lambda t0, t1: mr.count(o[:1], d[:1], v, f, np.float32([t0]), np.float32([t1]))[0]
    assert one(1, np.inf) == 1 and one(0, 1) == 1 and one(up, np.inf) == 0 and one(0, down) == 0
    assert one(2, 1) == -1 and one(np.nan, 1) == -1 and one(-1, 1) == -1
    assert np.isnan(mr.closest(o[:1] * np.nan, d[:1], v, f)["t"][0])
    # faces that are not valid never hit
    junk = np.int32([[0, 0, 1], [0, 1, 7], [-1, 1, 2]])
    assert (mr.count(o, d, v, junk) == 0).all()


def test_parity_on_icosphere_cube_and_shell():
    dirs = mr.inside_dirs(_header())
    rng = np.random.default_rng(5)
    p = rng.uniform(-1.3, 1.3, (1200, 3)).astype(np.float32)
    r, c = np.linalg.norm(p.astype(np.float64), axis=1), np.abs(p).max(1)
    k = (r < 0.9) | (r > 1.05)
    assert np.array_equal(mr.contains(p[k], *mr.icosphere(2), dirs), r[k] < 0.9)
    k = (c < 0.95) | (c > 1.05)
    assert np.array_equal(mr.contains(p[k], *mr.cube(8, half=1.0), dirs), c[k] < 0.95)
    k = (r < 0.44) | ((r > 0.55) & (r < 0.9)) | (r > 1.05)
    assert np.array_equal(mr.contains(p[k], *mr.shell(), dirs), (r[k] > 0.55) & (r[k] < 0.9))
    assert not mr.contains(np.float32([[np.nan, 0, 0]]), *mr.icosphere(1), dirs)[0]


def test_the_inside_directions_are_skewed():
    d = mr.inside_dirs(_header()).astype(np.float64)
    u = d / np.linalg.norm(d, axis=1, keepdims=True)
    s10, c10 = np.sin(np.radians(10)), np.cos(np.radians(10))
    assert (np.abs(u) > s10).all()                                     # 10 degrees off every coordinate plane -- and so off every axis
    assert (np.abs(u).max(1) < c10).all()
    assert (np.abs(u).sum(1) / np.sqrt(3) < c10).all()                 # and off every cube diagonal
    g = np.abs(u @ u.T)[np.triu_indices(3, 1)]
    assert (np.degrees(np.arccos(g)) >= 75).all()                      # pairwise far from parallel, as the header says


# ---- what the GPU tests rely on -----------------------------------------------------------------------------------------------------------
def test_the_probe_rays_are_clear():
    v, f = mr.icosphere(2)
    o, d = mr.probe_rays()
    assert len(f) == 320 and o.shape == (4096, 3)
    H = mr.hits(o, d, v, f)
    bad = mr.unclear(o, d, v, f, H=H)
    ref = mr.closest(o, d, v, f, H=H)
    hit = ref["face"] >= 0
    print("unclear rays: %d of %d; hitting: %.1f %%" % (bad.sum(), len(o), 100 * hit.mean()))
    assert bad.mean() <= 0.01 and 0.8 < hit.mean() < 0.98                               # hits and misses both
    t = np.sort(np.where(H["hit"], H["t"], np.inf), 1)
    assert not (np.isfinite(t[:, 1]) & (t[:, 1] == t[:, 0])).any()                             # no ties
    dirs = mr.inside_dirs(_header())
    assert np.array_equal(mr.contains(o, v, f, dirs), np.linalg.norm(o, axis=1) < 0.9)         # parity = the analytic answer, all 4 096
    # the second range of the GPU test
    t0 = np.where(hit, ref["t"] * 1.5, 0.5).astype(np.float32)
    assert mr.unclear(o, d, v, f, t0, None).mean() <= 0.01


def test_the_fan_rays_are_clear():
    fv, ff = mr.fan(7)
    v = np.concatenate([fv, np.float32([[-3, -3, -0.5], [3, -3, -0.5], [0, 4, 0.7]])])
    f = np.concatenate([ff, np.int32([[8, 9, 10]])])
    rng = np.random.default_rng(2)
    o = np.concatenate([rng.uniform(-2, 2, (1500, 3)) * [1, 1, 0.5] + [0, 0, 2], rng.uniform(-1, 1, (500, 3))]).astype(np.float32)
    d = (rng.uniform(-1, 1, (2000, 3)) * [1, 1, 0.3] - o * [0, 0, 1]).astype(np.float32)
    H = mr.hits(o, d, v, f)
    assert mr.unclear(o, d, v, f, H=H).mean() <= 0.01 and (mr.closest(o, d, v, f, H=H)["face"] >= 0).mean() > 0.3
    assert (mr.count(o, d, v, f, H=H) >= 2).sum() > 100                                        # the fan above the big face: two hits


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_meshray_header_is_bound():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    d = _lib.declarations("meshray")
    assert sorted(d) == NAMES
    for name in NAMES:
        assert d[name].stream, name
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
    assert [p.name for p in d["ia_meshray_count"].params[-4:]] == ["limit", "count", "tests", "stream"]
    assert [p.name for p in d["ia_meshray_closest"].params[:5]] == ["origins", "dirs", "t_min", "t_max", "P"]
    assert "ia_meshray.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_meshray.hip"))
    assert os.path.normpath(_lib.header_path("meshray")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_meshray.hip" in build.source_manifest() and "ia_meshray.hip" in build.library_manifest()
    with pytest.raises(_lib.IAError, match=r"instantavatar_hip_meshray\.h"):
        _lib.call("ia_meshray_nothing")
    from instantavatar_amd import meshdist
    assert meshdist.inside_dirs().tobytes() == mr.inside_dirs(_header()).tobytes() and meshdist.inside_dirs().shape == (3, 3)


def test_host_side_argument_errors():
    """what the entry points decide before any launch"""
    from instantavatar_amd import _lib
    A = 4096                                                  # (a non-null address that is never read: every call below is refused)
    inv = float(np.float32(1.0 / np.float64(np.float32(0.5))))

    def closest(P=4, nf=2, h=0.5, inv_h=inv, hi=1.0, n_pairs=2, ws=A, ws_bytes=1 << 20, inside=0, o=A, t=A):
        return _lib.call("ia_meshray_closest", o, A, None, None, P, nf, 0.0, 0.0, 0.0, hi, 1.0, 1.0, h, inv_h, n_pairs, ws, ws_bytes, inside,
                         t, None, None, None, None)

    def count(limit=1, P=4, inside=0, out=A, ws_bytes=1 << 20):
        return _lib.call("ia_meshray_count", A, A, None, None, P, 2, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 0.5, inv, 2, A, ws_bytes, inside, limit, out,
                         None, None)
    with pytest.raises(_lib.IAError, match="P = -1"):
        closest(P=-1)
    with pytest.raises(_lib.IAError, match="nf = -2"):
        closest(nf=-2)
    with pytest.raises(_lib.IAError, match="cell edge"):
        closest(h=0.0)
    with pytest.raises(_lib.IAError, match=r"not fp32\(1 / h\)"):
        closest(inv_h=2.0000002)
    with pytest.raises(_lib.IAError, match="not finite"):
        closest(hi=float("inf"))
    with pytest.raises(_lib.IAError, match="n_pairs"):
        closest(n_pairs=-1)
    with pytest.raises(_lib.IAError, match="faces_inside = 2"):
        closest(inside=2)
    with pytest.raises(_lib.IAError, match="null pointer"):
        closest(ws=None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        closest(o=None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        closest(t=None)
    with pytest.raises(_lib.IAError, match="workspace too small"):
        closest(ws_bytes=16)
    assert closest(P=0, o=None, t=None, ws=None, ws_bytes=0) == 0             # nothing to do: nothing is read
    for limit in (0, -3):
        with pytest.raises(_lib.IAError, match="limit = %d" % limit):
            count(limit=limit)
    with pytest.raises(_lib.IAError, match="null pointer"):
        count(out=None)
    with pytest.raises(_lib.IAError, match="workspace too small"):
        count(ws_bytes=16)
    with pytest.raises(_lib.IAError, match="faces_inside = -1"):
        count(inside=-1)
    assert count(P=0, out=None) == 0


# ---- the drivers' refusals -------------------------------------------------------------------------------------------------------------------
def test_signed_needs_deviation(tmp_path, capsys):
    from instantavatar_amd.drivers import extract_mesh
    with pytest.raises(SystemExit) as e:
        extract_mesh.main(["--synthetic", "--resolution", "48", "--simplify", "3", "--signed", "--out", str(tmp_path / "no")])
    assert e.value.code == 2 and "--deviation" in capsys.readouterr().err and not os.path.exists(tmp_path / "no")
    with pytest.raises(SystemExit) as e:                                     # and --deviation still needs a processed mesh
        extract_mesh.main(["--synthetic", "--resolution", "48", "--deviation", "100", "--signed", "--out", str(tmp_path / "no")])
    assert e.value.code == 2 and not os.path.exists(tmp_path / "no")


def test_compare_mesh_refusals_keep_their_order(tmp_path, capsys):
    from instantavatar_amd.drivers import compare_mesh
    with pytest.raises(SystemExit) as e:
        compare_mesh.main([str(tmp_path / "a.ply"), str(tmp_path / "b.ply"), "--signed"])
    assert e.value.code == 2 and "no such file" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        compare_mesh.main(["a.stl", "b.ply", "--signed"])
    assert e.value.code == 2


def test_report_table_prints_the_signed_row_only_with_the_keys():
    from instantavatar_amd import meshdist
    d = dict(mean=1.0, rms=1.0, p50=1.0, p95=1.0, max=1.0)
    rep = dict(a_to_b=dict(d), b_to_a=dict(d), chamfer=1.0, hausdorff=1.0, normal_consistency=1.0, f_score={}, samples=[5, 5])
    plain = meshdist.report_table(rep)
    assert len(plain) == 4 and not any("signed" in r for r in plain)
    rep["a_to_b"].update(signed_mean=-1.0, inside_share=1.0, signed_p05=-1.0, signed_p95=-1.0)
    rows = meshdist.report_table(rep)
    assert len(rows) == 5 and "signed mean -1.00000e+00" in rows[2] and "inside 1.00000" in rows[2] and rows[:2] + rows[3:] == plain
