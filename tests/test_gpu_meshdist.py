"""The surface distance on the GPU (include/instantavatar_hip_meshdist.h; DESIGN.md section 4, "surface distance") against the float64
references of tests/meshdist_refs.py: closest point of a mesh through triangle grids of several shapes, surface samples, `compare`,
and the two drivers.

Tolerance, derived and not measured: |dist - d_ref| <= 2^-22 (d_ref + L), L = the diagonal of the box around the points and the mesh.
The fp32 rounding of the result is 2^-24 relative; the fp64 evaluation contributes at most sqrt(c 2^-52) L with c <= 64 rounding steps,
which is 2^-23 L; the tolerance doubles this.  The reported face is judged by its meaning -- the reference's distance from the point to
THAT face is within the tolerance of the minimum -- and by its index where the reference's best and second-best faces differ by more
than the tolerance.  Outputs are compared byte for byte across grids, calls and query orders."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import meshdist_refs as md

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("dist", "face", "bary", "point")


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _grid(v, f, cell=None, box=None):
    from instantavatar_amd.meshdist import TriangleGrid
    return TriangleGrid(_dev(v, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3), cell, box)


def _closest(grid, pts, **kw):
    r = grid.closest(_dev(pts, torch.float32), **kw)
    torch.cuda.synchronize()
    return {k: _np(x) for k, x in r.items()}


def _same(a, b, keys=KEYS):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in keys)


def _check(got, ref, pts, v, f, L, D=None):
    """the checks of one result against the reference: distance, the face by its meaning, the closest point; -> the rows whose face
    index the reference decides"""
    pts = np.asarray(pts, np.float32)
    fin = np.isfinite(pts).all(1)
    tol = md.tolerance(np.where(fin, ref["dist"], 0), L)
    assert np.isnan(got["dist"][~fin]).all() and (got["face"][~fin] == -1).all() and (got["bary"][~fin] == 0).all()
    assert got["point"][~fin].tobytes() == pts[~fin].tobytes()
    g = {k: x[fin] for k, x in got.items()}
    r = {k: x[fin] for k, x in ref.items()}
    p, tol = pts[fin].astype(np.float64), tol[fin]
    err = np.abs(g["dist"].astype(np.float64) - r["dist"])
    print("max |dist - ref| / tolerance = %.3g" % (err / tol).max())
    assert (err <= tol).all()
    assert (g["face"] >= 0).all() and (g["face"] < len(f)).all()
    D = md.face_distances2(pts[fin], v, f) if D is None else D[fin]
    assert (np.abs(np.sqrt(D[np.arange(len(p)), g["face"]]) - r["dist"]) <= tol).all()          # the face by its meaning
    t = np.asarray(v, np.float32).astype(np.float64)[np.asarray(f, np.int64)[g["face"]]]
    b = g["bary"].astype(np.float64)
    assert (b >= 0).all() and (np.abs(b.sum(1) - 1) <= 2.0 ** -22).all()                          # on the face
    assert (np.abs((b[:, :, None] * t).sum(1) - g["point"]).max(1) <= tol).all()                   # the barycentric combination
    assert (np.abs(np.linalg.norm(p - g["point"], axis=1) - g["dist"]) <= tol).all()
    clear = md.decided(r, L)
    assert (g["face"][clear] == r["face"][clear]).all()
    out = np.zeros(len(pts), bool)
    out[fin] = clear
    return out


# ---- 1. one triangle --------------------------------------------------------------------------------------------------------------------
def test_one_triangle_all_seven_regions():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = np.int32([[0, 1, 2]])
    cases = [([-0.5, -0.5], [1, 0, 0]), ([2.0, -0.25], [0, 1, 0]), ([-0.25, 2.0], [0, 0, 1]), ([0.25, -1.0], [0.75, 0.25, 0]),
             ([-1.0, 0.75], [0.25, 0, 0.75]), ([1.0, 1.0], [0, 0.5, 0.5]), ([0.25, 0.5], [0.25, 0.25, 0.5])]
    pts = np.float32([[xy[0], xy[1], z] for xy, _ in cases for z in (0.0, 0.5, -2.0)])
    bary = np.float32([b for _, b in cases for _ in range(3)])
    for cell in (None, 0.25, 8.0):
        got = _closest(_grid(v, f, cell), pts)
        want = (bary[:, :, None] * v[None]).sum(1)
        assert got["bary"].tobytes() == bary.tobytes()                # exact, zeros included: every number is dyadic
        assert got["point"].tobytes() == want.astype(np.float32).tobytes() and (got["face"] == 0).all()
        assert got["dist"].tobytes() == np.sqrt(((pts.astype(np.float64) - want) ** 2).sum(1)).astype(np.float32).tobytes()
    ref = md.closest(pts, v, f)
    _check(got, ref, pts, v, f, md.diagonal(pts, v))


# ---- 2. / 3. the icosphere through six grids -----------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _ico():
    v, f = md.icosphere(2)
    pts, n_uniform = md.queries(v, f)
    D = md.face_distances2(np.where(np.isfinite(pts).all(1)[:, None], pts, 0), v, f)
    return v, f, pts, n_uniform, md.closest(pts, v, f), D


ICO_GRIDS = {"1": (4.0, [1, 1, 1], None), "2^3": (1.05, [2, 2, 2], None), "8^3": (0.2625, [8, 8, 8], None),
             "37^3": (2.1 / 37 * 1.0001, [37, 37, 37], None),
             "65^3": (2.1 / 65 * 1.0001, [65, 65, 65], None),      # 274 625 cells = 1 073 workgroups: the scan's carry past 1 024 sums
             "3x11x5": (0.30003, [3, 11, 5], (np.float32([-0.45, -1.65, -0.75]), np.float32([0.45, 1.65, 0.75])))}     # the mesh leaves this box
ICO_POINTS = {"65^3": 512}      # the first so many query points only: a point far from the surface walks ~30 shells of such a grid


def test_icosphere_results_do_not_depend_on_the_grid():
    v, f, pts, _, _, _ = _ico()
    assert len(f) == 320 and len(pts) == 4096
    assert (65 ** 3 + 255) // 256 > 1024                      # why 65: the scan over the cells' counts carries past its first 1 024 sums
    results = {}
    for name, (cell, dims, box) in ICO_GRIDS.items():
        g = _grid(v, f, cell, box or (np.float32([-1.05] * 3), np.float32([1.05] * 3)))
        assert g.dims == dims, (name, g.dims)
        q = pts[:ICO_POINTS.get(name, len(pts))]
        results[name] = _closest(g, q, counters=True)
        again = _closest(g, q, counters=True)
        assert _same(results[name], again, KEYS + ("tests",)), name                                   # a second call: the same bytes
        assert _same(results[name], _closest(g, q, sort=True)), name                                  # and in Morton order
    default = _closest(_grid(v, f), pts)
    for name, r in results.items():
        assert _same(r, {k: default[k][:len(r["dist"])] for k in KEYS}), name
    print("point-triangle tests per point: " + ", ".join("%s: %.1f" % (k, r["tests"].mean()) for k, r in results.items()))


def test_icosphere_against_the_reference():
    """every check of `_check` -- among them: the index of every point whose best and second-best face differ by more than the
    tolerance equals the reference's -- and then the index itself for at least 90 % of the uniform points, decided or not
    (tests/test_cpu_meshdist_refs.py shows from the reference alone that this seed admits it; the decided points alone are 707 of
    3 061, since outside a convex mesh the closest point mostly lies on an edge or a vertex that several faces share)."""
    v, f, pts, n_uniform, ref, D = _ico()
    got = _closest(_grid(v, f, *ICO_GRIDS["8^3"][::2]), pts)
    clear = _check(got, ref, pts, v, f, md.diagonal(pts, v), D)
    same = got["face"][:n_uniform] == ref["face"][:n_uniform]
    print("face index decided by the reference: %d of %d uniform points, %d of all; equal to the reference's: %d of %d uniform points"
          % (clear[:n_uniform].sum(), n_uniform, clear.sum(), same.sum(), n_uniform))
    assert same.mean() >= 0.9, same.mean()


# ---- 4. the cube on cell planes ---------------------------------------------------------------------------------------------------------
def test_cube_with_vertices_and_queries_on_cell_planes():
    v, f = md.cube(8)                                          # vertices at multiples of 0.225 = the cell edge, from lo = -0.9
    k = np.arange(-6, 7, dtype=np.float32)
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3) * np.float32(0.225)          # cube edges and corners included
    planes = (np.float32(-0.9) + np.arange(9, dtype=np.float32) * np.float32(0.225))                        # the cell planes as fp32 forms them
    rng = np.random.RandomState(1)
    on = rng.rand(600, 3).astype(np.float32) * 3 - 1.5
    on[np.arange(600), rng.randint(0, 3, 600)] = planes[rng.randint(0, 9, 600)]
    pts = np.concatenate([lattice, on, v])
    want = md.cube_surface_distance(pts.astype(np.float64), half=np.float64(np.float32(0.9)))
    L = md.diagonal(pts, v)
    first = None
    for cell, box in ((0.225, (np.float32([-0.9] * 3), np.float32([0.9] * 3))), (0.225, (np.float32([-1.125] * 3), np.float32([1.125] * 3))),
                      (0.45, None), (None, None)):
        got = _closest(_grid(v, f, cell, box), pts)
        assert (np.abs(got["dist"].astype(np.float64) - want) <= md.tolerance(want, L)).all()
        first = first or got
        assert _same(got, first)
    _check(first, md.closest(pts, v, f), pts, v, f, L)


# ---- 5. a face over the whole grid, a fan inside, faces that do not count -------------------------------------------------------------------
def test_spanning_face_fan_and_invalid_faces():
    fv, ff = md.fan(7)
    big = np.float32([[-3, -3, -0.5], [3, -3, -0.5], [0, 4, 0.7]])
    v = np.concatenate([fv, big])
    f = np.concatenate([ff, np.int32([[8, 9, 10]])])
    rng = np.random.RandomState(2)
    pts = np.concatenate([(rng.rand(1500, 3) * 4 - 2) * [1, 1, 0.5], v, v[f].mean(1)]).astype(np.float32)
    L = md.diagonal(pts, v)
    base = None
    for cell in (0.11, 0.5, None):
        got = _closest(_grid(v, f, cell), pts, counters=True)
        base = base or got
        assert _same(got, base)
    _check(base, md.closest(pts, v, f), pts, v, f, L)
    # faces that must change nothing: collinear, repeated index, out of range, negative, through a NaN vertex
    nv = len(v)
    v2 = np.concatenate([v, np.float32([[np.nan, 0, 0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]])])
    junk = np.int32([[0, 1, nv], [nv + 1, nv + 2, nv + 3], [2, 2, 3], [0, 1, nv + 4], [-1, 2, 3]])
    f2 = np.concatenate([f[:3], junk[:2], f[3:6], junk[2:], f[6:]])
    index = np.concatenate([np.arange(3), 5 + np.arange(3), 11 + np.arange(2)])                      # face of f -> its row in f2
    assert np.array_equal(f2[index], f)
    for cell in (0.11, None):
        got = _closest(_grid(v2, f2, cell), pts)
        assert _same(got, base, ("dist", "bary", "point")) and np.array_equal(got["face"], index[base["face"]])
    one = _closest(_grid(v2, f2, 100.0), pts, counters=True)
    assert (one["tests"] == len(f)).all()                                                            # the 1-cell grid lists the valid faces only
    none = _closest(_grid(v2, junk), pts[:100], counters=True)
    assert np.isposinf(none["dist"]).all() and (none["face"] == -1).all() and (none["bary"] == 0).all() and (none["tests"] == 0).all()
    assert none["point"].tobytes() == pts[:100].tobytes()
    empty = _closest(_grid(v, np.zeros((0, 3), np.int32)), pts[:5])
    assert np.isposinf(empty["dist"]).all() and (empty["face"] == -1).all()


# ---- 6. pruning is real ------------------------------------------------------------------------------------------------------------------
def test_the_grid_prunes():
    v, f, pts, _, _, _ = _ico()
    fin = np.isfinite(pts).all(1)
    one = _closest(_grid(v, f, 4.0, (np.float32([-1.05] * 3), np.float32([1.05] * 3))), pts, counters=True)
    assert (one["tests"][fin] == len(f)).all() and (one["tests"][~fin] == 0).all()
    v, f = md.icosphere(3)
    rng = np.random.RandomState(7)
    d = rng.standard_normal((4096, 3))
    pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * (1 + 0.05 * (2 * rng.rand(4096, 1) - 1))).astype(np.float32)
    g = _grid(v, f)
    got = _closest(g, pts, counters=True)
    total = int(got["tests"].astype(np.int64).sum())
    print("icosphere(3), default grid %s (cell %.4f): %d tests for %d points x %d faces = %.4f of brute force, %.1f per point"
          % (g.dims, g.cell, total, len(pts), len(f), total / (len(pts) * len(f)), total / len(pts)))
    assert len(f) == 1280 and total < len(pts) * len(f) / 2                                      # (measured: see profiles/meshdist_timing.txt)
    ref = md.closest(pts, v, f)
    _check(got, ref, pts, v, f, md.diagonal(pts, v))


# ---- 7. sampling ---------------------------------------------------------------------------------------------------------------------------
def test_surface_samples():
    from instantavatar_amd import _lib, meshdist
    v, f = md.icosphere(2)
    v = (v.astype(np.float64) * [1.0, 0.6, 1.7]).astype(np.float32)
    n = 4096
    ref = md.sample(v, f, n)
    A = ref["cum"][-1]
    assert np.abs(ref["t"][:, None] - ref["cum"][None, :]).min() > 1e-12 * A          # no sample sits on a boundary of the prefix sum
    mesh = (_dev(v), _dev(f))
    got = {k: _np(x) for k, x in meshdist.sample_surface(mesh, n).items()}
    assert np.array_equal(got["face"], ref["face"])
    assert np.abs(got["bary"].astype(np.float64) - ref["bary"]).max() <= 2.0 ** -22
    t = v.astype(np.float64)[f[got["face"]]]
    scale = np.abs(v).max()
    assert np.abs((ref["bary"][:, :, None] * t).sum(1) - got["points"]).max() <= 2.0 ** -22 * scale
    assert np.abs(ref["points"] - got["points"]).max() <= 2.0 ** -24 * scale
    counts = np.bincount(got["face"], minlength=len(f))
    assert np.abs(counts - n * md.areas(v, f) / A).max() <= 1.0
    again = {k: _np(x) for k, x in meshdist.sample_surface(mesh, n).items()}
    assert _same(got, again, ("points", "face", "bary"))
    one = {k: _np(x) for k, x in meshdist.sample_surface(mesh, 1).items()}
    r1 = md.sample(v, f, 1)
    assert one["face"][0] == r1["face"][0] and np.abs(one["points"] - r1["points"]).max() <= 2.0 ** -24 * scale
    zero = meshdist.sample_surface(mesh, 0)
    assert zero["points"].shape == (0, 3) and zero["face"].shape == (0,) and zero["bary"].shape == (0, 3)
    with pytest.raises(_lib.IAError, match="area"):
        meshdist.sample_surface((_dev(v), _dev(np.int32([[0, 0, 1]]))), 5)
    # invalid faces carry no area and are never chosen
    f2 = np.concatenate([np.int32([[0, 0, 1], [0, 1, 9999]]), f])
    shifted = _np(meshdist.sample_surface((_dev(v), _dev(f2)), n)["face"])
    assert np.array_equal(shifted, ref["face"] + 2)


# ---- 8. compare -----------------------------------------------------------------------------------------------------------------------------
def _close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(abs(a), abs(b))


def test_compare_two_spheres():
    from instantavatar_amd import meshdist
    from instantavatar_amd.mesh import Mesh
    v, f = md.icosphere(3)
    vb = (v.astype(np.float64) * 1.01).astype(np.float32)
    mk = lambda x: Mesh(_dev(x), _dev(f), torch.zeros((len(x), 3), device=DEV), torch.zeros((len(x), 3), device=DEV))
    a, b = mk(v), mk(vb)
    n, taus = 20000, (0.005, 0.0095, 0.02)
    rep = a.compare(b, samples=n, taus=taus)
    sa, sb = meshdist.sample_surface(a, n), meshdist.sample_surface(b, n)
    ra, rb = meshdist.TriangleGrid(b.verts, b.faces).closest(sa["points"]), meshdist.TriangleGrid(a.verts, a.faces).closest(sb["points"])
    na, nb = md.unit_normals(v, f), md.unit_normals(vb, f)
    cons = lambda n_src, s, n_dst, r: np.abs((n_src[_np(s["face"])] * n_dst[_np(r["face"])]).sum(1))
    want = md.report(_np(ra["dist"]), _np(rb["dist"]), cons(na, sa, nb, ra), cons(nb, sb, na, rb), taus)
    for d in ("a_to_b", "b_to_a"):
        for k in ("mean", "rms", "p50", "p95", "max"):
            assert _close(rep[d][k], want[d][k]), (d, k, rep[d][k], want[d][k])
    for k in ("chamfer", "hausdorff", "normal_consistency"):
        assert _close(rep[k], want[k]), (k, rep[k], want[k])
    assert set(rep["f_score"]) == set(want["f_score"]) and all(_close(rep["f_score"][t], want["f_score"][t]) for t in want["f_score"])
    assert rep["samples"] == [n, n] and rep["chamfer"] == (rep["a_to_b"]["mean"] + rep["b_to_a"]["mean"]) / 2
    assert 0.005 < rep["chamfer"] < 0.0101 and rep["hausdorff"] <= 0.0101 + 1e-6 and rep["normal_consistency"] > 0.999
    assert rep["f_score"][0.02] == 1.0 and rep["f_score"][0.005] == 0.0
    # against the reference distances themselves, for a part of the samples
    ref = md.closest(_np(sa["points"])[:512], vb, f)
    assert (np.abs(_np(ra["dist"])[:512] - ref["dist"]) <= md.tolerance(ref["dist"], md.diagonal(vb))).all()
    swapped = b.compare(a, samples=n, taus=taus)
    assert swapped["b_to_a"] == rep["a_to_b"] and swapped["a_to_b"] == rep["b_to_a"]                # exactly
    assert swapped["chamfer"] == rep["chamfer"] and swapped["normal_consistency"] == rep["normal_consistency"]
    L = md.diagonal(v)
    for samples in (n, 0):
        own = a.compare(a, samples=samples)
        assert own["hausdorff"] <= 2.0 ** -22 * L, own["hausdorff"]
    assert np.isnan(own["normal_consistency"]) and own["samples"] == [len(v), len(v)]
    back = meshdist.interpolate(b.verts, b.faces, ra["face"], ra["bary"])
    assert back.dtype == torch.float32
    # bary and point are both roundings of the fp64 values: three products of a 2^-24 error and a coordinate, and two roundings
    assert float((back - ra["point"]).abs().max()) <= 5 * 2.0 ** -24 * float(np.abs(vb).max())
    per_vertex = a.distance_to(b)
    assert per_vertex["dist"].shape == (len(v),) and float(per_vertex["dist"].max()) <= 0.0101
    colours = meshdist.heat(per_vertex["dist"], 0.02)
    assert colours.shape == (len(v), 3) and float(colours.min()) >= 0 and float((colours.sum(1) - 1).abs().max()) < 1e-6


# ---- 9. drivers ---------------------------------------------------------------------------------------------------------------------------
def test_drivers(tmp_path, capsys):
    from instantavatar_amd import mesh as M
    from instantavatar_amd.drivers import compare_mesh, extract_mesh
    from instantavatar_amd.pipeline import build_synthetic_model
    common = ["--synthetic", "--resolution", "48", "--simplify", "3", "--render", "64"]
    assert extract_mesh.main(common + ["--out", str(tmp_path / "plain")]) == 0
    plain_out = capsys.readouterr().out
    assert extract_mesh.main(common + ["--deviation", "2000", "--out", str(tmp_path / "dev")]) == 0
    out = capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "dev")) == sorted(os.listdir(tmp_path / "plain") + ["deviation.json", "deviation_front.png"])
    assert "deviation:" not in plain_out and out.count("deviation:") == 1 and "spacings" in out
    for name in os.listdir(tmp_path / "plain"):
        if name.endswith(".ply"):
            assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "dev" / name, "rb").read()
    rep = json.load(open(tmp_path / "dev" / "deviation.json"))
    model = build_synthetic_model(DEV, seed=42)[0]
    model.eval()
    extracted = model.extract_mesh(resolution=48, level=10.0, largest=True)
    lo, hi = M.field_box(model.net_coarse)
    spacing = float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / 47
    final = model.simplify_mesh(extracted, 3 * spacing)
    want = extracted.compare(final, samples=2000)
    for k in ("a_to_b", "b_to_a", "chamfer", "hausdorff", "normal_consistency"):
        assert rep[k] == want[k], k
    assert rep["resolution"] == 48 and rep["samples"] == 2000 and rep["spacing"] == spacing
    assert rep["extracted"] == dict(vertices=extracted.verts.shape[0], faces=extracted.faces.shape[0])
    assert rep["processed"] == dict(vertices=final.verts.shape[0], faces=final.faces.shape[0])
    assert 0 < rep["chamfer"] < 3 * spacing
    from PIL import Image
    img = np.asarray(Image.open(tmp_path / "dev" / "deviation_front.png"))
    assert img.shape == (64, 64, 4) and (img[..., 3] > 0).sum() > 50
    # compare_mesh reproduces the report from files
    extracted.to_ply(str(tmp_path / "extracted.ply"))
    argv = [str(tmp_path / "extracted.ply"), str(tmp_path / "dev" / "canonical.ply"), "--samples", "2000", "--tau", "0.01", "--out", str(tmp_path / "cmp")]
    assert compare_mesh.main(argv) == 0
    table = capsys.readouterr().out
    assert "chamfer" in table and "a_to_b" in table and "F-score at tau = 0.01" in table
    got = json.load(open(tmp_path / "cmp" / "compare.json"))
    for k in ("a_to_b", "b_to_a", "chamfer", "hausdorff", "normal_consistency"):
        assert got[k] == rep[k], k
    assert sorted(os.listdir(tmp_path / "cmp")) == ["a_error.ply", "b_error.ply", "compare.json"]
    err = M.Mesh.from_ply(str(tmp_path / "cmp" / "a_error.ply"), DEV)
    assert torch.equal(err.verts, extracted.verts) and torch.equal(err.faces, extracted.faces)
    with pytest.raises(SystemExit) as e:
        extract_mesh.main(["--synthetic", "--resolution", "48", "--deviation", "2000", "--out", str(tmp_path / "no")])
    assert e.value.code == 2 and "--deviation" in capsys.readouterr().err and not os.path.exists(tmp_path / "no")
