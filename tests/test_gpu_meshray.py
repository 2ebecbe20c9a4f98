"""The ray queries on the GPU (include/instantavatar_hip_meshray.h; DESIGN.md section 4, "ray queries") against the float64 brute force
of tests/meshray_refs.py: first hit and hit count through triangle grids of several shapes, the inside test, signed distances, the signed
`compare`, and the two drivers.

Outputs are compared byte for byte across grids, calls, ray orders and prefixes: the grid only prunes.  Against the reference, hit / miss,
the face and the count are compared on every CLEAR ray (meshray_refs.unclear; tests/test_cpu_meshray_refs.py shows that the rays used
here are all clear), and |t - fp32(t_ref)| <= 2^-23 |t_ref| + 1e-9 (L + |o|) / |d|, L the mesh diagonal: one rounding to fp32 plus a
generous bound on fp64 differences -- from the rounding model, not from a measurement."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import meshdist_refs as md
import meshray_refs as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("t", "face", "bary", "point")


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _grid(v, f, cell=None, box=None):
    from instantavatar_amd.meshdist import TriangleGrid
    return TriangleGrid(_dev(v, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3), cell, box)


def _opt(x):
    return None if x is None else (x if np.isscalar(x) else _dev(np.asarray(x, np.float32)))


def _cast(grid, o, d, t_min=None, t_max=None, **kw):
    r = grid.raycast(_dev(o, torch.float32), _dev(d, torch.float32), _opt(t_min), _opt(t_max), **kw)
    torch.cuda.synchronize()
    return {k: _np(x) for k, x in r.items()}


def _count(grid, o, d, t_min=None, t_max=None, **kw):
    r = grid.count_hits(_dev(o, torch.float32), _dev(d, torch.float32), _opt(t_min), _opt(t_max), **kw)
    torch.cuda.synchronize()
    return {k: _np(x) for k, x in r.items()}


def _same(a, b, keys=KEYS):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in keys)


def _dirs():
    from instantavatar_amd import _lib
    with open(_lib.header_path("meshray")) as f:
        return mr.inside_dirs(f.read())


# ---- 1. one triangle, dyadic numbers, exact bytes -------------------------------------------------------------------------------------------
def test_one_triangle_exact():
    v = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    f = np.int32([[0, 1, 2]])
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    xy = [(0.25, 0.25), (0.125, 0.5), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.0, 0.0), (1.0, 0.0), (0.0, 1.0)]     # interior, edges, vertices
    rows = []      # (o, d, t_min, t_max, t, face, bary, count)
    for x, y in xy:
        b = (1 - x - y, x, y)
        rows.append(((x, y, 1), (0, 0, -1), 0, inf, 1.0, 0, b, 1))                           # from above
        rows.append(((x, y, -1), (0, 0, 2), 0, inf, 0.5, 0, b, 1))                           # from below, t in units of d
    miss = lambda o, d, t0=0, t1=inf: rows.append((o, d, t0, t1, inf, -1, (0, 0, 0), 0))
    bad = lambda o, d, t0=0, t1=inf: rows.append((o, d, t0, t1, nan, -1, (0, 0, 0), -1))
    miss((0.75, 0.75, 1), (0, 0, -1))                                                        # beside the triangle
    miss((0.25, 0.25, 0.5), (1, 0, 0))                                                       # parallel to the plane: det = 0
    miss((-1, 0.25, 0), (1, 0, 0))                                                           # in the plane: det = 0
    miss((0.25, 0.25, 1), (0, 0, 1))                                                         # behind the origin
    miss((0.25, 0.25, 1), (0, 0, 0))                                                         # no direction
    up, down = np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(1), np.float32(0))
    rows.append(((0.25, 0.25, 1), (0, 0, -1), 1.0, inf, 1.0, 0, (0.5, 0.25, 0.25), 1))       # t = t_min
    rows.append(((0.25, 0.25, 1), (0, 0, -1), 0, 1.0, 1.0, 0, (0.5, 0.25, 0.25), 1))         # t = t_max
    rows.append(((0.25, 0.25, 1), (0, 0, -1), 1.0, 1.0, 1.0, 0, (0.5, 0.25, 0.25), 1))
    miss((0.25, 0.25, 1), (0, 0, -1), up, inf)                                               # one ulp outside
    miss((0.25, 0.25, 1), (0, 0, -1), 0, down)
    miss((0.25, 0.25, 1), (0, 0, -1), inf, inf)
    bad((nan, 0.25, 1), (0, 0, -1))
    bad((0.25, 0.25, 1), (0, inf, -1))
    bad((0.25, 0.25, 1), (0, 0, -1), nan, inf)
    bad((0.25, 0.25, 1), (0, 0, -1), 0, nan)
    bad((0.25, 0.25, 1), (0, 0, -1), 2.0, 1.0)
    bad((0.25, 0.25, 1), (0, 0, -1), -1.0, 1.0)
    o, d = np.float32([r[0] for r in rows]), np.float32([r[1] for r in rows])
    t0, t1 = np.float32([r[2] for r in rows]), np.float32([r[3] for r in rows])
    t, face, bary, cnt = np.float32([r[4] for r in rows]), np.int32([r[5] for r in rows]), np.float32([r[6] for r in rows]), np.int32([r[7] for r in rows])
    point = np.where(face[:, None] >= 0, (bary[:, :, None] * v[None]).sum(1), o).astype(np.float32)
    ref = mr.closest(o, d, v, f, t0, t1)
    assert np.array_equal(ref["t"].astype(np.float32), t, equal_nan=True) and np.array_equal(ref["face"], face)      # the table above is the reference's
    assert np.array_equal(mr.count(o, d, v, f, t0, t1), cnt) and np.array_equal(ref["bary"], bary)
    bary = ref["bary"].astype(np.float32)                     # exact, and the reference's bytes: a zero weight may be -0 (u, v carry the sign of 1 / det)
    for cell in (None, 0.25, 8.0):
        g = _grid(v, f, cell)
        got = _cast(g, o, d, t0, t1, counters=True)
        assert got["t"].tobytes() == t.tobytes() and np.array_equal(got["face"], face), cell
        assert got["bary"].tobytes() == bary.tobytes() and np.array_equal(got["point"], point, equal_nan=True), cell
        assert (got["tests"][np.isnan(t)] == 0).all()
        for limit in (None, 1, 3):
            assert np.array_equal(_count(g, o, d, t0, t1, limit=limit)["count"], cnt), (cell, limit)
        none = _cast(g, o[:0], d[:0])
        assert none["t"].shape == (0,) and none["point"].shape == (0, 3) and _count(g, o[:0], d[:0])["count"].shape == (0,)
    # the default range, and one direction for all rays
    g = _grid(v, f)
    r = g.raycast(_dev(o[:16:2]), _dev(np.float32([0, 0, -1])))
    assert _np(r["t"]).tobytes() == t[:16:2].tobytes()


# ---- 2. / 3. the icosphere through seven grids ---------------------------------------------------------------------------------------------
BOX = (np.float32([-1.05] * 3), np.float32([1.05] * 3))
ICO_GRIDS = {"1": (4.0, [1, 1, 1], BOX), "2^3": (1.05, [2, 2, 2], BOX), "8^3": (0.2625, [8, 8, 8], BOX),
             "65^3": (2.1 / 65 * 1.0001, [65, 65, 65], BOX),       # 274 625 cells: the cell scan carries past its first block
             "3x11x5": (0.30003, [3, 11, 5], (np.float32([-0.45, -1.65, -0.75]), np.float32([0.45, 1.65, 0.75]))),     # anisotropic; the mesh leaves this box
             "small": (0.125, [6, 6, 6], (np.float32([-0.375] * 3), np.float32([0.375] * 3)))}                                # every face clamped into boundary cells
LIMITS = (1, 2, None)


@functools.lru_cache(None)
def _ico():
    v, f = mr.icosphere(2)
    o, d = mr.probe_rays()
    H = mr.hits(o, d, v, f)
    return v, f, o, d, H


def test_icosphere_results_do_not_depend_on_the_grid():
    v, f, o, d, _ = _ico()
    assert len(f) == 320 and len(o) == 4096
    default = _grid(v, f)
    assert default.faces_inside == 1
    base = _cast(default, o, d)
    base_n = {lim: _count(default, o, d, limit=lim)["count"] for lim in LIMITS}
    for name, (cell, dims, box) in ICO_GRIDS.items():
        g = _grid(v, f, cell, box)
        assert g.dims == dims and g.faces_inside == 0, (name, g.dims)
        got = _cast(g, o, d, counters=True)
        assert _same(got, base), name                                                                  # no output but `tests` knows the grid
        assert _same(got, _cast(g, o, d, counters=True), KEYS + ("tests",)), name                      # a second call: the same bytes
        assert _same(got, _cast(g, o, d, counters=True, sort=True), KEYS + ("tests",)), name           # in Morton order
        head = _cast(g, o[:1000], d[:1000], counters=True)
        assert _same(head, {k: x[:1000] for k, x in got.items()}, KEYS + ("tests",)), name             # a prefix of the rays
        for lim in LIMITS:
            n = _count(g, o, d, limit=lim, counters=True)
            assert n["count"].tobytes() == base_n[lim].tobytes(), (name, lim)
            assert _same(n, _count(g, o, d, limit=lim, counters=True), ("count", "tests")), (name, lim)
            assert _same(n, _count(g, o, d, limit=lim, counters=True, sort=True), ("count", "tests")), (name, lim)
            assert _same(_count(g, o[:1000], d[:1000], limit=lim), {"count": n["count"][:1000]}, ("count",)), (name, lim)
    assert _same(base, _cast(default, o, d, sort=True)) and _same(base, _cast(default, o, d, sort=False))
    assert np.array_equal(base_n[1], np.minimum(base_n[None], 1)) and np.array_equal(base_n[2], np.minimum(base_n[None], 2))


def test_icosphere_against_the_reference():
    v, f, o, d, H = _ico()
    ref = mr.closest(o, d, v, f, H=H)
    clear = ~mr.unclear(o, d, v, f, H=H)
    assert (~clear).mean() <= 0.01
    L = md.diagonal(v)
    got = _cast(_grid(v, f), o, d)
    hit = ref["face"] >= 0
    assert np.array_equal(got["face"][clear], ref["face"][clear])
    assert np.array_equal(np.isfinite(got["t"])[clear], hit[clear]) and np.isposinf(got["t"][clear & ~hit]).all()
    both = hit & (got["face"] >= 0)
    tol = mr.t_tolerance(ref["t"][both], o[both], d[both], L)
    err = np.abs(got["t"][both].astype(np.float64) - ref["t"][both].astype(np.float32).astype(np.float64))
    print("hits: %d of %d rays, unclear: %d; max |t - ref| / tolerance = %.3g" % (hit.sum(), len(o), (~clear).sum(), (err / tol).max()))
    assert (err <= tol).all()
    b = got["bary"].astype(np.float64)
    assert (b >= 0).all() and (np.abs(b.sum(1) - 1)[both] <= 2.0 ** -22).all() and (b[got["face"] < 0] == 0).all()
    at = o.astype(np.float64) + got["t"].astype(np.float64)[:, None] * d.astype(np.float64)
    assert (np.abs(got["point"][both] - at[both]).max(1) <= 2.0 ** -22 * L).all()
    assert got["point"][got["face"] < 0].tobytes() == o[got["face"] < 0].tobytes()
    for lim in LIMITS:
        n = _count(_grid(v, f), o, d, limit=lim)["count"]
        assert np.array_equal(n[clear], mr.count(o, d, v, f, limit=lim, H=H)[clear]), lim
    # a range per ray: the far half of each ray only
    t0 = np.where(hit, ref["t"] * 1.5, 0.5).astype(np.float32)
    H2 = mr.hits(o, d, v, f, t0, None)
    clear2 = ~mr.unclear(o, d, v, f, t0, None, H=H2)
    r2, g2 = mr.closest(o, d, v, f, t0, None, H=H2), _cast(_grid(v, f, 0.2625, BOX), o, d, t0)
    assert (~clear2).mean() <= 0.01 and np.array_equal(g2["face"][clear2], r2["face"][clear2])
    assert np.array_equal(_count(_grid(v, f), o, d, t0)["count"][clear2], mr.count(o, d, v, f, t0, None, H=H2)[clear2])


# ---- 4. the cube on cell planes -----------------------------------------------------------------------------------------------------------
def test_cube_rays_along_cell_planes_and_through_edges():
    v, f = mr.cube(8, half=1.0)                                                                 # vertices at multiples of 0.25: every number is dyadic
    o, d = mr.cube_rays()
    H = mr.hits(o, d, v, f)
    ref, n_ref = mr.closest(o, d, v, f, H=H), mr.count(o, d, v, f, H=H)
    want = mr.slab_hit(o, d, 1.0)
    assert np.array_equal(ref["t"], want)                                                       # exact: the reference's t IS the slab test's
    tied = (H["hit"] & (H["t"] == ref["t"][:, None])).sum(1)
    assert (tied >= 2).sum() > 400 and (tied >= 4).sum() > 50                                   # edges and vertices of the triangulation
    one = (np.float32([-1.0] * 3), np.float32([1.0] * 3))
    first = None
    for cell, box in ((0.25, one), (0.25, (np.float32([-1.25] * 3), np.float32([1.25] * 3))), (0.5, None), (None, None), (4.0, one),
                      (0.25, (np.float32([-0.5] * 3), np.float32([0.5] * 3)))):
        g = _grid(v, f, cell, box)
        got = _cast(g, o, d)
        got["count"] = _count(g, o, d)["count"]
        first = first or got
        assert _same(got, first, KEYS + ("count",)), (cell, box)
    assert np.array_equal(first["t"], want.astype(np.float32))
    assert np.array_equal(first["face"], ref["face"])                                           # the smallest index among the tied faces
    assert np.array_equal(first["count"], n_ref)


# ---- 5. a face over the whole grid, a fan inside, faces that do not count, a permuted order -----------------------------------------------
def test_spanning_face_fan_invalid_faces_and_permutation():
    fv, ff = mr.fan(7)
    big = np.float32([[-3, -3, -0.5], [3, -3, -0.5], [0, 4, 0.7]])
    v = np.concatenate([fv, big])
    f = np.concatenate([ff, np.int32([[8, 9, 10]])])
    rng = np.random.default_rng(2)
    o = np.concatenate([rng.uniform(-2, 2, (1500, 3)) * [1, 1, 0.5] + [0, 0, 2], rng.uniform(-1, 1, (500, 3))]).astype(np.float32)
    d = (rng.uniform(-1, 1, (2000, 3)) * [1, 1, 0.3] - o * [0, 0, 1]).astype(np.float32)
    H = mr.hits(o, d, v, f)
    ref, clear = mr.closest(o, d, v, f, H=H), ~mr.unclear(o, d, v, f, H=H)
    assert (~clear).mean() <= 0.01 and (ref["face"] >= 0).mean() > 0.3
    base = None
    for cell in (0.11, 0.5, None):
        g = _grid(v, f, cell)
        got = _cast(g, o, d)
        got["count"] = _count(g, o, d)["count"]
        base = base or got
        assert _same(got, base, KEYS + ("count",)), cell
    assert np.array_equal(base["face"][clear], ref["face"][clear]) and np.array_equal(base["count"][clear], mr.count(o, d, v, f, H=H)[clear])
    # faces that must change nothing: collinear, repeated index, out of range, negative, through a NaN vertex -- and another order
    nv = len(v)
    v2 = np.concatenate([v, np.float32([[np.nan, 0, 0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0], [1.5, 1.5, 1.5]])])
    junk = np.int32([[0, 1, nv], [nv + 1, nv + 2, nv + 3], [2, 2, 3], [0, 1, nv + 4], [-1, 2, 3]])
    perm = np.random.default_rng(3).permutation(len(f))
    f2 = np.concatenate([f[perm][:3], junk[:2], f[perm][3:6], junk[2:], f[perm][6:]])
    row = np.concatenate([np.arange(3), 5 + np.arange(3), 11 + np.arange(2)])                    # row of f[perm] -> its row in f2
    index = np.empty(len(f), np.int64)
    index[perm] = row                                                                            # face of f -> its row in f2
    assert np.array_equal(f2[index], f)
    for cell in (0.11, None):
        g = _grid(v2, f2, cell)
        got = _cast(g, o, d)
        assert _same(got, base, ("t",)) and np.array_equal(got["face"][clear], np.where(base["face"] >= 0, index[base["face"]], -1)[clear])
        assert np.array_equal(_count(g, o, d)["count"], base["count"])
    one = _cast(_grid(v2, f2, 100.0, (np.float32([-4] * 3), np.float32([4] * 3))), o, d, counters=True)
    assert (one["tests"] == len(f)).all()                                                        # the 1-cell grid lists the valid faces only
    for mesh in ((v2, junk), (v, np.zeros((0, 3), np.int32))):
        g = _grid(*mesh)
        none = _cast(g, o[:100], d[:100], counters=True)
        assert np.isposinf(none["t"]).all() and (none["face"] == -1).all() and (none["bary"] == 0).all() and (none["tests"] == 0).all()
        assert none["point"].tobytes() == o[:100].tobytes() and (_count(g, o[:100], d[:100])["count"] == 0).all()


# ---- 6. pruning is real --------------------------------------------------------------------------------------------------------------------
def test_the_grid_prunes():
    v, f = mr.icosphere(3)
    o, d = mr.probe_rays()
    o, d = o[:2048], d[:2048]                                                                    # the rays from outside
    P, nf = len(o), len(f)
    g = _grid(v, f)
    first = _cast(g, o, d, counters=True)["tests"].astype(np.int64)
    every = _count(g, o, d, counters=True)["tests"].astype(np.int64)
    any_hit = _count(g, o, d, limit=1, counters=True)["tests"].astype(np.int64)
    print("icosphere(3), default grid %s: tests per ray: first hit %.1f, count %.1f, any-hit %.1f (brute force: %d)"
          % (g.dims, first.mean(), every.mean(), any_hit.mean(), nf))
    assert nf == 1280 and first.sum() < P * nf / 4 and every.sum() < P * nf / 4
    assert first.sum() < every.sum() and any_hit.sum() <= first.sum()
    one = _grid(v, f, 4.0, BOX)
    assert (_cast(one, o, d, counters=True)["tests"] == nf).all() and (_count(one, o, d, counters=True)["tests"] == nf).all()


# ---- 7. the inside test and the signed distance --------------------------------------------------------------------------------------------
def _contain_points(grid, keep, seed):
    """points in [-1.6, 1.6]^3 (beyond the box as well), a third of them with one coordinate on a plane of the grid's cells"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.6, 1.6, (3000, 3)).astype(np.float32)
    axis = rng.integers(0, 3, 1000)
    step = (rng.uniform(0, 1, 1000) * (np.asarray(grid.dims)[axis] + 1)).astype(np.int64).astype(np.float32)
    p[np.arange(1000), axis] = np.asarray(grid.lo, np.float32)[axis] + step * np.float32(grid.cell)          # a plane as fp32 forms it
    p = np.concatenate([p, np.float32([[0, 0, 0], [np.nan, 0, 0], [0, np.inf, 0]])])
    with np.errstate(invalid="ignore"):
        return p[keep(p.astype(np.float64)) | ~np.isfinite(p).all(1)]


def test_contains_and_signed_distance():
    dirs = _dirs()
    r = lambda p: np.linalg.norm(p, axis=1)
    c = lambda p: np.abs(p).max(1)
    cases = [(mr.icosphere(2), lambda p: (r(p) < 0.9) | (r(p) > 1.05), lambda p: r(p) < 0.9),
             (mr.cube(8, half=1.0), lambda p: (c(p) < 0.95) | (c(p) > 1.05), lambda p: c(p) < 0.95),
             (mr.shell(), lambda p: (r(p) < 0.44) | ((r(p) > 0.55) & (r(p) < 0.9)) | (r(p) > 1.05), lambda p: (r(p) > 0.55) & (r(p) < 0.9))]
    for (v, f), keep, inside in cases:
        g = _grid(v, f)
        p = _contain_points(g, keep, len(f))
        fin = np.isfinite(p).all(1)
        with np.errstate(invalid="ignore"):
            want = inside(p.astype(np.float64)) & fin
        assert fin.sum() > 1000 and 0.02 < want.mean() < 0.9
        assert np.array_equal(mr.contains(p[fin], v, f, dirs), want[fin])                          # the reference meets the analytic answer
        got = _np(g.contains(_dev(p)))
        assert got.dtype == bool and np.array_equal(got, want)
        for cell in (0.37, 4.0):
            assert np.array_equal(_np(_grid(v, f, cell, BOX).contains(_dev(p))), want)
        sd, cl = g.signed_distance(_dev(p)), g.closest(_dev(p))
        assert np.array_equal(_np(sd["inside"]), want)
        assert np.array_equal(_np(sd["dist"]), np.where(want, -_np(cl["dist"]), _np(cl["dist"])), equal_nan=True)
        assert all(torch.equal(sd[k], cl[k]) for k in ("face", "bary"))
    from instantavatar_amd.mesh import Mesh
    (v, f), p = cases[0][0], np.float32([[0, 0, 0], [2, 0, 0], [0.5, 0.5, 0.5]])
    m = Mesh(_dev(v), _dev(f), None, None)
    assert _np(m.contains(_dev(p))).tolist() == [True, False, True]
    hit = m.raycast(_dev(p), _dev(np.float32([1, 0, 0])))
    assert _np(hit["face"]).tolist()[1] == -1 and abs(float(hit["t"][0]) - 1) < 0.02
    blocked = _grid(v, f).occluded(_dev(np.float32([[0, 0, 0], [0, 0, 0], [2, 0, 0], [np.nan, 0, 0]])),
                                   _dev(np.float32([[0.5, 0, 0], [2, 0, 0], [-2, 0.1, 0], [1, 1, 1]])))
    assert _np(blocked).tolist() == [False, True, True, False]
    small = Mesh(_dev(v * np.float32(0.5)), _dev(f), None, None)
    sd = small.signed_distance_to(m)
    assert bool(sd["inside"].all()) and float(sd["dist"].max()) < -0.4


# ---- 8. compare(signed=True) ---------------------------------------------------------------------------------------------------------------
def test_signed_compare_two_spheres():
    from instantavatar_amd import meshdist
    from instantavatar_amd.mesh import Mesh
    v, f = md.icosphere(3)
    vb = (v.astype(np.float64) * 1.01).astype(np.float32)
    mk = lambda x: Mesh(_dev(x), _dev(f), torch.zeros((len(x), 3), device=DEV), torch.zeros((len(x), 3), device=DEV))
    a, b = mk(v), mk(vb)
    n, taus = 20000, (0.005, 0.02)
    plain, rep = a.compare(b, samples=n, taus=taus), a.compare(b, samples=n, taus=taus, signed=True)
    extra = {"signed_mean", "inside_share", "signed_p05", "signed_p95"}
    for d in ("a_to_b", "b_to_a"):
        assert set(rep[d]) == set(plain[d]) | extra and all(rep[d][k] == plain[d][k] for k in plain[d]), d      # bit for bit
    assert all(rep[k] == plain[k] for k in plain if k not in ("a_to_b", "b_to_a")) and set(rep) == set(plain)
    ab, ba = rep["a_to_b"], rep["b_to_a"]
    assert abs(ab["signed_mean"] + ab["mean"]) <= 1e-9 * ab["mean"] and abs(ba["signed_mean"] - ba["mean"]) <= 1e-9 * ba["mean"]
    assert ab["inside_share"] == 1.0 and ba["inside_share"] == 0.0
    assert -0.0101 <= ab["signed_p05"] <= ab["signed_p95"] < 0 < ba["signed_p05"] <= ba["signed_p95"] <= 0.0101
    rows, rows_plain = meshdist.report_table(rep), meshdist.report_table(plain)
    assert len(rows) == len(rows_plain) + 2 and [r for r in rows if "signed mean" not in r] == rows_plain
    assert meshdist.compare(a, b, n, taus, signed=True) == rep


# ---- 9. drivers ------------------------------------------------------------------------------------------------------------------------------
def test_drivers_signed(tmp_path, capsys):
    from instantavatar_amd.drivers import compare_mesh, extract_mesh
    common = ["--synthetic", "--resolution", "48", "--simplify", "3", "--deviation", "2000"]
    assert extract_mesh.main(common + ["--out", str(tmp_path / "dev")]) == 0
    plain_out = capsys.readouterr().out
    assert extract_mesh.main(common + ["--signed", "--out", str(tmp_path / "sgn")]) == 0
    out = capsys.readouterr().out
    assert "bias:" not in plain_out and out.count("bias:") == 1 and "spacings" in out.split("bias:")[1].splitlines()[0]
    assert [ln for ln in out.splitlines() if ln.startswith("deviation:")] == [ln for ln in plain_out.splitlines() if ln.startswith("deviation:")]
    assert len(out.splitlines()) == len(plain_out.splitlines()) + 1
    assert sorted(os.listdir(tmp_path / "dev")) == sorted(os.listdir(tmp_path / "sgn"))
    for name in os.listdir(tmp_path / "dev"):
        if name != "deviation.json":
            assert open(tmp_path / "dev" / name, "rb").read() == open(tmp_path / "sgn" / name, "rb").read(), name
    plain, rep = json.load(open(tmp_path / "dev" / "deviation.json")), json.load(open(tmp_path / "sgn" / "deviation.json"))
    extra = {"signed_mean", "inside_share", "signed_p05", "signed_p95"}
    for d in ("a_to_b", "b_to_a"):
        assert not extra & set(plain[d]) and set(rep[d]) == set(plain[d]) | extra
        assert {k: x for k, x in rep[d].items() if k not in extra} == plain[d]
        assert abs(rep[d]["signed_mean"]) <= rep[d]["mean"] and 0.0 <= rep[d]["inside_share"] <= 1.0
    assert {k: x for k, x in rep.items() if k not in ("a_to_b", "b_to_a")} == {k: x for k, x in plain.items() if k not in ("a_to_b", "b_to_a")}
    line = [ln for ln in out.splitlines() if ln.startswith("bias:")][0]
    assert "%+.3e" % rep["b_to_a"]["signed_mean"] in line and "%.1f %%" % (100 * rep["b_to_a"]["inside_share"]) in line
    # compare_mesh on the written files
    argv = [str(tmp_path / "dev" / "canonical.ply"), str(tmp_path / "sgn" / "canonical.ply"), "--samples", "2000"]
    assert compare_mesh.main(argv + ["--out", str(tmp_path / "c0")]) == 0
    t0 = capsys.readouterr().out
    assert compare_mesh.main(argv + ["--signed", "--out", str(tmp_path / "c1")]) == 0
    t1 = capsys.readouterr().out
    assert "signed mean" not in t0 and t1.count("signed mean") == 2
    strip = lambda text: [ln for ln in text.splitlines() if "signed mean" not in ln and not ln.startswith("wrote")]
    assert strip(t0) == strip(t1)
    j0, j1 = json.load(open(tmp_path / "c0" / "compare.json")), json.load(open(tmp_path / "c1" / "compare.json"))
    assert not extra & set(j0["a_to_b"]) and extra <= set(j1["a_to_b"]) and extra <= set(j1["b_to_a"])
    assert all(j1["a_to_b"][k] == j0["a_to_b"][k] for k in j0["a_to_b"]) and j1["chamfer"] == j0["chamfer"]
    for name in ("a_error.ply", "b_error.ply"):
        assert open(tmp_path / "c0" / name, "rb").read() == open(tmp_path / "c1" / name, "rb").read()
