"""tests/meshops_refs.py, the float64 reference of the mesh processing ("mesh simplification"), is itself checked
here on meshes whose answers are known: a plane, a cube, a sphere.  Then the binding table of include/instantavatar_hip_meshops.h and
what the entry points and the Python layer refuse before anything is launched.  No GPU."""
import os

import numpy as np
import pytest
import torch

import meshops_refs as mo

NAMES = ["ia_mesh_adjacency_build", "ia_mesh_adjacency_workspace_bytes", "ia_mesh_cluster_count", "ia_mesh_cluster_emit",
         "ia_mesh_cluster_workspace_bytes", "ia_mesh_taubin", "ia_mesh_vertex_normals"]
BOX = (np.float32([-1, -1, -1]), np.float32([1, 1, 1]))


def _balanced(faces):
    d = mo.directed_edge_counts(faces)
    return all(d.get((b, a), 0) == c for (a, b), c in d.items())


def _closed_output_ok(out):
    f = out["faces"]
    assert _balanced(f), "a directed edge is used more often than its reverse"
    assert ((f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])).all()
    assert np.array_equal(np.unique(f), np.arange(len(out["verts"]))), "an output vertex that no face references"
    assert (np.abs(out["verts"] - out["centre"]) <= out["half"] * (1 + 1e-12)).all()


@pytest.fixture(scope="module")
def cube37():
    v, f = mo.cube(37, 0.9)
    return v, f, mo.simplify(v, f, None, *BOX, 0.25, 1e-3), mo.simplify(v, f, None, *BOX, 0.25, 1e-3, plain_mean=True)


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def test_cell_index_is_the_fp32_formula():
    lo, h = np.float32([-1, -1, -1]), np.float32(0.25)
    n = mo.grid_dims(lo, np.float32([1, 1, 1]), h)
    assert n.tolist() == [8, 8, 8]
    p = np.float32([[-1, -0.75, 0.999], [1, 5, -7], [-0.7500001, np.nextafter(np.float32(-0.75), np.float32(0)), 0.0]])
    assert mo.cell_index(p, lo, h, n).tolist() == [[0, 1, 7], [7, 7, 0], [0, 1, 4]]       # a vertex ON a cell face belongs to the upper cell
    assert mo.grid_dims([0, 0, 0], [0, 1, 0.26], 0.25).tolist() == [1, 4, 2]


def test_plane_stays_a_plane():
    """every coordinate is a dyadic fraction, so the fp32 vertices lie on z = x / 2 + y / 4 + 1 / 8 exactly: A has rank 1, m lies on
    the plane, and so does the minimiser, to rounding.  (The cell edge is a power of two: with another one fp32(1 / h) puts a vertex
    that lies within an ulp of a cell face into the neighbouring cell, and the clamp then moves it by that ulp.)"""
    v, f = mo.plane_grid(24, (-0.75, -0.75, -0.4375), (0.0625, 0.0, 0.03125), (0.0, 0.0625, 0.015625))
    assert np.array_equal(v[:, 2].astype(np.float64), v[:, 0] / 2.0 + v[:, 1] / 4.0 + 0.125)
    out = mo.simplify(v, f, None, *BOX, 0.25, 1e-3)
    assert len(out["verts"]) > 20 and len(out["faces"]) > 20
    p = out["verts"]
    assert np.abs(p[:, 2] - (p[:, 0] / 2 + p[:, 1] / 4 + 0.125)).max() <= 1e-12 * 2.0


def test_cube_quadric_beats_the_mean_a_hundredfold(cube37):
    v, f, q, mean = cube37
    assert len(v) == 6 * 37 * 37 + 2 and len(f) == 12 * 37 * 37
    dq, dm = mo.cube_surface_distance(q["verts"]).max(), mo.cube_surface_distance(mean["verts"]).max()
    print("cube: quadric %.3g, plain mean %.3g, ratio 1/%.0f" % (dq, dm, dm / dq))
    assert np.array_equal(q["faces"], mean["faces"]) and dq <= dm / 100


def test_icosphere_error_falls_with_the_cell():
    v, f = mo.icosphere(5)
    assert len(v) == 10242
    err = {}
    for cell in (0.1, 0.25):
        out = mo.simplify(v, f, None, np.float32([-1.1] * 3), np.float32([1.1] * 3), cell, 1e-3)
        err[cell] = np.abs(np.linalg.norm(out["verts"], axis=1) - 1).max()
    print("icosphere: radial error %.3g at 0.1, %.3g at 0.25" % (err[0.1], err[0.25]))
    assert err[0.1] < err[0.25] / 4


def test_closed_input_gives_balanced_output(cube37):
    v, f, q, _ = cube37
    q = dict(q, half=0.125)
    _closed_output_ok(q)
    assert len(q["faces"]) < len(f) and len(q["verts"]) < len(v)
    s, g = mo.noisy_icosphere(3)
    for cell in (0.2, 0.45):
        out = mo.simplify(s, g, mo.colours_of(s), np.float32([-1.1] * 3), np.float32([1.1] * 3), cell)
        _closed_output_ok(dict(out, half=np.float64(np.float32(cell)) / 2))
        vc = out["vert_cluster"]
        assert vc.min() >= -1 and vc.max() == len(out["verts"]) - 1
        k = int(vc.max())
        assert np.allclose(out["colors"][k], mo.colours_of(s)[vc == k].astype(np.float64).mean(0), atol=1e-15)


def test_bad_input_is_ignored_by_the_reference():
    v, f = mo.noisy_icosphere(2)
    want = mo.simplify(v, f, None, *BOX, 0.4)
    v2 = np.concatenate([v, np.float32([[np.nan, 0, 0], [0, 0, 0]])])
    nan, lone = len(v), len(v) + 1
    f2 = np.concatenate([f, np.int32([[0, 1, nan], [0, 0, 1], [0, 1, len(v2)], [-1, 2, 3]])])
    got = mo.simplify(v2, f2, None, *BOX, 0.4)
    assert np.array_equal(got["faces"], want["faces"]) and np.array_equal(got["verts"], want["verts"])
    assert got["vert_cluster"][nan] == -1 and got["vert_cluster"][lone] == -1
    assert len(mo.neighbours(v2, f2)[nan]) == 0 and not mo.vertex_normals(v2, f2)[[nan, lone]].any()
    one = mo.simplify(v, f, None, np.float32([-2] * 3), np.float32([2] * 3), 4.0)
    assert len(one["verts"]) == 0 and len(one["faces"]) == 0 and (one["vert_cluster"] == -1).all()


def test_taubin_smooths_without_shrinking():
    v, f = mo.noisy_icosphere(3, 0.02)
    assert len(v) == 642
    out = mo.taubin(v, f, 10)
    shrunk = mo.taubin(v, f, 10, 0.5, 0.5)
    r0, r1 = mo.roughness(v, f), mo.roughness(out, f)
    vol = mo.signed_volume(v, f)
    d_taubin, d_laplace = abs(mo.signed_volume(out, f) - vol), abs(mo.signed_volume(shrunk, f) - vol)
    print("taubin: roughness %.3g -> %.3g, |dV| %.3g against %.3g" % (r0, r1, d_taubin, d_laplace))
    assert r1 < r0 and d_taubin < d_laplace
    assert np.array_equal(mo.taubin(v, f, 0), v)
    assert np.array_equal(mo.taubin(mo.taubin(v, f, 1), f, 1), mo.taubin(v, f, 2))


def test_vertex_normals_of_a_sphere_point_outwards():
    v, f = mo.icosphere(3)
    n = mo.vertex_normals(v, f)
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-12) and (np.einsum("ni,ni->n", n, v.astype(np.float64)) > 0.99).all()


# ---- the binding --------------------------------------------------------------------------------------------------------------------
def test_meshops_header_is_bound():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    d = _lib.declarations("meshops")
    assert sorted(d) == NAMES
    for name in NAMES:
        assert d[name].stream == (not name.endswith("_bytes")), name           # every launching entry point takes a stream
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
    assert "ia_meshops.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_meshops.hip"))
    assert os.path.normpath(_lib.header_path("meshops")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    with pytest.raises(_lib.IAError, match=r"instantavatar_hip_meshops\.h"):
        _lib.call("ia_mesh_edge_collapse")


def test_host_side_argument_errors():
    """what the entry points decide before any launch"""
    from instantavatar_amd import _lib
    L = _lib.lib()
    P = 4096                                                  # (a non-null address that is never read: every call below is refused)
    box = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
    too_many = (2 ** 31 - 1) // 6 + 1
    assert L.ia_mesh_cluster_workspace_bytes(8, 8, 0) == 0 and L.ia_mesh_cluster_workspace_bytes(8, 8, 2 ** 27 + 1) == 0
    assert L.ia_mesh_cluster_workspace_bytes(8, too_many, 8) == 0 and L.ia_mesh_adjacency_workspace_bytes(8, too_many) == 0
    assert L.ia_mesh_adjacency_workspace_bytes(-1, 0) == 0
    nb = L.ia_mesh_cluster_workspace_bytes(8, 8, 512)
    na = L.ia_mesh_adjacency_workspace_bytes(8, 8)
    assert nb > 0 and na > 0
    for h in (0.0, -0.25, float("inf")):
        with pytest.raises(_lib.IAError, match="cell edge"):
            _lib.call("ia_mesh_cluster_count", P, P, 8, 8, *box, h, 4.0, P, nb, P, None)
    with pytest.raises(_lib.IAError, match="cell edge"):
        _lib.call("ia_mesh_cluster_emit", P, P, P, 8, 8, *box, 0.0, 4.0, 1e-3, P, nb, P, 8, P, 8, P, P, None)
    # 2 / 2^-8 = 512 cells per axis = 2^27 in all is the most; a little smaller cell makes 513 per axis
    with pytest.raises(_lib.IAError, match="workspace too small"):
        _lib.call("ia_mesh_cluster_count", P, P, 8, 8, *box, 2.0 ** -8, 256.0, P, nb, P, None)
    with pytest.raises(_lib.IAError, match=r"more than 2\^27"):
        _lib.call("ia_mesh_cluster_count", P, P, 8, 8, *box, 0.0039, 256.0, P, nb, P, None)
    with pytest.raises(_lib.IAError, match=r"more than 2\^27"):
        _lib.call("ia_mesh_cluster_emit", P, P, P, 8, 8, *box, 1e-30, 1e30, 1e-3, P, nb, P, 8, P, 8, P, P, None)
    with pytest.raises(_lib.IAError, match="nf = %d above" % too_many):
        _lib.call("ia_mesh_cluster_count", P, P, 8, too_many, *box, 0.25, 4.0, P, nb, P, None)
    with pytest.raises(_lib.IAError, match="nf = %d above" % too_many):
        _lib.call("ia_mesh_adjacency_build", P, P, 8, too_many, P, na, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_mesh_cluster_count", None, P, 8, 8, *box, 0.25, 4.0, P, nb, P, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_mesh_cluster_count", P, P, 8, 8, *box, 0.25, 4.0, P, nb, None, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_mesh_cluster_emit", P, None, P, 8, 8, *box, 0.25, 4.0, 1e-3, P, nb, P, 8, P, 8, P, P, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_mesh_cluster_emit", P, P, P, 8, 8, *box, 0.25, 4.0, 1e-3, P, nb, None, 8, P, 8, P, P, None)
    with pytest.raises(_lib.IAError, match="reg"):
        _lib.call("ia_mesh_cluster_emit", P, P, P, 8, 8, *box, 0.25, 4.0, 0.0, P, nb, P, 8, P, 8, P, P, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_mesh_adjacency_build", P, None, 8, 8, P, na, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_mesh_taubin", P, 8, 8, None, na, 0.5, -0.53, 1, P, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_mesh_vertex_normals", P, P, 8, 8, P, na, None, None)
    with pytest.raises(_lib.IAError, match="workspace too small"):
        _lib.call("ia_mesh_adjacency_build", P, P, 8, 8, P, na - 1, None)
    with pytest.raises(_lib.IAError, match="workspace too small"):
        _lib.call("ia_mesh_taubin", P, 8, 8, P, na - 1, 0.5, -0.53, 1, 2 * P, None)
    with pytest.raises(_lib.IAError, match="iters = -1"):
        _lib.call("ia_mesh_taubin", P, 8, 8, P, na, 0.5, -0.53, -1, 2 * P, None)
    with pytest.raises(_lib.IAError, match="aliases"):
        _lib.call("ia_mesh_taubin", P, 8, 8, P, na, 0.5, -0.53, 1, P, None)


def test_cpu_tensors_raise():
    from instantavatar_amd import _lib, mesh
    from instantavatar_amd.pipeline import AvatarModel
    f = lambda *s: torch.zeros(s)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    b = lambda *s: torch.zeros(s, dtype=torch.uint8)
    box = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0)
    calls = {
        "ia_mesh_cluster_count": (f(8, 3), i(8, 3), 8, 8, *box, 0.25, 4.0, b(1 << 16), 1 << 16, i(2)),
        "ia_mesh_cluster_emit": (f(8, 3), i(8, 3), f(8, 3), 8, 8, *box, 0.25, 4.0, 1e-3, b(1 << 16), 1 << 16, f(8, 3), 8, i(8, 3), 8, f(8, 3), i(8)),
        "ia_mesh_adjacency_build": (f(8, 3), i(8, 3), 8, 8, b(1 << 16), 1 << 16),
        "ia_mesh_taubin": (f(8, 3), 8, 8, b(1 << 16), 1 << 16, 0.5, -0.53, 1, f(8, 3)),
        "ia_mesh_vertex_normals": (f(8, 3), i(8, 3), 8, 8, b(1 << 16), 1 << 16, f(8, 3)),
    }
    assert set(calls) == {n for n in NAMES if not n.endswith("_bytes")}
    for name, args in calls.items():
        with pytest.raises(_lib.IAError, match="GPU"):
            _lib.call(name, *args, None)
    m = mesh.Mesh(f(8, 3), i(8, 3), f(8, 3), f(8, 3))
    for fn in (lambda: mesh.simplify(m, 0.25), lambda: m.simplify(0.25, (BOX[0], BOX[1])), lambda: mesh.smooth(m), lambda: m.smooth(3),
               lambda: mesh.vertex_normals(m.verts, m.faces)):
        with pytest.raises(_lib.IAError, match="GPU"):
            fn()

    class Net:
        center = torch.zeros(3)

        def _center_scale_host(self):
            return [0.0, 0.0, 0.0], [2.0, 2.0, 2.0]
    model = AvatarModel(None, Net(), None)
    with pytest.raises(_lib.IAError, match="GPU"):
        model.simplify_mesh(m, 0.25)
    with pytest.raises(_lib.IAError, match="GPU"):
        model.smooth_mesh(m, 2)
    with pytest.raises(_lib.IAError, match="cell edge"):
        mesh.cluster_grid(BOX[0], BOX[1], 0.0)
    with pytest.raises(_lib.IAError, match=r"more than 2\^27"):
        mesh.cluster_grid(BOX[0], BOX[1], 0.0039)
    assert mesh.cluster_grid(BOX[0], BOX[1], 2.0 ** -8) == [512, 512, 512] and mesh.cluster_grid([0, 0, 0], [0, 1, 0.26], 0.25) == [1, 4, 2]


def test_the_driver_refuses_bad_flags_before_it_touches_a_device():
    from instantavatar_amd.drivers import extract_mesh as drv
    for argv in (["--synthetic", "--simplify", "0.5"], ["--synthetic", "--smooth", "-1"], ["--synthetic", "--simplify", "-2"]):
        with pytest.raises(SystemExit):
            drv.main(argv)
