"""What the mesh extraction promises without a GPU: the committed marching-tetrahedra table is what its generator prints,
the float64 reference of tests/mesh_refs.py produces closed, consistently oriented meshes, the PLY / OBJ writers round-trip,
the new prototypes are declared in a header of their own and exported, and the Python entry points refuse CPU tensors."""
import os
import sys

import numpy as np
import pytest
import torch

import mesh_refs as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ia_iso_workspace_bytes", "ia_iso_lattice_points", "ia_iso_count", "ia_iso_emit", "ia_mesh_component_workspace_bytes",
       "ia_mesh_largest_count", "ia_mesh_largest_emit", "ia_unit_negative", "ia_forward_skin")


def _generator():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import gen_marching_tets
    finally:
        sys.path.pop(0)
    return gen_marching_tets


def test_generator_reproduces_the_committed_table():
    gen = _generator()
    with open(os.path.join(ROOT, "instantavatar_amd", "csrc", "ia_mt_table.h")) as f:
        assert f.read() == gen.header_text()


def test_table_agrees_with_the_reference_rules():
    """the generator (integer arithmetic) and the reference (float64 geometry) are written separately: same triangles"""
    gen = _generator()
    corners, ntri, edges = gen.tables()
    for k, vs in enumerate(mr.kuhn_tets()):
        assert corners[k] == [4 * v[0] + 2 * v[1] + v[2] for v in vs]
        for case in range(16):
            tris = mr.tet_triangles(vs, case)
            assert ntri[k][case] == len(tris)
            codes = []
            for tri in tris:
                for i, j in tri:
                    i, j = min(i, j), max(i, j)
                    codes.append(((4 * vs[i][0] + 2 * vs[i][1] + vs[i][2]) << 3) | mr.SLOTS.index(tuple(vs[j] - vs[i])))
            assert edges[k][case][:len(codes)] == codes, (k, case)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_reference_is_closed_on_noise(seed):
    v, f, _ = mr.marching_tets(mr.noise_lattice(9, seed), 9, cap=True)
    assert 1300 < len(v) < 1700 and 2700 < len(f) < 3400
    assert mr.is_closed_oriented(f)
    assert f.max() == len(v) - 1 and len(np.unique(f)) == len(v)        # welded: every vertex is used


def test_reference_sphere():
    N = 17
    v, f, _ = mr.marching_tets(mr.sphere_lattice(N), N)
    assert mr.is_closed_oriented(f) and mr.euler_characteristic(len(v), f) == 2
    vol = mr.signed_volume(v, f)
    assert 0.95 * 4 / 3 * np.pi * 0.6 ** 3 < vol < 4 / 3 * np.pi * 0.6 ** 3      # inscribed, and wound outwards
    assert np.abs(np.linalg.norm(v, axis=1) - 0.6).max() < 0.02
    label, area = mr.components(v, f)
    assert len(area) == 1 and (label == 0).all()
    v2, f2, _ = mr.marching_tets(mr.two_spheres_lattice(20), 20)
    _, area2 = mr.components(v2, f2)
    assert len(area2) == 2
    vo, fo, src = mr.largest_component(v2, f2)
    assert mr.is_closed_oriented(fo) and mr.euler_characteristic(len(vo), fo) == 2 and (vo[:, 0] < 0.05).all()
    assert np.array_equal(vo, v2[src]) and (np.diff(src) > 0).all()


def test_reference_open_without_cap():
    s = np.full(5 ** 3, 20.0, np.float32)
    v, f, _ = mr.marching_tets(s, 5, cap=False)
    assert len(f) == 0
    v, f, _ = mr.marching_tets(s, 5, cap=True)
    assert mr.is_closed_oriented(f) and mr.euler_characteristic(len(v), f) == 2


def _mesh(nv=50, nf=80, seed=0):
    from instantavatar_amd.mesh import Mesh
    rng = np.random.RandomState(seed)
    n = rng.normal(size=(nv, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[::9] = 0
    return Mesh(torch.as_tensor(rng.normal(size=(nv, 3)).astype(np.float32)), torch.as_tensor(rng.randint(0, nv, (nf, 3)).astype(np.int32)),
                torch.as_tensor(n.astype(np.float32)), torch.as_tensor(rng.uniform(-0.2, 1.2, (nv, 3)).astype(np.float32)))


def test_ply_round_trip(tmp_path):
    m = _mesh()
    m.to_ply(str(tmp_path / "m.ply"))
    got = mr.read_ply(str(tmp_path / "m.ply"))
    assert got["payload_bytes"] == got["expected_bytes"] == 50 * 27 + 80 * 13
    assert got["vertex"].dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")
    vert = got["vertex"]
    assert np.array_equal(np.stack([vert["x"], vert["y"], vert["z"]], 1), m.verts.numpy())
    assert np.array_equal(np.stack([vert["nx"], vert["ny"], vert["nz"]], 1), m.normals.numpy())
    assert np.array_equal(got["faces"], m.faces.numpy())
    c = m.colors.numpy()
    want = (np.clip(c, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(vert["red"], want[:, 2]) and np.array_equal(vert["green"], want[:, 1]) and np.array_equal(vert["blue"], want[:, 0])
    from instantavatar_amd.mesh import Mesh
    empty = Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3), torch.zeros(0, 3))
    empty.to_ply(str(tmp_path / "e.ply"))
    assert mr.read_ply(str(tmp_path / "e.ply"))["payload_bytes"] == 0


def test_obj_round_trip(tmp_path):
    m = _mesh(seed=1)
    m.to_obj(str(tmp_path / "m.obj"))
    got = mr.read_obj(str(tmp_path / "m.obj"))
    assert np.array_equal(got["verts"].astype(np.float32), m.verts.numpy())         # %.9g round-trips fp32
    assert np.array_equal(got["normals"].astype(np.float32), m.normals.numpy())
    assert np.array_equal(got["faces"], m.faces.numpy())
    want = (np.clip(m.colors.numpy(), 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)[:, ::-1]
    assert np.array_equal(np.round(got["colors"] * 255).astype(np.uint8), want)


def test_new_prototypes_are_declared_and_exported():
    from instantavatar_amd import _lib, build
    decl = _lib.declarations("mesh")            # a header of their own: include/instantavatar_hip_mesh.h
    assert set(decl) == set(NEW)                # (disjoint from every other header's: tests/test_cpu_abi_headers.py)
    for name in NEW:
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
        assert decl[name].stream == (not name.endswith("_bytes")), name       # every launching entry point takes a stream
    assert "ia_isosurface.hip" in build.SOURCES
    assert os.path.normpath(_lib.header_path("mesh")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    inc = [os.path.basename(h) for h in build.includes_of(os.path.join(build.CSRC, "ia_isosurface.hip"))]
    assert "ia_mt_table.h" in inc and "ia_search_dev.h" in inc               # an edit of either rebuilds the unit
    assert "ia_scan.h" in inc and "ia_mesh_dev.h" in inc                     # so does one of the mesh units' shared scan and face pieces


def test_host_side_argument_checks():
    """what the entry points decide before any launch"""
    from instantavatar_amd import _lib
    L = _lib.lib()
    assert L.ia_iso_workspace_bytes(1) == 0 and L.ia_iso_workspace_bytes(565) == 0
    n = 564 ** 3
    blocks = (n + 255) // 256
    al = lambda b: (b + 255) // 256 * 256
    assert L.ia_iso_workspace_bytes(564) == al(n) + al(4 * n) + 2 * al(4 * blocks)
    assert 7 * 564 ** 3 < 2 ** 31 and 12 * 563 ** 3 < 2 ** 31 <= 12 * 564 ** 3      # what IA_ISO_MAX_N = 564 is derived from
    lat = _lib.OccGrid()
    lat.G = 600
    with pytest.raises(_lib.IAError, match="outside"):
        _lib.call("ia_iso_lattice_points", lat, 0, 0, None, None)
    lat.G = 4
    with pytest.raises(_lib.IAError, match="outside the lattice"):
        _lib.call("ia_iso_lattice_points", lat, 60, 5, None, None)
    with pytest.raises(_lib.IAError):
        _lib.call("ia_mesh_largest_count", None, None, 0, 0, 0.0, None, 0, None, None)


def test_cpu_tensors_raise():
    from instantavatar_amd import _lib, mesh
    from instantavatar_amd.pipeline import AvatarModel
    f = lambda *s: torch.zeros(s)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    b = lambda *s: torch.zeros(s, dtype=torch.uint8)
    lat, grid = mesh.lattice_desc(4, [-1, -1, -1], [1, 1, 1]), _lib.SnarfGrid()
    calls = {
        "ia_iso_lattice_points": (lat, 0, 64, f(64, 3)),
        "ia_iso_count": (f(64), 4, 10.0, 1, b(4096), 4096, i(2)),
        "ia_iso_emit": (f(64), lat, 10.0, 1, b(4096), 4096, f(8, 3), 8, i(8, 3), 8),
        "ia_mesh_largest_count": (f(8, 3), i(8, 3), 8, 8, 1.0, b(4096), 4096, i(2)),
        "ia_mesh_largest_emit": (f(8, 3), i(8, 3), 8, 8, b(4096), 4096, f(8, 3), 8, i(8, 3), 8, i(8)),
        "ia_unit_negative": (f(8, 3), 8, f(8, 3)),
        "ia_forward_skin": (f(8, 3), 8, f(96), grid, f(4, 4), f(8, 3)),
    }
    assert set(calls) == {n for n in NEW if not n.endswith("_bytes")}
    for name, args in calls.items():
        with pytest.raises(_lib.IAError, match="GPU"):
            _lib.call(name, *args, None)

    class Net:
        center = torch.zeros(3)
    model = AvatarModel(None, Net(), None)
    with pytest.raises(_lib.IAError):
        model.extract_mesh(resolution=8)
    with pytest.raises(_lib.IAError):
        mesh.isosurface(torch.zeros(8 ** 3), mesh.lattice_desc(8, [-1, -1, -1], [1, 1, 1]))
    with pytest.raises(_lib.IAError):
        mesh.largest_component(f(8, 3), i(8, 3), 1.0)
    from instantavatar_amd.deformers.smpl_deformer import SMPLDeformer
    with pytest.raises(NotImplementedError, match="SNARF"):
        AvatarModel(SMPLDeformer.__new__(SMPLDeformer), Net(), None).pose_mesh(_mesh(), {})
