"""The mesh processing on the GPU (include/instantavatar_hip_meshops.h; DESIGN.md section 4, "mesh simplification") against the float64
references of tests/meshops_refs.py: vertex clustering with quadrics, Taubin smoothing, vertex normals from the faces; then
`AvatarModel.smooth_mesh` / `simplify_mesh` on the synthetic model and the extract_mesh driver with --smooth / --simplify.

Tolerances, derived and not measured.  Topology is integer work on the same fp32 cell formula: counts, faces and the vertex map are
compared for equality.  Positions: all arithmetic is fp64 on a system of condition number at most (1 + reg) / reg = 1001, so the
value before the final rounding agrees with the reference to many orders below one fp32 ulp, and the rounding itself is half an
ulp of a coordinate inside the box: 2 x 2^-24 x the largest |box coordinate| leaves room for a rounding that falls the other way.
Colours are means of values in [0, 1]: 2^-23.  Taubin, one iteration: two roundings, the second step's gain of at most
1 + 2 |mu| = 2.06 on the first's half ulp, about 1.5 ulp: 2 x 2^-24 x the largest |coordinate|.  Normals are components of a unit
vector rounded once: 2^-23."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_refs as mr
import meshops_refs as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (np.float32([-1, -1, -1]), np.float32([1, 1, 1]))
WIDE = (np.float32([-1.1] * 3), np.float32([1.1] * 3))


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(v, f, c=None):
    from instantavatar_amd.mesh import Mesh
    c = mo.colours_of(v) if c is None else c
    return Mesh(_dev(v, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3), torch.zeros((len(v), 3), device=DEV),
                _dev(c, torch.float32).reshape(-1, 3))


def _bad_mesh():
    """an icosphere plus a NaN vertex and four collinear vertices in cells the sphere does not reach, one of them unreferenced; faces
    that use the NaN vertex, repeat an index, leave [0, nv), and one without area (valid: it makes neighbours, adds nothing to a
    quadric or a normal, and is dropped because two of its corners share a cell)"""
    v, f = mo.noisy_icosphere(2)
    n = len(v)
    v2 = np.concatenate([v, np.float32([[np.nan, 0, 0], [0, 0, 0], [0.05, 0, 0], [0.1, 0, 0], [0.3, 0, 0]])])
    f2 = np.concatenate([f[:50], np.int32([[0, 1, n], [0, 0, 1], [0, 1, len(v2)], [-1, 2, 3], [n + 1, n + 2, n + 4], [5, 5, 5]]), f[50:]])
    return v2, f2, n


CASES = {
    "icosphere3_cell0.2": lambda: (*mo.noisy_icosphere(3), WIDE, 0.2),
    "icosphere3_cell0.45": lambda: (*mo.noisy_icosphere(3), WIDE, 0.45),
    "cube12_on_cell_faces": lambda: (*mo.cube(12, 0.75), BOX, 0.25),          # coordinates are multiples of 0.125 = h / 2
    "fan300": lambda: (*mo.fan(300), BOX, 0.25),
    "coarse_cell": lambda: (*mo.icosphere(4), WIDE, 1.1),                      # 8 cells of 1 782 .. 2 067 corners: both long-segment sorts
    "fan256_257_vertices": lambda: (*mo.fan(256), BOX, 0.3),
    "fan1024_1025_vertices": lambda: (*mo.fan(1024), BOX, 0.2),
    "bad_faces_and_a_nan": lambda: (*_bad_mesh()[:2], BOX, 0.4),
    "outside_the_box": lambda: (*mo.noisy_icosphere(3), (np.float32([-0.6, -0.5, -0.7]), np.float32([0.6, 0.7, 0.5])), 0.3),
    "one_cell": lambda: (*mo.noisy_icosphere(2), (np.float32([-2] * 3), np.float32([2] * 3)), 4.0),
    "no_faces": lambda: (mo.noisy_icosphere(2)[0], np.zeros((0, 3), np.int32), BOX, 0.25),
}
CLOSED = ("icosphere3_cell0.2", "icosphere3_cell0.45", "cube12_on_cell_faces", "coarse_cell", "outside_the_box")


def _simplify(v, f, box, cell, c=None, reg=1e-3):
    from instantavatar_amd import mesh
    out = mesh.simplify(_mesh(v, f, c), cell, box, reg)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_simplify_against_reference(name):
    v, f, box, cell = CASES[name]()
    col = mo.colours_of(v)
    ref = mo.simplify(v, f, col, box[0], box[1], cell)
    got = _simplify(v, f, box, cell, col)
    again = _simplify(v, f, box, cell, col)
    gv, gf, gc, gm = _np(got.verts), _np(got.faces), _np(got.colors), _np(got.vert_cluster)
    print("%s: %d -> %d vertices, %d -> %d faces" % (name, len(v), len(gv), len(f), len(gf)))
    assert (len(gv), len(gf)) == (len(ref["verts"]), len(ref["faces"]))
    assert np.array_equal(gf, ref["faces"]) and np.array_equal(gm, ref["vert_cluster"])
    tol = 2 * 2.0 ** -24 * float(np.abs(np.concatenate(box)).max())
    if len(gv):
        err, cerr = np.abs(gv.astype(np.float64) - ref["verts"]).max(), np.abs(gc.astype(np.float64) - ref["colors"]).max()
        print("%s: max position error %.3e (tolerance %.3e), colour error %.3e" % (name, err, tol, cerr))
        assert err <= tol and cerr <= 2.0 ** -23
        n = _np(got.normals).astype(np.float64)
        assert np.abs(n - mo.vertex_normals(gv, gf)).max() <= 2.0 ** -23
    if name in ("one_cell", "no_faces"):
        assert len(gv) == 0 and len(gf) == 0 and (gm == -1).all()
    else:
        assert len(gf) > 0
    for a, b in ((got.verts, again.verts), (got.faces, again.faces), (got.colors, again.colors), (got.vert_cluster, again.vert_cluster),
                 (got.normals, again.normals)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls differ"
    if name in CLOSED:
        d = mr.directed_edge_counts(gf)
        assert all(d.get((b, a), 0) == c for (a, b), c in d.items()), "a directed edge is used more often than its reverse"
        assert ((gf[:, 0] != gf[:, 1]) & (gf[:, 1] != gf[:, 2]) & (gf[:, 0] != gf[:, 2])).all()
        assert np.array_equal(np.unique(gf), np.arange(len(gv))), "an output vertex that no face references"
        h = np.float64(np.float32(cell))
        assert (np.abs(gv.astype(np.float64) - ref["centre"]) <= h / 2 + tol).all(), "an output vertex outside its cell"


def test_simplify_ignores_what_it_must():
    v2, f2, n = _bad_mesh()
    got = _simplify(v2, f2, BOX, 0.4)
    clean_v, clean_f = mo.noisy_icosphere(2)
    want = _simplify(clean_v, clean_f, BOX, 0.4, mo.colours_of(v2)[:n])
    # the collinear vertices lie in cells the sphere does not reach and the face through them has no area: nothing else changes
    assert torch.equal(got.faces, want.faces) and torch.equal(got.verts.view(torch.int32), want.verts.view(torch.int32))
    assert _np(got.vert_cluster)[n:].tolist() == [-1] * 5


def test_simplify_capacities_and_default_box():
    from instantavatar_amd import _lib, mesh
    v, f = mo.noisy_icosphere(3)
    m = _mesh(v, f)
    auto = mesh.simplify(m, 0.3)
    lo, hi = v.min(0), v.max(0)
    ref = mo.simplify(v, f, None, lo, hi, 0.3)
    assert np.array_equal(_np(auto.faces), ref["faces"])
    # rows past the capacities stay untouched
    geo = [float(x) for x in lo] + [float(x) for x in hi] + [float(np.float32(0.3)), float(np.float32(1.0 / np.float64(np.float32(0.3))))]
    n = mesh.cluster_grid(lo, hi, 0.3)
    nb = int(_lib.call("ia_mesh_cluster_workspace_bytes", len(v), len(f), n[0] * n[1] * n[2]))
    ws, counts = torch.empty(nb, dtype=torch.uint8, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    _lib.call("ia_mesh_cluster_count", m.verts, m.faces, len(v), len(f), *geo, ws, nb, counts)
    nv2, nf2 = counts.tolist()
    assert (nv2, nf2) == (len(ref["verts"]), len(ref["faces"])) and nv2 > 8 and nf2 > 8
    vo, fo = torch.full((nv2, 3), 7.0, device=DEV), torch.full((nf2, 3), 7, dtype=torch.int32, device=DEV)
    co = torch.full((nv2, 3), 7.0, device=DEV)
    _lib.call("ia_mesh_cluster_emit", m.verts, m.faces, m.colors, len(v), len(f), *geo, 1e-3, ws, nb, vo, nv2 - 5, fo, nf2 - 3, co, None)
    torch.cuda.synchronize()
    assert (vo[nv2 - 5:] == 7).all() and (co[nv2 - 5:] == 7).all() and (fo[nf2 - 3:] == 7).all()
    assert torch.equal(vo[:nv2 - 5], auto.verts[:nv2 - 5]) and torch.equal(fo[:nf2 - 3], auto.faces[:nf2 - 3])


# ---- Taubin -------------------------------------------------------------------------------------------------------------------------
def _smooth(v, f, iters, lam=0.5, mu=-0.53):
    from instantavatar_amd import mesh
    out = mesh.smooth(_mesh(v, f), iters, lam, mu)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", ["icosphere3", "fan300", "fan1024", "fan1100", "bad_faces_and_a_nan"])
def test_taubin_one_iteration_against_reference(name):
    v, f = {"icosphere3": lambda: mo.noisy_icosphere(3), "fan300": lambda: mo.fan(300), "fan1024": lambda: mo.fan(1024),
            "fan1100": lambda: mo.fan(1100),            # the hub's 2 200 neighbour entries pass the sort's LDS buffer of 2 048
            "bad_faces_and_a_nan": lambda: _bad_mesh()[:2]}[name]()
    got = _np(_smooth(v, f, 1).verts)
    ref = mo.taubin(v, f, 1)
    fin = np.isfinite(v).all(1)
    tol = 2 * 2.0 ** -24 * float(np.abs(v[fin]).max())
    err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64)).max()
    print("taubin %s: max error %.3e (tolerance %.3e)" % (name, err, tol))
    assert err <= tol
    nb = mo.neighbours(v, f)
    still = np.array([len(x) == 0 for x in nb])
    assert np.array_equal(got[still].view(np.uint32), v[still].view(np.uint32)), "a vertex without neighbours must keep its bits"
    assert not np.array_equal(got[~still], v[~still])
    if name == "bad_faces_and_a_nan":
        assert still.sum() == 2 and np.isnan(got[~fin]).any()       # the NaN vertex and the unreferenced one
        clean_v, clean_f = mo.noisy_icosphere(2)
        assert np.array_equal(got[:len(clean_v)], _np(_smooth(clean_v, clean_f, 1).verts)), "bad faces must be ignored"
    if name.startswith("fan"):
        assert len(nb[0]) == len(v) - 1


def test_taubin_iterations_compose_and_zero_copies():
    v, f = mo.noisy_icosphere(3)
    three = _smooth(v, f, 3)
    x = v
    for _ in range(3):
        x = _np(_smooth(x, f, 1).verts)
    assert np.array_equal(_np(three.verts).view(np.uint32), x.view(np.uint32))
    v2, f2, _ = _bad_mesh()
    zero = _smooth(v2, f2, 0)
    assert np.array_equal(_np(zero.verts).view(np.uint32), v2.view(np.uint32))
    m = _mesh(v, f)
    out = m.smooth(2)
    assert out.faces is m.faces and out.colors is m.colors and not torch.equal(out.verts, m.verts)
    assert mo.roughness(_np(_smooth(v, f, 10).verts), f) < mo.roughness(v, f)


# ---- vertex normals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere3", "fan300", "bad_faces_and_a_nan", "cube12"])
def test_vertex_normals_against_reference(name):
    from instantavatar_amd import mesh
    v, f = {"icosphere3": lambda: mo.noisy_icosphere(3), "fan300": lambda: mo.fan(300), "bad_faces_and_a_nan": lambda: _bad_mesh()[:2],
            "cube12": lambda: mo.cube(12, 0.75)}[name]()
    got = _np(mesh.vertex_normals(_dev(v), _dev(f))).astype(np.float64)
    ref = mo.vertex_normals(v, f)
    assert np.abs(got - ref).max() <= 2.0 ** -23
    ln = np.linalg.norm(got, axis=1)
    zero = (got == 0).all(1)
    assert (zero | (np.abs(ln - 1) <= 2.0 ** -23)).all()
    lone = np.array([len(x) == 0 for x in mo.neighbours(v, f)])
    assert zero[lone].all() and np.array_equal(zero, (ref == 0).all(1))
    if name == "bad_faces_and_a_nan":
        assert lone.sum() == 2 and zero.sum() == 5               # and the three whose only face has no area
    else:
        assert not zero[~lone].any()
    smoothed = _smooth(v, f, 2)
    assert np.abs(_np(smoothed.normals) - mo.vertex_normals(_np(smoothed.verts), f, valid_on=v)).max() <= 2.0 ** -23


# ---- the synthetic model ------------------------------------------------------------------------------------------------------------
def test_smooth_then_simplify_the_model_mesh():
    import world
    from instantavatar_amd import mesh as M, raster
    from instantavatar_amd.pipeline import make_batch
    model = world.build(DEV, 64, 16)[0]
    base = model.extract_mesh(resolution=64)
    lo, hi = M.field_box(model.net_coarse)
    cell = 4 * float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / 63
    smooth = model.smooth_mesh(base, 5)
    out = model.simplify_mesh(smooth, cell)
    torch.cuda.synchronize()
    bv, bf = _np(base.verts), _np(base.faces)
    sv = _np(smooth.verts)
    tol = 2 * 2.0 ** -24 * float(np.abs(np.concatenate([lo, hi])).max())
    # (five iterations accumulate ten roundings, each amplified by at most 2.06 per later half-step pair: compared per iteration
    # in test_taubin_*; here the reference continues from the GPU's own smoothed vertices)
    ref = mo.simplify(sv, bf, _np(base.colors), lo, hi, cell)
    gv, gf = _np(out.verts), _np(out.faces)
    print("model mesh at resolution 64: %d -> %d vertices, %d -> %d faces (face ratio %.4f)" % (len(bv), len(gv), len(bf), len(gf), len(gf) / len(bf)))
    assert np.array_equal(gf, ref["faces"]) and np.array_equal(_np(out.vert_cluster), ref["vert_cluster"])
    assert np.abs(gv.astype(np.float64) - ref["verts"]).max() <= tol
    assert 0 < len(gf) < len(bf)
    assert smooth.faces is base.faces and not np.array_equal(sv, bv)
    poses, tr = world.poses(8)
    posed = model.pose_mesh(out, make_batch(DEV, 8, poses[5], tr[5]))
    assert posed.faces is out.faces and posed.verts.shape == out.verts.shape and not torch.equal(posed.verts, out.verts)
    img = out.render(raster.look_at_box(lo, hi, 64, DEV))
    torch.cuda.synchronize()
    assert int((img["mask"] != 0).sum()) > 50


def test_extract_mesh_driver_with_smooth_and_simplify(tmp_path):
    import re
    import world
    poses, tr = world.poses(8)
    np.savez(tmp_path / "track.npz", poses=poses[:2], trans=tr[:2])
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "instantavatar_amd.drivers.extract_mesh", "--synthetic", "--resolution", "48", "--smooth", "3", "--simplify", "4",
           "--poses", str(tmp_path / "track.npz"), "--out", str(tmp_path / "out")]
    r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    files = {name: mr.read_ply(str(tmp_path / "out" / (name + ".ply"))) for name in ("canonical", "posed_0", "posed_1")}
    for name, p in files.items():
        assert p["payload_bytes"] == p["expected_bytes"] > 0, name
        assert np.array_equal(p["faces"], files["canonical"]["faces"]), name
        assert len(p["vertex"]) == len(files["canonical"]["vertex"])
        assert np.array_equal(np.unique(p["faces"]), np.arange(len(p["vertex"]))), "a vertex that no face references"
    m = re.search(r"processed mesh: (\d+) -> (\d+) vertices, (\d+) -> (\d+) faces \(smooth [\d.]+ s, simplify [\d.]+ s\)", r.stdout)
    assert m, r.stdout[-2000:]
    n0, n1, f0, f1 = map(int, m.groups())
    assert n1 < n0 and f1 < f0 and (n1, f1) == (len(files["canonical"]["vertex"]), len(files["canonical"]["faces"]))
    assert ("canonical mesh: %d vertices, %d faces" % (n0, f0)) in r.stdout
