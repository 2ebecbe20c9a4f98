"""What the rasteriser promises without a GPU ("rasteriser"): the integer coverage rule of the numpy
reference (tests/raster_refs.py) on hand-made triangles and on a closed sphere, the edge-function reference against an
independent ray-triangle brute force, the new prototypes in a header and a table of their own, and the argument checks the
entry points make before any launch.

The edge-function / ray comparison, and what its depth bound is held against.  Face ids are compared with the rays through
the ORIGINAL (unsnapped, float64) geometry, on every pixel at least 1/128 pixel from every projected edge -- snapping to 8
sub-pixel bits moves a vertex by at most sqrt(2) / 512 = 1 / 362 pixel, so a sample farther than 1 / 128 from every edge is
on the same side of all of them before and after.  Depth to 1e-9 cannot hold against that geometry: moving a vertex by 1/362
pixel moves the interpolated depth by about that fraction of the depth difference across a pixel (measured on this input:
3.4e-4 relative), and inv_z is rounded to fp32 (6e-8).  The 1e-9 bound is therefore asserted against the rays through the
geometry the rasteriser is DEFINED on -- the vertices unprojected from the integer xy and the fp32 inv_z -- where screen-space
interpolation of 1 / z is exact and only float64 rounding is left (measured 1.1e-15); the face ids must agree there too."""
import os

import numpy as np
import pytest
import torch

import raster_refs as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ia_raster_workspace_bytes", "ia_raster_project", "ia_raster_visibility", "ia_raster_resolve")
H, W = 29, 37
CASES = rr.hand_cases()


def _run(name, cull=False):
    c = CASES[name]
    return rr.rasterize(c["xy"], c["inv_z"], c["faces"], H, W, cull)


# ---- top-left rule on hand-made integer triangles -----------------------------------------------------------------------
def test_vertices_on_pixel_centres():
    """(2,2) (10,2) (2,8): the top edge (y = 2) and the left edge (x = 2) own their samples, the hypotenuse does not"""
    for name in ("on_centres", "on_centres_flipped"):           # the rule does not depend on the winding
        cov = _run(name)["face_id"] >= 0
        assert cov[2, 2:10].all() and not cov[2, 10], name      # top edge: covered up to, not including, the right vertex
        assert cov[2:8, 2].all() and not cov[8, 2], name        # left edge: covered down to, not including, the bottom vertex
        # the hypotenuse from (10,2) to (2,8) passes through the sample (6,5): a right edge, not covered
        assert not cov[5, 6] and cov[5, 5], name
        want = np.zeros((H, W), bool)
        for y in range(2, 8):
            for x in range(2, 10):
                want[y, x] = 3 * (x - 2) + 4 * (y - 2) < 24    # strictly inside the hypotenuse
        assert np.array_equal(cov, want), name


def test_edge_through_sample_points():
    """the diagonal (3,3)-(11,11) passes through the samples (4,4) .. (10,10): exactly one of the two triangles on its sides
    covers them -- the one for which it is a left edge"""
    below, above = _run("edge_through_samples")["face_id"] >= 0, _run("edge_through_samples_other_side")["face_id"] >= 0
    diag = np.arange(4, 11)
    assert not (below & above).any()
    assert (below[diag, diag] ^ above[diag, diag]).all()
    assert above[diag, diag].all()        # (3,3) (11,3) (11,11) lies to the right of the diagonal: its left edge, which owns its samples
    both = below | above
    want = np.zeros((H, W), bool)
    want[3:11, 3:11] = True                        # the square [3, 11) x [3, 11): its top and left edges own their samples
    assert np.array_equal(both, want)


@pytest.mark.parametrize("name", ["quad", "quad_mixed_winding", "quad_subpixel"])
def test_two_triangles_sharing_an_edge_cover_the_quad_once(name):
    r = _run(name)
    assert r["cover"].max() == 1
    if name != "quad_subpixel":
        want = np.zeros((H, W), bool)
        want[3:17, 4:20] = True
        assert np.array_equal(r["cover"] == 1, want)
    else:
        assert 200 < r["cover"].sum() < 300
        # every sample strictly inside the quad is covered (float64 point-in-convex-polygon, at a distance from the boundary)
        q = CASES[name]["xy"].astype(np.float64) / 256
        y, x = np.mgrid[0:H, 0:W]
        inside = np.ones((H, W), bool)
        for i in range(4):
            a, b = q[i], q[(i + 1) % 4]
            inside &= ((b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0])) > 1e-6
        assert np.array_equal(r["cover"] == 1, inside)


def test_sliver_covers_no_sample():
    r = _run("sliver")
    assert r["cover"].sum() == 0 and (r["face_id"] == -1).all() and r["skipped"] == 0


def test_skipped_faces_and_ties():
    assert _run("degenerate")["skipped"] == 2 and _run("degenerate")["cover"].sum() == 0
    r = _run("invalid_vertex")
    assert r["skipped"] == 2 and set(np.unique(r["face_id"])) == {-1, 1}
    r = _run("beyond_range")
    assert r["skipped"] == 1 and set(np.unique(r["face_id"])) == {-1, 1}
    r = _run("duplicate")
    assert set(np.unique(r["face_id"])) == {-1, 0} and r["cover"].max() == 2           # the exact tie: the smaller index
    r = _run("duplicate_behind")
    assert set(np.unique(r["face_id"])) == {-1, 0, 1}
    both, culled = _run("front_and_back"), _run("front_and_back", cull=True)
    assert culled["skipped"] > 0 and not np.array_equal(both["face_id"], culled["face_id"])
    assert (_run("screen_filling")["face_id"] == 0).all()
    assert (_run("off_screen")["face_id"] == -1).all() and (_run("off_screen_right")["face_id"] == -1).all()


# ---- a closed sphere ------------------------------------------------------------------------------------------------
_pair = {}


def _sphere_pair():
    if not _pair:
        Hh, Ww = 80, 96
        V, F = rr.sphere_pair()
        w2c, fx, fy, cx, cy = rr.pair_camera(Hh, Ww)
        pr = rr.project(V, w2c, fx, fy, cx, cy)
        _pair.update(V=V, F=F, cam=(fx, fy, cx, cy), pr=pr, H=Hh, W=Ww, ref=rr.rasterize(pr["xy"], pr["inv_z"], F, Hh, Ww))
    return _pair


def test_closed_sphere_front_faces_cover_the_silhouette_once():
    P = _sphere_pair()
    nf = len(P["F"]) // 2                              # the first sphere alone: closed, radius 0.5
    assert nf == 1280
    nv = len(P["V"]) // 2
    xy, w, F = P["pr"]["xy"][:nv], P["pr"]["inv_z"][:nv], P["F"][:nf]
    every = rr.rasterize(xy, w, F, P["H"], P["W"], cull=False)
    front = rr.rasterize(xy, w, F, P["H"], P["W"], cull=True)
    sil = every["cover"] > 0
    assert 1000 < sil.sum() < 1400
    assert np.array_equal(front["cover"] == 1, sil) and front["cover"].max() == 1
    assert np.array_equal(every["face_id"], front["face_id"])          # the nearest fragment of a closed surface is a front face
    assert set(np.unique(every["cover"][sil])) <= {1, 2}               # a convex body: front + back, or front alone on a back sliver


# ---- the edge-function reference against ray-triangle intersection ------------------------------------------------------
def test_edge_functions_agree_with_ray_intersection():
    P = _sphere_pair()
    fx, fy, cx, cy = P["cam"]
    pr, F, Hh, Ww, ref = P["pr"], P["F"], P["H"], P["W"], P["ref"]
    assert pr["valid"].all() and (ref["face_id"] >= 0).sum() == 1576
    dist = rr.edge_distance(pr["u"], pr["v"], F, pr["valid"], Hh, Ww)
    keep = dist >= 1.0 / 128
    left_out = 1 - keep.mean()
    fid, _ = rr.ray_cast(pr["p"], F, fx, fy, cx, cy, Hh, Ww)
    print("left out: %.4f of the pixels; face ids that differ among the kept: %d, among all: %d"
          % (left_out, (fid != ref["face_id"])[keep].sum(), (fid != ref["face_id"]).sum()))
    assert left_out <= 0.05
    assert np.array_equal(fid[keep], ref["face_id"][keep])
    # the geometry the rasteriser is defined on: see the module docstring
    snapped = rr.unproject(pr["xy"], pr["inv_z"], fx, fy, cx, cy)
    fid2, depth2 = rr.ray_cast(snapped, F, fx, fy, cx, cy, Hh, Ww)
    assert np.array_equal(fid2[keep], ref["face_id"][keep])
    hit = keep & (fid2 >= 0)
    err = np.abs(rr.depth_of(ref) - depth2)[hit] / depth2[hit]
    print("depth, %d pixels: max relative difference %.3e" % (hit.sum(), err.max()))
    assert hit.sum() > 1400 and err.max() <= 1e-9
    for cull in (False, True):
        r = rr.rasterize(pr["xy"], pr["inv_z"], F, Hh, Ww, cull)
        cov = r["face_id"] >= 0
        near = cov & (r["second"] > 0) & (r["iz"] - r["second"] <= 32 * 2.0 ** -24 * r["iz"])
        assert cov.sum() == 1576 and near.sum() == 0          # what the GPU depth-order test leaves out: nothing


def test_interpolation_reproduces_linear_functions():
    """perspective-correct interpolation is exact for a function that is linear in camera space"""
    P = _sphere_pair()
    fx, fy, cx, cy = P["cam"]
    snapped = rr.unproject(P["pr"]["xy"], P["pr"]["inv_z"], fx, fy, cx, cy)
    coef = np.array([[0.3, -1.2, 0.7], [2.0, 0.1, -0.4]])
    attrs = snapped @ coef.T + np.array([0.25, -3.0])
    out, scale = rr.interpolate(P["ref"], P["F"], P["pr"]["inv_z"], attrs)
    hit = P["ref"]["face_id"] >= 0
    y, x = np.mgrid[0:P["H"], 0:P["W"]]
    z = rr.depth_of(P["ref"])
    point = np.stack([(x - cx) / fx * z, (y - cy) / fy * z, z], -1)
    want = point @ coef.T + np.array([0.25, -3.0])
    assert np.abs(out - want)[hit].max() <= 1e-12 * scale[hit].max()
    assert (out[~hit] == 0).all()


# ---- declarations and build plumbing ----------------------------------------------------------------------------------
def test_raster_prototypes_are_declared_and_exported():
    from instantavatar_amd import _lib, build
    decl = _lib.declarations("raster")            # a header of their own: include/instantavatar_hip_raster.h
    assert set(decl) == set(NEW)                  # (disjoint from every other header's: tests/test_cpu_abi_headers.py)
    for name in NEW:
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
        assert decl[name].stream == (not name.endswith("_bytes")), name       # every launching entry point takes a stream
    assert "ia_raster.hip" in build.SOURCES
    assert os.path.normpath(_lib.header_path("raster")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_raster.hip" in build.source_manifest()


def test_host_side_argument_checks():
    """what the entry points decide before any launch (pointers are made-up addresses: nothing is dereferenced on the host)"""
    from instantavatar_amd import _lib
    L = _lib.lib()
    P = 4096                                      # a non-null "device pointer"
    assert L.ia_raster_workspace_bytes(8, 8, 0, 16) == 0 and L.ia_raster_workspace_bytes(8, 8, 16, 16385) == 0
    assert L.ia_raster_workspace_bytes(-1, 8, 16, 16) == 0 and L.ia_raster_workspace_bytes(8, -1, 16, 16) == 0
    al = lambda b: (b + 255) // 256 * 256
    assert L.ia_raster_workspace_bytes(8, 1000, 16, 16) == 256 + al(4000)
    assert L.ia_raster_workspace_bytes(0, 0, 1, 16384) == 512
    nb = L.ia_raster_workspace_bytes(8, 8, 16, 16)
    with pytest.raises(_lib.IAError, match="H = 0"):
        _lib.call("ia_raster_visibility", P, P, 8, P, 8, 0, 16, 0, P, P, nb, None)
    with pytest.raises(_lib.IAError, match="W = 16385"):
        _lib.call("ia_raster_resolve", P, P, 8, P, 8, P, 16, 16385, None, 0, P, nb, P, P, None, P, None)
    with pytest.raises(_lib.IAError, match="C = 9"):
        _lib.call("ia_raster_resolve", P, P, 8, P, 8, P, 16, 16, P, 9, P, nb, P, P, P, P, None)
    with pytest.raises(_lib.IAError, match="without attrs"):
        _lib.call("ia_raster_resolve", P, P, 8, P, 8, P, 16, 16, None, 3, P, nb, P, P, None, P, None)
    with pytest.raises(_lib.IAError, match="workspace too small"):
        _lib.call("ia_raster_visibility", P, P, 8, P, 8, 16, 16, 0, P, P, nb - 1, None)
    with pytest.raises(_lib.IAError, match="workspace too small"):
        _lib.call("ia_raster_resolve", P, P, 8, P, 8, P, 16, 16, None, 0, P, nb - 1, P, P, None, P, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_raster_visibility", P, P, 8, P, 8, 16, 16, 0, None, P, nb, None)
    with pytest.raises(_lib.IAError, match="near"):
        _lib.call("ia_raster_project", P, 8, P, 100.0, 100.0, 8.0, 8.0, 0.0, P, P, None)
    with pytest.raises(_lib.IAError, match="nv < 0"):
        _lib.call("ia_raster_project", P, -1, P, 100.0, 100.0, 8.0, 8.0, 0.1, P, P, None)


def test_cpu_tensors_raise():
    from instantavatar_amd import _lib, raster
    from instantavatar_amd.mesh import Mesh
    from instantavatar_amd.pipeline import AvatarModel
    f = lambda *s: torch.zeros(s)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    calls = {
        "ia_raster_project": (f(8, 3), 8, f(4, 4), 100.0, 100.0, 8.0, 8.0, 0.1, i(8, 2), f(8)),
        "ia_raster_visibility": (i(8, 2), f(8), 8, i(4, 3), 4, 16, 16, 0, torch.zeros(256, dtype=torch.int64), torch.zeros(512, dtype=torch.uint8), 512),
        "ia_raster_resolve": (i(8, 2), f(8), 8, i(4, 3), 4, torch.zeros(256, dtype=torch.int64), 16, 16, None, 0,
                              torch.zeros(512, dtype=torch.uint8), 512, i(256), f(256), None, i(2)),
    }
    assert set(calls) == {n for n in NEW if not n.endswith("_bytes")}
    for name, args in calls.items():
        with pytest.raises(_lib.IAError, match="GPU"):
            _lib.call(name, *args, None)
    cam = raster.Camera(np.array([[100.0, 0, 8], [0, 100.0, 8], [0, 0, 1]]), torch.eye(4), 16, 16)
    assert (cam.fx, cam.fy, cam.cx, cam.cy, cam.near) == (100.0, 100.0, 8.0, 8.0, 0.05)
    with pytest.raises(_lib.IAError):
        raster.rasterize(f(8, 3), i(4, 3), cam)
    mesh = Mesh(f(8, 3), i(4, 3), f(8, 3), f(8, 3))
    with pytest.raises(_lib.IAError):
        mesh.render(cam)
    with pytest.raises(_lib.IAError):
        AvatarModel(None, None, None).render_mesh(mesh, cam)
    with pytest.raises(ValueError):
        raster.Camera(np.eye(4), torch.eye(4), 16, 16)


def test_sequence_camera_is_the_camera_of_its_rays():
    """AnimateSequence.camera(): the ray through pixel (x, y) is K^-1 [x, y, 1] -- the sample position of the rasteriser"""
    from instantavatar_amd.drivers.animate import AnimateSequence
    seq = AnimateSequence(np.zeros((2, 72), np.float32), np.zeros((2, 3), np.float32), np.zeros(10, np.float32), "cpu", size=24)
    cam = seq.camera()
    assert (cam.H, cam.W) == (24, 24) and torch.equal(cam.w2c, torch.eye(4))
    assert cam.fx == cam.fy == float(np.float32(2000 * 24 / 1080)) and cam.cx == cam.cy == 540 * 24 / 1080      # fp32, as the C ABI takes them
    d = seq.rays_d.reshape(24, 24, 3).numpy().astype(np.float64)
    y, x = np.mgrid[0:24, 0:24]
    u, v = cam.fx * d[..., 0] / d[..., 2] + cam.cx, cam.fy * d[..., 1] / d[..., 2] + cam.cy
    assert np.abs(u - x).max() < 1e-4 and np.abs(v - y).max() < 1e-4
    assert np.abs(cam.rays_d().numpy() - seq.rays_d.reshape(-1, 3).numpy()).max() < 1e-6
