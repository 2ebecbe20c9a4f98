"""tests/texture_refs.py, the float64 reference of the texture atlas ("texture atlas"), is itself checked here on
cases that can be verified by hand: the layout, the corner texels, literal snap cases, sampling of a ramp.  Then the binding table of
include/instantavatar_hip_texture.h and what the entry points and the Python layer refuse before anything is launched.  No GPU."""
import os

import numpy as np
import pytest
import torch

import texture_refs as tx

NAMES = ["ia_tex_atlas_size", "ia_tex_corner_uv", "ia_tex_sample", "ia_tex_snap", "ia_tex_texel_points"]


# ---- layout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 5, 8, 16])
def test_every_texel_of_a_full_atlas_has_exactly_one_owner(B):
    nf = 8                                                      # 4 blocks, 2 per row, all full
    assert tx.atlas_size(nf, B) == 2 * B
    owner, h, i, j = tx.texel_owner(nf, B)
    assert owner.shape == (2 * B, 2 * B) and (owner >= 0).all() and (owner < nf).all()
    count = np.bincount(owner.reshape(-1), minlength=nf)
    assert (count[0::2] == B * (B - 1) // 2).all() and (count[1::2] == B * (B + 1) // 2).all()      # i + j <= B - 2, and the rest
    assert count.sum() == 4 * B * B
    # the owner of a texel is the face of ITS block and half; the corners of a face are texels it owns
    uv = tx.corner_uv(nf, B)
    for f in range(nf):
        q = f >> 1
        ys, xs = np.nonzero(owner == f)
        assert (xs // B == q % 2).all() and (ys // B == q // 2).all()
        for k in range(3):
            x, y = (uv[f, k] - 0.5).astype(int)
            assert owner[y, x] == f


def test_corner_table_is_the_one_of_the_definition():
    assert tx.corner_local(8, 0).tolist() == [[0, 0], [5, 0], [0, 5]]
    assert tx.corner_local(8, 1).tolist() == [[7, 7], [2, 7], [7, 2]]
    uv = tx.corner_uv(3, 4)                                     # T = 8: face 2 sits in block 1 at column 1, row 0; L = 1
    assert uv[2].tolist() == [[4.5, 0.5], [5.5, 0.5], [4.5, 1.5]] and uv[1].tolist() == [[3.5, 3.5], [2.5, 3.5], [3.5, 2.5]]


@pytest.mark.parametrize("B", [4, 5, 8, 16])
def test_bilinear_footprint_inside_a_face_reads_only_texels_the_face_owns(B):
    nf, N = 3, 32                                               # both halves of block 0 and a half-empty block 1; weights k / 32 are exact
    T = tx.atlas_size(nf, B)
    owner = tx.texel_owner(nf, B)[0]
    uv = tx.corner_uv(nf, B)
    for f in range(nf):
        for a in range(N + 1):
            for b in range(N + 1 - a):
                w = np.array([N - a - b, a, b]) / N
                u, v = w @ uv[f]
                for (x, y) in tx.bilinear_footprint(T, u, v):
                    assert owner[y, x] == f, (B, f, a, b, x, y)


@pytest.mark.parametrize("nf,blocks", [(0, 1), (1, 1), (2, 1), (3, 2), (7, 2), (8, 2), (9, 3), (33, 5), (50, 5), (51, 6)])
def test_atlas_size(nf, blocks):
    for B in (4, 5, 8, 64):
        assert tx.atlas_size(nf, B) == blocks * B
    assert tx.atlas_size(nf, 3) == 0 and tx.atlas_size(nf, 65) == 0 and tx.atlas_size(-1, 8) == 0


def test_atlas_size_limit():
    assert tx.atlas_size(2 * 256 * 256, 64) == 16384 and tx.atlas_size(2 * 256 * 256 + 1, 64) == 0
    assert tx.atlas_size(2 * 4096 * 4096, 4) == 16384 and tx.atlas_size(2 * 4096 * 4096 + 1, 4) == 0


@pytest.mark.parametrize("nf", [1, 2, 3, 7])
def test_unowned_texels(nf):
    B = 5
    owner, h, i, j = tx.texel_owner(nf, B)
    T = owner.shape[0]
    nb = T // B
    for y in range(T):
        for x in range(T):
            f = 2 * ((y // B) * nb + x // B) + (0 if x % B + y % B <= B - 2 else 1)
            assert owner[y, x] == (f if f < nf else -1)
    n_minus = (owner < 0).sum()
    lower, upper = B * (B - 1) // 2, B * (B + 1) // 2
    assert n_minus == {1: upper, 2: 0, 3: upper + 2 * B * B, 7: upper}[nf]
    assert lower + upper == B * B


# ---- texel points -------------------------------------------------------------------------------------------------------------------
def _random_mesh(nv, nf, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nv, 3)).astype(np.float32), rng.integers(0, nv, (nf, 3)).astype(np.int32)


@pytest.mark.parametrize("B", [4, 5, 8])
def test_corner_texels_return_the_vertices_exactly(B):
    verts, faces = _random_mesh(11, 7, 3)
    faces[:, 1] = (faces[:, 0] + 1) % 11
    faces[:, 2] = (faces[:, 0] + 2) % 11
    T = tx.atlas_size(7, B)
    out = tx.texel_points(verts, faces, B)
    uv = tx.corner_uv(7, B)
    for f in range(7):
        for k in range(3):
            x, y = (uv[f, k] - 0.5).astype(int)
            g = y * T + x
            assert out["owner"][g] == f
            assert np.array_equal(out["pts"][g], verts[faces[f, k]].astype(np.float64)), (f, k)
    n = out["normal"][out["owner"] >= 0]
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-12)


def test_texel_points_are_affine_and_extrapolate_in_the_gutter():
    verts = np.float32([[0, 0, 0], [5, 0, 0], [0, 5, 0]])
    out = tx.texel_points(verts, np.int32([[0, 1, 2]]), 8)       # L = 5: texel (i, j) of half 0 lies at (i, j, 0)
    owner = out["owner"].reshape(8, 8)
    pts = out["pts"].reshape(8, 8, 3)
    for j in range(8):
        for i in range(8):
            if i + j <= 6:
                assert owner[j, i] == 0 and pts[j, i].tolist() == [i, j, 0]      # (6, 0), (3, 3): u0 = -0.2, outside the triangle
            else:
                assert owner[j, i] == -1 and not pts[j, i].any()
    assert np.array_equal(out["normal"][0], [0, 0, 1])
    moved = tx.texel_points(verts, np.int32([[0, 1, 2]]), 8, t=np.full(64, 0.25))
    assert moved["pts"].reshape(8, 8, 3)[2, 1].tolist() == [1, 2, 0.25]


def test_faces_that_own_nothing():
    verts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [np.nan, 0, 0]])
    faces = np.int32([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 1, 5], [0, -1, 2], [2, 1, 0]])      # fine, degenerate, NaN, out of range x 2, fine
    out = tx.texel_points(verts, faces, 4)
    owner = set(out["owner"].tolist())
    assert owner == {-1, 0, 1, 5}
    deg = out["owner"] == 1
    assert deg.any() and not out["normal"][deg].any() and np.isfinite(out["pts"]).all()      # a degenerate face keeps its texels, normal 0
    assert not out["pts"][out["owner"] < 0].any()


# ---- snap ---------------------------------------------------------------------------------------------------------------------------
def _snap1(column, dist=1.0, level=0.0, owner=None):
    t, miss = tx.snap(np.float32(column).reshape(-1, 1), level, dist, owner)
    return float(t[0]), miss


def test_snap_literal_cases():
    # K = 5, dist = 1: h = 0.5, t_k = -1, -0.5, 0, 0.5, 1
    assert tx.snap_offsets(5, 1.0)[0].tolist() == [-1, -0.5, 0, 0.5, 1]
    assert _snap1([1, 1, 1, -1, -1]) == (0.25, 0)                         # one crossing, in [0, 0.5]: 0 + 0.5 * (1 / 2)
    assert _snap1([1, 1, 3, -1, -1]) == (0.375, 0)                        # 0.5 * (3 / 4)
    assert _snap1([-1, 3, 1, -1, -1]) == (0.25, 0)                        # two: -1 + 0.5 / 4 = -0.875 and 0.25 -> the nearer
    assert _snap1([1, -1, -1, -3, 1]) == (-0.75, 0)                       # two: -0.75 and 0.5 + 0.5 * 3 / 4 = 0.875
    assert _snap1([-1, 1, 1, 1, -1]) == (-0.75, 0)                        # a tie, -0.75 and 0.75: the smaller k
    assert _snap1([1, 1, 1, 1, 1]) == (0.0, 1) and _snap1([-1, -1, -1, -1, -1]) == (0.0, 1)      # none
    assert _snap1([1, np.nan, -1, -1, -1]) == (0.0, 1)                    # both intervals next to the NaN are no crossings
    assert _snap1([1, np.nan, 1, -1, -1]) == (0.25, 0)
    assert _snap1([1, np.inf, -1, -1, -1]) == (0.0, 1)
    assert _snap1([1, 1, 1, -1, -1], dist=0.0) == (0.0, 0)                # dist = 0: no snap, nothing counted
    assert _snap1([1, 1, 0, -1, -1]) == (0.0, 0)                          # s = 0 counts as >= 0: the root is t_2 = 0, and it is a snap
    assert _snap1([11, 11, 11, 9, 9], level=10.0) == (0.25, 0)
    assert _snap1([1, 1, 1, 1, 1], owner=np.array([-1])) == (0.0, 0)      # an unowned texel is not counted
    assert _snap1([1, 1, 1, -1, -1], owner=np.array([-1])) == (0.0, 0)


def test_snap_of_a_linear_density_is_exact():
    # sigma = level + 40 (0.3 - t) along the normal crosses at t = 0.3 whatever K
    for K in (3, 9, 17):
        tk, _ = tx.snap_offsets(K, 0.5)
        t, miss = tx.snap((10 + 40 * (0.3 - tk.astype(np.float64))).reshape(K, 1), 10.0, 0.5)
        assert miss == 0 and abs(float(t[0]) - 0.3) < 4 * np.finfo(np.float32).eps


# ---- sampling -----------------------------------------------------------------------------------------------------------------------
def test_sampling_at_a_texel_centre_returns_the_texel():
    rng = np.random.default_rng(0)
    atlas = rng.random((6, 6, 3))
    uv = np.array([[x + 0.5, y + 0.5] for y in range(6) for x in range(6)])
    assert np.array_equal(tx.sample(atlas, uv), atlas.reshape(-1, 3))


def test_sampling_a_linear_ramp_is_exact_and_the_edge_clamps():
    T = 7
    y, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    atlas = np.stack([0.25 * x + 0.5 * y + 1, 2.0 * x, -1.0 * y + 3], -1)
    rng = np.random.default_rng(1)
    uv = 0.5 + rng.random((200, 2)) * (T - 1)
    want = np.stack([0.25 * (uv[:, 0] - 0.5) + 0.5 * (uv[:, 1] - 0.5) + 1, 2 * (uv[:, 0] - 0.5), -(uv[:, 1] - 0.5) + 3], -1)
    assert np.abs(tx.sample(atlas, uv) - want).max() < 1e-13
    # outside the centres of the border texels the border texel is returned
    assert np.array_equal(tx.sample(atlas, [[0.2, 3.5], [-5, 3.5], [6.9, 3.5], [99, 3.5], [3.5, 1e9]]), atlas[[3, 3, 3, 3, 6], [0, 0, 6, 6, 3]])
    assert not tx.sample(atlas, [[np.nan, 1], [1, np.inf], [2.5, 2.5]], mask=[1, 1, 0]).any()


# ---- the whole bake on the sphere: the condition tests/test_gpu_texture.py relies on --------------------------------------------------
def test_reference_bake_of_a_sphere_snaps_every_texel():
    r, level = 0.5, 10.0
    verts, faces = tx.octasphere(2, r)
    assert faces.shape == (128, 3) and np.allclose(np.linalg.norm(verts.astype(np.float64), axis=1), r, atol=1e-7)
    v = verts.astype(np.float64)
    n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    assert ((n * v[faces].mean(1)).sum(1) > 0).all()             # outward winding
    sag = tx.max_sag(verts, faces, r)
    assert 0 < sag < 0.1 * r                                      # (a sanity check of max_sag, nothing depends on the figure)
    A, b = np.array([[0.3, 0.1, 0.0], [0.0, 0.2, 0.1], [0.1, 0.0, 0.3]]), np.array([0.5, 0.4, 0.6])
    field = lambda p: (p @ A.T + b, level + 50 * (r - np.linalg.norm(p, axis=1)))
    dist, K, B = 2 * sag, 9, 8
    out = tx.bake(verts, faces, field, B, dist, level, K)
    assert out["size"] == 64 and (out["owner"] >= 0).all()
    assert out["unsnapped"] == 0
    h = 2 * dist / (K - 1)
    g_min = r - sag - dist                                       # no sample point is nearer to the centre (see test_gpu_texture.py)
    assert np.abs(np.linalg.norm(out["pts"], axis=1) - r).max() <= h * h / (8 * g_min) + 16 * np.finfo(np.float32).eps * r
    assert np.abs(out["atlas"].reshape(-1, 3) - (out["pts"] @ A.T + b)).max() < 1e-12


# ---- the binding --------------------------------------------------------------------------------------------------------------------
def test_texture_header_is_bound():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    d = _lib.declarations("texture")
    assert sorted(d) == NAMES
    for name in NAMES:
        assert d[name].stream == (name != "ia_tex_atlas_size"), name           # every launching entry point takes a stream
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
    assert "ia_texture.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_texture.hip"))
    assert os.path.normpath(_lib.header_path("texture")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_texture.hip" in build.source_manifest() and "ia_texture.hip" in build.library_manifest()
    with pytest.raises(_lib.IAError, match=r"instantavatar_hip_texture\.h"):
        _lib.call("ia_tex_unwrap")


def test_atlas_size_of_the_library_equals_the_reference():
    from instantavatar_amd import _lib
    L = _lib.lib()
    for nf in (0, 1, 2, 3, 7, 8, 9, 33, 127, 128, 129, 4414, 217032, 2 * 256 * 256, 2 * 256 * 256 + 1, 2 * 4096 * 4096, 2 * 4096 * 4096 + 1, 2 ** 31 - 1, -1):
        for B in (3, 4, 5, 8, 16, 64, 65):
            assert L.ia_tex_atlas_size(nf, B) == tx.atlas_size(nf, B), (nf, B)


def test_host_side_argument_errors():
    """what the entry points decide before any launch"""
    from instantavatar_amd import _lib
    P = 4096                                                  # (a non-null address that is never read: every call below is refused)
    for B in (3, 65):
        with pytest.raises(_lib.IAError, match="block edge %d" % B):
            _lib.call("ia_tex_corner_uv", 8, B, 2 * B, P, None)
        with pytest.raises(_lib.IAError, match="block edge %d" % B):
            _lib.call("ia_tex_texel_points", P, 8, P, 8, B, 2 * B, 0, 1, None, 0.0, P, None, None, None)
    big = 2 * 256 * 256 + 1                                   # 257 blocks of 64 per row: 16448 texels
    with pytest.raises(_lib.IAError, match="above 16384"):
        _lib.call("ia_tex_corner_uv", big, 64, 16448, P, None)
    with pytest.raises(_lib.IAError, match="above 16384"):
        _lib.call("ia_tex_texel_points", P, 8, P, big, 64, 16448, 0, 1, None, 0.0, P, None, None, None)
    with pytest.raises(_lib.IAError, match="is not the atlas size"):
        _lib.call("ia_tex_corner_uv", 8, 8, 8, P, None)
    with pytest.raises(_lib.IAError, match="is not the atlas size"):
        _lib.call("ia_tex_texel_points", P, 8, P, 8, 8, 24, 0, 1, None, 0.0, P, None, None, None)
    for nf in (-1,):
        with pytest.raises(_lib.IAError, match="nf = -1"):
            _lib.call("ia_tex_corner_uv", nf, 8, 8, P, None)
    with pytest.raises(_lib.IAError, match="nv = -1"):
        _lib.call("ia_tex_texel_points", P, -1, P, 8, 8, 16, 0, 1, None, 0.0, P, None, None, None)
    for first, count in ((-1, 4), (0, -1), (250, 7), (257, 0)):          # an atlas of 16^2 = 256 texels
        with pytest.raises(_lib.IAError, match="outside the atlas"):
            _lib.call("ia_tex_texel_points", P, 8, P, 8, 8, 16, first, count, None, 0.0, P, None, None, None)
    with pytest.raises(_lib.IAError, match="t_scalar"):
        _lib.call("ia_tex_texel_points", P, 8, P, 8, 8, 16, 0, 4, None, float("nan"), P, None, None, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_tex_texel_points", P, 8, P, 8, 8, 16, 0, 4, None, 0.0, None, None, None, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_tex_texel_points", P, 8, None, 8, 8, 16, 0, 4, None, 0.0, P, None, None, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_tex_corner_uv", 8, 8, 16, None, None)
    for K in (2, 4, 8, 1, 19, 18, -3):
        with pytest.raises(_lib.IAError, match="K = %d" % K):
            _lib.call("ia_tex_snap", P, K, 8, 10.0, 0.1, None, P, P, None)
    with pytest.raises(_lib.IAError, match="n = -1"):
        _lib.call("ia_tex_snap", P, 9, -1, 10.0, 0.1, None, P, P, None)
    for dist in (-0.1, float("inf"), float("nan")):
        with pytest.raises(_lib.IAError, match="dist"):
            _lib.call("ia_tex_snap", P, 9, 8, 10.0, dist, None, P, P, None)
    with pytest.raises(_lib.IAError, match="level"):
        _lib.call("ia_tex_snap", P, 9, 8, float("nan"), 0.1, None, P, P, None)
    for args in ((None, 9, 8, 10.0, 0.1, None, P, P), (P, 9, 8, 10.0, 0.1, None, None, P), (P, 9, 8, 10.0, 0.1, None, P, None)):
        with pytest.raises(_lib.IAError, match="null pointer"):
            _lib.call("ia_tex_snap", *args, None)
    for T in (0, -4, 16385):
        with pytest.raises(_lib.IAError, match="T = %d" % T):
            _lib.call("ia_tex_sample", P, T, P, None, 8, P, None)
    with pytest.raises(_lib.IAError, match="R = -1"):
        _lib.call("ia_tex_sample", P, 16, P, None, -1, P, None)
    for args in ((None, 16, P, None, 8, P), (P, 16, None, None, 8, P), (P, 16, P, None, 8, None)):
        with pytest.raises(_lib.IAError, match="null pointer"):
            _lib.call("ia_tex_sample", *args, None)
    # empty work is accepted without a launch
    assert _lib.call("ia_tex_snap", None, 9, 0, 10.0, 0.1, None, None, None, None) == 0
    assert _lib.call("ia_tex_sample", None, 16, None, None, 0, None, None) == 0
    assert _lib.call("ia_tex_corner_uv", 0, 8, 8, None, None) == 0
    assert _lib.call("ia_tex_texel_points", None, 0, None, 0, 8, 8, 64, 0, None, 0.0, None, None, None, None) == 0


def test_cpu_tensors_and_bad_arguments_raise_in_python():
    from instantavatar_amd import _lib, mesh, raster, texture
    from instantavatar_amd.pipeline import AvatarModel
    f = lambda *s: torch.zeros(s)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    calls = {
        "ia_tex_corner_uv": (8, 8, 16, f(8, 3, 2)),
        "ia_tex_texel_points": (f(8, 3), 8, i(8, 3), 8, 8, 16, 0, 4, None, 0.0, f(4, 3), None, None),
        "ia_tex_snap": (f(9, 8), 9, 8, 10.0, 0.1, None, f(8), i(1)),
        "ia_tex_sample": (f(16, 16, 3), 16, f(8, 2), None, 8, f(8, 3)),
    }
    assert set(calls) == set(NAMES) - {"ia_tex_atlas_size"}
    for name, args in calls.items():
        with pytest.raises(_lib.IAError, match="GPU"):
            _lib.call(name, *args, None)
    m = mesh.Mesh(f(8, 3), i(8, 3), f(8, 3), f(8, 3))
    assert m.texture is None
    field = lambda p: (p, p[:, 0])
    with pytest.raises(_lib.IAError, match="GPU"):
        texture.bake(m, field)
    assert texture.atlas_size(8, 8) == 16 and texture.atlas_size(33, 5) == 25
    for nf, B in ((8, 3), (8, 65), (2 * 256 * 256 + 1, 64), (-1, 8)):
        with pytest.raises(_lib.IAError, match="block edge"):
            texture.atlas_size(nf, B)
    with pytest.raises(_lib.IAError, match="no texture"):
        m.to_obj_textured("unused.obj")
    with pytest.raises(_lib.IAError, match="no texture"):
        raster.render_textured(m, None)
    tex = texture.Texture(f(16, 16, 3), torch.zeros((16, 16, 4), dtype=torch.uint8), f(8, 3, 2), 8, 16, i())
    with pytest.raises(_lib.IAError, match="GPU"):
        texture.sample(tex, f(5, 2))

    class Net:
        center = torch.zeros(3)
    with pytest.raises(_lib.IAError, match="GPU"):
        AvatarModel(None, Net(), None).bake_texture(m)
    assert np.array_equal(texture.snap_offsets(9, 0.3), tx.snap_offsets(9, 0.3)[0])


def test_obj_texture_coordinates():
    from instantavatar_amd import texture
    uv = torch.as_tensor(tx.corner_uv(3, 4), dtype=torch.float32)
    tex = texture.Texture(None, None, uv, 4, 8, None)
    vt = tex.vt()
    assert vt.shape == (3, 3, 2) and vt[0].tolist() == [[0.5 / 8, 1 - 0.5 / 8], [1.5 / 8, 1 - 0.5 / 8], [0.5 / 8, 1 - 1.5 / 8]]
    assert (vt > 0).all() and (vt < 1).all()


def test_the_driver_refuses_bad_flags_before_it_touches_a_device():
    from instantavatar_amd.drivers import extract_mesh as drv
    for argv in (["--synthetic", "--texture", "3"], ["--synthetic", "--texture", "65"], ["--synthetic", "--texture", "-8"],
                 ["--synthetic", "--snap", "2"], ["--synthetic", "--texture", "8", "--snap", "-1"]):
        with pytest.raises(SystemExit):
            drv.main(argv)
