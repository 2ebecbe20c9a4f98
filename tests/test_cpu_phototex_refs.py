"""tests/phototex_refs.py, the float64 reference of the photo texture ("photo texture"), is itself checked here on
cases that can be verified by hand: a triangle that faces the camera under a ramp image, every kind of rejection, two frames of
constant colour, the fallback.  Then the binding table of include/instantavatar_hip_phototex.h, what the entry points and the Python
layer refuse before anything is launched, and that the scenes of the GPU test leave (almost) no texel-frame pair undecided.  No GPU."""
import os

import numpy as np
import pytest
import torch

import phototex_refs as pr

NAMES = ["ia_phototex_acc_bytes", "ia_phototex_accumulate", "ia_phototex_resolve", "ia_phototex_zero"]

# one triangle in the plane z = 2 whose normal (b - a) x (c - a) = (0, 0, -0.49) points at a camera in the origin (w2c = I)
A, B_, C_ = (-0.3, -0.3, 2.0), (-0.3, 0.4, 2.0), (0.4, -0.3, 2.0)
TRI = np.array([A, B_, C_], np.float32)
FACE = np.array([[0, 1, 2]], np.int32)
H, W = 30, 34
INTR = (20.0, 20.0, 10.0, 8.0, 0.1)                   # u = 10 x + 10 in [7, 14], v = 10 y + 8 in [5, 12] on the triangle
EYE = np.eye(4, dtype=np.float32)


def ramp_image():
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.stack([3 * i + 2 * j + 5, 200 - 4 * i - 2 * j, i + 7 * j + 1], -1).astype(np.uint8)


def ramp_at(u, v):
    return np.stack([3 * u + 2 * v + 5, 200 - 4 * u - 2 * v, u + 7 * v + 1], -1) / 255.0


def texel_uv(B):
    """the pixel position of every texel of the one-face atlas, from the weights alone"""
    owner, w = pr.texel_weights(1, B)
    p = w @ TRI.astype(np.float64)
    return owner, np.stack([10 * p[:, 0] + 10, 10 * p[:, 1] + 8], 1)


@pytest.mark.parametrize("B", [4, 5, 8])
def test_a_ramp_image_comes_back_at_the_projected_point_without_a_half_pixel_offset(B):
    depth = np.full((H, W), 2.0, np.float32)
    r = pr.project_frame(TRI, FACE, B, EYE, INTR, ramp_image(), None, depth)
    owner, uv = texel_uv(B)
    assert (owner >= 0).sum() == B * (B - 1) // 2
    assert r["ok"].tolist() == (owner >= 0).tolist()                   # the gutter texels extrapolate, still inside this image
    assert np.abs(r["uv"] - uv)[owner >= 0].max() < 1e-12
    # bilinear filtering reproduces an affine function: pixel (i, j) is sampled AT (i, j)
    assert np.abs(r["colour"] - ramp_at(uv[:, 0], uv[:, 1]))[r["ok"]].max() < 1e-13
    assert np.abs(r["colour"] - ramp_at(uv[:, 0] - 0.5, uv[:, 1] - 0.5))[r["ok"]].max() > 1e-3
    cosine = 2.0 / np.sqrt(((uv[:, 0] - 10) / 10) ** 2 + ((uv[:, 1] - 8) / 10) ** 2 + 4.0)      # n = (0, 0, -1): c = z / |x|
    assert np.abs(r["cos"] - cosine)[r["ok"]].max() < 1e-14 and np.abs(r["weight"] - cosine ** 2)[r["ok"]].max() < 1e-14
    assert r["decided"].all()
    out = pr.bake(TRI, FACE, B, [(TRI, EYE, INTR, ramp_image(), None, depth)])
    assert out["size"] == B and out["unseen"] == 0 and (out["seen"].reshape(-1) == (owner >= 0)).all()
    assert np.abs(out["atlas"].reshape(-1, 3) - ramp_at(uv[:, 0], uv[:, 1]))[owner >= 0].max() < 1e-13
    assert (out["atlas"].reshape(-1, 3)[owner < 0] == 0).all()


def test_every_kind_of_rejection():
    B = 8
    img = ramp_image()
    full = np.full((H, W), 2.0, np.float32)
    owner, uv = texel_uv(B)
    own = owner >= 0
    ok = lambda **kw: pr.project_frame(kw.pop("tri", TRI), FACE, B, kw.pop("w2c", EYE), kw.pop("intr", INTR), kw.pop("img", img),
                                       kw.pop("mask", None), kw.pop("depth", full), **kw)["ok"]
    assert ok().sum() == own.sum() == 28
    assert not ok(depth=np.full((H, W), 1.5, np.float32)).any()          # an occluder in front
    assert not ok(depth=np.full((H, W), 2.5, np.float32)).any()          # the texel in front of what the frame shows: two-sided
    assert ok(depth=np.full((H, W), 2.0199, np.float32)).sum() == 28 and not ok(depth=np.full((H, W), 2.0201, np.float32)).any()
    assert ok(depth=np.full((H, W), 2.5, np.float32), depth_tol=0.6).sum() == 28
    assert not ok(depth=np.zeros((H, W), np.float32)).any()              # not covered
    assert not ok(depth=np.zeros((H, W), np.float32), depth_tol=5.0).any()           # ... whatever the tolerance
    assert not ok(tri=TRI[[0, 2, 1]]).any()                              # back-facing
    cosine = 2.0 / np.sqrt(((uv[:, 0] - 10) / 10) ** 2 + ((uv[:, 1] - 8) / 10) ** 2 + 4.0)      # n = (0, 0, -1): c = z / |x|
    steep = own & (cosine > float(np.float32(0.99)))
    assert 0 < steep.sum() < 28 and ok(cos_min=0.99).tolist() == steep.tolist() and ok(cos_min=0.0).sum() == 28
    assert not ok(intr=INTR[:4] + (2.5,)).any()                          # behind near
    assert not ok(tri=np.array([A, A, C_], np.float32)).any()            # degenerate
    assert not ok(tri=np.array([A, (np.nan, 0, 2), C_], np.float32)).any()
    # one pixel of one footprint
    g = int(np.flatnonzero(own)[10])
    i0, j0 = int(np.floor(uv[g, 0])), int(np.floor(uv[g, 1]))
    for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
        touched = own & (np.floor(uv[:, 0]) >= i0 + di - 1) & (np.floor(uv[:, 0]) <= i0 + di) \
            & (np.floor(uv[:, 1]) >= j0 + dj - 1) & (np.floor(uv[:, 1]) <= j0 + dj)
        assert touched[g]
        mask = np.ones((H, W), np.float32)
        mask[j0 + dj, i0 + di] = 0.0
        assert ok(mask=mask).tolist() == (own & ~touched).tolist()
        mask[j0 + dj, i0 + di] = 0.5                                     # >= 0.5 passes
        assert ok(mask=mask).sum() == 28
        hole = full.copy()
        hole[j0 + dj, i0 + di] = 0.0
        assert ok(depth=hole).tolist() == (own & ~touched).tolist()
    # a footprint that crosses the border of the image: the same scene on narrower and lower images
    for w_img, h_img in ((12, 20), (24, 10), (9, 7)):
        inside = own & (uv[:, 0] >= 0) & (uv[:, 0] < w_img - 1) & (uv[:, 1] >= 0) & (uv[:, 1] < h_img - 1)
        assert 0 < inside.sum() < 28
        assert ok(img=img[:h_img, :w_img], depth=full[:h_img, :w_img]).tolist() == inside.tolist()
    shifted = INTR[:2] + (-6.5, 8.0, 0.1)                               # u = 10 x - 6.5 in [-9.5, -2.5]: left of the image
    assert not ok(intr=shifted).any()


def test_two_frames_of_constant_colour_average_with_the_cosine_weights():
    B = 5
    c1, c2 = np.array([10, 200, 90], np.uint8), np.array([250, 40, 30], np.uint8)
    img = lambda c: np.broadcast_to(c, (H, W, 3)).copy()
    # the second camera stands 1.5 to the right: x' = x - 1.5; the principal point moves so that the triangle stays in the image
    w2c2 = EYE.copy()
    w2c2[0, 3] = -1.5
    intr2 = (20.0, 20.0, 22.0, 8.0, 0.1)
    depth = np.full((H, W), 2.0, np.float32)
    frames = [(TRI, EYE, INTR, img(c1), None, depth), (TRI, w2c2, intr2, img(c2), None, depth)]
    out = pr.bake(TRI, FACE, B, frames, power=2.0)
    owner, w = pr.texel_weights(1, B)
    p = w @ TRI.astype(np.float64)
    own = owner >= 0
    assert (out["seen"].reshape(-1)[own] == 2).all()
    w1 = (2.0 / np.linalg.norm(p, axis=1)) ** 2
    w2 = (2.0 / np.linalg.norm(p - [1.5, 0, 0], axis=1)) ** 2
    want = (w1[:, None] * c1 / 255.0 + w2[:, None] * c2 / 255.0) / (w1 + w2)[:, None]
    assert np.abs(out["atlas"].reshape(-1, 3) - want)[own].max() < 1e-14
    assert (w1 / w2)[own].max() > 1.5                                    # the weights do differ
    # power 0: the plain mean
    out0 = pr.bake(TRI, FACE, B, frames, power=0.0)
    assert np.abs(out0["atlas"].reshape(-1, 3)[own] - (c1 / 255.0 + c2 / 255.0) / 2).max() < 1e-15


def test_min_frames_and_the_base_atlas():
    B = 8
    owner, uv = texel_uv(B)
    own = owner >= 0
    img = np.full((H, W, 3), 51, np.uint8)                               # 0.2
    depth = np.full((H, W), 2.0, np.float32)
    hole = depth.copy()
    g = int(np.flatnonzero(own)[3])
    hole[int(np.floor(uv[g, 1])), int(np.floor(uv[g, 0]))] = 0.0
    frames = [(TRI, EYE, INTR, img, None, depth), (TRI, EYE, INTR, img, None, hole)]
    base = np.random.RandomState(0).rand(B, B, 3)
    out = pr.bake(TRI, FACE, B, frames, base=base, min_frames=2)
    seen = out["seen"].reshape(-1)
    assert seen[g] == 1 and set(seen[own].tolist()) == {1, 2} and (seen[~own] == 0).all()
    atlas, flat = out["atlas"].reshape(-1, 3), base.reshape(-1, 3)
    assert np.abs(atlas[own & (seen == 2)] - 0.2).max() < 1e-15
    assert (atlas[own & (seen == 1)] == flat[own & (seen == 1)]).all()   # seen, but by too few frames: the base
    assert (atlas[~own] == 0).all() and out["unseen"] == 0               # no owner: zero, whatever the base holds
    one = pr.bake(TRI, FACE, B, frames[1:], base=base)
    assert one["unseen"] == (own & (one["seen"].reshape(-1) == 0)).sum() > 0
    unseen = own & (one["seen"].reshape(-1) == 0)
    assert (one["atlas"].reshape(-1, 3)[unseen] == flat[unseen]).all()
    none = pr.bake(TRI, FACE, B, frames[1:])
    assert (none["atlas"].reshape(-1, 3)[unseen] == 0).all()
    empty = pr.bake(TRI, FACE, B, [], base=base)
    assert (empty["atlas"].reshape(-1, 3)[own] == flat[own]).all() and empty["unseen"] == own.sum()


def test_the_reference_depth_map_is_the_plane_of_the_triangle():
    d = pr.raster_depth(TRI, FACE, EYE, INTR, H, W)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    closed = (i >= 7) & (j >= 5) & ((i - 7) + (j - 5) <= 7)          # (pixels ON an edge may fall either way: rounding)
    interior = (i > 7) & (j > 5) & ((i - 7) + (j - 5) < 7)
    assert (d[interior] > 0).all() and (d[~closed] == 0).all() and np.abs(d[d > 0] - 2.0).max() < 1e-6


@pytest.mark.parametrize("nf,B,F", pr.KERNEL_CASES)
def test_the_scenes_of_the_kernel_test_leave_at_most_one_percent_undecided(nf, B, F):
    """the cap of tests/test_gpu_phototex.py, checked on the reference alone for the committed seeds (expected: none undecided), and
    that every scene does exercise acceptance and each kind of rejection that it is meant to hold"""
    case = pr.kernel_case(nf, B, F)
    out = pr.bake(case["verts"], case["faces"], B, case["frames"], **pr.KERNEL_OPTIONS)
    own = out["owner"].reshape(-1) >= 0
    pairs = F * own.sum()
    undecided = (~out["decided"][:, own]).sum()
    assert undecided <= 0.01 * pairs, (undecided, pairs)
    assert out["ok"].sum() > 0, "nothing is accepted"
    assert (~out["ok"][:, own]).sum() > 0, "nothing is rejected"
    assert not out["ok"][:, ~own].any()
    assert case["images"].shape == (F, pr.KERNEL_H, pr.KERNEL_W, 3) and pr.KERNEL_H != pr.KERNEL_W
    m = {k: np.concatenate([r["margins"][k][own] for r in out["per_frame"]]) for k in out["per_frame"][0]["margins"]}
    if F > 1:
        assert (m["near"] < 0).any()                                     # the last camera has a vertex behind `near`
    if nf == 20:
        assert (m["left"] < 0).any() and (m["facing"] < 0).any()
        assert (m["mask"][np.isfinite(m["mask"])] < 0).any() and (m["depth"][np.isfinite(m["depth"])] < 0).any()


# ---- the binding --------------------------------------------------------------------------------------------------------------------
def test_phototex_header_is_bound():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    d = _lib.declarations("phototex")
    assert sorted(d) == NAMES
    assert len(_lib.declarations()) == 89
    for name in NAMES:
        assert d[name].stream == (name != "ia_phototex_acc_bytes"), name       # every launching entry point takes a stream
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
    assert "ia_phototex.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_phototex.hip"))
    assert os.path.normpath(_lib.header_path("phototex")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_phototex.hip" in build.source_manifest() and "ia_phototex.hip" in build.library_manifest()
    with pytest.raises(_lib.IAError, match=r"instantavatar_hip_phototex\.h"):
        _lib.call("ia_phototex_nothing")


def test_accumulator_size():
    from instantavatar_amd import _lib
    assert _lib.call("ia_phototex_acc_bytes", 0) == 0 and _lib.call("ia_phototex_acc_bytes", -1) == 0
    assert _lib.call("ia_phototex_acc_bytes", 1) == 40                    # S [3] and W as fp64, seen as int32, 4 bytes unused
    assert _lib.call("ia_phototex_acc_bytes", 16384 * 16384) == 40 * 16384 * 16384


def test_host_side_argument_errors():
    """what the entry points decide before any launch"""
    from instantavatar_amd import _lib
    P = 4096                                                  # (a non-null, aligned address that is never read: every call below is refused)

    def acc(nv=8, nf=8, B=8, T=16, first=0, count=4, F=1, intr=(100.0, 100.0, 8.0, 8.0, 0.05), H=16, W=16, cos_min=0.3, power=2.0,
            depth_tol=0.02, verts=P, faces=P, w2c=P, images=P, masks=None, depth=P, rec=P):
        return _lib.call("ia_phototex_accumulate", verts, nv, faces, nf, B, T, first, count, F, w2c, *intr, images, masks, depth, H, W,
                         cos_min, power, depth_tol, rec, None)
    for B in (3, 65):
        with pytest.raises(_lib.IAError, match="block edge %d" % B):
            acc(B=B, T=2 * B)
    with pytest.raises(_lib.IAError, match="above 16384"):
        acc(nf=2 * 256 * 256 + 1, B=64, T=16448)
    with pytest.raises(_lib.IAError, match="is not the atlas size"):
        acc(T=24)
    with pytest.raises(_lib.IAError, match="nf = -1"):
        acc(nf=-1)
    with pytest.raises(_lib.IAError, match="nv = -1"):
        acc(nv=-1)
    for first, count in ((-1, 4), (0, -1), (250, 7), (257, 0)):          # an atlas of 16^2 = 256 texels
        with pytest.raises(_lib.IAError, match="outside the atlas"):
            acc(first=first, count=count)
    for F in (0, -1, 65537):
        with pytest.raises(_lib.IAError, match="F = %d" % F):
            acc(F=F)
    for H_, W_ in ((0, 16), (16, 0), (16385, 16), (16, 16385), (-4, 16)):
        with pytest.raises(_lib.IAError, match="image"):
            acc(H=H_, W=W_)
    for bad in (float("nan"), float("inf")):
        for k in range(4):
            intr = [100.0, 100.0, 8.0, 8.0, 0.05]
            intr[k] = bad
            with pytest.raises(_lib.IAError, match="intrinsics"):
                acc(intr=tuple(intr))
    for near in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.IAError, match="near"):
            acc(intr=(100.0, 100.0, 8.0, 8.0, near))
    for c in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(_lib.IAError, match="cos_min"):
            acc(cos_min=c)
    for p in (-1.0, float("nan"), float("inf")):
        with pytest.raises(_lib.IAError, match="power"):
            acc(power=p)
    for d in (-0.01, float("nan"), float("inf")):
        with pytest.raises(_lib.IAError, match="depth_tol"):
            acc(depth_tol=d)
    for null in ("verts", "faces", "w2c", "images", "depth", "rec"):
        with pytest.raises(_lib.IAError, match="null pointer"):
            acc(**{null: None})
    with pytest.raises(_lib.IAError, match="8-byte aligned"):
        acc(rec=P + 4)
    with pytest.raises(_lib.IAError, match="count = -1"):
        _lib.call("ia_phototex_zero", P, -1, None)
    with pytest.raises(_lib.IAError, match="null pointer"):
        _lib.call("ia_phototex_zero", None, 4, None)
    with pytest.raises(_lib.IAError, match="8-byte aligned"):
        _lib.call("ia_phototex_zero", P + 2, 4, None)
    with pytest.raises(_lib.IAError, match="count = -1"):
        _lib.call("ia_phototex_resolve", P, None, P, -1, 1, P, P, P, None)
    for m in (0, -1):
        with pytest.raises(_lib.IAError, match="min_frames = %d" % m):
            _lib.call("ia_phototex_resolve", P, None, P, 4, m, P, P, P, None)
    for args in ((None, None, P, 4, 1, P, P, P), (P, None, None, 4, 1, P, P, P), (P, None, P, 4, 1, None, P, P), (P, None, P, 4, 1, P, None, P),
                 (P, None, P, 4, 1, P, P, None)):
        with pytest.raises(_lib.IAError, match="null pointer"):
            _lib.call("ia_phototex_resolve", *args, None)
    # empty work is accepted without a launch
    assert _lib.call("ia_phototex_zero", None, 0, None) == 0
    assert acc(count=0, rec=None) == 0
    assert acc(nv=0, nf=0, T=8, count=64, faces=None, verts=None, rec=None) == 0
    assert _lib.call("ia_phototex_resolve", None, None, None, 0, 1, None, None, None, None) == 0


def test_cpu_tensors_and_bad_arguments_raise_in_python():
    from instantavatar_amd import _lib, mesh, phototex, raster, texture
    from instantavatar_amd.pipeline import AvatarModel
    f = lambda *s: torch.zeros(s)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    calls = {
        "ia_phototex_zero": (u8(160), 4),
        "ia_phototex_accumulate": (f(1, 8, 3), 8, i(8, 3), 8, 8, 16, 0, 4, 1, f(1, 4, 4), 100.0, 100.0, 8.0, 8.0, 0.05, u8(1, 16, 16, 3), None,
                                   f(1, 16, 16), 16, 16, 0.3, 2.0, 0.02, u8(160)),
        "ia_phototex_resolve": (u8(160), None, i(4), 4, 1, f(4, 3), i(4), i(1)),
    }
    assert set(calls) == set(NAMES) - {"ia_phototex_acc_bytes"}
    for name, args in calls.items():
        with pytest.raises(_lib.IAError, match="GPU"):
            _lib.call(name, *args, None)
    m = mesh.Mesh(f(8, 3), i(8, 3), f(8, 3), f(8, 3))
    with pytest.raises(_lib.IAError, match="GPU"):
        phototex.bake(m, [])
    with pytest.raises(_lib.IAError, match="GPU"):
        phototex.coverage_image(i(16, 16), i(16, 16))

    class Frames:
        images = u8(2, 16, 16, 3)
    with pytest.raises(_lib.IAError, match="GPU"):
        AvatarModel(None, None, None).bake_photo_texture(m, Frames())


def test_the_driver_refuses_photo_without_a_texture_or_a_frame_source():
    from instantavatar_amd.drivers import extract_mesh as drv
    for argv in (["--synthetic", "--photo"], ["--ckpt", "x.ckpt", "--texture", "8", "--photo"],
                 ["--synthetic", "--texture", "8", "--photo", "--photo-frames", "0"]):
        with pytest.raises(SystemExit) as e:
            drv.main(argv)
        assert e.value.code == 2
