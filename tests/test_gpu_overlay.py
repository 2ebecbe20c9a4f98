"""The sequence-inspection kernels on the GPU (csrc/ia_overlay.hip through instantavatar_amd/overlay.py and the C ABI) against the
references of tests/overlay_refs.py, which tests/test_cpu_overlay_refs.py checks on the CPU.  Everything integer -- blend, outline,
skeleton, pixel counts -- is compared for equality, untouched pixels included; the face shade is within one level of the float64
reference (fp32 error of a normalised cross product times 255 is far below one level, so only a rounding tie can differ).  The shapes
are the smallest at which the kernels can go wrong: widths that are no multiple of 4 or of the tile, one and two rows, more than one
tile, pointers that are not aligned.  Then frame independence, refusals that write nothing, the inspector and the driver."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

import overlay_refs as ov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%s: differs at %d places, first at %s: %s, reference %s" % (what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _odd_view(a):
    """the array on the device at an odd byte offset: the kernels' bytewise routes"""
    flat = torch.zeros(a.size + 1, dtype=torch.uint8, device=DEV)
    v = flat[1:].view(a.shape)
    v.copy_(_dev(a))
    return flat, v


# ---- blend --------------------------------------------------------------------------------------------------------------------------------
def _blend_case(n, H, W, seed):
    g = np.random.default_rng(seed)
    images = g.integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    layer = g.integers(0, 256, (n, H, W, 4)).astype(np.uint8)
    alpha = layer[..., 3].reshape(-1).copy()
    edge = np.array([0, 1, 254, 255], np.uint8)
    spread = np.arange(0, alpha.size, max(1, alpha.size // 11))          # the edge alphas, spread over the batch
    alpha[spread] = edge[np.arange(len(spread)) % 4]
    layer[..., 3] = alpha.reshape(n, H, W)
    return images, layer


@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (37, 67), (16, 64), (5, 130)])
def test_blend_exact_aliased_and_not(H, W):
    from instantavatar_amd.overlay import blend
    images, layer = _blend_case(3, H, W, 100 * H + W)
    if H * W > 1:
        assert {0, 1, 254, 255} <= set(layer[..., 3].reshape(-1).tolist())
    img_d, lay_d = _dev(images), _dev(layer)
    for opacity in (0, 1, 128, 255, 256):
        want = ov.blend(images, layer, opacity)
        out = blend(img_d, lay_d, opacity)
        _same(_np(out), want, "blend %dx%d at %d" % (H, W, opacity))
        assert np.array_equal(_np(img_d), images), "out of place: the input is kept"
        inplace = img_d.clone()
        assert blend(inplace, lay_d, opacity, out=inplace) is inplace
        _same(_np(inplace), want, "blend in place %dx%d at %d" % (H, W, opacity))
    _same(_np(blend(img_d, lay_d, 0)), images, "opacity 0 is the image")
    # pointers at odd offsets: the bytewise route, in place; the byte in front is not touched
    flat, odd = _odd_view(images)
    _, odd_layer = _odd_view(layer)
    blend(odd, odd_layer, 77, out=odd)
    _same(_np(odd), ov.blend(images, layer, 77), "blend bytewise %dx%d" % (H, W))
    assert flat[0] == 0
    _same(_np(blend(_dev(images[0]), _dev(layer[0]), 200)), ov.blend(images[0], layer[0], 200), "[H,W,3] in, [H,W,3] out")


# ---- outline ------------------------------------------------------------------------------------------------------------------------------
def _outline_masks(H, W, seed):
    g = np.random.default_rng(seed)
    coarse = g.random((H // 4 + 2, W // 4 + 2)) < 0.55
    blobs = np.kron(coarse, np.ones((4, 4), bool))[:H, :W].astype(bool)
    noise = g.random((H, W)) < 0.5
    frames = [np.where(blobs, g.integers(1, 256, (H, W)), 0), np.where(noise, 255, 0), np.full((H, W), 255), np.zeros((H, W), int)]
    for side in range(4):                      # a block that touches one border, zero elsewhere; and its complement
        m = np.zeros((H, W), int)
        if side == 0:
            m[:, :max(1, W // 3)] = 255
        elif side == 1:
            m[:, W - max(1, W // 3):] = 255
        elif side == 2:
            m[:max(1, H // 3), :] = 7
        else:
            m[H - max(1, H // 3):, :] = 1
        frames += [m, np.where(m > 0, 0, 200)]
    return np.stack(frames).astype(np.uint8)


@pytest.mark.parametrize("W", [1, 5, 63, 64, 65, 130])
def test_outline_exact_with_untouched_pixels(W):
    from instantavatar_amd.overlay import outline
    for H in (1, 2, 37):
        masks = _outline_masks(H, W, 10 * W + H)
        images = np.random.default_rng(W + H).integers(0, 256, masks.shape + (3,)).astype(np.uint8)
        m_d = _dev(masks)
        for t in (1, 2, 8):
            rgb = (250 - t, 3 + t, 128)
            img_d = _dev(images)
            assert outline(img_d, m_d, t, rgb) is img_d
            _same(_np(img_d), ov.outline(images, masks, t, rgb), "outline %dx%d t = %d" % (H, W, t))
    # a tall frame: more than one tile of rows, the halo rows of a tile come from its neighbours
    masks = _outline_masks(70, W, W)[:2]
    images = np.zeros(masks.shape + (3,), np.uint8)
    _same(_np(outline(_dev(images), _dev(masks), 8, (1, 2, 3))), ov.outline(images, masks, 8, (1, 2, 3)), "outline 70x%d t = 8" % W)


# ---- skeleton -----------------------------------------------------------------------------------------------------------------------------
SIZES = [(37, 67), (64, 64)]
RGB = [((37 * s + 11) % 256, (91 * s + 5) % 256, (53 * s + 200) % 256) for s in range(64)]


def _skeleton(H, W, points, segments, hw, rad, thr=0.2, what="", seed=0):
    """points [n,K,3]: draws on a seeded random batch, compares every byte"""
    from instantavatar_amd.overlay import draw_skeleton
    points = np.asarray(points, np.float32)
    n = points.shape[0]
    images = np.random.default_rng(seed).integers(0, 256, (n, H, W, 3)).astype(np.uint8)
    seg = np.asarray(segments, np.int64).reshape(-1, 2)
    col = np.asarray(RGB[:len(seg)], np.uint8).reshape(-1, 3)
    img_d = _dev(images)
    assert draw_skeleton(img_d, _dev(points), seg.tolist(), col.tolist(), (9, 250, 30), thr, hw, rad) is img_d
    want = ov.skeleton(images, points, seg, col, (9, 250, 30), thr, hw, rad)
    _same(_np(img_d), want, "skeleton %s %dx%d hw %d rad %d" % (what, H, W, hw, rad))
    return images, want


def _three(points):
    """a frame -> three: as it is, moved by a quarter pixel, moved by (0.375, -0.625)"""
    p = np.asarray(points, np.float32)
    q, r = p.copy(), p.copy()
    q[:, :2] += 0.25
    r[:, 0] += 0.375
    r[:, 1] -= 0.625
    return np.stack([p, q, r])


@pytest.mark.parametrize("H,W", SIZES)
def test_skeleton_geometry(H, W):
    c = 1.0
    pts = [[5, 10, c], [40, 10, c], [20, 3, c], [20, 30, c], [8, 8, c], [30, 30, c], [50, 20, c], [50, 20, c]]
    segs = [(0, 1), (2, 3), (4, 5), (6, 6), (6, 7)]            # horizontal, vertical, diagonal, zero length twice
    for hw, rad in ((1, 0), (6, 10), (64, 128), (1, 128), (64, 0)):
        images, want = _skeleton(H, W, _three(pts), segs, hw, rad, what="lines")
        assert (want != images).any()
    # ends outside the image: negative, beyond W and H, and both outside with the line crossing the image
    pts = [[-20, 10, c], [30, 12, c], [10, 5, c], [W + 40, H + 9, c], [-15, -9, c], [W + 25, H + 31, c], [-3, H + 5, c], [W + 2, -7, c]]
    images, want = _skeleton(H, W, _three(pts), [(0, 1), (2, 3), (4, 5), (6, 7)], 5, 7, what="outside")
    assert (want != images).any()
    # overlapping segments and discs: the order rule
    pts = [[10, 10, c], [50, 30, c], [10, 30, c], [50, 10, c], [30, 5, c], [30, 35, c], [30, 20, c]]
    _skeleton(H, W, _three(pts), [(0, 1), (2, 3), (4, 5), (0, 3), (1, 2), (6, 0)], 10, 14, what="overlap")
    _skeleton(H, W, _three(pts), [(6, 0), (1, 2), (0, 3), (4, 5), (2, 3), (0, 1)], 10, 14, what="overlap reversed")


@pytest.mark.parametrize("H,W", SIZES)
def test_skeleton_validity(H, W):
    nan, inf = float("nan"), float("inf")
    thr = 0.3
    below, equal, above = 0.29, float(np.float32(0.3)), float(np.nextafter(np.float32(0.3), np.float32(1)))
    pts = [[10, 10, 1], [40, 12, below], [40, 20, equal], [40, 28, above], [nan, 10, 1], [20, inf, 1], [20, 20, nan], [25, 25, inf],
           [32768.5, 10, 1], [10, -32769, 1], [30, 5, 1], [-inf, 5, 1]]
    segs = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7), (0, 8), (0, 9), (0, 10), (0, 11), (-1, 0), (0, 12), (12, 0), (3, -5), (10, 2 ** 30)]
    images, want = _skeleton(H, W, _three(pts), segs, 4, 9, thr=thr, what="validity")
    drawn = ov.skeleton(images, _three(pts), [(0, 3), (0, 10)], [RGB[2], RGB[9]], (9, 250, 30), thr, 4, 9)
    assert np.array_equal(want, drawn), "of the sixteen segments only (0, 3) and (0, 10) have two valid ends"
    # S = 0 (discs only), K = 1, and a frame in which nothing is valid: not a byte changes
    _skeleton(H, W, _three(pts), [], 1, 12, thr=thr, what="S = 0")
    _skeleton(H, W, _three([[12.5, 9.25, 1]]), [(0, 0)], 7, 3, what="K = 1")
    images, want = _skeleton(H, W, _three([[10, 10, 0.2], [nan, nan, nan]]), [(0, 1), (0, 0)], 64, 128, thr=0.2, what="nothing valid")
    assert np.array_equal(images, want)


@pytest.mark.parametrize("H,W", SIZES)
def test_skeleton_quarter_pixel_ties_and_the_far_ends(H, W):
    # coordinates on eighths: 4 x + 0.5 is then an integer or a half, and distances land on the bound
    pts = [[k + e, 7 + 3 * k + e2, 1] for k, (e, e2) in enumerate([(0.125, 0), (0.375, 0.125), (0.625, 0.875), (0.875, 0.5), (-0.125, 0.25), (0.5, 0.625)])]
    pts = [[4 + 9 * i + p[0], p[1], 1] for i, p in enumerate(pts)]
    for hw, rad in ((3, 3), (4, 5), (2, 8)):
        _skeleton(H, W, _three(pts), [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 5), (0, 0)], hw, rad, what="ties")
    # ends at +-32768: the diagonal through the image, and a line whose bounding box touches column 0 while it passes 23 170 pixels
    # away (cross product 2^34: its square does not fit 64 bits)
    far = 32768.0
    pts = [[-far, -far, 1], [far, far, 1], [-far, 0, 1], [0, far, 1], [far, -far, 1], [-far, far, 1]]
    images, want = _skeleton(H, W, np.stack([pts] * 3), [(0, 1), (2, 3), (4, 5)], 2, 0, what="far ends")
    assert (want != images).any(-1).sum() == 3 * min(H, W), "the diagonal of every frame, and nothing of the other two lines"
    _skeleton(H, W, np.stack([pts] * 3), [(0, 1), (2, 3), (4, 5), (1, 2), (3, 4)], 64, 128, what="far ends, wide")


def test_skeleton_200_random():
    H, W = SIZES[0]
    g = np.random.default_rng(2024)
    for call in range(8):                      # 8 calls of 25 frames
        K, S = int(g.integers(1, 65)) if call else 64, int(g.integers(0, 13)) if call else 12
        pts = np.concatenate([g.uniform(-20, [W + 20, H + 20], (25, K, 2)), g.random((25, K, 1))], -1)
        pts[..., :2] = np.round(pts[..., :2] * 8) / 8 if call % 2 else pts[..., :2]          # every other call on eighths: ties
        segs = g.integers(-1, K + 1, (S, 2))
        _skeleton(H, W, pts, segs, int(g.integers(1, 65)), int(g.integers(0, 129)), thr=0.4, what="random call %d" % call, seed=call)
    # the 24 limbs of BODY_25 in the module's own tables
    from instantavatar_amd import overlay
    pts = np.concatenate([g.uniform(0, [W, H], (3, 25, 2)), g.random((3, 25, 1))], -1).astype(np.float32)
    images = g.integers(0, 256, (3, H, W, 3)).astype(np.uint8)
    got = _np(overlay.draw_skeleton(_dev(images), _dev(pts)))
    want = ov.skeleton(images, pts, overlay.BODY25_SEGMENTS, overlay.LIMB_COLOURS, overlay.MODEL_POINT_COLOUR, 0.2, overlay.HALF_WIDTH_Q,
                       overlay.MODEL_RADIUS_Q)
    _same(got, want, "BODY_25 defaults")


# ---- stats --------------------------------------------------------------------------------------------------------------------------------
def _stats(a, b):
    from instantavatar_amd.overlay import mask_stats
    r = mask_stats(a, b)
    return np.stack([_np(r.inter), _np(r.union), _np(r.a_area), _np(r.b_area)], -1), _np(r.iou)


@pytest.mark.parametrize("W", [63, 64, 65, 255, 256, 257])
def test_stats_exact(W):
    g = np.random.default_rng(W)
    for H in (1, 5):
        a = np.where(g.random((3, H, W)) < 0.5, g.integers(1, 256, (3, H, W)), 0).astype(np.uint8)
        b = np.where(g.random((3, H, W)) < 0.4, g.integers(1, 256, (3, H, W)), 0).astype(np.uint8)
        a[1], b[1] = 255, 1                    # full
        a[2] = 0                               # empty against random
        want = ov.stats(a, b)
        got, iou = _stats(_dev(a), _dev(b))
        _same(got, want, "stats %dx%d" % (H, W))
        assert np.array_equal(iou, np.where(want[:, 1] > 0, want[:, 0].astype(np.float32) / np.maximum(want[:, 1], 1).astype(np.float32), 0).astype(np.float32))
        assert iou[1] == 1.0 and iou[2] == 0.0
        # bool tensors are valid input; so are frames that do not start on 16 bytes (a head in front of the wide body) and two masks
        # at different offsets (bytewise)
        _same(_stats(_dev(a) > 0, _dev(b) > 0)[0], want, "stats of bool %dx%d" % (H, W))
        fa, va = _odd_view(a)
        fb, vb = _odd_view(b)
        _same(_stats(va, vb)[0], want, "stats, both one byte off, %dx%d" % (H, W))
        _same(_stats(va, _dev(b))[0], want, "stats, one of them a byte off, %dx%d" % (H, W))
    e = torch.zeros((2, 3, W), dtype=torch.uint8, device=DEV)
    got, iou = _stats(e, e)
    assert not got.any() and not iou.any(), "union == 0 gives iou = 0"


def test_stats_of_a_large_frame_and_again():
    from instantavatar_amd.overlay import mask_stats
    full = torch.full((1, 1024, 1024), 255, dtype=torch.uint8, device=DEV)
    half = full.clone()
    half[:, :, 512:] = 0
    got, iou = _stats(full, half)
    assert got.tolist() == [[1 << 19, 1 << 20, 1 << 20, 1 << 19]] and iou.tolist() == [0.5]
    again, _ = _stats(full, half)
    assert np.array_equal(got, again)
    g = np.random.default_rng(1)
    a = (g.random((3, 300, 500)) < 0.5).astype(np.uint8)
    b = (g.random((3, 300, 500)) < 0.5).astype(np.uint8)
    first, second = _stats(_dev(a), _dev(b))[0], _stats(_dev(a), _dev(b))[0]
    _same(first, ov.stats(a, b), "stats 300x500")
    assert np.array_equal(first, second)
    r = mask_stats(_dev(a[0]), _dev(b[0]))     # [H,W] in, 0-d out
    assert r.inter.dim() == 0 and int(r.inter) == first[0, 0] and int(r.b_area) == first[0, 3]


# ---- face shade ---------------------------------------------------------------------------------------------------------------------------
def _shade(fid, verts, faces, w2c, tint, what):
    from instantavatar_amd.overlay import face_shade
    got = _np(face_shade(_dev(fid.astype(np.int32)), _dev(verts.astype(np.float32)), _dev(faces.astype(np.int32)), _dev(w2c.astype(np.float32)), tint))
    ref = ov.face_shade(fid, verts.astype(np.float32), faces, w2c.astype(np.float32), tint)
    want = np.floor(ref + np.array([0.5, 0.5, 0.5, 0])).astype(np.int64)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got[..., 3], want[..., 3]), what + ": alpha is 255 on covered pixels and 0 elsewhere, exactly"
    empty = want[..., 3] == 0
    assert not got[empty].any(), what + ": empty pixels are four zero bytes"
    assert np.abs(got.astype(np.int64) - want).max() <= 1, what
    return got, want


def test_face_shade_cases():
    rot = lambda ax, a: np.array({0: [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]],
                                  1: [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]}[ax])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = rot(0, 0.4) @ rot(1, -0.7), [0.1, -0.2, 3.0]
    # a tetrahedron, a quad wound away from the camera (|n_z|: it is shaded like its front), a degenerate face, a face with a vertex
    # index out of range and one with a negative index
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0.5], [2, 1, 0.5], [3, 1, 0.7], [3, 0, 0.7]], np.float64)
    faces = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3], [4, 5, 6], [4, 6, 7], [0, 1, 1], [3, 3, 3], [0, 1, 8], [0, -1, 2]])
    g = np.random.default_rng(3)
    for H, W in ((1, 1), (5, 7), (37, 67)):
        fid = g.integers(-1, len(faces), (H, W))
        fid.reshape(-1)[:: 7] = [-1, len(faces), 2 ** 31 - 1, -(2 ** 31), 8, 9, 6][H % 7]          # damaged ids and the damaged faces
        got, want = _shade(fid, verts, faces, w2c, (90, 170, 255), "%dx%d" % (H, W))
    fid = np.arange(-1, 11).reshape(3, 4)
    got, want = _shade(fid, verts, faces, w2c, (200, 100, 50), "one pixel per face")
    flat = got.reshape(-1, 4)
    assert not flat[0].any() and not flat[9:].any(), "id -1, the faces with damaged indices and ids >= nf are empty"
    assert flat[7].tolist() == [50, 25, 13, 255] == flat[8].tolist(), "degenerate: s = 0.25 (12.5 rounds up)"
    assert (flat[1:7, 3] == 255).all() and np.abs(flat[5].astype(int) - flat[6].astype(int)).max() <= 1, "the two halves of the planar quad share a shade"
    flipped = faces.copy()
    flipped[4:6] = flipped[4:6, ::-1]
    back = _shade(fid, verts, flipped, w2c, (200, 100, 50), "flipped quad")[0]
    assert np.abs(back[1, 1:3].astype(int) - got[1, 1:3].astype(int)).max() <= 1 and (back[1, 1:3, 3] == 255).all(), "|n_z|: winding does not matter"
    # through the rasteriser: every covered pixel of a tetrahedron gets a shade, nothing else does
    from instantavatar_amd.raster import Camera, rasterize
    K = np.array([[60.0, 0, 24], [0, 60.0, 24], [0, 0, 1]])
    cam = Camera(K, _dev(w2c.astype(np.float32)), 48, 48)
    frame = rasterize(_dev(verts[:4].astype(np.float32)), _dev(faces[:4].astype(np.int32)), cam)
    got, _ = _shade(_np(frame.face_id), verts[:4], faces[:4], w2c, (90, 170, 255), "rasterised tetrahedron")
    assert np.array_equal(got[..., 3] == 255, _np(frame.mask)) and _np(frame.mask).sum() > 50


# ---- frame independence -------------------------------------------------------------------------------------------------------------------
def test_a_frame_gives_the_same_bytes_at_another_batch_position():
    from instantavatar_amd import overlay
    H, W = 37, 67
    g = np.random.default_rng(8)
    images, layer = _blend_case(3, H, W, 5)
    masks = _outline_masks(H, W, 5)[[0, 1, 4]]
    pts = np.concatenate([g.uniform(0, [W, H], (3, 25, 2)), g.random((3, 25, 1))], -1).astype(np.float32)

    def run(order):
        o = list(order)
        out = overlay.blend(_dev(images[o]), _dev(layer[o]), 140)
        overlay.outline(out, _dev(masks[o]), 2)
        overlay.draw_skeleton(out, _dev(pts[o]))
        return _np(out), _stats(_dev(masks[o]), _dev(layer[o][..., 3]))[0]

    base, base_stats = run([0, 1, 2])
    for order in ([2, 0, 1], [1], [1, 1, 0]):
        got, got_stats = run(order)
        assert np.array_equal(got, base[order]) and np.array_equal(got_stats, base_stats[order]), order


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    from instantavatar_amd import _lib, overlay
    n, H, W = 2, 6, 9
    u8 = lambda *shape: torch.full(shape, 171, dtype=torch.uint8, device=DEV)
    images, layer, out, masks = u8(n, H, W, 3), u8(n, H, W, 4), u8(n, H, W, 3), u8(n, H, W)
    counts = torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    pts = torch.ones((n, 4, 3), device=DEV)
    seg = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    col = u8(2, 3)
    fid = torch.zeros((H, W), dtype=torch.int32, device=DEV)
    verts, faces, w2c = torch.rand((4, 3), device=DEV), torch.zeros((2, 3), dtype=torch.int32, device=DEV), torch.eye(4, device=DEV)
    layer1 = u8(H, W, 4)
    need = int(_lib.call("ia_overlay_stats_workspace_bytes", n, H, W))
    assert need > 0 and _lib.call("ia_overlay_stats_workspace_bytes", 0, H, W) == 0 and _lib.call("ia_overlay_stats_workspace_bytes", 1, 0, W) == 0
    assert _lib.call("ia_overlay_stats_workspace_bytes", 1, 1 << 16, 1 << 15) == 0 and _lib.call("ia_overlay_stats_workspace_bytes", 70000, H, W) == 0
    ws = u8(need + 64)
    blend = lambda *a: _lib.call("ia_overlay_blend", *a)
    outline = lambda *a: _lib.call("ia_overlay_outline", *a)
    shade = lambda *a: _lib.call("ia_overlay_face_shade", *a)
    skel = lambda *a: _lib.call("ia_overlay_skeleton", *a)
    stats = lambda *a: _lib.call("ia_overlay_stats", *a)
    sk = lambda **kw: skel(*[kw.get(k, v) for k, v in (("points", pts), ("n", n), ("K", 4), ("segments", seg), ("rgb", col), ("S", 2), ("r", 1), ("g", 2), ("b", 3),
                                                        ("thr", 0.5), ("hw", 4), ("rad", 4), ("H", H), ("W", W), ("images", images))])
    for call, match in ((lambda: blend(images, layer, n, H, W, 128, out, None), r"stream = NULL"),
                        (lambda: outline(masks, n, H, W, 2, 1, 2, 3, images, None), r"stream = NULL"),
                        (lambda: shade(fid, H, W, verts, 4, faces, 2, w2c, 1, 2, 3, layer1, None), r"stream = NULL"),
                        (lambda: skel(pts, n, 4, seg, col, 2, 1, 2, 3, 0.5, 4, 4, H, W, images, None), r"stream = NULL"),
                        (lambda: stats(masks, masks, n, H, W, counts, ws, need, None), r"stream = NULL")):
        with pytest.raises(_lib.IAError, match=match):
            call()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for call, match in (
                (lambda: blend(images, layer, 0, H, W, 128, out), r"0 frames"), (lambda: blend(images, layer, n, 0, W, 128, out), r"2 frames of 0 x 9"),
                (lambda: blend(images, layer, n, H, -1, 128, out), r"6 x -1"), (lambda: blend(images, layer, n, H, W, 257, out), r"opacity 257"),
                (lambda: blend(images, layer, n, H, W, -1, out), r"opacity -1"), (lambda: blend(images, None, n, H, W, 128, out), r"are required"),
                (lambda: blend(images, layer, n, H, W, 128, None), r"are required"),
                (lambda: blend(images, layer, 1, H, W, 128, images.view(-1)[3:].data_ptr()), r"not overlap it otherwise"),
                (lambda: outline(masks, n, H, W, 0, 1, 2, 3, images), r"thickness 0"), (lambda: outline(masks, n, H, W, 9, 1, 2, 3, images), r"thickness 9"),
                (lambda: outline(masks, n, H, W, 2, 256, 2, 3, images), r"colour \(256, 2, 3\)"), (lambda: outline(None, n, H, W, 2, 1, 2, 3, images), r"are required"),
                (lambda: outline(masks, n, H, 0, 2, 1, 2, 3, images), r"6 x 0"),
                (lambda: shade(fid, H, W, verts, 4, faces, 0, w2c, 1, 2, 3, layer1), r"0 faces"), (lambda: shade(fid, H, W, verts, 0, faces, 2, w2c, 1, 2, 3, layer1), r"0 vertices"),
                (lambda: shade(fid, 0, W, verts, 4, faces, 2, w2c, 1, 2, 3, layer1), r"0 x 9"), (lambda: shade(fid, H, W, verts, 4, faces, 2, w2c, 1, -2, 3, layer1), r"tint"),
                (lambda: shade(fid, H, W, verts, 4, faces, 2, None, 1, 2, 3, layer1), r"are required"),
                (lambda: shade(fid, H, W, verts, 4, faces, 2, w2c, 1, 2, 3, layer1.view(-1)[1:].data_ptr()), r"4-byte aligned"),
                (lambda: sk(K=0), r"K = 0"), (lambda: sk(K=65), r"K = 65"), (lambda: sk(S=-1), r"S = -1"), (lambda: sk(S=65), r"S = 65"),
                (lambda: sk(hw=0), r"half_width_q 0"), (lambda: sk(hw=65), r"half_width_q 65"), (lambda: sk(rad=-1), r"radius_q -1"),
                (lambda: sk(rad=129), r"radius_q 129"), (lambda: sk(b=300), r"point colour"), (lambda: sk(thr=float("nan")), r"threshold is NaN"),
                (lambda: sk(segments=None), r"segments and segment_rgb when S > 0"), (lambda: sk(points=None), r"are required"),
                (lambda: sk(n=0), r"0 frames"), (lambda: sk(W=40000), r"6 x 40000"),
                (lambda: stats(masks, masks, n, H, W, counts, ws, need - 1), r"workspace of \d+ bytes, \d+ needed"),
                (lambda: stats(masks, masks, n, H, W, counts, None, need), r"workspace of 0 bytes"),
                (lambda: stats(masks, None, n, H, W, counts, ws, need), r"are required"), (lambda: stats(masks, masks, -1, H, W, counts, ws, need), r"-1 frames")):
            with pytest.raises(_lib.IAError, match=match):
                call()
    side.synchronize()
    for t in (images, layer, out, masks, col, layer1, ws):
        assert (t == 171).all(), "a refused call wrote something"
    assert (counts == -7).all()
    # the module's own checks
    with pytest.raises(_lib.IAError, match="no CPU path"):
        overlay.blend(images.cpu(), layer.cpu())
    with pytest.raises(_lib.IAError, match="uint8"):
        overlay.mask_stats(masks.float(), masks.float())
    with pytest.raises(_lib.IAError, match=r"2 segments but 1 colours"):
        overlay.draw_skeleton(images, pts, [(0, 1), (1, 2)], [(1, 2, 3)])
    # and nothing is written behind the last element: stats' workspace and outputs at their stated sizes
    with torch.cuda.stream(side):
        stats(masks, masks, n, H, W, counts, ws, need)
    side.synchronize()
    assert (ws[need:] == 171).all() and counts.tolist() == [[H * W] * 4] * 2


# ---- the inspector --------------------------------------------------------------------------------------------------------------------------
H0 = W0 = 48
K0 = np.array([[2000.0 * 48 / 1080, 0, 24], [0, 2000.0 * 48 / 1080, 24], [0, 0, 1]])


def _truth(body_dict, n=3):
    """-> body, kp_vertex, (betas, pose, transl) on the device, keypoints [n,25,3] = the kernel's own projections at these poses with
    confidence 1, masks [n,H,W] bool = the rasteriser's own silhouettes"""
    from instantavatar_amd import synthetic
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.keypoints import SMPL_KP_VERTEX, KeypointRefiner
    from instantavatar_amd.raster import Camera, rasterize
    body = SMPL.from_dict(body_dict).to(DEV)
    kpv = tuple(v % int(body.v_template.shape[0]) for v in SMPL_KP_VERTEX)
    poses, tr = synthetic.procedural_pose_track(8)
    params = (torch.zeros(10, device=DEV), _dev(poses[:n].astype(np.float32)), _dev(tr[:n].astype(np.float32)))
    r = KeypointRefiner(body, (K0 @ np.eye(4)[:3]).astype(np.float32), np.zeros((n, 25, 3), np.float32), kp_vertex=kpv)
    o = r.loss(*params)
    kp = torch.cat([o["uv"], torch.ones((n, 25, 1), device=DEV)], -1)
    cam = Camera(K0, torch.eye(4, device=DEV), H0, W0)
    masks = torch.stack([rasterize(o["verts"][f], body.faces_tensor, cam).mask for f in range(n)])
    return body, kpv, params, kp, masks


@functools.lru_cache(maxsize=None)
def _small():
    from instantavatar_amd import synthetic
    return _truth(synthetic.make_mesh_body(sides=3, rings=2))


def test_inspector_is_exact_on_its_own_silhouettes_and_projections():
    from instantavatar_amd.overlay import SequenceInspector, worst_frames
    body, kpv, params, kp, masks = _small()
    assert masks.sum((1, 2)).min() > 20
    insp = SequenceInspector(body, K0, np.eye(4), H0, W0, keypoints=kp, masks=masks, kp_vertex=kpv)
    rep = {k: _np(v) for k, v in insp.report(*params).items()}
    assert sorted(rep) == ["inter", "iou", "kp_err_px", "mask_area", "n_confident", "sil_area", "union"] and all(v.shape == (3,) for v in rep.values())
    assert np.array_equal(rep["inter"], rep["union"]) and np.array_equal(rep["inter"], rep["mask_area"]) and np.array_equal(rep["inter"], rep["sil_area"])
    assert np.array_equal(rep["mask_area"], _np(masks.sum((1, 2)))) and (rep["iou"] == 1.0).all()
    assert (rep["kp_err_px"] == 0).all() and (rep["n_confident"] == 24).all(), "MidHip is not counted"
    # frame 1 moved: it alone is off, and it heads the list of the worst
    betas, pose, transl = (p.clone() for p in params)
    pose[1, 3 * 16 + 2] += 0.9
    transl[1, 0] += 0.25
    moved = insp.report(betas, pose, transl)
    m = {k: _np(v) for k, v in moved.items()}
    assert m["iou"][1] < 1 and m["kp_err_px"][1] > 0 and m["inter"][1] < m["union"][1]
    for f in (0, 2):
        assert m["iou"][f] == 1.0 and m["kp_err_px"][f] == 0
    assert worst_frames(moved, 1) == [1] and worst_frames(moved, 3)[0] == 1 and worst_frames(moved, 0) == []
    # keypoints alone, masks alone, neither
    rk = SequenceInspector(body, K0, np.eye(4), H0, W0, keypoints=kp, kp_vertex=kpv).report(betas, pose, transl)
    assert sorted(rk) == ["kp_err_px", "n_confident"] and np.array_equal(_np(rk["kp_err_px"]), m["kp_err_px"]) and worst_frames(rk, 1) == [1]
    rm = SequenceInspector(body, K0, np.eye(4), H0, W0, masks=masks.to(torch.uint8) * 255, kp_vertex=kpv).report(betas, pose, transl)
    assert sorted(rm) == ["inter", "iou", "mask_area", "sil_area", "union"] and np.array_equal(_np(rm["iou"]), m["iou"])
    with pytest.raises(ValueError, match="neither keypoints nor masks"):
        SequenceInspector(body, K0, np.eye(4), H0, W0, kp_vertex=kpv)
    # confidence at the threshold is not counted
    low = kp.clone()
    low[0, :, 2] = 0.2
    low[2, 3:, 2] = 0.1
    rl = SequenceInspector(body, K0, np.eye(4), H0, W0, keypoints=low, kp_vertex=kpv, threshold=0.2).report(*params)
    assert _np(rl["n_confident"]).tolist() == [0, 24, 3] and _np(rl["kp_err_px"]).tolist() == [0, 0, 0]


def _regions(insp, params, idx):
    """the pixels `overlay` may change, layer by layer through the module: silhouette, outline, detected skeleton, model points"""
    from instantavatar_amd import overlay
    from instantavatar_amd.raster import rasterize
    verts, uv = insp._posed(*params)
    sil = torch.stack([rasterize(verts[f], insp.faces, insp.camera).mask for f in idx])
    sel = torch.as_tensor(idx, device=DEV)
    blank = lambda: torch.zeros((len(idx), insp.H, insp.W, 3), dtype=torch.uint8, device=DEV)
    line = overlay.outline(blank(), insp.masks[sel], 2, (1, 1, 1)).any(-1) if insp.has_masks else torch.zeros_like(sil)
    lim = [(1, 1, 1)] * 24
    det = overlay.draw_skeleton(blank(), insp.keypoints[sel], overlay.BODY25_SEGMENTS, lim, (1, 1, 1), insp.threshold, overlay.HALF_WIDTH_Q,
                                overlay.DETECTION_RADIUS_Q).any(-1) if insp.has_keypoints else torch.zeros_like(sil)
    model = torch.cat([uv[sel], torch.ones((len(idx), 25, 1), device=DEV)], -1)
    pts = overlay.draw_skeleton(blank(), model, (), (), (1, 1, 1), 0.5, overlay.HALF_WIDTH_Q, overlay.MODEL_RADIUS_Q).any(-1)
    return tuple(_np(t.bool()) for t in (sil, line, det, pts))      # (torch's any() of uint8 is uint8)


def test_inspector_overlay_changes_its_layers_pixels_only():
    from instantavatar_amd import overlay
    body, kpv, params, kp, masks = _small()
    insp = overlay.SequenceInspector(body, K0, np.eye(4), H0, W0, keypoints=kp, masks=masks, kp_vertex=kpv)
    images = np.random.default_rng(0).integers(0, 40, (2, H0, W0, 3)).astype(np.uint8)          # dark: every layer colour differs from it
    img_d = _dev(images)
    out = _np(insp.overlay(img_d, [2, 0], *params))
    assert np.array_equal(_np(img_d), images) and out.shape == images.shape and out.dtype == np.uint8
    sil, line, det, pts = _regions(insp, params, [2, 0])
    region = sil | line | det | pts
    assert sil.sum() > 40 and line.sum() > 10 and det.sum() > 10 and pts.sum() > 10
    assert np.array_equal(out[~region], images[~region]), "a pixel outside every layer changed"
    assert (out[region] != images[region]).any(-1).all(), "a pixel inside a layer kept its colour"
    assert (out[pts] == np.array(overlay.MODEL_POINT_COLOUR, np.uint8)).all(), "the model points lie on top"
    body_only = sil & ~line & ~det & ~pts
    lay = np.stack([_np(overlay.face_shade(_rast(insp, params, f), insp._posed(*params)[0][f], insp.faces, insp.camera.w2c)) for f in (2, 0)])
    assert np.array_equal(out[body_only], ov.blend(images, lay, 128)[body_only])
    assert np.array_equal(_np(insp.overlay(img_d, [2, 0], *params, opacity=0.0))[~(line | det | pts)], images[~(line | det | pts)])
    with pytest.raises(ValueError, match="frame indices"):
        insp.overlay(img_d, [0, 3], *params)


def _rast(insp, params, f):
    from instantavatar_amd.raster import rasterize
    return rasterize(insp._posed(*params)[0][f], insp.faces, insp.camera).face_id


# ---- the driver -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _driver_truth():
    from instantavatar_amd import synthetic
    return _truth(synthetic.make_mesh_body())          # the body `--synthetic-mesh-body` builds


def _sequence(tmp_path, masks=True, keypoints=True, images=True):
    from PIL import Image
    body, kpv, params, kp, m = _driver_truth()
    root = os.path.join(os.fspath(tmp_path), "seq")
    os.makedirs(root)
    np.savez(os.path.join(root, "cameras.npz"), intrinsic=K0, extrinsic=np.eye(4), height=H0, width=W0)
    pose, transl = _np(params[1]), _np(params[2])
    np.savez(os.path.join(root, "poses.npz"), betas=np.zeros(10, np.float32), thetas=pose, transl=transl)
    moved_pose, moved_transl = pose.copy(), transl.copy()
    moved_pose[1, 3 * 16 + 2] += 0.9
    moved_transl[1, 0] += 0.25
    np.savez(os.path.join(root, "poses_moved.npz"), betas=np.zeros(10, np.float32), thetas=moved_pose, transl=moved_transl)
    frames = np.random.default_rng(1).integers(0, 40, (3, H0, W0, 3)).astype(np.uint8)
    if keypoints:
        np.save(os.path.join(root, "keypoints.npy"), _np(kp).astype(np.float64))
    for d, on in (("masks", masks), ("images", images)):
        if on:
            os.makedirs(os.path.join(root, d))
    for f in range(3):
        if masks:
            Image.fromarray(_np(m[f]).astype(np.uint8) * 255).save(os.path.join(root, "masks", "f%02d.png" % f))
        if images:
            Image.fromarray(frames[f]).save(os.path.join(root, "images", "f%02d.png" % f))
    return root, frames


def _csv(path):
    with open(path, newline="") as f:
        rows = list(csv.reader(f))
    return rows[0], rows[1:]


def test_driver_end_to_end(tmp_path, capsys):
    from PIL import Image
    from instantavatar_amd import overlay
    from instantavatar_amd.drivers import inspect_sequence as drv
    body, kpv, params, kp, m = _driver_truth()
    root, frames = _sequence(tmp_path)
    moved = os.path.join(root, "poses_moved.npz")
    assert drv.main(["--data", root, "--synthetic-mesh-body", "--poses", moved, "--worst", "1", "--every", "2"]) == 0
    said = capsys.readouterr().out
    head, rows = _csv(os.path.join(root, "inspect", "report.csv"))
    assert head == ["name", "inter", "union", "mask_area", "sil_area", "iou", "n_confident", "kp_err_px"] and [r[0] for r in rows] == ["f00", "f01", "f02"]
    iou, err = [float(r[5]) for r in rows], [float(r[7]) for r in rows]
    assert iou[0] == iou[2] == 1.0 and iou[1] < 1 and err[0] == err[2] == 0 and err[1] > 0 and rows[0][1] == rows[0][2] == rows[0][3] == rows[0][4]
    assert "inspected 3 frames 48x48" in said and "worst frames by IoU: f01" in said and "median 1.0000, minimum" in said and "(f01)" in said
    # the worst frame and every second: f01, then f00 and f02
    assert sorted(os.listdir(os.path.join(root, "inspect"))) == ["overlay_f00.png", "overlay_f01.png", "overlay_f02.png", "report.csv"]
    z = np.load(moved)
    moved_params = (params[0], _dev(z["thetas"]), _dev(z["transl"]))
    insp = overlay.SequenceInspector(body, K0, np.eye(4), H0, W0, keypoints=kp, masks=m, kp_vertex=kpv)
    region = np.logical_or.reduce(_regions(insp, moved_params, [0, 1, 2]))
    direct = _np(insp.overlay(_dev(frames), [0, 1, 2], *moved_params))
    for f in range(3):
        with Image.open(os.path.join(root, "inspect", "overlay_f%02d.png" % f)) as im:
            assert im.mode == "RGB" and im.size == (W0, H0)
            pic = np.asarray(im)
        assert np.array_equal(pic[~region[f]], frames[f][~region[f]]), f
        assert (pic[region[f]] != frames[f][region[f]]).any(-1).all(), f
        assert np.array_equal(pic, direct[f]), "the file holds what SequenceInspector.overlay gives"
    # --compare: the same columns again; the default pose file is poses.npz here, and the moved one is worse in frame 1 only
    out2 = os.path.join(os.fspath(tmp_path), "second")
    assert drv.main(["--data", root, "--synthetic-mesh-body", "--compare", moved, "--worst", "0", "--out", out2]) == 0
    said = capsys.readouterr().out
    head, rows = _csv(os.path.join(out2, "report.csv"))
    assert head[8:] == [c + "_compare" for c in head[1:8]] and len(rows) == 3 and os.listdir(out2) == ["report.csv"]
    assert float(rows[1][5]) == 1.0 and float(rows[1][12]) == iou[1] and float(rows[1][14]) == err[1]
    assert "IoU better in 0 of 3 frames" in said and "keypoint error better in 0 of 3 frames" in said
    assert drv.main(["--data", root, "--synthetic-mesh-body", "--poses", moved, "--compare", os.path.join(root, "poses.npz"), "--worst", "0", "--out", out2]) == 0
    said = capsys.readouterr().out
    assert "IoU better in 1 of 3 frames" in said and "keypoint error better in 1 of 3 frames" in said


def test_driver_without_masks_without_keypoints_and_its_errors(tmp_path, capsys):
    from PIL import Image
    from instantavatar_amd.drivers import inspect_sequence as drv
    root, frames = _sequence(tmp_path / "a", masks=False, images=False)
    moved = os.path.join(root, "poses_moved.npz")
    assert drv.main(["--data", root, "--synthetic-mesh-body", "--poses", moved, "--worst", "1"]) == 0
    said = capsys.readouterr().out
    head, rows = _csv(os.path.join(root, "inspect", "report.csv"))
    assert head == ["name", "n_confident", "kp_err_px"] and [r[0] for r in rows] == ["000000", "000001", "000002"]
    assert "worst frames by keypoint error: 000001" in said and "IoU" not in said
    with Image.open(os.path.join(root, "inspect", "overlay_000001.png")) as im:          # no images: a grey canvas of cameras.npz's size
        pic = np.asarray(im)
    assert pic.shape == (H0, W0, 3) and (pic == 64).all(-1).sum() > H0 * W0 // 2 and (pic != 64).any()
    root, frames = _sequence(tmp_path / "b", keypoints=False)
    assert drv.main(["--data", root, "--synthetic-mesh-body", "--worst", "0"]) == 0
    head, rows = _csv(os.path.join(root, "inspect", "report.csv"))
    assert head == ["name", "inter", "union", "mask_area", "sil_area", "iou"] and all(float(r[5]) == 1.0 for r in rows)
    assert "keypoint error" not in capsys.readouterr().out
    # the error paths name their files
    os.remove(os.path.join(root, "images", "f02.png"))
    with pytest.raises(SystemExit, match=r"images: 2 images but 3 rows of poses in .*poses\.npz"):
        drv.main(["--data", root, "--synthetic-mesh-body"])
    Image.fromarray(np.zeros((H0, W0 + 2, 3), np.uint8)).save(os.path.join(root, "images", "f02.png"))
    with pytest.raises(SystemExit, match=r"f02\.png: is 50 x 48, the frames are 48 x 48"):
        drv.main(["--data", root, "--synthetic-mesh-body", "--worst", "3"])
    os.remove(os.path.join(root, "masks", "f01.png"))
    with pytest.raises(SystemExit, match=r"masks: 2 masks but 3 rows of poses in .*poses\.npz"):
        drv.main(["--data", root, "--synthetic-mesh-body"])
    for f in ("f00.png", "f02.png"):
        os.remove(os.path.join(root, "masks", f))
    os.rmdir(os.path.join(root, "masks"))
    with pytest.raises(SystemExit, match=r"neither .*keypoints\.npy nor .*masks"):
        drv.main(["--data", root, "--synthetic-mesh-body"])
