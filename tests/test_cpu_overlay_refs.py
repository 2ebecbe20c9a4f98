"""tests/overlay_refs.py, the reference of the sequence-inspection kernels, is itself checked here against small cases whose answers are
written out as literals.  Then the binding table of include/instantavatar_hip_overlay.h, the tables of instantavatar_amd/overlay.py,
drivers/convert_openpose.py on a temporary directory and the refusals of drivers/inspect_sequence.py that need no device.  No GPU."""
import json
import os

import numpy as np
import pytest

import overlay_refs as ov


def _img(rows):
    """rows of '#' / '.' -> uint8 0 / 255"""
    return np.array([[255 if c == "#" else 0 for c in r] for r in rows], np.uint8)


# ---- blend ------------------------------------------------------------------------------------------------------------------------------
def test_blend_3x3_at_opacity_0_128_256():
    img = np.tile(np.array([100, 0, 255], np.uint8), (3, 3, 1))
    lay = np.tile(np.array([200, 255, 0, 0], np.uint8), (3, 3, 1))
    lay[..., 3] = [[255, 255, 255], [0, 0, 0], [1, 254, 128]]
    # by hand: a = (opacity A + 127) // 255, out = (img (256 - a) + layer a + 128) >> 8 per channel
    by_a = {0: (100, 0, 255), 1: (100, 1, 254), 64: (125, 64, 191), 127: (150, 127, 128), 128: (150, 128, 128), 129: (150, 128, 127),
            255: (200, 254, 1), 256: (200, 255, 0)}
    a_of = {0: [[0, 0, 0], [0, 0, 0], [0, 0, 0]], 128: [[128, 128, 128], [0, 0, 0], [1, 127, 64]], 256: [[256, 256, 256], [0, 0, 0], [1, 255, 129]]}
    for opacity, a in a_of.items():
        want = np.array([[by_a[v] for v in row] for row in a], np.uint8)
        assert np.array_equal(ov.blend(img, lay, opacity), want), opacity
    assert np.array_equal(ov.blend(img, lay, 0), img)


# ---- outline ----------------------------------------------------------------------------------------------------------------------------
def test_outline_5x5():
    block = _img([".....", ".###.", ".###.", ".###.", "....."])
    assert np.array_equal(ov.outline_pixels(block, 1), _img([".....", ".###.", ".#.#.", ".###.", "....."]) > 0)
    assert np.array_equal(ov.outline_pixels(block, 2), block > 0)
    full = np.full((5, 5), 255, np.uint8)
    assert not ov.outline_pixels(full, 1).any() and not ov.outline_pixels(full, 8).any(), "the image border is not an edge"
    assert not ov.outline_pixels(np.zeros((5, 5), np.uint8), 3).any()
    corner = full.copy()
    corner[0, 0] = 0
    assert np.array_equal(ov.outline_pixels(corner, 1), _img([".#...", "##...", ".....", ".....", "....."]) > 0)
    assert np.array_equal(ov.outline_pixels(corner, 2), _img([".##..", "###..", "###..", ".....", "....."]) > 0)
    images = np.full((1, 5, 5, 3), 9, np.uint8)
    out = ov.outline(images, corner[None], 1, (1, 2, 3))
    assert out[0, 0, 1].tolist() == [1, 2, 3] and out[0, 0, 0].tolist() == [9, 9, 9] and (out[0, 2:] == 9).all() and (images == 9).all()


# ---- skeleton -----------------------------------------------------------------------------------------------------------------------------
def _drawn(points, segments, hw, rad=0, thr=0.5, size=9, colours=None, point_rgb=(255, 0, 0)):
    """a black size x size frame with the skeleton drawn in.  Discs cannot be switched off -- at radius 0 a point that sits on a pixel
    centre still paints that pixel -- so by default they are drawn in the segments' red and `_painted` is the union of both"""
    img = np.zeros((size, size, 3), np.uint8)
    colours = colours if colours is not None else [(255, 0, 0)] * len(segments)
    return ov.skeleton_frame(img, np.asarray(points, np.float32), segments, colours, point_rgb, thr, hw, rad)


def _painted(out):
    return {(int(x), int(y)) for y, x in zip(*np.nonzero(out.any(-1)))}


def test_segments_on_9x9():
    # horizontal, (2,4) - (6,4): half a pixel wide it is the row itself, one pixel wide rows 3 .. 5 and the two cap pixels
    pts = [[2, 4, 1], [6, 4, 1]]
    assert _painted(_drawn(pts, [(0, 1)], 2)) == {(x, 4) for x in range(2, 7)}
    assert _painted(_drawn(pts, [(0, 1)], 4)) == {(x, y) for x in range(2, 7) for y in (3, 4, 5)} | {(1, 4), (7, 4)}
    # diagonal, (1,1) - (5,5): the neighbours (k, k +- 1) are 1 / sqrt 2 = 0.707 px away: outside at 0.5 px, inside at 0.75 px where
    # their foot lies within the segment (x + y from 3 to 9)
    pts = [[1, 1, 1], [5, 5, 1]]
    diag = {(k, k) for k in range(1, 6)}
    assert _painted(_drawn(pts, [(0, 1)], 2)) == diag
    assert _painted(_drawn(pts, [(0, 1)], 3)) == diag | {(1, 2), (2, 1), (2, 3), (3, 2), (3, 4), (4, 3), (4, 5), (5, 4)}
    # zero length at (4,4), one pixel wide: the plus
    assert _painted(_drawn([[4, 4, 1], [4, 4, 1]], [(0, 1)], 4)) == {(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)}
    assert _painted(_drawn([[4, 4, 1]], [(0, 0)], 4)) == {(4, 4), (3, 4), (5, 4), (4, 3), (4, 5)}


def test_a_tie_at_an_eighth_of_a_pixel():
    """x = 4.125 quantises to 4 * 4.125 + 0.5 = 17 -> 17 quarter pixels: pixel 5 (centre 20) is then exactly 3 away and inside at hw = 3
    (<=), pixel 3 (centre 12) is 5 away.  x = 4.124 quantises to 16: only pixel 4."""
    assert ov.quantise(4.125) == 17 and ov.quantise(4.124) == 16 and ov.quantise(-0.125) == 0 and ov.quantise(-0.126) == -1
    assert _painted(_drawn([[4.125, 4, 1]], [(0, 0)], 3)) == {(4, 4), (5, 4)}
    assert _painted(_drawn([[4.124, 4, 1]], [(0, 0)], 3)) == {(4, 4)}


def test_validity_and_the_order_rule():
    pts = [[2, 4, 1], [6, 4, 1], [4, 1, 1], [4, 7, 1]]
    assert not ov.point_valid([1, 1, 0.5], 0.5) and ov.point_valid([1, 1, 0.500001], 0.5), "equal to the threshold is not drawn"
    assert not ov.point_valid([np.nan, 1, 1], 0) and not ov.point_valid([1, np.inf, 1], 0) and not ov.point_valid([1, 1, np.inf], 0)
    assert ov.point_valid([32768, -32768, 1], 0) and not ov.point_valid([32768.01, 0, 1], 0)
    # one end at the threshold, then indices outside [0, K): only the radius-0 discs of the valid points (colour 1) are drawn
    assert _painted(_drawn([[2, 4, 1], [6, 4, 0.5]], [(0, 1)], 2, thr=0.5, point_rgb=(1, 1, 1))) == {(2, 4)}
    assert _painted(_drawn(pts, [(0, 4), (-1, 1)], 2, point_rgb=(1, 1, 1))) == {(2, 4), (6, 4), (4, 1), (4, 7)}
    out = _drawn(pts, [(0, 1), (2, 3)], 2, colours=[(255, 0, 0), (0, 255, 0)])
    assert out[4, 4].tolist() == [0, 255, 0] and out[4, 3].tolist() == [255, 0, 0] and out[3, 4].tolist() == [0, 255, 0]
    out = _drawn(pts, [(2, 3), (0, 1)], 2, colours=[(0, 255, 0), (255, 0, 0)])
    assert out[4, 4].tolist() == [255, 0, 0], "the higher index lies on top"
    out = _drawn(pts, [(0, 1)], 2, rad=4, point_rgb=(0, 0, 255))                                  # discs (blue) over segments
    assert out[4, 2].tolist() == [0, 0, 255] and out[4, 3].tolist() == [0, 0, 255] and out[4, 4].tolist() == [255, 0, 0]
    assert out[1, 4].tolist() == [0, 0, 255] and out[0, 4].tolist() == [0, 0, 255] and out[0, 3].tolist() == [0, 0, 0]


def test_the_cross_product_is_squared_exactly():
    """ends at +-32768.  The line y = x through a 64 x 64 image, half a pixel wide, is the diagonal only.  The line from (-32768, 0) to
    (0, 32768) passes 23 170 pixels from the image while its bounding box touches column 0: there the cross product is 2^34 and its
    square 2^68 -- truncated to 64 bits it would be 0 and the pixel inside."""
    lo, hi = ov.quantise(-32768.0), ov.quantise(32768.0)
    assert (lo, hi) == (-131072, 131072)
    assert np.array_equal(ov.segment_pixels(64, 64, (lo, lo), (hi, hi), 2), np.eye(64, dtype=bool))
    a, b = (lo, 0), (0, hi)
    c = (b[0] - a[0]) * (0 - a[1]) - (b[1] - a[1]) * (0 - a[0])
    assert abs(c) == 2 ** 34 and (c * c) % 2 ** 64 == 0
    assert not ov.segment_pixels(64, 64, a, b, 64).any()


# ---- stats and shade --------------------------------------------------------------------------------------------------------------------
def test_stats_and_shade_literals():
    a = _img(["##..", "##.."])[None]
    b = _img([".##.", "...."])[None]
    b[0, 0, 1] = 1                                     # any non-zero byte counts
    assert ov.stats(a, b).tolist() == [[1, 5, 4, 2]]
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 0, 1], [0, 1, 9]])
    fid = np.array([[0, 1, 2], [3, 4, -1]], np.int32)
    lay = ov.face_shade_bytes(fid, verts, faces, np.eye(4), (100, 200, 40))
    assert lay[0, 0].tolist() == [100, 200, 40, 255]                # facing the camera: s = 1
    assert lay[0, 1].tolist() == [25, 50, 10, 255]                  # edge on: s = 0.25
    assert lay[0, 2].tolist() == [25, 50, 10, 255]                  # degenerate: s = 0.25
    assert not lay[1].any(), "a vertex index or a face id out of range, and an empty pixel, give zeros"


# ---- the binding and the tables ---------------------------------------------------------------------------------------------------------
def test_overlay_header_is_declared_and_built():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    names = ["ia_overlay_blend", "ia_overlay_face_shade", "ia_overlay_outline", "ia_overlay_skeleton", "ia_overlay_stats",
             "ia_overlay_stats_workspace_bytes"]
    assert sorted(_lib.declarations("overlay")) == names
    assert os.path.normpath(_lib.header_path("overlay")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_overlay.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_overlay.hip"))
    for name in names:
        d = _lib.declarations("overlay")[name]
        assert d.stream == (name != "ia_overlay_stats_workspace_bytes"), name
    d = _lib.declarations("overlay")["ia_overlay_skeleton"]
    assert [p.name for p in d.params][:3] == ["points", "n", "K"] and d.params[9].name == "threshold" and d.params[9].kind == "scalar"


def test_body25_tables():
    from instantavatar_amd import overlay
    seg = overlay.BODY25_SEGMENTS
    assert len(seg) == 24 and len(set(map(frozenset, seg))) == 24 and all(0 <= i < 25 and 0 <= j < 25 and i != j for i, j in seg)
    assert {i for s in seg for i in s} == set(range(25)), "every BODY_25 point has a limb"
    # a tree rooted at the neck: 24 edges over 25 connected points
    seen, todo = {1}, [1]
    while todo:
        k = todo.pop()
        for i, j in seg:
            for u, v in ((i, j), (j, i)):
                if u == k and v not in seen:
                    seen.add(v)
                    todo.append(v)
    assert len(seen) == 25
    col = overlay.LIMB_COLOURS
    assert len(col) == 24 and len(set(col)) == 24 and all(len(c) == 3 and all(0 <= v <= 255 for v in c) and max(c) == 255 for c in col)
    assert overlay.MODEL_POINT_COLOUR not in col


# ---- convert_openpose -------------------------------------------------------------------------------------------------------------------
def test_convert_openpose(tmp_path, capsys):
    from instantavatar_amd.drivers import convert_openpose as drv
    jdir = tmp_path / "seq" / "openpose"
    jdir.mkdir(parents=True)
    rs = np.random.RandomState(0)
    rows = rs.rand(3, 75) * 100
    for i, name in enumerate(["b_000002", "a_000001", "c_000003"]):          # written out of order: the files are read sorted
        people = [] if i == 2 else [{"pose_keypoints_2d": rows[i].tolist()}, {"pose_keypoints_2d": [0.0] * 75}]
        (jdir / (name + "_keypoints.json")).write_text(json.dumps({"version": 1.3, "people": people}))
    (jdir / "notes.txt").write_text("not json")
    assert drv.main(["--json-dir", os.fspath(jdir)]) == 0
    said = capsys.readouterr().out
    kp = np.load(tmp_path / "seq" / "keypoints.npy")
    assert kp.shape == (3, 25, 3) and kp.dtype == np.float64
    assert np.array_equal(kp[0], rows[1].reshape(25, 3)) and np.array_equal(kp[1], rows[0].reshape(25, 3)) and not kp[2].any()
    assert "no person in 1 frame" in said and "c_000003_keypoints.json" in said.split("no person")[1]
    assert drv.main(["--json_dir", os.fspath(jdir), "--output_file", "other.npy"]) == 0 and (tmp_path / "seq" / "other.npy").exists()
    (jdir / "d_000004_keypoints.json").write_text(json.dumps({"people": [{"pose_keypoints_2d": [1.0] * 54}]}))
    with pytest.raises(SystemExit, match=r"d_000004_keypoints\.json: pose_keypoints_2d holds 54 numbers"):
        drv.main(["--json-dir", os.fspath(jdir)])
    (jdir / "d_000004_keypoints.json").write_text("{")
    with pytest.raises(SystemExit, match=r"d_000004_keypoints\.json: not an OpenPose JSON file"):
        drv.main(["--json-dir", os.fspath(jdir)])
    with pytest.raises(SystemExit, match=r"nowhere: is missing"):
        drv.main(["--json-dir", os.fspath(tmp_path / "nowhere")])
    (tmp_path / "empty").mkdir()
    with pytest.raises(SystemExit, match=r"holds no \*\.json files"):
        drv.main(["--json-dir", os.fspath(tmp_path / "empty")])


# ---- inspect_sequence: what is refused before a device is touched --------------------------------------------------------------------------
def test_inspect_sequence_refuses_before_it_touches_a_device(tmp_path):
    from instantavatar_amd.drivers import inspect_sequence as drv
    root = tmp_path / "seq"
    root.mkdir()
    with pytest.raises(SystemExit, match=r"cameras\.npz: is missing"):
        drv.main(["--data", os.fspath(root)])
    np.savez(root / "cameras.npz", intrinsic=np.eye(3), extrinsic=np.eye(4), height=8, width=8)
    with pytest.raises(SystemExit, match=r"poses\.npz: is missing"):
        drv.main(["--data", os.fspath(root)])
    np.savez(root / "poses.npz", betas=np.zeros(10), thetas=np.zeros((3, 72)), transl=np.zeros((3, 3)))
    with pytest.raises(SystemExit, match=r"neither .*keypoints\.npy nor .*masks: nothing to measure"):
        drv.main(["--data", os.fspath(root)])
    np.save(root / "keypoints.npy", np.zeros((2, 25, 3)))
    with pytest.raises(SystemExit, match=r"keypoints\.npy: 2 rows of keypoints but 3 rows of poses in .*poses\.npz"):
        drv.main(["--data", os.fspath(root)])
    np.save(root / "keypoints.npy", np.zeros((3, 25, 3)))
    (root / "masks").mkdir()
    with pytest.raises(SystemExit, match=r"masks: 0 masks but 3 rows of poses in .*poses\.npz"):
        drv.main(["--data", os.fspath(root)])
    (root / "masks").rmdir()
    np.savez(root / "poses_optimized.npz", betas=np.zeros(10), thetas=np.zeros((4, 72)), transl=np.zeros((4, 3)))
    with pytest.raises(SystemExit, match=r"keypoints\.npy: 3 rows of keypoints but 4 rows of poses in .*poses_optimized\.npz"):
        drv.main(["--data", os.fspath(root)])            # the optimised file is the default when it is there
    with pytest.raises(SystemExit, match=r"poses_optimized\.npz: 4 rows of poses but 3 rows of poses in .*poses\.npz"):
        drv.main(["--data", os.fspath(root), "--poses", os.fspath(root / "poses.npz"), "--compare", os.fspath(root / "poses_optimized.npz")])
    inp = drv.check_inputs(root, poses=root / "poses.npz", downscale=2.0)
    assert inp["names"] == ["000000", "000001", "000002"] and inp["K"][0, 0] == 0.5 and inp["K"][2, 2] == 1 and inp["mask_files"] is None
    assert drv.WORKERS == 16
