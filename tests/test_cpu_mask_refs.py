"""tests/mask_refs.py, the numpy reference of the mask cleaner, is itself checked here: against scipy.ndimage on seeded masks, and
against small cases whose answers are written out as literals.  Then the binding table of include/instantavatar_hip_masks.h and the
refusals of drivers/clean_masks.py that need no device.  No GPU."""
import os

import numpy as np
import pytest

import mask_refs as mr


def _img(rows):
    """rows of '#' / '.' -> uint8 0 / 255"""
    return np.array([[255 if c == "#" else 0 for c in r] for r in rows], np.uint8)


# ---- against scipy.ndimage ------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (1, 9), (7, 1), (5, 7), (12, 65), (33, 40)]


@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_box_morphology_equals_ndimage(k):
    ndi = pytest.importorskip("scipy.ndimage")
    box = np.ones((k, k), bool)
    for i, (H, W) in enumerate(SIZES):
        fg = mr.threshold(mr.random_mask(H, W, 10 * k + i))
        assert np.array_equal(mr.erode(fg, k), ndi.binary_erosion(fg, box, border_value=1)), (H, W)
        assert np.array_equal(mr.dilate(fg, k), ndi.binary_dilation(fg, box, border_value=0)), (H, W)
        want = ndi.binary_erosion(ndi.binary_dilation(ndi.binary_dilation(ndi.binary_erosion(fg, box, border_value=1), box), box), box, border_value=1)
        assert np.array_equal(mr.open_close(fg, k), want), (H, W)


@pytest.mark.parametrize("connectivity", [8, 4])
def test_labels_equal_ndimage_partition_with_first_pixel_numbering(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = np.ones((3, 3), bool) if connectivity == 8 else ndi.generate_binary_structure(2, 1)
    cases = [mr.threshold(mr.random_mask(H, W, 100 + i, flip=0.15)) for i, (H, W) in enumerate(SIZES)]
    cases += [mr.open_close(mr.threshold(mr.random_mask(40, 70, 7)), 5), mr.serpentine(9, 12) > 0, mr.spiral(13) > 0, mr.checkerboard(6, 7) > 0]
    for fg in cases:
        H, W = fg.shape
        lab, n = ndi.label(fg, structure)
        index = np.arange(1, H * W + 1).reshape(H, W)
        want = np.zeros((H, W), np.int32)
        if n:
            first = ndi.minimum(index, lab, np.arange(1, n + 1))            # per scipy label: 1 + index of its first pixel
            want = np.where(lab > 0, np.asarray(first)[np.maximum(lab, 1) - 1], 0).astype(np.int32)
        got = mr.label(fg, connectivity)
        assert np.array_equal(got, want), (H, W)
        m, area, nc = mr.largest(got)
        assert nc == n
        if n:
            sizes = ndi.sum(fg, lab, np.arange(1, n + 1))
            best = min((l for l in range(1, n + 1) if sizes[l - 1] == sizes.max()), key=lambda l: first[l - 1])
            assert area == int(sizes.max()) and np.array_equal(m, np.where(lab == best, 255, 0))


# ---- written out by hand --------------------------------------------------------------------------------------------------------------
def test_diagonal_touch_is_one_component_at_8_and_two_at_4():
    a = _img([".........",
              ".###.....",
              ".###.....",
              ".###.....",
              "....##...",
              "....##...",
              "........."])
    assert a.shape == (7, 9)
    l8 = mr.label(a > 0, 8)
    l4 = mr.label(a > 0, 4)
    first, second = 1 + 1 * 9 + 1, 1 + 4 * 9 + 4
    want8 = np.where(a > 0, first, 0)
    want4 = want8.copy()
    want4[4:6, 4:6] = second
    assert np.array_equal(l8, want8) and np.array_equal(l4, want4)
    assert mr.largest(l8)[1:] == (13, 1) and mr.largest(l4)[1:] == (9, 2)
    r = mr.clean(a, k=1, connectivity=4)
    assert np.array_equal(r["masks"], np.where(want4 == first, 255, 0)) and r["area"] == 9 and r["n_components"] == 2


def test_open_removes_a_speck_and_close_fills_a_hole():
    a = np.zeros((12, 14), np.uint8)
    a[2:10, 3:12] = 9                     # any value above the threshold
    clean = np.where(a > 0, 255, 0).astype(np.uint8)
    speck = a.copy()
    speck[0, 0] = 255
    assert np.array_equal(mr.clean(speck, k=3)["binary"], clean) and mr.clean(speck, k=1)["n_components"] == 2
    hole = a.copy()
    hole[5, 6] = 0
    assert np.array_equal(mr.clean(hole, k=3)["binary"], clean) and np.array_equal(mr.clean(hole, k=3)["masks"], clean)
    assert mr.clean(hole, k=1)["binary"][5, 6] == 0 and mr.clean(hole, k=3)["area"] == 72
    # a threshold: 9 > 8 but not > 9
    assert mr.clean(a, thr=8, k=1)["area"] == 72 and mr.clean(a, thr=9, k=1)["area"] == 0


def test_a_blob_on_the_border_survives_erosion():
    a = _img(["##....",
              "##....",
              "......",
              "......",
              "......"])
    # outside counts as foreground: the corner pixel's 3 x 3 box holds 4 image pixels, all set
    assert np.array_equal(mr.erode(a > 0, 3), _img(["#.....", "......", "......", "......", "......"]) > 0)
    assert np.array_equal(mr.open_close(a > 0, 3), a > 0)
    # ... and away from the border the same blob goes
    b = np.zeros((6, 7), np.uint8)
    b[2:4, 2:4] = 255
    assert not mr.erode(b > 0, 3).any() and mr.clean(b, k=3)["area"] == 0 and mr.clean(b, k=3)["n_components"] == 0
    # dilation does not bring anything in from outside
    assert np.array_equal(mr.dilate(np.zeros((3, 4), bool), 31), np.zeros((3, 4), bool))
    assert mr.erode(np.ones((3, 4), bool), 31).all()


def test_of_two_equal_blobs_the_earlier_one_wins():
    a = _img(["......##",
              "......##",
              "........",
              "##......",
              "##......"])
    r = mr.clean(a, k=1)
    assert r["n_components"] == 2 and r["area"] == 4
    assert np.array_equal(r["masks"], _img(["......##", "......##", "........", "........", "........"]))
    assert sorted(np.unique(r["labels"])) == [0, 7, 25]
    e = mr.clean(np.zeros((4, 5), np.uint8))
    assert e["area"] == 0 and e["n_components"] == 0 and not e["masks"].any() and not e["labels"].any()


def test_long_chains_are_one_component_labelled_by_their_first_pixel():
    for a in (mr.serpentine(33, 67), mr.spiral(65)):
        for c in (8, 4):
            r = mr.clean(a, k=1, connectivity=c)
            assert r["n_components"] == 1 and r["area"] == int((a > 0).sum()) and set(np.unique(r["labels"])) == {0, 1}
    cb = mr.checkerboard(6, 8)
    assert mr.clean(cb, k=1, connectivity=8)["n_components"] == 1 and mr.clean(cb, k=1, connectivity=4)["n_components"] == 24


def test_apply():
    img = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3) + 1
    m = np.array([[0, 255, 1], [0, 0, 7]], np.uint8)
    out = mr.apply(img, m)
    assert np.array_equal(out[m != 0], img[m != 0]) and not out[m == 0].any()


# ---- the binding table ------------------------------------------------------------------------------------------------------------------
def test_masks_header_is_a_table_of_its_own():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    assert sorted(_lib.declarations("masks")) == ["ia_mask_apply", "ia_mask_clean", "ia_mask_clean_workspace_bytes"]
    assert os.path.normpath(_lib.header_path("masks")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_masks.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_masks.hip"))
    d = _lib.declarations("masks")["ia_mask_clean"]
    assert d.stream and [p.name for p in d.params][-3:] == ["ws", "ws_bytes", "stream"]


# ---- the driver's refusals that need no device --------------------------------------------------------------------------------------------
def _sequence(tmp_path, n=2):
    from PIL import Image
    root = os.path.join(os.fspath(tmp_path), "seq")
    os.makedirs(os.path.join(root, "masks_sam"))
    for i in range(n):
        Image.fromarray(mr.random_mask(8, 9, i)).save(os.path.join(root, "masks_sam", "%04d.png" % i))
    return root


def test_driver_refuses_before_it_touches_a_device(tmp_path):
    from instantavatar_amd.drivers import clean_masks as drv
    root = _sequence(tmp_path)
    assert [os.path.basename(f) for f in drv.check_args(root)] == ["0000.png", "0001.png"]
    with pytest.raises(SystemExit, match=r"--kernel 4.*odd"):
        drv.main(["--data", root, "--kernel", "4"])
    with pytest.raises(SystemExit, match=r"--kernel 33.*\[1, 31\]"):
        drv.main(["--data", root, "--kernel", "33"])
    with pytest.raises(SystemExit, match=r"--connectivity 6"):
        drv.main(["--data", root, "--connectivity", "6"])
    with pytest.raises(SystemExit, match=r"--threshold 256"):
        drv.main(["--data", root, "--threshold", "256"])
    with pytest.raises(SystemExit, match=r"nowhere.*is missing"):
        drv.main(["--data", os.path.join(root, "nowhere")])
    with pytest.raises(SystemExit, match=r"masks_rvm.*is missing"):
        drv.main(["--data", root, "--source", "masks_rvm"])
    with pytest.raises(SystemExit, match=r"masks: --source is the output directory"):
        drv.main(["--data", root, "--source", "masks"])
    os.makedirs(os.path.join(root, "masks"))
    with pytest.raises(SystemExit, match=r"masks: --source is the output directory"):
        drv.main(["--data", root, "--source", "masks", "--overwrite"])
    with pytest.raises(SystemExit, match=r"masks: exists already.*--overwrite"):
        drv.main(["--data", root])
    assert os.listdir(os.path.join(root, "masks")) == [] and not os.path.exists(os.path.join(root, "masked_images"))
    assert len(drv.check_args(root, overwrite=True)) == 2
    os.makedirs(os.path.join(root, "empty"))
    with pytest.raises(SystemExit, match=r"empty: holds no files"):
        drv.main(["--data", root, "--source", "empty", "--overwrite"])


def test_refine_smpl_points_at_the_driver_when_masks_are_missing():
    import inspect
    from instantavatar_amd.drivers import refine_smpl
    assert "instantavatar_amd.drivers.clean_masks" in inspect.getsource(refine_smpl.read_masks)
