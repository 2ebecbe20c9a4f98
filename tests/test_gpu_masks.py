"""The mask cleaner on the GPU (csrc/ia_masks.hip through instantavatar_amd/masks.py and the C ABI) against the numpy reference of
tests/mask_refs.py, which tests/test_cpu_mask_refs.py checks on the CPU.  Everything is integer, so every comparison is for equality:
masks, binary (the morphology stage alone), labels (the labelling stage alone), area and n_components.  The shapes are the smallest
at which the kernels can go wrong: widths around the 64-bit word, one and two rows, runs that cross words, boxes larger than the image,
long union chains.  Then refusals, ia_mask_apply, and the driver on a small directory."""
import functools
import os

import numpy as np
import pytest
import torch

import mask_refs as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("masks", "binary", "labels", "area", "n_components")


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _run(src, **kw):
    """src [n,H,W] uint8 (numpy) -> the five outputs as numpy arrays"""
    from instantavatar_amd.masks import clean_masks
    r = clean_masks(_dev(src), return_stages=True, **kw)
    torch.cuda.synchronize()
    return {k: getattr(r, k).cpu().numpy() for k in KEYS}


def _same(got, want, what):
    for k in KEYS:          # binary first would name the stage; all five are asserted
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = np.argwhere(got[k] != want[k])
        assert len(bad) == 0, "%s: %s differs at %d places, first at %s: %s, reference %s" % (
            what, k, len(bad), tuple(bad[0]), got[k][tuple(bad[0])], want[k][tuple(bad[0])])


def _check(src, what, k=5, connectivity=8, thr=0):
    src = np.asarray(src, np.uint8)
    src = src[None] if src.ndim == 2 else src
    got = _run(src, threshold=thr, kernel_size=k, connectivity=connectivity)
    _same(got, mr.clean_batch(src, thr, k, connectivity), "%s (k %d, connectivity %d)" % (what, k, connectivity))
    return got


# ---- widths around the word size, kernel sizes, both connectivities ----------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 5, 63, 64, 65, 130])
def test_widths_around_the_word_size(W):
    for H in (1, 2, 37):
        for k in (1, 3, 5, 7):
            for c in (8, 4):
                _check(mr.random_mask(H, W, 1000 * H + 10 * W + k), "random %d x %d" % (H, W), k=k, connectivity=c, thr=0 if k != 3 else 100)


def test_a_box_larger_than_the_image():
    for seed in range(3):
        _check(mr.random_mask(5, 7, seed), "random 5 x 7", k=31)
    _check(np.full((5, 7), 255, np.uint8), "full 5 x 7", k=31)
    one_off = np.full((5, 7), 255, np.uint8)
    one_off[2, 3] = 0
    got = _check(one_off, "5 x 7 with one hole", k=31)
    assert got["area"][0] == 0          # the erosion sees the hole from every pixel


def test_dense_noise_without_morphology():
    """every second run is one or two pixels long: the most runs per word the labelling sees"""
    g = np.random.default_rng(5)
    for c in (8, 4):
        _check(np.where(g.random((3, 40, 200)) < 0.55, 255, 0), "dense noise", k=1, connectivity=c)


# ---- a batch -----------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_three_frames_in_any_order():
    frames = np.stack([mr.random_mask(37, 130, 1), mr.serpentine(37, 130), mr.random_mask(37, 130, 2, cell=9)])
    got = _check(frames, "batch")
    for order in ([2, 0, 1], [1, 2, 0]):
        again = _run(frames[order], kernel_size=5, connectivity=8)
        for k in KEYS:
            assert np.array_equal(again[k], got[k][order]), (order, k)
    alone = _run(frames[1:2], kernel_size=5, connectivity=8)
    for k in KEYS:
        assert np.array_equal(alone[k], got[k][1:2]), k
    # [H,W] in, [H,W] out
    from instantavatar_amd.masks import clean_masks
    r = clean_masks(_dev(frames[0]))
    assert r.masks.shape == (37, 130) and r.area.dim() == 0 and r.binary is None and r.labels is None
    assert np.array_equal(r.masks.cpu().numpy(), got["masks"][0]) and int(r.area) == got["area"][0]


# ---- long union chains ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [8, 4])
def test_long_chains(connectivity):
    for name, a in (("serpentine", mr.serpentine(33, 67)), ("spiral", mr.spiral(65))):
        got = _check(a, name, k=1, connectivity=connectivity)
        assert got["n_components"][0] == 1 and got["area"][0] == int((a > 0).sum())
        assert np.array_equal(got["labels"][0], (a > 0).astype(np.int32)), name + ": labels are the first pixel's, 1"
        assert np.array_equal(got["masks"][0], a)
    # the same corridors entered from the far end: the first pixel is no longer where the chain starts
    for name, a in (("serpentine", mr.serpentine(33, 67)[::-1, ::-1]), ("spiral", mr.spiral(65)[::-1, ::-1])):
        got = _check(a, name + " reversed", k=1, connectivity=connectivity)
        assert got["n_components"][0] == 1


def test_checkerboard():
    a = mr.checkerboard(12, 70)
    g8 = _check(a, "checkerboard", k=1, connectivity=8)
    g4 = _check(a, "checkerboard", k=1, connectivity=4)
    assert g8["n_components"][0] == 1 and g8["area"][0] == 12 * 70 // 2
    assert g4["n_components"][0] == 12 * 70 // 2 and g4["area"][0] == 1 and g4["masks"][0].sum() == 255 and g4["masks"][0, 0, 0] == 255


def test_the_tie_goes_to_the_earlier_component():
    a = np.zeros((20, 140), np.uint8)
    a[12:16, 2:8] = 255          # starts later in row-major order ...
    a[3:7, 126:132] = 255        # ... than this one, which lies to its right: equal areas
    a[8:11, 61:67] = 255         # and a smaller one that crosses a word boundary
    for k in (1, 3):
        got = _check(a, "tie", k=k)
        assert got["n_components"][0] == 3 and got["area"][0] == 24
        want = np.zeros_like(a)
        want[3:7, 126:132] = 255
        assert np.array_equal(got["masks"][0], want)


def test_empty_full_and_border_frames():
    H, W = 9, 130
    ring = np.zeros((H, W), np.uint8)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = 255, 255, 255, 255
    frames = np.stack([np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), ring])
    got = _check(frames, "zero / full / ring", k=1)
    assert got["area"].tolist() == [0, H * W, 2 * W + 2 * H - 4] and got["n_components"].tolist() == [0, 1, 1]
    assert not got["masks"][0].any() and (got["masks"][1] == 255).all() and np.array_equal(got["masks"][2], ring)
    got = _check(frames, "zero / full / ring", k=5)
    assert got["area"].tolist() == [0, H * W, 0]
    cross = np.zeros((37, 65), np.uint8)         # touches all four borders, thick enough for the 5 x 5 box
    cross[15:22], cross[:, 30:37] = 255, 255
    got = _check(cross, "cross", k=5)
    assert got["n_components"][0] == 1 and np.array_equal(got["masks"][0], cross)


# ---- a realistic frame -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _realistic():
    sil = mr.body_silhouette(270, 480, DEV)
    raw, speck = mr.degrade(sil, 11)
    return sil, raw, speck, mr.clean(raw)


def test_a_realistic_frame():
    sil, raw, speck, want = _realistic()
    assert sil.sum() > 3000 and speck.sum() > 100
    got = _run(raw[None])
    _same(got, {k: np.asarray(v)[None].astype(got[k].dtype) for k, v in want.items()}, "body 270 x 480")
    m = got["masks"][0] != 0
    assert not (m & speck).any() and not m[:14, :14].any(), "speckles or the detached blob in the cleaned mask"
    assert got["n_components"][0] >= 2 and (m & sil).sum() > 0.5 * sil.sum()


def test_two_calls_give_the_same_bytes():
    _, raw, _, _ = _realistic()
    frames = np.stack([raw, mr.random_mask(270, 480, 3), raw[::-1].copy()])
    a, b = _run(frames), _run(frames)
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["area"][0] == a["area"][2] and a["n_components"][0] == a["n_components"][2]       # (a flip keeps the components' sizes)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_carry_a_message():
    from instantavatar_amd import _lib
    from instantavatar_amd.masks import apply_masks, clean_masks
    src = _dev(mr.random_mask(8, 9, 0))
    with pytest.raises(_lib.IAError, match="no CPU path"):
        clean_masks(src.cpu())
    with pytest.raises(_lib.IAError, match="no CPU path"):
        apply_masks(torch.zeros((2, 2, 3), dtype=torch.uint8), torch.zeros((2, 2), dtype=torch.uint8))
    with pytest.raises(_lib.IAError, match=r"kernel_size 4.*odd"):
        clean_masks(src, kernel_size=4)
    with pytest.raises(_lib.IAError, match=r"kernel_size 33"):
        clean_masks(src, kernel_size=33)
    with pytest.raises(_lib.IAError, match=r"connectivity 6"):
        clean_masks(src, connectivity=6)
    with pytest.raises(_lib.IAError, match=r"threshold 300"):
        clean_masks(src, threshold=300)
    with pytest.raises(_lib.IAError, match=r"uint8"):
        clean_masks(src.float())
    n, H, W = 1, 8, 9
    masks, area, nc = torch.empty_like(src), torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)
    need = int(_lib.call("ia_mask_clean_workspace_bytes", n, H, W))
    assert need > 0 and _lib.call("ia_mask_clean_workspace_bytes", 0, H, W) == 0 and _lib.call("ia_mask_clean_workspace_bytes", 1, 1 << 20, 1 << 20) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.IAError, match=r"stream = NULL"):
        _lib.call("ia_mask_clean", src, n, H, W, 0, 5, 8, masks, None, None, area, nc, ws, need, None)
    with pytest.raises(_lib.IAError, match=r"stream = NULL"):
        _lib.call("ia_mask_apply", torch.empty((8, 9, 3), dtype=torch.uint8, device=DEV), masks, n, H, W, torch.empty((8, 9, 3), dtype=torch.uint8, device=DEV), None)
    side = torch.cuda.Stream(DEV)          # the entry points take no NULL stream, which torch's default stream is
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with pytest.raises(_lib.IAError, match=r"workspace of \d+ bytes, \d+ needed"):
            _lib.call("ia_mask_clean", src, n, H, W, 0, 5, 8, masks, None, None, area, nc, ws, need - 1)
        with pytest.raises(_lib.IAError, match=r"overlaps src"):
            _lib.call("ia_mask_clean", src, n, H, W, 0, 5, 8, src, None, None, area, nc, ws, need)
        # the workspace is not written behind its stated size, and the outputs not behind their last element
        ws = torch.full((need + 64,), 255, dtype=torch.uint8, device=DEV)
        out = torch.full((H * W + 16,), 7, dtype=torch.uint8, device=DEV)
        _lib.call("ia_mask_clean", src, n, H, W, 0, 3, 8, out, None, None, area, nc, ws, need)
    side.synchronize()
    assert (ws[need:] == 255).all() and (out[H * W:] == 7).all()
    assert np.array_equal(out[:H * W].cpu().numpy().reshape(H, W), mr.clean(src.cpu().numpy(), k=3)["masks"])


# ---- ia_mask_apply ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 5, 7), (3, 37, 130)])
def test_apply_exact_aliased_and_not(shape):
    from instantavatar_amd.masks import apply_masks
    g = np.random.default_rng(sum(shape))
    images = g.integers(1, 256, shape + (3,)).astype(np.uint8)
    masks = np.where(g.random(shape) < 0.5, g.integers(1, 256, shape), 0).astype(np.uint8)
    want = mr.apply(images, masks)
    img_d, m_d = _dev(images), _dev(masks)
    out = apply_masks(img_d, m_d)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(img_d.cpu().numpy(), images)
    assert apply_masks(img_d, m_d, out=img_d) is img_d and np.array_equal(img_d.cpu().numpy(), want)
    # a view at an odd byte offset takes the bytewise route
    flat = torch.zeros(images.size + 1, dtype=torch.uint8, device=DEV)
    odd = flat[1:].view(images.shape)
    odd.copy_(_dev(images))
    assert np.array_equal(apply_masks(odd, m_d, out=odd).cpu().numpy(), want) and flat[0] == 0
    assert np.array_equal(apply_masks(_dev(images[0]), _dev(masks[0])).cpu().numpy(), want[0])


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------
def test_driver_end_to_end(tmp_path, capsys):
    from PIL import Image
    from instantavatar_amd.drivers import clean_masks as drv
    root = os.path.join(os.fspath(tmp_path), "seq")
    os.makedirs(os.path.join(root, "masks_sam"))
    os.makedirs(os.path.join(root, "images"))
    H, W = 40, 70
    raws = [mr.random_mask(H, W, 1, cell=12), np.zeros((H, W), np.uint8), mr.random_mask(H, W, 2, cell=12), mr.random_mask(H, W, 3, cell=12)]
    g = np.random.default_rng(0)
    images = g.integers(1, 256, (4, H, W, 3)).astype(np.uint8)
    for i, raw in enumerate(raws):
        if i == 3:      # a colour mask file goes through "L"
            Image.fromarray(np.stack([raw] * 3, -1)).save(os.path.join(root, "masks_sam", "f%02d.png" % i))
        else:
            Image.fromarray(raw).save(os.path.join(root, "masks_sam", "f%02d.png" % i))
        if i != 2:      # frame 2 has no image: no masked image for it
            Image.fromarray(images[i]).save(os.path.join(root, "images", "f%02d.png" % i))
    assert drv.main(["--data", root, "--chunk", "3"]) == 0
    said = capsys.readouterr().out
    assert "cleaned 4 masks 70x40" in said and "no foreground in 1 frame" in said and "f01" in said.split("no foreground")[1]
    assert sorted(os.listdir(os.path.join(root, "masks"))) == ["f00.png", "f01.png", "f02.png", "f03.png"]
    assert sorted(os.listdir(os.path.join(root, "masked_images"))) == ["f00.png", "f01.png", "f03.png"]
    for i, raw in enumerate(raws):
        with Image.open(os.path.join(root, "masks", "f%02d.png" % i)) as im:
            assert im.mode == "L" and im.size == (W, H)
            m = np.asarray(im)
        assert set(np.unique(m)) <= {0, 255} and np.array_equal(m, mr.clean(raw)["masks"]), i
        if i != 2:
            with Image.open(os.path.join(root, "masked_images", "f%02d.png" % i)) as im:
                assert im.mode == "RGB" and np.array_equal(np.asarray(im), mr.apply(images[i], m)), i
    before = open(os.path.join(root, "masks", "f00.png"), "rb").read()
    with pytest.raises(SystemExit, match=r"masks: exists already.*--overwrite"):
        drv.main(["--data", root])
    assert drv.main(["--data", root, "--overwrite", "--kernel", "1", "--connectivity", "4"]) == 0
    with Image.open(os.path.join(root, "masks", "f00.png")) as im:
        assert np.array_equal(np.asarray(im), mr.clean(raws[0], k=1, connectivity=4)["masks"])
    assert before != open(os.path.join(root, "masks", "f00.png"), "rb").read() or np.array_equal(mr.clean(raws[0])["masks"], mr.clean(raws[0], k=1, connectivity=4)["masks"])
    # mixed sizes and an unreadable file name their files
    Image.fromarray(np.zeros((H, W + 1), np.uint8)).save(os.path.join(root, "masks_sam", "f04.png"))
    with pytest.raises(SystemExit, match=r"f04\.png: is 71 x 40, the first mask is 70 x 40"):
        drv.main(["--data", root, "--overwrite"])
    with open(os.path.join(root, "masks_sam", "f04.png"), "wb") as f:
        f.write(b"not a png")
    with pytest.raises(SystemExit, match=r"f04\.png: not a readable mask image"):
        drv.main(["--data", root, "--overwrite"])
