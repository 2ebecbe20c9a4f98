"""datasets/sequence_dir.py against the reference's dataset classes executing on the CPU
(tests/golden/sequence_dir_golden.npz, written by tests/golden/make_sequence_dir_golden.py on the directory of
tests/sequence_fixture.py), its refusals, and the second header of the binding.  No GPU."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sequence_fixture as fx  # noqa: E402

from instantavatar_amd.datasets import sequence_dir as sd  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, "golden", "sequence_dir_golden.npz"))


def host_rays(K, c2w, H, W):
    """peoplesnapshot.py:12-25 restated (float32 pixel grid, float64 camera, float32 result)"""
    x, y = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    xy = np.stack([x, y, np.ones_like(x)], axis=-1).reshape(-1, 3).astype(np.float32)
    d = xy @ np.linalg.inv(K).T @ c2w[:3, :3].T
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(c2w[:3, 3], (len(d), 1)).reshape(H, W, 3).astype(np.float32), d.reshape(H, W, 3).astype(np.float32)


@pytest.mark.parametrize("case", fx.CASES, ids=[c[0] for c in fx.CASES])
def test_read_sequence_equals_the_reference(case, tmp_path):
    name, kind, split, opt, cached = case
    fx.write_sequence(tmp_path / "seq", kind, cached=cached)
    seq = sd.read_sequence(tmp_path / "seq", kind, split, opt)
    g = lambda k: GOLDEN[name + "/" + k]
    assert [os.path.basename(f) for f in seq.image_files] == list(g("image_files"))
    assert [os.path.basename(f) for f in seq.mask_files] == list(g("mask_files"))
    assert (seq.H, seq.W) == tuple(g("image_shape")) and (seq.H0, seq.W0) == (fx.H0, fx.W0)
    assert sorted(seq.smpl_params) == ["betas", "body_pose", "global_orient", "transl"]
    for k, v in seq.smpl_params.items():
        ref = g("smpl/" + k)
        assert v.dtype == np.float32 and v.shape == ref.shape and np.array_equal(v, ref), k     # bit-equal
    # camera: the same float64 operations (np.linalg.inv of the same matrix) -- equal to float64 rounding
    np.testing.assert_allclose(seq.K, g("K"), rtol=1e-15, atol=0)
    np.testing.assert_allclose(seq.c2w, g("c2w"), rtol=1e-14, atol=1e-15)
    ro, rd = host_rays(seq.K, seq.c2w, seq.H, seq.W)
    assert np.array_equal(ro, g("rays_o"))
    np.testing.assert_allclose(rd, g("rays_d"), rtol=0, atol=6e-8)      # one float32 ulp below 1 where the float64 values differ in the last bit
    assert seq.near == opt.get("near") and seq.far == opt.get("far") and seq.downscale == 1
    want = {"ps_fallback": "poses.npz", "ps_slice": "poses.npz", "ps_anim": "anim_nerf_train.npz", "ps_split": "train.npz",
            "ps_refine": "anim_nerf_test.npz", "ps_refine_missing": "poses.npz", "ps_val": "poses.npz", "cu_cached": "train.npz",
            "cu_fitting": "poses_optimized.npz", "cu_val": "poses_optimized.npz"}[name]
    assert os.path.basename(seq.pose_file) == want


def test_downscale_two_halves_the_size_and_the_intrinsics(tmp_path):
    fx.write_sequence(tmp_path / "seq", "peoplesnapshot")
    one = sd.read_sequence(tmp_path / "seq", "peoplesnapshot", "train", dict(start=0, end=6, downscale=1))
    two = sd.read_sequence(tmp_path / "seq", "peoplesnapshot", "train", dict(start=0, end=6, downscale=2))
    assert (two.H, two.W, two.H0, two.W0) == (fx.H0 // 2, fx.W0 // 2, fx.H0, fx.W0)
    assert np.array_equal(two.K[:2], one.K[:2] / 2) and np.array_equal(two.K[2], one.K[2]) and np.array_equal(two.c2w, one.c2w)


def _ps(tmp_path, **kw):
    root = tmp_path / "seq"
    fx.write_sequence(root, kw.pop("kind", "peoplesnapshot"), **kw)
    return root


OPT = dict(start=0, end=6, downscale=1)


def test_a_pose_row_mismatch_names_both_counts_and_both_files(tmp_path):
    root = _ps(tmp_path, cached={"anim_nerf_train": 4})
    with pytest.raises(sd.SequenceError) as e:
        sd.read_sequence(root, "peoplesnapshot", "train", OPT)           # 7 frames, a cached file of 4 rows (not sliced)
    msg = str(e.value)
    assert "7 frames" in msg and "4 rows" in msg and "anim_nerf_train.npz" in msg and os.path.join("images", "*.png") in msg


def test_malformed_directories_are_refused_with_the_file_named(tmp_path):
    root = _ps(tmp_path)
    os.rename(root / "cameras.npz", root / "cameras.bak")
    with pytest.raises(sd.SequenceError, match="cameras.npz"):
        sd.read_sequence(root, "peoplesnapshot", "train", OPT)
    os.rename(root / "cameras.bak", root / "cameras.npz")
    # unequal image and mask counts
    os.rename(root / "masks" / "mask_0003.npy", root / "mask_0003.bak")
    with pytest.raises(sd.SequenceError, match=r"7 images .* 6 masks"):
        sd.read_sequence(root, "peoplesnapshot", "train", OPT)
    os.rename(root / "mask_0003.bak", root / "masks" / "mask_0003.npy")
    # an image whose size differs from cameras.npz
    from PIL import Image
    Image.fromarray(np.zeros((fx.H0, fx.W0 + 2, 3), np.uint8), "RGB").save(root / "images" / "image_0002.png")
    with pytest.raises(sd.SequenceError, match=r"image_0002.png is 24 x 22 .*cameras.npz says 24 x 20"):
        sd.read_sequence(root, "peoplesnapshot", "train", OPT)
    # the custom layout's masks are PNGs: a PeopleSnapshot directory read as custom has images but no masks
    with pytest.raises(sd.SequenceError, match=r"7 images .* 0 masks"):
        sd.read_sequence(root, "custom", "train", OPT)
    # no images at all
    for f in (root / "images").glob("*.png"):
        os.remove(f)
    with pytest.raises(sd.SequenceError, match=r"no images"):
        sd.read_sequence(root, "peoplesnapshot", "train", OPT)


def test_missing_pose_files_and_unknown_kinds_are_refused(tmp_path):
    root = _ps(tmp_path)
    os.remove(root / "poses.npz")
    with pytest.raises(sd.SequenceError, match="poses.npz is missing"):
        sd.read_sequence(root, "peoplesnapshot", "train", OPT)
    with pytest.raises(sd.SequenceError, match="unknown dataset kind"):
        sd.read_sequence(root, "surreal", "train", OPT)


def test_unsupported_resizes_are_refused_with_their_reasons(tmp_path):
    assert sd.resize_rule(24, 20, 1) == 1 and sd.resize_rule(24, 20, 2) == 2 and sd.resize_rule(25, 21, 1) == 1 and sd.resize_rule(24, 20, 2.0) == 2
    with pytest.raises(sd.SequenceError, match="downscale 3: only factor 2 is OpenCV's exact 2 x 2 box"):
        sd.resize_rule(24, 20, 3)
    with pytest.raises(sd.SequenceError, match="25 x 20 source: an odd size"):
        sd.resize_rule(25, 20, 2)
    with pytest.raises(sd.SequenceError, match="1.5 is not an integer"):
        sd.resize_rule(24, 20, 1.5)
    # and `from_directory` refuses them before it touches a device
    from instantavatar_amd.datasets.device_frames import DeviceFrames
    root = _ps(tmp_path, height=25, width=20)
    seq = sd.read_sequence(root, "peoplesnapshot", "train", dict(start=0, end=6, downscale=2))
    assert (seq.H, seq.W) == (12, 10)             # the reference's int(height / downscale): described, but not ingested
    with pytest.raises(sd.SequenceError, match="an odd size"):
        DeviceFrames.from_directory(seq, None, "cuda:0")
    seq3 = sd.read_sequence(_ps(tmp_path / "b"), "peoplesnapshot", "train", dict(start=0, end=6, downscale=3))
    with pytest.raises(sd.SequenceError, match="downscale 3"):
        DeviceFrames.from_directory(seq3, None, "cuda:0")


def test_pil_reduce_is_the_same_rounded_box():
    """the claim the GPU test relies on when it pins the uint8 kernel to `Image.reduce(2)` as well: PIL's 2 x 2 reduction equals
    (a + b + c + d + 2) >> 2 -- on every cell sum 0 .. 1020 and on the fixture's kind of frames, grey and 3-channel"""
    from PIL import Image
    cells = np.zeros((2, 2 * 1021), np.uint8)
    for s in range(1021):
        cells[0, 2 * s], cells[0, 2 * s + 1], cells[1, 2 * s], cells[1, 2 * s + 1] = [min(255, max(0, s - 255 * i)) for i in range(4)]
    assert np.array_equal(np.asarray(Image.fromarray(cells, "L").reduce(2)), fx.restate_u8(cells[None], 2)[0])
    rs = np.random.RandomState(3)
    img = rs.randint(0, 256, (1, 26, 34, 3)).astype(np.uint8)
    assert np.array_equal(np.asarray(Image.fromarray(img[0], "RGB").reduce(2)), fx.restate_u8(img, 2)[0])


def test_split_options_reads_a_reference_dataset_config(tmp_path):
    conf = tmp_path / "subject.yaml"
    conf.write_text("subject: s\ngender: male\nopt:\n  dataroot: ./data/${dataset.subject}/\n  train:\n    num_workers: 8\n    start: 0\n    end: 445\n"
                    "    skip: 4\n    downscale: 2\n    sampler: ${sampler}\n    fitting: ${model.opt.optimize_SMPL.enable}\n"
                    "    refine: ${model.opt.optimize_SMPL.is_refine}\n  test:\n    start: 446\n    end: 647\n    skip: 4\n    downscale: 2\n")
    assert sd.split_options(conf, "train", refine=True) == dict(start=0, end=445, skip=4, downscale=2, refine=True, fitting=False)
    assert sd.split_options(conf, "test") == dict(start=446, end=647, skip=4, downscale=2)
    with pytest.raises(sd.SequenceError, match="no opt.val"):
        sd.split_options(conf, "val")


def test_the_io_header_is_declared_and_built():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    io = _lib.declarations("io")
    assert list(io) == ["ia_io_ingest_chunk"] and io["ia_io_ingest_chunk"].stream
    assert [p.name for p in io["ia_io_ingest_chunk"].params] == ["src_images", "src_masks", "mask_form", "n", "H0", "W0", "factor", "images",
                                                                 "masks", "first", "n_frames", "stream"]
    main = _lib.declarations()
    assert len(main) == 89 and set(_lib.EXPORTED) == set(main)
    assert os.path.normpath(_lib.header_path("io")) in [os.path.normpath(h) for h in build.SHARED_HEADERS] and "ia_io.hip" in build.SOURCES
    _lib.lib()
    assert "ia_io_ingest_chunk" in _lib._bound          # bound next to the main table: reachable through `_lib.call`
