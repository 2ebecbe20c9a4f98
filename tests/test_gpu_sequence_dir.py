"""Sequence ingest on the device: `ia_io_ingest_chunk` (csrc/ia_io.hip) against the numpy restatement of
tests/sequence_fixture.py bit for bit (and, for uint8, against PIL's `Image.reduce(2)`, an independent implementation of the
same rounded box: tests/test_cpu_sequence_dir.py::test_pil_reduce_is_the_same_rounded_box), `DeviceFrames.from_directory`
against `DeviceFrames.from_arrays` fed with restated arrays and against the reference's val-split items
(tests/golden/sequence_dir_golden.npz), and the drivers' `--data` path."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import sequence_fixture as fx  # noqa: E402

from instantavatar_amd import _lib  # noqa: E402
from instantavatar_amd.datasets import sequence_dir as sd  # noqa: E402
from instantavatar_amd.datasets.device_frames import DeviceFrames  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = np.load(os.path.join(HERE, "golden", "sequence_dir_golden.npz"))
U8, GREY = 1, 2      # IA_IO_MASK_U8 / IA_IO_MASK_GREY


def ingest(src_img, src_msk, form, factor, chunk):
    """the stores after the chunks of [n, H0, W0(, 3)] host arrays went through two alternating device staging buffers on a
    side stream, as from_directory drives the kernel (src_img or src_msk None: a launch without that plane)"""
    n, H0, W0 = (src_img if src_img is not None else src_msk).shape[:3]
    H, W = H0 // factor, W0 // factor
    images = torch.full((n, H, W, 3), 77, dtype=torch.uint8, device=DEV)
    masks = torch.full((n, H, W), -1.0, device=DEV)
    px = H0 * W0
    stage = [torch.empty(chunk * px * 4, dtype=torch.uint8, device=DEV) for _ in range(2)]
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for k, first in enumerate(range(0, n, chunk)):
            m, s = min(chunk, n - first), stage[k % 2]
            s_img, s_msk = s[:chunk * px * 3], s[chunk * px * 3:]
            if src_img is not None:
                s_img[:m * px * 3].copy_(torch.from_numpy(np.ascontiguousarray(src_img[first:first + m])).reshape(-1))
            if src_msk is not None:
                s_msk[:m * px].copy_(torch.from_numpy(np.ascontiguousarray(src_msk[first:first + m])).reshape(-1))
            _lib.call("ia_io_ingest_chunk", s_img if src_img is not None else None, s_msk if src_msk is not None else None, form, m, H0, W0,
                      factor, images, masks, first, n)
    side.synchronize()
    return images.cpu().numpy(), masks.cpu().numpy()


# (H0, W0, factor): the issue's shapes -- a tail only (2 x 2, 66 x 2), groups and a tail (2 x 34, 24 x 20), several workgroups
# (130 x 258), an odd-sized copy whose frames start at odd addresses (23 x 19) -- plus the sizes at which rows are 16-byte
# (4 x 32) and 8-byte (6 x 40) aligned, where the kernel takes its wider load tiers, and a copy with aligned frames (24 x 20)
SHAPES = [(24, 20, 2), (2, 2, 2), (2, 34, 2), (66, 2, 2), (130, 258, 2), (23, 19, 1), (4, 32, 2), (6, 40, 2), (24, 20, 1)]


@pytest.mark.parametrize("H0, W0, factor", SHAPES, ids=["%dx%d_f%d" % s for s in SHAPES])
def test_kernel_equals_the_numpy_restatement_bit_for_bit(H0, W0, factor):
    from PIL import Image
    n = 5
    rs = np.random.RandomState(H0 * 1000 + W0)
    img = rs.randint(0, 256, (n, H0, W0, 3)).astype(np.uint8)
    img[0, :, : W0 // 2] = 255                                     # saturated cells: the sum needs more than 8 bits
    m01 = (rs.rand(n, H0, W0) < 0.5).astype(np.uint8)
    grey = rs.randint(0, 256, (n, H0, W0)).astype(np.uint8)
    want_img, want_m01, want_grey = fx.restate_u8(img, factor), fx.restate_mask(m01, "peoplesnapshot", factor), fx.restate_mask(grey, "custom", factor)
    for chunk in (1, 3, n):
        got_img, got_m01 = ingest(img, m01, U8, factor, chunk)      # image + uint8 mask in one launch per chunk
        assert np.array_equal(got_img, want_img), ("image", chunk, int((got_img != want_img).sum()))
        assert np.array_equal(got_m01.view(np.uint32), want_m01.view(np.uint32)), ("uint8 mask", chunk)
        left, got_grey = ingest(None, grey, GREY, factor, chunk)    # masks alone: the image store stays as it was
        assert np.array_equal(got_grey.view(np.uint32), want_grey.view(np.uint32)), ("grey mask", chunk, float(np.abs(got_grey - want_grey).max()))
        assert (left == 77).all()
        got_img2, left_m = ingest(img, None, U8, factor, chunk)     # images alone
        assert np.array_equal(got_img2, want_img) and (left_m == -1.0).all()
    assert set(np.unique(want_m01)) <= {0.0, 1.0}
    if factor == 2:
        for i in range(n):
            assert np.array_equal(got_img[i], np.asarray(Image.fromarray(img[i], "RGB").reduce(2)).reshape(want_img[i].shape)), i
            assert np.array_equal(got_m01[i], np.asarray(Image.fromarray(m01[i], "L").reduce(2)).astype(np.float32)), i


def test_kernel_refuses_what_it_does_not_restate():
    src = torch.zeros(25 * 20 * 4, dtype=torch.uint8, device=DEV)
    images, masks = torch.zeros((2, 12, 10, 3), dtype=torch.uint8, device=DEV), torch.zeros((2, 12, 10), device=DEV)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        for args, why in (((U8, 1, 24, 20, 3, images, masks, 0, 2), "downscale factor 3"), ((U8, 1, 25, 20, 2, images, masks, 0, 2), "even source size"),
                          ((U8, 1, 24, 20, 2, images, masks, 2, 2), "outside the store"), ((7, 1, 24, 20, 2, images, masks, 0, 2), "unknown mask form")):
            with pytest.raises(_lib.IAError, match=why):
                _lib.call("ia_io_ingest_chunk", src[:1500], src[1500:], *args)
    with pytest.raises(_lib.IAError, match="default stream"):
        _lib.call("ia_io_ingest_chunk", src[:1500], src[1500:], U8, 1, 24, 20, 2, images, masks, 0, 2, None)
    torch.cuda.synchronize()
    assert not images.any() and not masks.any()


@pytest.mark.parametrize("kind", sd.KINDS)
@pytest.mark.parametrize("downscale", [1, 2])
def test_from_directory_equals_from_arrays_on_restated_arrays(kind, downscale, tmp_path):
    wrote = fx.write_sequence(tmp_path / "seq", kind)
    seq = sd.read_sequence(tmp_path / "seq", kind, "train", dict(start=0, end=6, downscale=downscale))
    ref = DeviceFrames.from_arrays(fx.restate_u8(wrote["images"], downscale), fx.restate_mask(wrote["mask_bytes"], kind, downscale),
                                   seq.K, seq.c2w, seq.smpl_params, None, DEV)
    lines = []
    for chunk in (1, 3, None):
        got = DeviceFrames.from_directory(seq, None, DEV, chunk=chunk, log=lines.append)
        assert got.images.dtype == torch.uint8 and got.masks.dtype == torch.float32 and (got.N, got.H, got.W) == (7, 24 // downscale, 20 // downscale)
        assert torch.equal(got.images, ref.images) and torch.equal(got.masks.view(torch.int32), ref.masks.view(torch.int32)), chunk
        assert torch.equal(got.rays_o, ref.rays_o) and torch.equal(got.rays_d, ref.rays_d)
        assert sorted(got.smpl_params) == sorted(ref.smpl_params) and all(torch.equal(got.smpl_params[k], ref.smpl_params[k]) for k in ref.smpl_params)
    assert len(lines) == 3 and all("loaded 7 frames 20x24" in l and "MB/s decoded" in l for l in lines), lines
    # a sliced split takes the files of the slice
    part = DeviceFrames.from_directory(sd.read_sequence(tmp_path / "seq", kind, "train", dict(start=1, end=5, skip=2, downscale=downscale)), None, DEV)
    assert torch.equal(part.images, ref.images[1:6:2]) and torch.equal(part.masks, ref.masks[1:6:2])


@pytest.mark.parametrize("name", fx.VAL_CASES)
def test_val_frame_equals_the_reference_item(name, tmp_path):
    _, kind, split, opt, cached = next(c for c in fx.CASES if c[0] == name)
    fx.write_sequence(tmp_path / "seq", kind, cached=cached)
    frames = DeviceFrames.from_directory(sd.read_sequence(tmp_path / "seq", kind, split, opt), None, DEV)
    b = frames.frame(0)
    g = lambda k: GOLDEN[name + "/item/" + k]
    assert np.array_equal(b["rgb"][0].cpu().numpy(), g("rgb")) and np.array_equal(b["alpha"][0].cpu().numpy(), g("alpha"))     # exact to float32
    np.testing.assert_allclose(b["near"][0].cpu().numpy(), g("near"), rtol=0, atol=1e-6)
    np.testing.assert_allclose(b["far"][0].cpu().numpy(), g("far"), rtol=0, atol=1e-6)
    np.testing.assert_allclose(frames.rays_d.cpu().numpy(), GOLDEN[name + "/rays_d"], rtol=0, atol=1e-6)
    assert np.array_equal(frames.rays_o.cpu().numpy(), GOLDEN[name + "/rays_o"])


def test_a_file_that_differs_from_its_header_check_is_refused_while_decoding(tmp_path):
    fx.write_sequence(tmp_path / "seq", "peoplesnapshot")
    seq = sd.read_sequence(tmp_path / "seq", "peoplesnapshot", "train", dict(start=0, end=6, downscale=1))
    np.save(tmp_path / "seq" / "masks" / "mask_0004.npy", np.zeros((24, 20), np.float32))
    with pytest.raises(sd.SequenceError, match="mask_0004.npy: a float32 mask"):
        DeviceFrames.from_directory(seq, None, DEV)


def _run(module, args, timeout=600):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", module] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (module, args, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_drivers_train_and_evaluate_a_sequence_directory(tmp_path):
    """an 80 x 72 PeopleSnapshot directory at downscale 2: 40 x 36 is the smallest training size confs/sampler/patch.yaml's 32-pixel
    patches fit into with room to move"""
    seq = str(tmp_path / "seq")
    fx.write_sequence(seq, "peoplesnapshot", height=80, width=72)
    ckpt = str(tmp_path / "ck" / "last.ckpt")
    data = ["--data", seq, "--dataset", "peoplesnapshot", "--downscale", "2", "--synthetic-body"]
    text = _run("instantavatar_amd.drivers.train", data + ["--start", "0", "--end", "3", "--val-frame", "4", "--steps", "4", "--res", "40", "--ckpt", ckpt])
    assert "[train] loaded 4 frames 72x80 -> 36x40 (peoplesnapshot, downscale 2)" in text and "MB/s decoded" in text, text
    assert "[val] loaded 1 frames" in text and "4 frames 36x40" in text and "val/rgb_loss" in text and "saved " in text, text
    assert torch.load(ckpt, weights_only=False)["global_step"] == 4
    out = str(tmp_path / "eval")
    text = _run("instantavatar_amd.drivers.eval", data + ["--start", "5", "--end", "6", "--ckpt", ckpt, "--epochs", "1", "--out", out])
    assert "[test] loaded 2 frames" in text and "wrote 2 test images" in text, text
    assert sorted(os.listdir(os.path.join(out, "test"))) == ["0.png", "1.png"] and os.path.exists(os.path.join(out, "results.txt"))
    from PIL import Image
    assert Image.open(os.path.join(out, "test", "0.png")).size == (3 * 36, 40)      # [ground truth | rendering | error map]


def test_eval_driver_wants_exactly_one_data_source(capsys):
    from instantavatar_amd.drivers import eval as eval_driver
    for argv in ([], ["--synthetic", "--data", "somewhere"]):
        with pytest.raises(SystemExit) as e:
            eval_driver.main(argv)
        assert e.value.code == 2 and "exactly one of --synthetic / --data" in capsys.readouterr().err
