"""The PNG encoder on the GPU (csrc/ia_png.hip through instantavatar_amd/png.py and the C ABI) against the Python reference of
tests/png_refs.py, which tests/test_cpu_png_refs.py checks on the CPU against zlib and PIL.  Everything is integer, so every
comparison is for equality of bytes.  Shapes, strip heights, batch sizes and contents are the smallest at which the kernels can go
wrong: one pixel, odd sizes, three and four channels, a short last strip, runs around the three-byte and the 258-byte thresholds,
runs across strip boundaries, noise (the stored fallback), and a tree deeper than the 15-bit limit.  Then refusals and the driver."""
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import png_refs as pr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _encode(imgs, **kw):
    from instantavatar_amd import png
    enc = png.encode(torch.as_tensor(np.array(imgs)).to(DEV), **kw)
    host = enc.to_host()
    return enc, host, [bytes(host.stream(i)) for i in range(len(host))]


def _pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)))


def _kinds(enc, i):
    return ["stored" if k else "dynamic" for k in enc.strip_kinds[i].cpu().tolist()]


def _first_difference(a, b):
    k = next((j for j, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "lengths %d / %d, first difference at byte %d: %s / %s" % (len(a), len(b), k, a[k:k + 8].hex(), b[k:k + 8].hex())


@pytest.mark.parametrize("shape", pr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_every_content_equals_the_reference_and_round_trips(shape):
    H, W, C = shape
    names = list(pr.contents(*shape))
    for sr in pr.strip_heights(H):
        for swap in (False, True):
            refs = [pr.case(shape, n, swap, sr) for n in names]
            enc, host, got = _encode(np.stack([r[0] for r in refs]), swap_rb=swap, strip_rows=sr)
            stored = 0
            for i, (name, (img, stream, kinds, infos, filt)) in enumerate(zip(names, refs)):
                what = (shape, sr, swap, name)
                assert zlib.decompress(got[i]) == filt, what                      # round trip: the filtered bytes ...
                want = img[..., [2, 1, 0] + [3] * (C - 3)] if swap else img
                assert np.array_equal(_pixels(host.png_bytes(i)), want), what     # ... and through PIL the pixels
                assert _kinds(enc, i) == kinds, what
                assert got[i] == stream, (what, _first_difference(got[i], stream))
                assert len(got[i]) <= pr.bound_bytes(1, H, W, C, sr), what
                stored += kinds.count("stored")
                if name in pr.NOT_STORED and shape != (1, 1, 4):                  # (1 x 1: see test_cpu_png_refs: stored is shorter there)
                    assert "stored" not in _kinds(enc, i), what
                if name == "random":
                    assert "stored" in _kinds(enc, i), what
            assert int(enc.n_stored.item()) == host.n_stored == stored > 0
            from instantavatar_amd import png
            assert int(enc.offsets[-1]) <= png.bound_bytes(len(names), H, W, C, sr) == pr.bound_bytes(len(names), H, W, C, sr)


@pytest.mark.parametrize("shape", pr.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_batches_of_one_and_three_and_determinism(shape):
    """image i encoded alone has the bytes it has inside a batch, wherever it stands; two calls give the same bytes"""
    H, W, C = shape
    names = list(pr.contents(*shape))
    for sr in pr.strip_heights(H):
        want = {n: pr.case(shape, n, False, sr)[1] for n in names}
        imgs = {n: pr.case(shape, n, False, sr)[0] for n in names}
        for trio in (names[0:3], names[3:6], [names[7], names[6], names[0]]):
            enc, host, got = _encode(np.stack([imgs[n] for n in trio]), strip_rows=sr)
            assert got == [want[n] for n in trio], (shape, sr, trio)
            again = _encode(np.stack([imgs[n] for n in trio]), strip_rows=sr)[2]
            assert again == got
            assert int(enc.n_stored.item()) == sum(pr.case(shape, n, False, sr)[2].count("stored") for n in trio)
        for n in names:
            enc, host, got = _encode(imgs[n][None], strip_rows=sr)
            assert got == [want[n]], (shape, sr, n)
    enc, host, got = _encode(imgs["disc"])                                        # [H,W,C] in, the default strip height
    assert len(host) == 1 and got[0] == pr.case(shape, "disc", False, pr.DEFAULT_STRIP_ROWS)[1]


def test_the_avatar_frame_and_a_tree_deeper_than_fifteen_bits():
    for sr in pr.strip_heights(64):
        img, stream, kinds, infos, filt = pr.case((64, 64, 4), "avatar", False, sr)
        others = [pr.avatar_frame(64, seed) for seed in (1, 2)]
        enc, host, got = _encode(np.stack([img] + others), strip_rows=sr)
        assert got[0] == stream, _first_difference(got[0], stream)
        assert int(enc.n_stored.item()) == 0 and set(_kinds(enc, 0)) == {"dynamic"} and kinds == _kinds(enc, 0)
        for i, o in enumerate(others):
            assert zlib.decompress(got[i + 1]) == pr.filter_image(o)[0].tobytes() and np.array_equal(_pixels(host.png_bytes(i + 1)), o)
        assert _encode(img[None], strip_rows=sr)[2][0] == stream
        assert _encode(img[None], strip_rows=sr, swap_rb=True)[2][0] == pr.case((64, 64, 4), "avatar", True, sr)[1]
    for sr in (16, 128):
        img, stream, kinds, infos, filt = pr.case((128, 128, 4), "fibonacci", False, sr)
        enc, host, got = _encode(img[None], strip_rows=sr)
        assert zlib.decompress(got[0]) == filt
        assert got[0] == stream, _first_difference(got[0], stream)
        assert _kinds(enc, 0) == kinds == ["dynamic"] * len(kinds)
    assert infos[0]["ll_depth"] > 15          # (sr = 128: the limit rule was needed)


def test_apng_of_a_batch_of_three(tmp_path):
    shape = (33, 19, 4)
    names = ("disc", "runs", "random")
    imgs = [pr.case(shape, n, False, 16)[0] for n in names]
    enc, host, got = _encode(np.stack(imgs), strip_rows=16)
    path = str(tmp_path / "a.png")
    enc.write_apng(path, fps=25, loop=0)
    assert open(path, "rb").read() == pr.apng_bytes(got, 33, 19, 4, fps=25, loop=0)
    im = Image.open(path)
    assert im.n_frames == 3
    for k in range(3):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("RGBA")), imgs[k]) and abs(im.info["duration"] - 40.0) < 1e-6
    enc.write_png(str(tmp_path / "1.png"), 1)
    assert np.array_equal(np.asarray(Image.open(str(tmp_path / "1.png"))), imgs[1])


def test_bad_arguments_return_a_status_and_write_nothing():
    from instantavatar_amd import _lib, png
    n, H, W, C, sr = 2, 5, 7, 4, 2
    imgs = torch.as_tensor(np.stack([pr.case((5, 7, 4), k, False, 2)[0] for k in ("disc", "random")])).to(DEV)
    bound = png.bound_bytes(n, H, W, C, sr)
    out = torch.full((bound,), 0xAB, dtype=torch.uint8, device=DEV)
    meta = torch.full((n + 2,), -7, dtype=torch.int64, device=DEV)
    kinds = torch.full((n, 3), -7, dtype=torch.int32, device=DEV)
    ws = torch.full((int(_lib.call("ia_png_workspace_bytes", n, H, W, C, sr)),), 0xCD, dtype=torch.uint8, device=DEV)

    side = torch.cuda.Stream(DEV)                    # (the entry point takes no NULL stream, which torch's default one is)
    torch.cuda.synchronize()

    def enc(C=C, sr=sr, out_bytes=bound, stream=side.cuda_stream, ws_bytes=None):
        return _lib.call("ia_png_encode", imgs, n, H, W, C, 0, sr, out, out_bytes, meta, meta[n + 1:].view(torch.int32), kinds, ws,
                         ws.numel() if ws_bytes is None else ws_bytes, stream)
    for kw in (dict(C=2), dict(sr=0), dict(out_bytes=bound - 1), dict(stream=None), dict(ws_bytes=ws.numel() - 1)):
        with pytest.raises(_lib.IAError, match="ia_png_encode"):
            enc(**kw)
        torch.cuda.synchronize()
        assert bool((out == 0xAB).all()) and bool((meta == -7).all()) and bool((kinds == -7).all()) and bool((ws == 0xCD).all()), kw
    assert _lib.lib().ia_png_encode(imgs.data_ptr(), n, H, W, 2, 0, sr, out.data_ptr(), bound, meta.data_ptr(), meta[n + 1:].data_ptr(), None,
                                    ws.data_ptr(), ws.numel(), side.cuda_stream) < 0          # the status itself
    assert enc() == 0                                            # and the same buffers are accepted when the arguments are right
    torch.cuda.synchronize()
    total = int(meta[n])
    assert meta[0] == 0 and 0 < total <= bound and bool((out[total:] == 0xAB).all())      # nothing behind the last stream is touched
    assert bytes(out[:int(meta[1])].cpu().numpy()) == pr.case((5, 7, 4), "disc", False, 2)[1]
    with pytest.raises(_lib.IAError, match="GPU"):
        png.encode(torch.zeros((1, 5, 7, 4), dtype=torch.uint8))                          # no CPU path


def test_animate_driver_with_and_without_gpu_png(tmp_path):
    from instantavatar_amd.drivers import animate
    plain, gpu = str(tmp_path / "plain"), str(tmp_path / "gpu")
    common = ["--synthetic", "--size", "64", "--max-frames", "4", "--jitter-seed", "1"]
    assert animate.main(common + ["--out", plain]) == 0
    assert animate.main(common + ["--out", gpu, "--gpu-png", "--apng"]) == 0
    assert sorted(os.listdir(plain)) == sorted(["%d.png" % i for i in range(4)] + ["animation.gif"])
    assert sorted(os.listdir(gpu)) == sorted(["%d.png" % i for i in range(4)] + ["animation.gif", "animation.png"])
    anim = Image.open(os.path.join(gpu, "animation.png"))
    assert anim.n_frames == 4
    frames = []
    for i in range(4):
        a = np.asarray(Image.open(os.path.join(plain, "%d.png" % i)))
        b = np.asarray(Image.open(os.path.join(gpu, "%d.png" % i)))
        assert a.shape == (64, 64, 4) and np.array_equal(a, b), i
        anim.seek(i)
        assert np.array_equal(np.asarray(anim.convert("RGBA")), a), i
        # the plain run's files are what PIL's encoder gives for the same arrays: the default route is untouched
        buf = io.BytesIO()
        Image.fromarray(a, "RGBA").save(buf, format="PNG")
        assert open(os.path.join(plain, "%d.png" % i), "rb").read() == buf.getvalue(), i
        frames.append(a)
    assert (np.stack(frames)[..., 3] > 128).mean() > 0.02 and any(not np.array_equal(frames[0], f) for f in frames[1:])
    assert open(os.path.join(plain, "animation.gif"), "rb").read() == open(os.path.join(gpu, "animation.gif"), "rb").read()
    buf = io.BytesIO()
    ims = [Image.fromarray(f, "RGBA") for f in frames]
    ims[0].save(buf, format="GIF", save_all=True, append_images=ims[1:], duration=33, loop=0)
    assert open(os.path.join(plain, "animation.gif"), "rb").read() == buf.getvalue()


def _same_pictures(a, b, animations=()):
    """every <name>.png of the plain run `a` is in the --gpu-png run `b` with the same pixels; -> their names"""
    names = sorted(f for f in os.listdir(a) if f.endswith(".png"))
    assert names and set(names) <= set(os.listdir(b)) and set(os.listdir(b)) - set(os.listdir(a)) == set(animations)
    for f in names:
        x, y = np.asarray(Image.open(os.path.join(a, f))), np.asarray(Image.open(os.path.join(b, f)))
        assert x.shape == y.shape and np.array_equal(x, y), f
    return names


def _animation_holds(path, frames):
    im = Image.open(path)
    assert im.n_frames == len(frames)
    for k, f in enumerate(frames):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("RGBA")), np.asarray(Image.open(f).convert("RGBA"))), (path, k)


def test_novel_view_with_normals_and_scene_take_the_flags(tmp_path):
    from instantavatar_amd.drivers import novel_view, scene
    P = lambda n: str(tmp_path / n)
    common = ["--synthetic", "--frames", "3", "--downscale", "8", "--jitter-seed", "3", "--normals"]
    assert novel_view.main(common + ["--out", P("nv0")]) == 0 and novel_view.main(common + ["--out", P("nv1"), "--gpu-png", "--apng"]) == 0
    names = _same_pictures(P("nv0"), P("nv1"), animations=["rotation.png"])
    assert names == sorted("%s%d.png" % (p, i) for p in ("", "normal_", "shaded_") for i in range(3))
    _animation_holds(P("nv1/rotation.png"), [P("nv1/%d.png" % i) for i in range(3)])
    assert open(P("nv0/rotation.gif"), "rb").read() == open(P("nv1/rotation.gif"), "rb").read()
    common = ["--synthetic", "--seeds", "42", "43", "--size", "64", "--max-frames", "2", "--jitter-seed", "3"]
    assert not scene.main(common + ["--out", P("sc0")]) and not scene.main(common + ["--out", P("sc1"), "--gpu-png", "--apng"])
    assert _same_pictures(P("sc0"), P("sc1"), animations=["scene.png"]) == ["0.png", "1.png"]
    _animation_holds(P("sc1/scene.png"), [P("sc1/0.png"), P("sc1/1.png")])
    assert open(P("sc0/scene.gif"), "rb").read() == open(P("sc1/scene.gif"), "rb").read()
    assert not scene.main(common + ["--out", P("sc2"), "--gpu-png", "--no-gif"]) and sorted(os.listdir(P("sc2"))) == ["0.png", "1.png"]
    for drv in (novel_view, scene):
        with pytest.raises(SystemExit):
            drv.main(["--synthetic", "--apng", "--out", P("no")])              # --apng needs --gpu-png


def test_mesh_pictures_take_the_flags(tmp_path):
    from instantavatar_amd.drivers import animate, extract_mesh
    P = lambda n: str(tmp_path / n)
    common = ["--synthetic", "--max-frames", "2", "--size", "64", "--mesh-preview", "32"]
    assert animate.main(common + ["--out", P("mp0")]) == 0 and animate.main(common + ["--out", P("mp1"), "--gpu-png"]) == 0
    assert _same_pictures(P("mp0"), P("mp1")) == ["mesh_0.png", "mesh_1.png"]
    track = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aist_demo_200.npz")
    common = ["--synthetic", "--resolution", "32", "--poses", track, "--max-frames", "2", "--render", "64"]
    assert extract_mesh.main(common + ["--out", P("em0")]) == 0 and extract_mesh.main(common + ["--out", P("em1"), "--gpu-png", "--apng"]) == 0
    pngs = lambda d: [f for f in sorted(os.listdir(d)) if f.endswith(".png")]
    assert pngs(P("em0")) == ["canonical_front.png", "posed_0.png", "posed_1.png", "posed_shaded_0.png", "posed_shaded_1.png"]
    assert pngs(P("em1")) == sorted(pngs(P("em0")) + ["posed.png", "posed_shaded.png"])
    for f in pngs(P("em0")):
        assert np.array_equal(np.asarray(Image.open(os.path.join(P("em0"), f))), np.asarray(Image.open(os.path.join(P("em1"), f)))), f
    _animation_holds(P("em1/posed.png"), [P("em1/posed_%d.png" % i) for i in range(2)])
    _animation_holds(P("em1/posed_shaded.png"), [P("em1/posed_shaded_%d.png" % i) for i in range(2)])
