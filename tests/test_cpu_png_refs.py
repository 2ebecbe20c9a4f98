"""tests/png_refs.py -- the numpy / Python reference the GPU PNG encoder is compared with byte for byte (tests/test_gpu_png.py) --
checked against zlib, PIL and the written definition (include/instantavatar_hip_png.h, DESIGN.md section 4 "PNG encoding"), and
what the C entry points decide on the host before any launch.  No GPU."""
import io
import os
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

import png_refs as pr

CASES = pr.all_cases()
IDS = ["%dx%dx%d-%s" % (s + (n,)) for s, n in CASES]


def _open(data):
    """PIL with its CRC checks on: a wrong chunk CRC or a truncated stream raises"""
    from PIL import ImageFile, PngImagePlugin
    assert ImageFile.LOAD_TRUNCATED_IMAGES is False
    im = Image.open(io.BytesIO(data))
    assert isinstance(im, PngImagePlugin.PngImageFile)
    return im


def _pixels(data, C):
    im = _open(data)
    assert im.mode == {3: "RGB", 4: "RGBA"}[C]
    return np.asarray(im)


@pytest.mark.parametrize("shape,name", CASES, ids=IDS)
def test_the_stream_inflates_to_the_filtered_bytes_and_the_file_to_the_pixels(shape, name):
    H, W, C = shape
    for sr in pr.strip_heights(H):
        for swap in (False, True):
            img, stream, kinds, infos, filt = pr.case(shape, name, swap, sr)
            assert stream[:2] == b"\x78\x01" and (stream[0] * 256 + stream[1]) % 31 == 0
            assert zlib.decompress(stream) == filt, (sr, swap)
            d = zlib.decompressobj()
            assert d.decompress(stream) == filt and d.eof and d.unused_data == b""        # nothing behind the Adler-32
            assert len(filt) == H * (W * C + 1) and len(kinds) == -(-H // sr)
            want = img[..., [2, 1, 0] + [3] * (C - 3)] if swap else img
            assert np.array_equal(_pixels(pr.png_bytes(stream, H, W, C), C), want), (sr, swap)
            assert len(stream) <= pr.bound_bytes(1, H, W, C, sr)
            for info in infos:
                assert pr.kraft(info["ll"]) == (1 << max(info["ll"]), 1 << max(info["ll"])) and max(info["ll"]) <= 15
                assert pr.kraft(info["cl"]) == (1 << max(info["cl"]), 1 << max(info["cl"])) and max(info["cl"]) <= 7
                assert info["ll"][256] > 0 and 257 <= info["hlit"] <= 286 and 4 <= info["hclen"] <= 19


def test_filter_types_follow_the_rule_and_undo_to_the_pixels():
    """PIL's decoder undoes the filters (above); here the choice: every type's cost is recomputed the slow way for one image"""
    img = pr.avatar_frame(64)
    filt, types = pr.filter_image(img)
    assert set(types.tolist()) - {0} and filt[:, 0].tolist() == types.tolist()
    raw = img.reshape(64, -1).astype(int)
    for y in (0, 1, 20, 33, 63):
        costs = []
        for t in range(5):
            tot = 0
            for x in range(raw.shape[1]):
                a = raw[y, x - 4] if x >= 4 else 0
                b = raw[y - 1, x] if y else 0
                c = raw[y - 1, x - 4] if (y and x >= 4) else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = [0, a, b, (a + b) // 2, a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)][t]
                f = (raw[y, x] - pred) & 255
                tot += f if f < 128 else 256 - f
            costs.append(tot)
        assert types[y] == costs.index(min(costs)), (y, costs)
    assert pr.filter_image(np.zeros((3, 3, 4), np.uint8))[1].tolist() == [0, 0, 0]           # all five tie: the lowest type


def test_tokens_of_runs_around_the_thresholds():
    def toks(n):
        return pr.strip_tokens(np.full(n, 5, np.uint8))
    L, M = ("L", 5), lambda k: ("M", k)
    assert toks(1) == [L] and toks(2) == [L, L] and toks(3) == [L, L, L] and toks(4) == [L, M(3)]
    assert toks(259) == [L, M(258)] and toks(260) == [L, M(258), L] and toks(261) == [L, M(258), L, L]
    assert toks(262) == [L, M(258), M(3)] and toks(600) == [L, M(258), M(258), M(83)]
    s = np.concatenate([np.full(4, 1), np.full(2, 2), np.full(5, 1)]).astype(np.uint8)
    assert pr.strip_tokens(s) == [("L", 1), ("M", 3), ("L", 2), ("L", 2), ("L", 1), ("M", 4)]
    for n in range(3, 259):                                   # the length codes: the RFC's table, every length once
        sym, eb, ev = pr.length_code(n)
        code, eb2, first = pr.LENGTH_CODES[sym - 257]
        assert code == sym and eb == eb2 and first + ev == n and 0 <= ev < (1 << eb) or n == 258
    assert pr.length_code(258) == (285, 0, 0) and pr.length_code(257) == (284, 5, 30)
    # every run length of the issue occurs in the runs image, and a strip never looks behind its first byte
    img, stream, kinds, infos, filt = pr.case((33, 19, 4), "runs", False, 2)
    assert kinds.count("dynamic") > 0


def test_code_lengths_limit_and_tie_rules():
    fib = [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765]
    for limit, freq in ((15, fib), (7, fib[:12]), (7, [1] * 19), (15, [3] * 286), (7, [0, 5, 0, 5]), (15, [1, 0, 0, 1000000])):
        st = {}
        lens = pr.build_lengths(freq, limit, st)
        used = [l for l in lens if l]
        assert len(used) == sum(1 for f in freq if f) and max(used) <= limit
        assert pr.kraft(lens)[0] == pr.kraft(lens)[1], (limit, freq)
        order = sorted((f, s) for s, f in enumerate(freq) if f)                 # a more frequent symbol never has the longer code
        assert all(lens[a[1]] >= lens[b[1]] for a, b in zip(order, order[1:]))
    st = {}
    assert max(pr.build_lengths(fib, 15, st)) == 15 and st["depth"] == 19      # the limit did something
    assert pr.build_lengths([5, 5, 5, 5], 15) == [2, 2, 2, 2] and pr.build_lengths([1, 1, 2], 15) == [2, 2, 1]
    assert pr.build_lengths([2, 1, 1], 15) == [1, 2, 2] and pr.build_lengths([1, 1, 1], 15) == [2, 2, 1]       # ties: the highest symbol first
    # the deep-tree case of the GPU test does exceed the limit, in the strip that holds the whole image
    infos = pr.case((128, 128, 4), "fibonacci", False, 128)[3]
    assert infos[0]["ll_depth"] > 15 and max(infos[0]["ll"]) == 15
    assert pr.code_length_tokens([0] * 139 + [3] * 8 + [0] * 4 + [2, 2]) == [(18, 127), (0, 0), (3, 0), (16, 3), (3, 0), (17, 1), (2, 0), (2, 0)]
    assert pr.code_length_tokens([0] * 10 + [0] + [7] * 4) == [(18, 0), (7, 0), (16, 0)]


def test_the_stored_fallback_where_the_reference_takes_it():
    """n_stored = 0 for the zeros, constant, ramp, disc and avatar contents wherever a strip is large enough for a dynamic block to pay;
    the one shape where it is not is 1 x 1 x 4 (five filtered bytes: stored 10 bytes, the shortest dynamic block 12)"""
    for shape, name in CASES:
        for sr in pr.strip_heights(shape[0]):
            kinds = pr.case(shape, name, False, sr)[2]
            if name in pr.NOT_STORED + ("avatar",) and shape != (1, 1, 4):
                assert "stored" not in kinds, (shape, name, sr)
            if name == "random" or shape == (1, 1, 4):
                assert "stored" in kinds, (shape, name, sr)
    big = np.random.default_rng(0).integers(0, 256, 70000, dtype=np.uint8)
    piece = pr.stored_strip(big, True)                      # two stored blocks, BFINAL on the second
    assert len(piece) == pr.stored_bytes(70000) == 70010 and piece[0] == 0 and piece[65540] == 1
    assert zlib.decompress(b"\x78\x01" + piece + struct.pack(">I", zlib.adler32(big.tobytes()))) == big.tobytes()
    assert pr.encode_strip(big, True)[1] == "stored"


def test_adler_combination():
    g = np.random.default_rng(4)
    data = g.integers(0, 256, 200000, dtype=np.uint8)
    for cuts in ([200000], [1, 199999], [65521, 70000, 64479], [3] * 5 + [199985]):
        parts, at = [], 0
        for c in cuts:
            parts.append(pr.strip_sums(data[at:at + c]))
            at += c
        assert pr.adler_combine(parts) == zlib.adler32(data.tobytes())


def test_apng_frames_count_and_duration():
    shape = (33, 19, 4)
    imgs = [pr.case(shape, n, False, 16)[0] for n in ("disc", "hramp", "random")]
    streams = [pr.case(shape, n, False, 16)[1] for n in ("disc", "hramp", "random")]
    for fps, ms in ((30, 1000.0 / 30), (25, 40.0), (12.5, 80.0)):
        im = _open(pr.apng_bytes(streams, 33, 19, 4, fps=fps, loop=0))
        assert im.is_animated and im.n_frames == 3 and im.info.get("loop") == 0
        for k in range(3):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGBA")), imgs[k]), k
            assert abs(im.info["duration"] - ms) < 1e-6 * ms + 1e-9, (fps, im.info["duration"])
    one = _open(pr.apng_bytes(streams[:1], 33, 19, 4))
    assert getattr(one, "n_frames", 1) == 1 and np.array_equal(np.asarray(one), imgs[0])
    bad = bytearray(pr.png_bytes(streams[0], 33, 19, 4))
    bad[-20] ^= 1                                           # PIL's checks are on: a flipped bit in the IDAT chunk is noticed
    with pytest.raises(Exception):
        _open(bytes(bad)).load()


def test_package_framing_equals_the_reference():
    from instantavatar_amd import png
    shape = (5, 7, 3)
    streams = [pr.case(shape, n, False, 2)[1] for n in ("disc", "random")]
    assert png.frame_png(streams[0], 5, 7, 3) == pr.png_bytes(streams[0], 5, 7, 3)
    for fps in (30, 12.5):
        assert png.frame_apng(streams, 5, 7, 3, fps=fps, loop=2) == pr.apng_bytes(streams, 5, 7, 3, fps=fps, loop=2)
    assert png.DEFAULT_STRIP_ROWS == pr.DEFAULT_STRIP_ROWS and png.MAX_STRIP_BYTES == pr.MAX_STRIP_BYTES
    assert png.default_strip_rows(1920, 4) == 16 and png.default_strip_rows(4096, 4) == 7 and png.default_strip_rows(1, 3) == 16


def test_binding_table_bound_and_host_side_refusals():
    from instantavatar_amd import _lib, build
    d = _lib.declarations("png")
    assert sorted(d) == ["ia_png_bound_bytes", "ia_png_encode", "ia_png_strips", "ia_png_workspace_bytes"]
    assert d["ia_png_encode"].stream and len(d["ia_png_encode"].params) == 15
    assert hasattr(_lib.lib(), "ia_png_encode") and "ia_png_encode" in _lib._bound
    assert "ia_png.hip" in build.SOURCES and "ia_png.hip" in build.source_manifest() and "ia_png.hip" in build.library_manifest()
    assert os.path.normpath(_lib.header_path("png")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    with open(_lib.header_path("png")) as f:
        text = f.read()
    assert "#define IA_PNG_DEFAULT_STRIP_ROWS %d" % pr.DEFAULT_STRIP_ROWS in text and "#define IA_PNG_MAX_STRIP_BYTES %d" % pr.MAX_STRIP_BYTES in text
    # the bound is a closed expression: the C function and the reference agree, and the default strip fits 1920 x 4 bytes
    for n, H, W, C, sr in ((1, 1, 1, 4, 16), (3, 33, 19, 4, 2), (3, 33, 19, 3, 16), (2, 33, 19, 4, 33), (8, 1080, 1920, 4, 16), (1, 64, 64, 4, 100),
                           (1, 40, 8000, 4, 3), (1, 5, 7, 2, 2), (1, 5, 7, 4, 0), (0, 5, 7, 4, 2), (1, 40, 8000, 4, 4), (200, 1080, 1920, 4, 16)):
        want = pr.bound_bytes(n, H, W, C, sr) if 0 < n and pr.bound_bytes(n, H, W, C, sr) < 2 ** 31 else 0
        assert _lib.call("ia_png_bound_bytes", n, H, W, C, sr) == want, (n, H, W, C, sr)
        assert (_lib.call("ia_png_workspace_bytes", n, H, W, C, sr) > 0) == (want > 0)
        assert _lib.call("ia_png_strips", H, W, C, sr) == (-(-H // sr) if pr.check_strip_rows(H, W, C, sr) else 0)
    assert _lib.call("ia_png_bound_bytes", 8, 1080, 1920, 4, 16) > 0 and 16 * (1920 * 4 + 1) <= pr.MAX_STRIP_BYTES
    P = 4096                                                  # (a non-null address that is never read: every call below is refused)

    def enc(n=1, H=5, W=7, C=4, sr=2, out_bytes=1 << 20, ws_bytes=1 << 24, stream=P, images=P):
        return _lib.call("ia_png_encode", images, n, H, W, C, 0, sr, P, out_bytes, P, P, None, P, ws_bytes, stream)
    for kw, msg in ((dict(C=2), "C = 2"), (dict(sr=0), "strip_rows 0"), (dict(out_bytes=pr.bound_bytes(1, 5, 7, 4, 2) - 1), "ia_png_bound_bytes"),
                    (dict(stream=None), "stream = NULL"), (dict(ws_bytes=16), "ia_png_workspace_bytes"), (dict(images=None), "are required"),
                    (dict(H=40, W=8000, sr=4), "filtered bytes"), (dict(n=-1), "n < 0")):
        with pytest.raises(_lib.IAError, match=msg):
            enc(**kw)
    assert enc(n=0) == 0
