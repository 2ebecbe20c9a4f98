"""PNG and animated PNG from frames that are on the device (csrc/ia_png.hip, include/instantavatar_hip_png.h; the definition is
DESIGN.md section 4, "PNG encoding").  `encode` filters and deflates a whole batch in one call; what comes back is, per image, the
complete zlib stream of its IDAT chunk.  Only those compressed bytes cross to the host (`Encoded.to_host`: one copy of the offsets,
one of the payload); signature, IHDR, chunk lengths and CRCs -- `zlib.crc32` over the compressed bytes -- are framed there.

    enc = png.encode(frames_u8, swap_rb=True)          # [n,H,W,4] or [n,H,W,3] uint8 on the GPU
    enc.write_png("0.png", 0); enc.write_apng("animation.png", fps=30)

There is no CPU path: without a device the call raises, as elsewhere in the package."""
import struct
import zlib

import torch

from . import _lib

DEFAULT_STRIP_ROWS = 16            # IA_PNG_DEFAULT_STRIP_ROWS
MAX_STRIP_BYTES = 126976           # IA_PNG_MAX_STRIP_BYTES
SIGNATURE = b"\x89PNG\r\n\x1a\n"


def default_strip_rows(W, C):
    """16 rows, fewer where 16 filtered rows of this width would not fit a strip (wider than 1920 x 4 bytes)"""
    return max(1, min(DEFAULT_STRIP_ROWS, MAX_STRIP_BYTES // (int(W) * int(C) + 1)))


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(kind)) & 0xFFFFFFFF)


def ihdr(H, W, C):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, {3: 2, 4: 6}[C], 0, 0, 0))


def frame_png(stream, H, W, C):
    """one zlib stream -> the bytes of a PNG file: signature, IHDR, one IDAT, IEND"""
    return SIGNATURE + ihdr(H, W, C) + chunk(b"IDAT", bytes(stream)) + chunk(b"IEND", b"")


def delay_fraction(fps):
    """the frame delay 1 / fps as APNG's 16-bit fraction: 1 / fps for an integer fps up to 65535, else round(1000 / fps) / 1000"""
    if float(fps) == int(fps) and 1 <= int(fps) <= 65535:
        return 1, int(fps)
    return max(1, min(65535, int(round(1000.0 / float(fps))))), 1000


def frame_apng(streams, H, W, C, fps=30, loop=0):
    """zlib streams of equally sized frames -> the bytes of an animated PNG: acTL, then per frame an fcTL (the full frame, dispose
    none, blend source) and its data, IDAT for frame 0 and fdAT for the others, sequence numbers running through fcTL and fdAT"""
    num, den = delay_fraction(fps)
    out = [SIGNATURE, ihdr(H, W, C), chunk(b"acTL", struct.pack(">II", len(streams), int(loop)))]
    seq = 0
    for i, s in enumerate(streams):
        out.append(chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, W, H, 0, 0, num, den, 0, 0)))
        seq += 1
        if i == 0:
            out.append(chunk(b"IDAT", bytes(s)))
        else:
            out.append(chunk(b"fdAT", struct.pack(">I", seq) + bytes(s)))
            seq += 1
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


class HostStreams:
    """the zlib streams of n frames of one size in host memory: `payload` (uint8 tensor or bytes-like), `offsets` (n + 1 ints)"""

    def __init__(self, payload, offsets, H, W, C, n_stored=0):
        self.payload = memoryview(payload.numpy() if isinstance(payload, torch.Tensor) else payload)
        self.offsets = [int(o) for o in offsets]
        self.H, self.W, self.C, self.n_stored = int(H), int(W), int(C), int(n_stored)

    def __len__(self):
        return len(self.offsets) - 1

    def stream(self, i):
        return self.payload[self.offsets[i]:self.offsets[i + 1]]

    def png_bytes(self, i):
        return frame_png(self.stream(i), self.H, self.W, self.C)

    def write_png(self, path, i):
        with open(path, "wb") as f:
            f.write(self.png_bytes(i))

    def apng_bytes(self, fps=30, loop=0, order=None):
        return frame_apng([self.stream(i) for i in (range(len(self)) if order is None else order)], self.H, self.W, self.C, fps, loop)

    def write_apng(self, path, fps=30, loop=0):
        with open(path, "wb") as f:
            f.write(self.apng_bytes(fps, loop))


class Encoded:
    """what `encode` returns: `stream` (device uint8, the streams one behind the other), `offsets` (device int64 [n + 1]),
    `n_stored` (device int32 [1]: strips that took the stored fallback), `strip_kinds` (device int32 [n, S]: 1 = stored)"""

    def __init__(self, stream, meta, strip_kinds, n, H, W, C, strip_rows):
        self.stream, self._meta, self.strip_kinds = stream, meta, strip_kinds
        self.offsets = meta[:n + 1]
        self.n_stored = meta[n + 1:].view(torch.int32)[:1]
        self.n, self.H, self.W, self.C, self.strip_rows = n, H, W, C, strip_rows
        self._host = None

    def __len__(self):
        return self.n

    def to_host(self):
        """-> HostStreams.  Two copies: the offsets (with n_stored behind them), then exactly the compressed bytes, into pinned memory"""
        if self._host is None:
            meta = self._meta.cpu()
            total = int(meta[self.n])
            payload = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
            payload[:total].copy_(self.stream[:total])
            self._host = HostStreams(payload[:total], meta[:self.n + 1].tolist(), self.H, self.W, self.C,
                                     int(meta[self.n + 1:].view(torch.int32)[0]))
        return self._host

    def png_bytes(self, i):
        return self.to_host().png_bytes(i)

    def write_png(self, path, i):
        self.to_host().write_png(path, i)

    def write_apng(self, path, fps=30, loop=0):
        self.to_host().write_apng(path, fps, loop)


_streams = {}


class _side_stream:
    """with _side_stream(device): the entry point takes no NULL stream (torch's default one), so the launches go to one side stream per
    device, which picks up after torch's current stream; the current stream picks up after it at the end -- ordered on the device, no
    host synchronisation (the pattern of masks.py)"""

    def __init__(self, device):
        if device not in _streams:
            _streams[device] = torch.cuda.Stream(device)
        self.side, self.cur = _streams[device], torch.cuda.current_stream(device)
        self.ctx = torch.cuda.stream(self.side)

    def __enter__(self):
        self.side.wait_stream(self.cur)
        self.ctx.__enter__()

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        self.cur.wait_stream(self.side)


def bound_bytes(n, H, W, C, strip_rows):
    return int(_lib.call("ia_png_bound_bytes", int(n), int(H), int(W), int(C), int(strip_rows)))


def encode(images_u8, swap_rb=False, strip_rows=None):
    """images_u8 [n,H,W,C] (or [H,W,C]) uint8 on the GPU, C = 3 or 4 -> Encoded.  swap_rb: channels 0 and 2 are exchanged while reading
    (frames in the model's (B, G, R) order become RGB files).  strip_rows: rows per independently compressed strip (default 16)."""
    if not isinstance(images_u8, torch.Tensor) or images_u8.dtype != torch.uint8 or images_u8.dim() not in (3, 4):
        raise _lib.IAError("png.encode takes a uint8 tensor [n,H,W,C] or [H,W,C]")
    _lib.require_cuda(images_u8)
    im = images_u8[None] if images_u8.dim() == 3 else images_u8
    im = im.contiguous()
    n, H, W, C = (int(x) for x in im.shape)
    if strip_rows is None:
        strip_rows = default_strip_rows(W, max(C, 1))
    strip_rows = int(strip_rows)
    dev = im.device
    meta = torch.zeros(n + 2, dtype=torch.int64, device=dev)
    if n == 0:
        return Encoded(torch.empty(0, dtype=torch.uint8, device=dev), meta, torch.empty((0, 0), dtype=torch.int32, device=dev), 0, H, W, C, strip_rows)
    bound = bound_bytes(n, H, W, C, strip_rows)
    S = int(_lib.call("ia_png_strips", H, W, C, strip_rows))
    if bound == 0 or S == 0:
        raise _lib.IAError("png.encode: %d images of %d x %d x %d in strips of %d rows: C is 3 or 4, sizes are positive, a strip holds at most "
                           "%d filtered bytes and the batch less than 2^31 bytes" % (n, H, W, C, strip_rows, MAX_STRIP_BYTES))
    with torch.cuda.device(dev):
        # (allocated on the current stream, which also is where they are used and freed; the side stream runs in between)
        out = torch.empty(bound, dtype=torch.uint8, device=dev)
        kinds = torch.empty((n, S), dtype=torch.int32, device=dev)
        ws = torch.empty(int(_lib.call("ia_png_workspace_bytes", n, H, W, C, strip_rows)), dtype=torch.uint8, device=dev)
        with _side_stream(dev):
            _lib.call("ia_png_encode", im, n, H, W, C, 1 if swap_rb else 0, strip_rows, out, bound, meta, meta[n + 1:].view(torch.int32), kinds,
                      ws, ws.numel())
    return Encoded(out, meta, kinds, n, H, W, C, strip_rows)
