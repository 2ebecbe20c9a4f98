"""GPU time of `ia_png_encode`, the size of its files next to PIL's, and the wall time of the drivers' write phase on both routes.

    python tools/time_png.py --out profiles/png_timing.txt [--repeat 20] [--frames 200] [--parts a b c]

The pictures are the synthetic avatar over the first frames of the `aist` pose track (tests/golden/aist_demo_200.npz), rendered here
and left on the device as the drivers leave them: 8-bit, model channel order, alpha = opacity.
  a  one `ia_png_encode` call on 32 frames of 512 x 512 and on 8 frames of 1080 x 1920 (the 1080 x 1080 picture centred on a
     transparent canvas): device events around the call on a side stream, `--repeat` calls after five warm-up calls
  b  over `--frames` frames of 512 x 512: the bytes of the GPU route's files over the bytes of PIL's default `save` of the same arrays
  c  `drivers.animate.render_sequence` on those frames, `write_s` of its result (encoding and writing, GIF / animated PNG included):
     PIL with 8 workers against --gpu-png, without a GIF, and PIL with its GIF against --gpu-png --apng; the routes alternate three
     times in this one process, each figure is reported with its spread
`--parts a` alone is what a `rocprofv3 --kernel-trace --stats` run of its own takes for the kernel split."""
import argparse
import io
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--parts", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from instantavatar_amd import _lib, png
    from instantavatar_amd.drivers import animate
    from instantavatar_amd.pipeline import build_synthetic_model
    if not torch.cuda.is_available():
        raise SystemExit("time_png: no GPU; a time measured elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    model, _, _ = build_synthetic_model(dev, seed=42)
    model.eval()
    z = np.load(os.path.join(ROOT, "tests", "golden", "aist_demo_200.npz"))
    poses, trans = z["poses"].astype(np.float32), z["trans"].astype(np.float32)
    jitter = animate.fixed_jitter(1, dev)

    def render(size, count):
        seq = animate.AnimateSequence(poses[:count], trans[:count], np.zeros(10, np.float32), dev, size=size)
        out = torch.empty((count, size, size, 4), dtype=torch.uint8, device=dev)
        with torch.inference_mode():
            for i in range(count):
                animate.pack_rgba8(model.render_image_fast(seq.batch(i), (size, size), jitter=jitter)[:4], out[i])
        torch.cuda.synchronize()
        return seq, out

    lines = ["ia_png_encode (%s): PNG filters + deflate (distance-1 matches, one dynamic-Huffman block per strip of %d rows)"
             % (torch.cuda.get_device_name(0), png.DEFAULT_STRIP_ROWS),
             "pictures: the synthetic avatar over the aist track, 8-bit RGBA on the device, channels 0 and 2 swapped while reading"]
    n512 = max(32, args.frames if ("b" in args.parts or "c" in args.parts) else 32)
    seq512, frames512 = render(512, n512)

    if "a" in args.parts:
        _, sq = render(1080, 8)
        wide = torch.zeros((8, 1080, 1920, 4), dtype=torch.uint8, device=dev)
        wide[:, :, 420:1500] = sq
        side = torch.cuda.Stream(dev)
        lines += ["(a) one call: device events on a side stream, median (min .. max) of %d calls after 5 warm-up calls; 5 launches per call" % args.repeat,
                  "%12s %6s %26s %12s %16s %14s %8s" % ("frames", "batch", "ms per batch", "us per frame", "input GB/s", "of HBM peak", "stored")]
        for name, batch in (("512x512", frames512[:32]), ("1080x1920", wide)):
            n, H, W, C = batch.shape
            sr = png.default_strip_rows(W, C)
            bound = png.bound_bytes(n, H, W, C, sr)
            out = torch.empty(bound, dtype=torch.uint8, device=dev)
            meta = torch.zeros(n + 2, dtype=torch.int64, device=dev)
            ws = torch.empty(int(_lib.call("ia_png_workspace_bytes", n, H, W, C, sr)), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def call():
                _lib.call("ia_png_encode", batch, n, H, W, C, 1, sr, out, bound, meta, meta[n + 1:].view(torch.int32), None, ws, ws.numel())
            ms = []
            with torch.cuda.stream(side):
                for _ in range(5):
                    call()
                side.synchronize()
                for _ in range(args.repeat):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(side)
                    call()
                    e1.record(side)
                    side.synchronize()
                    ms.append(e0.elapsed_time(e1))
            med = float(np.median(ms))
            gbs = batch.numel() / (med * 1e-3) / 1e9
            m = meta.cpu()
            lines.append("%12s %6d %10.3f (%6.3f .. %6.3f) %12.1f %16.1f %13.2f%% %8d" % (
                name, n, med, min(ms), max(ms), med * 1e3 / n, gbs, 100.0 * gbs / HBM_PEAK_GBS, int(m[n + 1:].view(torch.int32)[0])))
            lines.append("%12s compressed: %d bytes of %d (%.2f %%); %d strips" % ("", int(m[n]), batch.numel(), 100.0 * int(m[n]) / batch.numel(),
                                                                                 n * int(_lib.call("ia_png_strips", H, W, C, sr))))
        lines.append("input GB/s = the pixels a call reads once (n H W 4 bytes) over the median; HBM peak taken as %.0f GB/s" % HBM_PEAK_GBS)

    if "b" in args.parts:
        fr = frames512[:args.frames]
        host = png.encode(fr, swap_rb=True).to_host()
        gpu_total = sum(len(host.png_bytes(i)) for i in range(len(host)))
        arrays = fr.cpu().numpy()
        pil_total = 0
        for i, f in enumerate(arrays):
            buf = io.BytesIO()
            rgba = animate._bgra_to_rgba(f)
            Image.fromarray(rgba, "RGBA").save(buf, format="PNG")
            pil_total += len(buf.getvalue())
            if i % 37 == 0 and not np.array_equal(np.asarray(Image.open(io.BytesIO(host.png_bytes(i)))), rgba):
                raise SystemExit("time_png: frame %d of the GPU route does not decode to its pixels" % i)
        lines.append("(b) %d frames of 512x512: GPU route %d bytes, PIL default save %d bytes: ratio %.4f (stored strips: %d)"
                     % (len(host), gpu_total, pil_total, gpu_total / float(pil_total), host.n_stored))

    if "c" in args.parts:
        import statistics
        seq = animate.AnimateSequence(poses[:args.frames], trans[:args.frames], np.zeros(10, np.float32), dev, size=512)
        routes = (("PIL, 8 workers, no GIF", dict(gif=None)), ("--gpu-png, no GIF", dict(gif=None, gpu_png=True)),
                  ("PIL, 8 workers, with its GIF", dict(gif="animation.gif")), ("--gpu-png --apng, no GIF", dict(gif=None, gpu_png=True, apng="animation.png")))
        times = {name: [] for name, _ in routes}
        sizes = {}
        for trip in range(3):
            for name, kw in routes:
                d = tempfile.mkdtemp(prefix="time_png_")
                try:
                    res = animate.render_sequence(model, seq, d, jitter=jitter, log=None, **kw)
                    times[name].append(res["write_s"])
                    sizes[name] = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))
                finally:
                    shutil.rmtree(d, ignore_errors=True)
        lines += ["(c) write phase of drivers.animate.render_sequence, %d frames of 512x512 (`write_s`: encoding and writing the files into a "
                  "temporary directory; the routes alternate, three trips in one process; %d CPUs usable)" % (args.frames, len(os.sched_getaffinity(0))),
                  "%34s %10s %22s %14s" % ("route", "median s", "min .. max s", "bytes written")]
        for name, _ in routes:
            t = times[name]
            lines.append("%34s %10.3f %10.3f .. %8.3f %14d" % (name, statistics.median(t), min(t), max(t), sizes[name]))
        for a, b in ((routes[0][0], routes[1][0]), (routes[2][0], routes[3][0])):
            outside = max(times[b]) < min(times[a])
            lines.append("%s against %s: %s" % (b, a, "every GPU trip is faster than every PIL trip (outside the spread), %.1fx by the medians"
                                                % (statistics.median(times[a]) / statistics.median(times[b])) if outside
                                                else "NOT outside the spread on the fast side"))
        lines.append("(on the PIL route the copies of raw pixels to the host run behind the frames and are part of the render loop, not of write_s)")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
