"""GPU time of `ia_mask_clean` on batches of raw masks, and the host time of the same step in numpy / scipy.

    python tools/time_masks.py --out profiles/mask_clean_timing.txt [--sizes 540x960:32 1080x1920:16 1080x1920:64] [--repeat 30]

The masks are the synthetic mesh body's rasterised silhouette (tests/mask_refs.body_silhouette) with seeded speckles, pinholes and a
detached blob (mask_refs.degrade), a different seed per frame.  GPU times are device events around ONE call (a whole batch) on a side
stream, `--repeat` calls after a warm-up of five: median, minimum and maximum.  Before timing the batch's masks are compared for
equality with the host restatement on the frames that are timed there.  The host baseline is the only one there is: the step did not
exist before, and cv2 is not a dependency.  It is tests/mask_refs.clean (pure numpy, labelling by minimum propagation: slow by
construction) on one frame of the smallest size, and the same definition through scipy.ndimage (binary_erosion / binary_dilation /
label, `host_scipy` below) where scipy is installed."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_scipy(ndi, src, k=5):
    """mask_refs.clean's `masks` through scipy.ndimage: threshold 0, k x k open and close, 8-connected, largest, tie to the first"""
    import numpy as np
    box = np.ones((k, k), bool)
    b = src > 0
    b = ndi.binary_dilation(ndi.binary_erosion(b, box, border_value=1), box)
    b = ndi.binary_erosion(ndi.binary_dilation(b, box), box, border_value=1)
    lab, n = ndi.label(b, np.ones((3, 3), bool))           # scipy labels in raster order of the first pixel: argmax = the tie rule
    if n == 0:
        return np.zeros(src.shape, np.uint8)
    return np.where(lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:])), 255, 0).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", nargs="+", default=["540x960:32", "1080x1920:16", "1080x1920:64"], help="HxW:frames per batch")
    ap.add_argument("--repeat", type=int, default=30)
    ap.add_argument("--host-frames", type=int, default=2, help="frames per size timed through scipy (0: no host timing at all)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import mask_refs as mr
    from instantavatar_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("time_masks: no GPU; a time measured elsewhere says nothing about it")
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(dev)
    lines = ["ia_mask_clean on batches of raw masks (%s): threshold 0, 5 x 5 open and close, 8-connected, keep the largest" % torch.cuda.get_device_name(0),
             "raw mask = rasterised synthetic mesh body + seeded speckles, pinholes and a detached blob, one seed per frame",
             "GPU: device events around one call (the whole batch, 10 launches) on a side stream; median (min .. max) of %d calls after 5 warm-up calls" % args.repeat,
             "%12s %7s %26s %12s %10s   %s" % ("frames", "batch", "ms per batch", "us per frame", "GB/s", "outputs")]
    host = []
    for spec in args.sizes:
        hw, n = spec.split(":")
        H, W = (int(v) for v in hw.split("x"))
        n = int(n)
        sil = mr.body_silhouette(H, W, dev)
        scale = H * W / (270 * 480)
        raws = np.stack([mr.degrade(sil, 100 + i, int(400 * scale), int(300 * scale))[0] for i in range(n)])
        src = torch.as_tensor(raws).to(dev)
        nb = int(_lib.call("ia_mask_clean_workspace_bytes", n, H, W))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        masks, binary = torch.empty_like(src), torch.empty_like(src)
        labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
        area, nc = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        variants = (("masks", None, None, 2), ("masks + binary + labels", binary, labels, 7))
        for name, b, l, bytes_px in variants:
            def call():
                _lib.call("ia_mask_clean", src, n, H, W, 0, 5, 8, masks, b, l, area, nc, ws, nb)
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
            lines.append("%12s %7d %10.3f (%6.3f .. %6.3f) %12.1f %10.1f   %s" % (
                "%dx%d" % (H, W), n, med, min(ms), max(ms), med * 1e3 / n, bytes_px * n * H * W / (med * 1e-3) / 1e9, name))
        got = masks.cpu().numpy()
        kept = area.cpu().numpy()
        # the host side: scipy on the first frames of every size, numpy on one frame of the smallest
        if ndi is not None and args.host_frames > 0:
            t = []
            for i in range(min(args.host_frames, n)):
                t0 = time.perf_counter()
                m = host_scipy(ndi, raws[i])
                t.append(time.perf_counter() - t0)
                if not np.array_equal(m, got[i]):
                    raise SystemExit("time_masks: frame %d of %dx%d differs from the scipy restatement" % (i, H, W))
            host.append("%12s %7d %10.1f ms per frame (min of %d frames), scipy.ndimage %s; masks equal the GPU's" % ("%dx%d" % (H, W), 1, min(t) * 1e3, len(t), __import__("scipy").__version__))
        if spec == args.sizes[0] and args.host_frames > 0:
            t0 = time.perf_counter()
            r = mr.clean(raws[0])
            dt = time.perf_counter() - t0
            if not np.array_equal(r["masks"], got[0]) or r["area"] != kept[0]:
                raise SystemExit("time_masks: frame 0 of %dx%d differs from tests/mask_refs.clean" % (H, W))
            host.append("%12s %7d %10.1f ms for one frame, tests/mask_refs.clean (numpy); masks equal the GPU's" % ("%dx%d" % (H, W), 1, dt * 1e3))
        lines.append("%12s kept component: %d .. %d pixels of %d" % ("", kept.min(), kept.max(), H * W))
    lines += ["GB/s = the bytes a call must move (src read, outputs written: 2 or 7 bytes per pixel) over the median; not a kernel's share of peak",
              "host (%d CPUs visible, one used):" % (os.cpu_count() or 1)] + host
    if ndi is None:
        lines.append("%12s scipy is not installed here: no scipy figure" % "")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
