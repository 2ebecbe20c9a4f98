"""GPU time of the sequence-inspection kernels (csrc/ia_overlay.hip) and of `SequenceInspector.report` / `.overlay` per frame.

    python tools/time_overlay.py --out profiles/overlay_timing.txt [--frames 32] [--size 1080x1920] [--repeat 20]

The frames are seeded noise; the masks are the rasterised synthetic mesh body (sides 16, rings 15: about SMPL's size) at 32 poses of the
procedural track, the detections its own projections moved by seeded noise.  Kernel times are device events around ONE call (the whole
batch) on a side stream, `--repeat` calls after five warm-up calls: median, minimum and maximum.  Next to each stands the bytes the
algorithm must move and, for blend and stats -- the two that stream every pixel -- the share of the measured HBM peak (6.29 TB/s,
float4 copy) those bytes over the median give.  Outline and skeleton write only the pixels they draw, so their bytes are the reads
they cannot avoid and no share is given.  `report` and `overlay` are host clocks around a call that ends in a device synchronise:
they hold the body model, the rasteriser and the host's launch work, not these kernels alone."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 6.29e12      # bytes / s, measured (float4 copy)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", default="1080x1920", help="HxW")
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, overlay, synthetic
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.keypoints import SMPL_KP_VERTEX
    if not torch.cuda.is_available():
        raise SystemExit("time_overlay: no GPU; a time measured elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    H, W = (int(v) for v in args.size.split("x"))
    n = args.frames
    body = SMPL.from_dict(synthetic.make_mesh_body(sides=16, rings=15)).to(dev)
    kpv = tuple(v % int(body.v_template.shape[0]) for v in SMPL_KP_VERTEX)
    f = 2000.0 * H / 1080
    K = np.array([[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]])
    poses, tr = synthetic.procedural_pose_track(n)
    params = (torch.zeros(10, device=dev), torch.as_tensor(poses.astype(np.float32), device=dev), torch.as_tensor(tr.astype(np.float32), device=dev))
    g = torch.Generator(device=dev).manual_seed(0)
    # pass 1: the body's own silhouettes and projections, to build masks and detections from
    first = overlay.SequenceInspector(body, K, np.eye(4), H, W, keypoints=np.zeros((n, 25, 3), np.float32), kp_vertex=kpv)
    verts, uv = first._posed(*params)
    from instantavatar_amd.raster import rasterize
    frames = [rasterize(verts[i], first.faces, first.camera) for i in range(n)]
    masks = torch.stack([fr.mask for fr in frames]).to(torch.uint8) * 255
    masks = torch.roll(masks, 3, 2)                                      # three pixels off: an IoU below 1
    kp = torch.cat([uv + 2 * torch.randn(uv.shape, device=dev, generator=g), torch.rand((n, 25, 1), device=dev, generator=g)], -1)
    insp = overlay.SequenceInspector(body, K, np.eye(4), H, W, keypoints=kp, masks=masks, kp_vertex=kpv)
    images = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
    layer = torch.stack([overlay.face_shade(fr.face_id, verts[i], first.faces, first.camera.w2c) for i, fr in enumerate(frames)])
    sil = torch.stack([fr.mask for fr in frames])
    out = torch.empty_like(images)
    counts = torch.empty((n, 4), dtype=torch.int32, device=dev)
    nb = int(_lib.call("ia_overlay_stats_workspace_bytes", n, H, W))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    seg = torch.as_tensor(np.asarray(overlay.BODY25_SEGMENTS, np.int32), device=dev)
    col = torch.as_tensor(np.asarray(overlay.LIMB_COLOURS, np.uint8), device=dev)
    model = torch.cat([uv, torch.ones((n, 25, 1), device=dev)], -1).contiguous()
    fid0, v0, layer0 = frames[0].face_id, verts[0].contiguous(), torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    nv, nf = int(v0.shape[0]), int(first.faces.shape[0])
    px = n * H * W
    drawn = int((overlay.draw_skeleton(torch.zeros_like(images), kp, point_rgb=(255, 255, 255), radius_q=6) != 0).any(-1).sum())
    lined = int((overlay.outline(torch.zeros_like(images), masks) != 0).any(-1).sum())
    covered = int(sil[0].sum())
    kernels = (
        ("ia_overlay_blend", lambda: _lib.call("ia_overlay_blend", images, layer, n, H, W, 128, out), 10 * px, True,
         "10 B/pixel: 3 image + 4 layer read, 3 written"),
        ("ia_overlay_stats", lambda: _lib.call("ia_overlay_stats", masks, sil, n, H, W, counts, ws, nb), 2 * px, True, "2 B/pixel: both masks read"),
        ("ia_overlay_outline t = 2", lambda: _lib.call("ia_overlay_outline", masks, n, H, W, 2, 255, 255, 255, out), px + 3 * lined, False,
         "1 B/pixel read + 3 B per outline pixel (%d)" % lined),
        ("ia_overlay_skeleton 24 limbs", lambda: _lib.call("ia_overlay_skeleton", kp, n, 25, seg, col, 24, 255, 255, 255, 0.2, 6, 6, H, W, out),
         n * 25 * 12 + 3 * drawn, False, "the points + 3 B per drawn pixel (%d)" % drawn),
        ("ia_overlay_skeleton S = 0", lambda: _lib.call("ia_overlay_skeleton", model, n, 25, None, None, 0, 255, 255, 0, 0.5, 6, 8, H, W, out),
         n * 25 * 12, False, "the points + the discs' pixels"),
        ("ia_overlay_face_shade (1 frame)", lambda: _lib.call("ia_overlay_face_shade", fid0, H, W, v0, nv, first.faces, nf, first.camera.w2c, 90, 170, 255, layer0),
         8 * H * W + 48 * covered, False, "8 B/pixel + 48 B of face and vertices per covered pixel (%d), mostly cached" % covered),
    )
    side = torch.cuda.Stream(dev)
    lines = ["sequence inspection on %d frames of %dx%d (%s); body: synthetic mesh body, %d vertices, %d faces" % (n, H, W, torch.cuda.get_device_name(0), nv, nf),
             "kernels: device events around one call (the whole batch) on a side stream; median (min .. max) of %d calls after 5 warm-up calls" % args.repeat,
             "%-34s %26s %12s %10s %8s   %s" % ("entry", "ms per call", "us per frame", "GB/s", "of HBM", "algorithmic bytes")]
    torch.cuda.synchronize()
    for name, call, nbytes, streams, what in kernels:
        ms = []
        side.wait_stream(torch.cuda.current_stream(dev))
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
        rate = nbytes / (med * 1e-3)
        per = 1 if "1 frame" in name else n
        lines.append("%-34s %10.3f (%6.3f .. %6.3f) %12.1f %10.1f %8s   %s" % (
            name, med, min(ms), max(ms), med * 1e3 / per, rate / 1e9, "%.0f %%" % (100 * rate / HBM_PEAK) if streams else "-", what))
    lines.append("of HBM = algorithmic bytes over the median, as a share of the measured peak of %.2f TB/s; bound by bandwidth, not arithmetic" % (HBM_PEAK / 1e12))
    lines.append("(repeated calls on the same buffers: the %.0f MB of ia_overlay_stats fit the 256 MiB Infinity Cache and part of the %.0f MB of ia_overlay_blend stays "
                 "there, so a share can read above what HBM alone gives)" % (2 * px / 1e6, 10 * px / 1e6))
    for name, call in (("SequenceInspector.report", lambda: insp.report(*params)),
                       ("SequenceInspector.overlay (8 frames)", lambda: insp.overlay(images[:8], list(range(8)), *params))):
        for _ in range(2):
            call()
        torch.cuda.synchronize()
        t = []
        for _ in range(max(3, args.repeat // 4)):
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        per = 8 if "8 frames" in name else n
        lines.append("%-40s %9.2f ms per call (min %.2f), %8.1f us per frame: host clock, device synchronised; body model, rasteriser and launches included"
                     % (name, float(np.median(t)) * 1e3, min(t) * 1e3, float(np.median(t)) * 1e6 / per))
    rep = insp.report(*params)
    lines.append("the report of this sequence: IoU median %.4f, keypoint error median %.2f px" % (float(rep["iou"].median()), float(rep["kp_err_px"].median())))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
