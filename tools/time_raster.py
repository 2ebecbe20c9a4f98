"""GPU time of the rasteriser's three entry points on the synthetic model's mesh, and the silhouette IoU of the raster mask
against the volumetric frame (`alpha >= 0.5` of `render_image_fast`) under the same camera.

    python tools/time_raster.py --resolution 256 --sizes 512 1024 --frames 0 100 199 --out profiles/raster_timing.txt

Times are device events around `--calls` back-to-back calls of one entry point (after a warm-up of the same shape), divided by
the number of calls; median of `--repeat` such windows.  The mesh is posed into frame --frames[0] of the aist track
(tests/golden/aist_demo_200.npz) under the animate driver's camera scaled to the image size."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--frames", type=int, nargs="+", default=[0, 100, 199])
    ap.add_argument("--iou-size", type=int, default=512)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib
    from instantavatar_amd.drivers.animate import AnimateSequence
    from instantavatar_amd.pipeline import build_synthetic_model
    dev = torch.device("cuda:0")
    model, _, _ = build_synthetic_model(dev)
    model.eval()
    z = np.load(os.path.join(ROOT, "tests", "golden", "aist_demo_200.npz"))
    poses, trans = z["poses"].astype(np.float32), z["trans"].astype(np.float32)
    betas = np.zeros(10, np.float32)
    mesh = model.extract_mesh(resolution=args.resolution)
    nv, nf = mesh.verts.shape[0], mesh.faces.shape[0]
    lines = ["rasteriser on the synthetic model's mesh (%s): lattice %d, %d vertices, %d faces, posed into frame %d of the aist track"
             % (torch.cuda.get_device_name(0), args.resolution, nv, nf, args.frames[0]),
             "GPU time per call in us: device events around %d back-to-back calls, median of %d windows after a warm-up" % (args.calls, args.repeat),
             "%10s %10s %10s %10s %12s %12s %12s %12s" % ("image", "covered", "skipped", "queued", "project", "visibility", "resolve C=6", "resolve C=0")]

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / args.calls)
        return float(np.median(out))

    for size in args.sizes:
        seq = AnimateSequence(poses, trans, betas, dev, size=size)
        cam = seq.camera()
        posed = model.pose_mesh(mesh, seq.batch(args.frames[0], rays=False))
        verts, faces = posed.verts.contiguous(), posed.faces.contiguous()
        attrs = torch.cat([posed.colors, posed.normals], 1).contiguous()
        H, W = cam.H, cam.W
        nb = int(_lib.call("ia_raster_workspace_bytes", nv, nf, H, W))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        xy, inv_z = torch.empty((nv, 2), dtype=torch.int32, device=dev), torch.empty(nv, device=dev)
        vis = torch.empty(H * W, dtype=torch.int64, device=dev)
        face_id, depth = torch.empty(H * W, dtype=torch.int32, device=dev), torch.empty(H * W, device=dev)
        out, counts = torch.empty((H * W, 6), device=dev), torch.empty(2, dtype=torch.int32, device=dev)
        project = lambda: _lib.call("ia_raster_project", verts, nv, cam.w2c, cam.fx, cam.fy, cam.cx, cam.cy, cam.near, xy, inv_z)
        visibility = lambda: _lib.call("ia_raster_visibility", xy, inv_z, nv, faces, nf, H, W, 1, vis, ws, nb)
        resolve6 = lambda: _lib.call("ia_raster_resolve", xy, inv_z, nv, faces, nf, vis, H, W, attrs, 6, ws, nb, face_id, depth, out, counts)
        resolve0 = lambda: _lib.call("ia_raster_resolve", xy, inv_z, nv, faces, nf, vis, H, W, None, 0, ws, nb, face_id, depth, None, counts)
        t = [timed(f) for f in (project, visibility, resolve6, resolve0)]
        queued = int(ws[:4].view(torch.int32)[0])
        skipped, covered = counts.tolist()
        lines.append("%10s %10d %10d %10d %12.1f %12.1f %12.1f %12.1f" % ("%dx%d" % (W, H), covered, skipped, queued, *t))
    lines += ["covered = pixels with a fragment; skipped = faces culled, degenerate after snapping or with an invalid vertex (cull on);",
              "queued = faces whose clipped box holds more than 16 samples (drained by one wave each)", ""]

    size = args.iou_size
    seq = AnimateSequence(poses, trans, betas, dev, size=size)
    cam = seq.camera()
    lines.append("silhouette IoU at %dx%d: raster mask of the posed lattice-%d mesh against alpha >= 0.5 of render_image_fast, same batch" % (size, size, args.resolution))
    lines.append("%10s %12s %12s %12s %10s" % ("frame", "raster px", "volume px", "both", "IoU"))
    for i in args.frames:
        batch = seq.batch(i)
        alpha = model.render_image_fast(batch, (size, size))[2].reshape(size, size) >= 0.5
        mask = model.render_mesh(mesh, dict(seq.batch(i, rays=False), camera=cam))["mask"]
        both, either = int((alpha & mask).sum()), int((alpha | mask).sum())
        lines.append("%10d %12d %12d %12d %10.4f" % (i, int(mask.sum()), int(alpha.sum()), both, both / max(either, 1)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
