"""GPU time of the rigged export (csrc/ia_rig.hip) on the synthetic model's mesh and the first --frames frames of the `aist` track:
the three entry points alone, per number of influences, on the simplified mesh of profiles/texture_timing.txt and on the unsimplified
one; what `ia_rig_skin` writes per second next to the HBM peak profiles/overlay_timing.txt measured; for comparison the per-frame
route, --frames x `AvatarModel.pose_mesh`; and how far a rig of 4, 8 and 24 influences is from that route.  HIP events, the median of
`--repeat` runs after one warm-up.

    python tools/time_rig.py --resolution 256 --simplify 4 --frames 200 --out profiles/rig_timing.txt"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 6.29e12          # bytes per second, measured: profiles/overlay_timing.txt


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--simplify", type=float, default=4.0, help="cell edge in lattice spacings")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--influences", type=int, nargs="+", default=[4, 8, 24])
    ap.add_argument("--track", default=os.path.join(ROOT, "tests", "golden", "aist_demo_200.npz"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, mesh as M, rig
    from instantavatar_amd.pipeline import build_synthetic_model, make_batch
    dev = "cuda:0"
    model, _, _ = build_synthetic_model(dev)
    z = np.load(args.track)
    F = min(args.frames, len(z["poses"]))
    poses, trans = z["poses"][:F, :72].astype(np.float32), z["trans"][:F].astype(np.float32)
    poses_d, trans_d = torch.as_tensor(poses, device=dev), torch.as_tensor(trans, device=dev)

    def timed(fn):
        ms = []
        for r in range(args.repeat + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r:
                ms.append(a.elapsed_time(b))
        return statistics.median(ms)

    full = model.extract_mesh(resolution=args.resolution)
    lo, hi = M.field_box(model.net_coarse)
    spacing = float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / (args.resolution - 1)
    small = model.simplify_mesh(full, args.simplify * spacing)
    d, fd = model.deformer, model.deformer.deformer
    bones, quat, root = rig.track(d, poses_d, trans_d)
    t_track = timed(lambda: _lib.call("ia_rig_track", d._joints_rest, d._parents32, poses_d, trans_d, d.tfs_inv_t, F, bones, quat, root))
    batches = [make_batch(dev, 8, poses[f], trans[f]) for f in range(F)]
    lines = ["rigged export on the synthetic model's mesh (%s): GPU time in ms between HIP events, median of %d after a warm-up" % (torch.cuda.get_device_name(0), args.repeat),
             "%d frames of %s; ia_rig_track (bones, quaternions and root translations of all frames, one launch): %.3f ms" % (F, os.path.basename(args.track), t_track),
             "",
             "%-12s %9s %3s %12s %12s %10s %8s %14s %12s %12s" % ("mesh", "vertices", "K", "weights ms", "skin ms", "GB/s", "of HBM", "pose_mesh ms", "max dev", "mean dev")]
    for name, m in (("simplified", small), ("full", full)):
        n = m.verts.shape[0]
        t_pose = timed(lambda: [model.pose_mesh(m, b) for b in batches])
        want = torch.stack([model.pose_mesh(m, b).verts for b in batches])
        for K in args.influences:
            j, w = torch.empty((n, K), dtype=torch.uint8, device=dev), torch.empty((n, K), device=dev)
            t_w = timed(lambda: _lib.call("ia_rig_weights", m.verts, n, fd.lbs_voxel_channel_last(), 1, fd.grid_desc(), K, j, w, None))
            r = rig.Rig(j, w, None, None, None, None)
            xv, xn = torch.empty((F, n, 3), device=dev), torch.empty((F, n, 3), device=dev)
            t_s = timed(lambda: _lib.call("ia_rig_skin", m.verts, m.normals, n, j, w, K, bones, F, xv, xn))
            written = 24.0 * F * n
            mx, mean = rig.deviation(xv, want)
            lines.append("%-12s %9d %3d %12.3f %12.3f %10.1f %7.1f%% %14.3f %12.3e %12.3e" % (
                name, n, K, t_w, t_s, written / (t_s * 1e-3) / 1e9, 100.0 * written / (t_s * 1e-3) / HBM_PEAK, t_pose, float(mx.max()), float(mean.mean())))
            del xv, xn, r
        del want
        torch.cuda.empty_cache()
    lines += ["",
              "weights      = ia_rig_weights on the mesh's vertices from the channel-last weight volume (K joints and weights per vertex)",
              "skin         = ia_rig_skin: positions and normals of all %d frames in one launch; GB/s = the 24 bytes it writes per vertex and frame over that" % F,
              "               time, of HBM = that rate as a share of the measured peak of %.2f TB/s (profiles/overlay_timing.txt)" % (HBM_PEAK / 1e12),
              "pose_mesh    = the per-frame route: %d x AvatarModel.pose_mesh (ia_smpl_tfs, the voxel pass, ia_forward_skin, the normals), Python included" % F,
              "max dev      = the largest distance over all frames and vertices between the rig's positions and pose_mesh's; mean dev = the mean distance",
              "Measured with tools/time_rig.py.  First figures: only the number of workgroups of ia_rig_skin was chosen by measurement (csrc/ia_rig.hip)."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
