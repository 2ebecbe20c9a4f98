"""GPU time of the soft-silhouette entries for one frame -- projection, render forward (alpha, loss, d_alpha), render backward,
projection backward, body-model backward -- and the wall time of one frame's 10 LBFGS steps (`SilhouetteRefiner.refine`), on a
`synthetic.make_mesh_body` tessellated to about SMPL's size (sides 16, rings 15: 6 776 vertices, 13 440 faces) at 540^2 and 1080^2,
sigma = 1e-4 and the reference's blur radius.  The camera is the one of `animate` (focal 2000 at 1080, the body 5 m away); the mask is
the silhouette of the true pose, quantised to bytes; the start is the true pose moved by 0.03 rad per joint and 2 cm.  Each kernel
figure is the median over `--repeat` windows of `--calls` calls between two device events, after a warm-up window; the LBFGS figure is
the median of `--repeat` runs of a host clock around `refine`, which ends in host reads of the loss.  There is no earlier implementation
to compare with.

    python tools/time_silhouette.py --out profiles/silhouette_timing.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[540, 1080])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, synthetic
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.raster import Camera
    from instantavatar_amd.silhouette import SilhouetteRefiner
    if not torch.cuda.is_available():
        raise SystemExit("time_silhouette: no GPU; the figures are GPU times and are not estimated on a CPU")
    dev = torch.device("cuda:0")
    body = SMPL.from_dict(synthetic.make_mesh_body(sides=16, rings=15)).to(dev)
    V, nf = int(body.v_template.shape[0]), int(body.faces_tensor.shape[0])
    pose_np, transl_np = synthetic.procedural_pose_track(8)
    rs = np.random.RandomState(0)
    betas = torch.zeros(10, device=dev)
    pose_true, transl_true = torch.tensor(pose_np[3:4], device=dev), torch.tensor(transl_np[3:4], device=dev)
    pose0 = pose_true + 0.03 * torch.tensor(rs.randn(1, 72), dtype=torch.float32, device=dev)
    transl0 = transl_true + 0.02 * torch.tensor(rs.randn(1, 3), dtype=torch.float32, device=dev)
    lines = ["the soft silhouette of one frame: %d vertices, %d faces (synthetic.make_mesh_body(16, 15)), sigma 1e-4, on %s" % (V, nf, torch.cuda.get_device_name(0)),
             "GPU time per call in us between two device events: median (min .. max) of %d windows of %d calls, after a warm-up window" % (args.repeat, args.calls)]

    def timed(fn):
        def window():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            b.synchronize()
            return 1e3 * a.elapsed_time(b) / args.calls
        window()
        t = [window() for _ in range(args.repeat)]
        return "%9.1f  (%.1f .. %.1f)" % (statistics.median(t), min(t), max(t))

    for S in args.sizes:
        f = 2000.0 * S / 1080
        cam = Camera(np.array([[f, 0, S / 2], [0, f, S / 2], [0, 0, 1.0]]), torch.eye(4, device=dev), S, S)
        r = SilhouetteRefiner(body, body.faces_tensor, cam, torch.zeros((1, S, S), device=dev))
        sil = r.sil
        target = sil.render(r._posed(betas, pose_true[0].contiguous(), transl_true[0].contiguous()))
        r.masks = (torch.round(target * 255) / 255)[None].contiguous()
        b, p, t = betas, pose0[0].contiguous(), transl0[0].contiguous()
        v = r._posed(b, p, t).clone()
        screen, inv_z = sil.project(v)
        alpha, loss, d_alpha = sil._render(screen, inv_z, r.masks[0])
        d_screen, d_verts, g = torch.empty_like(screen), torch.empty_like(v), torch.empty(75, device=dev)
        ws = sil._ws
        common = (screen, inv_z, V, sil.faces, nf, S, S, sil.sigma, sil.blur_radius)
        entries = [
            ("ia_sil_project_fwd", lambda: _lib.call("ia_sil_project_fwd", v, V, *sil._cam(), screen, inv_z)),
            ("ia_sil_render_fwd", lambda: _lib.call("ia_sil_render_fwd", *common, r.masks[0], alpha, loss, d_alpha, ws, ws.numel())),
            ("ia_sil_render_bwd", lambda: _lib.call("ia_sil_render_bwd", *common, alpha, d_alpha, sil._vf[0], sil._vf[1], d_screen, ws, ws.numel())),
            ("ia_sil_project_bwd", lambda: _lib.call("ia_sil_project_bwd", v, V, *sil._cam(), d_screen, d_verts)),
            ("ia_sil_body_bwd", lambda: _lib.call("ia_sil_body_bwd", r.body, b, p, t, 1, d_verts, None, g[:72], g[72:], r._ws, r._ws.numel())),
        ]
        covered = float((target >= 0.5).float().mean())
        lines.append("%d x %d (the body covers %.1f %% of the image; start loss %.3e)" % (S, S, 100 * covered, float(loss)))
        for name, fn in entries:
            lines.append("  %-22s %s" % (name, timed(fn)))
        walls, last = [], None
        for _ in range(args.repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, _, last = r.refine(betas, pose0, transl0, iters=args.iters)
            torch.cuda.synchronize()
            walls.append(1e3 * (time.perf_counter() - t0))
        walls = walls[1:]
        lines.append("  %-22s %9.1f ms wall  (%.1f .. %.1f) of %d runs after one warm-up run; loss %.3e -> %.3e"
                     % ("%d LBFGS steps" % args.iters, statistics.median(walls), min(walls), max(walls), args.repeat, float(last[0, 0]), float(last[0, 1])))
    lines.append("each LBFGS closure evaluation is ia_kp_loss_fwd (the posed vertices), the five entries above and the host read of the loss that torch.optim.LBFGS makes")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
