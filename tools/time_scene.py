"""GPU time of the scene composition (csrc/ia_scene.hip) on the synthetic model: the three kernels at --size^2 for K = 1, 2, 4 layers
with shadow maps of --shadow-size^2 (inputs: real renders of the model, every layer the same frame at another offset in depth), and
the wall time of a whole `Scene.render` (camera render + light render per avatar + composition) next to K plain
`render_image_fast` calls on the same models in the same run -- `render_image_fast` is the yardstick.  Kernels: HIP events around
--inner launches, the median of --repeat runs after a warm-up; whole frames: wall time with a synchronisation, median of --repeat.

    python tools/time_scene.py --size 512 --shadow-size 256 --out profiles/scene_timing.txt"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--shadow-size", type=int, default=256)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frame-gpu-ms", type=float, default=2.16, help="GPU time of one avatar's 512^2 frame (README) the kernels are set against")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, scene, synthetic
    from instantavatar_amd.drivers import animate
    from instantavatar_amd.pipeline import build_synthetic_model
    dev = torch.device("cuda:0")
    Kmax = max(args.layers)
    model, _, _ = build_synthetic_model(dev)
    model.eval()
    poses, trans = synthetic.procedural_pose_track(64)
    offsets = [((k - (Kmax - 1) / 2.0) * 0.9, 0.0, 0.0) for k in range(Kmax)]
    seqs = [scene.place(animate.AnimateSequence(poses[:8], trans[:8], np.zeros(10, np.float32), dev, size=args.size), o) for o in offsets]
    jitter = animate.fixed_jitter(1, dev)
    H = W = args.size
    R, S = H * W, args.shadow_size
    light = (-2.0, -4.0, 2.0)

    def gpu_ms(fn):
        ms = []
        for r in range(args.repeat + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            if r:
                ms.append(a.elapsed_time(b) / args.inner)
        return statistics.median(ms)

    def wall_ms(fn):
        ms = []
        for r in range(args.repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms)

    lines = ["scene composition on the synthetic model (%s): frames of %d x %d, shadow maps of %d x %d, PCF radius %d"
             % (torch.cuda.get_device_name(0), W, H, S, S, args.radius),
             "kernels: GPU time in ms between HIP events around %d launches, median of %d after a warm-up; frames: wall ms, median of %d"
             % (args.inner, args.repeat, args.repeat),
             "%3s %10s %10s %10s %10s %9s %12s | %12s %14s %8s" % ("K", "ground", "shadow", "composite", "sum", "GB/s", "of a frame", "Scene.render", "K x fast render", "ratio")]
    worst = 0.0
    for K in args.layers:
        ground = scene.ground_under([model] * K, seqs[:K], color2=(0.4, 0.4, 0.4), cell=0.5)
        sc = scene.Scene([model] * K, seqs[:K], ground=ground, light=light, shadow_size=S, shadow_radius=args.radius, jitter=jitter)
        # the inputs of the three kernels, from a real frame
        layers, maps, projs = [], [], []
        for k in range(K):
            batch = seqs[k].batch(1)
            batch["rays_o"], batch["rays_d"], batch["bg_color"] = seqs[0].rays_o, seqs[0].rays_d, sc._zero_bg
            rgb, depth, alpha, _ = model.render_image_fast(batch, (H, W), jitter=jitter)
            layers.append((rgb[0].reshape(R, 3), alpha[0].reshape(R), depth[0].reshape(R)))
            m, cam = sc.light_view(k, 1, batch)
            maps.append(m)
            projs.append(scene.light_rays_projection(cam))
        c = torch.stack([l[0] for l in layers]).contiguous()
        a = torch.stack([l[1] for l in layers]).contiguous()
        d = torch.stack([l[2] for l in layers]).contiguous()
        maps, proj = torch.stack(maps).contiguous(), torch.as_tensor(np.stack(projs), device=dev)
        o, dr = seqs[0].rays_o.reshape(R, 3).contiguous(), seqs[0].rays_d.reshape(R, 3).contiguous()
        t_g, a_g, shade = torch.empty(R, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
        c_g, P, out_rgb = torch.empty((R, 3), device=dev), torch.empty((R, 3), device=dev), torch.empty((R, 3), device=dev)
        out_a, out_d = torch.empty(R, device=dev), torch.empty(R, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        g = ground
        f_ground = lambda: _lib.call("ia_scene_ground", o, dr, R, *g.normal, g.offset, *g.color, *g.color2, g.cell, *g.centre, g.r0, g.r1, t_g, a_g, c_g, P)
        f_shadow = lambda: _lib.call("ia_scene_shadow", P, a_g, R, maps, proj, K, S, args.radius, 0.6, 0.05, shade)
        f_comp = lambda: _lib.call("ia_scene_composite", c, a, d, K, R, t_g, a_g, c_g, shade, None, 0, 0.3, out_rgb, out_a, out_d, counter)
        tg, ts, tc = gpu_ms(f_ground), gpu_ms(f_shadow), gpu_ms(f_comp)
        total = tg + ts + tc
        moved = R * (20 * K + 40 + 24 + 32 + 20)      # composite: 20 K + 40 bytes per pixel; ground: 24 in, 32 out; shadow: 16 in, 4 out
        worst = max(worst, total / args.frame_gpu_ms)
        t_scene = wall_ms(lambda: sc.render(1))

        def plain():
            for k in range(K):
                model.render_image_fast(seqs[k].batch(1), (H, W), jitter=jitter)
        t_plain = wall_ms(plain)
        lines.append("%3d %10.4f %10.4f %10.4f %10.4f %9.0f %11.1f%% | %12.2f %14.2f %8.2f"
                     % (K, tg, ts, tc, total, moved / total / 1e6, 100 * total / args.frame_gpu_ms, t_scene, t_plain, t_scene / t_plain))
    lines.append("of a frame: the three kernels against the %.2f ms of GPU time one avatar's 512^2 frame takes.  Scene.render holds, per avatar, the camera "
                 "render and a light render of %d^2 rays (with the host-side light camera and ray set-up), then the composition; the ratio is "
                 "against the camera renders alone." % (args.frame_gpu_ms, S))
    if worst > 0.1:
        lines.append("the kernels exceed a tenth of a frame: see the note below")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
