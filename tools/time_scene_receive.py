"""GPU time of `ia_scene_receive` (csrc/ia_scene.hip: the avatars of a scene receive shadows) on the synthetic model at --size^2 with
light-view maps of --shadow-size^2: K = 1, 2, 4 avatars side by side and behind one another (seen from the camera), PCF radius
0, 1, 3, with and without the normals of the facing term -- next to `ia_scene_composite` on the same layers, and the wall time of a
whole `Scene.render` with and without receive=True in the same run (the second is what the parent commit renders).  Inputs are real
renders of the model.  Kernels: HIP events around --inner launches, --repeat runs after a warm-up, median and min .. max; whole
frames: wall time with a synchronisation, median and min .. max of --repeat.

It also prints the evidence for or against the default self-bias: for one avatar lit from the front, the share of the pixels with
alpha >= 0.5 that face the light (cosv > cos1) and nevertheless get a shade below 0.99, i.e. shadow themselves, for bias_self =
0.02, 0.05 and 0.10 m; and the kernel's register, scratch and LDS use as the compiler reports it.

    python tools/time_scene_receive.py --size 512 --shadow-size 256 --out profiles/scene_receive_timing.txt"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def resource_usage():
    """the compiler's resource-usage remarks for k_scene_receive (one compile of ia_scene.hip to nowhere), or why there are none"""
    from instantavatar_amd import build
    src = os.path.join(build.CSRC, "ia_scene.hip")
    cmd = [build.HIPCC] + build.FLAGS + build.extra_flags(src) + [build.cuid_flag(src), "-x", "hip", "-c", src, "-o", os.devnull,
                                                                   "-Rpass-analysis=kernel-resource-usage"]
    try:
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return "k_scene_receive: resource usage not read (%s)" % e
    found, inside = {}, False
    for line in text.splitlines():
        m = re.search(r"remark: +(?:\S+:\d+:\d+: +)?(Function Name: (\S+)|([A-Za-z ]+(?:\[[^\]]+\])?): (\S+))", line)
        if not m:
            continue
        if m.group(2):
            inside = "k_scene_receive" in m.group(2)
        elif inside:
            found[m.group(3).strip()] = m.group(4)
    if not found:
        return "k_scene_receive: resource usage not read (no remarks from %s)" % build.HIPCC
    keys = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]
    return "k_scene_receive as compiled for gfx950: " + ", ".join("%s %s" % (k, found.get(k, "?")) for k in keys)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--shadow-size", type=int, default=256)
    ap.add_argument("--layers", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--radii", type=int, nargs="+", default=[0, 1, 3])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frame-gpu-ms", type=float, default=2.16, help="GPU time of one avatar's 512^2 frame (README) the kernel is set against")
    ap.add_argument("--no-resources", action="store_true", help="do not compile ia_scene.hip for the resource-usage line")
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
    jitter = animate.fixed_jitter(1, dev)
    H = W = args.size
    R, S = H * W, args.shadow_size
    light = (-2.0, -4.0, 2.0)

    def sequences(layout, K):
        if layout == "side by side":
            offsets = [((k - (K - 1) / 2.0) * 0.9, 0.0, 0.0) for k in range(K)]
        else:                                                   # behind one another: the layers overlap in the frame
            offsets = [(0.15 * k, 0.0, 0.9 * k) for k in range(K)]
        return [scene.place(animate.AnimateSequence(poses[:8], trans[:8], np.zeros(10, np.float32), dev, size=args.size), o) for o in offsets]

    def spread(ms):
        return "%8.4f (%.4f .. %.4f)" % (statistics.median(ms), min(ms), max(ms))

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
        return ms

    def wall_ms(fn):
        ms = []
        for r in range(args.repeat + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r:
                ms.append(1e3 * (time.perf_counter() - t0))
        return ms

    lines = ["ia_scene_receive on the synthetic model (%s): frames of %d x %d, light-view maps of %d x %d, light at %s"
             % (torch.cuda.get_device_name(0), W, H, S, S, light),
             "kernels: GPU ms between HIP events around %d launches, median (min .. max) of %d after a warm-up; frames: wall ms, median (min .. max) of %d"
             % (args.inner, args.repeat, args.repeat)]
    if not args.no_resources:
        lines.append(resource_usage())
    worst = 0.0
    for layout in ("side by side", "behind one another"):
        for K in args.layers:
            if K == 1 and layout != "side by side":
                continue
            seqs = sequences(layout, K)
            sc = scene.Scene([model] * K, seqs, light=light, shadow_size=S, jitter=jitter, receive=True)
            plain = scene.Scene([model] * K, seqs, light=light, shadow_size=S, jitter=jitter)
            # the kernel's inputs, from a real frame
            layers, nrms, maps_a, maps_d, projs = [], [], [], [], []
            for k in range(K):
                batch = seqs[k].batch(1)
                batch["rays_o"], batch["rays_d"], batch["bg_color"] = seqs[0].rays_o, seqs[0].rays_d, sc._zero_bg
                rgb, depth, alpha, _, nrm = model.render_image_fast(batch, (H, W), jitter=jitter, normals=True)
                layers.append((rgb[0].reshape(R, 3), alpha[0].reshape(R), depth[0].reshape(R)))
                nrms.append(nrm[0].reshape(R, 3))
                m, s, cam = sc.light_view_maps(k, 1, batch)
                maps_a.append(m)
                maps_d.append(s)
                projs.append(scene.light_rays_projection(cam))
            c = torch.stack([l[0] for l in layers]).contiguous()
            a = torch.stack([l[1] for l in layers]).contiguous()
            d = torch.stack([l[2] for l in layers]).contiguous()
            nrm = torch.stack(nrms).contiguous()
            maps_a, maps_d, proj = torch.stack(maps_a).contiguous(), torch.stack(maps_d).contiguous(), torch.as_tensor(np.stack(projs), device=dev)
            o, dr = seqs[0].rays_o.reshape(R, 3).contiguous(), seqs[0].rays_d.reshape(R, 3).contiguous()
            c_out, shade = torch.empty((K, R, 3), device=dev), torch.empty((K, R), device=dev)
            out_rgb, out_a, out_d = torch.empty((R, 3), device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
            counter = torch.zeros(1, dtype=torch.int32, device=dev)
            covered = float((a > 0).any(0).float().mean())
            lines.append("")
            lines.append("K = %d, %s: %.1f %% of the pixels have a layer with a > 0" % (K, layout, 100 * covered))
            t_comp = gpu_ms(lambda: _lib.call("ia_scene_composite", c, a, d, K, R, None, None, None, None, None, 0, 0.3, out_rgb, out_a, out_d, counter))
            lines.append("  %-34s %s ms" % ("ia_scene_composite", spread(t_comp)))
            for radius in args.radii:
                for with_n in (True, False):
                    f = lambda: _lib.call("ia_scene_receive", o, dr, R, c, a, d, nrm if with_n else None, maps_a, maps_d, proj, K, S, *light, radius,
                                          0.6, 0.05, 0.02, 0.05, 0.0, 0.25, c_out, shade)
                    t = gpu_ms(f)
                    worst = max(worst, statistics.median(t) / args.frame_gpu_ms)
                    lines.append("  %-34s %s ms = %.2f %% of a frame" % ("ia_scene_receive r = %d, %s" % (radius, "normals" if with_n else "no normals"),
                                                                          spread(t), 100 * statistics.median(t) / args.frame_gpu_ms))
            t_with, t_without = wall_ms(lambda: sc.render(1)), wall_ms(lambda: plain.render(1))
            ground = scene.ground_under([model] * K, seqs, color2=(0.4, 0.4, 0.4), cell=0.5)
            g_with = scene.Scene([model] * K, seqs, ground=ground, light=light, shadow_size=S, jitter=jitter, receive=True)
            g_without = scene.Scene([model] * K, seqs, ground=ground, light=light, shadow_size=S, jitter=jitter)
            t_gwith, t_gwithout = wall_ms(lambda: g_with.render(1)), wall_ms(lambda: g_without.render(1))
            lines.append("  %-34s %s ms" % ("Scene.render, light, no ground", spread(t_without)))
            lines.append("  %-34s %s ms   (light renders, normal passes, receive)" % ("  the same with receive=True", spread(t_with)))
            lines.append("  %-34s %s ms   (what the parent commit renders)" % ("Scene.render, light and ground", spread(t_gwithout)))
            lines.append("  %-34s %s ms   (ratio %.2f: the normal pass per avatar and one launch)"
                         % ("  the same with receive=True", spread(t_gwith), statistics.median(t_gwith) / statistics.median(t_gwithout)))
    lines.append("")
    lines.append("of a frame: against the %.2f ms of GPU time one avatar's 512^2 frame takes.  Without a ground a scene without receive renders no "
                 "light views at all, so the first pair of frame times holds them; the second pair is the cost of the option itself." % args.frame_gpu_ms)
    if worst > 0.1:
        lines.append("the kernel exceeds a tenth of a frame in at least one row")

    # the self-shadow fraction of one avatar lit from the front
    seq = animate.AnimateSequence(poses[:8], trans[:8], np.zeros(10, np.float32), dev, size=args.size)
    root = seq.transl[1].double().cpu().numpy()
    front = root + np.array([-0.3, -0.5, -2.0])
    lines.append("")
    lines.append("self-shadowing of one avatar lit from the front (light at root + (-0.3, -0.5, -2.0), PCF radius 1, maps of %d^2): of the pixels with "
                 "alpha >= 0.5 that face the light (cosv > 0.25), the share with a shade below 0.99" % S)
    for bias_self in (0.02, 0.05, 0.10):
        sc = scene.Scene([model], [seq], light=front, shadow_size=S, jitter=jitter, receive=True, bias_self=bias_self)
        out = sc.render(1)
        batch = seq.batch(1)
        batch["bg_color"] = sc._zero_bg
        rgb, depth, alpha, _, nrm = model.render_image_fast(batch, (H, W), jitter=jitter, normals=True)
        X = seq.rays_o.reshape(R, 3) + (depth.reshape(R, 1) / alpha.reshape(R, 1)) * seq.rays_d.reshape(R, 3)
        l = torch.as_tensor(front, dtype=torch.float32, device=dev)[None] - X
        cosv = (nrm.reshape(R, 3) * l).sum(1) / l.norm(dim=1)
        lit = (alpha.reshape(R) >= 0.5) & (cosv > 0.25)
        dark = lit & (out["layer_shade"].reshape(R) < 0.99)
        n_lit, n_dark = int(lit.sum()), int(dark.sum())
        lines.append("  bias_self = %.2f m: %6.2f %% of %d pixels" % (bias_self, 100.0 * n_dark / max(1, n_lit), n_lit))
    lines.append("where no limb stands between such a pixel and the light, a shade below 0.99 is the bias failing (acne); a share that stops falling "
                 "as the bias grows is real self-shadowing (an arm in front of the trunk).")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
