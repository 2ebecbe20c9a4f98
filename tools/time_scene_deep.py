"""GPU time of `ia_scene_deep_composite` (csrc/ia_scene_deep.hip: exact scene compositing where avatars interleave along a ray) and what
`Scene(exact=True)` costs, on the synthetic model at --size^2:

  1. the merge kernel for K = 2 / 4 / 8 avatars on the REAL active sets and sample lists of two arrangements -- side by side (small
     overlap) and one behind the other (full overlap) -- as GPU ms between HIP events, and the bytes it reads per second against the
     HBM rate the project measured (profiles/overlay_timing.txt: 6.29 TB/s);
  2. wall time of `Scene.render` with two avatars, `exact` on and off in the same run, in both arrangements;
  3. the shares of overlap and interleaved pixels.

Median (min .. max) of --repeat after a warm-up.  The compiler's resource usage per K is printed first (VGPRs, scratch).

    python tools/time_scene_deep.py --size 512 --out profiles/scene_deep_timing.txt"""
import argparse
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 6.29      # profiles/overlay_timing.txt


def resource_usage():
    """the compiler's resource-usage remarks for k_scene_deep<K> (one compile of ia_scene_deep.hip to nowhere), or why there are none"""
    from instantavatar_amd import build
    src = os.path.join(build.CSRC, "ia_scene_deep.hip")
    cmd = [build.HIPCC] + build.FLAGS + build.extra_flags(src) + [build.cuid_flag(src), "-x", "hip", "-c", src, "-o", os.devnull,
                                                                   "-Rpass-analysis=kernel-resource-usage"]
    try:
        text = subprocess.run(cmd, capture_output=True, text=True, timeout=600).stderr
    except (OSError, subprocess.TimeoutExpired) as e:
        return ["k_scene_deep: resource usage not read (%s)" % e]
    found, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: +(?:\S+:\d+:\d+: +)?(Function Name: (\S+)|([A-Za-z ]+(?:\[[^\]]+\])?): (\S+))", line)
        if not m:
            continue
        if m.group(2):
            k = re.search(r"k_scene_deepILi(\d+)E", m.group(2))
            name = int(k.group(1)) if k else None
        elif name is not None:
            found.setdefault(name, {})[m.group(3).strip()] = m.group(4)
    if not found:
        return ["k_scene_deep: resource usage not read (no remarks from %s)" % build.HIPCC]
    keys = ["VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"]
    return ["k_scene_deep<%d> as compiled for gfx950: " % K + ", ".join("%s %s" % (k, found[K].get(k, "?")) for k in keys) for K in sorted(found)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--layers", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-resources", action="store_true", help="do not compile ia_scene_deep.hip for the resource-usage lines")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, scene, synthetic
    from instantavatar_amd.drivers import animate
    from instantavatar_amd.pipeline import build_synthetic_model
    dev = torch.device("cuda:0")
    models = []
    for seed in (42, 43):
        model, _, _ = build_synthetic_model(dev, seed=seed)
        model.eval()
        models.append(model)
    poses, trans = synthetic.procedural_pose_track(64)
    jitter = animate.fixed_jitter(1, dev)
    H = W = args.size
    R = H * W

    def make(layout, K, **kw):
        if layout == "side by side":
            offsets = [((k - (K - 1) / 2.0) * 0.9, 0.0, 0.0) for k in range(K)]
        else:                                                   # one behind the other: the layers overlap in the frame
            offsets = [(0.0, 0.0, 1.5 * k) for k in range(K)]
        seqs = [scene.place(animate.AnimateSequence(poses[:8], trans[:8], np.zeros(10, np.float32), dev, size=args.size), o) for o in offsets]
        return scene.Scene([models[k % 2] for k in range(K)], seqs, jitter=jitter, phases=[2 * k for k in range(K)], **kw)

    def spread(ms):
        return "%9.4f (%.4f .. %.4f)" % (statistics.median(ms), min(ms), max(ms))

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

    lines = ["ia_scene_deep_composite on the synthetic model (%s): frames of %d x %d, %d slots per list" % (torch.cuda.get_device_name(0), W, H, models[0].renderer.MAX_SAMPLES),
             "kernel: GPU ms between HIP events around %d launches, median (min .. max) of %d after a warm-up; frames: wall ms, median (min .. max) of %d"
             % (args.inner, args.repeat, args.repeat),
             "bytes: 24 per filled slot (z, delta, sigma, rgb) + 8 per list and pixel (the empty head behind a list) + 20 per pixel written; of HBM: "
             "against the measured %.2f TB/s (profiles/overlay_timing.txt)" % HBM_TBS]
    if not args.no_resources:
        lines += resource_usage()
    for layout in ("side by side", "one behind the other"):
        lines.append("")
        lines.append("%s" % layout)
        for K in args.layers:
            sc = make(layout, K, exact=True)
            out = sc.render(0)
            n, inter = int(out["overlap"]), int(out["interleaved"])
            if n == 0:
                lines.append("  K = %d: no active pixel" % K)
                continue
            deep, active, rows = sc.last_deep, sc.last_active, sc.last_rows
            ms = gpu_ms(lambda: scene.composite_exact(out, deep, active, rows))
            whole = statistics.median(ms)
            S = int(deep["z"].shape[1])
            o3, o1, o2 = torch.empty((n, 3), device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev)
            cnt = torch.zeros(1, dtype=torch.int32, device=dev)
            kern = gpu_ms(lambda: _lib.call("ia_scene_deep_composite", deep["z"], deep["delta"], deep["sigma"], deep["rgb"], K, S, n, None, None, None,
                                            None, None, None, 0, 0.01, o3, o1, o2, cnt))
            filled = int((deep["delta"] > 0).sum())
            nbytes = 24 * filled + 8 * K * n + 20 * n
            rate = nbytes / (statistics.median(kern) * 1e-3) / 1e12
            lines.append("  K = %d: %6d active pixels = %.3f %% of the frame, %d interleaved = %.3f %%; %.1f filled slots per list and pixel"
                         % (K, n, 100.0 * n / R, inter, 100.0 * inter / R, filled / float(K * n)))
            lines.append("    ia_scene_deep_composite          %s ms; %.2f MB read or written = %.3f TB/s = %.1f %% of HBM"
                         % (spread(kern), nbytes / 1e6, rate, 100.0 * rate / HBM_TBS))
            lines.append("    composite_exact (gathers, merge, scatter, pack) %.4f ms" % whole)
        plain, exact = make(layout, 2), make(layout, 2, exact=True)
        t_plain, t_exact = wall_ms(lambda: plain.render(0)), wall_ms(lambda: exact.render(0))
        lines.append("  Scene.render, two avatars, exact=False %s ms" % spread(t_plain))
        lines.append("  Scene.render, two avatars, exact=True  %s ms = %.2f x" % (spread(t_exact), statistics.median(t_exact) / statistics.median(t_plain)))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
