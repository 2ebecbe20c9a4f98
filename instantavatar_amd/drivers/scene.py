"""Several avatars in one frame, on a ground that receives their shadows, in front of a background (`instantavatar_amd.scene`;
DESIGN.md section 4, "scene composition").

    python -m instantavatar_amd.drivers.scene --synthetic --seeds 42 43 44 --spacing 0.9 --size 512 --max-frames 64 \\
        --ground --checker 0.5 --light -2 -4 2 --background 0.9,0.8,0.7 --out scene/out
    python -m instantavatar_amd.drivers.scene --subjects subjects.json --poses data/animation/aist_demo.npz --ground --light -2 -4 2
    python -m instantavatar_amd.drivers.scene --synthetic --seeds 42 43 --spacing 0.6 --light -3 -1 4 --receive-shadows

`--receive-shadows` (needs `--light`, not `--ground`): the avatars receive shadows too, each other's and their own
(`scene.receive`); `--shadow-bias OTHER SELF` sets the two depth biases in metres, `--no-terminator` leaves out the attached shadow
of surfaces that face away from the light.  One more line is printed: the share of avatar pixels that lie in shadow.

`--exact`: where two avatars share a pixel the frame is composited from every sample of every avatar in depth order, not from whole
layers (`scene.composite_exact`; a second, host-driven pass over those pixels), so bodies that intertwine along a ray come out
right; `--exact-ground` includes the pixels where one avatar and the ground meet.  Two more shares are printed, of the pixels that
were recomposited (overlap) and of those where the avatars' samples really interleave, and the warning about contested pixels is
dropped.

`--subjects` takes the list of `animate --subjects` (ckpt, betas, gender, poses, seed, smpl_dir per entry) plus, per entry, an
`"offset": [x, y, z]` in metres and a `"phase": frames`.  Writes `<i>.png` and `scene.gif` through `animate.write_frames`.  The
scene renders eagerly on one GPU (no captured graphs, no frames in flight, no ranks)."""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

from .. import scene, synthetic
from . import animate


def _background(text, H, W, device):
    """FILE (an image, resized to the frame) or R,G,B in [0, 1] -> what `scene.composite` takes, in the model's channel order (B, G, R)"""
    parts = text.split(",")
    if len(parts) == 3:
        try:
            r, g, b = (float(p) for p in parts)
            return (b, g, r)
        except ValueError:
            pass
    from PIL import Image
    im = np.asarray(Image.open(text).convert("RGB").resize((W, H)), np.float32) / 255.0
    return torch.as_tensor(np.ascontiguousarray(im[..., ::-1]), device=device)


def _track(path, max_frames):
    if not path and max_frames > 64:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests", "golden", "aist_demo_200.npz")
    if path:
        z = np.load(path)
        poses, trans = z["poses"].astype(np.float32), z["trans"].astype(np.float32)
    else:
        poses, trans = synthetic.procedural_pose_track(64)
    if max_frames:
        poses, trans = poses[:max_frames], trans[:max_frames]
    return poses, trans


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--subjects", help="JSON list of per-subject overrides as for animate --subjects, plus \"offset\": [x,y,z] and \"phase\": frames")
    ap.add_argument("--synthetic", action="store_true", help="synthetic bodies + fields, one per --seeds entry")
    ap.add_argument("--seeds", type=int, nargs="+", default=[42, 43])
    ap.add_argument("--spacing", type=float, default=0.9, help="--synthetic: metres between neighbouring avatars, side by side")
    ap.add_argument("--poses", help="npz with `poses` [n,>=72] and `trans` [n,3]")
    ap.add_argument("--ckpt")
    ap.add_argument("--betas")
    ap.add_argument("--smpl-dir", default="./data/SMPLX/smpl")
    ap.add_argument("--gender", default="neutral")
    ap.add_argument("--confs", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "confs"))
    ap.add_argument("--deformer", default="fast_snarf")
    ap.add_argument("--network", default="ngp")
    ap.add_argument("--renderer", default="raymarcher_acc")
    ap.add_argument("--size", type=int, default=512, help="square image edge in pixels")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--jitter-seed", type=int, default=None, help="one occupancy-probe jitter for all renders: the files become a function of the arguments")
    ap.add_argument("--ground", action="store_true", help="a floor through the lowest body vertex of the run")
    ap.add_argument("--checker", type=float, default=0.0, metavar="CELL", help="checker cells of CELL metres on the ground")
    ap.add_argument("--light", type=float, nargs=3, metavar=("X", "Y", "Z"), help="a point light (camera frame: +y down); with --ground: shadows")
    ap.add_argument("--shadow-size", type=int, default=256)
    ap.add_argument("--shadow-strength", type=float, default=0.6)
    ap.add_argument("--receive-shadows", action="store_true", help="the avatars receive shadows too, each other's and their own (needs --light)")
    ap.add_argument("--shadow-bias", type=float, nargs=2, default=[0.02, 0.05], metavar=("OTHER", "SELF"),
                    help="--receive-shadows: metres a caster must lie nearer to the light than the receiver, for another avatar and for "
                         "the receiver's own (this project's choices, not measurements)")
    ap.add_argument("--no-terminator", action="store_true", help="--receive-shadows: no attached shadow on surfaces that face away from the light")
    ap.add_argument("--exact", action="store_true", help="composite every sample in depth order where avatars share a pixel (exact where they interleave)")
    ap.add_argument("--exact-ground", action="store_true", help="--exact: also where one avatar and the ground share a pixel")
    ap.add_argument("--background", metavar="FILE|R,G,B")
    ap.add_argument("--out", default="scene/out")
    ap.add_argument("--no-gif", action="store_true")
    animate.add_png_args(ap, apng_name="scene.png")
    args = ap.parse_args(argv)
    animate.check_png_args(ap, args)
    if args.exact_ground and not args.exact:
        ap.error("--exact-ground needs --exact")
    if args.receive_shadows and args.light is None:
        ap.error("--receive-shadows needs --light X Y Z: there is nothing to cast a shadow without a light")
    device = torch.device("cuda", torch.cuda.current_device())
    if args.subjects:
        with open(args.subjects) as f:
            entries = json.load(f)
        if not isinstance(entries, list) or not entries:
            ap.error("--subjects: a non-empty JSON list of objects")
        for e in entries:
            unknown = set(e) - {"ckpt", "betas", "gender", "poses", "seed", "smpl_dir", "offset", "phase"}
            if unknown:
                ap.error("--subjects: unknown keys %s" % sorted(unknown))
    elif args.synthetic:
        n = len(args.seeds)
        entries = [{"seed": s, "offset": [(k - (n - 1) / 2.0) * args.spacing, 0.0, 0.0]} for k, s in enumerate(args.seeds)]
    else:
        ap.error("--subjects or --synthetic is required")
    if not 1 <= len(entries) <= scene.MAX_LAYERS:
        ap.error("1 .. %d avatars can share a frame, got %d" % (scene.MAX_LAYERS, len(entries)))
    models, seqs, phases = [], [], []
    for e in entries:
        a = copy.copy(args)
        for k, v in e.items():
            if k not in ("offset", "phase"):
                setattr(a, k, v)
        if not a.synthetic and not (a.ckpt and a.poses):
            ap.error("--ckpt and --poses (here or per subject) are required unless --synthetic is given")
        model, betas = animate.build_model(a, device, quiet=True)
        model.eval()
        poses, trans = _track(a.poses, args.max_frames)
        seq = animate.AnimateSequence(poses, trans, betas, device, size=args.size)
        scene.place(seq, e.get("offset", [0.0, 0.0, 0.0]))
        models.append(model)
        seqs.append(seq)
        phases.append(int(e.get("phase", 0)))
    H, W = seqs[0].H, seqs[0].W
    ground = None
    if args.ground:
        opts = dict(color=(0.75, 0.75, 0.75))
        if args.checker > 0:
            opts.update(color2=(0.45, 0.45, 0.45), cell=args.checker)
        ground = scene.ground_under(models, seqs, **opts)
    jitter = None if args.jitter_seed is None else animate.fixed_jitter(args.jitter_seed, device)
    sc = scene.Scene(models, seqs, ground=ground, light=args.light, shadow_size=args.shadow_size, shadow_strength=args.shadow_strength,
                     background=None if args.background is None else _background(args.background, H, W, device), jitter=jitter,
                     phases=phases, receive=args.receive_shadows, receive_normals=not args.no_terminator, bias_other=args.shadow_bias[0],
                     bias_self=args.shadow_bias[1], exact=args.exact, exact_ground=args.exact_ground)
    n = len(sc)
    shadowed = torch.zeros(2, dtype=torch.int64, device=device)       # avatar pixels (alpha >= 0.5 in any layer), and those of them in shadow
    deep = torch.zeros(2, dtype=torch.int64, device=device)           # --exact: recomposited pixels, and those of them that interleave
    want_host = not args.gpu_png or not args.no_gif          # raw pixels on the host: PIL's PNG route, and the GIF
    host = torch.empty((n if want_host else 0, H, W, 4), dtype=torch.uint8, pin_memory=True)
    frames_dev = torch.empty((n, H, W, 4), dtype=torch.uint8, device=device) if args.gpu_png else None
    sc.render(0)                       # warm-up: workspaces, the loop-length hint
    sc.contested_total.zero_()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        out = sc.render(i)
        if want_host:
            host[i].copy_(out["rgba8"], non_blocking=True)
        if frames_dev is not None:
            frames_dev[i].copy_(out["rgba8"])
        if args.exact:
            deep += torch.stack([out["overlap"], out["interleaved"]])
        if args.receive_shadows:
            solid = torch.stack([l[1] for l in sc.last_layers]) >= 0.5
            shadowed += torch.stack([solid.any(0).sum(), (solid & (out["layer_shade"] < 0.99)).any(0).sum()])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if args.gpu_png:        # one batch call on the device, only the compressed streams come over; the GIF stays PIL's
        enc = animate.write_frames(frames_dev, args.out, gpu_png=True)
        if args.apng:
            enc.write_apng(os.path.join(args.out, "scene.png"), fps=30, loop=0)
        if not args.no_gif and n:
            animate.write_gif(host.numpy(), os.path.join(args.out, "scene.gif"))
    else:
        animate.write_frames(host.numpy(), args.out, gif=None if args.no_gif else "scene.gif")
    share = int(sc.contested_total) / float(max(1, n * H * W))
    print("rendered %d frames (%dx%d) of %d avatar(s)%s in %.3f s = %.1f frames/s (eager; PNG / GIF I/O excluded)"
          % (n, W, H, len(seqs), (" with ground shadows" if sc.shadows else "") + (" that receive shadows" if sc.receive else ""), dt, n / dt if dt > 0 else 0.0))
    print("contested pixels: %.4f %% of all" % (100.0 * share))
    if args.receive_shadows:
        pixels, dark = shadowed.tolist()        # the one read of the counters
        print("avatar pixels in shadow: %.2f %% (shade below 0.99 in a layer with alpha >= 0.5; %d avatar pixels over %d frames)"
              % (100.0 * dark / max(1, pixels), pixels, n))
    if args.exact:
        over, inter = deep.tolist()
        print("overlap pixels: %.4f %% of all (recomposited from the avatars' samples); interleaved pixels: %.4f %% of all"
              % (100.0 * over / max(1, n * H * W), 100.0 * inter / max(1, n * H * W)))
    elif share > 0:
        print("warning: at contested pixels two avatars are closer along the ray than %.2f m; layered compositing may order them wrongly there"
              % sc.contact)
    print("wrote %d frames to %s" % (n, args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
