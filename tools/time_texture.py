"""GPU time of the texture atlas (csrc/ia_texture.hip) on the synthetic model's simplified mesh, and what the texture buys: every
entry point alone, a whole bake (`AvatarModel.bake_texture`) and a textured picture, per block size; then the PSNR over the covered
pixels of `canonical_front` at --size^2 of the textured simplified mesh and of the vertex-coloured simplified mesh, both against the
picture of the unsimplified vertex-coloured mesh.  HIP events, the median of `--repeat` runs after one warm-up.

    python tools/time_texture.py --resolution 256 --simplify 4 --blocks 8 16 --out profiles/texture_timing.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--simplify", type=float, default=4.0, help="cell edge in lattice spacings")
    ap.add_argument("--blocks", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--size", type=int, default=512, help="edge of the pictures the PSNR is taken on")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, mesh as M, raster, texture
    from instantavatar_amd.pipeline import build_synthetic_model
    dev = "cuda:0"
    model, _, _ = build_synthetic_model(dev)

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
    snap = max(2.0, args.simplify) * spacing
    nv, nf = small.verts.shape[0], small.faces.shape[0]
    cam = raster.look_at_box(lo, hi, args.size, dev)
    target = full.render(cam)
    covered = target["mask"]

    def psnr(img):
        both = covered & img["mask"]
        d = img["rgba8"][..., :3][both].double() - target["rgba8"][..., :3][both].double()
        return float(10 * torch.log10(255.0 ** 2 / (d * d).mean())), int(both.sum())

    p_vertex, n_px = psnr(small.render(cam))
    lines = ["texture atlas on the synthetic model's mesh (%s): GPU time in ms between HIP events, median of %d after a warm-up" % (torch.cuda.get_device_name(0), args.repeat),
             "resolution %d: %d vertices, %d faces; simplified with a cell of %g lattice spacings: %d vertices, %d faces; snap %g spacings, %d steps"
             % (args.resolution, full.verts.shape[0], full.faces.shape[0], args.simplify, nv, nf, snap / spacing, args.steps),
             "%6s %7s %10s %10s %10s %10s %10s %10s %10s %10s %10s" % ("block", "atlas", "corner_uv", "points", "snap", "field x1", "sample", "bake", "picture",
                                                                 "unsnapped", "PSNR dB")]
    for B in args.blocks:
        T = texture.atlas_size(nf, B)
        n = T * T
        uv = torch.empty((nf, 3, 2), device=dev)
        pts, own, t = torch.empty((n, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
        sig, cnt = torch.full((args.steps, n), 5.0, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        sig[args.steps // 2:] = 15.0
        rgb, s1 = torch.empty((n, 3), device=dev), torch.empty(n, device=dev)
        net = model.net_coarse
        baked = model.bake_texture(small, block=B, snap=snap, steps=args.steps)
        img = baked.render(cam)
        R = args.size ** 2
        out = torch.empty((R, 3), device=dev)
        flat_uv, flat_mask = img["uv"].reshape(R, 2).contiguous(), img["mask"].reshape(R).float()
        ms = dict(
            corner_uv=timed(lambda: _lib.call("ia_tex_corner_uv", nf, B, T, uv)),
            points=timed(lambda: _lib.call("ia_tex_texel_points", small.verts, nv, small.faces, nf, B, T, 0, n, t, 0.0, pts, None, own)),
            snap=timed(lambda: _lib.call("ia_tex_snap", sig, args.steps, n, 10.0, snap, own, t, cnt)),
            field=timed(lambda: _lib.call("ia_field_fwd", pts, n, None, net.field_desc(n), rgb, s1)),
            sample=timed(lambda: _lib.call("ia_tex_sample", baked.texture.atlas, T, flat_uv, flat_mask, R, out)),
            bake=timed(lambda: model.bake_texture(small, block=B, snap=snap, steps=args.steps)),
            picture=timed(lambda: baked.render(cam)))
        owned = int((baked.texture.rgba8[..., 3] != 0).sum())
        p_tex, n_tex = psnr(img)
        assert n_tex == n_px
        lines.append("%6d %7s %10.3f %10.3f %10.3f %10.3f %10.3f %10.3f %10.3f %9.2f%% %10.2f" % (
            B, "%d^2" % T, ms["corner_uv"], ms["points"], ms["snap"], ms["field"], ms["sample"], ms["bake"], ms["picture"],
            100.0 * int(baked.texture.unsnapped) / max(owned, 1), p_tex))
        del uv, pts, own, t, sig, rgb, s1, out, baked, img
        torch.cuda.empty_cache()
    lines += ["",
              "PSNR of the vertex-coloured simplified mesh against the same target: %.2f dB (%d pixels covered by both pictures, %d^2 image)" % (p_vertex, n_px, args.size),
              "",
              "corner_uv = ia_tex_corner_uv; points = ia_tex_texel_points over the whole atlas with t and owner; snap = ia_tex_snap on the whole atlas",
              "field x1  = one ia_field_fwd over the atlas's texels: a bake with a snap makes steps + 1 of them, which is nearly all of its time",
              "sample    = ia_tex_sample on the %d^2 picture; picture = Mesh.render of the textured mesh (raster + sample + packing)" % args.size,
              "bake      = AvatarModel.bake_texture, Python included; unsnapped = share of owned texels without a crossing within the snap distance",
              "PSNR dB   = textured simplified mesh against the unsimplified vertex-coloured mesh, 8-bit, over the pixels both cover",
              "Measured with tools/time_texture.py.  First figures: nothing to compare with, nothing tuned."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
