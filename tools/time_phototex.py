"""GPU time of the photo texture (csrc/ia_phototex.hip) on the synthetic model: --frames teacher renderings at --res^2 through a full
turn projected onto the atlas of the simplified mesh and, with --full, of the unsimplified one, per block size.  Timed: the
preparation of the frames (pose_mesh + rasterize per frame), ONE ia_phototex_accumulate launch over all frames and the whole atlas,
ia_phototex_resolve, and a whole `AvatarModel.bake_photo_texture` (base=None), Python included.  HIP events, the median of --repeat
runs after one warm-up.

    python tools/time_phototex.py --resolution 256 --simplify 4 --blocks 8 16 --frames 8 --res 512 --full --out profiles/phototex_timing.txt"""
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
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--res", type=int, default=512, help="edge of the frames in pixels")
    ap.add_argument("--full", action="store_true", help="also the unsimplified mesh")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, mesh as M, raster, texture
    from instantavatar_amd.drivers import eval as eval_driver
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
    frames = eval_driver.synthetic_photo_set(dev, model, args.res, args.frames)
    cam = frames.camera()
    F, H, W = len(frames), frames.H, frames.W
    p = frames.smpl_params
    batches = [{"betas": p["betas"][0][None], "global_orient": p["global_orient"][i][None], "body_pose": p["body_pose"][i][None],
                "transl": p["transl"][i][None]} for i in range(F)]
    lines = ["photo texture on the synthetic model (%s): GPU time in ms between HIP events, median of %d after a warm-up" % (torch.cuda.get_device_name(0), args.repeat),
             "%d frames of %d x %d pixels through a full turn; cos_min 0.3, power 2, depth_tol 0.02, min_frames 1" % (F, W, H),
             "%-12s %8s %6s %8s %10s %10s %10s %10s %10s %12s %8s %8s" % ("mesh", "faces", "block", "atlas", "prepare", "accumulate", "resolve", "bake", "zero",
                                                                          "Gpairs/s", "seen", "median")]
    meshes = [("simplified", small)] + ([("extracted", full)] if args.full else [])
    for name, mesh in meshes:
        nv, nf = mesh.verts.shape[0], mesh.faces.shape[0]

        def prepare():
            out = []
            for b in batches:
                posed = model.pose_mesh(mesh, b)
                out.append((posed.verts, raster.rasterize(posed.verts, posed.faces, cam).depth))
            return out
        t_prepare = timed(prepare)
        prepared = prepare()
        verts = torch.stack([v for v, _ in prepared]).contiguous()
        depth = torch.stack([d for _, d in prepared]).contiguous()
        w2c = cam.w2c[None].expand(F, 4, 4).contiguous()
        faces = mesh.faces.to(torch.int32).contiguous()
        for B in args.blocks:
            T = texture.atlas_size(nf, B)
            n = T * T
            acc = torch.empty(int(_lib.call("ia_phototex_acc_bytes", n)), dtype=torch.uint8, device=dev)
            owner = torch.empty(n, dtype=torch.int32, device=dev)
            pts = torch.empty((n, 3), device=dev)
            _lib.call("ia_tex_texel_points", mesh.verts, nv, faces, nf, B, T, 0, n, None, 0.0, pts, None, owner)
            atlas, seen, unseen = torch.empty((n, 3), device=dev), torch.empty(n, dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
            zero = lambda: _lib.call("ia_phototex_zero", acc, n)
            accumulate = lambda: _lib.call("ia_phototex_accumulate", verts, nv, faces, nf, B, T, 0, n, F, w2c, cam.fx, cam.fy, cam.cx, cam.cy, cam.near,
                                           frames.images, frames.masks, depth, H, W, 0.3, 2.0, 0.02, acc)
            resolve = lambda: _lib.call("ia_phototex_resolve", acc, None, owner, n, 1, atlas, seen, unseen)
            t_zero, t_acc = timed(zero), timed(accumulate)
            zero()
            accumulate()
            t_res = timed(resolve)
            t_bake = timed(lambda: model.bake_photo_texture(mesh, frames, block=B, base=None, chunk_frames=F))
            owned = owner >= 0
            hit = seen[owned & (seen > 0)]
            med = int(hit.sort().values[(hit.numel() - 1) // 2]) if hit.numel() else 0
            lines.append("%-12s %8d %6d %8s %10.3f %10.3f %10.3f %10.3f %10.3f %12.3f %7.1f%% %8d" % (
                name, nf, B, "%d^2" % T, t_prepare, t_acc, t_res, t_bake, t_zero, int(owned.sum()) * F / t_acc / 1e6,
                100.0 * hit.numel() / max(int(owned.sum()), 1), med))
            del acc, owner, pts, atlas, seen
            torch.cuda.empty_cache()
    lines += ["",
              "prepare    = pose_mesh + raster.rasterize of every frame (the depth maps), Python included",
              "accumulate = ONE ia_phototex_accumulate over all frames and the whole atlas; Gpairs/s = owned texels x frames / that time",
              "resolve    = ia_phototex_resolve over the whole atlas; zero = ia_phototex_zero (40 bytes per texel)",
              "bake       = AvatarModel.bake_photo_texture(base=None) with all frames in one chunk: prepare + stacking + the three entry points",
              "seen       = share of the owned texels that at least one frame saw; median = median number of frames per seen texel",
              "Measured with tools/time_phototex.py.  First figures: nothing to compare with, nothing tuned."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
