"""Write the avatar's geometry as triangle meshes: the canonical mesh and, with a pose track, one posed mesh per frame.

    python -m instantavatar_amd.drivers.extract_mesh --ckpt checkpoints/last.ckpt --smpl-dir ./data/SMPLX/smpl --gender male \\
        --betas data/subject/anim_nerf_train.npz --poses data/animation/aist_demo.npz --max-frames 8 --out meshes/subject
    python -m instantavatar_amd.drivers.extract_mesh --synthetic --resolution 128 --out /tmp/mesh

The canonical mesh is the isosurface sigma = --level of the canonical density field by marching tetrahedra on a
--resolution^3 lattice over the field's box (`AvatarModel.extract_mesh`; DESIGN.md section 4, "isosurface"); the level is this
project's choice, the reference has none.  Posed meshes are the same vertices skinned forward with the frame's bone
transforms (`AvatarModel.pose_mesh`), in the world frame of the animate driver's camera; they share faces and colours with
the canonical mesh.  Files: `canonical.<format>`, `posed_<i>.<format>`.

--render SIZE also draws the meshes with the GPU rasteriser ("rasteriser"), SIZE x SIZE pixels:
`canonical_front.png` is the canonical mesh seen by a camera on the -z side of the field's box, on the axis through the box
centre, looking along +z at the centre with world +y up in the image, focal length SIZE pixels, at the distance at which the
box's nearest face spans 90 % of the image (`raster.look_at_box`); with --poses, `posed_<i>.png` (vertex colours) and
`posed_shaded_<i>.png` (lit from the camera) show every posed mesh under the animate driver's camera scaled to SIZE.  Alpha is
the raster mask.

--smooth ITERS and --simplify K process the canonical mesh before anything is written ("mesh simplification"):
first ITERS Taubin iterations, then vertex clustering with quadrics on a grid whose cell edge is K lattice spacings, a spacing
being max(hi - lo) / (resolution - 1) of the field's box.  The processed mesh is the one that is written, posed and drawn.  One
line reports `N -> M vertices, N -> M faces` and the wall time of each stage.

--texture BLOCK bakes the colour field into a texture atlas over the final mesh, half a block of BLOCK^2 texels per face (DESIGN.md
section 4, "texture atlas"; `AvatarModel.bake_texture`), after moving every texel's point along the face normal onto the isosurface
where that lies within --snap lattice spacings (default max(2, --simplify)).  It additionally writes `canonical_textured.obj` / `.mtl` /
`.png`, with --poses `posed_<i>_textured.obj` (which share that one .mtl and .png), with --render `canonical_front_textured.png` and
`posed_textured_<i>.png`, and reports the atlas size and the share of texels that found no surface within --snap.

--rig K additionally writes `avatar.glb`, a glTF 2.0 binary of the final mesh with a skin of 24 joints and the K (1 .. 24) largest
skinning weights per vertex ("rigged export"; `AvatarModel.rig_mesh`, `Mesh.to_glb`): textured with --texture,
vertex-coloured without, and with --poses animated by the pose track at --fps key frames per second.  With --poses one line reports
the maximum and the mean distance, over all frames and vertices, between the rig's skinning and the posed meshes.

--deviation [SAMPLES] (with --smooth or --simplify) measures how far the processed mesh lies from the extracted one (DESIGN.md section 4,
"surface distance"; `Mesh.compare`): SAMPLES surface samples per direction (default 100 000), one `deviation:` line with the mean, the
95th percentile and the maximum of the distances both ways in metres and in lattice spacings, and `deviation.json` with the whole
report.  With --render it also writes `deviation_front.png`: the EXTRACTED mesh under the camera of `canonical_front.png`, every
vertex coloured by its distance to the final mesh, blue (0) over green to red (2 lattice spacings and more).  --signed (with
--deviation) adds on which side the processed surface lies ("ray queries"): one `bias:` line with the mean signed
offset of the processed surface from the extracted one in metres and lattice spacings -- negative: inside, the surface shrank -- and the
share of its samples inside, and the signed keys in `deviation.json`.

--photo (with --texture BLOCK) additionally textures the mesh from the frames of a sequence ("photo texture";
`AvatarModel.bake_photo_texture`): every frame's posed mesh is rasterised for its depth map and the frame's pixels are projected
onto the texels that face its camera and are neither hidden nor outside the mask; texels that no frame saw keep the colour of the
field-baked atlas.  The frames are the `train` split of --data DIR (with --dataset / --start / --end / --skip / --downscale as in
the train driver), or with --synthetic --photo-frames N renderings of the synthetic subject at --photo-res^2 whose body turns
through a full circle.  It writes `canonical_phototextured.obj` / `.mtl` / `.png` and `coverage.png` (the atlas layout, red: no
frame saw the texel, over green to blue: the largest count), with --render `canonical_front_phototextured.png`; with --rig,
`avatar.glb` carries the photo texture.  One line reports the frames used, the share of owned texels seen at least once, the
median number of frames per seen texel and the wall time."""
import argparse
import os
import sys
import time

import numpy as np

from . import animate, sequence_args


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", help="npz with `poses` [n,>=72] and `trans` [n,3]: also write posed_<i> per frame")
    ap.add_argument("--ckpt", help="Lightning checkpoint of DNeRFModel")
    ap.add_argument("--betas", help="npz with `betas` (the subject's anim_nerf_train.npz)")
    ap.add_argument("--smpl-dir", default="./data/SMPLX/smpl")
    ap.add_argument("--gender", default="neutral")
    ap.add_argument("--confs", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "confs"))
    ap.add_argument("--deformer", default="fast_snarf")
    ap.add_argument("--network", default="ngp")
    ap.add_argument("--renderer", default="raymarcher_acc")
    ap.add_argument("--synthetic", action="store_true", help="synthetic SMPL-like body + field (no SMPL pickle / checkpoint needed)")
    ap.add_argument("--seed", type=int, default=None, help="--synthetic: seed of the synthetic body + field")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--resolution", type=int, default=256, help="lattice samples per axis (2 .. 564)")
    ap.add_argument("--level", type=float, default=10.0, help="density of the isosurface (this project's choice; the reference has none)")
    ap.add_argument("--keep", choices=("largest", "all"), default="largest", help="largest: only the connected component with the largest area")
    ap.add_argument("--format", choices=("ply", "obj"), default="ply")
    ap.add_argument("--render", type=int, default=0, metavar="SIZE", help="also write SIZE x SIZE pictures of the meshes (GPU rasteriser)")
    ap.add_argument("--smooth", type=int, default=0, metavar="ITERS", help="Taubin iterations on the canonical mesh (0: none)")
    ap.add_argument("--simplify", type=float, default=0.0, metavar="K", help="cluster the vertices on a grid of K >= 1 lattice spacings (0: no)")
    ap.add_argument("--texture", type=int, default=0, metavar="BLOCK", help="bake a texture atlas with BLOCK in 4 .. 64 texels per block edge (0: no)")
    ap.add_argument("--snap", type=float, default=None, metavar="K", help="--texture: snap the texels onto the isosurface within K lattice spacings "
                    "(default max(2, --simplify); 0: no snap)")
    ap.add_argument("--rig", type=int, default=0, metavar="K", help="also write avatar.glb: the mesh rigged with K in 1 .. 24 influences per vertex (0: no)")
    ap.add_argument("--fps", type=float, default=30.0, help="--rig with --poses: key frames per second of the glTF animation")
    ap.add_argument("--deviation", type=int, nargs="?", const=100000, default=None, metavar="SAMPLES", help="with --smooth / --simplify: report the "
                    "distance between the extracted and the processed mesh from SAMPLES surface samples per direction (default 100000)")
    ap.add_argument("--signed", action="store_true", help="--deviation: also report on which side of the extracted surface the processed one lies")
    ap.add_argument("--photo", action="store_true", help="--texture: also texture the mesh from the frames of --data DIR (or, with --synthetic, "
                    "from generated frames): canonical_phototextured.{obj,mtl,png}, coverage.png")
    ap.add_argument("--photo-frames", type=int, default=8, metavar="N", help="--photo --synthetic: the number of generated frames")
    ap.add_argument("--photo-res", type=int, default=256, metavar="SIZE", help="--photo --synthetic: the edge of the generated frames in pixels")
    sequence_args.add_data_arguments(ap)
    ap.add_argument("--out", default="meshes/out")
    animate.add_png_args(ap, apng_name="posed.png, posed_shaded.png, posed_textured.png of the --render pictures")
    args = ap.parse_args(argv)
    animate.check_png_args(ap, args)
    if args.deviation is not None and not (args.smooth or args.simplify):
        ap.error("--deviation compares the extracted mesh with the processed one: it needs --smooth or --simplify")
    if args.deviation is not None and args.deviation < 0:
        ap.error("--deviation %d: the number of samples cannot be negative" % args.deviation)
    if args.signed and args.deviation is None:
        ap.error("--signed gives the deviation its sign: it needs --deviation")
    if args.photo and not args.texture:
        ap.error("--photo textures the atlas of --texture BLOCK from the frames: it needs --texture")
    if args.photo and not (args.synthetic or args.data):
        ap.error("--photo needs a frame source: --data DIR, or --synthetic")
    if args.photo and (args.photo_frames < 1 or args.photo_res < 8):
        ap.error("--photo-frames must be at least 1 and --photo-res at least 8")
    if not args.synthetic and not args.ckpt:
        ap.error("--ckpt is required unless --synthetic is given")
    if args.smooth < 0:
        ap.error("--smooth %d: the number of iterations cannot be negative" % args.smooth)
    if args.simplify != 0 and not args.simplify >= 1:
        ap.error("--simplify %g: the cell edge is given in lattice spacings and must be at least 1" % args.simplify)
    if args.texture != 0 and not 4 <= args.texture <= 64:
        ap.error("--texture %d: the block edge must lie in 4 .. 64 texels" % args.texture)
    if args.snap is not None and not (args.texture and args.snap >= 0 and np.isfinite(args.snap)):
        ap.error("--snap needs --texture and a distance >= 0 in lattice spacings")
    if args.rig != 0 and not 1 <= args.rig <= 24:
        ap.error("--rig %d: the number of influences per vertex must lie in 1 .. 24" % args.rig)
    if not (args.fps > 0 and np.isfinite(args.fps)):
        ap.error("--fps %g: the frame rate must be positive" % args.fps)
    import torch
    device = torch.device("cuda:0")
    model, betas = animate.build_model(args, device)
    model.eval()
    os.makedirs(args.out, exist_ok=True)
    write = lambda mesh, name: getattr(mesh, "to_" + args.format)(os.path.join(args.out, "%s.%s" % (name, args.format)))
    timings = {}
    mesh = model.extract_mesh(resolution=args.resolution, level=args.level, largest=args.keep == "largest", timings=timings)
    extracted = mesh
    if args.smooth or args.simplify:
        from .. import mesh as mesh_mod
        stages = []

        def timed(name, fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            stages.append("%s %.3f s" % (name, time.perf_counter() - t0))
            return out
        if args.smooth:
            mesh = timed("smooth", lambda: model.smooth_mesh(mesh, args.smooth))
        if args.simplify:
            lo, hi = mesh_mod.field_box(model.net_coarse)
            cell = args.simplify * float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / (args.resolution - 1)
            mesh = timed("simplify", lambda: model.simplify_mesh(mesh, cell))
    write(mesh, "canonical")
    print("canonical mesh: %d vertices, %d faces at resolution %d, level %g (field %.3f s, count + emit %.3f s, component filter %.3f s)"
          % (extracted.verts.shape[0], extracted.faces.shape[0], args.resolution, args.level, timings["field"], timings["isosurface"], timings["component"]))
    if mesh is not extracted:
        print("processed mesh: %d -> %d vertices, %d -> %d faces (%s)"
              % (extracted.verts.shape[0], mesh.verts.shape[0], extracted.faces.shape[0], mesh.faces.shape[0], ", ".join(stages)))
    if args.deviation is not None:
        import json
        from .. import mesh as mesh_mod, meshdist
        lo, hi = mesh_mod.field_box(model.net_coarse)
        spacing = float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / (args.resolution - 1)
        report = extracted.compare(mesh, samples=args.deviation, signed=True) if args.signed else extracted.compare(mesh, samples=args.deviation)
        ab, ba = report["a_to_b"], report["b_to_a"]
        print("deviation: extracted -> processed mean %.3e p95 %.3e max %.3e m (%.3f / %.3f / %.3f spacings), processed -> extracted mean %.3e "
              "p95 %.3e max %.3e m (%.3f / %.3f / %.3f spacings), %d samples each way"
              % (ab["mean"], ab["p95"], ab["max"], ab["mean"] / spacing, ab["p95"] / spacing, ab["max"] / spacing, ba["mean"], ba["p95"],
                 ba["max"], ba["mean"] / spacing, ba["p95"] / spacing, ba["max"] / spacing, args.deviation))
        if args.signed:
            print("bias: the processed surface lies %+.3e m (%+.3f spacings) from the extracted one on average (negative: inside), "
                  "%.1f %% of its samples inside" % (ba["signed_mean"], ba["signed_mean"] / spacing, 100.0 * ba["inside_share"]))
        report.update(resolution=args.resolution, spacing=spacing, samples=args.deviation,
                      extracted=dict(vertices=int(extracted.verts.shape[0]), faces=int(extracted.faces.shape[0])),
                      processed=dict(vertices=int(mesh.verts.shape[0]), faces=int(mesh.faces.shape[0])))
        with open(os.path.join(args.out, "deviation.json"), "w") as out:
            json.dump(meshdist.report_json(report), out, indent=1, sort_keys=True)
        if args.render:
            from PIL import Image
            from .. import raster
            cam = raster.look_at_box(lo, hi, args.render, device)
            painted = mesh_mod.Mesh(extracted.verts, extracted.faces, extracted.normals,
                                    meshdist.heat(extracted.distance_to(mesh)["dist"], 2.0 * spacing))
            Image.fromarray(animate._bgra_to_rgba(painted.render(cam)["rgba8"].cpu().numpy()), "RGBA").save(os.path.join(args.out, "deviation_front.png"))
    textured = None
    if args.texture:
        from .. import mesh as mesh_mod
        lo, hi = mesh_mod.field_box(model.net_coarse)
        spacing = float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / (args.resolution - 1)
        snap = (max(2.0, args.simplify) if args.snap is None else args.snap) * spacing
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        textured = model.bake_texture(mesh, block=args.texture, snap=snap, level=args.level)       # (a copy: `mesh` keeps none)
        tex = textured.texture
        unsnapped, n_owned = torch.stack([tex.unsnapped, (tex.rgba8[..., 3] != 0).sum().to(torch.int32)]).tolist()   # the one host read
        textured.to_obj_textured(os.path.join(args.out, "canonical_textured.obj"))
        print("texture: atlas %d x %d texels in blocks of %d, snap %.4g, %d of %d owned texels (%.2f %%) without a surface crossing (%.3f s, "
              "file writing included)" % (tex.size, tex.size, tex.block, snap, unsnapped, n_owned, 100.0 * unsnapped / max(n_owned, 1),
                                          time.perf_counter() - t0))
    photo = None
    if args.photo:
        from PIL import Image
        from .. import phototex
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.data:
            from ..utils.sampler import EdgeSampler
            frames = sequence_args.load_directory(args, "train", EdgeSampler(num_sample=4096, ratio_mask=0.6, ratio_edge=0.3, kernel_size=16), device)
        else:
            from . import eval as eval_driver
            frames = eval_driver.synthetic_photo_set(device, model, args.photo_res, args.photo_frames)
        photo, seen = model.bake_photo_texture(mesh, frames, block=args.texture, base=textured.texture)
        owned = photo.texture.rgba8[..., 3] != 0
        counts = seen[owned & (seen > 0)]
        median = counts.sort().values[(counts.numel() - 1) // 2].long() if counts.numel() else torch.zeros((), dtype=torch.long, device=device)
        n_owned, n_seen, median = torch.stack([owned.sum(), (owned & (seen > 0)).sum(), median]).tolist()     # the one host read
        photo.to_obj_textured(os.path.join(args.out, "canonical_phototextured.obj"))
        Image.fromarray(animate._bgra_to_rgba(phototex.coverage_image(seen, owned).cpu().numpy()), "RGBA").save(os.path.join(args.out, "coverage.png"))
        print("photo texture: %d frames, %d of %d owned texels (%.2f %%) seen at least once, median %d frames per seen texel (%.3f s, frames and "
              "file writing included)" % (len(frames), n_seen, n_owned, 100.0 * n_seen / max(n_owned, 1), median, time.perf_counter() - t0))
    if args.render:
        from PIL import Image
        from .. import mesh as mesh_mod, raster
        cam = raster.look_at_box(*mesh_mod.field_box(model.net_coarse), args.render, device)
        front = mesh.render(cam)["rgba8"].cpu().numpy()
        Image.fromarray(animate._bgra_to_rgba(front), "RGBA").save(os.path.join(args.out, "canonical_front.png"))
        if textured is not None:
            front = textured.render(cam)["rgba8"].cpu().numpy()
            Image.fromarray(animate._bgra_to_rgba(front), "RGBA").save(os.path.join(args.out, "canonical_front_textured.png"))
        if photo is not None:
            front = photo.render(cam)["rgba8"].cpu().numpy()
            Image.fromarray(animate._bgra_to_rgba(front), "RGBA").save(os.path.join(args.out, "canonical_front_phototextured.png"))
    n = 0
    rig = model.rig_mesh(mesh, influences=args.rig) if args.rig else None
    animation = None
    if args.poses:
        z = np.load(args.poses)
        poses, trans = z["poses"].astype(np.float32), z["trans"].astype(np.float32)
        if args.max_frames:
            poses, trans = poses[:args.max_frames], trans[:args.max_frames]
        seq = animate.AnimateSequence(poses, trans, betas, device, size=args.render or 8)      # (its SMPL parameters; its camera with --render)
        cam = seq.camera() if args.render else None
        colour, shaded, painted = [], [], []
        t0 = time.perf_counter()
        if rig is not None:
            from .. import rig as rig_mod
            bones, quat, root_t = rig_mod.track(model.deformer, seq.thetas, seq.transl)
            animation = (quat, root_t)
            skinned = rig_mod.skin(rig, mesh, bones)[0]
            dev_max, dev_sum = torch.zeros((), dtype=torch.float64, device=device), torch.zeros((), dtype=torch.float64, device=device)
        for i in range(len(seq)):
            posed = model.pose_mesh(mesh, seq.batch(i, rays=False))
            if rig is not None:
                d_max, d_mean = rig_mod.deviation(skinned[i:i + 1], posed.verts[None])
                dev_max, dev_sum = torch.maximum(dev_max, d_max[0]), dev_sum + d_mean[0]
            write(posed, "posed_%d" % i)
            if cam is not None:
                img = posed.render(cam)
                keep = (lambda t: t.clone()) if args.gpu_png else (lambda t: t.cpu().numpy())
                colour.append(keep(img["rgba8"]))
                shaded.append(keep(img["shaded8"]))
            if textured is not None:
                posed.texture = textured.texture
                posed.to_obj_textured(os.path.join(args.out, "posed_%d_textured.obj" % i), mtllib="canonical_textured.mtl")
                if cam is not None:
                    painted.append(keep(posed.render(cam)["rgba8"]))
        n = len(seq)
        if cam is not None:
            for frames, prefix, name in ((colour, "posed_", "posed.png"), (shaded, "posed_shaded_", "posed_shaded.png")) + \
                    (((painted, "posed_textured_", "posed_textured.png"),) if textured is not None else ()):
                if args.gpu_png and frames:
                    enc = animate.write_frames(torch.stack(frames), args.out, prefix=prefix, gpu_png=True)
                    if args.apng:
                        enc.write_apng(os.path.join(args.out, name), fps=args.fps, loop=0)
                else:
                    animate.write_frames(frames, args.out, prefix=prefix)
        print("posed meshes: %d frames in %.3f s (file writing included)" % (n, time.perf_counter() - t0))
        if rig is not None and n:
            print("rig: %d influences per vertex deviate from the posed meshes by at most %.3e, %.3e on average over %d frames"
                  % (args.rig, float(dev_max), float(dev_sum) / n, n))
    if rig is not None:
        (photo if photo is not None else textured if textured is not None else mesh).to_glb(os.path.join(args.out, "avatar.glb"), rig, animation, args.fps)
        print("rig: avatar.glb with %d vertices, 24 joints, %d influences%s%s" % (
            mesh.verts.shape[0], args.rig, ", photo-textured" if photo is not None else ", textured" if textured is not None else "", ", %d key frames at %g per second" % (n, args.fps) if n else ""))
    print("wrote canonical.%s%s to %s" % (args.format, " and %d posed meshes" % n if n else "", args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
