"""`animate.py` without Lightning / Hydra (reference animate.py:13-118): render a novel-pose sequence
with a trained (or synthetic) avatar and write PNG frames + a GIF.

    python -m instantavatar_amd.drivers.animate --poses data/animation/aist_demo.npz \\
        --ckpt checkpoints/last.ckpt --smpl-dir ./data/SMPLX/smpl --gender male --out animation/aist_demo
    python -m instantavatar_amd.drivers.animate --synthetic --max-frames 8 --downscale 8 --out /tmp/anim

Camera, ray construction and the pose-track conventions are the reference's AnimateDataset
(animate.py:13-80): 1080x1080 pinhole with f = 2000, c2w = I, `trans - trans[0] + (0, 0.15, 5)`,
near/far = |transl| -+ 1.  Frames are replayed from one captured HIP graph (pipeline.GraphedRenderer)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

from .. import synthetic
from ..pipeline import AvatarModel, build_synthetic_model
from . import checkpoint as ckpt_io
from . import config as cfg


def make_rays(K, c2w, H, W):
    """animate.py:13-25"""
    x, y = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    xy = np.stack([x, y, np.ones_like(x)], axis=-1).reshape(-1, 3).astype(np.float32)
    d_c = xy @ np.linalg.inv(K).T
    d_w = d_c @ c2w[:3, :3].T
    d_w = d_w / np.linalg.norm(d_w, axis=1, keepdims=True)
    o_w = np.tile(c2w[:3, 3], (len(d_w), 1))
    return o_w.astype(np.float32), d_w.astype(np.float32)


class AnimateSequence:
    """AnimateDataset (animate.py:27-80) as device-resident batches."""

    def __init__(self, poses72, trans, betas, device, downscale=2, size=None):
        """size: a square image of that edge instead of 1080 // downscale (the same camera scaled by size / 1080: the 512 x 512
        frame BASELINE.json's metric is quoted on)."""
        H = W = 1080
        K = np.eye(3)
        K[0, 0] = K[1, 1] = 2000
        K[0, 2] = H // 2
        K[1, 2] = W // 2
        if size:
            K[:2] *= size / H
            H = W = int(size)
        elif downscale > 1:
            H, W = H // downscale, W // downscale
            K[:2] /= downscale
        self.H, self.W = H, W
        self.K = K
        o, d = make_rays(K, np.eye(4), H, W)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)
        self.rays_o, self.rays_d = t(o)[None], t(d)[None]
        self.thetas = t(poses72[..., :72])
        self.transl = t(trans - trans[0:1] + np.array([0, 0.15, 5], np.float32))
        self.betas = t(betas).reshape(1, 10)

    def __len__(self):
        return self.transl.shape[0]

    def camera(self, near=0.05):
        """the sequence's camera for the mesh rasteriser (`raster.Camera`): its K, w2c = I, its image size -- the camera its rays
        were made from, so a raster frame overlays a rendered one"""
        from ..raster import Camera
        return Camera(self.K, torch.eye(4, device=self.rays_o.device), self.H, self.W, near=near)

    def batch(self, idx, rays=True):
        """rays=False: the SMPL parameters only (views, no launch) -- all a captured frame graph reads per frame; its rays
        are static and near / far are recomputed from the ray origins inside the renderer (snarf_deformer.py:101-103)."""
        pose = {"betas": self.betas, "global_orient": self.thetas[idx:idx + 1, :3], "body_pose": self.thetas[idx:idx + 1, 3:],
                "transl": self.transl[idx:idx + 1]}
        if not rays:
            return pose
        dist = torch.sqrt((self.transl[idx] ** 2).sum())
        ones = torch.ones(1, self.rays_d.shape[1], device=self.rays_d.device)
        return {"rays_o": self.rays_o, "rays_d": self.rays_d, **pose, "near": ones * (dist - 1), "far": ones * (dist + 1)}


def build_model(args, device, quiet=False):
    if args.synthetic:
        model, _, _ = build_synthetic_model(device, seed=int(getattr(args, "seed", None) or 42))
        if args.ckpt:  # synthetic body, trained weights (e.g. written by drivers.train --synthetic)
            missing, unexpected = ckpt_io.load_checkpoint(model, args.ckpt, map_location=device, strict_self_check=True)
            if not quiet:
                print("checkpoint %s loaded (step %d)" % (args.ckpt, model.global_step))
        return model, np.zeros(10, np.float32)
    deformer, net, renderer = cfg.build_plugins(args.confs, args.deformer, args.network, args.renderer, gender=args.gender,
                                                deformer_kwargs=dict(model_path=args.smpl_dir))
    model = AvatarModel(deformer, net, renderer).to(device)
    renderer.initialize(1)
    betas = np.zeros(10, np.float32)
    if args.betas:
        betas = np.load(args.betas)["betas"].reshape(-1)[:10].astype(np.float32)
    missing, unexpected = ckpt_io.load_checkpoint(model, args.ckpt, map_location=device, strict_self_check=True)
    if not quiet:
        print("checkpoint %s: %d tensors not on the path ignored, %d own tensors kept at init" % (args.ckpt, len(unexpected), len(missing)))
    if not getattr(deformer, "initialized", False):
        deformer.initialize(torch.as_tensor(betas, device=device).reshape(1, 10), device)
        deformer.initialized = True
    # The reference's animate.py never calls net.initialize: `center` / `scale` come from the checkpoint
    # (buffers written by training, DNeRF.py:134).  Only a checkpoint without them falls back to the bbox.
    if "net_coarse.center" in missing or "net_coarse.scale" in missing:
        net.initialize(deformer.bbox)
    else:
        net.bbox = deformer.bbox    # attribute only (NeRFNGPNet.initialize is a no-op once `bbox` exists)
    return model, betas


def _bgra_to_rgba(f):
    return np.ascontiguousarray(np.asarray(f)[..., [2, 1, 0, 3]])


def write_frames(frames, out_dir, gif=None, indices=None, workers=8, prefix="", gpu_png=False):
    """8-bit [H, W, 4] frames in the MODEL's channel order -> `<i>.png` (+ optionally one GIF) with the colours the reference's
    files have.  The reference writes with cv2.imwrite (animate.py:113), which takes channel 0 as BLUE: the model's channels are
    in the (B, G, R) order of the cv2.imread training images (peoplesnapshot.py:100), so its files hold the intended colours;
    for the GIF it converts BGRA -> RGBA first (:115).  PIL takes channel 0 as RED: the same reorder serves both.
    indices: the file number of every frame (a rank of a multi-GPU job writes only the frames it rendered); PNG encoding
    runs on `workers` threads (zlib releases the GIL).  prefix: `<prefix><i>.png` (the mesh previews).
    gpu_png: the opt-in route of `--gpu-png`.  `frames` is then a uint8 tensor ON THE DEVICE (or, already encoded, a
    `png.HostStreams`): the batch is filtered and deflated there in one call with the channel swap folded into the read
    (`png.encode(..., swap_rb=True)`), only the compressed streams are copied to the host, and the threads (at most 16) just frame
    and write the files.  The pixels of the files are the same; their bytes are the device encoder's, not PIL's.  Returns the
    HostStreams then (None otherwise)."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(out_dir, exist_ok=True)
    if gpu_png:
        from .. import png
        if gif:
            raise ValueError("write_frames: the GIF is written from pixels on the host; with gpu_png=True call write_gif for it")
        enc = frames if isinstance(frames, png.HostStreams) else png.encode(frames, swap_rb=True).to_host()
        indices = list(range(len(enc))) if indices is None else list(indices)
        with ThreadPoolExecutor(max_workers=max(1, min(16, workers))) as ex:
            list(ex.map(lambda j: enc.write_png(os.path.join(out_dir, "%s%d.png" % (prefix, indices[j])), j), range(len(enc))))
        return enc
    from PIL import Image
    indices = list(range(len(frames))) if indices is None else list(indices)

    def one(job):
        i, f = job
        Image.fromarray(_bgra_to_rgba(f), "RGBA").save(os.path.join(out_dir, "%s%d.png" % (prefix, i)))
    with ThreadPoolExecutor(max_workers=max(1, workers)) as ex:
        list(ex.map(one, zip(indices, frames)))
    if gif and len(frames):
        write_gif(frames, os.path.join(out_dir, gif))


def write_gif(frames, path):
    from PIL import Image
    ims = [Image.fromarray(_bgra_to_rgba(f), "RGBA") for f in frames]
    ims[0].save(path, save_all=True, append_images=ims[1:], duration=33, loop=0)


def pack_rgba8(out, dst):
    """(rgb [1,H,W,3], depth, alpha [1,H,W], counter) of one frame -> `dst` uint8 [H,W,4] on the device: animate.py:107-113's
    `cat([rgb, alpha[..., None]]) * 255 -> uint8` as ONE launch on the current stream (`ia_pack_rgba8`)."""
    from .. import _lib
    rgb, _, alpha, _ = out
    _lib.require_cuda(rgb, alpha, dst)
    _lib.call("ia_pack_rgba8", rgb, alpha, alpha.numel(), dst)


def pack_normals8(out, rays_d, dst_normal, dst_shaded, light=None):
    """the normal map of a frame rendered with normals=True (`out[4]`) -> two uint8 [H,W,4] images on the device in ONE launch
    (`ia_pack_normals8`): ((n + 1) / 2, covered) and (s, s, s, covered), s = max(0, n . l); l = `light` (device float [3]) or the
    direction towards the camera along every pixel's own ray (-rays_d, the camera-frame directions of the sequence)."""
    from .. import _lib
    nrm = out[4]
    _lib.require_cuda(nrm, rays_d, dst_normal, dst_shaded)
    _lib.call("ia_pack_normals8", nrm, rays_d, light, nrm.numel() // 3, dst_normal, dst_shaded)


def write_normal_frames(normal, shaded, out_dir, indices, workers=8, gpu_png=False):
    """8-bit [n,H,W,4] normal / shaded images -> `normal_<i>.png`, `shaded_<i>.png`.  The channels are written as they are:
    red / green / blue = x / y / z of (n + 1) / 2 in the camera frame (x right, y down, z away from the camera), alpha = covered.
    gpu_png: `normal` and `shaded` are uint8 tensors on the device and are encoded there (no channel swap), see write_frames."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(out_dir, exist_ok=True)
    if gpu_png:
        from .. import png
        indices = list(indices)
        for name, batch in (("normal", normal), ("shaded", shaded)):
            enc = png.encode(batch, swap_rb=False).to_host()
            with ThreadPoolExecutor(max_workers=max(1, min(16, workers))) as ex:
                list(ex.map(lambda j: enc.write_png(os.path.join(out_dir, "%s_%d.png" % (name, indices[j])), j), range(len(enc))))
        return
    from PIL import Image
    jobs = [("normal_%d.png" % i, f) for i, f in zip(indices, normal)] + [("shaded_%d.png" % i, f) for i, f in zip(indices, shaded)]

    def one(job):
        Image.fromarray(np.ascontiguousarray(job[1]), "RGBA").save(os.path.join(out_dir, job[0]))
    with ThreadPoolExecutor(max_workers=max(1, workers)) as ex:
        list(ex.map(one, jobs))


def fixed_jitter(seed, device, iters=5, G=64):
    """One occupancy-probe jitter for the whole sequence (density_grid.py:98 draws a fresh torch.rand per frame): with it a
    frame is a function of its pose alone, so a sequence rendered by 1, 2 or 8 ranks gives the same files."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    return torch.rand((iters, G * G * G, 3), generator=g).to(device)


def _make_renderer(model, first, size, in_flight, probes, jitter, normals=False):
    from ..pipeline import PipelinedRenderer
    return PipelinedRenderer(model, first, size, n_in_flight=in_flight, margin=1, probe_batches=probes, jitter=jitter, normals=normals)


def render_sequence(model, seq, out_dir, gif="animation.gif", launch=None, in_flight=3, jitter=None, make_renderer=None, log=print,
                    max_buffer_bytes=1 << 30, normals=False, gpu_png=False, apng=None):
    """animate.py:104-118 / novel_view.py:117-127 for one rank of a job of `launch.world_size` ranks.

    The frames of `seq` are dealt round-robin to the ranks (parallel.shard_frames; frames are independent: no data-path
    collective).  A rank renders its frames through `pipeline.PipelinedRenderer`: `in_flight` captured HIP graphs replayed
    round-robin on their own streams, so a second frame fills the gaps the latency-bound tail of the first leaves.  Behind
    every frame, on the frame's stream, the image is packed to 8-bit RGBA on the device (pack_rgba8) and copied to pinned
    host memory asynchronously: the loop never waits for the GPU.  Frames whose wave-front loop needed more iterations than
    the graph holds are rendered again eagerly.  Every rank writes its own `<i>.png`; the GIF is written by rank 0 from the
    frames gathered there (RCCL gather of the packed images).
    normals: the surface-normal pass is captured behind every frame and `normal_<i>.png` / `shaded_<i>.png` are written next to
    `<i>.png` (packed on the device by one more launch, copied by the same copier stream; `<i>.png` is what it is without).
    gpu_png: the packed frames of a chunk are PNG-encoded on the device in one batch call once the chunk's render loop has been
    synchronised (`png.encode`); only the compressed streams are copied to the host, where threads frame and write the files.  The
    per-frame copies of raw pixels to pinned memory are not made; a GIF, when one is asked for, still is PIL's, from one copy of the
    frames at the end.  apng: a file name (`animation.png`): rank 0 additionally writes the sequence as one animated PNG from the
    frames' compressed streams, gathered from the ranks as they are (needs gpu_png).
    Returns a dict: frames (of the sequence), local (rendered here), render_s (this rank's render loop, I/O and graph capture
    excluded), write_s (this rank's encoding and file writing, the GIF and the animated PNG included), frames_per_sec (whole job: frames / max over ranks of render_s), incomplete (re-rendered frames)."""
    from .launch import Launch
    from ..parallel import shard_frames
    launch = launch or Launch(device=seq.rays_o.device)
    size = (seq.H, seq.W)
    dev = seq.rays_o.device
    on_gpu = dev.type == "cuda"
    if apng and not gpu_png:
        raise ValueError("render_sequence: apng needs gpu_png=True (the animated PNG is made of the device encoder's streams)")
    to_host = not gpu_png         # the per-frame copies of raw pixels
    streams = []                  # gpu_png: the HostStreams of every chunk, for the animated PNG
    mine = shard_frames(len(seq), launch.rank, launch.world_size)
    n = len(mine)
    # the packed frames stay on the device (the GIF gather travels over RCCL from there) and in pinned host memory (PNG encoding).
    # With a GIF every frame is kept until the end, as the reference does (animate.py:106-116); without one the sequence goes
    # through buffers of at most `max_buffer_bytes` (render a chunk, write its files, reuse the buffers)
    per_frame = seq.H * seq.W * 4 * (3 if normals else 1)
    cap = n if gif else max(1, min(n, int(max_buffer_bytes) // per_frame))
    dev_frames = torch.empty((cap, seq.H, seq.W, 4), dtype=torch.uint8, device=dev)
    host = torch.empty((cap if to_host else 0, seq.H, seq.W, 4), dtype=torch.uint8, pin_memory=on_gpu)
    if normals:      # [0]: normal images, [1]: shaded images
        dev_extra = torch.empty((2, cap, seq.H, seq.W, 4), dtype=torch.uint8, device=dev)
        host_extra = torch.empty((2, cap if to_host else 0, seq.H, seq.W, 4), dtype=torch.uint8, pin_memory=on_gpu)
        rays_d_cam = seq.rays_d.reshape(-1, 3).contiguous()
    sync = torch.cuda.synchronize if on_gpu else (lambda: None)
    render_s, write_s, redo = 0.0, 0.0, []
    if n:
        probes = [seq.batch(mine[(j * max(n // 8, 1)) % n]) for j in range(min(8, n))]   # wave-front loop length over the shard
        renderer = (make_renderer or _make_renderer)(model, seq.batch(mine[0]), size, max(1, min(in_flight, n)), probes, jitter,
                                                     **({"normals": True} if normals else {}))

        # device -> host copies run on their own stream behind an event: a frame's stream goes straight on to its next frame
        # instead of standing still for the PCIe transfer (every frame of a chunk has its own slot: nothing is reused in flight)
        copier = torch.cuda.Stream(device=dev) if (on_gpu and to_host) else None

        def keep(slot):
            def consume(out, k):
                pack_rgba8(out[:4], dev_frames[slot])
                if normals:
                    pack_normals8(out, rays_d_cam, dev_extra[0, slot], dev_extra[1, slot])
                if not to_host:
                    return
                if copier is None:
                    host[slot].copy_(dev_frames[slot])
                    if normals:
                        host_extra[:, slot].copy_(dev_extra[:, slot])
                    return
                ev = torch.cuda.Event()
                ev.record()
                copier.wait_event(ev)
                with torch.cuda.stream(copier):
                    host[slot].copy_(dev_frames[slot], non_blocking=True)
                    if normals:
                        host_extra[0, slot].copy_(dev_extra[0, slot], non_blocking=True)
                        host_extra[1, slot].copy_(dev_extra[1, slot], non_blocking=True)
            return consume
        with torch.inference_mode():
            for c0 in range(0, n, cap):
                c1 = min(n, c0 + cap)
                sync()
                t0 = time.perf_counter()
                for j in range(c0, c1):
                    renderer(seq.batch(mine[j], rays=False), keep(j - c0))
                renderer.synchronize()
                if copier is not None:
                    copier.synchronize()
                render_s += time.perf_counter() - t0
                renderer.finish()
                bad = [c for c in renderer.incomplete_calls if c0 <= c < c1]     # (call number = position in `mine`)
                for c in bad:
                    keep(c - c0)(model.render_image_fast(seq.batch(mine[c]), size, jitter=jitter, **({"normals": True} if normals else {})), 0)
                sync()
                redo += bad
                t0 = time.perf_counter()
                if gpu_png:
                    streams.append(write_frames(dev_frames[:c1 - c0], out_dir, indices=mine[c0:c1], gpu_png=True))
                    if normals:
                        write_normal_frames(dev_extra[0, :c1 - c0], dev_extra[1, :c1 - c0], out_dir, mine[c0:c1], gpu_png=True)
                elif not gif:
                    write_frames(host[:c1 - c0].numpy(), out_dir, indices=mine[c0:c1])
                    if normals:
                        write_normal_frames(host_extra[0, :c1 - c0].numpy(), host_extra[1, :c1 - c0].numpy(), out_dir, mine[c0:c1])
                write_s += time.perf_counter() - t0
    slowest = launch.max_over_ranks(render_s)
    t0 = time.perf_counter()
    if apng:
        _write_apng(streams, seq, launch, os.path.join(out_dir, apng))
    if gif:
        if gpu_png:
            host = dev_frames[:n].cpu()
        else:
            write_frames(host.numpy(), out_dir, indices=mine)
            if normals and n:
                write_normal_frames(host_extra[0].numpy(), host_extra[1].numpy(), out_dir, mine)
        parts = launch.gather_to_main(dev_frames if launch.backend == "nccl" else host)
        if launch.is_main:
            w = launch.world_size
            write_gif([parts[i % w][i // w].numpy() for i in range(len(seq))], os.path.join(out_dir, gif))
    write_s += time.perf_counter() - t0
    launch.barrier()
    res = dict(frames=len(seq), local=n, render_s=render_s, write_s=write_s, frames_per_sec=(len(seq) / slowest if slowest > 0 else 0.0),
               incomplete=len(redo), in_flight=in_flight, world_size=launch.world_size)
    if log is not None and launch.is_main:
        log("rendered %d frames (%dx%d) in %.3f s = %.1f frames/s (%d rank(s), %d in flight per GPU, PNG / GIF I/O and graph capture "
            "excluded; %d re-rendered eagerly)" % (res["frames"], seq.W, seq.H, slowest, res["frames_per_sec"], launch.world_size, in_flight, len(redo)))
    return res


def _write_apng(streams, seq, launch, path, fps=30):
    """the chunks' compressed streams of this rank (`png.HostStreams`, in the order of its frames) -> one animated PNG of the whole
    sequence, written by rank 0: the ranks' payloads and stream sizes are gathered as they are (bytes, not pixels); frame i of the
    sequence is stream i // world_size of rank i % world_size (parallel.shard_frames)"""
    from .. import png
    sizes = [s.offsets[j + 1] - s.offsets[j] for s in streams for j in range(len(s))]
    payload = torch.from_numpy(np.concatenate([np.frombuffer(s.payload, np.uint8) for s in streams] or [np.zeros(0, np.uint8)]).copy())
    parts = launch.gather_to_main(payload)
    counts = launch.gather_to_main(torch.tensor(sizes, dtype=torch.int64))
    if not launch.is_main:
        return
    w = launch.world_size
    ranks = [png.HostStreams(p, [0] + np.cumsum(c.numpy()).tolist(), seq.H, seq.W, 4) for p, c in zip(parts, counts)]
    with open(path, "wb") as f:
        f.write(png.frame_apng([ranks[i % w].stream(i // w) for i in range(len(seq))], seq.H, seq.W, 4, fps=fps, loop=0))


def mesh_preview(model, seq, out_dir, resolution, launch=None, log=print, gpu_png=False):
    """`--mesh-preview`: the canonical mesh is extracted ONCE at lattice `resolution`; every frame is then one forward skinning
    (`pose_mesh`) plus the raster launches (`Mesh.render`) under the sequence's camera, written as `mesh_<i>.png` (vertex colours,
    alpha = covered).  Frames are dealt to the ranks as render_sequence deals them.  Returns a dict like render_sequence's."""
    from .launch import Launch
    from ..parallel import shard_frames
    launch = launch or Launch(device=seq.rays_o.device)
    mine = shard_frames(len(seq), launch.rank, launch.world_size)
    cam = seq.camera()
    dev = seq.rays_o.device
    t0 = time.perf_counter()
    mesh = model.extract_mesh(resolution=resolution)
    torch.cuda.synchronize()
    extract_s = time.perf_counter() - t0
    host = torch.empty((len(mine), seq.H, seq.W, 4), dtype=torch.uint8, **(dict(device=dev) if gpu_png else dict(pin_memory=dev.type == "cuda")))
    t0 = time.perf_counter()
    for j, i in enumerate(mine):
        host[j].copy_(model.pose_mesh(mesh, seq.batch(i, rays=False)).render(cam)["rgba8"], non_blocking=True)
    torch.cuda.synchronize()
    render_s = time.perf_counter() - t0
    if gpu_png:         # (`host` stayed on the device: it is encoded there)
        write_frames(host, out_dir, indices=mine, prefix="mesh_", gpu_png=True)
    else:
        write_frames(host.numpy(), out_dir, indices=mine, prefix="mesh_")
    slowest = launch.max_over_ranks(render_s)
    launch.barrier()
    res = dict(frames=len(seq), local=len(mine), render_s=render_s, extract_s=extract_s, frames_per_sec=(len(seq) / slowest if slowest > 0 else 0.0),
               vertices=int(mesh.verts.shape[0]), faces=int(mesh.faces.shape[0]))
    if log is not None and launch.is_main:
        log("mesh preview: %d vertices, %d faces at lattice %d (extracted once in %.3f s); %d frames (%dx%d) in %.3f s = %.1f frames/s "
            "(%d rank(s); pose_mesh + rasteriser + copy to the host, PNG I/O excluded)" % (res["vertices"], res["faces"], resolution, extract_s,
                                                                                          res["frames"], seq.W, seq.H, slowest, res["frames_per_sec"], launch.world_size))
    return res


def add_png_args(ap, apng_name="animation.png"):
    ap.add_argument("--gpu-png", action="store_true",
                    help="encode the PNG files on the GPU (PNG filters + deflate with run-length matches and dynamic Huffman codes, "
                         "instantavatar_amd.png): only compressed bytes are copied to the host.  Same pixels, other file bytes than PIL's")
    ap.add_argument("--apng", action="store_true", help="also write the sequence as one lossless animated PNG (%s); needs --gpu-png" % apng_name)


def check_png_args(ap, args):
    if args.apng and not args.gpu_png:
        ap.error("--apng needs --gpu-png")


def add_launch_args(ap):
    ap.add_argument("--in-flight", type=int, default=3, help="frames in flight per GPU (captured HIP graphs replayed round-robin on their own streams)")
    ap.add_argument("--normals", action="store_true",
                    help="also write normal_<i>.png (surface normals of the posed density field, (n + 1) / 2 in the camera frame) and "
                         "shaded_<i>.png (max(0, n . l), lit from the camera) next to <i>.png; SNARF deformer only")
    add_png_args(ap)
    ap.add_argument("--jitter-seed", type=int, default=None,
                    help="use ONE occupancy-probe jitter for all frames (drawn from this seed) instead of a fresh draw per frame "
                         "(density_grid.py:98): the files no longer depend on how many ranks rendered the sequence")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", help="npz with `poses` [n,>=72] and `trans` [n,3] (data/animation/aist_demo.npz)")
    ap.add_argument("--ckpt", help="Lightning checkpoint of DNeRFModel")
    ap.add_argument("--betas", help="npz with `betas` (the subject's anim_nerf_train.npz)")
    ap.add_argument("--smpl-dir", default="./data/SMPLX/smpl")
    ap.add_argument("--gender", default="neutral")
    ap.add_argument("--confs", default=os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "confs"))
    ap.add_argument("--deformer", default="fast_snarf")
    ap.add_argument("--network", default="ngp")
    ap.add_argument("--renderer", default="raymarcher_acc")
    ap.add_argument("--synthetic", action="store_true", help="synthetic SMPL-like body + field (no SMPL pickle / checkpoint needed)")
    ap.add_argument("--downscale", type=int, default=2)
    ap.add_argument("--size", type=int, default=0, help="square image edge in pixels (overrides --downscale), e.g. 512")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--out", default="animation/out")
    ap.add_argument("--no-gif", action="store_true")
    ap.add_argument("--subjects", help="BASELINE config 5 (a batch of subjects, one per GPU): a JSON list of per-subject overrides "
                    "[{\"ckpt\": ..., \"betas\": ..., \"gender\": ..., \"out\": ..., (\"poses\": ..., \"seed\": ...)}, ...]; rank r of the job renders "
                    "the WHOLE sequence of subject r (r modulo the list) with that subject's weights into its `out` -- independent "
                    "replicas, no frame sharding, no data-path collective")
    ap.add_argument("--seed", type=int, default=None, help="--synthetic: seed of the synthetic body + field (another seed = another subject)")
    ap.add_argument("--mesh-preview", type=int, default=0, metavar="RES",
                    help="instead of the volumetric frames: extract the canonical mesh once at lattice RES, then per frame pose it and "
                         "rasterise it under the same camera -> mesh_<i>.png; SNARF deformer only")
    add_launch_args(ap)
    args = ap.parse_args(argv)
    check_png_args(ap, args)
    from .launch import Launch
    launch = Launch.from_env(who="animate")
    device = launch.device
    replica = None
    if args.subjects:
        import json
        with open(args.subjects) as f:
            subjects = json.load(f)
        if not isinstance(subjects, list) or not subjects:
            ap.error("--subjects: a non-empty JSON list of objects")
        mine = subjects[launch.rank % len(subjects)]
        unknown = set(mine) - {"ckpt", "betas", "gender", "out", "poses", "seed", "smpl_dir"}
        if unknown:
            ap.error("--subjects: unknown keys %s" % sorted(unknown))
        for k, v in mine.items():
            setattr(args, k, v)
        if "out" not in mine:
            args.out = os.path.join(args.out, "subject_%d" % (launch.rank % len(subjects)))
        replica = Launch(device=device)     # this rank's own one-rank "job": render_sequence deals it every frame
    if not args.synthetic and not (args.ckpt and args.poses):
        ap.error("--ckpt and --poses are required unless --synthetic is given")
    try:
        model, betas = build_model(args, device, quiet=not launch.is_main)
        model.eval()
        track = args.poses
        if not track and args.max_frames > 64:   # a longer synthetic run: the pose track the reference ships (its first 200 frames travel with the tests)
            track = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests", "golden", "aist_demo_200.npz")
        if track:
            z = np.load(track)
            poses, trans = z["poses"].astype(np.float32), z["trans"].astype(np.float32)
        else:
            poses, trans = synthetic.procedural_pose_track(64)
        if args.max_frames:
            poses, trans = poses[:args.max_frames], trans[:args.max_frames]
        seq = AnimateSequence(poses, trans, betas, device, args.downscale, size=args.size or None)
        if args.mesh_preview:
            if replica is not None:
                ap.error("--mesh-preview does not combine with --subjects")
            res = mesh_preview(model, seq, args.out, args.mesh_preview, launch=launch, gpu_png=args.gpu_png)
            if launch.is_main:
                print("wrote %d mesh previews (%dx%d) to %s" % (res["frames"], seq.W, seq.H, args.out))
            return 0
        jitter = None if args.jitter_seed is None else fixed_jitter(args.jitter_seed, device)
        res = render_sequence(model, seq, args.out, gif=None if args.no_gif else "animation.gif", launch=replica or launch,
                              in_flight=args.in_flight, jitter=jitter, log=None if replica else print, normals=args.normals,
                              gpu_png=args.gpu_png, apng="animation.png" if args.apng else None)
        if replica is not None:
            # whole-job figure of the replicas: all frames of all subjects over the slowest rank's render loop
            slowest = launch.max_over_ranks(res["render_s"])
            total = launch.sum_over_ranks(res["frames"])
            print("rank %d: subject %d, %d frames (%dx%d) to %s" % (launch.rank, launch.rank % len(subjects), res["frames"], seq.W, seq.H, args.out))
            launch.barrier()
            if launch.is_main:
                print("rendered %d frames of %d subject replica(s) in %.3f s = %.1f frames/s (one subject per rank; PNG / GIF I/O and graph capture excluded)"
                      % (int(total), launch.world_size, slowest, total / slowest if slowest > 0 else 0.0))
        elif launch.is_main:
            print("wrote %d frames (%dx%d) to %s" % (res["frames"], seq.W, seq.H, args.out))
    finally:
        launch.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
