#!/usr/bin/env python3
"""bench.py -- novel-pose rendering throughput of the InstantAvatar hot path on MI355X.

A "step" is one frame of DNeRFModel.render_image_fast (models/DNeRF.py:72-97) at
512x512: SMPL joint chain -> skinning-voxel precompute -> per-frame occupancy
build (5 x 64^3 probes through the deformer + field) -> occupancy-grid ray march
with Fast-SNARF root finding, hash-grid + MLP field and alpha compositing.
Inputs (camera rays, SMPL poses, weights) are resident in HBM before the timed
region.  Synthetic SMPL-like body, procedural pose track, synthetic field
(see instantavatar_amd/synthetic.py): no dataset / checkpoint exists offline.

  python bench.py --gpus N --steps K --warmup W          # the plain run: set-up, spin-up, W warm-up and K timed frames, the line
  python bench.py --gpus N --steps K --warmup W --full   # + everything else the bench measures, after the timed frames (below)
  (N > 1: one rank per GPU over RCCL; frames are sharded across ranks, no data-path
   collective -> weak scaling.  Under torch.distributed.run the ranks read RANK /
   LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment; started directly with
   --gpus N > 1 the script re-executes itself through torch.distributed.run on
   127.0.0.1 and fails loudly when fewer than N devices exist.)
  python bench.py --gpus N --train-only   # train it/s (configs 2/4) as the headline line
  python bench.py --gpus 2 --dry-run      # launch / sharding / reduction plumbing on gloo, no kernels
  python bench.py ... --dump-outputs DIR  # also write the last timed frame's outputs as DIR/<name>.npy (render paths)

A plain run does only what its headline needs (`metric`, `value`, `ms_per_step` and the statistics of the timed frames).
--full adds, after the timed region and without touching it: the latency of one frame in flight, the procedural pose
track, the instrumented pass with the roofline block and the counter summaries of profiles/, the isolated hash-grid
lookup, the training legs (--train-steps) and the CPU baseline (--cpu-frames).  Both print the same headline.

Prints ONE JSON line (rank 0).
"""
import argparse
import ctypes as C
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np
import torch

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8.0 TB/s spec (6.3 TB/s measured copy)
L2_PEAK_GBS = 34500.0   # MI355X_MICROARCH.md "L2 (per XCD)": ~34.5 TB/s aggregate over the 8 XCDs
MFMA_F16_PEAK_TFLOPS = 2500.0  # dense fp16/bf16 MFMA peak


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--full", action="store_true", help="after the timed steps, also measure everything else this file knows: one frame "
                    "in flight, the procedural pose track, the instrumented pass + roofline, the isolated hash-grid lookup, training "
                    "(--train-steps) and the CPU baseline (--cpu-frames).  Off by default: a plain run stops at its headline line")
    ap.add_argument("--cpu-frames", type=int, default=None, help="with --full: frames timed on the CPU oracle after one warm-up frame "
                    "(0 = skip; minimum 3; default 3)")
    ap.add_argument("--spinup-max-ms", type=float, default=4000.0,
                    help="upper bound of the adaptive, untimed and REPORTED spin-up: 10-frame windows are run until three "
                         "consecutive windows agree within 3 %% (reported as spinup_ms / value_first_window / value_steady)")
    ap.add_argument("--in-flight", type=int, default=3,
                    help="independent frames in flight per GPU (one captured graph and one HIP stream each; 1 = strictly one frame "
                         "after the other).  The frames of a sequence are independent units (animate.py)")
    ap.add_argument("--graph-margin", type=int, default=1, help="wave-front iterations a captured frame holds beyond what the 12 probe "
                    "poses needed (a frame that needs more is detected and rendered again eagerly, inside the timed region)")
    ap.add_argument("--train-only", action="store_true", help="headline = training throughput (rays/s over all ranks)")
    ap.add_argument("--force-collectives", action="store_true", help="with --gpus 1: start a 1-rank RCCL group and take the multi-rank "
                    "training path (bucketed all-reduce from inside the backward, density MAX-reduce) -- the eager-vs-graph gap of the "
                    "N-rank step measured on one GPU")
    ap.add_argument("--tile-shard", action="store_true", help="latency mode (SURVEY 8e, optional): EVERY frame is split by image rows over "
                    "the N ranks (parallel.render_frame_tiled: occupancy build duplicated, blocks all-gathered over RCCL); strong scaling")
    ap.add_argument("--dry-run", action="store_true", help="no kernels: exercises launch, frame sharding and the "
                    "collectives on the gloo backend (CPU test of the N > 1 plumbing)")
    ap.add_argument("--no-profile", action="store_true", help="with --full: skip the instrumented pass (in-library event timing) and "
                    "what is derived from it (roofline, isolated hash-grid lookup)")
    ap.add_argument("--no-graph", action="store_true", help="launch every frame eagerly instead of replaying the captured HIP "
                    "graph (eager: ~110 launches per frame from Python, a few hundred microseconds slower and jittery)")
    ap.add_argument("--train-steps", type=int, default=None,
                    help="with --full: training iterations timed after the render loop (0 = skip).  Default: 100 on one GPU; 0 on "
                         "several -- the frames/s line of a scaling run must not depend on a second workload (use --train-only, or pass "
                         "a count)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step rendered (rank 0: rgb, depth, alpha, counter of its "
                         "frame, float32) as DIR/<name>.npy -- at most 64 MB, a fixed pixel sample of larger frames.  The timed "
                         "frames draw their random numbers from a generator seeded right before the timed region, so the same "
                         "arguments give the same inputs (pose, occupancy-probe jitter) on every run (render paths only)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1 (the number of timed steps)")
    if args.dump_outputs and (args.train_only or args.dry_run):
        ap.error("--dump-outputs writes a rendered frame: not available with --train-only / --dry-run")
    if not args.full and ((args.train_steps or 0) > 0 or (args.cpu_frames or 0) > 0):
        ap.error("--train-steps / --cpu-frames size parts of the --full run: pass --full with them (a plain run measures its headline only)")
    if not args.full:
        args.train_steps = args.cpu_frames = 0
    if args.train_steps is None:
        args.train_steps = 100 if args.gpus == 1 else 0
    if args.cpu_frames is None:
        args.cpu_frames = 3
    return args


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(out_dir, arrays):
    """Writes `arrays` ({name: tensor of one frame, leading dims [..., H, W(, C)]}) as out_dir/<name>.npy in float32.  If they
    exceed DUMP_MAX_BYTES together, the same fixed, seeded sample of pixels is taken from each (sorted flat pixel indices,
    written as pixel_index.npy in float64).  Returns {name: shape} of what was written."""
    os.makedirs(out_dir, exist_ok=True)
    host = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    n_pix = next(iter(host.values())).shape[1] * next(iter(host.values())).shape[2]
    per_pix = sum(a.size // n_pix for a in host.values()) * 4
    if per_pix * n_pix > DUMP_MAX_BYTES:
        keep = np.sort(np.random.RandomState(0).choice(n_pix, (DUMP_MAX_BYTES - (1 << 20)) // (per_pix + 8), replace=False))
        host = {k: a.reshape(a.shape[0], n_pix, -1)[:, keep].reshape((a.shape[0], len(keep)) + a.shape[3:]) for k, a in host.items()}
        host["pixel_index"] = keep.astype(np.float64)
    for k, a in host.items():
        np.save(os.path.join(out_dir, k + ".npy"), a)
    return {k: list(a.shape) for k, a in host.items()}


def cpu_baseline(body, fp, model, poses, tr, res, n_frames):
    """The CPU restatement (oracle/) timed on this box's host cores on a bounded sample of the same workload: one untimed
    warm-up frame, then `n_frames` (>= 3) full frames timed one by one; value = 1 / median frame time (SURVEY 8d protocol)."""
    from oracle import oracle as orc
    from instantavatar_amd import synthetic as syn
    fd = model.deformer.deformer
    init = dict(tfs_inv_t=model.deformer.tfs_inv_t[0].cpu().numpy(),
                lbs_voxel=np.ascontiguousarray(fd.lbs_voxel_final[0].cpu().numpy()),
                offset_kernel=fd.offset_kernel.reshape(3).cpu().numpy().astype(np.float32),
                scale_kernel=fd.scale_kernel.reshape(3).cpu().numpy().astype(np.float32),
                bbox=model.deformer.bbox.cpu().numpy(), D=fd.resolution // 4, H=fd.resolution, W=fd.resolution)
    ro, rd = syn.make_camera_rays(res)
    rng = np.random.RandomState(0)
    orc.lib()
    n_frames = max(int(n_frames), 3)
    times = []
    t_all = time.time()
    for i in range(n_frames + 1):          # frame 0 = warm-up (page faults of the 25 MB grid, OpenMP pool start-up)
        f = (i * 37) % len(poses)
        world = orc.make_world(body, init, fp, np.zeros(10, np.float32), poses[f, 3:], poses[f, :3], tr[f], syn.INIT_BONES)
        jit = rng.rand(5, 64 ** 3, 3).astype(np.float32)
        t0 = time.time()
        orc.render_image_fast(world, ro, rd, jit)
        if i > 0:
            times.append(time.time() - t0)
    med = float(np.median(times))
    cores = os.cpu_count() or 1
    # BASELINE config 1 ("config 1 ... and one 512x512 frame"): a 128 x 128 frame of the body in its
    # canonical pose -- the deformer's transforms are the identity up to the root frame -- with an 8-level hash grid
    cano = orc.smpl_forward(body, np.zeros(10, np.float32), syn.cano_pose("A_pose"), want_verts=False)["joints"]
    fp8 = syn.make_field(np.asarray(cano, np.float32), init["bbox"], seed=42, n_levels=8)
    ro1, rd1 = syn.make_camera_rays(128)
    w1 = orc.make_world(body, init, fp8, np.zeros(10, np.float32), syn.cano_pose("A_pose"), poses[0, :3], tr[0], syn.INIT_BONES)
    t1 = []
    for i in range(4):                     # 1 warm-up + 3
        jit = rng.rand(5, 64 ** 3, 3).astype(np.float32)
        t0 = time.time()
        out1 = orc.render_image_fast(w1, ro1, rd1, jit)
        if i > 0:
            t1.append(time.time() - t0)
    med1 = float(np.median(t1))
    config1 = {"value": 1.0 / med1, "unit": "frames/s", "rays_per_sec": 128 * 128 / med1, "frame_seconds": [round(t, 3) for t in t1],
               "what": "BASELINE config 1: one 128x128 frame, canonical pose (identity deformer transforms), 8-level hash grid + 2x64 MLPs, "
                       "occupancy build + render through oracle/ (C + OpenMP, fp32); 1 warm-up + median of 3"}
    return {"value": 1.0 / med, "unit": "frames/s", "cores": cores, "kind": "port", "config1_128x128_identity_8_levels": config1,
            "sample": ("1 warm-up + %d full %dx%d frames of the bench's pose track (occupancy build + render) through oracle/ -- a C + OpenMP "
                       "restatement of the reference's algorithm (fp32), all host cores; median frame time.  The reference itself has no CPU "
                       "path (its kernels are CUDA-only), so this port stands in for the 'PyTorch-CPU path' of BASELINE.json" % (n_frames, res, res)),
            "frame_seconds": [round(t, 3) for t in times], "seconds": time.time() - t_all}


def train_throughput(model, dev, poses, tr, rank, world_size, n_steps, res=512, n_rays=4096, warmup=3, graphed=True,
                     sampler="patch", refine=False):
    """train.py analogue (configs 2/4): one frame + 4096 rays per step and rank, targets rendered from the synthetic
    field, Adam(lr 1e-2), occupancy update every 20 steps, gradient all-reduce over RCCL.
    sampler="patch": the reference's default data path (confs/SNARF_NGP.yaml -> sampler: patch, 4 patches of 32 x 32
    anchored on mask pixels, random background; peoplesnapshot.py:99-151) through the device-resident frames
    (datasets.DeviceFrames, utils.sampler.PatchSampler).  sampler="uniform": 4096 rays drawn uniformly over the image
    (the lighter workload rounds 1-2 quoted; kept as a secondary figure).
    refine=True: BASELINE config 4 (confs/SNARF_NGP_refine.yaml): an already formed field (the synthetic one, not re-initialised),
    per-frame SMPL parameters as trainable embedding tables started 0.03 rad / 1 cm off the poses the targets were rendered
    at, `sampler: edge` (EdgeSampler 4096 / 0.6 / 0.3 / 16), NGPLoss, Adam with the third parameter group at lr 1e-5, no
    sigma noise and no density regulariser (is_refine); the gradient reaches the SMPL tables through tfs by implicit
    differentiation of the Broyden roots on the fused route."""
    from instantavatar_amd.pipeline import build_synthetic_model, make_batch
    from instantavatar_amd.training import GraphedTrainStep, NeRFLoss, configure_optimizer
    n_frames = 4
    targets = []
    with torch.no_grad():
        for f in range(n_frames):
            b = make_batch(dev, res, poses[f], tr[f])
            rgb, _, alpha, _ = model.render_image_fast(b, (res, res))
            targets.append((b, rgb.reshape(1, -1, 3), alpha.reshape(1, -1)))
    trainee, _, _ = build_synthetic_model(dev, resolution=128, n_levels=16)
    smpl = dict(betas=np.zeros((1, 10), np.float32), body_pose=poses[:n_frames, 3:].copy(),
                global_orient=poses[:n_frames, :3].copy(), transl=tr[:n_frames].copy())
    if refine:
        from instantavatar_amd.models.structures.body_model_param import SMPLParamEmbedding
        from instantavatar_amd.training import NGPLoss
        rs = np.random.RandomState(99)
        smpl = dict(smpl, body_pose=(smpl["body_pose"] + 0.03 * rs.randn(n_frames, 69)).astype(np.float32),
                    global_orient=(smpl["global_orient"] + 0.03 * rs.randn(n_frames, 3)).astype(np.float32),
                    transl=(smpl["transl"] + 0.01 * rs.randn(n_frames, 3)).astype(np.float32))
        trainee.SMPL_param = SMPLParamEmbedding(**{k: torch.as_tensor(v.copy()) for k, v in smpl.items()}).to(dev)
    else:
        trainee.net_coarse.reset_parameters()
    trainee.train()
    from instantavatar_amd.parallel import broadcast_module_state
    broadcast_module_state(trainee, world_size)   # replicas identical to rank 0 (parameters and buffers), not by seed
    opt = configure_optimizer(trainee, smpl_lr=1e-5) if refine else configure_optimizer(trainee)
    loss_fn = (NGPLoss if refine else NeRFLoss)(dict(w_rgb=1.0, w_alpha=0.1, w_reg=0.1))
    g = torch.Generator(device=dev).manual_seed(1234 + rank)
    # one rank: the step is replayed from a captured HIP graph (every 20th step, the occupancy update, runs eagerly);
    # several ranks: eager steps with the bucketed RCCL all-reduce started from inside the backward
    stepper = GraphedTrainStep(trainee, opt, loss_fn, world_size=world_size, enabled=graphed, is_refine=refine)
    if sampler in ("patch", "edge"):
        from instantavatar_amd.datasets.device_frames import DeviceFrames
        from instantavatar_amd.utils.sampler import EdgeSampler, PatchSampler
        imgs = torch.stack([(t[1].reshape(res, res, 3).clamp(0, 1) * 255).round().to(torch.uint8) for t in targets])
        masks = torch.stack([(t[2].reshape(res, res) > 0.5).float() for t in targets])
        K = np.array([[2000.0 * res / 1080, 0, res / 2], [0, 2000.0 * res / 1080, res / 2], [0, 0, 1]])
        smp = (PatchSampler(num_patch=4, patch_size=32, ratio_mask=1, dilate=0) if sampler == "patch" else
               EdgeSampler(num_sample=n_rays, ratio_mask=0.6, ratio_edge=0.3, kernel_size=16))     # confs/sampler/{patch,edge}.yaml
        frames = DeviceFrames(imgs, masks, K, np.eye(4), smpl, smp)
        assert 4 * 32 * 32 == n_rays

        def step(i):   # (after the capture the sampler writes straight into the graph's static input tensors)
            return stepper(frames.batch((i + rank) % n_frames, generator=g, out=stepper.inputs))
    else:
        bg = torch.ones((1, n_rays, 3), device=dev)

        def step(i):
            b, rgb, alpha = targets[(i + rank) % n_frames]
            sel = torch.randint(0, res * res, (n_rays,), device=dev, generator=g)
            dst = stepper.inputs
            if dst is not None:   # graph replay: the ray gathers write straight into the static input tensors
                for k in ("rays_o", "rays_d", "near", "far"):
                    torch.index_select(b[k], 1, sel, out=dst[k])
                torch.index_select(rgb, 1, sel, out=dst["rgb"])
                torch.index_select(alpha, 1, sel, out=dst["alpha"])
                for k in ("global_orient", "body_pose", "transl"):
                    dst[k].copy_(b[k], non_blocking=True)
                return stepper()
            batch = dict(b)
            for k in ("rays_o", "rays_d", "near", "far"):
                batch[k] = b[k][:, sel]
            batch["rgb"], batch["alpha"] = rgb[:, sel], alpha[:, sel]
            batch["bg_color"] = bg
            return stepper(batch)

    from instantavatar_amd import parallel as _par
    if graphed and stepper.enabled and _par.collectives_on(world_size):
        # N ranks: three host-launched steps before anything is captured (step 0 is eager by rule; 1-2 are held back here):
        # a mis-set-up communicator shows up as an ordinary RCCL error in an eager all-reduce, not inside a stream capture
        stepper.enabled = False
        for i in range(3):
            step(i)
        torch.cuda.synchronize()
        torch.distributed.barrier()
        stepper.enabled = True
    for i in range(max(warmup, 3)):
        step(i)
    torch.cuda.synchronize()
    if world_size > 1:
        torch.distributed.barrier()
    # one rank: three timed windows of n_steps (a 70-180 ms window is at the mercy of one host hiccup: the uniform-ray leg read
    # 923 / 1 035 / 1 185 instead of ~1 380 it/s in three of thirty bench runs of round 6 -- the list shows it); several ranks:
    # one barrier-bracketed window
    windows = []
    first = last = None
    for w in range(3 if world_size == 1 else 1):
        t0 = time.perf_counter()
        for i in range(n_steps):
            out = step(warmup + w * n_steps + i)
            if i == 0 and w == 0:
                first = out["mse_loss"].detach().clone()   # (a replayed step returns static output tensors)
            last = out["mse_loss"].detach()
        torch.cuda.synchronize()
        if world_size > 1:
            torch.distributed.barrier()
        windows.append(time.perf_counter() - t0)
    dt = windows[0]      # quoted: the FIRST window (steps 3 .. 3 + n_steps of a fresh model, as rounds 1-5 measured) -- the later windows
                         # are further into training (patch 571 -> 606 -> 620 it/s as the field forms, refinement 919 -> 830 -> 811) and are
                         # listed for the reader, who also sees a host hiccup in the first one by comparing
    if world_size > 1:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        dt = float(t.item())
    r = trainee.renderer
    r._train_counts_check()
    extra = {}
    if refine:
        moved = {k: float((getattr(trainee.SMPL_param, k).weight.detach().cpu() - torch.as_tensor(smpl[k])).abs().max()) for k in ("body_pose", "global_orient", "transl")}
        extra = {"config": "SNARF_NGP_refine (SMPLParamEmbedding + SNARFDeformer, tfs.requires_grad, fused route, is_refine)",
                 "smpl_tables_max_abs_change": moved, "train_overflow": int(r.train_overflow)}
    return {**extra, "it_per_sec": n_steps / dt, "windows_it_per_sec": [round(n_steps / w_, 1) for w_ in windows],
            "rays_per_sec": n_steps * n_rays * world_size / dt, "steps": n_steps,
            "rays_per_step_per_gpu": n_rays, "sampler": sampler, "mse_first": float(first), "mse_last": float(last),
            "samples_candidates_last_step": list(getattr(r, "last_train_counts", ()) or ()),
            "launch_mode": ("hip_graph (%d replays, %d eager steps)" % (stepper.replays, stepper.eager_steps)) if stepper.replays
                           else "eager", "graph_capture_error": stepper.capture_error,
            "graph_collectives": bool(stepper.replays) and _par.collectives_on(world_size),
            "note": "global batch = n_gpus x 4096 rays (weak scaling); occupancy update every 20 steps included"}


def fit_stage_throughput(dev, n_steps, res=256, n_frames=4, warmup=25, graphed=True):
    """it/s of the fit stage (drivers/fit.py: `training_step` with the SMPLDeformer plugin, SMPLParamEmbedding tables for betas /
    pose / translation under optimisation, NGPLoss with the depth term, PatchSampler 4 x 32^2) on synthetic frames: the body model
    forward + backward as `ia_smpl_lbs_fwd/_bwd`, the render over compact samples (`render_train_fused_smpl`), the step replayed
    from a captured HIP graph (as drivers/fit.py runs it).  Wall clock of `n_steps` steps between two device
    synchronisations; median of three such windows."""
    from instantavatar_amd.drivers import fit as fit_driver
    from instantavatar_amd.training import NGPLoss, configure_optimizer, training_step
    frames, body_model, _ = fit_driver.synthetic_frames(dev, res=res, n_frames=n_frames, noise=0.02, patch=32)
    model = fit_driver.build_fit_model(frames, body_model, dev)
    opt = configure_optimizer(model, lr=1e-3, smpl_lr=1e-4)
    loss_fn = NGPLoss(dict(w_rgb=1.0, w_alpha=0.1, w_reg=0.1, w_lpips=0.0, w_depth_reg=0.01))
    model.train()
    from instantavatar_amd.training import GraphedTrainStep
    stepper = GraphedTrainStep(model, opt, loss_fn, enabled=graphed)
    first = last = None
    for it in range(warmup):
        out = stepper(frames.batch(it % n_frames, out=stepper.inputs))
        first = float(out["mse_loss"]) if first is None else first
    torch.cuda.synchronize()
    r0, e0 = stepper.replays, stepper.eager_steps
    windows, it0 = [], warmup
    for _ in range(3):     # three timed windows, the median is quoted (a 0.15 s window is at the mercy of one slow eager update step)
        t0 = time.perf_counter()
        for it in range(it0, it0 + n_steps):
            out = stepper(frames.batch(it % n_frames, out=stepper.inputs))
        torch.cuda.synchronize()
        windows.append(time.perf_counter() - t0)
        it0 += n_steps
    dt = sorted(windows)[1]
    last = float(out["mse_loss"])
    mode = ("hip_graph (%d replays, %d eager steps, %d graphs)" % (stepper.replays - r0, stepper.eager_steps - e0, len(stepper.graphs))
            if stepper.enabled else "eager")
    return {"it_per_sec": n_steps / dt, "ms_per_step": dt / n_steps * 1e3, "steps": n_steps, "mse_first": first, "mse_last": last,
            "windows_it_per_sec": [round(n_steps / w, 1) for w in windows],
            "config": "SNARF_NGP_fitting analogue: SMPLDeformer + SMPLParamEmbedding (betas, pose, transl optimised), %d frames %dx%d, 4 x 32^2 patches"
                      % (n_frames, res, res), "launch_mode": mode, "graph_capture_error": stepper.capture_error}


def frame_coherent_samples(model, batch, res):
    """Canonical-space field samples of one real frame, in the order the pipeline produces them:
    for every ray that hits the body a run of march steps around the rendered depth (ray-major,
    step-minor), mapped to canonical space by the search kernel -> compact candidate list."""
    from instantavatar_amd.models.structures.utils import Rays
    rgb, depth, alpha, counter = model.render_image_fast(batch, (res, res))
    rays = Rays(o=batch["rays_o"], d=batch["rays_d"], near=batch["near"], far=batch["far"])
    model.deformer.transform_rays_w2s(rays)
    sel = (alpha.reshape(-1) > 0.5).nonzero().reshape(-1)
    o, d = rays.o.reshape(-1, 3)[sel], rays.d.reshape(-1, 3)[sel]
    S = 64
    ks = (torch.arange(S, device=o.device, dtype=torch.float32) - 8) * (2.0 / 256)  # step = (far - near) / MAX_SAMPLES
    t = depth.reshape(-1)[sel][:, None] + ks[None]
    pts = (o[:, None] + d[:, None] * t[..., None]).reshape(-1, 3).contiguous()
    sc = model.deformer.search_compact(pts)
    n = int(sc["n_cand"].item())
    return sc["cand_xc"][:n].contiguous()


def _time_encode(net, x, reps=20):
    with torch.no_grad():
        for _ in range(3):
            net.encode_planes(x)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            net.encode_planes(x)
        b.record()
        torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3  # us


def _morton_order(x, bb):
    """Permutation that sorts the points by the 30-bit Morton code of their position in the box, and the time of
    building it (quantise + interleave + sort, torch ops) in microseconds."""
    def spread(v):  # 10 bits -> every third bit
        v = (v | (v << 16)) & 0x030000FF
        v = (v | (v << 8)) & 0x0300F00F
        v = (v | (v << 4)) & 0x030C30C3
        v = (v | (v << 2)) & 0x09249249
        return v
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    q = ((x - bb[0]) / (bb[1] - bb[0]) * 1023.0).clamp_(0, 1023).to(torch.int64)
    code = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
    order = torch.argsort(code)
    torch.cuda.synchronize()
    return order, (time.perf_counter() - t0) * 1e6


def hashgrid_roofline(model, dev, n=1 << 20, reps=20, frame_batch=None, res=512):
    """The hash-grid lookup in isolation (north_star: fraction of the HBM roofline on the hash-grid
    lookup): the XCD-sharded encoding kernel timed with events on the launch stream, (a) on 2^20 uniformly
    random points of the field's bounding box -- the worst case, no two samples share a fine-level line --
    and (b) on the canonical samples of a real 512^2 frame in pipeline order.  Algorithmic bytes = 512 B per
    sample; `frac` is the random-point figure."""
    net = model.net_coarse
    bb = model.deformer.bbox
    g = torch.Generator(device=dev).manual_seed(7)
    x = torch.rand((n, 3), device=dev, generator=g) * (bb[1] - bb[0]) + bb[0]
    # the encoder's XCD balance is a caller's hint (ia_field.enc_split): the path's samples are spatially coherent (3 tiles of four
    # of the second level group to the XCDs that own the cheap coarse hashed levels), these random points are not (2) -- with the
    # product's setting they take `avg_launch_us_with_coherent_hint`
    us_hint = None
    if hasattr(net, "sample_coherence"):
        us_hint = _time_encode(net, x, reps)
        net.sample_coherence(False)
    try:
        us = _time_encode(net, x, reps)
    finally:
        if hasattr(net, "sample_coherence"):
            net.sample_coherence(True)
    gbs = n * 512 / (us * 1e-6) / 1e9
    out = {"kernel": "k_encode_xcd", "samples": n, "avg_launch_us": us, "enc_split": 2, "avg_launch_us_with_coherent_hint": us_hint,
           "Gsamples_per_s": n / us * 1e-3, "bound": "hbm",
           "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
           "note": ("the 26 MB fp16 table is served from the per-XCD L2s (one hashed level per XCD): the binding limit is the "
                    "L2 request rate (see l2_*, profiles/)")}
    if frame_batch is not None:
        try:
            xc = frame_coherent_samples(model, frame_batch, res)
            if xc.shape[0] >= 8192:
                usc = _time_encode(net, xc, reps)
                gc = xc.shape[0] * 512 / (usc * 1e-6) / 1e9
                out["frame_coherent"] = {"samples": int(xc.shape[0]), "avg_launch_us": usc, "enc_split": int(getattr(net, "enc_split", 2)),
                                         "Gsamples_per_s": xc.shape[0] / usc * 1e-3,
                                         "achieved": gc, "frac": gc / HBM_PEAK_GBS,
                                         "what": "canonical candidates of one 512x512 frame (64 march steps around the surface of "
                                                 "every hit ray, ray-major), as the render loop feeds them to the encoder"}
        except Exception as e:  # never let the auxiliary figure kill the bench line
            out["frame_coherent"] = {"error": repr(e)[:200]}
    try:
        # cell binning (SURVEY 7 / VERDICT r01 weak 5): the same random points in 30-bit Morton order, so that the
        # lanes of a wave sit in one small cube -- what binning can buy at most; the sort is timed beside it
        order, sort_us = _morton_order(x, bb)
        usm = _time_encode(net, x[order].contiguous(), reps)          # (coherent again: the product's hint)
        gm = n * 512 / (usm * 1e-6) / 1e9
        out["morton_binned"] = {"avg_launch_us": usm, "Gsamples_per_s": n / usm * 1e-3, "achieved": gm, "frac": gm / HBM_PEAK_GBS,
                                "binning_us_torch_sort": sort_us,
                                "what": "the same 2^20 random points sorted by Morton code first (the sort is not part of avg_launch_us)"}
    except Exception as e:
        out["morton_binned"] = {"error": repr(e)[:200]}
    cj, src = _profile_json("pmc_encode", ("ia_field.hip",))
    out["counters_source"] = src
    if cj is not None:
        try:
            c = cj["k_encode_xcd<16>"]
            req = c["l2_read_requests_per_sample"]
            out.update(l2_hit_rate=c["l2_hit_rate"], l2_read_requests_per_sample=req,
                       l2_request_rate_frac=req * n / (us * 1e-6) / 269e9, l2_request_ceiling="8 XCD x 16 channels x 2.1 GHz = 269 G/s",
                       traffic=c["fabric_fetch_bytes_per_launch_x2_corrected"], traffic_source=src)
            cc = cj.get("k_encode_xcd<16>/frame_coherent")
            if cc and isinstance(out.get("frame_coherent"), dict) and "avg_launch_us" in out["frame_coherent"]:
                fc = out["frame_coherent"]
                # requests per sample from the counter pass (same sample set), rate from THIS run's launch time
                fc.update(l2_read_requests_per_sample=cc.get("l2_read_requests_per_sample"), l1_accesses_per_sample=cc.get("l1_accesses_per_sample"),
                          l2_hit_rate=cc.get("l2_hit_rate"),
                          l2_request_rate_frac=(cc["l2_read_requests_per_sample"] * fc["samples"] / (fc["avg_launch_us"] * 1e-6) / 269e9
                                                if cc.get("l2_read_requests_per_sample") else None),
                          stall=("TCP_PENDING_STALL_CYCLES = 49 % of the vector L1's cycles, mean TCP->TCC round trip 198 clk, ~47 L2 requests in "
                                 "flight per CU (Little): the L1's outstanding-miss capacity x the L2 latency bounds the request rate; 65 % of "
                                 "the wave cycles wait for an issue slot behind it (profiles/r04_pmc_encode_stall/)"))
        except Exception:
            pass
    return out


def rank_report(rank, world_size, dev, extra):
    """One record per rank, gathered on rank 0 and echoed by every rank on stderr: what each process really saw (device, RCCL
    world size and backend, its own counts), so that a scaling run explains itself without the builder present."""
    import torch.distributed as dist
    rec = {"rank": rank, "shared_device_dev_mode": os.environ.get("IA_BENCH_SHARE_DEVICE") == "1",
           "device": (torch.cuda.get_device_name(dev) if dev is not None else "cpu (dry run)"), "device_index": (dev.index if dev is not None else None),
           "world_size_seen": (dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1),
           "backend": (dist.get_backend() if dist.is_available() and dist.is_initialized() else None),
           "hsa_ipc_legacy": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY"), "pid": os.getpid()}
    rec.update(extra)
    print("[bench rank %d/%d] %s" % (rank, world_size, json.dumps(rec)), file=sys.stderr, flush=True)
    if world_size > 1:
        got = [None] * world_size
        dist.all_gather_object(got, rec)
        return got
    return [rec]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def relaunch_distributed(args):
    """`python bench.py --gpus N` started directly (no WORLD_SIZE): run N ranks of this script on this
    node through torch.distributed.run, rendezvous on 127.0.0.1, and return their exit code."""
    if not args.dry_run and os.environ.get("IA_BENCH_SHARE_DEVICE") != "1":
        n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if n_dev < args.gpus:
            raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node" % (args.gpus, n_dev))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def dry_run(args, rank, world_size):
    """--dry-run: the multi-rank plumbing of the bench without a single kernel (gloo, CPU): process-group
    start-up, round-robin frame sharding, barrier-bracketed timing with the MAX over ranks, the gradient
    average / density MAX / parameter broadcast helpers.  A "frame" is a 1 ms sleep."""
    import torch.distributed as dist
    from instantavatar_amd.parallel import broadcast_module_state, reduce_density_cache, shard_frames
    from instantavatar_amd.training import all_reduce_grads
    if world_size > 1:
        dist.init_process_group("gloo")
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)
    if os.environ.get("IA_BENCH_CHILD") == "1":
        # the child job of supervised_train, without kernels: its own group came up (on its own port), one collective, one line
        t = torch.ones(1)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"metric": "train_rays_per_sec", "dry_run": True,
                              "train": {"it_per_sec": 1.0, "rays_per_sec": 4096.0 * world_size, "ranks_in_child_group": int(t.item()),
                                        "graph_collectives": os.environ.get("IA_GRAPH_COLLECTIVES", "1") != "0"}}))
        dist.destroy_process_group()
        return
    if args.train_only and world_size > 1:
        tr_res, sup = supervised_train(args, rank, world_size, max(args.steps, 1), dry=True)
        if rank == 0:
            print(json.dumps({"metric": "train_rays_per_sec", "value": (tr_res or {}).get("rays_per_sec"), "n_gpus": world_size, "dry_run": True,
                              "train": dict(tr_res or {}, supervised=sup)}))
        dist.barrier()
        dist.destroy_process_group()
        return
    n_total = args.steps + args.warmup
    my = shard_frames(n_total * world_size, rank, world_size)
    assert len(my) == n_total
    torch.manual_seed(100 + rank)            # deliberately different replicas ...
    toy = torch.nn.Linear(8, 4)
    broadcast_module_state(toy, world_size)   # ... made identical by the start-up broadcast
    toy(torch.full((2, 8), float(rank + 1))).sum().backward()
    all_reduce_grads(toy, world_size)
    dens = torch.zeros(2, 2, 2)
    dens.view(-1)[rank % 8] = 1.0 + rank
    reduce_density_cache(dens, world_size)
    for _ in range(args.warmup):
        time.sleep(0.001)
    if world_size > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        time.sleep(0.001)
    if world_size > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    counts = [len(my) - args.warmup]
    checks = [float(toy.weight.sum()), float(toy.weight.grad.sum()), float(dens.sum())]
    if world_size > 1:
        t = torch.tensor([dt], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        gathered = [None] * world_size
        dist.all_gather_object(gathered, (counts[0], checks))
        counts = [g[0] for g in gathered]
        assert all(abs(g[1][k] - checks[k]) < 1e-6 for g in gathered for k in range(3)), "replicas differ after the collectives"
    ranks = rank_report(rank, world_size, None, {"frames_timed": len(my)})
    if rank == 0:
        print(json.dumps({"metric": "novel_pose_render_frames_per_sec_512x512", "value": sum(counts) / dt, "unit": "frames/s",
                          "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
                          "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                          "config": {"workload": "DRY RUN (no kernels; 1 ms sleep per frame)", "frames_sharded_over": world_size},
                          "dry_run": True, "frames_per_rank": counts, "backend": "gloo", "ranks": ranks}))
    if world_size > 1:
        dist.destroy_process_group()


def supervised_train(args, rank, world_size, train_steps, dry=False):
    """N > 1: the training measurement runs in a CHILD job -- every rank starts `bench.py --train-only` again as its own
    child (same RANK / LOCAL_RANK / WORLD_SIZE, the next rendezvous port), the children form their own RCCL group and
    rank 0's child prints the line this rank parses.  The parents only watch: a child that does not finish within
    IA_BENCH_CHILD_TIMEOUT seconds (default 300; a hung stream capture of the RCCL collectives is the case this is for --
    GraphedTrainStep has replayed captured collectives with a 1-rank group only) is killed BY PID, the parents agree (MIN
    over ranks) that the attempt failed, and the phase is executed again with IA_GRAPH_COLLECTIVES=0 (eager N-rank steps).
    A capture that merely FAILS is handled inside the child (GraphedTrainStep: the ranks agree and all launch eagerly).
    Returns (the child's `train` dict on rank 0 / None elsewhere, report dict)."""
    import torch.distributed as dist
    timeout = float(os.environ.get("IA_BENCH_CHILD_TIMEOUT", "300"))
    base_port = int(os.environ.get("MASTER_PORT", "29500"))
    report = {"attempts": [], "timeout_s": timeout}
    for attempt, graph_coll in enumerate(("1", "0")):
        if attempt == 0 and os.environ.get("IA_GRAPH_COLLECTIVES", "1") == "0" and "IA_TEST_CHILD_HANG_RANK" not in os.environ:
            continue      # already asked for eager collectives: a single attempt
        # (without torchrun's TORCHELASTIC_* variables: with TORCHELASTIC_USE_AGENT_STORE the ranks would look for the AGENT's
        # store on the new port, where nobody listens -- the children rendezvous on their own, rank 0's child hosts the store)
        env = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC_")}
        env.update(IA_BENCH_CHILD="1", IA_BENCH_ATTEMPT=str(attempt), IA_GRAPH_COLLECTIVES=graph_coll, MASTER_PORT=str(base_port + 101 + attempt))
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", str(world_size), "--train-only", "--steps", str(train_steps),
               "--warmup", str(max(args.warmup, 3)), "--res", str(args.res)] + (["--no-graph"] if args.no_graph else []) + (["--dry-run"] if dry else [])
        t0 = time.perf_counter()
        proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=sys.stderr, text=True)
        out, state = "", "ok"
        try:
            out, _ = proc.communicate(timeout=timeout)
            if proc.returncode != 0:
                state = "exit code %d" % proc.returncode
        except subprocess.TimeoutExpired:
            proc.kill()           # the exact process this rank started
            out, _ = proc.communicate()
            state = "no result after %.0f s: killed" % timeout
        ok = torch.tensor([1.0 if state == "ok" else 0.0], device=("cuda" if dist.get_backend() == "nccl" else "cpu"))
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        report["attempts"].append({"IA_GRAPH_COLLECTIVES": graph_coll, "this_rank": state, "all_ranks_ok": bool(ok.item()),
                                   "seconds": round(time.perf_counter() - t0, 1)})
        if bool(ok.item()):
            train = None
            if rank == 0:
                lines = [ln for ln in out.splitlines() if ln.startswith("{")]
                train = json.loads(lines[-1]).get("train") if lines else {"error": "the child printed no line"}
            return train, report
    return ({"error": "both attempts failed"} if rank == 0 else None), report


def _device_code():
    """{translation unit: hash of its gfx950 code objects} of the library this process RUNS (ia_source_manifest)"""
    from instantavatar_amd import _lib
    m = _lib.lib().ia_source_manifest().decode()
    return {kv.split("=")[0]: kv.split("=")[1].split(":")[-1] for kv in m.split(";") if "=" in kv}


_DEV_CODE = [None]
PMC_ROUNDS = ("r06", "r05", "r04", "r03")


def _profile_json(stem, tus):
    """A committed PMC summary under profiles/ (rocprofv3 --pmc passes, tools/pmc_all.sh), newest round first -- accepted
    ONLY when it was collected on the device code this process runs: a summary carries the per-translation-unit hashes of
    the gfx950 code objects of the library it was collected on (instantavatar_amd/build.py: sha256 of `.hip_fatbin`), and
    those of the translation units `tus` that hold the profiled kernels must equal the running library's.  A rebuild of
    the same sources anywhere keeps the evidence, a changed kernel drops it.
    Returns (summary or None, source string saying which file was used or why none was)."""
    if _DEV_CODE[0] is None:
        _DEV_CODE[0] = _device_code()
    mine = _DEV_CODE[0]
    why = "no PMC summary under profiles/ (tools/pmc_all.sh)"
    for r in PMC_ROUNDS:
        n = "%s_%s.json" % (r, stem)
        p = os.path.join(ROOT, "profiles", n)
        if not os.path.exists(p):
            continue
        try:
            j = json.load(open(p))
        except Exception:
            continue
        theirs = j.get("device_code")
        if not isinstance(theirs, dict):
            why = "profiles/%s carries no device-code hashes (collected before round 4): not quoted" % n
            continue
        bad = [t for t in tus if not mine.get(t) or mine.get(t) in ("?",) or theirs.get(t) != mine.get(t)]
        if not bad:
            return j, "profiles/%s (device code of %s = %s)" % (n, "+".join(tus), "+".join(mine[t] for t in tus))
        why = ("profiles/%s was collected on other device code of %s (%s, this library: %s): not quoted" %
               (n, bad[0], theirs.get(bad[0]), mine.get(bad[0])))
    return None, why


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(relaunch_distributed(args))
    world_size = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world_size != args.gpus:
        raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world_size))
    if os.environ.get("IA_TEST_CHILD_HANG_RANK") == str(rank) and os.environ.get("IA_BENCH_CHILD") == "1" and os.environ.get("IA_BENCH_ATTEMPT") == "0":
        time.sleep(10 ** 6)   # test hook: this rank's FIRST child never gets anywhere -- what a hung stream capture looks like from outside
    if args.dry_run:
        return dry_run(args, rank, world_size)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (the product path has no CPU fallback)")
    from instantavatar_amd import build as _ia_build
    _ia_build.ensure_current(verbose=(rank == 0))   # (a snapshot may carry a library built before the last source edit; lock-protected)
    # IA_BENCH_SHARE_DEVICE=1 (development / tests/test_gpu_collectives.py): all ranks of an N > 1 run share cuda:0 and talk
    # over gloo -- RCCL refuses two ranks on one device.  Exercises the N-rank control flow of this file with the real kernels
    # on a one-GPU box (sharding, gathers, barriers, per-rank reports, the eager N-rank training step); the numbers it prints
    # are NOT scaling figures and the line says so.
    share = os.environ.get("IA_BENCH_SHARE_DEVICE") == "1" and world_size > 1
    if share:
        local_rank = 0
        os.environ["IA_GRAPH_COLLECTIVES"] = "0"     # gloo collectives cannot be captured into a HIP graph
    if torch.cuda.device_count() <= local_rank:
        raise SystemExit("bench.py: rank %d needs GPU %d, %d visible" % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world_size > 1:
        import torch.distributed as dist
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        assert dist.get_world_size() == args.gpus
    elif args.force_collectives:
        import torch.distributed as dist
        from instantavatar_amd import parallel
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        parallel.FORCE_COLLECTIVES = True

    from instantavatar_amd import _lib, synthetic as syn
    from instantavatar_amd.pipeline import build_synthetic_model, make_batch

    torch.manual_seed(42 + rank)
    model, body, fp = build_synthetic_model(dev, resolution=128, n_levels=16)
    res = args.res
    n_total = args.steps + args.warmup
    track = os.path.join(ROOT, "tests", "golden", "aist_demo_200.npz")
    poses, tr = syn.load_animation_track(track)          # BASELINE config 3 / SURVEY 8(d): first 200 frames of aist_demo.npz

    def max_over_ranks(x):
        if world_size > 1:
            t = torch.tensor([x], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
            return float(t.item())
        return x

    if args.tile_shard:
        # one frame at a time, all ranks on it: frames/s = 1 / latency.  Eager launches (the tiles' geometry differs per rank).
        from instantavatar_amd.parallel import render_frame_tiled, shard_rows
        gj = torch.Generator(device=dev)

        def frame(i):
            f = i % len(poses)
            gj.manual_seed(1000 + i)            # the SAME occupancy jitter on every rank: the grids must agree
            jit = torch.rand((5, 64 ** 3, 3), device=dev, generator=gj)
            return render_frame_tiled(model, make_batch(dev, res, poses[f], tr[f]), (res, res), world_size, rank, jitter=jit)
        for i in range(max(args.warmup, 2)):
            out = frame(i)
        torch.cuda.synchronize()
        if world_size > 1:
            torch.distributed.barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            out = frame(args.warmup + i)
        torch.cuda.synchronize()
        if world_size > 1:
            torch.distributed.barrier()
        dt = max_over_ranks(time.perf_counter() - t0)
        dumped = None
        if args.dump_outputs and rank == 0:
            dumped = {"dir": args.dump_outputs, "frame": (args.warmup + args.steps - 1) % len(poses),
                      "arrays": dump_outputs(args.dump_outputs, dict(zip(("rgb", "depth", "alpha", "counter"), out)))}
        ranks = rank_report(rank, world_size, dev, {"rows": list(shard_rows(res, rank, world_size)), "alpha_coverage_whole_frame": float((out[2] > 0.5).float().mean())})
        if rank == 0:
            print(json.dumps({"metric": "novel_pose_frame_latency_frames_per_sec_%dx%d_row_sharded" % (res, res), "value": args.steps / dt, "unit": "frames/s",
                              "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
                              "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                              "config": {"workload": "render_image_fast %dx%d, ONE frame at a time split by image rows over %d rank(s) (occupancy build on "
                                                     "every rank, row blocks all-gathered), eager launches, aist_demo.npz[:200]" % (res, res, world_size),
                                         "rows_per_rank": [list(shard_rows(res, r, world_size)) for r in range(world_size)]},
                              "ranks": ranks, "dump_outputs": dumped}))
        if world_size > 1:
            torch.distributed.destroy_process_group()
        return

    is_child = os.environ.get("IA_BENCH_CHILD") == "1"
    if args.train_only and world_size > 1 and not is_child:
        tr_res, sup = supervised_train(args, rank, world_size, max(args.steps, 1))
        if rank == 0:
            tr_res = dict(tr_res or {}, supervised=sup)
            it = tr_res.get("it_per_sec")
            print(json.dumps({"metric": "train_rays_per_sec", "value": tr_res.get("rays_per_sec"), "unit": "rays/s", "n_gpus": world_size,
                              "steps": args.steps, "warmup": args.warmup, "ms_per_step": (1e3 / it if it else None),
                              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                              "config": {"workload": "training_step, 4096 rays per step and GPU (PatchSampler 4 x 32 x 32 on %dx%d frames resident in "
                                                     "HBM), SNARF_NGP defaults, Adam, occupancy update every 20 steps, RCCL gradient "
                                                     "all-reduce; measured in a supervised child job (bench.supervised_train)" % (args.res, args.res)},
                              "train": tr_res}))
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
        return
    if args.train_only:
        tr_res = train_throughput(model, dev, poses, tr, rank, world_size, max(args.steps, 1), res=res, warmup=max(args.warmup, 3),
                                  graphed=not args.no_graph)
        if not args.no_graph and (world_size > 1 or args.force_collectives):
            # the same N-rank step launched eagerly (~60 launches + the collectives from Python): the gap a captured step closes
            from instantavatar_amd import parallel as par
            par.EXPOSED_EVENTS = []
            e = train_throughput(model, dev, poses, tr, rank, world_size, max(args.steps, 1), res=res, warmup=max(args.warmup, 3), graphed=False)
            torch.cuda.synchronize()
            mean_ms, max_ms = par.exposed_allreduce_ms(par.EXPOSED_EVENTS)
            par.EXPOSED_EVENTS = None
            tr_res["eager"] = {k: e[k] for k in ("it_per_sec", "rays_per_sec", "launch_mode")}
            # how long the compute stream stood still per step for gradient transfers the backward did not hide (the last
            # bucket: levels 0-3 + the MLP weights; the three 16.8 MB level groups travel under the scatter of the next one)
            tr_res["eager"]["exposed_allreduce_ms_per_step"] = {"mean": mean_ms, "max": max_ms}
            tr_res["collectives"] = "RCCL, %d rank(s)%s" % (world_size, " (forced on one rank)" if args.force_collectives else "")
        tr_res["ranks"] = rank_report(rank, world_size, dev, {"train_steps": int(tr_res["steps"]), "it_per_sec_local_clock": tr_res["it_per_sec"],
                                                               "exposed_allreduce_ms_per_step": (tr_res.get("eager") or {}).get("exposed_allreduce_ms_per_step")})
        if rank == 0:
            print(json.dumps({"metric": "train_rays_per_sec", "value": tr_res["rays_per_sec"], "unit": "rays/s", "n_gpus": world_size,
                              "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 / tr_res["it_per_sec"],
                              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
                              "config": {"workload": "training_step, %d rays per step and GPU (PatchSampler 4 x 32 x 32 on %dx%d frames resident in "
                                                     "HBM), SNARF_NGP defaults, Adam, occupancy update every 20 steps, RCCL gradient "
                                                     "all-reduce" % (4096, res, res)},
                              "train": tr_res}))
        if world_size > 1 or args.force_collectives:
            torch.distributed.destroy_process_group()
        return

    # frames are sharded round-robin over ranks (config 3: embarrassingly parallel)
    from instantavatar_amd.parallel import shard_frames
    my = shard_frames(n_total * world_size, rank, world_size)
    batches = [make_batch(dev, res, poses[f % len(poses)], tr[f % len(poses)]) for f in my[:8]]
    # share the (identical) camera rays between batches: one resident copy
    for b in batches[1:]:
        b["rays_o"], b["rays_d"] = batches[0]["rays_o"], batches[0]["rays_d"]
    pose_t = torch.as_tensor(poses, device=dev)
    tr_t = torch.as_tensor(tr, device=dev)

    # near / far per frame: constant tensors per distinct camera distance, made once (no fill kernels in the frame loop)
    _nf = {}

    def near_far(d):
        # Dead inputs of this path: transform_rays_w2s recomputes near / far from the ray origins in the SMPL-root frame
        # (snarf_deformer.py:101-103; the reference overwrites the batch's values the same way), so every frame is handed the SAME
        # two tensors.  Rounds 1-5 filled a fresh pair per distinct camera distance -- with a moving root (every aist_demo frame has
        # its own) two 1 MB fill kernels per frame for tensors nobody reads.
        if not _nf:
            _nf[0] = (torch.full_like(batches[0]["near"], d - 1), torch.full_like(batches[0]["far"], d + 1))
        return _nf[0]

    frame_inputs = [dict(batches[0]) for _ in range(max(args.in_flight, 1))]  # one input dict per frame in flight

    def frame(i, consume=None):
        f = my[i % n_total] % len(poses)
        b = batches[i % len(batches)]
        b["global_orient"], b["body_pose"], b["transl"] = pose_t[f:f + 1, :3], pose_t[f:f + 1, 3:], tr_t[f:f + 1]
        d = float(np.sqrt((tr[f] ** 2).sum()))
        b["near"], b["far"] = near_far(d)
        out = model.render_image_fast(b, (res, res))
        if consume is not None:
            consume(out, 0)
        return out, 0

    L = _lib.lib()
    eager_frame = frame
    graphed = None
    mode = "eager"
    if not args.no_graph:
        try:
            from instantavatar_amd.pipeline import GraphedRenderer
            # iteration count of the wave-front loop measured on 12 poses spread over this rank's frames
            probes = []
            for j in range(12):
                f = my[(j * max(n_total // 12, 1)) % n_total] % len(poses)
                pb = dict(batches[0])
                d = float(np.sqrt((tr[f] ** 2).sum()))
                pb["global_orient"], pb["body_pose"], pb["transl"] = pose_t[f:f + 1, :3], pose_t[f:f + 1, 3:], tr_t[f:f + 1]
                pb["near"], pb["far"] = torch.full_like(batches[0]["near"], d - 1), torch.full_like(batches[0]["far"], d + 1)
                probes.append(pb)
            if args.in_flight > 1:
                from instantavatar_amd.pipeline import PipelinedRenderer
                graphed = PipelinedRenderer(model, batches[0], (res, res), n_in_flight=args.in_flight, margin=args.graph_margin, probe_batches=probes)
            else:
                graphed = GraphedRenderer(model, batches[0], (res, res), margin=args.graph_margin, probe_batches=probes)

            def frame(i, consume=None):  # noqa: F811  (same work, replayed from the captured HIP graph(s))
                f = my[i % n_total] % len(poses)
                d = float(np.sqrt((tr[f] ** 2).sum()))
                b = frame_inputs[i % len(frame_inputs)]
                b["global_orient"], b["body_pose"], b["transl"] = pose_t[f:f + 1, :3], pose_t[f:f + 1, 3:], tr_t[f:f + 1]
                b["near"], b["far"] = near_far(d)
                if args.in_flight > 1:
                    return graphed(b, consume)
                out = graphed(b)
                if consume is not None:
                    consume(out, 0)
                return out, 0
            mode = "hip_graph" if args.in_flight == 1 else "hip_graph x%d in flight" % args.in_flight
        except Exception as e:  # capture not possible on this stack: stay eager (still the HIP path)
            print("graph capture failed, running eagerly:", repr(e)[:200], file=sys.stderr)
            frame = eager_frame

    n_acc = max(args.in_flight, 1)
    stat_acc = torch.zeros((n_acc, 2), device=dev)   # [samples per ray, coverage] per replica / stream: no cross-stream read-modify-write
    cnt_sum, cov_sum = stat_acc[:, 0], stat_acc[:, 1]

    def stats(out, k):
        """the two per-frame statistics, one launch on the frame's stream (`ia_frame_stats`)"""
        rgb, depth, alpha, counter = out
        _lib.check(L.ia_frame_stats(_lib.ptr(counter), _lib.ptr(alpha), counter.numel(), stat_acc[k].data_ptr(), _lib.stream()), "ia_frame_stats")

    frames_done = [0]
    last_out = [None]

    def run_frames(i0, n):
        """the loop body of the timed region (frame + the two statistics reductions, executed on the frame's stream), used
        unchanged by the spin-up windows and the warm-up, so that nothing is executed for the first time inside the timed region"""
        for i in range(i0, i0 + n):
            last_out[0] = frame(i, stats)[0]
            frames_done[0] += 1

    # Adaptive spin-up, untimed but REPORTED.  A GPU that idled through model construction, the first
    # replays of a freshly instantiated graph and the first launches of the statistics kernels are all
    # slower than the steady state; 10-frame windows are run until three consecutive windows agree within
    # 3 % (or --spinup-max-ms is used up).  `value_first_window` shows the ramp, `value_steady` the plateau;
    # `value` below is still the barrier-bracketed K-step measurement of the contract.
    windows = []
    t_spin = time.perf_counter()
    WIN = 10
    while True:
        torch.cuda.synchronize()
        tw = time.perf_counter()
        run_frames(len(windows) * WIN, WIN)
        torch.cuda.synchronize()
        windows.append(WIN / (time.perf_counter() - tw))
        if len(windows) >= 3 and max(windows[-3:]) / min(windows[-3:]) < 1.03:
            break
        if (time.perf_counter() - t_spin) * 1e3 > args.spinup_max_ms:
            break
    spinup_ms = (time.perf_counter() - t_spin) * 1e3
    run_frames(0, args.warmup)
    torch.cuda.synchronize()
    # the number of spin-up windows depends on timing: the timed frames' random draws (occupancy-probe jitter) start from a fixed
    # seed instead, so that the same arguments give the timed frames the same inputs
    torch.cuda.manual_seed(1234 + rank)
    rng_start = torch.cuda.get_rng_state()
    stat_acc.zero_()
    if world_size > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    frames_done[0] = 0
    t0 = time.perf_counter()
    run_frames(args.warmup, args.steps)
    torch.cuda.synchronize()
    if world_size > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    # the last timed frame, copied out before anything else replays its graph replica (outputs of a replayed graph are static buffers)
    last_frame = [t.clone() for t in last_out[0]] if args.dump_outputs and rank == 0 else None
    last_call = graphed.calls - 1 if graphed is not None else None
    rng_end = torch.cuda.get_rng_state()
    dt_local = dt                               # this rank's own clock around its K frames (the line reports the MAX over ranks)
    timed_frames = int(frames_done[0])          # what THIS rank rendered inside the timed region (the secondary runs below count on)
    main_samples_per_ray = float(cnt_sum.sum().item()) / args.steps
    main_alpha_coverage = float(cov_sum.sum().item()) / args.steps
    # frames whose wave-front loop needed more iterations than the graph holds (deferred check) are
    # rendered again eagerly; that time belongs to the job
    incomplete = graphed.finish() if graphed is not None else 0
    if incomplete:
        redo = [c for c in graphed.incomplete_calls]
        t_re = time.perf_counter()
        for _ in redo:
            eager_frame(args.warmup)
        torch.cuda.synchronize()
        dt += time.perf_counter() - t_re
    dumped = None
    if last_frame is not None:
        redone = graphed is not None and last_call in graphed.incomplete_calls
        if redone:
            # the graph held too few wave-front iterations for the last frame: its result is the eager render, with the random
            # draws its replay consumed (every timed frame advanced the generator's philox offset by the same amount)
            seed, off0 = rng_start.view(torch.int64).tolist()
            seed_end, off1 = rng_end.view(torch.int64).tolist()
            assert seed_end == seed and (off1 - off0) % args.steps == 0, (seed, seed_end, off0, off1)
            keep = torch.cuda.get_rng_state()
            torch.cuda.set_rng_state(torch.tensor([seed, off1 - (off1 - off0) // args.steps], dtype=torch.int64).view(torch.uint8))
            last_frame = list(eager_frame(args.warmup + args.steps - 1)[0])
            torch.cuda.synchronize()
            torch.cuda.set_rng_state(keep)
        dumped = {"dir": args.dump_outputs, "frame": int(my[(args.warmup + args.steps - 1) % n_total] % len(poses)),
                  "rerendered_eagerly": bool(redone),
                  "arrays": dump_outputs(args.dump_outputs, dict(zip(("rgb", "depth", "alpha", "counter"), last_frame)))}
    # Everything from here to the result line is the --full run: measurements of their own, after the timed region and
    # outside `value`.  A plain run skips them all.
    # with several frames in flight the per-frame LATENCY is not ms_per_step: replay ONE replica's graph back to back
    one_fps = None
    if args.full and graphed is not None and args.in_flight > 1:
        g0 = graphed.graphs[0]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for i in range(args.warmup, n_total):
            f = my[i % n_total] % len(poses)
            b = frame_inputs[0]
            b["global_orient"], b["body_pose"], b["transl"] = pose_t[f:f + 1, :3], pose_t[f:f + 1, 3:], tr_t[f:f + 1]
            b["near"], b["far"] = near_far(float(np.sqrt((tr[f] ** 2).sum())))
            g0(b)
        torch.cuda.synchronize()
        one_fps = args.steps / (time.perf_counter() - t1)
        g0.finish()
    # secondary figure: the procedural pose track rounds 1-2 quoted, through the same graphs (untimed for `value`)
    proc_track = None
    if args.full:
        dt2, err2, inc2 = 0.0, None, 0
        n_sec = min(max(args.steps, 20), 100)
        keep = (poses, tr, pose_t, tr_t)
        try:
            poses, tr = syn.procedural_pose_track(200)
            pose_t, tr_t = torch.as_tensor(poses, device=dev), torch.as_tensor(tr, device=dev)
            run_frames(0, 10)
            torch.cuda.synchronize()
            stat_acc.zero_()
            t2 = time.perf_counter()
            run_frames(10, n_sec)
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t2
            inc2 = graphed.finish() if graphed is not None else 0
        except Exception as e:
            err2 = repr(e)[:200]
        poses, tr, pose_t, tr_t = keep
        # (collectives outside the try: every rank takes part whether or not its own secondary run succeeded)
        failed = max_over_ranks(1.0 if err2 else 0.0)
        dt2 = max_over_ranks(dt2)
        if failed or dt2 <= 0:
            proc_track = {"error": err2 or "failed on another rank"}
        else:
            proc_track = {"frames_per_s": n_sec * world_size / dt2, "frames": n_sec, "samples_per_ray": float(cnt_sum.sum().item()) / n_sec,
                          "alpha_coverage": float(cov_sum.sum().item()) / n_sec, "frames_incomplete_in_graph": int(inc2) - int(incomplete),
                          "what": "synthetic.procedural_pose_track(200), the workload of the round-1/2 bench lines"}
    # per-kernel timing for the roofline block: HIP events around every launch of the two dominant
    # stages on the stream they run on.  Recording ~50 events per frame costs ~10 % of the frame,
    # so `value` comes from the un-instrumented pass above and the SAME K frames are then launched
    # once more with the events enabled (`ms_per_step_instrumented`).
    prof = args.full and not args.no_profile
    dt_prof = None
    if prof:
        _lib.check(L.ia_profile_enable(1))
        _lib.check(L.ia_profile_reset())
        torch.cuda.synchronize()
        tp0 = time.perf_counter()
        for i in range(args.warmup, n_total):
            eager_frame(i)
        torch.cuda.synchronize()
        dt_prof = time.perf_counter() - tp0
    dt = max_over_ranks(dt)

    roof = None
    kernels = {}
    if prof:
        for kid, name in ((0, "k_search"), (1, "k_field")):
            ms, n, units = C.c_double(), C.c_int64(), (C.c_uint64 * 2)()
            _lib.check(L.ia_profile_get(kid, C.byref(ms), C.byref(n), units))
            u3 = (C.c_uint64 * 3)()
            _lib.check(L.ia_profile_get_units(kid, u3, 3))
            kernels[name] = dict(ms=ms.value, launches=n.value, units=[int(u3[0]), int(u3[1]), int(u3[2])])
        _lib.check(L.ia_profile_enable(0))
        ks, kf = kernels["k_search"], kernels["k_field"]
        # algorithmic bytes: field = 512 B gathered (16 lv x 8 corners x 2 x fp16)
        # + 12 B in + 16 B out per sample; search = 384 B per trilinear fetch THAT LOADS (8 corners x 12 ch x 4 B; a
        # fetch whose 8 corners all lie outside the grid is zero by construction and moves nothing: counted in
        # units[1], excluded here) + 12 B in per point + 12 B out per surviving root (bounded by solves).
        kf["bytes"] = kf["units"][0] * (512 + 12 + 16)
        ks["bytes"] = ks["units"][2] * 384 + ks["units"][0] // 13 * 12
        dom = "k_field" if kf["ms"] >= ks["ms"] else "k_search"
        k = kernels[dom]
        nl = max(k["launches"], 1)
        per_launch_s = k["ms"] * 1e-3 / nl
        achieved = k["bytes"] / nl / per_launch_s / 1e9 if k["ms"] > 0 else 0.0
        # The 25 MB transform grid (k_search) and the 26 MB fp16 hash table (k_field) are L2 / Infinity-Cache
        # resident: the algorithmic bytes are served by the cache hierarchy, so the roof they are priced against
        # is the aggregate L2 bandwidth; the bytes that actually reached the fabric (PMC: FETCH_SIZE x2 + WRITE_SIZE,
        # profiles/, accepted only when collected on THIS build) divided by the same launch time give the HBM fraction.
        # (every kernel is keyed on ITS translation unit: a summary of another unit's kernel must not pass for this one's)
        KERNEL_TU = {"k_search": "ia_search.hip", "k_field": "ia_field.hip", "k_precompute": "ia_snarf.hip"}
        tj, tsrc = _profile_json("pmc_traffic", (KERNEL_TU[dom],))
        traffic = None
        if tj is not None:
            try:
                traffic = tj[dom]["hbm_bytes_per_launch"]
            except Exception:
                traffic = None
        roof = {"kernel": dom, "bound": "l2", "achieved": achieved, "peak": L2_PEAK_GBS, "unit": "GB/s",
                "frac": min(achieved / L2_PEAK_GBS, 1.0), "traffic": traffic, "traffic_source": tsrc,
                "hbm": ({"achieved": traffic / per_launch_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": traffic / per_launch_s / 1e9 / HBM_PEAK_GBS} if traffic else None),
                "note": ("achieved = algorithmic bytes per launch / average launch duration (HIP events on the launch stream, this run): "
                         "k_search = 384 B per trilinear fetch that loads (fetches with all 8 corners outside the grid are zero without "
                         "a load: `fetches_algorithm` counts them, `fetches_loaded` does not) + 12 B per point + 12 B per root; "
                         "k_field (encode + MLP kernels) = 540 B per sample (512 B hash-table gathers).  Both tables are served "
                         "from L1 / L2 / Infinity Cache, hence the L2 roof (34.5 TB/s aggregate); `hbm` prices the PMC fabric "
                         "traffic of the same kernel against the 8 TB/s HBM peak"),
                "avg_launch_us": per_launch_s * 1e6, "launches": k["launches"],
                "algorithmic_bytes_per_launch": k["bytes"] / nl,
                "solves": ks["units"][0], "fetches_algorithm": ks["units"][1], "fetches_loaded": ks["units"][2],
                "fetches_loaded_per_s": ks["units"][2] / (ks["ms"] * 1e-3) if ks["ms"] > 0 else 0.0,
                "ms_per_frame": {n: v["ms"] / args.steps for n, v in kernels.items()},
                "other": {n: {"avg_launch_us": v["ms"] * 1e3 / max(v["launches"], 1), "launches": v["launches"],
                              "GBps": (v["bytes"] / (v["ms"] * 1e-3) / 1e9 if v["ms"] > 0 else 0.0),
                              "units": v["units"]} for n, v in kernels.items()}}
        # resource usage of the search kernel as compiled into this library (hipFuncGetAttributes / occupancy query)
        vg, lds, thr, wgs = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        if L.ia_search_kernel_info(C.byref(vg), C.byref(lds), C.byref(thr), C.byref(wgs)) == 0:
            roof["kernel_resources"] = {"vgprs": vg.value, "lds_bytes_per_workgroup": lds.value, "threads_per_workgroup": thr.value,
                                        "workgroups_per_cu": wgs.value, "waves_per_simd": wgs.value * thr.value / 64 / 4.0}
        cj, csrc = _profile_json("pmc_search", ("ia_search.hip",))
        if cj is not None:
            # committed PMC passes of this kernel (tools/pmc_all.sh): what actually bounds k_search is the rate at which a
            # CU's vector L1 (TCP) looks up cache lines for divergent 16-byte gathers -- ~1 access per clock and CU
            keep = ("l1_hit_rate", "l2_hit_rate", "tcp_accesses_per_launch", "tcp_accesses_per_clk_per_cu_at_2.4GHz", "wave_cycle_split",
                    "avg_launch_us_in_pass", "launches")
            roof["counters"] = {v: {k: cj[v][k] for k in keep if k in cj[v]} for v in ("k_search/probe", "k_search/render") if v in cj}
        roof["counters_source"] = csrc
        pj, psrc = _profile_json("pmc_traffic", (KERNEL_TU["k_precompute"],))   # k_precompute lives in ia_snarf.hip
        if pj is not None:
            # the streaming kernel of the path priced against HBM from the same counter passes (FETCH_SIZE x 2 + WRITE_SIZE and
            # the launch time inside those passes): k_precompute reads the 50.3 MB skinning-weight volume and writes the 25.2 MB
            # transform grid once per frame (81.8 MB algorithmic)
            try:
                pc = pj["k_precompute"]
                roof["precompute_hbm"] = {"algorithmic_bytes": 81.8e6, "traffic": pc["hbm_bytes_per_launch"], "avg_launch_us_in_pass": pc["avg_launch_us_in_pass"],
                                          "achieved": pc["hbm_bytes_per_launch"] / (pc["avg_launch_us_in_pass"] * 1e-6) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                          "frac": pc["hbm_bytes_per_launch"] / (pc["avg_launch_us_in_pass"] * 1e-6) / 1e9 / HBM_PEAK_GBS, "source": psrc}
            except Exception:
                pass

    frames = args.steps * world_size
    fps = frames / dt
    frames_per_rank = [args.steps]
    if world_size > 1:   # what every rank really rendered inside the timed region (gathered, not assumed)
        got = [None] * world_size
        torch.distributed.all_gather_object(got, timed_frames)
        frames_per_rank = [int(g) for g in got]
        frames = sum(frames_per_rank)
        fps = frames / dt
    else:
        frames_per_rank = [timed_frames]
    result = {
        "metric": "novel_pose_render_frames_per_sec_512x512", "value": fps, "unit": "frames/s",
        "n_gpus": world_size, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "render_image_fast %dx%d, SNARF_NGP defaults (13 init bones, 128^2x32 skinning voxels, "
                               "16-level hash grid T=2^19, 64^3 occupancy rebuilt per frame with 5 probes, "
                               "MAX_SAMPLES 256, MAX_BATCH 291600), synthetic SMPL-like body animated by the first 200 frames of "
                               "data/animation/aist_demo.npz (animate.py:48-50 translation; tests/golden/aist_demo_200.npz)" % (res, res),
                   "pose_track": "aist_demo.npz[:200]",
                   "frames_sharded_over": world_size},
        "rays_per_sec": fps * res * res,
        "frames_per_rank": frames_per_rank,
        "samples_per_ray": main_samples_per_ray,
        "alpha_coverage": main_alpha_coverage,
        "frames_in_flight": (args.in_flight if graphed is not None else 1),
        "render_loop_iters": model.renderer.last_iters, "launch_mode": mode,
        "spinup_ms": spinup_ms, "spinup_windows": len(windows),
        "value_first_window": windows[0] * world_size, "value_steady": float(np.mean(windows[-3:])) * world_size,
        "frames_rerendered_eagerly": int(incomplete),
        "dump_outputs": dumped, "full": args.full,
    }
    if args.full:   # (a plain run's line carries none of these keys, nor roofline / hashgrid_lookup / mfma / train / cpu_baseline)
        result.update(procedural_track=proc_track,
                      one_frame_in_flight=({"frames_per_s": one_fps * world_size, "frame_latency_ms": 1e3 / one_fps} if one_fps else None),
                      ms_per_step_instrumented=(dt_prof / args.steps * 1e3) if dt_prof else None)
    result["ranks"] = rank_report(rank, world_size, dev, {"frames_timed": int(timed_frames), "frames_per_s_local_clock": timed_frames / dt_local,
                                                           "launch_mode": mode, "frames_in_flight": (args.in_flight if graphed is not None else 1)})
    if roof is not None:
        result["roofline"] = roof
    if rank == 0 and prof:
        result["hashgrid_lookup"] = hashgrid_roofline(model, dev, frame_batch=batches[0])
        mj, msrc = _profile_json("pmc_mfma", ("ia_field.hip",))
        result["mfma"] = dict(mj, source=msrc) if mj is not None else {"source": msrc}
    if args.train_steps > 0 and world_size > 1:
        tr_res, sup = supervised_train(args, rank, world_size, args.train_steps)     # (collective over the parents: every rank calls it)
        if rank == 0:
            result["train"] = dict(tr_res or {}, supervised=sup)
    elif args.train_steps > 0:
        try:
            result["train"] = train_throughput(model, dev, poses, tr, rank, world_size, args.train_steps, res=res, graphed=not args.no_graph)
            u = train_throughput(model, dev, poses, tr, rank, world_size, args.train_steps, res=res, graphed=not args.no_graph,
                                 sampler="uniform")
            result["train"]["uniform_rays"] = {k: u[k] for k in ("it_per_sec", "windows_it_per_sec", "rays_per_sec", "mse_last", "samples_candidates_last_step", "launch_mode")}
            # BASELINE config 4: SMPL refinement (its own try: the config-2 figures above survive a failure here)
            try:
                result["train"]["refine"] = train_throughput(model, dev, poses, tr, rank, world_size, args.train_steps, res=res,
                                                             graphed=not args.no_graph, sampler="edge", refine=True)
                if not args.no_graph and world_size == 1:
                    e = train_throughput(model, dev, poses, tr, rank, world_size, max(args.train_steps // 2, 10), res=res, graphed=False,
                                         sampler="edge", refine=True)
                    result["train"]["refine"]["eager"] = {k: e[k] for k in ("it_per_sec", "launch_mode")}
            except Exception as e:
                result["train"]["refine"] = {"error": repr(e)[:300]}
            # the fit stage (fit.py with deformer=smpl: the step before train.py in the Neuman pipeline, bash/run-neuman-demo.sh:6):
            # SMPLDeformer + SMPL parameter tables + a fresh field on 4 x 32^2 patches of 256^2 frames, eager steps
            if world_size == 1:
                try:
                    result["train"]["fit_stage"] = fit_stage_throughput(dev, max(args.train_steps, 20))
                except Exception as e:
                    result["train"]["fit_stage"] = {"error": repr(e)[:300]}
            hj, hsrc = _profile_json("pmc_hgbwd", ("ia_field.hip",))
            # the training step's dominant kernel against the measured atomic-request ceiling (PMC pass on this build)
            result["train"]["hashgrid_bwd_atomics"] = dict(hj.get("k_hashgrid_bwd<16>", {}), source=hsrc) if hj is not None else {"source": hsrc}
        except Exception as e:  # the headline line must survive a failure of the secondary workload
            result["train"] = {"error": repr(e)[:300]}
    if rank == 0 and world_size == 1 and args.cpu_frames > 0:
        result["cpu_baseline"] = cpu_baseline(body, fp, model, poses, tr, res, args.cpu_frames)
    if rank == 0:
        print(json.dumps(result))
    if world_size > 1:
        torch.distributed.barrier()   # rank 0 is still measuring the isolated encoder / printing: leave together
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
