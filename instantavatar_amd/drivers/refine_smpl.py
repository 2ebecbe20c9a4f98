"""Refine a custom sequence's SMPL parameters against its 2D keypoints (scripts/custom/refine-smpl.py of the reference, the step of
scripts/custom/process-sequence.sh between ROMP / OpenPose and training):

    python -m instantavatar_amd.drivers.refine_smpl --data DIR --gender male [--keypoints-threshold 0.2] [--downscale 1] \\
        [--steps 200] [--smpl-dir ./data/SMPLX/smpl] [--synthetic-body | --synthetic-mesh-body] [--silhouette [--silhouette-iters 10]]

reads DIR/cameras.npz, DIR/poses.npz (`thetas` or `global_orient` / `body_pose`, `betas`, `transl`) and DIR/keypoints.npy
([F,25,3]: x, y, confidence in BODY_25 order) and writes DIR/poses_optimized.npz with the keys of poses.npz -- the file
`train --data DIR --dataset custom` loads.  The loss and its gradient are HIP kernels (instantavatar_amd/keypoints.py).
`--silhouette` runs the reference's second stage after the keypoint stage: per frame, LBFGS over pose and translation on the MSE
between a soft silhouette of the body and DIR/masks/* (instantavatar_amd/silhouette.py); it needs a body model with faces."""
import argparse
import os

import numpy as np


def _error(path, what):
    from ..datasets.sequence_dir import SequenceError
    return SequenceError("%s: %s" % (path, what))


def read_inputs(root, downscale=1):
    """-> (proj [3,4], the arrays of poses.npz, pose [F,72], betas [10], transl [F,3], keypoints [F,25,3]); SequenceError names the
    file that is missing or does not fit"""
    root = os.fspath(root)
    cam_path, pose_path, kp_path = (os.path.join(root, n) for n in ("cameras.npz", "poses.npz", "keypoints.npy"))
    for p, what in ((cam_path, "not a sequence directory"), (pose_path, "no SMPL parameters to refine (ROMP's output)"),
                    (kp_path, "no 2D keypoints (OpenPose's output, [F,25,3])")):
        if not os.path.exists(p):
            raise _error(p, "is missing: " + what)
    camera = np.load(cam_path)
    missing = [k for k in ("intrinsic", "extrinsic") if k not in camera.files]
    if missing:
        raise _error(cam_path, "no %s (has %s)" % (", ".join(missing), ", ".join(camera.files)))
    K = np.array(camera["intrinsic"], np.float64)
    if downscale > 1:                                   # refine-smpl.py:165-166
        K[:2] /= downscale
    proj = (K @ np.asarray(camera["extrinsic"], np.float64)[:3]).astype(np.float32)
    try:
        params = dict(np.load(pose_path))
    except (OSError, ValueError) as e:
        raise _error(pose_path, "cannot read the SMPL parameters (%s)" % e)
    if "thetas" in params:
        pose = np.asarray(params["thetas"])
    elif "global_orient" in params and "body_pose" in params:
        pose = np.concatenate([params["global_orient"], params["body_pose"]], 1)
    else:
        raise _error(pose_path, "neither thetas nor global_orient / body_pose (has %s)" % ", ".join(sorted(params)))
    missing = [k for k in ("betas", "transl") if k not in params]
    if missing:
        raise _error(pose_path, "no %s (has %s)" % (", ".join(missing), ", ".join(sorted(params))))
    if pose.ndim != 2 or pose.shape[1] != 72 or params["betas"].size != 10 or params["transl"].shape != (pose.shape[0], 3):
        raise _error(pose_path, "pose %s, betas %s, transl %s: expected [F,72], 10 values and [F,3]"
                     % (pose.shape, params["betas"].shape, params["transl"].shape))
    try:
        kp = np.load(kp_path)
    except (OSError, ValueError) as e:
        raise _error(kp_path, "not a readable .npy array (%s)" % e)
    if kp.ndim != 3 or kp.shape[1:] != (25, 3):
        raise _error(kp_path, "keypoints are [F,25,3] (x, y, confidence in BODY_25 order), this array has shape %s" % (kp.shape,))
    if kp.shape[0] != pose.shape[0]:
        raise _error(kp_path, "%d rows of keypoints but %d rows of poses in %s" % (kp.shape[0], pose.shape[0], pose_path))
    return proj, params, pose.astype(np.float32), params["betas"].astype(np.float32).reshape(10), params["transl"].astype(np.float32), kp.astype(np.float32)


def read_masks(root, n_frames, pose_path, downscale, device):
    """DIR/masks/* sorted -> float32 [F,H,W] on the device: the first channel as cv2.imread returns it (blue of a colour file) / 255,
    not thresholded (refine-smpl.py:211-221); at a downscale above 1 through `ia_io_ingest_chunk`, the route of
    `DeviceFrames.from_directory` (factor 2: the 2 x 2 box).  SequenceError names the file that is missing or does not fit"""
    import glob
    import torch
    from PIL import Image
    from .. import _lib
    from ..datasets.sequence_dir import resize_rule
    mdir = os.path.join(os.fspath(root), "masks")
    if not os.path.isdir(mdir):
        raise _error(mdir, "is missing: no masks for --silhouette (one image per frame; `python -m instantavatar_amd.drivers.clean_masks "
                             "--data DIR` writes them from the raw masks in DIR/masks_sam)")
    files = sorted(glob.glob(os.path.join(mdir, "*")))
    if len(files) != n_frames:
        raise _error(mdir, "%d mask%s but %d rows of poses in %s" % (len(files), "" if len(files) == 1 else "s", n_frames, pose_path))
    planes = []
    for f in files:
        try:
            with Image.open(f) as im:
                a = np.asarray(im) if im.mode == "L" else np.asarray(im.convert("RGB"))[..., 2]
        except (OSError, ValueError) as e:
            raise _error(f, "not a readable mask image (%s)" % e)
        if planes and a.shape != planes[0].shape:
            raise _error(f, "is %d x %d, %s is %d x %d" % (a.shape + (files[0],) + planes[0].shape))
        planes.append(np.ascontiguousarray(a, np.uint8))
    H0, W0 = planes[0].shape
    factor = resize_rule(H0, W0, downscale)
    src = torch.as_tensor(np.stack(planes)).to(device)
    masks = torch.empty((n_frames, H0 // factor, W0 // factor), dtype=torch.float32, device=device)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        _lib.call("ia_io_ingest_chunk", None, src, 2, n_frames, H0, W0, factor, None, masks, 0, n_frames)      # 2: IA_IO_MASK_GREY
    side.synchronize()
    return masks


def silhouette_stage(root, body, K, extrinsic, pose_path, betas, pose, transl, downscale, iters, log=print):
    """the `--silhouette` stage on device tensors betas [10], pose [F,72], transl [F,3] -> (pose, transl)"""
    import torch
    from ..raster import Camera
    from ..silhouette import SilhouetteRefiner
    if body.faces_tensor.numel() == 0:
        raise _error("the body model", "has no faces: --silhouette needs triangles (an SMPL file with `f`, or --synthetic-mesh-body)")
    dev = pose.device
    masks = read_masks(root, pose.shape[0], pose_path, downscale, dev)
    w2c = torch.as_tensor(np.asarray(extrinsic, np.float32).reshape(4, 4), device=dev)
    cam = Camera(K, w2c, masks.shape[1], masks.shape[2])
    r = SilhouetteRefiner(body, body.faces_tensor, cam, masks)
    p, t, _ = r.refine(betas, pose, transl, iters=iters, log=log)
    return p, t


def write_outputs(root, params, betas, pose, transl):
    """DIR/poses_optimized.npz with the keys of poses.npz (refine-smpl.py:255-267)"""
    out = dict(params)
    for k in out:
        if k == "betas":
            out[k] = betas.astype(np.float32)
        elif k == "thetas":
            out[k] = np.array(out[k])
            out[k][:, :3], out[k][:, 3:] = pose[:, :3], pose[:, 3:]
        elif k == "global_orient":
            out[k] = pose[:, :3].copy()
        elif k == "body_pose":
            out[k] = pose[:, 3:].copy()
            out[k][:, -12:] = 0                          # :263-264: only where the file has a body_pose key
        elif k == "transl":
            out[k] = transl.copy()
    path = os.path.join(os.fspath(root), "poses_optimized.npz")
    np.savez(path, **out)
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", "--data_dir", dest="data", required=True, metavar="DIR")
    ap.add_argument("--gender", default="male")
    ap.add_argument("--keypoints-threshold", type=float, default=0.2)
    ap.add_argument("--downscale", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--smpl-dir", default="./data/SMPLX/smpl")
    ap.add_argument("--synthetic-body", action="store_true", help="the synthetic SMPL-like body (no SMPL pickle needed)")
    ap.add_argument("--synthetic-mesh-body", action="store_true", help="the synthetic body with triangles (synthetic.make_mesh_body)")
    ap.add_argument("--silhouette", action="store_true", help="refine each frame against its mask after the keypoint stage")
    ap.add_argument("--silhouette-iters", type=int, default=10, help="LBFGS steps per frame")
    args = ap.parse_args(argv)
    from ..datasets.sequence_dir import SequenceError
    try:
        proj, params, pose, betas, transl, kp = read_inputs(args.data, args.downscale)
    except SequenceError as e:
        raise SystemExit("--data %s: %s" % (args.data, e))
    import torch
    from .. import synthetic
    from ..deformers.smplx import SMPL
    from ..keypoints import KeypointRefiner
    dev = torch.device("cuda", torch.cuda.current_device())
    if args.synthetic_mesh_body:
        body = SMPL.from_dict(synthetic.make_mesh_body()).to(dev)
    else:
        body = (SMPL.from_dict(synthetic.make_body()) if args.synthetic_body else SMPL(args.smpl_dir, gender=args.gender)).to(dev)
    if args.silhouette:      # what the stage needs is checked before the keypoint stage runs
        try:
            if body.faces_tensor.numel() == 0:
                raise _error("the body model", "has no faces: --silhouette needs triangles (an SMPL file with `f`, or --synthetic-mesh-body)")
            mdir = os.path.join(args.data, "masks")
            if not os.path.isdir(mdir):
                raise _error(mdir, "is missing: no masks for --silhouette (one image per frame; `python -m instantavatar_amd.drivers.clean_masks "
                             "--data DIR` writes them from the raw masks in DIR/masks_sam)")
        except SequenceError as e:
            raise SystemExit("--data %s: %s" % (args.data, e))
    kw = {}
    if args.synthetic_mesh_body:      # fewer vertices than SMPL: stand-ins for nose, eyes, ears, toes and heels
        from ..keypoints import SMPL_KP_VERTEX
        kw["kp_vertex"] = tuple(v % int(body.v_template.shape[0]) for v in SMPL_KP_VERTEX)
    r = KeypointRefiner(body, proj, kp, threshold=args.keypoints_threshold, **kw)
    t = lambda a: torch.as_tensor(a, device=dev)
    b, p, tr, _ = r.refine(t(betas), t(pose), t(transl), steps=args.steps, lr=args.lr, log=print)
    if args.silhouette:
        camera = np.load(os.path.join(args.data, "cameras.npz"))
        K = np.array(camera["intrinsic"], np.float64)
        if args.downscale > 1:
            K[:2] /= args.downscale
        try:
            p, tr = silhouette_stage(args.data, body, K, camera["extrinsic"], os.path.join(args.data, "poses.npz"), b, p, tr, args.downscale,
                                     args.silhouette_iters)
        except SequenceError as e:
            raise SystemExit("--data %s: %s" % (args.data, e))
    path = write_outputs(args.data, params, b.cpu().numpy(), p.cpu().numpy(), tr.cpu().numpy())
    print("wrote %s (%d frames; keys %s)" % (path, pose.shape[0], ", ".join(sorted(params))))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
