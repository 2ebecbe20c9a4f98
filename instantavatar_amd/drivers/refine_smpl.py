"""Refine a custom sequence's SMPL parameters against its 2D keypoints (scripts/custom/refine-smpl.py of the reference, the step of
scripts/custom/process-sequence.sh between ROMP / OpenPose and training):

    python -m instantavatar_amd.drivers.refine_smpl --data DIR --gender male [--keypoints-threshold 0.2] [--downscale 1] \\
        [--steps 200] [--smpl-dir ./data/SMPLX/smpl] [--synthetic-body]

reads DIR/cameras.npz, DIR/poses.npz (`thetas` or `global_orient` / `body_pose`, `betas`, `transl`) and DIR/keypoints.npy
([F,25,3]: x, y, confidence in BODY_25 order) and writes DIR/poses_optimized.npz with the keys of poses.npz -- the file
`train --data DIR --dataset custom` loads.  The loss and its gradient are HIP kernels (instantavatar_amd/keypoints.py).  The
reference's `--silhouette` stage is not implemented (its own pipeline has it commented out)."""
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
    body = (SMPL.from_dict(synthetic.make_body()) if args.synthetic_body else SMPL(args.smpl_dir, gender=args.gender)).to(dev)
    r = KeypointRefiner(body, proj, kp, threshold=args.keypoints_threshold)
    t = lambda a: torch.as_tensor(a, device=dev)
    b, p, tr, _ = r.refine(t(betas), t(pose), t(transl), steps=args.steps, lr=args.lr, log=print)
    path = write_outputs(args.data, params, b.cpu().numpy(), p.cpu().numpy(), tr.cpu().numpy())
    print("wrote %s (%d frames; keys %s)" % (path, pose.shape[0], ", ".join(sorted(params))))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
