"""Look at a custom sequence before training on it (what scripts/visualize-SMPL.py of the reference shows in a viewer): per frame, how
well the SMPL parameters fit the masks and the 2D keypoints, and pictures of the frames that fit worst.

    python -m instantavatar_amd.drivers.inspect_sequence --data DIR [--poses FILE] [--compare FILE] [--worst 12] [--every 0] \\
        [--downscale 1] [--gender male] [--smpl-dir ./data/SMPLX/smpl] [--synthetic-mesh-body] [--keypoints-threshold 0.2] [--out DIR/inspect]

reads DIR/cameras.npz, the poses (default: DIR/poses_optimized.npz if it is there, else DIR/poses.npz), DIR/masks/* and DIR/keypoints.npy,
and writes into --out

    report.csv            one row per frame: name; with masks inter, union, mask_area, sil_area (pixel counts) and iou of the rasterised
                          body against the mask; with keypoints n_confident and kp_err_px, the mean pixel distance between the projected
                          model points and the detections above the threshold (MidHip excluded, as in refine_smpl).  With --compare FILE
                          the same columns again for the second pose file, suffixed _compare
    overlay_<name>.png    for the --worst frames (lowest IoU; highest keypoint error when there are no masks) and every --every-th frame:
                          the frame of DIR/images with the shaded body blended in, the mask outline, the detected skeleton in limb colours
                          and the projected model points as discs.  Without DIR/images the layers are drawn on a grey canvas

and prints the median and minimum IoU, the median and maximum keypoint error, the worst frames by name and, with --compare, in how many
frames each measure improved.  A sequence without masks has no IoU columns, one without keypoints.npy no keypoint columns; one without
either is refused.  The measures and the drawing are HIP (instantavatar_amd/overlay.py); files are decoded and encoded with PIL on at
most 16 host threads.

At --downscale d the masks and images are reduced as `refine_smpl` and the loaders reduce them, the intrinsics are divided by d, and the
keypoints -- detected on the full-size frames -- are divided by d as well, so that every layer is in the pixels of the picture
(kp_err_px is then in reduced pixels).  An IoU of 0 is also what a frame with an empty mask AND an empty silhouette gets."""
import argparse
import concurrent.futures
import csv
import glob
import os

import numpy as np

COLUMNS_MASKS = ("inter", "union", "mask_area", "sil_area", "iou")
COLUMNS_KEYPOINTS = ("n_confident", "kp_err_px")
CANVAS_GREY = 64
WORKERS = 16      # decode / encode threads at most; never sized from the machine


def _error(path, what):
    from ..datasets.sequence_dir import SequenceError
    return SequenceError("%s: %s" % (path, what))


def read_poses(path):
    """-> betas [10], pose [F,72], transl [F,3] (float32) of a poses.npz / poses_optimized.npz; SequenceError names the file"""
    from ..datasets.sequence_dir import SequenceError, load_smpl_param
    if not os.path.exists(path):
        raise _error(path, "is missing: no SMPL parameters to look at")
    try:
        p = load_smpl_param(path)
    except SequenceError:
        raise
    except ValueError as e:
        raise _error(path, "cannot read the SMPL parameters (%s)" % e)
    pose = np.concatenate([p["global_orient"].reshape(-1, 3), p["body_pose"].reshape(-1, 69)], 1)
    if p["transl"].shape != (pose.shape[0], 3):
        raise _error(path, "pose %s and transl %s: expected [F,72] and [F,3]" % (pose.shape, p["transl"].shape))
    return p["betas"].reshape(10), pose, p["transl"]


def check_inputs(data, poses=None, compare=None, downscale=1.0):
    """everything that can be refused without a device -> dict(K, extrinsic, camera, pose_path, params, compare_path, compare_params,
    keypoints or None, mask_files or None, image_files or None, names); SequenceError names the files"""
    root = os.fspath(data)
    cam_path = os.path.join(root, "cameras.npz")
    if not os.path.exists(cam_path):
        raise _error(cam_path, "is missing: not a sequence directory")
    camera = np.load(cam_path)
    missing = [k for k in ("intrinsic", "extrinsic") if k not in camera.files]
    if missing:
        raise _error(cam_path, "no %s (has %s)" % (", ".join(missing), ", ".join(camera.files)))
    K = np.array(camera["intrinsic"], np.float64)
    if downscale > 1:
        K[:2] /= downscale
    pose_path = os.fspath(poses) if poses else os.path.join(root, "poses_optimized.npz")
    if not poses and not os.path.exists(pose_path):
        pose_path = os.path.join(root, "poses.npz")
    params = read_poses(pose_path)
    F = params[1].shape[0]
    compare_params = None
    if compare:
        compare_params = read_poses(os.fspath(compare))
        if compare_params[1].shape[0] != F:
            raise _error(os.fspath(compare), "%d rows of poses but %d rows of poses in %s" % (compare_params[1].shape[0], F, pose_path))
    kp_path, mdir, idir = os.path.join(root, "keypoints.npy"), os.path.join(root, "masks"), os.path.join(root, "images")
    kp = None
    if os.path.exists(kp_path):
        try:
            kp = np.load(kp_path)
        except (OSError, ValueError) as e:
            raise _error(kp_path, "not a readable .npy array (%s)" % e)
        if kp.ndim != 3 or kp.shape[1:] != (25, 3):
            raise _error(kp_path, "keypoints are [F,25,3] (x, y, confidence in BODY_25 order), this array has shape %s" % (kp.shape,))
        if kp.shape[0] != F:
            raise _error(kp_path, "%d rows of keypoints but %d rows of poses in %s" % (kp.shape[0], F, pose_path))
        kp = kp.astype(np.float32)
        if downscale > 1:
            kp[..., :2] /= np.float32(downscale)
    mask_files = None
    if os.path.isdir(mdir):
        mask_files = sorted(glob.glob(os.path.join(mdir, "*")))
        if len(mask_files) != F:
            raise _error(mdir, "%d mask%s but %d rows of poses in %s" % (len(mask_files), "" if len(mask_files) == 1 else "s", F, pose_path))
    if kp is None and mask_files is None:
        raise _error(root, "neither %s nor %s: nothing to measure the poses against" % (kp_path, mdir))
    image_files = None
    if os.path.isdir(idir):
        image_files = sorted(f for f in glob.glob(os.path.join(idir, "*")) if os.path.isfile(f))
        if len(image_files) != F:
            raise _error(idir, "%d image%s but %d rows of poses in %s" % (len(image_files), "" if len(image_files) == 1 else "s", F, pose_path))
    named = mask_files or image_files
    names = [os.path.splitext(os.path.basename(f))[0] for f in named] if named else ["%06d" % i for i in range(F)]
    if len(set(names)) != len(names):
        names = ["%06d_%s" % (i, s) for i, s in enumerate(names)]
    return dict(K=K, extrinsic=np.asarray(camera["extrinsic"], np.float64), camera=camera, pose_path=pose_path, params=params,
                compare_path=os.fspath(compare) if compare else None, compare_params=compare_params, keypoints=kp, mask_files=mask_files,
                image_files=image_files, names=names)


def _decode_image(path, factor, dst):
    from PIL import Image
    try:
        with Image.open(path) as im:
            im = im.convert("RGB")
            a = np.asarray(im.reduce(factor) if factor > 1 else im)
    except (OSError, ValueError) as e:
        raise _error(path, "not a readable image (%s)" % e)
    if a.shape != dst.shape:
        raise _error(path, "is %d x %d%s, the frames are %d x %d" % (a.shape[1], a.shape[0], " after the reduction by %d" % factor if factor > 1 else "",
                                                                      dst.shape[1], dst.shape[0]))
    dst[...] = a


def _encode(path, a):
    from PIL import Image
    Image.fromarray(a).save(path)


def _frame_size(inp, downscale):
    """(H, W, factor) of the frames: from the first mask, else the first image, else the height / width of cameras.npz"""
    from PIL import Image
    from ..datasets.sequence_dir import resize_rule
    first = (inp["mask_files"] or inp["image_files"] or [None])[0]
    if first is not None:
        try:
            with Image.open(first) as im:
                W0, H0 = im.size
        except (OSError, ValueError) as e:
            raise _error(first, "not a readable image (%s)" % e)
    elif "height" in inp["camera"].files and "width" in inp["camera"].files:
        H0, W0 = int(inp["camera"]["height"]), int(inp["camera"]["width"])
    else:
        raise _error("cameras.npz", "no height / width, and neither masks nor images to take the frame size from")
    factor = resize_rule(H0, W0, downscale)
    return H0 // factor, W0 // factor, factor


def run(data, poses=None, compare=None, worst=12, every=0, downscale=1.0, gender="male", smpl_dir="./data/SMPLX/smpl", synthetic_mesh_body=False,
        keypoints_threshold=0.2, out=None, log=print):
    """-> dict(frames, out, columns, report: {column: numpy [F]}, worst: names, overlays: the files written, improved: {measure: count} or None)"""
    inp = check_inputs(data, poses, compare, downscale)
    import torch
    from .. import _lib, synthetic
    from ..deformers.smplx import SMPL
    from ..keypoints import SMPL_KP_VERTEX
    from ..overlay import SequenceInspector, worst_frames
    from .refine_smpl import read_masks
    if not torch.cuda.is_available():
        raise _lib.IAError("inspect_sequence needs a GPU; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    root = os.fspath(data)
    H, W, factor = _frame_size(inp, downscale)
    body = (SMPL.from_dict(synthetic.make_mesh_body()) if synthetic_mesh_body else SMPL(smpl_dir, gender=gender)).to(dev)
    kw = {}
    if synthetic_mesh_body:      # fewer vertices than SMPL: stand-ins for nose, eyes, ears, toes and heels (as refine_smpl)
        kw["kp_vertex"] = tuple(v % int(body.v_template.shape[0]) for v in SMPL_KP_VERTEX)
    masks = None
    if inp["mask_files"] is not None:
        masks = read_masks(root, len(inp["names"]), inp["pose_path"], downscale, dev) > 0
        if tuple(masks.shape[1:]) != (H, W):
            raise _error(os.path.join(root, "masks"), "the masks are %d x %d, the frames %d x %d" % (masks.shape[2], masks.shape[1], W, H))
    insp = SequenceInspector(body, inp["K"], inp["extrinsic"], H, W, keypoints=inp["keypoints"], masks=masks, threshold=keypoints_threshold, **kw)
    t = lambda a: torch.as_tensor(a, device=dev)
    params = tuple(t(a) for a in inp["params"])
    rep = insp.report(*params)
    columns = [c for c in COLUMNS_MASKS + COLUMNS_KEYPOINTS if c in rep]
    table = {c: rep[c].cpu().numpy() for c in columns}
    order = worst_frames(rep, worst)
    if inp["compare_params"] is not None:
        rep2 = insp.report(*(t(a) for a in inp["compare_params"]))
        table.update({c + "_compare": rep2[c].cpu().numpy() for c in columns})
    out_dir = os.fspath(out) if out else os.path.join(root, "inspect")
    os.makedirs(out_dir, exist_ok=True)
    names, F = inp["names"], len(inp["names"])
    head = list(table)
    with open(os.path.join(out_dir, "report.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name"] + head)
        for i in range(F):
            w.writerow([names[i]] + [("%d" % table[c][i]) if table[c].dtype.kind == "i" else ("%.6f" % table[c][i]) for c in head])
    # the pictures: the worst frames first, then every --every-th, each once
    picked = list(order) + [i for i in (range(0, F, int(every)) if every and every > 0 else ()) if i not in order]
    written = []
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(WORKERS, len(picked) or 1))) as pool:
        for first in range(0, len(picked), 8):
            idx = picked[first:first + 8]
            frames = np.full((len(idx), H, W, 3), CANVAS_GREY, np.uint8)
            if inp["image_files"] is not None:
                for j in [pool.submit(_decode_image, inp["image_files"][i], factor, frames[k]) for k, i in enumerate(idx)]:
                    j.result()
            pics = insp.overlay(torch.as_tensor(frames).to(dev), idx, *params).cpu().numpy()
            paths = [os.path.join(out_dir, "overlay_%s.png" % names[i]) for i in idx]
            for j in [pool.submit(_encode, p, pics[k]) for k, p in enumerate(paths)]:
                j.result()
            written += paths
    log("inspected %d frames %dx%d of %s with %s; report.csv (%s) and %d overlay%s in %s"
        % (F, W, H, root, inp["pose_path"], ", ".join(columns), len(written), "" if len(written) == 1 else "s", out_dir))
    if "iou" in table:
        log("IoU of the body's silhouette against the masks: median %.4f, minimum %.4f (%s)"
            % (float(np.median(table["iou"])), float(table["iou"].min()), names[int(np.argmin(table["iou"]))]))
    if "kp_err_px" in table:
        log("keypoint error: median %.2f px, maximum %.2f px (%s)"
            % (float(np.median(table["kp_err_px"])), float(table["kp_err_px"].max()), names[int(np.argmax(table["kp_err_px"]))]))
    if order:
        log("worst frames by %s: %s" % ("IoU" if "iou" in table else "keypoint error", ", ".join(names[i] for i in order)))
    improved = None
    if inp["compare_params"] is not None:
        improved = {}
        if "iou" in table:
            improved["iou"] = int((table["iou_compare"] > table["iou"]).sum())
        if "kp_err_px" in table:
            improved["kp_err_px"] = int((table["kp_err_px_compare"] < table["kp_err_px"]).sum())
        log("%s against %s: %s" % (inp["compare_path"], inp["pose_path"], "; ".join(
            "%s better in %d of %d frames" % ("IoU" if k == "iou" else "keypoint error", v, F) for k, v in improved.items())))
    return dict(frames=F, out=out_dir, columns=head, report=table, worst=[names[i] for i in order], overlays=written, improved=improved)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", "--data_dir", dest="data", required=True, metavar="DIR")
    ap.add_argument("--poses", default=None, metavar="FILE", help="the pose file to look at (default: poses_optimized.npz, else poses.npz, of DIR)")
    ap.add_argument("--compare", default=None, metavar="FILE", help="a second pose file, measured the same way")
    ap.add_argument("--worst", type=int, default=12, help="overlays of this many worst frames")
    ap.add_argument("--every", type=int, default=0, help="and of every N-th frame (0: none)")
    ap.add_argument("--downscale", type=float, default=1.0)
    ap.add_argument("--gender", default="male")
    ap.add_argument("--smpl-dir", default="./data/SMPLX/smpl")
    ap.add_argument("--synthetic-mesh-body", action="store_true", help="the synthetic body with triangles (synthetic.make_mesh_body)")
    ap.add_argument("--keypoints-threshold", type=float, default=0.2)
    ap.add_argument("--out", default=None, metavar="DIR", help="default: DIR/inspect")
    args = ap.parse_args(argv)
    from ..datasets.sequence_dir import SequenceError
    try:
        run(args.data, args.poses, args.compare, args.worst, args.every, args.downscale, args.gender, args.smpl_dir, args.synthetic_mesh_body,
            args.keypoints_threshold, args.out)
    except SequenceError as e:
        raise SystemExit("--data %s: %s" % (args.data, e))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
