"""One split of one sequence directory in the reference's layout, described on the host: what
`PeopleSnapshotDataset.__init__` (instant_avatar/datasets/peoplesnapshot.py:39-93) and `CustomDataset.__init__`
(custom.py:39-87) set up -- the camera, the sliced file lists, the SMPL parameters -- before any pixel is read.

    <root>/cameras.npz              intrinsic [3,3], extrinsic [4,4], height, width
    <root>/images/*.png
    <root>/masks/*.npy              peoplesnapshot: uint8 0/1 arrays (what the reference's preprocessing writes)
    <root>/masks/*.png              custom: grey, read as float64 v / 255
    <root>/poses/...npz, poses.npz / poses_optimized.npz        (precedence: `pose_file`)

    seq = read_sequence(root, "peoplesnapshot", "train", dict(start=0, end=445, skip=4, downscale=2))
    frames = DeviceFrames.from_directory(seq, sampler, device)

The split options are the reference's `confs/dataset/**/*.yaml` blocks (`split_options` reads one with the project's own
resolver); a plain dict does as well.  Nothing is guessed: every inconsistency of a directory is an error that names the file.

The pixels are decoded and resized by `DeviceFrames.from_directory` (PIL on host threads, `ia_io_ingest_chunk` on the
device).  The resize is restated for the factors the reference's shipped configurations use, `resize_rule`: downscale 1 (a
copy) and downscale 2 on an even source size, where `cv2.resize(src, None, fx=0.5, fy=0.5)` with the default INTER_LINEAR is,
by OpenCV's own dispatch (INTER_LINEAR becomes INTER_AREA when both integer scales are exactly 2), the 2 x 2 box:
`(a + b + c + d + 2) >> 2` for uint8 sources, `((a/255 + b/255) + (c/255 + d/255)) * 0.25` in float64 for the custom layout's
float64 mask.  PARITY UNPINNED against OpenCV itself (no cv2 to compare with): the rule is restated from OpenCV's
published dispatch and has not been checked by running cv2.resize.  The tests pin the kernel to an independent integer /
float64 numpy restatement and, for uint8, to PIL's `Image.reduce(2)`, an independent implementation of the same rounded
box (checked on the CPU: the two agree on every cell sum 0 .. 1020 and on random grey and 3-channel frames,
tests/test_cpu_sequence_dir.py::test_pil_reduce_is_the_same_rounded_box).  Other factors and odd
source sizes would go through OpenCV's fixed-point bilinear path and its edge handling; they are refused, not approximated.
"""
import collections
import glob
import os

import numpy as np

KINDS = ("peoplesnapshot", "custom")
OPTION_KEYS = ("start", "end", "skip", "downscale", "near", "far", "refine", "fitting")

Sequence = collections.namedtuple(
    "Sequence", "root kind split image_files mask_files K c2w H0 W0 H W smpl_params pose_file near far downscale")


class SequenceError(ValueError):
    """a sequence directory that is not what the loaders expect; the message names the file"""


def resize_rule(H0, W0, downscale):
    """The integer factor (1 or 2) `DeviceFrames.from_directory` ingests a H0 x W0 source with, or a SequenceError that
    says why the combination is refused (see the module docstring)."""
    d = float(downscale)
    if d != int(d):
        raise SequenceError("downscale %r is not an integer: cv2.resize would interpolate bilinearly in fixed point, which is not "
                            "restated here (supported: 1 and 2)" % (downscale,))
    d = int(d)
    if d <= 1:
        if d < 1:
            raise SequenceError("downscale %r: the reference resizes only for downscale > 1 and 0 / negative factors mean nothing" % (downscale,))
        return 1
    if d != 2:
        raise SequenceError("downscale %d: only factor 2 is OpenCV's exact 2 x 2 box (INTER_LINEAR is replaced by INTER_AREA when both "
                            "scales are exactly 2); other factors take its fixed-point bilinear path, which is not restated here "
                            "(supported: 1 and 2)" % d)
    if H0 % 2 or W0 % 2:
        raise SequenceError("downscale 2 of a %d x %d source: an odd size takes OpenCV's edge handling, which is not restated here "
                            "(height and width must be even)" % (H0, W0))
    return 2


def pose_file(root, kind, split, opt):
    """(path, cached): the npz the split's SMPL parameters come from.  cached files (one row per frame of the split) are
    used as they are; the fallback (`poses.npz` / `poses_optimized.npz`, one row per frame of the SEQUENCE) is sliced."""
    j = lambda *p: os.path.join(root, *p)
    if kind == "peoplesnapshot":
        if opt.get("refine", False):                                   # peoplesnapshot.py:62-64
            cands = [j("poses", "anim_nerf_test.npz")]
        else:                                                          # :66-71
            cands = [j("poses", "anim_nerf_%s.npz" % split), j("poses", "%s.npz" % split)]
        fallback = j("poses.npz")
    else:
        cands = [] if opt.get("fitting", False) else [j("poses", "%s.npz" % split)]     # custom.py:62-69
        fallback = j("poses_optimized.npz")
    for c in cands:
        if os.path.exists(c):                                          # :73 / custom.py:71
            return c, True
    return fallback, False


def load_smpl_param(path):
    """peoplesnapshot.py:27-37"""
    try:
        z = dict(np.load(path))
    except OSError as e:
        raise SequenceError("%s: cannot read the SMPL parameters (%s)" % (path, e))
    if "thetas" in z:
        z["body_pose"] = z["thetas"][..., 3:]
        z["global_orient"] = z["thetas"][..., :3]
    missing = [k for k in ("betas", "body_pose", "global_orient", "transl") if k not in z]
    if missing:
        raise SequenceError("%s: no %s (has %s)" % (path, ", ".join(missing), ", ".join(sorted(z))))
    if z["betas"].size != 10:
        raise SequenceError("%s: betas has %d values, not 10" % (path, z["betas"].size))
    return {"betas": z["betas"].astype(np.float32).reshape(1, 10), "body_pose": z["body_pose"].astype(np.float32),
            "global_orient": z["global_orient"].astype(np.float32), "transl": z["transl"].astype(np.float32)}


def _file_size(path):
    """(height, width) of an image or mask file from its header"""
    if path.endswith(".npy"):
        try:
            a = np.load(path, mmap_mode="r")
        except (OSError, ValueError) as e:
            raise SequenceError("%s: not a readable .npy array (%s)" % (path, e))
        if a.ndim != 2:
            raise SequenceError("%s: a mask is a 2-D array, this one has shape %s" % (path, a.shape))
        return int(a.shape[0]), int(a.shape[1])
    from PIL import Image
    try:
        with Image.open(path) as im:
            return int(im.size[1]), int(im.size[0])
    except OSError as e:
        raise SequenceError("%s: not a readable image (%s)" % (path, e))


def read_sequence(root, kind, split, opt):
    """The split `split` ("train" | "val" | "test") of the sequence at `root`; opt: dict with start, end and optionally
    skip (1), downscale (1), near, far, refine (peoplesnapshot), fitting (custom) -- other keys of a reference config block
    (num_workers, batch_size, sampler) are ignored."""
    if kind not in KINDS:
        raise SequenceError("unknown dataset kind %r (one of %s)" % (kind, ", ".join(KINDS)))
    root = os.fspath(root)
    for k in ("start", "end"):
        if opt.get(k) is None:
            raise SequenceError("the split options need `%s` (got %s)" % (k, sorted(opt)))
    cam_path = os.path.join(root, "cameras.npz")
    if not os.path.exists(cam_path):
        raise SequenceError("%s is missing: not a sequence directory" % cam_path)
    camera = np.load(cam_path)
    missing = [k for k in ("intrinsic", "extrinsic", "height", "width") if k not in camera.files]
    if missing:
        raise SequenceError("%s: no %s (has %s)" % (cam_path, ", ".join(missing), ", ".join(camera.files)))
    K = np.array(camera["intrinsic"])                                  # peoplesnapshot.py:41-51
    c2w = np.linalg.inv(camera["extrinsic"])
    H0, W0 = int(camera["height"]), int(camera["width"])
    downscale = opt.get("downscale", 1)
    H, W = H0, W0
    if downscale > 1:
        H, W = int(camera["height"] / downscale), int(camera["width"] / downscale)
        K[:2] /= downscale
    start, end, skip = int(opt["start"]), int(opt["end"]) + 1, int(opt.get("skip", 1) or 1)     # :56-60
    img_pat = os.path.join(root, "images", "*.png")
    msk_pat = os.path.join(root, "masks", "*.npy" if kind == "peoplesnapshot" else "*.png")
    all_imgs, all_msks = sorted(glob.glob(img_pat)), sorted(glob.glob(msk_pat))
    if not all_imgs:
        raise SequenceError("no images: %s matches nothing" % img_pat)
    if len(all_imgs) != len(all_msks):
        raise SequenceError("%d images (%s) but %d masks (%s)" % (len(all_imgs), img_pat, len(all_msks), msk_pat))
    image_files, mask_files = all_imgs[start:end:skip], all_msks[start:end:skip]
    if not image_files:
        raise SequenceError("no images: [%d:%d:%d] of the %d files of %s is empty" % (start, end, skip, len(all_imgs), img_pat))
    for f in image_files + mask_files:
        hw = _file_size(f)
        if hw != (H0, W0):
            raise SequenceError("%s is %d x %d (height x width), but %s says %d x %d" % (f, hw[0], hw[1], cam_path, H0, W0))
    path, cached = pose_file(root, kind, split, opt)
    if not os.path.exists(path):
        raise SequenceError("%s is missing: no SMPL parameters for the split %r" % (path, split))
    smpl = load_smpl_param(path)
    if not cached:                                                     # :77-81
        smpl = {k: (v if k == "betas" else v[start:end:skip]) for k, v in smpl.items()}
    for k in ("body_pose", "global_orient", "transl"):
        if len(smpl[k]) != len(image_files):
            raise SequenceError("%d frames (%s[%d:%d:%d]) but %d rows of %s in %s%s" % (
                len(image_files), img_pat, start, end, skip, len(smpl[k]), k, path,
                " (a cached pose file is used as it is, one row per frame of the split)" if cached else ""))
    return Sequence(root, kind, split, image_files, mask_files, K, c2w, H0, W0, H, W, smpl, path,
                    opt.get("near", None), opt.get("far", None), downscale)


def split_options(conf_file, split, refine=False, fitting=False):
    """The `opt.<split>` block of a reference dataset config (confs/dataset/**/*.yaml), read with drivers/config.py's
    resolver; the interpolations such a block holds (`${sampler}`, `${model.opt.optimize_SMPL.*}`) resolve to `refine` /
    `fitting` as given and to nothing for the sampler (the drivers build theirs from confs/sampler)."""
    import yaml
    from ..drivers import config as cfg
    with open(conf_file) as f:
        raw = yaml.safe_load(f)
    ctx = {"sampler": None, "dataset": {"subject": raw.get("subject"), "gender": raw.get("gender")},
           "model": {"opt": {"optimize_SMPL": {"enable": bool(fitting), "is_refine": bool(refine)}}}}
    block = cfg.resolve(raw, ctx).get("opt", {}).get(split)
    if block is None:
        raise SequenceError("%s: no opt.%s block" % (conf_file, split))
    return {k: block[k] for k in OPTION_KEYS if k in block}
