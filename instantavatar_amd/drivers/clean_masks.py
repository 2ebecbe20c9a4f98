"""Clean the raw per-frame masks of a custom sequence (scripts/custom/extract-largest-connected-components.py of the reference, the
step of scripts/custom/process-sequence.sh between the segmentation network and `refine_smpl --silhouette` / training):

    python -m instantavatar_amd.drivers.clean_masks --data DIR [--source masks_sam] [--kernel 5] [--connectivity 8] \\
        [--threshold 0] [--chunk N] [--overwrite]

reads DIR/<source>/*.png (sorted; any image format PIL reads), thresholds at > threshold, opens and closes with the kernel x kernel
box, keeps the largest connected component and writes DIR/masks/<name>.png, 8-bit single-channel 0 / 255; where DIR/images/<name>
exists (the same file name as the mask) it also writes DIR/masked_images/<name>.png, the frame with everything outside the mask set to
0.  The cleaning is HIP (instantavatar_amd/masks.py), in chunks of frames; files are decoded and encoded with PIL on host threads.

A single-channel mask file is taken as it is.  A colour file goes through PIL's "L" conversion (ITU-R 601-2 luma, (299 R + 587 G +
114 B) / 1000 in integers), which can differ from cv2's grey conversion by one level: under the default threshold 0 that only
matters for pixels that are nearly black.

Frames that end up without any foreground (the reference script stops at the first one) and frames whose kept component is less than
half of the foreground after morphology -- usually a segmentation failure -- are named in the report; the run goes on.  DIR/masks is
never overwritten unless --overwrite is given, and --source masks (cleaning the output in place) is refused."""
import argparse
import concurrent.futures
import glob
import os

import numpy as np


def _error(path, what):
    from ..datasets.sequence_dir import SequenceError
    return SequenceError("%s: %s" % (path, what))


def check_args(data, source="masks_sam", kernel=5, connectivity=8, threshold=0, overwrite=False):
    """everything that can be refused without a device -> the sorted source files; SequenceError names the path or the option"""
    root = os.fspath(data)
    if kernel % 2 != 1 or not 1 <= kernel <= 31:
        raise _error("--kernel %d" % kernel, "the box is odd and in [1, 31]")
    if connectivity not in (4, 8):
        raise _error("--connectivity %d" % connectivity, "8 or 4")
    if not 0 <= threshold <= 255:
        raise _error("--threshold %d" % threshold, "outside [0, 255] (foreground is pixel > threshold)")
    if not os.path.isdir(root):
        raise _error(root, "is missing: not a sequence directory")
    out = os.path.join(root, "masks")
    src = os.path.join(root, source)
    if os.path.normpath(src) == os.path.normpath(out) or (os.path.exists(src) and os.path.exists(out) and os.path.samefile(src, out)):
        raise _error(src, "--source is the output directory: the raw masks would be overwritten by the cleaned ones")
    if not os.path.isdir(src):
        raise _error(src, "is missing: no raw masks (one image per frame, the segmentation network's output)")
    if os.path.exists(out) and not overwrite:
        raise _error(out, "exists already: give --overwrite to replace the masks in it")
    files = sorted(f for f in glob.glob(os.path.join(src, "*")) if os.path.isfile(f))
    if not files:
        raise _error(src, "holds no files")
    stems = [os.path.splitext(os.path.basename(f))[0] for f in files]
    if len(set(stems)) != len(stems):
        raise _error(src, "two files share the name %s: their masks would be written to the same file"
                     % next(s for s in stems if stems.count(s) > 1))
    return files


def _decode_mask(path, dst):
    from PIL import Image
    try:
        with Image.open(path) as im:
            a = np.asarray(im if im.mode == "L" else im.convert("L"))
    except (OSError, ValueError) as e:
        raise _error(path, "not a readable mask image (%s)" % e)
    if a.shape != dst.shape:
        raise _error(path, "is %d x %d, the first mask is %d x %d" % (a.shape[1], a.shape[0], dst.shape[1], dst.shape[0]))
    dst[...] = a


def _decode_image(path, dst):
    from PIL import Image
    try:
        with Image.open(path) as im:
            a = np.asarray(im.convert("RGB"))
    except (OSError, ValueError) as e:
        raise _error(path, "not a readable image (%s)" % e)
    if a.shape != dst.shape:
        raise _error(path, "is %d x %d, its mask is %d x %d" % (a.shape[1], a.shape[0], dst.shape[1], dst.shape[0]))
    dst[...] = a


def _encode(path, a):
    from PIL import Image
    Image.fromarray(a).save(path)


def run(data, source="masks_sam", kernel=5, connectivity=8, threshold=0, chunk=None, overwrite=False, workers=None, log=print):
    """-> dict(frames, empty: names without foreground, small: names whose kept component is under half of the foreground,
    masked_images: how many were written)"""
    files = check_args(data, source, kernel, connectivity, threshold, overwrite)
    import torch
    from PIL import Image
    from .. import _lib
    from ..masks import apply_masks, clean_masks
    if not torch.cuda.is_available():
        raise _lib.IAError("clean_masks needs a GPU; there is no CPU path")
    dev = torch.device("cuda", torch.cuda.current_device())
    root = os.fspath(data)
    try:
        with Image.open(files[0]) as im:
            W, H = im.size
    except (OSError, ValueError) as e:
        raise _error(files[0], "not a readable mask image (%s)" % e)
    N = len(files)
    chunk = max(1, min(N, int(chunk) if chunk else (32 << 20) // (H * W) or 1))      # default: about 32 MB of mask pixels
    workers = max(1, min(16, os.cpu_count() or 1, int(workers) if workers else 16))
    out_dir, img_dir, mimg_dir = (os.path.join(root, d) for d in ("masks", "images", "masked_images"))
    os.makedirs(out_dir, exist_ok=True)
    names = [os.path.splitext(os.path.basename(f))[0] for f in files]
    empty, small, n_masked = [], [], 0
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        for first in range(0, N, chunk):
            n = min(chunk, N - first)
            raw = np.empty((n, H, W), np.uint8)
            jobs = [pool.submit(_decode_mask, files[first + i], raw[i]) for i in range(n)]
            with_image = [i for i in range(n) if os.path.isfile(os.path.join(img_dir, os.path.basename(files[first + i])))]
            frames = np.empty((len(with_image), H, W, 3), np.uint8)
            jobs += [pool.submit(_decode_image, os.path.join(img_dir, os.path.basename(files[first + i])), frames[j])
                     for j, i in enumerate(with_image)]
            for j in jobs:
                j.result()
            r = clean_masks(torch.as_tensor(raw).to(dev), threshold=threshold, kernel_size=kernel, connectivity=connectivity, return_stages=True)
            fg = (r.binary != 0).sum((1, 2)).cpu().numpy()
            area = r.area.cpu().numpy()
            masks = r.masks.cpu().numpy()
            jobs = [pool.submit(_encode, os.path.join(out_dir, names[first + i] + ".png"), masks[i]) for i in range(n)]
            if with_image:
                os.makedirs(mimg_dir, exist_ok=True)
                sel = torch.as_tensor(with_image, device=dev)
                cut = apply_masks(torch.as_tensor(frames).to(dev), r.masks[sel].contiguous()).cpu().numpy()
                jobs += [pool.submit(_encode, os.path.join(mimg_dir, names[first + i] + ".png"), cut[j]) for j, i in enumerate(with_image)]
                n_masked += len(with_image)
            for j in jobs:
                j.result()
            for i in range(n):
                if area[i] == 0:
                    empty.append(names[first + i])
                elif 2 * int(area[i]) < int(fg[i]):
                    small.append(names[first + i])
    log("cleaned %d masks %dx%d from %s into %s (kernel %d, connectivity %d, threshold %d, chunks of %d)%s"
        % (N, W, H, os.path.join(root, source), out_dir, kernel, connectivity, threshold, chunk,
           "; %d masked images into %s" % (n_masked, mimg_dir) if n_masked else ""))
    if empty:
        log("no foreground in %d frame%s (an all-zero mask was written): %s" % (len(empty), "" if len(empty) == 1 else "s", ", ".join(empty)))
    if small:
        log("kept component under half of the foreground in %d frame%s (a segmentation failure?): %s"
            % (len(small), "" if len(small) == 1 else "s", ", ".join(small)))
    return dict(frames=N, empty=empty, small=small, masked_images=n_masked)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", "--data_dir", dest="data", required=True, metavar="DIR")
    ap.add_argument("--source", default="masks_sam", help="the directory under DIR that holds the raw masks")
    ap.add_argument("--kernel", type=int, default=5, help="side of the box of the open and the close (odd, 1 = no morphology)")
    ap.add_argument("--connectivity", type=int, default=8)
    ap.add_argument("--threshold", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=None, help="frames cleaned per call (default: about 32 MB of mask pixels)")
    ap.add_argument("--overwrite", action="store_true", help="replace the files of an existing DIR/masks")
    args = ap.parse_args(argv)
    from ..datasets.sequence_dir import SequenceError
    try:
        run(args.data, args.source, args.kernel, args.connectivity, args.threshold, args.chunk, args.overwrite)
    except SequenceError as e:
        raise SystemExit("--data %s: %s" % (args.data, e))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
