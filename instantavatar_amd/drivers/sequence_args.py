"""`--data DIR` of the train, fit and eval drivers: the flags that name a sequence directory in the reference's layout and
the options of its splits (datasets/sequence_dir.py), and the load of one split onto the device."""
import os


def add_data_arguments(ap):
    """`--data` and the split options of a sequence directory (shared by the train, fit and eval drivers)"""
    ap.add_argument("--data", metavar="DIR", help="a sequence directory in the reference's layout: cameras.npz, images/*.png, masks/*.npy "
                                                  "(peoplesnapshot) or masks/*.png (custom), poses/ or poses.npz / poses_optimized.npz")
    ap.add_argument("--dataset", choices=("peoplesnapshot", "custom"), default="peoplesnapshot", help="--data: the directory's layout")
    ap.add_argument("--dataset-conf", metavar="FILE.yaml", help="--data: take the split options from the opt.<split> block of a reference "
                                                                "dataset config instead of the flags below")
    ap.add_argument("--start", type=int, default=0, help="--data: first file of the split (index into the sorted file list)")
    ap.add_argument("--end", type=int, help="--data: last file of the split, inclusive (default: the last file)")
    ap.add_argument("--skip", type=int, default=1)
    ap.add_argument("--downscale", type=float, default=1, help="--data: 1 or 2 (see datasets/sequence_dir.py)")
    ap.add_argument("--near", type=float)
    ap.add_argument("--far", type=float)


def split_options(args, split, frame=None, **flags):
    """the options dict of sequence_dir.read_sequence for `split`, from --dataset-conf or from the flags (frame: a one-frame split)"""
    from ..datasets import sequence_dir as sd
    if args.dataset_conf:
        return sd.split_options(args.dataset_conf, split, refine=flags.get("refine", False), fitting=flags.get("fitting", False))
    import glob
    end = args.end if args.end is not None else len(glob.glob(os.path.join(args.data, "images", "*.png"))) - 1
    opt = dict(start=args.start, end=end, skip=args.skip, downscale=int(args.downscale) if args.downscale == int(args.downscale) else args.downscale,
               near=args.near, far=args.far, **flags)
    if frame is not None:
        opt.update(start=frame, end=frame, skip=1)
    return opt


def load_directory(args, split, sampler, device, say=print, frame=None, **flags):
    """`--data`: one split of a sequence directory -> datasets.DeviceFrames; the load is reported on the driver's log"""
    from ..datasets import sequence_dir as sd
    from ..datasets.device_frames import DeviceFrames
    try:
        seq = sd.read_sequence(args.data, args.dataset, split, split_options(args, split, frame=frame, **flags))
        say("[%s] %d frames of %s, SMPL parameters from %s" % (split, len(seq.image_files), args.data, seq.pose_file))
        return DeviceFrames.from_directory(seq, sampler, device, log=lambda line: say("[%s] %s" % (split, line)))
    except sd.SequenceError as e:
        raise SystemExit("--data %s: %s" % (args.data, e))
