"""Collect OpenPose's per-frame JSON files into the keypoints.npy that `refine_smpl` and `inspect_sequence` read
(scripts/custom/convert_openpose_json_to_npy.py of the reference):

    python -m instantavatar_amd.drivers.convert_openpose --json-dir DIR/openpose [--output keypoints.npy]

reads the *.json files of --json-dir in sorted order, takes `people[0].pose_keypoints_2d` of each (75 numbers: x, y, confidence of the 25
BODY_25 points) and writes the [F,25,3] float64 array to --output, a path relative to the PARENT of --json-dir as in the reference (so
the default lands at DIR/keypoints.npy).  CPU only.

One deviation: a frame in which OpenPose found nobody (`people` is empty) gives a row of zeros -- confidence 0, so neither the
refinement nor the inspection looks at it -- and is named in the report, where the reference script stops with an IndexError."""
import argparse
import glob
import json
import os

import numpy as np


def _error(path, what):
    from ..datasets.sequence_dir import SequenceError
    return SequenceError("%s: %s" % (path, what))


def convert(json_dir, output="keypoints.npy", log=print):
    """-> dict(path, frames, empty: the names of the files without a person)"""
    json_dir = os.fspath(json_dir)
    if not os.path.isdir(json_dir):
        raise _error(json_dir, "is missing: no directory of OpenPose's JSON files")
    files = sorted(glob.glob(os.path.join(json_dir, "*.json")))
    if not files:
        raise _error(json_dir, "holds no *.json files")
    rows, empty = [], []
    for f in files:
        try:
            with open(f) as fh:
                people = json.load(fh)["people"]
        except (OSError, ValueError, KeyError, TypeError) as e:
            raise _error(f, "not an OpenPose JSON file (%s: %s)" % (type(e).__name__, e))
        if not people:
            rows.append(np.zeros((25, 3)))
            empty.append(os.path.basename(f))
            continue
        try:
            row = np.asarray(people[0]["pose_keypoints_2d"], np.float64)
        except (KeyError, TypeError, ValueError) as e:
            raise _error(f, "people[0] has no usable pose_keypoints_2d (%s: %s)" % (type(e).__name__, e))
        if row.shape != (75,):
            raise _error(f, "pose_keypoints_2d holds %s numbers, BODY_25 has 75" % (row.size if row.ndim == 1 else row.shape,))
        rows.append(row.reshape(25, 3))
    path = os.path.normpath(os.path.join(json_dir, os.pardir, output))
    np.save(path, np.stack(rows))
    log("wrote %s: %d frames of 25 points from %s" % (path, len(rows), json_dir))
    if empty:
        log("no person in %d frame%s (a row of zeros was written): %s" % (len(empty), "" if len(empty) == 1 else "s", ", ".join(empty)))
    return dict(path=path, frames=len(rows), empty=empty)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json-dir", "--json_dir", dest="json_dir", required=True, metavar="DIR")
    ap.add_argument("--output", "--output_file", dest="output", default="keypoints.npy")
    args = ap.parse_args(argv)
    from ..datasets.sequence_dir import SequenceError
    try:
        convert(args.json_dir, args.output)
    except SequenceError as e:
        raise SystemExit("--json-dir %s: %s" % (args.json_dir, e))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
