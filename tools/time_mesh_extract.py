"""Wall time of `AvatarModel.extract_mesh` on the synthetic model, split into field evaluation, count + emit, component
filter and vertex attributes (`timings=`: a synchronisation after every stage), best of `--repeat` runs after one warm-up.

    python tools/time_mesh_extract.py --resolutions 256 512 --out profiles/mesh_extract_timing.txt"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from instantavatar_amd.pipeline import build_synthetic_model
    model, _, _ = build_synthetic_model("cuda:0")
    lines = ["extract_mesh on the synthetic model (%s), level 10, largest component, cap on; wall time in ms, best of %d after a warm-up"
             % (torch.cuda.get_device_name(0), args.repeat),
             "%10s %10s %10s %12s %12s %12s %12s %12s" % ("resolution", "vertices", "faces", "field", "count+emit", "component", "attributes", "total")]
    for res in args.resolutions:
        best = None
        for _ in range(args.repeat + 1):
            t = {}
            mesh = model.extract_mesh(resolution=res, timings=t)
            if _ and (best is None or sum(t.values()) < sum(best.values())):
                best = t
        lines.append("%10d %10d %10d %12.2f %12.2f %12.2f %12.2f %12.2f" % (
            res, mesh.verts.shape[0], mesh.faces.shape[0], 1e3 * best["field"], 1e3 * best["isosurface"], 1e3 * best["component"],
            1e3 * best["attributes"], 1e3 * sum(best.values())))
        del mesh
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
