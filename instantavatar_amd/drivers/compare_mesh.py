"""Measure the distance between two triangle meshes on the GPU.

    python -m instantavatar_amd.drivers.compare_mesh meshes/a/canonical.ply scan.obj --samples 200000 --tau 0.005 0.01 --out report/

A and B are PLY or OBJ files (`Mesh.from_ply` / `Mesh.from_obj`: what the extract_mesh driver writes, or plain files).  The table
holds, for each direction, the mean, the root mean square, the median, the 95th percentile and the maximum of the distances from
--samples deterministic surface samples of one mesh to the other (0: from its vertices), then the Chamfer distance -- the mean of
the two directions' mean UNSQUARED distances --, the Hausdorff distance of the samples, the normal consistency and one F-score per
--tau (`meshdist.compare`; DESIGN.md section 4, "surface distance").  --out DIR writes `compare.json` with those numbers and
`a_error.ply` / `b_error.ply`: each mesh with every vertex coloured by its distance to the other, blue (0) over green to red
(--heat-max and more; default: the Hausdorff distance of the report).  --signed adds, per direction, on which side of the other mesh the
samples lie ("ray queries"): the mean signed distance, its 5th and 95th percentile and the share of samples inside
-- negative means inside the other mesh, which must be a closed surface."""
import argparse
import json
import os
import sys


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a", metavar="A", help="a .ply or .obj file")
    ap.add_argument("b", metavar="B", help="a .ply or .obj file")
    ap.add_argument("--samples", type=int, default=100000, help="surface samples per direction (0: the vertices)")
    ap.add_argument("--tau", type=float, nargs="*", default=[], metavar="T", help="distance thresholds of the F-scores")
    ap.add_argument("--heat-max", type=float, default=None, help="--out: the distance that is drawn red (default: the report's Hausdorff distance)")
    ap.add_argument("--signed", action="store_true", help="also report the signed distances (negative: inside the other, closed, mesh)")
    ap.add_argument("--out", default="", metavar="DIR", help="write compare.json, a_error.ply and b_error.ply there")
    args = ap.parse_args(argv)
    for path in (args.a, args.b):
        if not path.lower().endswith((".ply", ".obj")):
            ap.error("%s: meshes are read from .ply and .obj files" % path)
        if not os.path.isfile(path):
            ap.error("%s: no such file" % path)
    if args.samples < 0:
        ap.error("--samples %d: the number of samples cannot be negative" % args.samples)
    if any(not t >= 0 for t in args.tau):
        ap.error("--tau: a threshold must be a distance >= 0")
    if args.heat_max is not None and not args.heat_max > 0:
        ap.error("--heat-max %g: the distance must be positive" % args.heat_max)
    import torch
    from .. import meshdist
    from ..mesh import Mesh
    device = torch.device("cuda:0")
    load = lambda path: (Mesh.from_ply if path.lower().endswith(".ply") else Mesh.from_obj)(path, device)
    a, b = load(args.a), load(args.b)
    report = a.compare(b, samples=args.samples, taus=args.tau, signed=True) if args.signed else a.compare(b, samples=args.samples, taus=args.tau)
    print("A = %s: %d vertices, %d faces;  B = %s: %d vertices, %d faces" % (args.a, a.verts.shape[0], a.faces.shape[0], args.b, b.verts.shape[0],
                                                                              b.faces.shape[0]))
    print("\n".join(meshdist.report_table(report)))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "compare.json"), "w") as out:
            json.dump(meshdist.report_json(dict(report, a=args.a, b=args.b)), out, indent=1, sort_keys=True)
        top = args.heat_max if args.heat_max is not None else report["hausdorff"]
        top = top if top > 0 and top == top and top != float("inf") else 1.0
        for name, m, other in (("a", a, b), ("b", b, a)):
            Mesh(m.verts, m.faces, m.normals, meshdist.heat(m.distance_to(other)["dist"], top)).to_ply(os.path.join(args.out, name + "_error.ply"))
        print("wrote compare.json, a_error.ply and b_error.ply to %s (red = %.5e)" % (args.out, top))
    return 0


if __name__ == "__main__":
    sys.exit(main())
