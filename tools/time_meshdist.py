"""GPU time of the surface distance (csrc/ia_meshdist.hip) on the synthetic model's canonical mesh and its simplified version: grid count +
build, surface sampling, closest point for surface samples in both directions with and without Morton-sorted queries, a whole
`compare`, and for scale the 1-cell (brute-force) grid.  HIP events around every stage, the median of `--repeat` runs after one warm-up.

    python tools/time_meshdist.py --resolution 256 --cell 4 --out profiles/meshdist_timing.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--cell", type=float, default=4.0, help="--simplify cell edge in lattice spacings")
    ap.add_argument("--points", type=int, default=1000000, help="surface samples per direction")
    ap.add_argument("--brute-points", type=int, default=100000, help="points of the 1-cell grid run")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, mesh as M, meshdist as D
    from instantavatar_amd.pipeline import build_synthetic_model
    model, _, _ = build_synthetic_model("cuda:0")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def median(fn):
        ms = [timed(fn) for _ in range(args.repeat + 1)][1:]
        return statistics.median(ms)

    big = model.extract_mesh(resolution=args.resolution)
    lo, hi = M.field_box(model.net_coarse)
    spacing = float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / (args.resolution - 1)
    small = model.simplify_mesh(big, args.cell * spacing)
    meshes = {"extracted": big, "simplified": small}
    lines = ["surface distance on the synthetic model's canonical mesh at resolution %d and its --simplify %g version (%s): GPU time in ms "
             "between HIP events, median of %d after a warm-up" % (args.resolution, args.cell, torch.cuda.get_device_name(0), args.repeat), ""]
    grids, samples = {}, {}
    lines.append("%-11s %9s %9s %15s %8s %11s %10s %10s %12s" % ("mesh", "vertices", "faces", "grid", "cell", "pairs", "count ms", "build ms",
                                                                "sample ms"))
    for name, m in meshes.items():
        g = grids[name] = D.TriangleGrid(m.verts, m.faces)
        count = torch.empty(1, dtype=torch.int64, device="cuda:0")
        t_count = median(lambda: _lib.call("ia_meshdist_grid_count", g.verts, g.faces, g.nv, g.nf, *g.geo, count))
        t_build = median(lambda: _lib.call("ia_meshdist_grid_build", g.verts, g.faces, g.nv, g.nf, *g.geo, g.n_pairs, g.ws, g.nbytes))
        samples[name] = D.sample_surface(m, args.points)
        cum = torch.cumsum(D.face_areas(g.verts, g.faces), 0)
        s = samples[name]
        t_sample = median(lambda: _lib.call("ia_meshdist_sample", g.verts, g.faces, g.nv, g.nf, cum.data_ptr(), args.points, s["points"], s["face"],
                                            s["bary"]))
        lines.append("%-11s %9d %9d %15s %8.5f %11d %10.3f %10.3f %12.3f" % (name, g.nv, g.nf, "x".join(map(str, g.dims)), g.cell, g.n_pairs,
                                                                           t_count, t_build, t_sample))
    lines += ["", "closest point of %d surface samples of one mesh on the other (kernel alone; `sorted` adds the Morton keys, the sort, the gather of "
              "the queries and the scatter of the results)" % args.points,
              "%-26s %12s %12s %14s %14s" % ("direction", "unsorted ms", "sorted ms", "tests / point", "of brute force")]
    for src, dst in (("extracted", "simplified"), ("simplified", "extracted")):
        g, pts = grids[dst], samples[src]["points"]
        plain = median(lambda: g.closest(pts, sort=False))
        morton = median(lambda: g.closest(pts, sort=True))
        tests = float(g.closest(pts, counters=True, sort=False)["tests"].double().mean())
        lines.append("%-26s %12.3f %12.3f %14.1f %14.5f" % (src + " -> " + dst, plain, morton, tests, tests / max(g.nf, 1)))
    rep = {}
    t_compare = median(lambda: rep.update(D.compare(big, small, samples=args.points)))
    lines += ["", "compare(extracted, simplified, samples = %d), host reads and both grid builds included: %.3f ms" % (args.points, t_compare),
              "  chamfer %.4e m = %.4f lattice spacings, hausdorff %.4e m = %.4f spacings, normal consistency %.4f"
              % (rep["chamfer"], rep["chamfer"] / spacing, rep["hausdorff"], rep["hausdorff"] / spacing, rep["normal_consistency"])]
    one = D.TriangleGrid(small.verts, small.faces, cell=4.0 * float((hi.astype(np.float64) - lo.astype(np.float64)).max()))
    few = samples["extracted"]["points"][:: max(1, args.points // args.brute_points)][:args.brute_points].contiguous()
    g = grids["simplified"]
    t_brute = median(lambda: one.closest(few, sort=False))
    t_grid = median(lambda: g.closest(few, sort=False))
    lines += ["", "for scale, %d of those samples on the simplified mesh: 1-cell grid %s (every face for every point) %.3f ms, default grid %.3f ms"
              % (few.shape[0], "x".join(map(str, one.dims)), t_brute, t_grid),
              "",
              "count     = ia_meshdist_grid_count: the number of (face, cell) pairs",
              "build     = ia_meshdist_grid_build: face records, cell counts, scan, lists",
              "sample    = ia_meshdist_sample: %d samples (binary search in the area prefix sum, R2 point in the face)" % args.points,
              "Measured with tools/time_meshdist.py.  First figures: nothing to compare with; only the default of `sort` was chosen from them."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
