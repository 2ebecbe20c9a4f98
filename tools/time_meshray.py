"""GPU time of the ray queries (csrc/ia_meshray.hip) on the synthetic model's canonical mesh and its simplified version: the camera rays
of `canonical_front` (`raster.look_at_box`) as first hit and as hit count, with and without Morton-sorted rays; the same rays through a
1-cell (brute-force) grid and the rasteriser's time for that view, for context only; `contains` and a signed `compare`.  HIP events around
every stage, the median of `--repeat` runs after one warm-up.

    python tools/time_meshray.py --resolution 256 --cell 4 --out profiles/meshray_timing.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--cell", type=float, default=4.0, help="--simplify cell edge in lattice spacings")
    ap.add_argument("--size", type=int, default=512, help="the edge of the view in pixels: size^2 rays")
    ap.add_argument("--points", type=int, default=1000000, help="points of `contains` and samples per direction of the signed `compare`")
    ap.add_argument("--brute-rays", type=int, default=16384, help="rays of the 1-cell grid run on the extracted mesh")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import mesh as M, meshdist as D, raster
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
        return statistics.median([timed(fn) for _ in range(args.repeat + 1)][1:])

    big = model.extract_mesh(resolution=args.resolution)
    lo, hi = M.field_box(model.net_coarse)
    extent = float((hi.astype(np.float64) - lo.astype(np.float64)).max())
    spacing = extent / (args.resolution - 1)
    small = model.simplify_mesh(big, args.cell * spacing)
    cam = raster.look_at_box(lo, hi, args.size, "cuda:0")
    c2w = torch.linalg.inv(cam.w2c.double())
    d = (cam.rays_d().double() @ c2w[:3, :3].T).float().contiguous()
    o = c2w[:3, 3].float().expand_as(d).contiguous()
    P = int(o.shape[0])
    lines = ["ray queries on the synthetic model's canonical mesh at resolution %d and its --simplify %g version (%s): the %d x %d camera rays of "
             "canonical_front; GPU time in ms between HIP events, median of %d after a warm-up"
             % (args.resolution, args.cell, torch.cuda.get_device_name(0), args.size, args.size, args.repeat), "",
             "%-11s %9s %15s %-10s %12s %10s %12s %10s %13s %8s" % ("mesh", "faces", "grid", "query", "unsorted ms", "Mrays/s", "sorted ms", "Mrays/s",
                                                                    "tests / ray", "hit %")]
    grids = {}
    for name, m in (("extracted", big), ("simplified", small)):
        g = grids[name] = D.TriangleGrid(m.verts, m.faces)
        for query, run, stat in (("first hit", lambda s, c=False: g.raycast(o, d, counters=c, sort=s), lambda r: (r["face"] >= 0)),
                                 ("count", lambda s, c=False: g.count_hits(o, d, counters=c, sort=s), lambda r: (r["count"] > 0)),
                                 ("any-hit", lambda s, c=False: g.count_hits(o, d, limit=1, counters=c, sort=s), lambda r: (r["count"] > 0))):
            plain, morton = median(lambda: run(False)), median(lambda: run(True))
            r = run(False, True)
            lines.append("%-11s %9d %15s %-10s %12.3f %10.1f %12.3f %10.1f %13.1f %8.1f"
                         % (name, g.nf, "x".join(map(str, g.dims)), query, plain, P / plain / 1e3, morton, P / morton / 1e3,
                            float(r["tests"].double().mean()), 100 * float(stat(r).double().mean())))
    lines += ["", "for context only (another algorithm, another output):"]
    for name, m, n in (("extracted", big, args.brute_rays), ("simplified", small, P)):
        one = D.TriangleGrid(m.verts, m.faces, cell=4.0 * extent, box=(lo, hi))
        k = torch.arange(n, device="cuda:0") * (P // n)
        ob, db = o[k].contiguous(), d[k].contiguous()
        t_one = median(lambda: one.raycast(ob, db, sort=False))
        t_grid = median(lambda: grids[name].raycast(ob, db, sort=False))
        t_rast = median(lambda: raster.rasterize(m.verts, m.faces, cam))
        lines.append("  %-11s first hit of %d of the rays: 1-cell grid %s (every face for every ray) %.3f ms, default grid %.3f ms; raster.rasterize "
                     "of the whole %d x %d view: %.3f ms" % (name, n, "x".join(map(str, one.dims)), t_one, t_grid, args.size, args.size, t_rast))
    pts = (torch.rand((args.points, 3), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(0))
           * torch.as_tensor(hi - lo, device="cuda:0") + torch.as_tensor(lo, device="cuda:0")).float()
    lines.append("")
    for name in ("extracted", "simplified"):
        g = grids[name]
        t_in = median(lambda: g.contains(pts))
        share = float(g.contains(pts).double().mean())
        o3, d3 = pts.repeat(3, 1), torch.as_tensor(D.inside_dirs(), device="cuda:0").repeat_interleave(args.points, 0)
        t_plain, t_sorted = median(lambda: g.count_hits(o3, d3, sort=False)), median(lambda: g.count_hits(o3, d3, sort=True))
        lines.append("contains(%d uniform points of the field's box) on %-11s %9.3f ms, %.2f %% inside; its %d rays alone: unsorted %.3f ms, sorted %.3f ms"
                     % (args.points, name + ":", t_in, 100 * share, 3 * args.points, t_plain, t_sorted))
    rep, rep_s = {}, {}
    t_plain = median(lambda: rep.update(D.compare(big, small, samples=args.points)))
    t_signed = median(lambda: rep_s.update(D.compare(big, small, samples=args.points, signed=True)))
    ba = rep_s["b_to_a"]
    lines += ["", "compare(extracted, simplified, samples = %d), host reads and both grid builds included: %.3f ms; with signed=True: %.3f ms"
              % (args.points, t_plain, t_signed),
              "  simplified relative to extracted: signed mean %+.4e m = %+.4f lattice spacings (unsigned mean %.4e m), %.2f %% of its samples inside"
              % (ba["signed_mean"], ba["signed_mean"] / spacing, ba["mean"], 100 * ba["inside_share"]),
              "",
              "first hit = ia_meshray_closest, count = ia_meshray_count without a limit, any-hit = ia_meshray_count with limit = 1",
              "sorted    = adds the entry points, the Morton keys, the sort, the gather of the rays and the scatter of the results",
              "tests / ray = ray-triangle evaluations per ray (the kernel's own counter)",
              "Measured with tools/time_meshray.py.  First figures: nothing to compare with, no target.  Not profiled with hardware counters: "
              "nothing here says where the kernel's time goes."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
