"""GPU time of the mesh processing (csrc/ia_meshops.hip) on the synthetic model's canonical mesh: adjacency build, 10 Taubin
iterations, cluster count + emit with a cell of K lattice spacings, vertex normals of the input mesh.  HIP events around every stage, the median of `--repeat` runs after one warm-up.

    python tools/time_meshops.py --resolutions 256 512 --cell 4 --out profiles/meshops_timing.txt"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolutions", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--cell", type=float, default=4.0, help="cell edge in lattice spacings")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    from instantavatar_amd import _lib, mesh as M
    from instantavatar_amd.pipeline import build_synthetic_model
    model, _, _ = build_synthetic_model("cuda:0")
    dev = "cuda:0"

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    lines = ["mesh processing on the synthetic model's canonical mesh (%s): GPU time in ms between HIP events, median of %d after a warm-up"
             % (torch.cuda.get_device_name(0), args.repeat),
             "Taubin: %d iterations (lambda 0.5, mu -0.53); clustering: cell = %g lattice spacings, reg 1e-3" % (args.iters, args.cell),
             "%10s %10s %10s %10s %10s %10s %10s %10s %10s %10s" % ("resolution", "vertices", "faces", "adjacency", "taubin", "count", "emit",
                                                                "normals", "verts out", "faces out")]
    for res in args.resolutions:
        m = model.extract_mesh(resolution=res)
        lo, hi = M.field_box(model.net_coarse)
        cell = args.cell * float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / (res - 1)
        nv, nf = m.verts.shape[0], m.faces.shape[0]
        n = M.cluster_grid(lo, hi, cell)
        h = np.float32(cell)
        geo = [float(x) for x in lo] + [float(x) for x in hi] + [float(h), float(np.float32(1.0 / np.float64(h)))]
        na = int(_lib.call("ia_mesh_adjacency_workspace_bytes", nv, nf))
        nc = int(_lib.call("ia_mesh_cluster_workspace_bytes", nv, nf, n[0] * n[1] * n[2]))
        wa, wc = torch.empty(na, dtype=torch.uint8, device=dev), torch.empty(nc, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        out, nrm, vmap = torch.empty((nv, 3), device=dev), torch.empty((nv, 3), device=dev), torch.empty(nv, dtype=torch.int32, device=dev)
        _lib.call("ia_mesh_cluster_count", m.verts, m.faces, nv, nf, *geo, wc, nc, counts)
        nv2, nf2 = counts.tolist()
        v2, c2, f2 = torch.empty((nv2, 3), device=dev), torch.empty((nv2, 3), device=dev), torch.empty((nf2, 3), dtype=torch.int32, device=dev)
        stages = {
            "adjacency": lambda: _lib.call("ia_mesh_adjacency_build", m.verts, m.faces, nv, nf, wa, na),
            "taubin": lambda: _lib.call("ia_mesh_taubin", m.verts, nv, nf, wa, na, 0.5, -0.53, args.iters, out),
            "count": lambda: _lib.call("ia_mesh_cluster_count", m.verts, m.faces, nv, nf, *geo, wc, nc, counts),
            "emit": lambda: _lib.call("ia_mesh_cluster_emit", m.verts, m.faces, m.colors, nv, nf, *geo, 1e-3, wc, nc, v2, nv2, f2, nf2, c2, vmap),
            "normals": lambda: _lib.call("ia_mesh_vertex_normals", m.verts, m.faces, nv, nf, wa, na, nrm),
        }
        ms = {k: [] for k in stages}
        for r in range(args.repeat + 1):
            for k, fn in stages.items():
                t = timed(fn)
                if r:
                    ms[k].append(t)
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append("%10d %10d %10d %10.3f %10.3f %10.3f %10.3f %10.3f %10d %10d" % (
            res, nv, nf, med["adjacency"], med["taubin"], med["count"], med["emit"], med["normals"], nv2, nf2))
        del m, wa, wc, out, nrm, vmap, v2, c2, f2
        torch.cuda.empty_cache()
    lines += ["",
              "adjacency = ia_mesh_adjacency_build: per vertex its faces and its distinct neighbours (count, scan, fill, sort per list)",
              "taubin    = ia_mesh_taubin: 2 x iterations half-steps over the neighbour lists",
              "count     = ia_mesh_cluster_count: cells, rank of the occupied cells, kept faces / clusters, corner and member lists",
              "emit      = ia_mesh_cluster_emit: faces, vertex map, one quadric and one 3 x 3 solve per kept cluster",
              "normals   = ia_mesh_vertex_normals on the input mesh (the simplified mesh's are cheaper in proportion)",
              "Measured with tools/time_meshops.py.  First figures: nothing to compare with, nothing tuned."]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
