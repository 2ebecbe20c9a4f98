"""Distance between surfaces: the closest point of a triangle mesh for many query points on the GPU (csrc/ia_meshdist.hip,
include/instantavatar_hip_meshdist.h; definitions in DESIGN.md section 4, "surface distance"), deterministic surface samples, and what
follows from the two: Chamfer and Hausdorff distances, normal consistency, F-scores, attribute transfer by barycentrics, error colours.

    grid = TriangleGrid(verts, faces)            # built once per mesh
    r = grid.closest(points)                     # dist, face, bary, point
    compare(mesh_a, mesh_b, samples=100000)      # the report both ways

The result of a query is the face with the smallest (squared distance, face index) over ALL valid faces, every distance being one
fixed fp64 expression; the grid only prunes, so the bytes of a result do not depend on the grid, and queries may be reordered freely
(`closest(..., sort=True)` walks them along a Morton curve so that the lanes of a wave visit similar cells).

Rays against the same grid (csrc/ia_meshray.hip, include/instantavatar_hip_meshray.h; DESIGN.md section 4, "ray queries"): the first
hit, the number of faces hit, and from the count a line-of-sight test, an inside test and the sign of the distance:

    r = grid.raycast(origins, dirs)              # t, face, bary, point
    grid.occluded(a, b)                          # is the segment a -> b blocked?
    grid.contains(points)                        # inside a closed surface (parity of three skewed rays)
    grid.signed_distance(points)                 # `closest`, negative inside
    compare(mesh_a, mesh_b, signed=True)         # ... and on which side the other surface lies"""
import math
import re

import numpy as np
import torch

from . import _lib

MAX_CELLS = 1 << 24
MAX_PAIRS = 2 ** 31 - 1
PLASTIC = 1.32471795724474602596
#: when `sort` is None, `closest` sorts the queries along a Morton curve from this many points and this many grid cells on.  Measured
#: (profiles/meshdist_timing.txt, 10^6 surface samples): on a grid of 4.7 M cells the sorted walk takes 9.3 ms against 12.9 ms, on one
#: of 14 k cells the sort costs more than it saves (1.6 ms against 1.0 ms)
SORT_FROM = 1 << 14
SORT_FROM_CELLS = 1 << 18
_inside_dirs = None


def inside_dirs():
    """[3,3] fp32: the three fixed ray directions of the inside test, as include/instantavatar_hip_meshray.h states them"""
    global _inside_dirs
    if _inside_dirs is None:
        with open(_lib.header_path("meshray")) as f:
            rows = re.findall(r"#define IA_MESHRAY_INSIDE_DIR_\d (.*)", f.read())
        _inside_dirs = np.array([[np.float32(x.strip().rstrip("f")) for x in r.split(",")] for r in rows], np.float32).reshape(3, 3)
    return _inside_dirs


def _mesh_arrays(mesh_or_verts, faces=None):
    if faces is None:
        if isinstance(mesh_or_verts, (tuple, list)):
            mesh_or_verts, faces = mesh_or_verts
        else:
            mesh_or_verts, faces = mesh_or_verts.verts, mesh_or_verts.faces
    verts = mesh_or_verts.detach().reshape(-1, 3).float().contiguous()
    return verts, faces.detach().reshape(-1, 3).to(torch.int32).contiguous()


def face_normals(verts, faces):
    """-> (ok [nf] bool, n [nf,3] fp64): the valid faces of the header's definition -- indices in range, pairwise different, finite
    corners, n = (p1 - p0) x (p2 - p0) finite and not zero in fp64 -- and that n (zero for the others)."""
    nv = verts.shape[0]
    f = faces.long()
    ok = ((f >= 0) & (f < nv)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    if nv == 0 or f.shape[0] == 0:
        return torch.zeros(f.shape[0], dtype=torch.bool, device=verts.device), torch.zeros((f.shape[0], 3), dtype=torch.float64, device=verts.device)
    p = verts.double()[f.clamp(0, nv - 1)]
    ok = ok & torch.isfinite(p).all(2).all(1)
    p = torch.where(ok[:, None, None], p, torch.zeros_like(p))
    n = torch.linalg.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ok = ok & torch.isfinite(n).all(1) & (n != 0).any(1)
    return ok, torch.where(ok[:, None], n, torch.zeros_like(n))


def face_areas(verts, faces):
    """[nf] fp64: |n| / 2 of the valid faces, 0 for the others"""
    _, n = face_normals(verts, faces)
    return torch.sqrt((n * n).sum(1)) * 0.5


def grid_dims(lo, hi, h):
    """cells per axis, max(1, ceil((hi - lo) / h)) in float64 on the fp32 values, as the library forms them"""
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    return [int(x) for x in np.maximum(np.ceil((hi - lo) / np.float64(np.float32(h))), 1.0)]


class TriangleGrid:
    """The uniform grid of the triangles of (verts, faces), built once on the device and read by `closest`.

    box: (lo, hi); default: the bounds of the valid faces' vertices.  cell: the cell edge; default: 2 sqrt(mean area of the valid faces)
    -- about 1.3 edge lengths of an equilateral face of that area, so that a face is listed in a handful of cells and a cell holds a
    handful of faces -- multiplied by 1.26 (a doubling of the cell's volume) until the grid has at most MAX_CELLS = 2^24 cells; the box's
    largest extent (or 1) when there is no valid face.  A tuning choice, not a measured claim: results do not depend on it.
    Host reads: one for the default box / cell, one for the number of (face, cell) pairs."""

    def __init__(self, verts, faces=None, cell=None, box=None):
        self.verts, self.faces = _mesh_arrays(verts, faces)
        self.faces_inside = 1 if box is None else 0         # the box below is the valid faces' own bounds: the ray walk may clip to it
        _lib.require_cuda(self.verts, self.faces)
        dev = self.verts.device
        self.nv, self.nf = int(self.verts.shape[0]), int(self.faces.shape[0])
        if box is None or cell is None:
            ok, n = face_normals(self.verts, self.faces)
            area = torch.sqrt((n * n).sum(1)) * 0.5
            used = torch.zeros(self.nv, dtype=torch.bool, device=dev)
            if self.nf and self.nv:
                used[self.faces.long().clamp(0, self.nv - 1)[ok].reshape(-1)] = True
            v = self.verts.double()
            big = torch.full_like(v, float("inf"))
            stats = torch.cat([torch.where(used[:, None], v, big).amin(0) if self.nv else big.new_zeros(3),
                               torch.where(used[:, None], v, -big).amax(0) if self.nv else big.new_zeros(3),
                               (area.sum() / ok.sum().clamp(min=1)).reshape(1)]).tolist()
            if not all(math.isfinite(x) for x in stats[:6]):
                stats[:6] = [0.0] * 6
            if box is None:
                box = (stats[:3], stats[3:6])
        self.lo, self.hi = np.asarray(box[0], np.float32).reshape(3), np.asarray(box[1], np.float32).reshape(3)
        if not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all()):
            raise _lib.IAError("TriangleGrid: the box is not finite")
        if cell is None:
            extent = float((self.hi.astype(np.float64) - self.lo.astype(np.float64)).max())
            h = np.float32(2.0 * math.sqrt(stats[6])) if stats[6] > 0 else np.float32(extent if extent > 0 else 1.0)
            while not h > 0 or np.prod([float(x) for x in grid_dims(self.lo, self.hi, h)]) > MAX_CELLS:
                h = np.float32(h * 1.26) if h > 0 else np.float32(1.0)
        else:
            h = np.float32(cell)
            if not (h > 0 and np.isfinite(h)):
                raise _lib.IAError("TriangleGrid: the cell edge %r must be positive and finite" % (cell,))
        self.cell = float(h)
        self.dims = grid_dims(self.lo, self.hi, h)
        self.n_cells = self.dims[0] * self.dims[1] * self.dims[2]
        if self.n_cells > MAX_CELLS:
            raise _lib.IAError("TriangleGrid: a grid of %d x %d x %d cells is more than 2^24: enlarge the cell" % tuple(self.dims))
        self.geo = [float(x) for x in self.lo] + [float(x) for x in self.hi] + [float(h), float(np.float32(1.0 / np.float64(h)))]
        count = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.call("ia_meshdist_grid_count", self.verts, self.faces, self.nv, self.nf, *self.geo, count)
        self.n_pairs = int(count.item())
        if self.n_pairs > MAX_PAIRS:
            raise _lib.IAError("TriangleGrid: %d (face, cell) pairs are more than 2^31 - 1: enlarge the cell" % self.n_pairs)
        self.nbytes = int(_lib.call("ia_meshdist_grid_workspace_bytes", self.nf, self.n_cells, self.n_pairs))
        if self.nbytes == 0:
            raise _lib.IAError("TriangleGrid: %d faces, %d cells or %d pairs are beyond the library's caps" % (self.nf, self.n_cells, self.n_pairs))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        _lib.call("ia_meshdist_grid_build", self.verts, self.faces, self.nv, self.nf, *self.geo, self.n_pairs, self.ws, self.nbytes)

    def morton_order(self, points):
        """the permutation that sorts `points` along a 30-bit Morton curve over the grid's box (non-finite coordinates count as lo)"""
        lo = torch.as_tensor(self.lo, device=points.device)
        ext = torch.as_tensor(np.maximum(self.hi - self.lo, np.float32(1e-30)), device=points.device)
        q = (torch.nan_to_num((points - lo) / ext, nan=0.0, posinf=1.0, neginf=0.0).clamp(0, 1) * 1023.0).long()

        def spread(x):
            x = (x | (x << 16)) & 0x30000FF
            x = (x | (x << 8)) & 0x300F00F
            x = (x | (x << 4)) & 0x30C30C3
            return (x | (x << 2)) & 0x9249249
        return torch.argsort(spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2))

    @torch.no_grad()
    def closest(self, points, counters=False, sort=None):
        """-> dict(dist [P] fp32, face [P] int32 (-1: none), bary [P,3] fp32, point [P,3] fp32) and, with counters, tests [P] int32 = the
        point-triangle evaluations made per point.  sort: walk the queries in Morton order and scatter the results back (the bytes
        are the same either way); None: from SORT_FROM points on a grid of SORT_FROM_CELLS cells on.  No host read."""
        _lib.require_cuda(points)
        pts = points.detach().reshape(-1, 3).float().contiguous()
        P, dev = int(pts.shape[0]), pts.device
        out = dict(dist=torch.empty(P, device=dev), face=torch.empty(P, dtype=torch.int32, device=dev), bary=torch.empty((P, 3), device=dev),
                   point=torch.empty((P, 3), device=dev))
        if counters:
            out["tests"] = torch.empty(P, dtype=torch.int32, device=dev)
        if P == 0:
            return out
        order = self.morton_order(pts) if (P >= SORT_FROM and self.n_cells >= SORT_FROM_CELLS if sort is None else sort) else None
        run = out if order is None else {k: torch.empty_like(v) for k, v in out.items()}
        _lib.call("ia_meshdist_closest", pts if order is None else pts[order].contiguous(), P, self.nf, *self.geo, self.n_pairs, self.ws,
                  self.nbytes, run["dist"], run["face"], run["bary"], run["point"], run.get("tests"))
        if order is not None:
            for k in out:
                out[k][order] = run[k]
        return out

    # ---- rays (include/instantavatar_hip_meshray.h) ------------------------------------------------------------------------------
    def _rays(self, origins, dirs, t_min, t_max):
        _lib.require_cuda(origins, dirs)
        o = origins.detach().reshape(-1, 3).float()
        d = dirs.detach().to(o.device).float().expand_as(o) if dirs.dim() == 1 else dirs.detach().reshape(-1, 3).float()
        if d.shape != o.shape:
            raise _lib.IAError("rays: %d origins and %d directions" % (o.shape[0], d.shape[0]))
        P = int(o.shape[0])

        def rng(t):
            if t is None or isinstance(t, torch.Tensor):
                if t is not None and t.numel() != P:
                    raise _lib.IAError("rays: %d origins and a range of %d values" % (P, t.numel()))
                return None if t is None else t.detach().reshape(-1).float().to(o.device).contiguous()
            return torch.full((P,), float(t), device=o.device)
        return o.contiguous(), d.contiguous(), rng(t_min), rng(t_max), P

    def ray_order(self, o, d):
        """the permutation that sorts rays along the Morton curve of the point where they enter the grid's box (their origin when it
        lies inside or the ray misses the box): neighbouring lanes then walk neighbouring cells"""
        lo, hi = torch.as_tensor(self.lo, device=o.device), torch.as_tensor(self.hi, device=o.device)
        ta, tb = (lo - o) / d, (hi - o) / d
        t_in = torch.nan_to_num(torch.minimum(ta, tb), nan=-float("inf")).amax(1).clamp(min=0)
        return self.morton_order(torch.nan_to_num(o + torch.nan_to_num(t_in, posinf=0.0)[:, None] * d, nan=0.0))

    def _walk(self, name, o, d, t0, t1, P, extra, out, sort):
        order = self.ray_order(o, d) if sort else None
        run = out if order is None else {k: torch.empty_like(v) for k, v in out.items()}
        take = (lambda x: x) if order is None else (lambda x: None if x is None else x[order].contiguous())
        _lib.call(name, take(o), take(d), take(t0), take(t1), P, self.nf, *self.geo, self.n_pairs, self.ws, self.nbytes, self.faces_inside,
                  *extra(run))
        if order is not None:
            for k in out:
                out[k][order] = run[k]
        return out

    @torch.no_grad()
    def raycast(self, origins, dirs, t_min=None, t_max=None, counters=False, sort=None):
        """The first hit of the rays o + t d, t in [t_min, t_max] (a number, a tensor [P] or None: 0 / +inf; d is not normalised and may be
        one direction for all): the face with the smallest (t, face index) over ALL valid faces that the ray hits, two-sided.
        -> dict(t [P] fp32 (+inf: no hit; NaN: a ray that is not finite or whose range is not ordered), face [P] int32 (-1: none),
        bary [P,3] fp32 = the weights of the face's corners, point [P,3] fp32 = their barycentric combination, or the origin where
        nothing is hit) and, with counters, tests [P] int32 = ray-triangle evaluations made.  sort=True walks the rays along the
        Morton curve of their entry points and scatters the results back; the bytes are the same either way.  None is False: the rays
        of a camera are coherent as they come, and the sort then costs more than it saves (profiles/meshray_timing.txt).  No host read."""
        o, d, t0, t1, P = self._rays(origins, dirs, t_min, t_max)
        dev = o.device
        out = dict(t=torch.empty(P, device=dev), face=torch.empty(P, dtype=torch.int32, device=dev), bary=torch.empty((P, 3), device=dev))
        if counters:
            out["tests"] = torch.empty(P, dtype=torch.int32, device=dev)
        if P:
            self._walk("ia_meshray_closest", o, d, t0, t1, P, lambda r: (r["t"], r["face"], r["bary"], r.get("tests")), out, sort)
        hit = out["face"] >= 0
        at = interpolate(self.verts, self.faces, out["face"], out["bary"]) if self.nf and self.nv else o
        out["point"] = torch.where(hit[:, None], at, o)
        return out

    @torch.no_grad()
    def count_hits(self, origins, dirs, t_min=None, t_max=None, limit=None, counters=False, sort=None):
        """-> dict(count [P] int32 = min(limit, the number of valid faces the ray hits), each face once; -1 for a ray that is not valid)
        and, with counters, tests [P].  limit = 1 is the any-hit query: the walk ends at the first hit it meets.  None: no limit."""
        o, d, t0, t1, P = self._rays(origins, dirs, t_min, t_max)
        limit = 2 ** 31 - 1 if limit is None else int(limit)
        if limit < 1:
            raise _lib.IAError("count_hits: limit = %d < 1" % limit)
        out = dict(count=torch.empty(P, dtype=torch.int32, device=o.device))
        if counters:
            out["tests"] = torch.empty(P, dtype=torch.int32, device=o.device)
        if P:
            self._walk("ia_meshray_count", o, d, t0, t1, P, lambda r: (limit, r["count"], r.get("tests")), out, sort)
        return out

    def occluded(self, a, b):
        """[P] bool: does the closed segment from a [P,3] to b [P,3] meet the mesh?  (the ray a + t (b - a), t in [0, 1], any-hit;
        b - a is formed in fp32; a segment that is not finite is not occluded)"""
        a = a.detach().reshape(-1, 3).float()
        return self.count_hits(a, b.detach().reshape(-1, 3).float() - a, 0.0, 1.0, limit=1)["count"] > 0

    def contains(self, points, sort=None):
        """[P] bool: is the point inside the mesh?  Each point is the origin of three rays over [0, +inf] with the fixed directions
        `inside_dirs()`; it is inside iff at least two of the three hit an odd number of faces.  This ASSUMES A CLOSED SURFACE (every
        ray that enters also leaves); the orientation of the faces does not matter.  A point that is not finite is not inside."""
        p = points.detach().reshape(-1, 3).float()
        P = int(p.shape[0])
        dirs = torch.as_tensor(inside_dirs(), device=p.device)
        # sort=None: scattered origins are assumed, for which the Morton sort wins from SORT_FROM rays on, on small and large grids
        # alike; surface samples come face by face and are coherent already (`compare` says sort=False) -- profiles/meshray_timing.txt
        n = self.count_hits(p.repeat(3, 1), dirs.repeat_interleave(P, 0), sort=3 * P >= SORT_FROM if sort is None else sort)["count"].reshape(3, P)
        return ((n > 0) & (n % 2 == 1)).sum(0) >= 2

    def signed_distance(self, points, counters=False, sort=None):
        """`closest` with the sign of `contains`: dist is negative inside the (closed) mesh; `inside` [P] bool is added to the dict"""
        out = self.closest(points, counters, sort)
        out["inside"] = self.contains(points, sort)
        out["dist"] = torch.where(out["inside"], -out["dist"], out["dist"])
        return out


def closest(points, mesh_or_verts, faces=None):
    """`TriangleGrid(mesh_or_verts, faces).closest(points)`: the grid is built for this one call"""
    return TriangleGrid(mesh_or_verts, faces).closest(points)


@torch.no_grad()
def sample_surface(mesh, n):
    """n deterministic samples of the surface of `mesh` (a Mesh or (verts, faces)), stratified over the area: sample i lies in the face
    that holds the area coordinate (i + 1/2) / n of the fp64 prefix sum of the face areas, at the i-th point of the R2 sequence folded
    into the triangle.  -> dict(points [n,3] fp32, face [n] int32, bary [n,3] fp32).  One host read: the total area, which must be
    positive and finite."""
    verts, faces = _mesh_arrays(mesh)
    _lib.require_cuda(verts, faces)
    n = int(n)
    if n < 0:
        raise _lib.IAError("sample_surface: n = %d < 0" % n)
    dev = verts.device
    cum = torch.cumsum(face_areas(verts, faces), 0)
    A = float(cum[-1]) if cum.numel() else 0.0
    if not (A > 0 and math.isfinite(A)):
        raise _lib.IAError("sample_surface: the total area of the valid faces is %r: nothing to sample" % A)
    out = dict(points=torch.empty((n, 3), device=dev), face=torch.empty(n, dtype=torch.int32, device=dev), bary=torch.empty((n, 3), device=dev))
    if n:
        _lib.call("ia_meshdist_sample", verts, faces, int(verts.shape[0]), int(faces.shape[0]), cum.data_ptr(), n, out["points"], out["face"],
                  out["bary"])
    return out


def interpolate(values, faces, face, bary):
    """barycentric attribute transfer: out [n,C] = sum_k bary[:, k] values[faces[face, k]], formed in fp64 and returned in the dtype of
    `values`; rows with face = -1 give NaN.  Plain tensor operations, any device."""
    f = face.long()
    idx = faces.long()[f.clamp(min=0)]
    out = (values.double()[idx] * bary.double()[:, :, None]).sum(1)
    out = torch.where((f >= 0)[:, None], out, torch.full_like(out, float("nan")))
    return out.to(values.dtype if values.dtype.is_floating_point else torch.float64)


def heat(d, d_max):
    """[n,3] colours in the model's channel order (B, G, R) for distances d: t = clamp(d / d_max, 0, 1) on the piecewise-linear ramp
    blue (t = 0) -> green (t = 1/2) -> red (t = 1); a distance that is not finite is red."""
    t = torch.nan_to_num(d.float() / float(d_max), nan=1.0, posinf=1.0, neginf=0.0).clamp(0, 1)
    b, r = (1 - 2 * t).clamp(0, 1), (2 * t - 1).clamp(0, 1)
    return torch.stack([b, 1 - b - r, r], 1)


def percentile_index(q, n):
    """the percentile is sorted[ceil(q n) - 1]"""
    return min(max(int(math.ceil(q * n)) - 1, 0), max(n - 1, 0))


def _direction(d):
    """[mean, rms, p50, p95, max] of the distances d (fp64 [n]) as a tensor; NaN when there is none"""
    n = d.numel()
    if n == 0:
        return torch.full((5,), float("nan"), dtype=torch.float64, device=d.device)
    s = torch.sort(d).values
    return torch.stack([d.mean(), torch.sqrt((d * d).mean()), s[percentile_index(0.5, n)], s[percentile_index(0.95, n)], s[n - 1]])


def _unit(n):
    return n / torch.sqrt((n * n).sum(1, keepdim=True)).clamp(min=1e-300)


@torch.no_grad()
def compare(a, b, samples=100000, taus=(), signed=False):
    """The distance report between two meshes (Mesh or (verts, faces)).  -> dict:
      a_to_b, b_to_a   dicts of mean, rms, p50, p95, max of the distances from `samples` surface samples (`sample_surface`) of the
                       source to the other mesh; with samples = 0 from the source's finite vertices; percentile q = sorted[ceil(q n) - 1]
      chamfer          (mean_ab + mean_ba) / 2: UNSQUARED distances, and HALVED (the mean of the two directions, not their sum)
      hausdorff        max(max_ab, max_ba) -- of the samples, so a lower bound of the surfaces' Hausdorff distance
      normal_consistency   the mean over both directions' samples of |n_src . n_dst|, fp64 unit normals of the sample's face and of the
                       closest face; NaN with samples = 0 (a vertex has no face of its own)
      f_score          {tau: 2 P R / (P + R)}, P = share(d_ab <= tau), R = share(d_ba <= tau), 0 when both are 0
      samples          the number of points per direction: [n_a, n_b]
    signed=True adds to each direction, from `TriangleGrid.signed_distance` (negative: the point lies inside the other mesh, which
    must be a closed surface for this to mean anything): signed_mean, inside_share (the share of the points inside), signed_p05 and
    signed_p95.  Every other key keeps its value bit for bit.
    The statistics are fp64 tensor operations gathered into ONE host read at the end; before it, building the two grids reads two
    numbers each and sampling reads each mesh's area."""
    va, fa = _mesh_arrays(a)
    vb, fb = _mesh_arrays(b)
    ga, gb = TriangleGrid(va, fa), TriangleGrid(vb, fb)
    taus = [float(t) for t in taus]
    res, cons, sres = [], [], []
    for (v, f, other, og) in ((va, fa, (vb, fb), gb), (vb, fb, (va, fa), ga)):
        if samples:
            s = sample_surface((v, f), samples)
            pts = s["points"]
        else:
            s, pts = None, v[torch.isfinite(v).all(1)]
        r = og.closest(pts)
        res.append(r["dist"].double())
        if signed:
            sres.append(torch.where(og.contains(pts, sort=False), -res[-1], res[-1]))
        if s is not None:
            n_src = _unit(face_normals(v, f)[1])[s["face"].long().clamp(min=0)]
            n_dst = _unit(face_normals(*other)[1])[r["face"].long().clamp(min=0)]
            cons.append(torch.where(r["face"] >= 0, (n_src * n_dst).sum(1).abs(), torch.full_like(n_src[:, 0], float("nan"))))
    dab, dba = res
    nan = torch.full((1,), float("nan"), dtype=torch.float64, device=va.device)
    share = lambda d, t: (d <= t).double().mean().reshape(1) if d.numel() else nan
    packed = torch.cat([_direction(dab), _direction(dba), torch.cat(cons).mean().reshape(1) if cons else nan]
                       + [share(d, t) for t in taus for d in (dab, dba)]).tolist()          # the one host read
    keys = ("mean", "rms", "p50", "p95", "max")
    out = dict(a_to_b=dict(zip(keys, packed[:5])), b_to_a=dict(zip(keys, packed[5:10])))
    out["chamfer"] = (packed[0] + packed[5]) / 2
    out["hausdorff"] = max(packed[4], packed[9])
    out["normal_consistency"] = packed[10]
    out["f_score"] = {}
    for k, t in enumerate(taus):
        p, r = packed[11 + 2 * k], packed[12 + 2 * k]
        out["f_score"][t] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    out["samples"] = [int(dab.numel()), int(dba.numel())]
    if signed:
        def side(d):
            n = d.numel()
            if n == 0:
                return torch.full((4,), float("nan"), dtype=torch.float64, device=d.device)
            srt = torch.sort(d).values
            return torch.stack([d.mean(), (d < 0).double().mean(), srt[percentile_index(0.05, n)], srt[percentile_index(0.95, n)]])
        extra = torch.cat([side(d) for d in sres]).tolist()      # a second host read, only here
        for key, vals in (("a_to_b", extra[:4]), ("b_to_a", extra[4:])):
            out[key].update(zip(("signed_mean", "inside_share", "signed_p05", "signed_p95"), vals))
    return out


def report_json(report):
    """the dict of `compare` as JSON holds it: F-score keys as strings, a number that is not finite as null"""
    def clean(x):
        if isinstance(x, dict):
            return {str(k): clean(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [clean(v) for v in x]
        return None if isinstance(x, float) and not math.isfinite(x) else x
    return clean(report)


def report_table(report):
    """the lines of the table compare_mesh prints: one row per direction, then the symmetric figures"""
    rows = ["%-8s %12s %12s %12s %12s %12s %9s" % ("", "mean", "rms", "p50", "p95", "max", "samples")]
    for key, n in zip(("a_to_b", "b_to_a"), report["samples"]):
        d = report[key]
        rows.append("%-8s %12.5e %12.5e %12.5e %12.5e %12.5e %9d" % (key, d["mean"], d["rms"], d["p50"], d["p95"], d["max"], n))
        if "signed_mean" in d:
            rows.append("%-8s signed mean %+.5e   p05 %+.5e   p95 %+.5e   inside %.5f   (negative: inside the other mesh)"
                        % ("", d["signed_mean"], d["signed_p05"], d["signed_p95"], d["inside_share"]))
    rows.append("chamfer (unsquared, halved) %.5e   hausdorff %.5e   normal consistency %.5f"
                % (report["chamfer"], report["hausdorff"], report["normal_consistency"]))
    for t, f in report["f_score"].items():
        rows.append("F-score at tau = %g: %.5f" % (float(t), f))
    return rows


# ---- readers of what Mesh.to_ply / to_obj / to_obj_textured write, and of plain PLY / OBJ files -----------------------------------------
_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
              "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _fan(polys):
    out = []
    for p in polys:
        if len(p) < 3:
            raise _lib.IAError("mesh reader: a face with %d vertices" % len(p))
        out += [(p[0], p[k], p[k + 1]) for k in range(1, len(p) - 1)]
    return np.asarray(out, np.int64).reshape(-1, 3)


def read_ply(path):
    """-> (verts [nv,3] f4, faces [nf,3] i4, normals [nv,3] f4 or None, rgb [nv,3] f4 in [0, 1] (RGB order) or None) of a binary
    little-endian or ASCII PLY with vertex properties x y z and optionally nx ny nz / red green blue (other properties are skipped)
    and a face list `vertex_indices` (or `vertex_index`); polygons are fan-triangulated."""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.find(b"end_header")
    if not blob.startswith(b"ply") or end < 0:
        raise _lib.IAError("%s: not a PLY file" % path)
    body = blob.index(b"\n", end) + 1
    fmt, elements = None, []
    for line in blob[:end].decode("ascii", "replace").splitlines():
        w = line.split()
        if not w or w[0] in ("ply", "comment", "obj_info"):
            continue
        if w[0] == "format":
            fmt = w[1]
        elif w[0] == "element":
            elements.append([w[1], int(w[2]), []])
        elif w[0] == "property" and elements:
            elements[-1][2].append(tuple(w[1:]))
    if fmt not in ("binary_little_endian", "ascii"):
        raise _lib.IAError("%s: PLY format %r is not read (binary_little_endian and ascii are)" % (path, fmt))
    vert = faces = None
    tokens = blob[body:].split() if fmt == "ascii" else None
    at = 0 if fmt == "ascii" else body
    for name, count, props in elements:
        lists = [p for p in props if p[0] == "list"]
        for p in props:
            for t in (p[1:3] if p[0] == "list" else p[:1]):
                if t not in _PLY_TYPES:
                    raise _lib.IAError("%s: PLY property type %r" % (path, t))
        if not lists:
            dt = np.dtype([(p[1], "<" + _PLY_TYPES[p[0]]) for p in props])
            if fmt == "ascii":
                rows = np.asarray(tokens[at:at + count * len(props)], dtype=np.float64).reshape(count, len(props))
                at += count * len(props)
                rec = np.empty(count, dt)
                for k, p in enumerate(props):
                    rec[p[1]] = rows[:, k]
            else:
                rec = np.frombuffer(blob, dt, count, at)
                at += count * dt.itemsize
            if name == "vertex":
                vert = rec
            continue
        if len(props) != 1:
            raise _lib.IAError("%s: PLY element %s mixes a list with other properties" % (path, name))
        ct, it = "<" + _PLY_TYPES[props[0][1]], "<" + _PLY_TYPES[props[0][2]]
        polys = None
        if fmt == "ascii":
            polys = []
            for _ in range(count):
                k = int(tokens[at])
                polys.append([int(x) for x in tokens[at + 1:at + 1 + k]])
                at += 1 + k
        else:
            tri = np.dtype([("n", ct), ("v", it, (3,))])
            if at + count * tri.itemsize <= len(blob) and (np.frombuffer(blob, tri, count, at)["n"] == 3).all():
                idx = np.frombuffer(blob, tri, count, at)["v"].astype(np.int64)
                at += count * tri.itemsize
            else:
                polys = []
                for _ in range(count):
                    k = int(np.frombuffer(blob, ct, 1, at)[0])
                    at += np.dtype(ct).itemsize
                    polys.append(np.frombuffer(blob, it, k, at).astype(np.int64).tolist())
                    at += k * np.dtype(it).itemsize
        if polys is not None:
            idx = _fan(polys)
        if name == "face":
            faces = idx
    if vert is None or not all(k in vert.dtype.names for k in "xyz"):
        raise _lib.IAError("%s: the PLY has no vertex element with x, y, z" % path)
    col = lambda names: np.stack([vert[k] for k in names], 1).astype(np.float32) if all(k in vert.dtype.names for k in names) else None
    rgb = col(("red", "green", "blue"))
    if rgb is not None and vert.dtype["red"].kind in "ui":
        rgb = rgb / np.float32(255)
    faces = np.zeros((0, 3), np.int64) if faces is None else faces
    return col("xyz"), faces.astype(np.int32), col(("nx", "ny", "nz")), rgb


def read_obj(path):
    """-> (verts, faces, normals or None, rgb or None) as `read_ply`, of a Wavefront OBJ with `v x y z [r g b]`, optional `vn` and `f`
    with any of the corner forms a, a/t, a//n, a/t/n (1-based); polygons are fan-triangulated, negative (relative) indices are
    refused.  The `vn` are taken as vertex normals when every corner pairs vertex a with normal a, as the writers do."""
    v, vn, polys, paired = [], [], [], True
    with open(path) as fh:
        for ln, line in enumerate(fh, 1):
            w = line.split()
            if not w or w[0].startswith("#"):
                continue
            if w[0] == "v":
                v.append([float(x) for x in w[1:7]])
            elif w[0] == "vn":
                vn.append([float(x) for x in w[1:4]])
            elif w[0] == "f":
                poly = []
                for corner in w[1:]:
                    parts = corner.split("/")
                    a = int(parts[0])
                    if a < 0 or (len(parts) > 2 and parts[2] and int(parts[2]) < 0) or (len(parts) > 1 and parts[1] and int(parts[1]) < 0):
                        raise _lib.IAError("%s, line %d: negative (relative) OBJ indices are not supported: %r" % (path, ln, corner))
                    paired = paired and len(parts) > 2 and parts[2] != "" and int(parts[2]) == a
                    poly.append(a - 1)
                polys.append(poly)
    if v and len({len(r) for r in v}) != 1:
        raise _lib.IAError("%s: `v` lines of different lengths" % path)
    va = np.asarray(v, np.float64).reshape(len(v), -1)
    if len(v) and va.shape[1] not in (3, 4, 6):
        raise _lib.IAError("%s: `v` lines with %d numbers" % (path, va.shape[1]))
    verts = va[:, :3].astype(np.float32) if len(v) else np.zeros((0, 3), np.float32)
    rgb = va[:, 3:6].astype(np.float32) if len(v) and va.shape[1] == 6 else None
    normals = np.asarray(vn, np.float64).astype(np.float32) if vn and paired and polys and len(vn) == len(v) else None
    return verts, _fan(polys).astype(np.int32), normals, rgb


def load_mesh(path, device):
    """a `mesh.Mesh` on `device` from a .ply or .obj file (`read_ply` / `read_obj`): missing normals are `mesh.vertex_normals` of the
    faces, missing colours are 0.5; colours come back in the model's channel order (B, G, R)"""
    from . import mesh as mesh_mod
    ext = str(path).lower().rsplit(".", 1)[-1]
    if ext not in ("ply", "obj"):
        raise _lib.IAError("%s: meshes are read from .ply and .obj files" % path)
    v, f, n, rgb = (read_ply if ext == "ply" else read_obj)(path)
    if len(f) and (f.min() < 0 or f.max() >= max(len(v), 1)) and ext == "obj":
        raise _lib.IAError("%s: a face names vertex %d of %d" % (path, int(f.max()) + 1, len(v)))
    verts = torch.as_tensor(np.ascontiguousarray(v), device=device)
    faces = torch.as_tensor(np.ascontiguousarray(f), device=device)
    colors = torch.as_tensor(np.ascontiguousarray(rgb[:, ::-1]), device=device) if rgb is not None else torch.full((len(v), 3), 0.5, device=device)
    normals = torch.as_tensor(np.ascontiguousarray(n), device=device) if n is not None else mesh_mod.vertex_normals(verts, faces)
    return mesh_mod.Mesh(verts, faces, normals, colors)
