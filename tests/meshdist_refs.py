"""Float64 numpy references of the surface distance ("surface distance"; include/instantavatar_hip_meshdist.h),
written from the rules: brute force over all valid faces with the Voronoi-region classification of the closest point (Ericson,
Real-Time Collision Detection 5.1.5) and the (d2, face index) rule, the surface sampling, the statistics of `compare`."""
import math

import numpy as np

import meshops_refs as mo
from meshops_refs import cube, cube_surface_distance, fan, icosphere, plane_grid  # noqa: F401  (the meshes the tests share)

PLASTIC = 1.32471795724474602596
REGIONS = ("v0", "v1", "e01", "v2", "e02", "e12", "face")


def valid_faces(verts, faces):
    """[nf] bool and n [nf,3] float64: the meshops validity, and n = (p1 - p0) x (p2 - p0) finite and not zero"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = mo.valid_faces(v, f) if len(f) else np.zeros(0, bool)
    n = np.zeros((len(f), 3))
    if ok.any():
        p = v.astype(np.float64)[f[ok]]
        with np.errstate(all="ignore"):
            n[ok] = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        ok = ok & np.isfinite(n).all(1) & (n != 0).any(1)
        n[~ok] = 0
    return ok, n


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def point_triangles(p, a, b, c):
    """closest points of triangles (a, b, c) [..., 3] to points p [..., 3] (broadcast) in float64
    -> (d2, bary [..., 3], closest [..., 3], region [...] index into REGIONS)"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    shape = np.broadcast(d1, d6).shape
    region = np.full(shape, 6, np.int64)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    for k in range(5, -1, -1):                              # the first condition that holds wins
        region = np.where(np.broadcast_to(conds[k], shape), k, region)
    with np.errstate(all="ignore"):
        e01, e02, e12 = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        fv, fw = vb * den, vc * den
    one, zero = np.ones(shape), np.zeros(shape)
    bc = lambda x: np.broadcast_to(x, shape)
    u = np.choose(region, [one, zero, 1.0 - bc(e01), zero, 1.0 - bc(e02), zero, (1.0 - bc(fv)) - bc(fw)])
    v = np.choose(region, [zero, one, bc(e01), zero, zero, 1.0 - bc(e12), bc(fv)])
    w = np.choose(region, [zero, zero, zero, one, bc(e02), bc(e12), bc(fw)])
    close = (u[..., None] * a + v[..., None] * b) + w[..., None] * c
    e = p - close
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2], np.stack([u, v, w], -1), close, region


def face_distances2(points, verts, faces, chunk=256):
    """[P, F] float64 squared distances to every face, +inf for the faces that are not valid"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok, _ = valid_faces(verts, faces)
    pts = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.full((len(pts), len(f)), np.inf)
    if ok.any():
        t = v[f[ok]]
        for s in range(0, len(pts), chunk):
            with np.errstate(all="ignore"):
                out[s:s + chunk][:, ok] = point_triangles(pts[s:s + chunk, None], t[None, :, 0], t[None, :, 1], t[None, :, 2])[0]
    return out


def closest(points, verts, faces):
    """-> dict(dist [P] float64, d2, face [P] int64, bary [P,3], point [P,3], second [P] = the smallest distance of another face) by
    brute force: the face with the lexicographically smallest (d2, face index); NaN / -1 / 0 / p for a point that is not finite,
    +inf / -1 for a mesh without valid faces"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    P = len(pts)
    fin = np.isfinite(pts).all(1)
    D = face_distances2(np.where(fin[:, None], pts, 0), verts, faces)
    out = dict(d2=np.full(P, np.inf), face=np.full(P, -1, np.int64), bary=np.zeros((P, 3)), point=pts.astype(np.float64), second=np.full(P, np.inf))
    if D.shape[1] and np.isfinite(D).any():
        best = D.argmin(1)                                   # (argmin returns the first, i.e. the smallest index, of equal values)
        d2 = D[np.arange(P), best]
        t = v[f[np.where(np.isfinite(d2), best, 0)]]
        _, bary, close, _ = point_triangles(np.where(fin[:, None], pts, 0).astype(np.float64), t[:, 0], t[:, 1], t[:, 2])
        got = fin & np.isfinite(d2)
        out["d2"] = np.where(got, d2, np.inf)
        out["face"] = np.where(got, best, -1)
        out["bary"] = np.where(got[:, None], bary, 0.0)
        out["point"] = np.where(got[:, None], close, pts.astype(np.float64))
        if D.shape[1] > 1:
            E = D.copy()
            E[np.arange(P), best] = np.inf
            out["second"] = np.sqrt(E.min(1))
    out["d2"] = np.where(fin, out["d2"], np.nan)
    out["dist"] = np.sqrt(out["d2"])
    return out


def tolerance(d_ref, L):
    """|dist - d_ref| <= 2^-22 (d_ref + L), L = the diagonal of the box around the points and the mesh: the fp32 rounding of the result is
    2^-24 relative, the fp64 evaluation contributes at most sqrt(64 x 2^-52) L = 2^-23 L; the tolerance doubles this"""
    return 2.0 ** -22 * (np.asarray(d_ref, np.float64) + L)


def decided(ref, L):
    """[P] bool: the best and the second-best face of `closest` differ by more than the tolerance, so the face index is determined"""
    with np.errstate(invalid="ignore"):
        return (ref["face"] >= 0) & (ref["second"] - ref["dist"] > tolerance(ref["dist"], L))


def diagonal(*arrays):
    p = np.concatenate([np.asarray(a, np.float64).reshape(-1, 3) for a in arrays])
    p = p[np.isfinite(p).all(1)]
    return float(np.linalg.norm(p.max(0) - p.min(0)))


def queries(verts, faces, total=4096, seed=5):
    """-> (points [total,3] fp32, n_uniform): first n_uniform points uniform in twice the mesh's box, then the mesh's own vertices, its
    edge midpoints and face centroids, the box's centre, 64 points 100 box diagonals away and 8 points with a NaN or an inf"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64)
    rng = np.random.RandomState(seed)
    lo, hi = v.min(0), v.max(0)
    c, e = (lo + hi) / 2, hi - lo
    edges = np.unique(np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1), axis=0)
    d = rng.standard_normal((64, 3))
    far = c + 100.0 * np.linalg.norm(e) * d / np.linalg.norm(d, axis=1, keepdims=True)
    bad = np.array([[np.nan, 0, 0], [0, np.nan, 0], [0, 0, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [0.1, 0.2, np.inf], [np.nan, np.nan, np.nan],
                    [np.inf, np.nan, -np.inf]])
    special = np.concatenate([v, v[edges].mean(1), v[f].mean(1), c[None], far, bad])
    n = total - len(special)
    assert n > 0
    return np.concatenate([c + (rng.rand(n, 3) - 0.5) * 2.0 * e, special]).astype(np.float32), n


# ---- sampling --------------------------------------------------------------------------------------------------------------------------
def areas(verts, faces):
    _, n = valid_faces(verts, faces)
    return np.sqrt((n * n).sum(1)) * 0.5


def sample(verts, faces, n):
    """-> dict(points [n,3] float64 (before the rounding to fp32), face [n], bary [n,3], t [n], cum [nf])"""
    v = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    cum = np.cumsum(areas(verts, faces))
    A = cum[-1]
    i = np.arange(n, dtype=np.float64)
    t = ((i + 0.5) / np.float64(max(n, 1))) * A
    face = np.minimum(np.searchsorted(cum, t, side="right"), len(f) - 1)       # the first f with cum[f] > t
    a1, a2 = 1.0 / PLASTIC, 1.0 / (PLASTIC * PLASTIC)
    r1, r2 = 0.5 + i * a1, 0.5 + i * a2
    r1, r2 = r1 - np.floor(r1), r2 - np.floor(r2)
    flip = r1 + r2 > 1.0
    r1, r2 = np.where(flip, 1.0 - r1, r1), np.where(flip, 1.0 - r2, r2)
    p = v[f[face]]
    pts = (p[:, 0] + r1[:, None] * (p[:, 1] - p[:, 0])) + r2[:, None] * (p[:, 2] - p[:, 0])
    return dict(points=pts, face=face, bary=np.stack([(1.0 - r1) - r2, r1, r2], 1), t=t, cum=cum)


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def percentile(d, q):
    s = np.sort(np.asarray(d, np.float64))
    return float(s[int(math.ceil(q * len(s))) - 1])


def direction(d):
    d = np.asarray(d, np.float64)
    return dict(mean=float(d.mean()), rms=float(np.sqrt((d * d).mean())), p50=percentile(d, 0.5), p95=percentile(d, 0.95), max=float(d.max()))


def unit_normals(verts, faces):
    _, n = valid_faces(verts, faces)
    ln = np.sqrt((n * n).sum(1))
    return n / np.where(ln > 0, ln, 1.0)[:, None]


def report(d_ab, d_ba, cons_ab=None, cons_ba=None, taus=()):
    """the dict of `meshdist.compare` from the two directions' distances (and their |n_src . n_dst|)"""
    out = dict(a_to_b=direction(d_ab), b_to_a=direction(d_ba))
    out["chamfer"] = (out["a_to_b"]["mean"] + out["b_to_a"]["mean"]) / 2
    out["hausdorff"] = max(out["a_to_b"]["max"], out["b_to_a"]["max"])
    if cons_ab is not None:
        out["normal_consistency"] = float(np.concatenate([cons_ab, cons_ba]).mean())
    out["f_score"] = {}
    for t in taus:
        p, r = float((np.asarray(d_ab) <= t).mean()), float((np.asarray(d_ba) <= t).mean())
        out["f_score"][float(t)] = 2 * p * r / (p + r) if p + r > 0 else 0.0
    return out
