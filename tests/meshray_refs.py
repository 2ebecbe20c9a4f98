"""Float64 numpy reference of the ray queries ("ray queries"; include/instantavatar_hip_meshray.h), written from the
rules: brute force over ALL valid faces with exactly the header's expressions, comparisons, box clause and (t, face index) rule, the hit
count, and the parity vote of the inside test.  No grid anywhere."""
import re

import numpy as np

import meshdist_refs as md
from meshops_refs import cube, fan, icosphere, plane_grid  # noqa: F401  (the meshes the tests share)

UNCLEAR = 1e-9


def inside_dirs(header_text):
    """the three fp32 directions of the inside test, read from the header's text"""
    rows = re.findall(r"#define IA_MESHRAY_INSIDE_DIR_(\d) (.*)", header_text)
    assert [k for k, _ in rows] == ["0", "1", "2"]
    return np.array([[np.float32(x.strip().rstrip("f")) for x in r.split(",")] for _, r in rows], np.float32)


def rd32(x):
    """the largest fp32 not above the float64 x"""
    with np.errstate(over="ignore"):
        f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f).astype(np.float32)


def ru32(x):
    """the smallest fp32 not below the float64 x"""
    with np.errstate(over="ignore"):
        f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _ranges(P, t_min, t_max):
    t0 = np.zeros(P, np.float32) if t_min is None else np.asarray(t_min, np.float32).reshape(P)
    t1 = np.full(P, np.inf, np.float32) if t_max is None else np.asarray(t_max, np.float32).reshape(P)
    return t0, t1


def valid_rays(o, d, t_min=None, t_max=None):
    o, d = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    t0, t1 = _ranges(len(o), t_min, t_max)
    with np.errstate(invalid="ignore"):
        return np.isfinite(o).all(1) & np.isfinite(d).all(1) & (t0 >= 0) & (t0 <= t1)


def hits(o, d, verts, faces, t_min=None, t_max=None):
    """every ray against every face: dict(hit [P,nf] bool, t, u, v, w, det [P,nf] float64 (as computed, whatever `hit` says), c [P,nf,3]).
    Faces that are not valid never hit; rays that are not valid hit nothing."""
    o32, d32 = np.asarray(o, np.float32).reshape(-1, 3), np.asarray(d, np.float32).reshape(-1, 3)
    P = len(o32)
    t0, t1 = _ranges(P, t_min, t_max)
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = md.valid_faces(v32, f)[0] if len(f) else np.zeros(0, bool)
    p = np.zeros((len(f), 3, 3))
    p32 = np.zeros((len(f), 3, 3), np.float32)
    if ok.any():
        p32[ok] = v32[f[ok]]
        p[ok] = p32[ok].astype(np.float64)
    O, D = o32.astype(np.float64)[:, None, :], d32.astype(np.float64)[:, None, :]
    with np.errstate(all="ignore"):
        p0 = p[None, :, 0]
        e1, e2 = p[None, :, 1] - p0, p[None, :, 2] - p0
        pv = _cross(D, e2)
        det = md._dot(e1, pv)
        inv = 1.0 / det
        tv = O - p0
        u = md._dot(tv, pv) * inv
        qv = _cross(tv, e1)
        v = md._dot(D, qv) * inv
        w = (1.0 - u) - v
        t = md._dot(e2, qv) * inv
        c = O + t[..., None] * D
        hit = (det != 0) & (u >= 0) & (v >= 0) & (w >= 0) & np.isfinite(t) & (t0.astype(np.float64)[:, None] <= t) & (t <= t1.astype(np.float64)[:, None])
        mn, mx = p32.min(1)[None], p32.max(1)[None]
        hit = hit & (rd32(c) <= mx).all(-1) & (ru32(c) >= mn).all(-1)
    hit = hit & ok[None, :] & valid_rays(o32, d32, t0, t1)[:, None]
    return dict(hit=hit, t=t, u=u, v=v, w=w, det=det, c=c, ok=ok)


def closest(o, d, verts, faces, t_min=None, t_max=None, H=None):
    """-> dict(t [P] float64 (+inf: no hit, NaN: a ray that is not valid), face [P] int32, bary [P,3] float64 = (w, u, v))"""
    H = hits(o, d, verts, faces, t_min, t_max) if H is None else H
    P, nf = H["hit"].shape
    t = np.where(H["hit"], H["t"], np.inf)
    face = np.full(P, -1, np.int32)
    best = np.full(P, np.inf)
    bary = np.zeros((P, 3))
    if nf:
        k = np.argmin(t, 1)                                  # the first index among equal t: the (t, face) rule
        got = H["hit"][np.arange(P), k]
        face[got] = k[got]
        best[got] = t[np.arange(P), k][got]
        for n, key in enumerate(("w", "u", "v")):
            bary[got, n] = H[key][np.arange(P), k][got]
    best[~valid_rays(o, d, t_min, t_max)] = np.nan
    return dict(t=best, face=face, bary=bary)


def count(o, d, verts, faces, t_min=None, t_max=None, limit=None, H=None):
    """[P] int32: min(limit, the number of valid faces hit); -1 for a ray that is not valid"""
    H = hits(o, d, verts, faces, t_min, t_max) if H is None else H
    n = H["hit"].sum(1).astype(np.int32)
    if limit is not None:
        n = np.minimum(n, np.int32(limit))
    n[~valid_rays(o, d, t_min, t_max)] = -1
    return n


def unclear(o, d, verts, faces, t_min=None, t_max=None, H=None, eps=UNCLEAR):
    """[P] bool: rays whose result a rounding could change -- some valid face with det != 0 has min(|u|, |v|, |w|) or the distance of
    t to an end of the range below eps, or the two smallest hit t differ by less than eps"""
    H = hits(o, d, verts, faces, t_min, t_max) if H is None else H
    P = H["hit"].shape[0]
    t0, t1 = _ranges(P, t_min, t_max)
    with np.errstate(all="ignore"):
        live = H["ok"][None, :] & (H["det"] != 0) & np.isfinite(H["det"])
        edge = np.minimum(np.minimum(np.abs(H["u"]), np.abs(H["v"])), np.abs(H["w"])) < eps
        end = (np.abs(H["t"] - t0.astype(np.float64)[:, None]) < eps) | (np.abs(H["t"] - t1.astype(np.float64)[:, None]) < eps)
        bad = (live & (edge | end)).any(1)
    t = np.sort(np.where(H["hit"], H["t"], np.inf), 1)
    if t.shape[1] >= 2:
        with np.errstate(invalid="ignore"):
            bad |= np.isfinite(t[:, 1]) & (t[:, 1] - t[:, 0] < eps)
    return bad


def contains(points, verts, faces, dirs):
    """[P] bool: the parity vote over the three directions `dirs` [3,3] fp32 -- inside iff at least two of the three counts are odd;
    a point that is not finite is not inside"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    odd = np.zeros(len(pts), np.int32)
    for k in range(3):
        n = count(pts, np.broadcast_to(np.asarray(dirs, np.float32)[k], pts.shape), verts, faces)
        odd += (n > 0) & (n % 2 == 1)
    return odd >= 2


def t_tolerance(t_ref, o, d, L):
    """|t - fp32(t_ref)| <= 2^-23 |t_ref| + 1e-9 (L + |o|) / |d|: one rounding to fp32, and a generous bound on fp64 differences"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    return 2.0 ** -23 * np.abs(t_ref) + 1e-9 * (L + np.linalg.norm(o, axis=1)) / np.linalg.norm(d, axis=1)


def sphere_hit(o, d, radius):
    """the smallest t >= 0 with |o + t d| = radius (float64), +inf when there is none"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    a, b, c = (d * d).sum(1), (o * d).sum(1), (o * o).sum(1) - radius * radius
    with np.errstate(invalid="ignore"):
        s = np.sqrt(b * b - a * c)
        t_a, t_b = (-b - s) / a, (-b + s) / a
    t = np.where(t_a >= 0, t_a, t_b)
    return np.where(np.isfinite(t) & (t >= 0), t, np.inf)


def slab_hit(o, d, half):
    """first t >= 0 at which the ray meets the SURFACE of the cube [-half, half]^3 (from outside: the entry; from inside: the exit)"""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (-half - o) / d, (half - o) / d
    near, far = np.minimum(ta, tb), np.maximum(ta, tb)
    par = d == 0
    near = np.where(par, np.where(np.abs(o) <= half, -np.inf, np.inf), near)
    far = np.where(par, np.where(np.abs(o) <= half, np.inf, -np.inf), far)
    t_in, t_out = near.max(1), far.min(1)
    t = np.where(t_in >= 0, t_in, t_out)
    return np.where((t_in <= t_out) & (t_out >= 0), t, np.inf)


def probe_rays(seed=7, n=2048):
    """the rays of the GPU tests: n origins on the radius-3 sphere and n in [-0.5, 0.5]^3, aimed at points of the radius-1.3 ball"""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((n, 3))
    outer = 3.0 * a / np.linalg.norm(a, axis=1, keepdims=True)
    inner = rng.uniform(-0.5, 0.5, (n, 3))
    b = rng.standard_normal((2 * n, 3))
    target = 1.3 * b / np.linalg.norm(b, axis=1, keepdims=True) * rng.uniform(0, 1, (2 * n, 1)) ** (1.0 / 3.0)
    o = np.concatenate([outer, inner]).astype(np.float32)
    return o, (target - o.astype(np.float64)).astype(np.float32)


def cube_rays():
    """rays along the cell planes of the cube(8, half=1) lattice, through its edges and vertices; origins outside, on the box's faces and inside"""
    k = np.arange(-4, 5) * 0.25                                                                # the cell planes = the cube's vertex lattice
    a, b = [x.reshape(-1) for x in np.meshgrid(k, k, indexing="ij")]
    o, d = [], []
    for axis in range(3):
        for start, sign in ((-2.0, 1.0), (-1.0, 1.0), (2.0, -1.0), (1.0, -1.0), (0.0, 1.0), (-2.0, -1.0)):     # outside, on the box's face, inside, away
            p = np.zeros((len(a), 3))
            p[:, axis], p[:, (axis + 1) % 3], p[:, (axis + 2) % 3] = start, a, b
            e = np.zeros((len(a), 3))
            e[:, axis] = sign
            o.append(p)
            d.append(e)
    for z in k:                                                                                 # through the cube's vertical edges, along cell diagonals
        o += [[[-2.0, -2.0, z]], [[2.0, -2.0, z]], [[-1.5, -2.0, z]]]
        d += [[[1.0, 1.0, 0.0]], [[-1.0, 1.0, 0.0]], [[1.0, 1.0, 0.0]]]
    o += [[[-2.0, -2.0, -2.0]], [[2.0, 2.0, 2.0]], [[-2.0, -2.0, -2.0]]]                        # through two cube vertices; and twice as fast
    d += [[[1.0, 1.0, 1.0]], [[-0.5, -0.5, -0.5]], [[2.0, 2.0, 2.0]]]
    return np.concatenate(o).astype(np.float32), np.concatenate(d).astype(np.float32)


def shell(subdivisions=2, outer=1.0, inner=0.5):
    """two concentric icospheres as one mesh: inside means between them"""
    v, f = icosphere(subdivisions)
    return np.concatenate([v * np.float32(outer), v * np.float32(inner)]), np.concatenate([f, f[:, ::-1] + len(v)]).astype(np.int32)
