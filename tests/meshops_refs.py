"""Float64 numpy references of the mesh processing ("mesh simplification"; include/instantavatar_hip_meshops.h):
vertex clustering with quadrics, Taubin smoothing, vertex normals from the faces, written from the rules; and the small meshes the
tests of them share.  Sums run in the stated order (np.add.at adds in the order of its index array)."""
import numpy as np

from mesh_refs import canonical_faces, directed_edge_counts, signed_volume  # noqa: F401  (shared with the tests of this module)

MAX_CELLS = 1 << 27
MAX_FACES = (2 ** 31 - 1) // 6


# ---- validity ---------------------------------------------------------------------------------------------------------------------
def finite_vertices(verts):
    return np.isfinite(np.asarray(verts, np.float32)).all(1)


def valid_faces(verts, faces):
    """[nf] bool: indices in [0, nv), pairwise different, all three vertices finite"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(verts)
    ok = ((f >= 0) & (f < nv)).all(1)
    ok &= (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    fin = finite_vertices(verts)
    g = np.clip(f, 0, max(nv - 1, 0))
    if nv:
        ok &= fin[g].all(1)
    return ok


# ---- clustering ---------------------------------------------------------------------------------------------------------------------
def grid_dims(lo, hi, h):
    """cells per axis: max(1, ceil((hi - lo) / h)) in float64 on the fp32 values"""
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    n = np.ceil((hi - lo) / np.float64(np.float32(h)))
    return np.maximum(n, 1).astype(np.int64)


def cell_index(verts, lo, h, n):
    """[nv,3] int64, per axis clamp((int)floorf((p - lo) * inv_h), 0, n - 1) with every operation in fp32, inv_h = fp32(1 / h)"""
    p = np.asarray(verts, np.float32)
    lo32 = np.asarray(lo, np.float32)
    inv_h = np.float32(1.0 / np.float64(np.float32(h)))
    with np.errstate(all="ignore"):
        t = np.floor(((p - lo32[None]).astype(np.float32) * inv_h).astype(np.float32)).astype(np.float64)
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(t, 0, (np.asarray(n) - 1)[None].astype(np.float64)).astype(np.int64)


def simplify(verts, faces, colors, lo, hi, h, reg=1e-3, plain_mean=False):
    """-> dict(verts [M,3] float64 (before the final rounding to fp32), faces [F,3] int32, colors [M,3] float64, vert_cluster [nv] int32,
    centre [M,3] float64 = the cell centre of every output vertex).  plain_mean: the clusters' means instead of the quadric
    minimisers (what the quadric is compared with)."""
    v32 = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    nv = len(v32)
    col = np.asarray(colors, np.float32).reshape(-1, 3).astype(np.float64) if colors is not None else np.zeros((nv, 3))
    h64 = np.float64(np.float32(h))
    assert h64 > 0
    lo64 = np.asarray(lo, np.float32).astype(np.float64)
    n = grid_dims(lo, hi, h)
    assert int(n[0]) * int(n[1]) * int(n[2]) <= MAX_CELLS and len(f) <= MAX_FACES
    fin = finite_vertices(v32)
    ijk = cell_index(v32, lo, h, n)
    key = (ijk[:, 0] * n[1] + ijk[:, 1]) * n[2] + ijk[:, 2]
    key = np.where(fin, key, -1)
    ok = valid_faces(v32, f)
    fv = f[ok]                                              # the valid faces, ascending
    fk = key[fv] if len(fv) else np.zeros((0, 3), np.int64)
    keep = (fk[:, 0] != fk[:, 1]) & (fk[:, 1] != fk[:, 2]) & (fk[:, 0] != fk[:, 2])
    kept_keys = np.unique(fk[keep])                         # ascending key = the numbering of the output
    M = len(kept_keys)
    faces_out = np.searchsorted(kept_keys, fk[keep]).astype(np.int32).reshape(-1, 3)
    pos = np.searchsorted(kept_keys, key)
    pos = np.clip(pos, 0, max(M - 1, 0))
    member = fin & (kept_keys[pos] == key) if M else np.zeros(nv, bool)
    vert_cluster = np.where(member, pos, -1).astype(np.int32)
    out = dict(faces=faces_out, vert_cluster=vert_cluster, verts=np.zeros((M, 3)), colors=np.zeros((M, 3)), centre=np.zeros((M, 3)))
    if M == 0:
        return out
    p = v32.astype(np.float64)
    kz = kept_keys % n[2]
    ky = kept_keys // n[2] % n[1]
    kx = kept_keys // (n[2] * n[1])
    o = lo64[None] + (np.stack([kx, ky, kz], 1).astype(np.float64) + 0.5) * h64
    # members: mean of p - o and of the colours, by ascending vertex index
    mv = np.nonzero(member)[0]
    mc = vert_cluster[mv]
    cnt = np.bincount(mc, minlength=M).astype(np.float64)
    m = np.zeros((M, 3))
    np.add.at(m, mc, p[mv] - o[mc])
    m /= cnt[:, None]
    cm = np.zeros((M, 3))
    np.add.at(cm, mc, col[mv])
    cm /= cnt[:, None]
    # quadric: every corner of every valid face whose vertex lies in a kept cluster, by ascending 3 f + k
    A, b = np.zeros((M, 3, 3)), np.zeros((M, 3))
    if len(fv):
        with np.errstate(all="ignore"):
            p0 = p[fv[:, 0]]
            nrm = np.cross(p[fv[:, 1]] - p0, p[fv[:, 2]] - p0)
            L = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
            good = (L > 0) & np.isfinite(L)
        corner_cluster = vert_cluster[fv].reshape(-1)       # order: 3 f + k over the valid faces
        corner_face = np.repeat(np.arange(len(fv)), 3)
        sel = (corner_cluster >= 0) & good[corner_face]
        cc, cf = corner_cluster[sel], corner_face[sel]
        nh = nrm[cf] / L[cf][:, None]
        a = L[cf] * 0.5
        q = p0[cf] - o[cc]
        d = -(nh[:, 0] * q[:, 0] + nh[:, 1] * q[:, 1] + nh[:, 2] * q[:, 2])
        np.add.at(A, cc, (a[:, None] * nh)[:, :, None] * nh[:, None, :])
        np.add.at(b, cc, (a * d)[:, None] * nh)
    x = m.copy()
    if not plain_mean:
        w = reg * (A[:, 0, 0] + A[:, 1, 1] + A[:, 2, 2])
        solve = (w > 0) & np.isfinite(w)
        if solve.any():
            Mx = A[solve] + w[solve][:, None, None] * np.eye(3)[None]
            x[solve] = np.linalg.solve(Mx, (w[solve][:, None] * m[solve] - b[solve])[:, :, None])[:, :, 0]
    x = np.clip(x, -h64 / 2, h64 / 2)
    out.update(verts=o + x, colors=cm, centre=o)
    return out


# ---- adjacency, Taubin, normals ---------------------------------------------------------------------------------------------------------
def neighbours(verts, faces):
    """per vertex the ascending array of the distinct other vertices of its valid faces"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(verts, f)]
    nb = [set() for _ in range(len(verts))]
    for a, b, c in f:
        nb[a].update((b, c))
        nb[b].update((a, c))
        nb[c].update((a, b))
    return [np.array(sorted(s), np.int64) for s in nb]


def _half_step(x32, nb, step):
    x = x32.astype(np.float64)
    out = x32.copy()
    for v, n in enumerate(nb):
        if len(n) == 0:
            continue
        s = np.zeros(3)
        for u in n:
            s = s + x[u]
        with np.errstate(all="ignore"):
            out[v] = (x[v] + step * (s / float(len(n)) - x[v])).astype(np.float32)
    return out


def taubin(verts, faces, iters=10, lam=0.5, mu=-0.53):
    """fp32 positions after `iters` iterations of the lambda | mu pair; every half-step rounds to fp32"""
    x = np.asarray(verts, np.float32).reshape(-1, 3).copy()
    nb = neighbours(x, faces)
    for _ in range(iters):
        x = _half_step(_half_step(x, nb, lam), nb, mu)
    return x


def roughness(verts, faces):
    """the umbrella roughness: sum over the vertices of |mean of the neighbours - x|^2"""
    x = np.asarray(verts, np.float64)
    return float(sum(((x[n].mean(0) - x[v]) ** 2).sum() for v, n in enumerate(neighbours(verts, faces)) if len(n)))


def vertex_normals(verts, faces, valid_on=None):
    """[nv,3] float64: per vertex the sum over its valid faces, ascending, of (p1 - p0) x (p2 - p0), normalised; zero where the sum is
    zero or not finite.  valid_on: the positions that decide which faces are valid (default: verts)."""
    p = np.asarray(verts, np.float32).reshape(-1, 3).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    f = f[valid_faces(verts if valid_on is None else valid_on, f)]
    s = np.zeros((len(p), 3))
    with np.errstate(all="ignore"):
        c = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
        good = np.isfinite(c).all(1)
        for k in range(3):                                   # (a face holds a vertex once, so the order over k is immaterial)
            np.add.at(s, f[good, k], c[good])
        ln = np.sqrt(s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1] + s[:, 2] * s[:, 2])
        ok = (ln > 0) & np.isfinite(ln)
        return np.where(ok[:, None], s / np.where(ok, ln, 1.0)[:, None], 0.0)


# ---- meshes ---------------------------------------------------------------------------------------------------------------------------
def icosphere(subdivisions, radius=1.0):
    """closed, outward-wound unit icosahedron subdivided: 10 * 4^s + 2 vertices"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, g = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            g += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = g
    return (np.array(v) * radius).astype(np.float32), np.array(f, np.int32)


def noisy_icosphere(subdivisions, noise=0.02, seed=0, radius=1.0):
    v, f = icosphere(subdivisions, radius)
    r = 1.0 + noise * np.random.RandomState(seed).uniform(-1, 1, len(v))
    return (v.astype(np.float64) * r[:, None]).astype(np.float32), f


def cube(quads, half=0.9):
    """closed, outward-wound surface of the cube [-half, half]^3 with quads x quads quads per side, every quad cut along one
    diagonal; the vertices are shared between the sides"""
    idx, verts, faces = {}, [], []

    def vid(i, j, k):
        if (i, j, k) not in idx:
            idx[(i, j, k)] = len(verts)
            verts.append([(2.0 * c / quads - 1.0) * half for c in (i, j, k)])
        return idx[(i, j, k)]
    for axis in range(3):
        u, w = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, quads):
            for a in range(quads):
                for b in range(quads):
                    def at(da, db):
                        c = [0, 0, 0]
                        c[axis], c[u], c[w] = side, a + da, b + db
                        return vid(*c)
                    q = [at(0, 0), at(1, 0), at(1, 1), at(0, 1)]         # counter-clockwise seen from +axis
                    if side == 0:
                        q = q[::-1]
                    faces += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    return np.array(verts, np.float32), np.array(faces, np.int32)


def cube_surface_distance(p, half=0.9):
    """distance of points to the surface of the cube [-half, half]^3"""
    a = np.abs(np.asarray(p, np.float64))
    outside = np.linalg.norm(np.maximum(a - half, 0.0), axis=1)
    inside = half - a.max(1)
    return np.where((a <= half).all(1), inside, outside)


def plane_grid(n, origin, e1, e2):
    """(n + 1)^2 vertices origin + i e1 + j e2 and 2 n^2 triangles"""
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.asarray(origin, np.float64)[None] + i.reshape(-1, 1) * np.asarray(e1, np.float64)[None] + j.reshape(-1, 1) * np.asarray(e2, np.float64)[None]
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + 1], 1)])
    return v.astype(np.float32), f.astype(np.int32)


def fan(valence, radius=0.8, lift=0.2):
    """a hub (vertex 0) joined to a closed rim of `valence` vertices: one vertex of that valence"""
    a = 2 * np.pi * np.arange(valence) / valence
    rim = np.stack([radius * np.cos(a), radius * np.sin(a), lift * np.sin(3 * a)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.1]], rim]).astype(np.float32)
    k = np.arange(valence)
    f = np.stack([np.zeros(valence, int), 1 + k, 1 + (k + 1) % valence], 1).astype(np.int32)
    return v, f


def colours_of(verts, seed=1):
    return np.random.RandomState(seed).rand(len(verts), 3).astype(np.float32)
