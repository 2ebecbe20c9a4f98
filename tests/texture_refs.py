"""Float64 / integer numpy restatement of the texture atlas ("texture atlas"): the block layout, the surface
point of a texel, the snap onto the level set, bilinear sampling, and a whole bake built from them.  Written from the definition,
not from csrc/ia_texture.hip; validated on hand-checkable cases in tests/test_cpu_texture_refs.py."""
import numpy as np

MIN_BLOCK, MAX_BLOCK, MAX_SIZE = 4, 64, 16384


def blocks_per_row(nf):
    nq = (int(nf) + 1) // 2
    nb = 1
    while nb * nb < nq:
        nb += 1
    return nb


def atlas_size(nf, B):
    """T, or 0 outside the limits"""
    if nf < 0 or not MIN_BLOCK <= B <= MAX_BLOCK:
        return 0
    T = blocks_per_row(nf) * B
    return T if T <= MAX_SIZE else 0


def corner_local(B, h):
    """[3,2] integer texels (x, y), local to the block, of the corners v0, v1, v2 of the face in half h"""
    L = B - 3
    c = np.array([[0, 0], [L, 0], [0, L]], np.int64)
    return B - 1 - c if h else c


def corner_uv(nf, B):
    """[nf,3,2] float64 continuous texel coordinates of the corners"""
    nb = blocks_per_row(nf)
    uv = np.zeros((nf, 3, 2), np.float64)
    for f in range(nf):
        q, h = f >> 1, f & 1
        uv[f] = corner_local(B, h) + np.array([(q % nb) * B, (q // nb) * B]) + 0.5
    return uv


def texel_owner(nf, B):
    """(owner [T,T] int64 by layout alone: the face index or -1, half [T,T], local i [T,T], local j [T,T]); array index [y, x]"""
    T = atlas_size(nf, B)
    nb = T // B
    y, x = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    i, j = x % B, y % B
    h = np.where(i + j <= B - 2, 0, 1)
    f = 2 * ((y // B) * nb + x // B) + h
    return np.where(f < nf, f, -1), h, i, j


def texel_points(verts, faces, B, t=None):
    """-> dict(pts [T*T,3] float64, normal [T*T,3] float64, owner [T*T] int64) in row-major texel order; t [T*T] float64 or None"""
    verts = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    nv, nf = len(verts), len(faces)
    owner, h, i, j = (a.reshape(-1) for a in texel_owner(nf, B))
    n_tex = len(owner)
    pts, nrm, own = np.zeros((n_tex, 3)), np.zeros((n_tex, 3)), owner.copy()
    tt = np.zeros(n_tex) if t is None else np.asarray(t, np.float64)
    L = B - 3
    for g in range(n_tex):
        f = owner[g]
        if f < 0:
            continue
        idx = faces[f]
        if (idx < 0).any() or (idx >= nv).any() or not np.isfinite(verts[idx]).all():
            own[g] = -1
            continue
        a, b, c = verts[idx]
        li, lj = (B - 1 - i[g], B - 1 - j[g]) if h[g] else (i[g], j[g])
        u1, u2 = li / L, lj / L
        u0 = 1.0 - u1 - u2
        with np.errstate(all="ignore"):
            m = np.cross(b - a, c - a)
            ln = np.sqrt((m * m).sum())
        n = m / ln if ln > 0 and np.isfinite(ln) else np.zeros(3)
        pts[g] = u0 * a + u1 * b + u2 * c + tt[g] * n
        nrm[g] = n
    return dict(pts=pts, normal=nrm, owner=own)


def snap_offsets(K, dist):
    """t_k [K] float32, formed as the kernel forms them"""
    h = np.float32(np.float32(2) * np.float32(dist)) / np.float32(K - 1)
    return ((np.arange(K) - (K - 1) // 2).astype(np.float32) * h).astype(np.float32), h


def snap(sigma, level, dist, owner=None):
    """sigma [K,n] -> (t [n] float32, unsnapped int): the crossing nearest to 0 along the normal, in fp32 in the stated order"""
    sigma = np.asarray(sigma, np.float32)
    K, n = sigma.shape
    assert K % 2 == 1 and 3 <= K <= 17
    t = np.zeros(n, np.float32)
    if not dist > 0:
        return t, 0
    tk, h = snap_offsets(K, dist)
    s = (sigma - np.float32(level)).astype(np.float32)
    miss = 0
    for i in range(n):
        if owner is not None and owner[i] < 0:
            continue
        best = None
        for k in range(K - 1):
            a, b = s[k, i], s[k + 1, i]
            if np.isfinite(a) and np.isfinite(b) and ((a >= 0) != (b >= 0)):
                r = np.float32(tk[k] + np.float32(h * np.float32(a / np.float32(a - b))))
                if best is None or abs(r) < abs(best):
                    best = r
        if best is None:
            miss += 1
        else:
            t[i] = best
    return t, miss


def sample(atlas, uv, mask=None):
    """atlas [T,T,C], uv [R,2] continuous texel coordinates -> [R,C] float64.  Clamp to the edge, two lerps in x, one in y."""
    atlas = np.asarray(atlas, np.float64)
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    T = atlas.shape[0]
    out = np.zeros((len(uv), atlas.shape[2]))
    for r, (u, v) in enumerate(uv):
        if (mask is not None and mask[r] == 0) or not (np.isfinite(u) and np.isfinite(v)):
            continue
        x, y = min(max(u - 0.5, 0.0), T - 1.0), min(max(v - 0.5, 0.0), T - 1.0)
        i0, j0 = int(np.floor(x)), int(np.floor(y))
        i1, j1 = min(i0 + 1, T - 1), min(j0 + 1, T - 1)
        fx, fy = x - i0, y - j0
        top = atlas[j0, i0] + fx * (atlas[j0, i1] - atlas[j0, i0])
        bot = atlas[j1, i0] + fx * (atlas[j1, i1] - atlas[j1, i0])
        out[r] = top + fy * (bot - top)
    return out


def bilinear_footprint(T, u, v):
    """the texels (x, y) that `sample` reads with a non-zero weight at the continuous coordinates (u, v)"""
    x, y = min(max(u - 0.5, 0.0), T - 1.0), min(max(v - 0.5, 0.0), T - 1.0)
    i0, j0 = int(np.floor(x)), int(np.floor(y))
    fx, fy = x - i0, y - j0
    xs = [(i0, 1 - fx), (min(i0 + 1, T - 1), fx)]
    ys = [(j0, 1 - fy), (min(j0 + 1, T - 1), fy)]
    return {(i, j) for i, wx in xs for j, wy in ys if wx * wy != 0}


def bake(verts, faces, field, B, dist, level, K=9):
    """the whole bake: field(points [n,3] float64) -> (rgb [n,3], sigma [n]).  -> dict(atlas [T,T,3], owner [T,T], pts [T*T,3] (the
    snapped points), t, unsnapped)"""
    T = atlas_size(len(faces), B)
    base = texel_points(verts, faces, B)
    t, miss = np.zeros(T * T, np.float32), 0
    if dist > 0:
        tk, _ = snap_offsets(K, dist)
        sig = np.stack([field(base["pts"] + np.float64(tk[k]) * base["normal"])[1] for k in range(K)])
        t, miss = snap(sig, level, dist, base["owner"])
    pts = texel_points(verts, faces, B, t)["pts"]
    rgb = field(pts)[0] * (base["owner"] >= 0)[:, None]
    return dict(atlas=rgb.reshape(T, T, 3), owner=base["owner"].reshape(T, T), pts=pts, t=t, unsnapped=miss, size=T)


# ---- meshes -------------------------------------------------------------------------------------------------------------------------
def octasphere(levels, r=0.5):
    """an octahedron subdivided `levels` times with every vertex on the sphere of radius r, outward winding: 8 * 4^levels faces"""
    v = [np.array(p, np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, g = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            g += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = g
    return (np.array(v) * r).astype(np.float32), np.array(f, np.int32)


def max_sag(verts, faces, r):
    """the largest distance between a face's plane and the sphere of radius r over the face: r - min over faces of the plane's
    distance to the centre (the vertices lie on the sphere)"""
    v = np.asarray(verts, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    return float(r - np.abs((n * a).sum(1)).min())
