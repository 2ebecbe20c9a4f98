"""float64 / int64 numpy references of the rasteriser ("rasteriser"; include/instantavatar_hip_raster.h):
the projection, coverage + visibility + interpolation written as the definition reads, and an independent brute force that
intersects the pixel rays with the triangles (Moeller-Trumbore).  Nothing here imports the package."""
import numpy as np

XY_MAX = 1 << 22
SUB = 256


def icosphere(sub):
    """unit icosphere, outward wound: (verts [nv,3] float64, faces [20 * 4^sub,3] int64)"""
    t = (1 + 5 ** .5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, float) / np.linalg.norm(x) for x in v]
    for _ in range(sub):
        cache, nf = {}, []

        def mid(a, b):
            k = (min(a, b), max(a, b))
            if k not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int64)


def sphere_pair():
    """two interpenetrating icosphere(3) meshes: radius 0.5 at the origin, radius 0.4 at (0.35, 0.1, 0.05) -> (verts fp32, faces int32)"""
    v, f = icosphere(3)
    V = np.concatenate([v * 0.5, v * 0.4 + np.array([0.35, 0.1, 0.05])]).astype(np.float32)
    return V, np.concatenate([f, f + len(v)]).astype(np.int32)


def pair_camera(H, W):
    """(w2c [4,4] fp32, fx, fy, cx, cy) of the depth-order tests: t = (0.02, -0.03, 3), f = 120, c = (W/2 - 0.3, H/2 + 0.2), as fp32"""
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, 3] = [0.02, -0.03, 3.0]
    return w2c, float(np.float32(120.0)), float(np.float32(120.0)), float(np.float32(W / 2 - 0.3)), float(np.float32(H / 2 + 0.2))


def project(verts, w2c, fx, fy, cx, cy, near=0.05):
    """-> dict: p [nv,3] camera space, u, v float64 (pixels), xy [nv,2] int64, inv_z [nv] fp32, valid [nv] bool.  float64 from the
    (fp32) inputs; invalid vertices have xy = 0 and inv_z = 0."""
    X, M = np.asarray(verts, np.float64), np.asarray(w2c, np.float64)
    with np.errstate(all="ignore"):
        p = X @ M[:3, :3].T + M[:3, 3]
        u, v = fx * p[:, 0] / p[:, 2] + cx, fy * p[:, 1] / p[:, 2] + cy
        rx, ry = np.rint(u * SUB), np.rint(v * SUB)
        w = (1.0 / p[:, 2]).astype(np.float32)
        valid = (p[:, 2] >= near) & np.isfinite(rx) & np.isfinite(ry) & np.isfinite(w) & (np.abs(rx) <= XY_MAX) & (np.abs(ry) <= XY_MAX) & (w > 0)
    xy = np.zeros((len(X), 2), np.int64)
    xy[valid, 0], xy[valid, 1] = rx[valid].astype(np.int64), ry[valid].astype(np.int64)
    return dict(p=p, u=u, v=v, xy=xy, inv_z=np.where(valid, w, np.float32(0)).astype(np.float32), valid=valid)


def vertex_ok(xy, inv_z):
    """what ia_raster_visibility accepts of hand-made input: a positive finite inv_z and |xy| <= 2^22"""
    w = np.asarray(inv_z, np.float64)
    return (w > 0) & np.isfinite(w) & (np.abs(np.asarray(xy, np.float64)) <= XY_MAX).all(1)


def rasterize(xy, inv_z, faces, H, W, cull=False):
    """Coverage and visibility as defined.  xy [nv,2]: integers in 1/256 pixel (the arithmetic is then exact in int64; Python ints
    where a product could pass 2^63 cannot occur below 2^22) -- or float64 positions in the same unit, for which the same formulas
    are evaluated in float64; inv_z [nv].  ->  dict: face_id [H,W] (-1 empty), iz (best inverse depth, float64, 0 empty), second
    (second-best inverse depth of the pixel, 0 when there is none), cover (fragments per pixel), lam [H,W,3] (the winner's weights
    l_0..l_2), skipped (faces with an invalid vertex, A == 0, or culled)."""
    xy = np.asarray(xy)
    exact = np.issubdtype(xy.dtype, np.integer)
    xy = xy.astype(np.int64) if exact else xy.astype(np.float64)
    w = np.asarray(inv_z, np.float64)
    ok = vertex_ok(xy, w)
    nv = len(xy)
    face_id = np.full((H, W), -1, np.int64)
    best, second = np.zeros((H, W)), np.zeros((H, W))
    cover = np.zeros((H, W), np.int64)
    lam = np.zeros((H, W, 3))
    skipped = 0
    for k, (a, b, c) in enumerate(np.asarray(faces, np.int64)):
        if min(a, b, c) < 0 or max(a, b, c) >= nv or not (ok[a] and ok[b] and ok[c]):
            skipped += 1
            continue
        (x0, y0), (x1, y1), (x2, y2) = xy[a], xy[b], xy[c]
        A = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
        if A == 0 or (cull and A > 0):
            skipped += 1
            continue
        s = 1 if A > 0 else -1
        # the samples of the bounding box, clipped to the screen (a sample outside the box fails an edge)
        bx0, bx1 = max(int(np.ceil(min(x0, x1, x2) / SUB)), 0), min(int(np.floor(max(x0, x1, x2) / SUB)), W - 1)
        by0, by1 = max(int(np.ceil(min(y0, y1, y2) / SUB)), 0), min(int(np.floor(max(y0, y1, y2) / SUB)), H - 1)
        if bx0 > bx1 or by0 > by1:
            continue
        py, px = np.mgrid[by0:by1 + 1, bx0:bx1 + 1]
        Px, Py = px * SUB, py * SUB
        E, cov = [], True
        for (xa, ya), (xb, yb) in (((x1, y1), (x2, y2)), ((x2, y2), (x0, y0)), ((x0, y0), (x1, y1))):
            e = s * ((xb - xa) * (Py - ya) - (yb - ya) * (Px - xa))
            dx, dy = s * (xb - xa), s * (yb - ya)
            top_left = dy < 0 or (dy == 0 and dx > 0)
            cov = cov & ((e > 0) | ((e == 0) & top_left))
            E.append(e)
        if not cov.any():
            continue
        l = np.stack([e.astype(np.float64) / float(abs(A)) for e in E], -1)
        iz = l[..., 0] * w[a] + l[..., 1] * w[b] + l[..., 2] * w[c]
        sl = (slice(by0, by1 + 1), slice(bx0, bx1 + 1))
        cover[sl] += cov
        better = cov & (iz > best[sl])           # strict: an exact tie stays with the smaller face index
        second[sl] = np.where(better, best[sl], np.where(cov & (iz > second[sl]), iz, second[sl]))
        best[sl] = np.where(better, iz, best[sl])
        face_id[sl] = np.where(better, k, face_id[sl])
        lam[sl] = np.where(better[..., None], l, lam[sl])
    return dict(face_id=face_id, iz=best, second=second, cover=cover, lam=lam, skipped=skipped)


def interpolate(ref, faces, inv_z, attrs):
    """perspective-correct attributes of a `rasterize` result: (out [H,W,C] = sum(l_i w_i a_i) / iz, 0 on empty pixels;
    scale [H,W,C] = sum |l_i w_i a_i| / iz, what a rounding-count bound multiplies)"""
    faces, w, attrs = np.asarray(faces, np.int64), np.asarray(inv_z, np.float64), np.asarray(attrs, np.float64)
    hit = ref["face_id"] >= 0
    if len(faces) == 0:
        z = np.zeros(hit.shape + (attrs.shape[1],))
        return z, z
    tri = faces[np.where(hit, ref["face_id"], 0)]                          # [H,W,3]
    t = ref["lam"] * w[tri]                                                # l_i w_i
    terms = t[..., None] * attrs[tri]                                      # [H,W,3,C]
    iz = np.where(hit, ref["iz"], 1.0)[..., None]
    return np.where(hit[..., None], terms.sum(2) / iz, 0.0), np.where(hit[..., None], np.abs(terms).sum(2) / iz, 0.0)


def depth_of(ref):
    with np.errstate(divide="ignore"):
        return np.where(ref["face_id"] >= 0, 1.0 / ref["iz"], 0.0)


def unproject(xy, inv_z, fx, fy, cx, cy):
    """camera-space vertices whose exact projection is (xy / 256, inv_z): what the rasteriser sees after snapping"""
    z = 1.0 / np.asarray(inv_z, np.float64)
    u, v = np.asarray(xy, np.float64)[:, 0] / SUB, np.asarray(xy, np.float64)[:, 1] / SUB
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)


def ray_cast(p_cam, faces, fx, fy, cx, cy, H, W, cull=False):
    """Brute force: the ray K^-1 [x, y, 1] of every pixel against every triangle of the CAMERA-space vertices p_cam
    (Moeller-Trumbore, float64).  -> (face_id [H,W] of the nearest hit (-1: none), depth [H,W] = its z, 0 for none).  The ray has
    d.z = 1, so the ray parameter IS the depth.  cull: only faces whose outward normal points at the camera."""
    y, x = np.mgrid[0:H, 0:W]
    d = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones((H, W))], -1).reshape(-1, 3)
    face_id, depth = np.full(H * W, -1, np.int64), np.full(H * W, np.inf)
    for k, (a, b, c) in enumerate(np.asarray(faces, np.int64)):
        v0, e1, e2 = p_cam[a], p_cam[b] - p_cam[a], p_cam[c] - p_cam[a]
        n = np.cross(e1, e2)
        if cull and np.dot(n, v0) >= 0:         # the origin is not on the outer side
            continue
        h = np.cross(d, e2)
        det = h @ e1
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / det
            bu = (h @ (-v0)) * inv
            q = np.cross(-v0, e1)
            bv = (d @ q) * inv
            t = (e2 @ q) * inv
        hit = (det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0) & (t < depth)
        face_id[hit], depth[hit] = k, t[hit]
    return face_id.reshape(H, W), np.where(face_id >= 0, depth, 0.0).reshape(H, W)


def edge_distance(u, v, faces, valid, H, W):
    """[H,W]: the distance in pixels from every pixel's sample to the nearest projected edge (segments between the float64
    screen positions u, v) of the faces whose vertices are all valid"""
    out = np.full((H, W), np.inf)
    P = np.stack([u, v], 1)
    for a, b, c in np.asarray(faces, np.int64):
        if not (valid[a] and valid[b] and valid[c]):
            continue
        tri = P[[a, b, c]]
        x0, x1 = max(int(np.floor(tri[:, 0].min())) - 1, 0), min(int(np.ceil(tri[:, 0].max())) + 1, W - 1)
        y0, y1 = max(int(np.floor(tri[:, 1].min())) - 1, 0), min(int(np.ceil(tri[:, 1].max())) + 1, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        Q = np.stack([xx, yy], -1).astype(np.float64)
        for i in range(3):
            A, B = tri[i], tri[(i + 1) % 3]
            ab = B - A
            tt = np.clip(((Q - A) @ ab) / max(ab @ ab, 1e-300), 0, 1)
            dist = np.linalg.norm(Q - (A + tt[..., None] * ab), axis=-1)
            out[y0:y1 + 1, x0:x1 + 1] = np.minimum(out[y0:y1 + 1, x0:x1 + 1], dist)
    return out


# ---- hand-made integer cases: coverage is exact, so the device must reproduce face_id bit for bit ----------------------------
def _px(*pts):
    return [(int(round(x * SUB)), int(round(y * SUB))) for x, y in pts]


def hand_cases():
    """name -> dict(xy int64 [nv,2], inv_z fp32 [nv], faces int32 [nf,3], H, W): every case at both image sizes is the caller's
    choice; the shapes fit 37 x 29"""
    C = {}

    def add(name, pts, faces, inv_z=None, raw=False):
        xy = np.array(pts if raw else _px(*pts), np.int64).reshape(-1, 2)
        w = np.full(len(xy), 0.5, np.float32) if inv_z is None else np.asarray(inv_z, np.float32)
        C[name] = dict(xy=xy, inv_z=w, faces=np.array(faces, np.int32).reshape(-1, 3))
    # vertices on pixel centres: the right-angle triangle (2,2) (10,2) (2,8), both windings
    add("on_centres", [(2, 2), (10, 2), (2, 8)], [(0, 1, 2)])
    add("on_centres_flipped", [(2, 2), (10, 2), (2, 8)], [(0, 2, 1)])
    # an edge through sample points: the diagonal (3,3)-(11,11) passes through (4,4) .. (10,10)
    add("edge_through_samples", [(3, 3), (11, 11), (3, 11)], [(0, 1, 2)])
    add("edge_through_samples_other_side", [(3, 3), (11, 3), (11, 11)], [(0, 1, 2)])
    # two triangles sharing the diagonal of a quad: every sample of the quad exactly once
    add("quad", [(4, 3), (20, 3), (20, 17), (4, 17)], [(0, 1, 2), (0, 2, 3)])
    add("quad_mixed_winding", [(4, 3), (20, 3), (20, 17), (4, 17)], [(0, 1, 2), (0, 3, 2)])
    add("quad_subpixel", [(4.25, 3.5), (20.75, 2.125), (22.5, 17.875), (3.0625, 16.5)], [(0, 1, 2), (0, 2, 3)])
    # a sliver between two sample columns: covers no sample
    add("sliver", [(5.25, 1), (5.75, 1), (5.5, 20)], [(0, 1, 2)])
    # one triangle that covers the whole screen and far beyond: the queue path, one wave on one face
    add("screen_filling", [(-3000, -2500), (9000, -2000), (-2000, 9000)], [(0, 1, 2)], inv_z=[0.2, 0.5, 0.8])
    add("off_screen", [(-30, -20), (-10, -20), (-20, -5)], [(0, 1, 2)])
    add("off_screen_right", [(100, 5), (130, 5), (110, 40)], [(0, 1, 2)])
    add("degenerate", [(2, 2), (6, 6), (10, 10), (2, 2)], [(0, 1, 2), (0, 3, 1)])
    # an invalid vertex (inv_z = 0, as ia_raster_project marks it), one past 2^22, and an index outside [0, nv)
    add("invalid_vertex", [(2, 2), (20, 3), (4, 18), (9, 25)], [(0, 1, 2), (0, 1, 3), (1, 2, 7)], inv_z=[0.5, 0.5, 0.0, 0.25])
    add("beyond_range", [(2 * SUB, 2 * SUB), (XY_MAX + 1, 3 * SUB), (4 * SUB, 18 * SUB), (20 * SUB, 20 * SUB)], [(0, 1, 2), (0, 3, 2)], raw=True)
    # a duplicated face row: the exact tie goes to the smaller index; and a nearer face in front of both
    add("duplicate", [(3, 2), (30, 5), (8, 26)], [(0, 1, 2), (0, 1, 2)], inv_z=[0.3, 0.6, 0.45])
    add("duplicate_behind", [(3, 2), (30, 5), (8, 26), (10, 8), (20, 9), (12, 18)], [(0, 1, 2), (3, 4, 5), (0, 1, 2)],
        inv_z=[0.3, 0.6, 0.45, 1.0, 1.0, 1.0])
    # front and back faces over each other: with cull the back face (nearer) disappears
    add("front_and_back", [(3, 2), (30, 5), (8, 26), (5, 4), (28, 20), (25, 3), (5, 4), (28, 20), (25, 3)], [(0, 2, 1), (3, 4, 5), (6, 8, 7)],
        inv_z=[0.25, 0.25, 0.25, 0.5, 0.5, 0.5, 0.75, 0.75, 0.75])
    # many small faces next to large ones: both paths write the same pixels (a fan of 1-pixel triangles under a large one)
    pts, faces = [(1, 1), (35, 2), (3, 27)], [(0, 1, 2)]
    w = [0.25, 0.25, 0.25]
    for j in range(6):
        for i in range(8):
            n = len(pts)
            pts += [(2.25 + 3 * i, 2.5 + 3 * j), (4.75 + 3 * i, 2.75 + 3 * j), (3.5 + 3 * i, 4.875 + 3 * j)]
            faces.append((n, n + 1, n + 2) if (i + j) % 2 else (n, n + 2, n + 1))
            w += [0.135 + 0.03 * ((i * 5 + j * 3) % 9)] * 3       # never within 2 % of the large face's 0.25
    add("small_over_large", pts, faces, inv_z=w)
    add("no_faces", [(2, 2), (10, 2), (2, 8)], np.zeros((0, 3), np.int32))
    return C
