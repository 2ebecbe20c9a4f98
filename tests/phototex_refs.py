"""Float64 numpy restatement of the photo texture ("photo texture"): per texel and frame the decision, the margin
of every test and the colour; then the weighted mean over the frames with the fallback atlas.  Written from the definition, not from
csrc/ia_phototex.hip; the atlas layout comes from tests/texture_refs.py.  Validated on hand-checkable cases in
tests/test_cpu_phototex_refs.py.

Margins are RELATIVE: the distance of a test from its threshold over the natural size of the quantities compared, positive = passes.
A texel-frame pair is DECIDED when no margin is smaller than `EPS` in absolute value, or when some test fails by more than that;
the other pairs may be flipped by a rounding difference of another evaluation order and are left out of comparisons."""
import numpy as np

import texture_refs as tx

EPS = 1e-9


def texel_weights(nf, B):
    """(owner [n] by layout, u [n,3] float64: the weights u0, u1, u2 of every texel, gutter texels included) in row-major order"""
    owner, h, i, j = (a.reshape(-1) for a in tx.texel_owner(nf, B))
    li, lj = np.where(h == 1, B - 1 - i, i), np.where(h == 1, B - 1 - j, j)
    L = float(B - 3)
    u1, u2 = li / L, lj / L
    return owner, np.stack([1.0 - u1 - u2, u1, u2], 1)


def project_frame(verts, faces, B, w2c, intr, image, mask, depth, cos_min=0.3, power=2.0, depth_tol=0.02):
    """One frame.  verts [nv,3] (posed), w2c [4,4], intr = (fx, fy, cx, cy, near), image [H,W,3] uint8, mask [H,W] or None, depth
    [H,W].  -> dict of per-texel arrays [n]: ok (bool), decided (bool), margins (dict name -> [n], +inf where a test is not
    evaluated), uv [n,2], z [n], cos [n], weight [n], colour [n,3]"""
    verts = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    w2c = np.asarray(w2c, np.float32).astype(np.float64).reshape(4, 4)
    fx, fy, cx, cy, near = (float(np.float32(x)) for x in intr)
    cos_min, power, depth_tol = (float(np.float32(x)) for x in (cos_min, power, depth_tol))      # the C ABI takes them as fp32
    image = np.asarray(image)
    assert image.dtype == np.uint8
    H, W = image.shape[:2]
    depth = np.asarray(depth, np.float32).astype(np.float64)
    mask = None if mask is None else np.asarray(mask, np.float32).astype(np.float64)
    nv, nf = len(verts), len(faces)
    owner, wts = texel_weights(nf, B)
    n = len(owner)
    R, t = w2c[:3, :3], w2c[:3, 3]
    ok = np.zeros(n, bool)
    decided = np.ones(n, bool)
    names = ("near", "left", "right", "top", "bottom", "pixel", "facing", "mask", "depth")
    margins = {k: np.full(n, np.inf) for k in names}
    uv, z, cs = np.zeros((n, 2)), np.zeros(n), np.zeros(n)
    weight, colour = np.zeros(n), np.zeros((n, 3))
    for g in range(n):
        f = owner[g]
        if f < 0:
            continue
        idx = faces[f]
        if (idx < 0).any() or (idx >= nv).any() or not np.isfinite(verts[idx]).all():
            continue
        a, b, c = verts[idx]
        with np.errstate(all="ignore"):
            m = np.cross(b - a, c - a)
            ln = np.sqrt((m * m).sum())
        if not (ln > 0 and np.isfinite(ln)):
            continue
        nrm = m / ln
        p = wts[g, 0] * a + wts[g, 1] * b + wts[g, 2] * c
        x = R @ p + t
        z[g] = x[2]
        mg = {"near": (x[2] - near) / max(abs(x[2]), near)}
        passed = x[2] >= near
        if passed:
            u, v = fx * x[0] / x[2] + cx, fy * x[1] / x[2] + cy
            uv[g] = u, v
            mg.update(left=u / W, right=(W - 1 - u) / W, top=v / H, bottom=(H - 1 - v) / H)
            inside = 0 <= u < W - 1 and 0 <= v < H - 1
            cosine = -float((R @ nrm) @ x) / np.sqrt(float(x @ x))
            cs[g] = cosine
            mg["facing"] = cosine - cos_min
            passed = inside and cosine > cos_min
            if inside:
                i0, j0 = int(np.floor(u)), int(np.floor(v))
                fu, fv = u - i0, v - j0
                mg["pixel"] = min(fu, 1 - fu, fv, 1 - fv)         # a flip moves the footprint to other pixels
                px = [(j0, i0), (j0, i0 + 1), (j0 + 1, i0), (j0 + 1, i0 + 1)]
                if mask is not None:
                    mg["mask"] = min(mask[q] - 0.5 for q in px)
                    passed = passed and all(mask[q] >= 0.5 for q in px)
                covered = all(depth[q] > 0 for q in px)
                if covered:
                    mg["depth"] = min((depth_tol - abs(x[2] - depth[q])) / max(abs(x[2]), depth[q], depth_tol) for q in px)
                    passed = passed and all(abs(x[2] - depth[q]) <= depth_tol for q in px)
                else:
                    mg["depth"] = -1.0                            # depth == 0 is exact: no rounding can cover the pixel
                    passed = False
                if passed:
                    c00, c10, c01, c11 = (image[q].astype(np.float64) for q in px)
                    colour[g] = ((1 - fu) * (1 - fv) * c00 + fu * (1 - fv) * c10 + (1 - fu) * fv * c01 + fu * fv * c11) / 255.0
                    weight[g] = cosine ** power
        for k, val in mg.items():
            margins[k][g] = val
        vals = np.array(list(mg.values()))
        decided[g] = bool((vals <= -EPS).any() or not (np.abs(vals) < EPS).any())
        ok[g] = passed
    return dict(ok=ok, decided=decided, margins=margins, uv=uv, z=z, cos=cs, weight=weight, colour=colour)


def bake(canonical_verts, faces, B, frames, base=None, cos_min=0.3, power=2.0, depth_tol=0.02, min_frames=1):
    """frames: a list of (posed verts [nv,3], w2c [4,4], intr, image, mask or None, depth).  -> dict(atlas [T,T,3] float64, seen [T,T],
    owner [T,T] (of the canonical mesh), unseen (owned texels no frame saw), ok [F,n], decided [F,n], per_frame (the project_frame
    dicts), size)"""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    T = tx.atlas_size(len(faces), B)
    n = T * T
    owner = tx.texel_points(canonical_verts, faces, B)["owner"]
    S, Wt, seen = np.zeros((n, 3)), np.zeros(n), np.zeros(n, np.int64)
    per_frame = []
    for posed, w2c, intr, image, mask, depth in frames:
        r = project_frame(posed, faces, B, w2c, intr, image, mask, depth, cos_min, power, depth_tol)
        per_frame.append(r)
        S += np.where(r["ok"][:, None], r["weight"][:, None] * r["colour"], 0.0)
        Wt += np.where(r["ok"], r["weight"], 0.0)
        seen += r["ok"]
    base = np.zeros((n, 3)) if base is None else np.asarray(base, np.float64).reshape(n, 3)
    with np.errstate(all="ignore"):
        mean = S / Wt[:, None]
    atlas = np.where((seen >= min_frames)[:, None], mean, base)
    atlas = np.where((owner >= 0)[:, None], atlas, 0.0)
    F = len(per_frame)
    return dict(atlas=atlas.reshape(T, T, 3), seen=seen.reshape(T, T), owner=owner.reshape(T, T),
                unseen=int(((owner >= 0) & (seen == 0)).sum()), ok=np.stack([r["ok"] for r in per_frame]) if F else np.zeros((0, n), bool),
                decided=np.stack([r["decided"] for r in per_frame]) if F else np.zeros((0, n), bool), per_frame=per_frame, size=T)


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """w2c [4,4] float32 of an OpenCV camera (x right, y down, z forward) at `eye` looking at `target` with the world direction `up`
    pointing up in the image (from (0, 0, -d) at the origin: R = diag(-1, -1, 1), the camera of `raster.look_at_box`)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    zc = target - eye
    zc /= np.linalg.norm(zc)
    down = -np.asarray(up, np.float64)
    xc = np.cross(down, zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    R = np.stack([xc, yc, zc])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ eye
    return w2c.astype(np.float32)


def icosahedron(r=0.5):
    """12 vertices on the sphere of radius r, 20 faces, outward winding"""
    g = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
                  (-g, 0, -1), (-g, 0, 1)], np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int32)
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * r
    return v.astype(np.float32), f


KERNEL_CASES = [(nf, B, F) for nf in (1, 2, 3, 20) for B in (4, 5, 8) for F in (1, 3)]
KERNEL_H, KERNEL_W = 20, 28                     # not square: an H / W swap shows
KERNEL_OPTIONS = dict(cos_min=0.3, power=2.0, depth_tol=0.1)    # (a pixel of these small images spans 0.05 m of the body)


def kernel_case(nf, B, F, seed=None):
    """The scene of the kernel-against-reference tests: the first `nf` faces of an icosahedron, `F` frames with jittered vertices and
    cameras around the direction of vertex 0 (which the faces 0 .. 2 share), random image bytes, masks with holes and the z-buffer
    depth of each posed body (all 20 faces, so that the edges of the first `nf` are no silhouettes: with B = 4 or 5 a face has no
    texel off its edges) with a few pixels moved and a few emptied.  The shared intrinsics put part of the mesh outside the
    image; with F > 1 the last camera stands closer and `near` lies just behind its nearest vertex (the faces at that vertex are
    then missing from its depth map), in front of every vertex of the other frames.  -> dict(verts [nv,3] (canonical), faces, frames: the
    list `bake` takes, plus the stacked arrays posed [F,nv,3], w2c [F,4,4], images, masks, depth and intr)"""
    seed = 800000 + 1000 * nf + 10 * B + F if seed is None else seed     # (chosen so that every scene has an accepted pair)
    rs = np.random.RandomState(seed)
    verts, body = icosahedron(0.5)
    faces = body[:nf].copy()
    H, W = KERNEL_H, KERNEL_W
    axis = verts[0].astype(np.float64) / np.linalg.norm(verts[0])
    posed = (verts[None].astype(np.float64) + 0.02 * rs.randn(F, len(verts), 3)).astype(np.float32)
    eyes = axis + 0.2 * rs.randn(F, 3)
    dist = np.full(F, 2.2)
    if F > 1:
        dist[-1] = 1.9                                            # the last camera stands closer: `near` cuts its nearest vertex only
        eyes[-1] = verts[faces[0]].astype(np.float64).mean(0) / 0.4 + 0.1 * rs.randn(3)      # ... and looks at face 0
    w2c = np.stack([look_at(d * e / np.linalg.norm(e), 0.05 * rs.randn(3)) for d, e in zip(dist, eyes)])
    zs = np.einsum("fij,fnj->fni", w2c[:, :3, :3].astype(np.float64), posed.astype(np.float64)) + w2c[:, None, :3, 3]
    near = float(np.float32(zs[-1, :, 2].min() + 0.03)) if F > 1 else 0.5
    intr = (40.0, 38.0, 8.25, 9.5, near)                         # the principal point left of the centre: the mesh leaves the image
    images = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    masks = np.ones((F, H, W), np.float32)
    depth = np.zeros((F, H, W), np.float32)
    for f in range(F):
        depth[f] = raster_depth(posed[f], body, w2c[f], intr, H, W)
        for _ in range(12):
            masks[f, rs.randint(H), rs.randint(W)] = rs.choice([0.0, 0.25, 0.75])
        covered = np.argwhere(depth[f] > 0)
        if len(covered):
            for j, i in covered[rs.choice(len(covered), 1 + len(covered) // 40, replace=False)]:
                depth[f, j, i] += rs.choice([-0.3, 0.3])
            for j, i in covered[rs.choice(len(covered), 1 + len(covered) // 50, replace=False)]:
                depth[f, j, i] = 0.0
    frames = [(posed[f], w2c[f], intr, images[f], masks[f], depth[f]) for f in range(F)]
    return dict(verts=verts, faces=faces, frames=frames, posed=posed, w2c=w2c, images=images, masks=masks, depth=depth, intr=intr)


def raster_depth(verts, faces, w2c, intr, H, W):
    """a plain float64 z-buffer of the mesh sampled AT the integer pixels (camera z, 0 = empty): the depth map the tests hand to both
    sides when the rasteriser itself is not under test.  Faces with a vertex behind `near` are skipped, as the rasteriser skips them."""
    verts = np.asarray(verts, np.float32).astype(np.float64)
    w2c = np.asarray(w2c, np.float32).astype(np.float64)
    fx, fy, cx, cy, near = (float(np.float32(x)) for x in intr)
    x = verts @ w2c[:3, :3].T + w2c[:3, 3]
    out = np.zeros((H, W))
    for a, b, c in np.asarray(faces, np.int64):
        if min(x[a, 2], x[b, 2], x[c, 2]) < near:
            continue
        P = np.array([[fx * x[k, 0] / x[k, 2] + cx, fy * x[k, 1] / x[k, 2] + cy] for k in (a, b, c)])
        area = (P[1, 0] - P[0, 0]) * (P[2, 1] - P[0, 1]) - (P[2, 0] - P[0, 0]) * (P[1, 1] - P[0, 1])
        if area == 0:
            continue
        lo, hi = np.floor(P.min(0)).astype(int), np.ceil(P.max(0)).astype(int)
        for j in range(max(lo[1], 0), min(hi[1], H - 1) + 1):
            for i in range(max(lo[0], 0), min(hi[0], W - 1) + 1):
                l0 = ((P[1, 0] - i) * (P[2, 1] - j) - (P[2, 0] - i) * (P[1, 1] - j)) / area
                l1 = ((P[2, 0] - i) * (P[0, 1] - j) - (P[0, 0] - i) * (P[2, 1] - j)) / area
                l2 = 1 - l0 - l1
                if min(l0, l1, l2) < 0:
                    continue
                iz = l0 / x[a, 2] + l1 / x[b, 2] + l2 / x[c, 2]
                d = 1 / iz
                if out[j, i] == 0 or d < out[j, i]:
                    out[j, i] = d
    return out.astype(np.float32)
