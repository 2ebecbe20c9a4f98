"""Plain numpy / Python-integer restatement of the five definitions of include/instantavatar_hip_overlay.h (DESIGN.md section 4,
"sequence inspection"): the reference tests/test_gpu_overlay.py compares the kernels with, itself checked against literals in
tests/test_cpu_overlay_refs.py.  Integer definitions are computed in int64 where the values fit and in Python integers (numpy object
arrays) where they do not -- the squared cross product of the skeleton -- so nothing is rounded; the face shade is float64."""
import math

import numpy as np


def blend(images, layer, opacity):
    """images [...,3] uint8, layer [...,4] uint8, opacity 0 .. 256 -> uint8 [...,3]"""
    img, lay = np.asarray(images).astype(np.int64), np.asarray(layer).astype(np.int64)
    a = (int(opacity) * lay[..., 3:4] + 127) // 255
    return ((img * (256 - a) + lay[..., :3] * a + 128) >> 8).astype(np.uint8)


def outline_pixels(mask, t):
    """mask [H,W] -> bool [H,W]: mask > 0 and a pixel of the image with mask == 0 within Chebyshev distance t"""
    m = np.asarray(mask)
    H, W = m.shape
    zero = m == 0
    near = np.zeros((H, W), bool)
    for dy in range(-t, t + 1):
        for dx in range(-t, t + 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))        # near[y] |= zero[y + dy]
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            if ys.start < ys.stop and xs.start < xs.stop:
                near[yd, xd] |= zero[ys, xs]
    return (m > 0) & near


def outline(images, masks, t, rgb):
    """images [n,H,W,3], masks [n,H,W] -> a copy of images with the outline pixels set to rgb"""
    out = np.array(images, np.uint8)
    for f in range(out.shape[0]):
        out[f][outline_pixels(masks[f], t)] = np.asarray(rgb, np.uint8)
    return out


def face_shade(face_id, verts, faces, w2c, tint):
    """float64: -> (layer [H,W,4] as float64 before the rounding of the colour bytes, i.e. tint * s and alpha 255; zeros where empty)"""
    fid = np.asarray(face_id)
    v, f, R = np.asarray(verts, np.float64), np.asarray(faces), np.asarray(w2c, np.float64).reshape(4, 4)[:3, :3]
    out = np.zeros(fid.shape + (4,), np.float64)
    for y, x in zip(*np.nonzero((fid >= 0) & (fid < len(f)))):
        idx = f[fid[y, x]]
        if (idx < 0).any() or (idx >= len(v)).any():
            continue
        d1, d2 = R @ (v[idx[1]] - v[idx[0]]), R @ (v[idx[2]] - v[idx[0]])
        c = np.cross(d1, d2)
        n = math.sqrt(float(c @ c))
        s = 0.25 + 0.75 * abs(c[2]) / n if n > 0 and math.isfinite(n) else 0.25
        out[y, x, :3], out[y, x, 3] = np.asarray(tint, np.float64) * s, 255.0
    return out


def face_shade_bytes(face_id, verts, faces, w2c, tint):
    layer = face_shade(face_id, verts, faces, w2c, tint)
    return np.floor(layer + np.array([0.5, 0.5, 0.5, 0.0])).astype(np.uint8)


def quantise(v):
    """floor(4 x + 0.5) of a float32 value, exactly"""
    return int(math.floor(4.0 * float(np.float32(v)) + 0.5))


def point_valid(p, threshold):
    x, y, c = (float(np.float32(v)) for v in p)
    return all(math.isfinite(v) for v in (x, y, c)) and c > float(np.float32(threshold)) and abs(x) <= 32768.0 and abs(y) <= 32768.0


def segment_pixels(H, W, a, b, hw):
    """bool [H,W]: the pixels whose centre (4 px, 4 py) lies in the capsule of half width hw around the quantised ends a, b"""
    X, Y = 4 * np.arange(W, dtype=np.int64)[None, :], 4 * np.arange(H, dtype=np.int64)[:, None]
    (ax, ay), (bx, by) = a, b
    dx, dy = bx - ax, by - ay
    ex, ey, fx, fy = X - ax, Y - ay, X - bx, Y - by
    L2, t = dx * dx + dy * dy, dx * ex + dy * ey
    end_a, end_b = ex * ex + ey * ey <= hw * hw, fx * fx + fy * fy <= hw * hw
    if L2 == 0:
        return np.broadcast_to(end_a, (H, W)).copy()
    c = (dx * ey - dy * ex).astype(object)                       # |c| < 2^38: its square needs Python integers
    mid = np.array(c * c <= hw * hw * L2, bool)
    return np.where(t <= 0, end_a, np.where(t >= L2, end_b, mid))


def skeleton_frame(image, points, segments, segment_rgb, point_rgb, threshold, hw, rad):
    """one frame: image [H,W,3], points [K,3] float32 -> a copy with the skeleton drawn in"""
    out = np.array(image, np.uint8)
    H, W = out.shape[:2]
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    K = len(pts)
    valid = [point_valid(p, threshold) for p in pts]
    q = [(quantise(p[0]), quantise(p[1])) if v else None for p, v in zip(pts, valid)]
    for s, (i, j) in enumerate(np.asarray(segments, np.int64).reshape(-1, 2)):        # ascending: a higher index paints over a lower
        if 0 <= i < K and 0 <= j < K and valid[i] and valid[j]:
            out[segment_pixels(H, W, q[i], q[j], hw)] = np.asarray(segment_rgb, np.uint8).reshape(-1, 3)[s]
    X, Y = 4 * np.arange(W, dtype=np.int64)[None, :], 4 * np.arange(H, dtype=np.int64)[:, None]
    for k in range(K):
        if valid[k]:
            out[(X - q[k][0]) ** 2 + (Y - q[k][1]) ** 2 <= rad * rad] = np.asarray(point_rgb, np.uint8)
    return out


def skeleton(images, points, segments, segment_rgb, point_rgb, threshold, hw, rad):
    return np.stack([skeleton_frame(images[f], points[f], segments, segment_rgb, point_rgb, threshold, hw, rad) for f in range(len(images))])


def stats(a, b):
    """a, b [n,H,W] -> int32 [n,4]: a > 0 & b > 0, a > 0 | b > 0, a > 0, b > 0"""
    A, B = np.asarray(a) != 0, np.asarray(b) != 0
    return np.stack([(A & B).sum((1, 2)), (A | B).sum((1, 2)), A.sum((1, 2)), B.sum((1, 2))], 1).astype(np.int32)
