"""float64 numpy restatement of the scene-composition entry points, written from the text of include/instantavatar_hip_scene.h
("scene composition"): `ground`, `shadow`, `composite`.  Inputs are taken as the fp32 values the kernels get
and converted to float64; nothing is rounded to fp32 on the way except where the header rounds a value that a DECISION or a later
stage depends on (fp32(t) in the hit test, the fp32 lerp weights are NOT rounded: that is part of the error the tests bound).

Next to its outputs every function returns a `report` of the margins of its discrete choices, which is what lets a GPU test assert
that no choice can flip between fp32 and fp64:
  composite  key_gap     the smallest relative gap |z_i - z_j| / max(|z_i|, |z_j|) between two DISTINCT keys of one pixel (inf: none)
  ground     cell_margin the smallest distance, in cells, of a checker coordinate of a hit pixel from a cell border (inf: no checker)
  shadow     border_margin the smallest distance, in pixels, of the projected centre tap of a contributing pixel from the map's border
"""
import numpy as np

MAX_LAYERS = 8


def plane_axes(n):
    """the two in-plane unit axes the header derives from the normal: the coordinate axis least aligned with n (lowest index among
    equals), Gram-Schmidt, cross product"""
    n = np.asarray(n, np.float32).astype(np.float64)
    ax = int(np.argmin(np.abs(n)))                       # argmin takes the first among equals
    e = np.zeros(3)
    e[ax] = 1.0
    s = e - n[ax] * n
    e1 = s / np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    e2 = np.array([n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]])
    return e1, e2


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def ground(rays_o, rays_d, normal, h, g0, g1, cell, centre, r0, r1):
    """-> dict(t_g [R], a_g [R], c_g [R,3], P [R,3], hit [R] bool, cell_margins [R] (inf where no hit or no checker), report)"""
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    o, d, n, centre = f64(rays_o).reshape(-1, 3), f64(rays_d).reshape(-1, 3), f64(normal), f64(centre)
    h, cell, r0, r1 = (float(np.float32(v)) for v in (h, cell, r0, r1))
    g0, g1 = f64(g0), f64(g1)
    R = o.shape[0]
    with np.errstate(all="ignore"):
        no, nd = _dot(n[None], o), _dot(n[None], d)
        t = (h - no) / nd
        tf = t.astype(np.float32)
        hit = (no > h) & (nd < 0) & np.isfinite(tf) & (tf > 0)
        p = o + t[:, None] * d
        q = p - centre[None]
        rho = np.sqrt(_dot(q, q))
        a = np.where(rho <= r0, 1.0, np.where(rho >= r1, 0.0, (r1 - rho) / (r1 - r0) if r1 > r0 else 0.0))
        odd = np.zeros(R, bool)
        margin, margins = np.inf, np.full(R, np.inf)
        if cell > 0:
            e1, e2 = plane_axes(normal)
            uc, vc = _dot(q, e1[None]) / cell, _dot(q, e2[None]) / cell
            fu, fv = np.floor(uc), np.floor(vc)
            fu = np.where(np.abs(fu) < 2.0 ** 62, fu, 0.0)
            fv = np.where(np.abs(fv) < 2.0 ** 62, fv, 0.0)
            odd = ((fu.astype(np.int64) + fv.astype(np.int64)) & 1) != 0
            both = np.stack([uc, vc])
            margins = np.where(hit, np.min(np.minimum(both - np.floor(both), np.ceil(both) - both), axis=0), np.inf)
            margin = float(margins.min()) if R else np.inf
    colour = np.where(odd[:, None], g1[None], g0[None])
    z = lambda x: np.where(hit.reshape((-1,) + (1,) * (x.ndim - 1)), x, 0.0)
    return dict(t_g=z(t), a_g=z(a), c_g=z(colour), P=z(p), hit=hit, cell_margins=margins, report=dict(cell_margin=margin))


def shadow(P, a_g, maps, proj, radius, strength, near):
    """-> dict(shade [R], abar [K,R], inside [K,R] bool (the layer contributes), uv [K,R,2], report)"""
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    P, a_g, maps, proj = f64(P).reshape(-1, 3), f64(a_g).reshape(-1), f64(maps), f64(proj)
    K, S = maps.shape[0], maps.shape[1]
    assert maps.shape == (K, S, S) and proj.shape == (K, 3, 4)
    strength, near, r = float(np.float32(strength)), float(np.float32(near)), int(radius)
    R = P.shape[0]
    lit = a_g != 0
    shade = np.ones(R)
    abar = np.zeros((K, R))
    inside = np.zeros((K, R), bool)
    uv = np.zeros((K, R, 2))
    margin = np.inf
    hi = float(S - 1)
    for k in range(K):
        M = proj[k]
        with np.errstate(all="ignore"):
            x = [((M[i, 0] * P[:, 0] + M[i, 1] * P[:, 1]) + M[i, 2] * P[:, 2]) + M[i, 3] for i in range(3)]
            z = x[2]
            u, v = x[0] / z, x[1] / z
            ok = lit & (z > near) & (u >= 0) & (u <= hi) & (v >= 0) & (v <= hi)
        inside[k], uv[k, :, 0], uv[k, :, 1] = ok, u, v
        if ok.any():
            uu, vv = u[ok], v[ok]
            margin = min(margin, float(np.min(np.minimum(np.minimum(uu, hi - uu), np.minimum(vv, hi - vv)))))
            total = np.zeros(uu.shape[0])
            for dy in range(-r, r + 1):
                y = np.minimum(np.maximum(vv + dy, 0.0), hi)
                j0 = np.floor(y).astype(np.int64)
                j1 = np.minimum(j0 + 1, S - 1)
                fy = y - j0
                for dx in range(-r, r + 1):
                    xx = np.minimum(np.maximum(uu + dx, 0.0), hi)
                    i0 = np.floor(xx).astype(np.int64)
                    i1 = np.minimum(i0 + 1, S - 1)
                    fx = xx - i0
                    m = maps[k]
                    top = m[j0, i0] + fx * (m[j0, i1] - m[j0, i0])
                    bot = m[j1, i0] + fx * (m[j1, i1] - m[j1, i0])
                    total += top + fy * (bot - top)
            abar[k, ok] = total / float((2 * r + 1) ** 2)
        shade = shade * (1.0 - strength * abar[k])
    shade = np.where(lit, shade, 1.0)
    return dict(shade=shade, abar=abar, inside=inside, uv=uv, report=dict(border_margin=margin))


def composite(c, a, d, ground=None, background=None, contact=0.3):
    """c [K,R,3], a [K,R], d [K,R]; ground: None or (t_g [R], a_g [R], c_g [R,3], shade [R]); background: None, [R,3] or [3]
    -> dict(rgb [R,3], alpha [R], depth [R], contested int, contested_mask [R], order (per pixel the indices composited),
    transmittance [R] (T behind the last contributor), report)"""
    f64 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    c, a, d = f64(c), f64(a), f64(d)
    K, R = a.shape
    if not 1 <= K <= MAX_LAYERS:
        raise ValueError("K = %d outside [1, %d]" % (K, MAX_LAYERS))
    assert c.shape == (K, R, 3) and d.shape == (K, R)
    contact = float(np.float32(contact))
    with np.errstate(all="ignore"):
        ok = (a > 0) & np.isfinite(a) & np.isfinite(d) & np.isfinite(c).all(-1)
        z = np.where(ok, d / np.where(ok, a, 1.0), np.inf)
    if ground is not None:
        t_g, a_g, c_g, sh = (f64(x) for x in ground)
        t_g, a_g, sh, c_g = t_g.reshape(R), a_g.reshape(R), sh.reshape(R), c_g.reshape(R, 3)
        with np.errstate(all="ignore"):
            okg = (a_g > 0) & np.isfinite(a_g) & np.isfinite(t_g) & np.isfinite(sh) & np.isfinite(c_g).all(-1)
    bg = None
    if background is not None:
        bg = f64(background)
        bg = np.broadcast_to(bg.reshape(1, 3), (R, 3)) if bg.size == 3 else bg.reshape(R, 3)
    rgb, alpha, depth, trans = np.zeros((R, 3)), np.zeros(R), np.zeros(R), np.zeros(R)
    mask = np.zeros(R, bool)
    order = []
    gap = np.inf
    for r in range(R):
        items = [(z[k, r], k, c[k, r], a[k, r], d[k, r]) for k in range(K) if ok[k, r]]
        for i in range(len(items)):
            for j in range(i + 1, len(items)):
                zi, zj = items[i][0], items[j][0]
                with np.errstate(all="ignore"):
                    if items[i][3] >= 0.5 and items[j][3] >= 0.5 and abs(zi - zj) < contact:
                        mask[r] = True
        if ground is not None and okg[r]:
            items.append((t_g[r], K, (c_g[r] * sh[r]) * a_g[r], a_g[r], a_g[r] * t_g[r]))
        items.sort(key=lambda it: (it[0], it[1]))
        keys = [it[0] for it in items]
        for i in range(len(keys)):
            for j in range(i + 1, len(keys)):
                if keys[i] != keys[j] and np.isfinite(keys[i]) and np.isfinite(keys[j]):
                    gap = min(gap, abs(keys[i] - keys[j]) / max(abs(keys[i]), abs(keys[j])))
        C, D, T = np.zeros(3), 0.0, 1.0
        for key, _, col, op, term in items:
            C = C + T * col
            D = D + T * term
            T = T * (1.0 - op)
        order.append([it[1] for it in items])
        if bg is not None:
            rgb[r], alpha[r] = C + T * bg[r], 1.0
        else:
            rgb[r], alpha[r] = C, 1.0 - T
        depth[r], trans[r] = D, T
    return dict(rgb=rgb, alpha=alpha, depth=depth, contested=int(mask.sum()), contested_mask=mask, order=order, transmittance=trans,
                report=dict(key_gap=gap))
