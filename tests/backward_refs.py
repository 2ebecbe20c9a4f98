"""float64 restatements of the training-render backward kernels, their seeded input sets, and the error bounds the GPU
tests apply (numpy only: no GPU, no product import).

Every reference takes the arrays the C entry takes (include/instantavatar_hip.h) and returns float64 results.  Sums come
with a condition magnitude M (the same expression with every summed term replaced by its absolute value) and the number of
terms per element; the tests assert |got - ref| <= K u M with u = 2^-24 and K = terms + fp32 roundings on the path of one
term (the worst-case bound of a sum in ANY order: atomics and scan order need no allowance).  The library is built with
-ffp-contract=off, so a rounding is one per spelled operation.

The compositor is a recurrence, not a flat sum: its yardstick is the reference expression evaluated in plain fp32 on the
host in two association orders (sequential and doubling scan), per ray and per output, times a margin, plus a floor of a
few u of the ray's largest magnitude (`composite_bounds`).  tests/test_cpu_backward_refs.py checks the margin's
association-order part on the same inputs, and that plain fp32 attains the K u M bounds of the other kernels.
"""
import numpy as np

U = 2.0 ** -24           # unit roundoff of fp32
U16 = 2.0 ** -11         # unit roundoff of fp16
TINY = 2.0 ** -126       # smallest normal fp32: absolute allowance where a product underflows (T after a saturated alpha)
INVALID = np.float32(-1e5)


# ---------------------------------------------------------------------------------------------------------------------
# candidate selection (snarf_deformer.py:147-158)
# ---------------------------------------------------------------------------------------------------------------------
def candidate_argmax_ref(cand_sigma, cand_cap, pt_off, pt_cnt, n_init):
    """Winning candidate per point and its sigma (fp32 values: comparisons only, exact in any precision).  The list of a
    point is cut at cand_cap; a list shorter than n_init also holds the invalid fill -1e5, which wins ties and gives -1."""
    P = len(pt_off)
    arg, sg = np.full(P, -1, np.int32), np.full(P, INVALID, np.float32)
    for p in range(P):
        po = int(pt_off[p])
        pc = max(0, min(int(pt_cnt[p]), int(cand_cap) - po))
        vals = np.asarray(cand_sigma[po:po + pc], np.float32)
        if pc < n_init:
            vals = np.concatenate([[INVALID], vals])        # (first: np.argmax takes the first of equal maxima)
            j = int(np.argmax(vals)) - 1
        else:
            j = int(np.argmax(vals))
        if j >= 0:
            arg[p], sg[p] = po + j, vals[j + (1 if pc < n_init else 0)]
    return arg, sg


def candidate_gather_ref(cand_rgb, cand_sigma, arg, fill):
    ok = arg >= 0
    a = np.where(ok, arg, 0)
    rgb = np.where(ok[:, None], np.asarray(cand_rgb, np.float32)[a], np.float32(0))
    sigma = np.where(ok, np.asarray(cand_sigma, np.float32)[a], np.float32(fill))
    return rgb.astype(np.float32), sigma.astype(np.float32)


def candidate_gather_bwd_ref(d_rgb, d_sigma, arg, n_cand):
    """unique scatter into zero arrays; a NULL upstream leaves its array zero"""
    d_cand_rgb, d_cand_sigma = np.zeros((n_cand, 3), np.float32), np.zeros(n_cand, np.float32)
    ok = arg >= 0
    if d_rgb is not None:
        d_cand_rgb[arg[ok]] = d_rgb[ok]
    if d_sigma is not None:
        d_cand_sigma[arg[ok]] = d_sigma[ok]
    return d_cand_rgb, d_cand_sigma


# ---------------------------------------------------------------------------------------------------------------------
# compositor (raymarcher_acc.py:25-36, 161-186)
# ---------------------------------------------------------------------------------------------------------------------
def _excl_cumprod(m, order):
    """T_k = prod_{j<k} m_j and the full product, in the dtype of m; order: 'seq' | 'tree' (doubling scan)"""
    n = len(m)
    if order == "seq":
        incl = np.cumprod(m, dtype=m.dtype)
    else:
        incl, o = m.copy(), 1
        while o < n:
            incl[o:] = incl[:-o] * incl[o:]
            o *= 2
    one = np.ones(1, m.dtype)
    return np.concatenate([one, incl[:-1]]) if n else one[:0], (incl[-1] if n else one[0])


def _rev_affine(mm, bb, g_end, order):
    """gT_k = b_k + m_k gT_{k+1}, gT_n = g_end; returns gT_0..gT_n"""
    n = len(mm)
    out = np.empty(n + 1, mm.dtype)
    out[n] = g_end
    if order == "seq":
        for k in range(n - 1, -1, -1):
            out[k] = bb[k] + mm[k] * out[k + 1]
    else:
        SM, SB, o = mm.copy(), bb.copy(), 1          # suffix compositions S_k = F_k o F_{k+1} o ...
        while o < n:
            SB[:-o] = SB[:-o] + SM[:-o] * SB[o:]
            SM[:-o] = SM[:-o] * SM[o:]
            o *= 2
        out[:n] = SB + SM * mm.dtype.type(g_end)
    return out


COMPOSITE_OUTPUTS = ("color", "depth", "alpha", "weights_dense", "s_sigma", "s_alpha", "s_T", "d_cand_rgb", "d_cand_sigma")


def composite_train_ref(cand_rgb, cand_sigma, cand_cap, pt_off, pt_cnt, n_init, ray_off, ray_cnt, s_z, nears, fars, n_rays,
                        max_samples, noise, noise_scale, bg, s_slot, d_color=None, d_depth=None, d_alpha=None,
                        d_weights=None, dtype=np.float64, order="seq"):
    """Forward and analytic backward of the training compositor.  dtype=np.float64 is the reference (with "mag": the
    ray's largest magnitude per output); dtype=np.float32 evaluates the same expressions op by op in fp32, in sequential
    (order="seq") or doubling-scan (order="tree") association: the yardstick of `composite_bounds`."""
    ft = np.dtype(dtype).type
    n_s = len(pt_off)
    n_c = len(cand_sigma)
    cand_rgb = np.asarray(cand_rgb, np.float32)
    arg, sg0 = candidate_argmax_ref(cand_sigma, cand_cap, pt_off, pt_cnt, n_init)
    R = dict(s_arg=arg, color=np.zeros((n_rays, 3), dtype), depth=np.zeros(n_rays, dtype), alpha=np.zeros(n_rays, dtype),
             weights_dense=np.zeros((n_rays, max_samples), dtype), s_sigma=np.zeros(n_s, dtype), s_alpha=np.zeros(n_s, dtype),
             s_T=np.zeros(n_s, dtype), d_cand_rgb=np.zeros((n_c, 3), dtype), d_cand_sigma=np.zeros(n_c, dtype))
    M = R["mag"] = {k: np.zeros(n_rays) for k in COMPOSITE_OUTPUTS}
    one = ft(1)
    for n in range(n_rays):
        off, cnt = int(ray_off[n]), int(ray_cnt[n])
        sl = slice(off, off + cnt)
        slot = np.asarray(s_slot[sl], np.int64)
        dt = (ft(fars[n]) - ft(nears[n])) / ft(max_samples)
        sg = sg0[sl].astype(dtype)
        nz = np.zeros(cnt, dtype)
        if noise is not None:
            nz = ft(noise_scale) * noise[n, slot].astype(dtype)
            sg = sg + nz
        tau = np.maximum(sg, ft(0)) * dt
        e = np.exp(-tau)
        a = one - e
        m = (one - a) + ft(np.float32(1e-10))
        T, T_end = _excl_cumprod(m, order)
        w = a * T
        ok = arg[sl] >= 0
        rgb = np.where(ok[:, None], cand_rgb[np.where(ok, arg[sl], 0)], np.float32(0)).astype(dtype)
        z = np.asarray(s_z[sl]).astype(dtype)
        b = np.ones(3, dtype) if bg is None else np.asarray(bg[n]).astype(dtype)
        if dtype == np.float32:          # plain fp32 accumulation in sample order
            c, dep, asum = np.zeros(3, dtype), ft(0), ft(0)
            for k in range(cnt):
                c = c + w[k] * rgb[k]
                dep = dep + w[k] * z[k]
                asum = asum + w[k]
        else:
            c, dep, asum = (w[:, None] * rgb).sum(0), (w * z).sum(), w.sum()
        R["color"][n], R["depth"][n], R["alpha"][n] = c + T_end * b, dep, asum
        R["weights_dense"][n, slot] = w
        R["s_sigma"][sl], R["s_alpha"][sl], R["s_T"][sl] = sg, a, T
        # ---- backward ----
        dc = np.zeros(3, dtype) if d_color is None else np.asarray(d_color[n]).astype(dtype)
        dd = ft(0) if d_depth is None else ft(d_depth[n])
        da = ft(0) if d_alpha is None else ft(d_alpha[n])
        dw = np.zeros(cnt, dtype) if d_weights is None else d_weights[n, slot].astype(dtype)
        gw = dc[0] * rgb[:, 0] + dc[1] * rgb[:, 1] + dc[2] * rgb[:, 2] + dd * z + da + dw
        gT_end = dc[0] * b[0] + dc[1] * b[1] + dc[2] * b[2]
        gT = _rev_affine(m, gw * a, gT_end, order)           # gT_k = gw_k a_k + gT_{k+1} (1 - a_k + 1e-10)
        g_alpha = gw * T - gT[1:] * T
        d_sig = np.where(sg > 0, g_alpha * e * dt, ft(0))    # d alpha / d sigma = exp(-tau) dt, relu: 0 at sigma <= 0
        d_rgb = w[:, None] * dc[None, :]
        wa = arg[sl][ok]
        R["d_cand_sigma"][wa], R["d_cand_rgb"][wa] = d_sig[ok], d_rgb[ok]
        if dtype != np.float64:
            continue
        # ---- the ray's largest magnitude per output: what the floor of the bound is measured in (`composite_bounds`).  alpha is
        # formed as 1 - exp(-tau), at magnitude 1 whatever its value, so everything that carries it as a factor is measured with
        # that factor at 1; a sample with sigma <= 0 has alpha = 0 exactly and contributes no magnitude ----
        live = sg > 0
        Tl = np.where(live, T, 0.0)
        top = lambda v: float(np.max(v)) if np.size(v) else 0.0
        gwabs = np.abs(dc[0] * rgb[:, 0]) + np.abs(dc[1] * rgb[:, 1]) + np.abs(dc[2] * rgb[:, 2]) + np.abs(dd * z) + abs(da) + np.abs(dw)
        GA = np.zeros(cnt + 1)                                # gT with every term replaced by its absolute value
        GA[cnt] = np.abs(dc * b).sum()
        for k in range(cnt - 1, -1, -1):
            GA[k] = gwabs[k] * a[k] + GA[k + 1] * m[k]
        M["s_sigma"][n] = top(np.abs(sg0[sl].astype(dtype)) + np.abs(nz))
        M["s_alpha"][n] = 1.0 if live.any() else 0.0
        M["s_T"][n] = 1.0 if cnt else 0.0                      # T_0 = 1
        M["weights_dense"][n] = M["alpha"][n] = top(Tl)
        M["color"][n] = max(top(Tl[:, None] * np.abs(rgb)), top(T_end * np.abs(b)))
        M["depth"][n] = top(Tl * np.abs(z))
        M["d_cand_rgb"][n] = top(Tl) * top(np.abs(dc))
        M["d_cand_sigma"][n] = top(np.where(live, (gwabs + GA[1:]) * T * abs(dt), 0.0))
    return R


# The compositor's outputs are recurrences (T, w, the backward's gT): no closed-form K.  The yardstick is the reference
# expression evaluated in plain fp32 on the host, per ray and per output array: the kernel's worst error in a ray may be
# MARGIN times the worst error of the sequential and the doubling-scan fp32 evaluations in that ray, plus a floor of FLOOR u
# times the ray's largest magnitude of that output.
#   MARGIN = 4 = 2 x 2.  One factor 2 for the association order: the wave scan is neither of the two host orders; on every
#   input set the two host orders stay within a factor 2 (plus the floor) of each other per ray and output, asserted in
#   tests/test_cpu_backward_refs.py.  One factor 2 for expf: the HIP math API documents the device expf at 1 ulp, the host's
#   is within 0.5 ulp on these arguments, and the error of alpha = 1 - exp(-tau) at magnitude 1 is dominated by it.
#   FLOOR = 8: the roundings that do not depend on the ray's length and that a short ray's fp32 evaluation may happen not
#   to show: dt (2), tau (1), expf (2 u), 1 - e (1), w = alpha T (1), the product with the colour / the gradient (1).
#   TINY: a product that underflows (T after a saturated alpha) may be flushed on the device.
# Where fp32 evaluation is exact in both orders and the magnitude is 0 the bound is 0: the output must equal the reference.
COMPOSITE_MARGIN, COMPOSITE_ASSOC, COMPOSITE_FLOOR = 4.0, 2.0, 8.0


def composite_ray_of(inp, R):
    """the ray every element of an output belongs to (-1: a candidate that is no sample's winner)"""
    n, ms = inp["n_rays"], inp["max_samples"]
    ray_s = np.repeat(np.arange(n), inp["ray_cnt"])
    ray_c = np.full(len(inp["cand_sigma"]), -1, np.int64)
    ok = R["s_arg"] >= 0
    ray_c[R["s_arg"][ok]] = ray_s[ok]
    rows = np.arange(n)
    return dict(color=np.repeat(rows, 3).reshape(n, 3), depth=rows, alpha=rows, weights_dense=np.repeat(rows, ms).reshape(n, ms),
                s_sigma=ray_s, s_alpha=ray_s, s_T=ray_s, d_cand_rgb=np.repeat(ray_c, 3).reshape(-1, 3), d_cand_sigma=ray_c)


def composite_ray_error(got, R, ray_of, n_rays):
    """worst |got - ref| per ray, per output: {output: [n_rays]}"""
    out = {}
    for k in COMPOSITE_OUTPUTS:
        err, r = np.abs(np.asarray(got[k], np.float64) - R[k]).ravel(), ray_of[k].ravel()
        e = np.zeros(n_rays)
        np.maximum.at(e, r[r >= 0], err[r >= 0])
        assert (err[r < 0] == 0).all(), (k, "a candidate that won no sample differs from the reference's zero")
        out[k] = e
    return out


def composite_bounds(inp):
    """(float64 reference, {output: bound per ray [n_rays]}, the two fp32 evaluations' errors per ray)"""
    args = composite_ref_args(inp)
    R = composite_train_ref(**args)
    ray_of = composite_ray_of(inp, R)
    n = inp["n_rays"]
    e_seq = composite_ray_error(composite_train_ref(**args, dtype=np.float32, order="seq"), R, ray_of, n)
    e_tree = composite_ray_error(composite_train_ref(**args, dtype=np.float32, order="tree"), R, ray_of, n)
    B = {}
    for k in COMPOSITE_OUTPUTS:
        e32 = np.maximum(e_seq[k], e_tree[k])
        B[k] = COMPOSITE_MARGIN * e32 + COMPOSITE_FLOOR * U * R["mag"][k] + TINY * ((e32 > 0) | (R["mag"][k] > 0))
    return R, B, ray_of, e_seq, e_tree


# ---------------------------------------------------------------------------------------------------------------------
# hash grid (tcnn kernel_grid_backward / kernel_grid_backward_input)
# ---------------------------------------------------------------------------------------------------------------------
class Levels:
    """The level descriptor of ia_hash_desc_init as plain arrays: scale fp32 [L], res [L], offset [L + 1].  A level is
    hashed when its entry count is below res^3 (tcnn grid_index; the library derives the flag by the same rule)."""

    def __init__(self, scale, res, offset):
        self.scale = np.asarray(scale, np.float32)
        self.res = np.asarray(res, np.int64)
        self.offset = np.asarray(offset, np.int64)
        self.n_levels = len(self.scale)
        self.size = self.offset[1:] - self.offset[:-1]
        self.hashed = self.res ** 3 > self.size
        self.n_entries = int(self.offset[-1])


def normalise32(x, center, fscale):
    """(raw, xn) as the kernels form them in fp32: raw = (x - c) / s + 0.5, xn = clamp(raw, 0, 1)"""
    x, c, s = np.asarray(x, np.float32), np.asarray(center, np.float32), np.asarray(fscale, np.float32)
    raw = ((x - c) / s + np.float32(0.5)).astype(np.float32)
    return raw, np.clip(raw, np.float32(0), np.float32(1))


def level_pos32(xn, scale_l):
    """fmaf(xn, scale_l, 0.5) in fp32: the float64 product of two fp32 numbers is exact, and on the 2^-12 lattice so is
    the float64 sum with 0.5 (45 bits at most), so one rounding to fp32 is the fused multiply-add"""
    return (np.asarray(xn, np.float64) * np.float64(scale_l) + 0.5).astype(np.float32)


def level_corners(xn, lv, l):
    """entry index (within the whole table) of the 8 corners [8, V] and the fractional position w [V, 3] (float64, exact)"""
    pos = level_pos32(xn, lv.scale[l])
    fl = np.floor(pos)
    w = pos.astype(np.float64) - fl.astype(np.float64)
    g = fl.astype(np.int64).astype(np.uint32)
    size, res = np.uint32(lv.size[l]), np.uint32(lv.res[l])
    idx = np.empty((8, len(pos)), np.int64)
    for c in range(8):
        cx, cy, cz = g[:, 0] + np.uint32(c & 1), g[:, 1] + np.uint32((c >> 1) & 1), g[:, 2] + np.uint32((c >> 2) & 1)
        if lv.hashed[l]:
            i = (cx ^ (cy * np.uint32(2654435761)) ^ (cz * np.uint32(805459861))) & (size - np.uint32(1))
        else:
            i = cx + cy * res + cz * res * res
            i = np.where(i >= size, i - size, i)
            i = np.minimum(i, size - np.uint32(1))
        idx[c] = i.astype(np.int64) + lv.offset[l]
    return idx, w


def _corner_weights(w, c, ft=np.float64):
    w = w.astype(ft)
    one = ft(1)
    wx = w[:, 0] if c & 1 else one - w[:, 0]
    wy = w[:, 1] if c & 2 else one - w[:, 1]
    wz = w[:, 2] if c & 4 else one - w[:, 2]
    return wx, wy, wz


def hashgrid_fwd_ref(x, center, fscale, lv, table):
    """float64 trilinear interpolation of the fp16 table [n_entries, 2] -> feat [V, 2L] and its magnitude sum |w t|"""
    _, xn = normalise32(x, center, fscale)
    t = np.asarray(table).astype(np.float64)
    feat, mag = np.zeros((len(xn), 2 * lv.n_levels)), np.zeros((len(xn), 2 * lv.n_levels))
    for l in range(lv.n_levels):
        idx, w = level_corners(xn, lv, l)
        for c in range(8):
            wx, wy, wz = _corner_weights(w, c)
            wt = (wx * wy * wz)[:, None]
            feat[:, 2 * l:2 * l + 2] += wt * t[idx[c]]
            mag[:, 2 * l:2 * l + 2] += wt * np.abs(t[idx[c]])
    return feat, mag


def hashgrid_bwd_ref(x, n_live, center, fscale, lv, dfeat, table=None, levels=None, dtype=np.float64):
    """dtable [n_entries, 2] = sum over live rows and corners of w_corner dfeat, with sum |term| and the number of terms
    per entry; with `table` (fp16 [n_entries, 2]) also dx [V, 3] = sum_levels scale_l sum_corners dw/dpos <t, dfeat> / fscale
    (0 where the raw coordinate is outside (0, 1)), its sum |term|; rows >= n_live contribute nothing and get dx = 0 here
    (the kernel leaves them untouched).  dtype=np.float32 forms every TERM in fp32 op by op (sums stay in float64)."""
    ft = np.dtype(dtype).type
    V = len(x)
    n_live = V if n_live is None else min(V, int(n_live))
    raw, xn = normalise32(x[:n_live], center, fscale)
    df = np.asarray(dfeat[:n_live]).astype(dtype)
    l0, l1 = (0, lv.n_levels) if levels is None else levels
    ne = lv.n_entries
    dt_, mt_, ct_ = np.zeros((ne, 2)), np.zeros((ne, 2)), np.zeros(ne, np.int64)
    gx, mx = np.zeros((n_live, 3)), np.zeros((n_live, 3))
    tab = None if table is None else np.asarray(table).astype(dtype)
    for l in range(l0, l1):
        idx, w = level_corners(xn, lv, l)
        d0, d1 = df[:, 2 * l], df[:, 2 * l + 1]
        sc = ft(lv.scale[l])
        for c in range(8):
            wx, wy, wz = _corner_weights(w, c, ft)
            wt = wx * wy * wz
            o0, o1 = int(lv.offset[l]), int(lv.offset[l + 1])      # (a level's corners stay inside the level's slice)
            loc = idx[c] - o0
            for f, d in ((0, d0), (1, d1)):
                v = (wt * d).astype(np.float64)
                dt_[o0:o1, f] += np.bincount(loc, weights=v, minlength=o1 - o0)
                mt_[o0:o1, f] += np.bincount(loc, weights=np.abs(v), minlength=o1 - o0)
            ct_[o0:o1] += np.bincount(loc, minlength=o1 - o0)
            if tab is not None:
                t0, t1 = tab[idx[c], 0], tab[idx[c], 1]
                dot = t0 * d0 + t1 * d1
                adot = (np.abs(t0 * d0) + np.abs(t1 * d1)).astype(np.float64)
                sx, sy, sz = (ft(1) if c & 1 else ft(-1)), (ft(1) if c & 2 else ft(-1)), (ft(1) if c & 4 else ft(-1))
                for ax, coef in ((0, sc * sx * wy * wz), (1, sc * wx * sy * wz), (2, sc * wx * wy * sz)):
                    gx[:, ax] += (coef * dot).astype(np.float64)
                    mx[:, ax] += np.abs(coef).astype(np.float64) * adot
    out = dict(dtable=dt_, m_table=mt_, n_table=ct_)
    if tab is not None:
        inside = (raw > 0) & (raw < 1)
        fs = np.asarray(fscale, np.float32).astype(np.float64)[None, :]
        dx, m_dx = np.zeros((V, 3)), np.zeros((V, 3))
        dx[:n_live], m_dx[:n_live] = np.where(inside, gx / fs, 0.0), np.where(inside, mx / np.abs(fs), 0.0)
        out.update(dx=dx, m_dx=m_dx)
    return out


def near_cell_face(x, center, fscale, lv, ulps=2):
    """rows whose fp32 `pos` lies within `ulps` ulp of an integer at some level and axis, or whose raw coordinate lies
    within `ulps` ulp of 0 or 1: where one rounding in the normalisation may move the point to the neighbouring cell"""
    raw, xn = normalise32(x, center, fscale)
    tol = ulps * np.spacing(np.float32(1))
    bad = (np.abs(raw) <= tol).any(1) | (np.abs(raw - 1) <= tol).any(1)
    free = (raw > -tol) & (raw < 1 + tol)      # (a coordinate clamped to exactly 0 or 1 has no rounding to differ by)
    for l in range(lv.n_levels):
        pos = (xn.astype(np.float64) * np.float64(lv.scale[l]) + 0.5)
        d = np.abs(pos - np.round(pos))
        bad |= (free & (d <= ulps * np.spacing(pos.astype(np.float32)).astype(np.float64))).any(1)
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# fit-stage scatters
# ---------------------------------------------------------------------------------------------------------------------
def smpl_nn_compact_bwd_ref(pts, cand_pt, idx, n_cand, cap, T_inv, d_cand_xc):
    """d_T_inv [V, 4, 4] (rows 0..2: += g [x, 1]^T at the vertex of the candidate's point), d_pts [P, 3] = R(T_inv[idx])^T g
    for the points with a candidate; magnitudes and the number of candidates per vertex"""
    P, V = len(pts), len(T_inv)
    n = min(int(cap), int(n_cand))
    i = np.asarray(cand_pt[:n], np.int64)
    v = np.asarray(idx, np.int64)[i]
    g = np.asarray(d_cand_xc[:n], np.float64)
    xh = np.concatenate([np.asarray(pts, np.float64)[i], np.ones((n, 1))], 1)
    terms = g[:, :, None] * xh[:, None, :]                         # [n, 3, 4]
    d_T, m_T = np.zeros((V, 4, 4)), np.zeros((V, 4, 4))
    for r in range(3):
        for c in range(4):
            d_T[:, r, c] = np.bincount(v, weights=terms[:, r, c], minlength=V)
            m_T[:, r, c] = np.bincount(v, weights=np.abs(terms[:, r, c]), minlength=V)
    Rm = np.asarray(T_inv, np.float64)[v][:, :3, :3]               # [n, r, b]
    d_pts, m_pts = np.zeros((P, 3)), np.zeros((P, 3))
    d_pts[i] = (Rm * g[:, :, None]).sum(1)
    m_pts[i] = np.abs(Rm * g[:, :, None]).sum(1)
    return dict(d_T_inv=d_T, m_T_inv=m_T, n_T_inv=np.bincount(v, minlength=V), d_pts=d_pts, m_pts=m_pts)


def ray_samples_bwd_ref(ray_off, ray_cnt, s_z, d_pts):
    n = len(ray_off)
    d_o, d_d, m_o, m_d = (np.zeros((n, 3)) for _ in range(4))
    g, z = np.asarray(d_pts, np.float64), np.asarray(s_z, np.float64)
    for r in range(n):
        sl = slice(int(ray_off[r]), int(ray_off[r]) + int(ray_cnt[r]))
        d_o[r], m_o[r] = g[sl].sum(0), np.abs(g[sl]).sum(0)
        d_d[r], m_d[r] = (z[sl, None] * g[sl]).sum(0), np.abs(z[sl, None] * g[sl]).sum(0)
    return dict(d_o=d_o, d_d=d_d, m_o=m_o, m_d=m_d)


# ---------------------------------------------------------------------------------------------------------------------
# seeded input sets, shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
RAY_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256)
MAX_SAMPLES = 256
# (name, n_init, noise, bg, upstream gradients present)
COMPOSITE_CASES = (
    ("all_n9_noise_bg", 9, True, True, ("color", "depth", "alpha", "weights")),
    ("all_n1_plain_white", 1, False, False, ("color", "depth", "alpha", "weights")),
    ("color_only", 9, True, False, ("color",)),
    ("depth_only", 9, False, True, ("depth",)),
    ("alpha_only", 1, True, True, ("alpha",)),
    ("weights_only", 9, True, True, ("weights",)),
)


def composite_inputs(n_init, with_noise, with_bg, grads, seed=0):
    """One mixed batch: the ray lengths where the per-lane split changes plus random ones (n_rays % 4 == 3), sigmas of both
    signs with exact zeros and early saturation, short / empty / losing candidate lists, lists cut by cand_cap."""
    rng = np.random.RandomState(1000 + seed)
    cnts = np.array(list(RAY_COUNTS) + list(rng.randint(0, MAX_SAMPLES + 1, 32)), np.int32)
    order = rng.permutation(len(cnts))
    cnts = cnts[order]
    n = len(cnts)
    assert n % 4 != 0
    off = np.concatenate([[0], np.cumsum(cnts)[:-1]]).astype(np.int32)
    S = int(cnts.sum())
    near = rng.uniform(0.5, 1.5, n).astype(np.float32)
    far = (near + np.float32(2)).astype(np.float32)
    slot = np.concatenate([np.sort(rng.choice(MAX_SAMPLES, c, replace=False)) for c in cnts] + [np.zeros(0, np.int64)]).astype(np.int32)
    ray_of = np.repeat(np.arange(n), cnts)
    dt = (far - near) / np.float32(MAX_SAMPLES)
    s_z = (near[ray_of] + (slot + rng.rand(S).astype(np.float32)) * dt[ray_of]).astype(np.float32)
    # candidate lists, allocated in a random sample order so that the cut by cand_cap falls on samples all over the batch
    hi = 9 if n_init > 1 else 2
    pt_cnt = rng.randint(0, hi + 1, S).astype(np.uint8)
    pt_cnt[rng.rand(S) < 0.1] = 0
    alloc = rng.permutation(S)
    pt_off = np.zeros(S, np.int32)
    pt_off[alloc] = np.concatenate([[0], np.cumsum(pt_cnt[alloc].astype(np.int64))[:-1]]).astype(np.int32)
    n_total = int(pt_cnt.sum())
    # the last lists are dropped by the capacity, and the first of them only partly
    cand_cap = next(int(pt_off[s]) + 1 for s in alloc if pt_cnt[s] >= 2 and pt_off[s] >= n_total - 60)
    ray_scale = np.array([0.05, 0.3, 1.0, 3.0])[rng.randint(0, 4, n)]
    cand_sigma = np.zeros(n_total, np.float32)
    for s in range(S):
        c = int(pt_cnt[s])
        cand_sigma[pt_off[s]:pt_off[s] + c] = (rng.randn(c) * 40 * ray_scale[ray_of[s]]).astype(np.float32)
    kind = rng.rand(S)
    for s in range(S):
        c, po = int(pt_cnt[s]), int(pt_off[s])
        if c == 0:
            continue
        if kind[s] < 0.06:      # every candidate below the invalid fill: the fill wins a short list, candidate 0.. a full one
            cand_sigma[po:po + c] = -2e5 - 16.0 * rng.permutation(c)
        elif kind[s] < 0.12:    # the winner is exactly zero
            cand_sigma[po:po + c] = -np.abs(cand_sigma[po:po + c]) - 1
            cand_sigma[po + rng.randint(c)] = 0.0
    for r in range(n):           # alpha rounds to 1 in fp32 (tau > 17.4) within the first samples of every third ray
        if r % 3 == 0 and cnts[r] > 0:
            for k in rng.choice(min(4, cnts[r]), min(2, cnts[r]), replace=False):
                s = off[r] + k
                if pt_cnt[s] > 0 and pt_off[s] < cand_cap:
                    cand_sigma[pt_off[s]] = 5000.0 + 100 * k
    cand_rgb = rng.rand(n_total, 3).astype(np.float32)
    noise = None
    if with_noise:
        noise = rng.randn(n, MAX_SAMPLES).astype(np.float32)
        for s in np.nonzero((kind >= 0.06) & (kind < 0.12))[0]:     # keeps the exact zeros exact
            noise[ray_of[s], slot[s]] = 0.0
    g = dict(color=rng.randn(n, 3).astype(np.float32), depth=rng.randn(n).astype(np.float32),
             alpha=rng.randn(n).astype(np.float32), weights=rng.randn(n, MAX_SAMPLES).astype(np.float32))
    return dict(cand_rgb=cand_rgb[:cand_cap].copy(), cand_sigma=cand_sigma[:cand_cap].copy(), cand_cap=cand_cap, pt_off=pt_off,
                pt_cnt=pt_cnt, n_init=n_init, ray_off=off, ray_cnt=cnts, s_z=s_z, nears=near, fars=far, n_rays=n,
                max_samples=MAX_SAMPLES, noise=noise, noise_scale=0.7, bg=rng.rand(n, 3).astype(np.float32) if with_bg else None,
                s_slot=slot, d_color=g["color"] if "color" in grads else None, d_depth=g["depth"] if "depth" in grads else None,
                d_alpha=g["alpha"] if "alpha" in grads else None, d_weights=g["weights"] if "weights" in grads else None)


def composite_ref_args(inp):
    return {k: inp[k] for k in ("cand_rgb", "cand_sigma", "cand_cap", "pt_off", "pt_cnt", "n_init", "ray_off", "ray_cnt", "s_z",
                                "nears", "fars", "n_rays", "max_samples", "noise", "noise_scale", "bg", "s_slot", "d_color",
                                "d_depth", "d_alpha", "d_weights")}


def candidate_inputs(n_init, seed=0):
    """point lists for the selection kernels: the compositor's lists (no ties: random values, distinct losers)"""
    inp = composite_inputs(n_init, False, False, (), seed=50 + seed)
    rng = np.random.RandomState(2000 + seed)
    P = len(inp["pt_off"])
    inp["d_rgb"], inp["d_sigma"] = rng.randn(P, 3).astype(np.float32), rng.randn(P).astype(np.float32)
    return inp


LATTICE = 4096                     # normalised coordinates on a 2^-12 lattice
BIG_V = 4096 * 256 + 256 + 101     # second grid-stride round: one full workgroup, then one whose second wave is partly dead
HASH_V = (1, 63, 65, 257, 6000)
HASH_CASES = tuple((L, V) for L in (8, 16) for V in HASH_V) + ((16, BIG_V),)     # the large case: the 16-level field


def _one_cell_block(lv, rng, n_reduced=8):
    """a 4 x 4 x 4 block of lattice points that shares one cell on every level < n_reduced"""
    while True:
        q = rng.randint(8, LATTICE - 8, 3)
        lo, hi = q / LATTICE, (q + 3) / LATTICE
        if all((np.floor(level_pos32(lo, lv.scale[l])) == np.floor(level_pos32(hi, lv.scale[l]))).all()
               for l in range(min(n_reduced, lv.n_levels))):
            return q


def hashgrid_lattice_inputs(lv, V, seed=0):
    """Field with centre 0 and scale 1; x = q / 4096 - 0.5 (exact in fp32, and so is x + 0.5).  The head of the array is
    structured: rows 0..63 in one cell on every reduced level, then runs of 1..90 rows per cell (they straddle wave
    boundaries), 30 % of the rows without gradient; then points outside the unit cube on one, two and three axes and on
    its faces; random lattice points after that."""
    rng = np.random.RandomState(3000 + seed + V % 977)
    q = rng.randint(0, LATTICE + 1, (V, 3)).astype(np.int64)
    i = 0
    base = _one_cell_block(lv, rng)
    while i < min(V, 2048):
        n = 64 if i == 0 else int(rng.randint(1, 91))
        n = min(n, V - i)
        q[i:i + n] = base + rng.randint(0, 4, (n, 3))
        base = _one_cell_block(lv, rng)
        i += n
    out = np.arange(min(V, 2048), min(V, 2048 + 96))
    for j, r in enumerate(out):
        axes = rng.permutation(3)[:1 + j % 3]
        q[r, axes] = np.where(rng.rand(len(axes)) < 0.5, -rng.randint(1, 900, len(axes)), LATTICE + rng.randint(1, 900, len(axes)))
    face = np.arange(min(V, 2144), min(V, 2144 + 32))
    q[face, rng.randint(0, 3, len(face))] = np.where(rng.rand(len(face)) < 0.5, 0, LATTICE)
    if V == 1:
        q[0] = (1000, 2000, 3000)
    if 60 < V < 2048:                           # some outside points in the small cases as well
        q[40, 0], q[41, 1], q[41, 2], q[42] = -7, LATTICE + 9, -300, (-1, LATTICE + 1, LATTICE + 555)
        q[43, 2], q[44, 0] = 0, LATTICE
    x = (q.astype(np.float64) / LATTICE - 0.5).astype(np.float32)
    dfeat = (rng.randn(V, 2 * lv.n_levels) * 1e-2).astype(np.float32)
    dfeat[rng.rand(V) < 0.3] = 0
    dfeat[0] = 0.01                             # (the one-cell wave starts and ends on live rows)
    if V > 63:
        dfeat[63] = -0.02
    table = (rng.uniform(-0.5, 0.5, (lv.n_entries, 2))).astype(np.float16)
    return dict(x=x, dfeat=dfeat, table=table, center=np.zeros(3, np.float32), fscale=np.ones(3, np.float32))


# a body-sized box as NeRFNGPNet.initialize(bbox) derives centre and scale from it: nothing dyadic
REAL_CENTER = np.array([0.0137, -0.2871, 0.0209], np.float32)
REAL_SCALE = np.array([2.0713, 2.3859, 1.1047], np.float32)
REAL_V = 40000


def hashgrid_real_inputs(lv, seed=0):
    rng = np.random.RandomState(4000 + seed)
    u = rng.rand(REAL_V, 3)
    u[:2000] = u[:2000] * 1.2 - 0.1             # some of them outside the box
    to_x = lambda u: ((u - 0.5) * REAL_SCALE.astype(np.float64) + REAL_CENTER.astype(np.float64)).astype(np.float32)
    x = to_x(u)
    # dx is piecewise constant across cells: rows within a few ulp of a cell face (3 % of random rows at 16 levels, where
    # an ulp of pos is 5e-4 of a cell) are drawn again, so that the comparison per point has next to nothing to exclude
    for _ in range(20):
        bad = near_cell_face(x, REAL_CENTER, REAL_SCALE, lv, ulps=4)
        if not bad.any():
            break
        x[bad] = to_x(rng.rand(int(bad.sum()), 3) * 1.1 - 0.05)
    dfeat = (rng.randn(REAL_V, 2 * lv.n_levels) * 1e-2).astype(np.float32)
    table = (rng.uniform(-0.5, 0.5, (lv.n_entries, 2))).astype(np.float16)
    return dict(x=x, dfeat=dfeat, table=table, center=REAL_CENTER, fscale=REAL_SCALE)


def smpl_nn_inputs(over_cap, seed=0):
    """hand-made compaction: P points, the valid ones (one candidate each) in a shuffled order; 300 of them on ONE vertex,
    most vertices without a candidate; rows of g with zeros; n_cand below or above cap"""
    rng = np.random.RandomState(5000 + seed)
    P, V = 3001, 517
    pts = rng.randn(P, 3).astype(np.float32)
    valid = rng.permutation(P)[:1800]
    idx = np.full(P, -1, np.int32)
    idx[valid] = rng.randint(0, 40, len(valid)) * 7
    idx[valid[:300]] = 11
    cand_pt = valid.astype(np.int32)
    g = rng.randn(len(valid), 3).astype(np.float32)
    g[rng.rand(len(valid)) < 0.2, rng.randint(0, 3)] = 0
    g[5:9] = 0
    T_inv = np.tile(np.eye(4, dtype=np.float32), (V, 1, 1))
    T_inv[:, :3, :] = rng.randn(V, 3, 4).astype(np.float32)
    if over_cap:
        cap, n_cand = 1500, len(valid)          # the counter ran past the capacity: rows >= cap do not exist
        cand_pt, g = cand_pt[:cap].copy(), g[:cap].copy()
    else:
        cap, n_cand = len(valid), 1700          # fewer candidates than capacity: rows >= n_cand are stale
    return dict(pts=pts, cand_pt=cand_pt, idx=idx, n_cand=n_cand, cap=cap, T_inv=T_inv, d_cand_xc=g)


RAY_SAMPLE_COUNTS = (0, 1, 63, 64, 65, 300, 0, 17, 64, 129, 300)


def ray_samples_inputs(seed=0):
    rng = np.random.RandomState(6000 + seed)
    cnt = np.array(RAY_SAMPLE_COUNTS, np.int32)
    assert len(cnt) % 4 != 0
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    S = int(cnt.sum())
    return dict(ray_off=off, ray_cnt=cnt, s_z=rng.uniform(0.5, 3.5, S).astype(np.float32), d_pts=rng.randn(S, 3).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# the K of |got - ref| <= K u M, per kernel output (fp32 roundings counted from the kernel sources, -ffp-contract=off)
# ---------------------------------------------------------------------------------------------------------------------
def bound_table(ref):
    # k_hashgrid_bwd, one term wt * d: up to three (1 - w), two products of the weights, one product with dfeat = 6
    return (ref["n_table"][:, None] + 6) * U * ref["m_table"]


def bound_dx(ref, n_levels):
    # 8 L terms per axis (levels x corners); one term scale * s * wy * wz * dot / fscale: two (1 - w), the dot's two
    # products and sum, three products (scale * +-1 is exact), the final division = 9
    return (8 * n_levels + 9) * U * ref["m_dx"]


def bound_feat(mag):
    # level_reduce: the product is rounded to half (1), eight half additions (8), fp32 weight arithmetic below that: K = 10
    # in units of the fp16 roundoff; 9 roundings may each fall into the subnormal halves (2^-25 absolute)
    return 10 * U16 * mag + 9 * 2.0 ** -25


def bound_T_inv(ref):
    # k_smpl_nn_bwd: one product g * x per term (none in column 3)
    return (ref["n_T_inv"][:, None, None] + 1) * U * ref["m_T_inv"]


def bound_pts(ref):
    # three terms T * g, one product each
    return 4 * U * ref["m_pts"]


def bound_rays(ref, ray_cnt):
    # k_ray_samples_bwd: cnt terms; d_o adds them as they are, d_d after one product z * g
    c = np.asarray(ray_cnt, np.float64)[:, None]
    return c * U * ref["m_o"], (c + 1) * U * ref["m_d"]
