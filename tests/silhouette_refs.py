"""Float64 restatement of the soft silhouette and its gradient -- ia_sil_project_fwd / _bwd, ia_sil_render_fwd / _bwd, ia_sil_body_bwd
(csrc/ia_silhouette.hip, csrc/ia_keypoints.hip; include/instantavatar_hip_silhouette.h; DESIGN.md section 4, "silhouette
refinement") -- with the seeded cases and the per-element error bound that tests/test_gpu_silhouette.py holds the kernels to and
tests/test_cpu_silhouette_refs.py validates on the CPU.  numpy only, no product import; the body-model pieces are those of
tests/keypoint_refs.py and tests/smpl_refs.py.

Every stage takes the fp32 arrays of the stage before it as EXACT inputs (the render takes fp32 screen / inv_z, the render backward
fp32 alpha / d_alpha, the projection backward fp32 d_screen, the body backward fp32 d_verts), so a comparison measures one kernel's
arithmetic and not the conditioning of x = d / sigma.  The render is evaluated densely, vectorised over [pixels, faces, edges].

The bound, per output ELEMENT: allow = K . u . M + extra, u = 2^-24.  M is a first-order worst-case rounding analysis of the
definition evaluated in fp32 (every operation rounded once, relative u), written with the real float64 terms:

  pair (pixel P, face f), edge k:  e = v_k+1 - v_k, w = P - v_k, t = clamp(w.e / |e|^2), q = w - t e, dist2 = |q|^2
      delta q_c   <= 2 u (|w_c| + t |e_c|) =: u mq_c
      delta x     <= u [6 |x| + (scale / sigma) 2 (|q_x| mq_x + |q_y| mq_y)] =: u mx       (delta t enters dist2 in second order)
      delta t     <= u [3 (|w_x e_x| + |w_y e_y|) / |e|^2 + 2 t] =: u mt                     (the clamp is 1-Lipschitz)
  alpha = 1 - prod (1 - p_f), 1 - p = 1 / (1 + exp(x)):  each factor carries 5 u relative (exp, add, divide, multiply) + p_f delta x
      M(alpha)    = 1 + (1 - alpha) sum_f (5 + p_f mx_f)
      M(d_alpha)  = 2 M(alpha) / (H W) + 4 |d_alpha|
      M(loss)     = sum_pixels 2 |alpha - m| M(alpha) / (H W) + (24 + tiles / 256) L        (two trees of 256 and a strided sum)
  d_screen[v] = sum over the pairs of v's faces of g = G s q, G = 2 up p c, up = d_alpha (1 - alpha), c = scale / sigma, s = 1 - t or t
      M(pair, c)  = G [ (12 + mx) s |q_c| + s mq_c + mt (|q_c| + s |e_c|) ] + (T_f + 16) |g_c|,   T_f = ceil(box pixels / 64)
                    (coefficient, q, t, and the face's summation: T_f terms per lane, a tree of 6, the gather)
  projection: p = R X + t carries 4 u sum |terms| =: u mp per row; u = fx p.x / p.z + cx
      M(screen)   = (f / |p.z|) mp_xy + |f p / p.z^2| mp_z + 3 |f p / p.z| + |u|;   M(inv_z) = (mp_z / |p.z| + 1) / |p.z|
      M(d_verts)  = the same propagation through d0 = du fx / p.z, d1, d2 = -(d0 p.x + d1 p.y) / p.z and R^T
K = 4: M is already a worst-case first-order bound (K = 1 would hold if every term were tight); a factor 2 covers the second-order
terms and a device expf / division of 2 ulp, and a factor 2 is margin.  Nothing in the bound comes from a kernel's output.

`extra` is the explicit allowance of the two genuine discontinuities (margin 1e-4 relative, ALLOW_MARGIN):
  * cut: a pair that is not inside and whose d lies within 1e-4 blur_radius of blur_radius may be in or out.  It is allowed
    p_f (1 - alpha) in alpha (and what follows from it in d_alpha and the loss) and its own gradient magnitude in d_screen.
  * tie: a pair whose two nearest edges differ by less than 1e-4 relative in dist2 and have different closest points may send its
    gradient to either edge.  It is allowed that pair's magnitude 2 G (|q| of either edge) on the face's three vertices.
The pairs given an allowance are at most 2 % (ALLOW_CAP) of the live pairs (contributing, |x| < 30) of each case; the shares of the
seeded cases are recorded in ALLOW_SHARE below.  Vertex ties (both edges' closest point is their shared vertex) are harmless: the
gradient goes to that vertex either way.

measured, the largest (error - extra) / (u M) over the seven cases (the bound is K = 4 times that unit):
                          float32, second association (CPU)      kernels (MI355X, tests/test_gpu_silhouette.py)
    ia_sil_project_fwd    0.729 screen, tubes-70x33              0.729 screen, tubes-70x33
    ia_sil_project_bwd    0.418 tubes-33x70                      0.339 tubes-40x48
    ia_sil_render_fwd     2.065 alpha, tubes-64x64-s1e-4         0.493 alpha, tubes-64x64-s1e-4
    ia_sil_render_bwd     2.133 tubes-64x64-s1e-4                0.092 tubes-70x33 / edge-cases
    ia_sil_body_bwd       (keypoint_refs' groups and K = 16)     2.492 of 16, d_pose[1][12] of f9-v257-star
The second association exceeds 1 because it forms q = P - (v + t e), whose rounding is u |v| (up to 64 px) where M counts the
definition's q = (P - v) - t e with u |P - v|: the association is there to show that K has room, not that M describes it.  The kernels
evaluate the definition's order and stay below 1.
`SilhouetteRefiner.refine` (three frames of 48 x 48, 336 faces, sigma 1e-3, 10 LBFGS steps; recorded, not gated):
    loss 4.981e-03 -> 3.300e-07, 2.238e-03 -> 3.990e-07, 1.967e-03 -> 2.569e-07;  IoU 0.867 -> 0.997, 0.926 -> 1.000, 0.934 -> 1.000
"""
import functools

import numpy as np

import keypoint_refs as kr
import smpl_refs as sr

U = 2.0 ** -24
K_BOUND = 4
XY_MAX = 16384.0
ALLOW_MARGIN = 1e-4
ALLOW_CAP = 0.02
#: the largest error / (u M) per entry: (float32 second association on the CPU, MI355X)
MEASURED = {"ia_sil_project_fwd": (0.729, 0.729), "ia_sil_project_bwd": (0.418, 0.339), "ia_sil_render_fwd": (2.065, 0.493),
            "ia_sil_render_bwd": (2.133, 0.092), "ia_sil_body_bwd": (None, 2.492), "refine_loss_ratio": (None, 1.78e-4)}
#: share of the live pairs that get an allowance, per case (measured with this file on the CPU)
ALLOW_SHARE = {"edge-cases": 0.0052, "no-faces": 0.0, "one-triangle": 0.0, "tubes-33x70": 0.0031, "tubes-40x48": 0.0036,
               "tubes-64x64-s1e-4": 0.0029, "tubes-70x33": 0.0038}
DEFECTS = {"half_pixel": "fwd", "max_hw": "fwd", "no_inside_sign": "fwd", "no_cut": "fwd", "t_unclamped": "fwd", "t_swapped": "bwd",
           "no_one_minus_alpha": "bwd", "wrong_mean_count": "fwd"}


def default_blur(sigma):
    """refine-smpl.py: blur_radius = log(1 / 1e-4 - 1) * sigma"""
    return float(np.log(1.0 / 1e-4 - 1.0) * sigma)


# ---- projection --------------------------------------------------------------------------------------------------------------
def project_ref(verts, w2c, cam, dtype=np.float64):
    """cam = (fx, fy, cx, cy, near) -> dict screen [nv,2], inv_z [nv], valid [nv] and the magnitudes m_screen, m_inv_z"""
    dt = dtype
    X, Rt = np.asarray(verts).astype(dt), np.asarray(w2c).reshape(4, 4)[:3].astype(dt)
    fx, fy, cx, cy, near = (dt(np.float32(v)) for v in cam)
    terms = Rt[None, :, :3] * X[:, None, :]                                   # [nv,3,3]
    p = ((terms[..., 0] + terms[..., 1]) + terms[..., 2]) + Rt[None, :, 3]
    mp = 4 * (np.abs(terms).sum(-1) + np.abs(Rt[None, :, 3]))
    f = np.array([fx, fy], dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = f * p[:, :2] / p[:, 2:3]
        uv = r + np.array([cx, cy], dt)
        iz = 1 / p[:, 2]
        valid = (p[:, 2] >= near) & (np.abs(uv) <= XY_MAX).all(1) & (iz > 0) & np.isfinite(iz)
        m_uv = f / np.abs(p[:, 2:3]) * mp[:, :2] + np.abs(r / p[:, 2:3]) * mp[:, 2:3] + 3 * np.abs(r) + np.abs(uv)
        m_iz = (mp[:, 2] / np.abs(p[:, 2]) + 1) * np.abs(iz)
    z = lambda a: np.where(valid.reshape((-1,) + (1,) * (a.ndim - 1)), a, 0).astype(dt)
    return dict(screen=z(uv), inv_z=z(iz), valid=valid, p=p, mp=mp, m_screen=z(m_uv), m_inv_z=z(m_iz), f=f, Rt=Rt)


def project_bwd_ref(verts, w2c, cam, d_screen, dtype=np.float64):
    """-> dict d_verts [nv,3] (zeros for an invalid vertex), m_d_verts"""
    r = project_ref(verts, w2c, cam, dtype)
    dt = dtype
    p, mp, f, Rt, ok = r["p"], r["mp"], r["f"], r["Rt"], r["valid"]
    ds = np.asarray(d_screen).astype(dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d01 = ds * f / p[:, 2:3]
        m01 = np.abs(d01) * (2 + mp[:, 2:3] / np.abs(p[:, 2:3]))
        s = d01[:, 0] * p[:, 0] + d01[:, 1] * p[:, 1]
        d2 = -s / p[:, 2]
        m2 = ((m01 * np.abs(p[:, :2]) + np.abs(d01) * mp[:, :2]).sum(1) + 3 * np.abs(d01 * p[:, :2]).sum(1)) / np.abs(p[:, 2]) \
            + np.abs(d2) * (mp[:, 2] / np.abs(p[:, 2]) + 1)
        d = np.concatenate([d01, d2[:, None]], 1)
        m = np.concatenate([m01, m2[:, None]], 1)
        t = Rt[None, :, :3] * d[:, :, None]                                   # [nv, row, c]
        g = (t[:, 0] + t[:, 1]) + t[:, 2]
        mg = (np.abs(Rt[None, :, :3]) * m[:, :, None]).sum(1) + 3 * np.abs(t).sum(1)
    return dict(d_verts=np.where(ok[:, None], g, 0).astype(dt), m_d_verts=np.where(ok[:, None], mg, 0))


# ---- render --------------------------------------------------------------------------------------------------------------------
def _area32(s32, fi):
    a, b, c = s32[fi[:, 0]], s32[fi[:, 1]], s32[fi[:, 2]]
    return (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (c[:, 0] - a[:, 0]) * (b[:, 1] - a[:, 1])     # float32, products rounded separately


def render_ref(screen, inv_z, faces, H, W, sigma, blur, mask=None, dtype=np.float64, second=False, defect=None):
    """ia_sil_render_fwd on fp32 screen [nv,2] / inv_z [nv] taken as exact.  -> dict with alpha [H*W], loss, d_alpha (with a mask) and
    the pair arrays [pixels, kept faces] the backward and the bound need.  dtype=np.float32 evaluates the same expressions in float32;
    second=True is the second association (t through a reciprocal, q = P - (v + t e), the product over the faces reversed).
    defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    dt = dtype
    s32, iz = np.asarray(screen, np.float32).reshape(-1, 2), np.asarray(inv_z, np.float32).reshape(-1)
    nv = s32.shape[0]
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    in_range = ((faces >= 0) & (faces < nv)).all(1) if nv else np.zeros(len(faces), bool)
    fi = np.where(in_range[:, None], faces, 0)
    vok = (iz > 0) & np.isfinite(iz) & (np.abs(s32) <= XY_MAX).all(1) if nv else np.zeros(0, bool)
    ok = in_range & (vok[fi].all(1) if nv else False)
    A = _area32(s32, fi) if nv else np.zeros(len(faces), np.float32)
    ok = ok & (A != 0)
    keep = np.nonzero(ok)[0]
    sgn = np.where(A[keep] > 0, 1.0, -1.0).astype(dt)
    v = s32.astype(dt)[fi[keep]]                                              # [nk,3,2]
    off = 0.5 if defect == "half_pixel" else 0.0
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    P = np.stack([xs.reshape(-1) + off, ys.reshape(-1) + off], -1).astype(dt)  # [np,2]
    e = np.roll(v, -1, axis=1) - v                                            # [nk,3,2]
    w = P[:, None, None, :] - v[None]                                         # [np,nk,3,2]
    len2 = e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]
    we = w[..., 0] * e[None, ..., 0] + w[..., 1] * e[None, ..., 1]
    tu = we * (dt(1) / len2)[None] if second else we / len2[None]
    t = tu if defect == "t_unclamped" else np.clip(tu, 0, 1)
    q = P[:, None, None, :] - (v[None] + t[..., None] * e[None]) if second else w - t[..., None] * e[None]
    d2 = q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]                        # [np,nk,3]
    E = e[None, ..., 0] * w[..., 1] - e[None, ..., 1] * w[..., 0]
    inside = (sgn[None, :, None] * E > 0).all(-1)
    kwin = np.argmin(d2, -1)                                                  # the first minimum: the lower edge wins a tie
    pick = lambda a: np.take_along_axis(a, kwin[..., None], 2)[..., 0]
    dist2 = pick(d2)
    side = max(H, W) if defect == "max_hw" else min(H, W)
    cs = dt(np.float32(2) / np.float32(side)) if dt is np.float32 else 2.0 / side
    scale = dt(cs * cs)
    sig, blr = dt(np.float32(sigma)), dt(np.float32(blur))
    d = dist2 * scale
    contrib = np.ones_like(inside) if defect == "no_cut" else (inside | (d < blr))
    pos = inside if defect != "no_inside_sign" else np.zeros_like(inside)
    x = np.where(pos, d / sig, -(d / sig))
    with np.errstate(over="ignore"):
        om = dt(1) / (dt(1) + np.exp(x))                                      # 1 - p
        pf = dt(1) / (dt(1) + np.exp(-x))
    fac = np.where(contrib, om, dt(1))
    prod = np.prod(fac[:, ::-1] if second else fac, axis=1, dtype=dt) if fac.shape[1] else np.ones(H * W, dt)
    alpha = (dt(1) - prod).astype(dt)
    out = dict(alpha=alpha, keep=keep, faces=fi, nv=nv, H=H, W=W, v=v, e=e, w=w, t=t, tu=tu, q=q, d2=d2, kwin=kwin, inside=inside, pos=pos, d=d,
               x=x, pf=pf, contrib=contrib, scale=scale, sigma=sig, blur=blr, dist2=dist2, pick=pick, P=P)
    if mask is not None:
        m = np.asarray(mask, np.float32).reshape(-1).astype(dt)
        r = alpha - m
        cnt = dt(H * H if defect == "wrong_mean_count" else H * W)
        sq = r * r
        out.update(loss=(sq[::-1] if second else sq).sum(dtype=dt) / cnt, d_alpha=(dt(2) * r / cnt).astype(dt), resid=r, cnt=cnt)
    return out


def _pair_mags(R):
    """the magnitudes of the module docstring on the winning edge of every pair: mq [np,nk,2], mx, mt [np,nk]"""
    pick = R["pick"]
    k = R["kwin"]
    ew = np.take_along_axis(np.broadcast_to(R["e"][None], R["w"].shape), k[..., None, None], 2)[:, :, 0]      # [np,nk,2]
    ww = np.take_along_axis(R["w"], k[..., None, None], 2)[:, :, 0]
    qw = np.take_along_axis(R["q"], k[..., None, None], 2)[:, :, 0]
    tw = pick(R["t"])
    mq = 2 * (np.abs(ww) + tw[..., None] * np.abs(ew))
    c = R["scale"] / R["sigma"]
    mx = 6 * np.abs(R["x"]) + c * 2 * (np.abs(qw) * mq).sum(-1)
    len2 = (ew * ew).sum(-1)
    mt = 3 * np.abs(ww * ew).sum(-1) / len2 + 2 * tw
    return dict(ew=ew, ww=ww, qw=qw, tw=tw, mq=mq, mx=mx, mt=mt, c=c)


def _allowed_pairs(R):
    """(cut [np,nk], tie [np,nk]) -- the pairs of the two discontinuities"""
    d, blur = R["d"], R["blur"]
    cut = ~R["inside"] & (np.abs(d - blur) <= ALLOW_MARGIN * blur)
    d2s = np.sort(R["d2"], -1)
    near = (d2s[..., 1] - d2s[..., 0]) <= ALLOW_MARGIN * d2s[..., 1]
    order = np.argsort(R["d2"], -1, kind="stable")
    k0, k1 = order[..., 0], order[..., 1]
    cp = R["v"][None] + R["t"][..., None] * R["e"][None]                      # closest points [np,nk,3,2]
    c0 = np.take_along_axis(cp, k0[..., None, None], 2)[:, :, 0]
    c1 = np.take_along_axis(cp, k1[..., None, None], 2)[:, :, 0]
    tie = near & (np.abs(c0 - c1).max(-1) > 0) & R["contrib"]
    return cut, tie, k1


def fwd_bound(R):
    """{output: (reference, allow [same shape], u M, extra)} of alpha and, with a mask, d_alpha and loss; and the allowance share"""
    pm = _pair_mags(R)
    a = R["alpha"]
    live = R["contrib"]
    M_a = 1 + (1 - a) * np.where(live, 5 + R["pf"] * pm["mx"], 0).sum(1)
    cut, tie, _ = _allowed_pairs(R)
    extra_a = np.where(cut, R["pf"] * (1 - a)[:, None] / np.maximum(1 - R["pf"], 0.5), 0).sum(1)
    out = {"alpha": (a, K_BOUND * U * M_a + extra_a, U * M_a, extra_a)}
    if "loss" in R:
        HW = R["cnt"]
        da, L, r = R["d_alpha"], R["loss"], R["resid"]
        M_d, ex_d = 2 * M_a / HW + 4 * np.abs(da), 2 * extra_a / HW
        tiles = -(-R["H"] // 16) * -(-R["W"] // 16)
        M_L = (2 * np.abs(r) * M_a).sum() / HW + (24 + tiles / 256) * L
        ex_L = (2 * np.abs(r) * extra_a + extra_a ** 2).sum() / HW
        out["d_alpha"] = (da, K_BOUND * U * M_d + ex_d, U * M_d, ex_d)
        out["loss"] = (np.array([L]), np.array([K_BOUND * U * M_L + ex_L]), np.array([U * M_L]), np.array([ex_L]))
    n_live = int((live & (np.abs(R["x"]) < 30)).sum())
    share = float((cut | tie).sum()) / max(n_live, 1)
    return out, share


def render_bwd_ref(R, alpha, d_alpha, second=False, defect=None, with_bound=True):
    """ia_sil_render_bwd on the geometry R of render_ref and fp32 alpha / d_alpha [H*W] taken as exact -> dict d_screen [nv,2], fgrad
    [kept faces,3,2] and (float64 only) the allowance arrays"""
    dt = R["alpha"].dtype.type
    al, da = np.asarray(alpha, np.float32).reshape(-1).astype(dt), np.asarray(d_alpha, np.float32).reshape(-1).astype(dt)
    up = da if defect == "no_one_minus_alpha" else da * (dt(1) - al)
    pm = _pair_mags(R)
    c = dt(R["scale"] / R["sigma"])
    gd = np.where(R["contrib"], up[:, None] * R["pf"] * np.where(R["pos"], c, -c), 0).astype(dt)             # d L / d dist2 [np,nk]
    tw = pm["tw"]
    sa, sb = (tw, 1 - tw) if defect == "t_swapped" else (1 - tw, tw)
    ga, gb = dt(-2) * sa * gd, dt(-2) * sb * gd
    nk = len(R["keep"])
    k = R["kwin"]
    fg = np.zeros((nk, 3, 2), dt)
    mfg, exf = np.zeros((nk, 3, 2)), np.zeros((nk, 3, 2))
    order = slice(None, None, -1) if second else slice(None)
    if with_bound:
        G = np.abs(2 * gd)
        cut, tie, k1 = _allowed_pairs(R)
        # T_f: pixels of the grown, clipped box over 64
        grow = np.sqrt(float(R["blur"]) / float(R["scale"]))
        lo, hi = R["v"].min(1) - grow - 1, R["v"].max(1) + grow + 1
        bw = np.clip(np.minimum(hi[:, 0], R["W"] - 1) - np.maximum(lo[:, 0], 0) + 1, 0, None)
        bh = np.clip(np.minimum(hi[:, 1], R["H"] - 1) - np.maximum(lo[:, 1], 0) + 1, 0, None)
        Tf = np.ceil(bw * bh / 64)
        q1 = np.take_along_axis(R["q"], k1[..., None, None], 2)[:, :, 0]
        qmax = np.maximum(np.abs(pm["qw"]), np.abs(q1))
    for corner in range(3):
        isa, isb = k == corner, (k + 1) % 3 == corner
        s = np.where(isa, ga, 0) + np.where(isb, gb, 0)
        g = s[..., None] * pm["qw"]
        fg[:, corner] = g[order].sum(0, dtype=dt)
        if with_bound:
            sm = np.where(isa, sa, 0) + np.where(isb, sb, 0)
            m = G[..., None] * ((12 + pm["mx"])[..., None] * sm[..., None] * np.abs(pm["qw"]) + sm[..., None] * pm["mq"]
                                + pm["mt"][..., None] * (np.abs(pm["qw"]) + sm[..., None] * np.abs(pm["ew"]))) * (isa | isb)[..., None] \
                + (Tf[None, :, None] + 16) * np.abs(g)
            mfg[:, corner] = m.sum(0)
            exf[:, corner] = (np.where(cut, 1, 0)[..., None] * np.abs(g)).sum(0) + (np.where(tie, G, 0)[..., None] * 2 * qmax).sum(0)
    ds, M, ex = np.zeros((R["nv"], 2), dt), np.zeros((R["nv"], 2)), np.zeros((R["nv"], 2))
    idx = R["faces"][R["keep"]]
    if second:
        idx, fg_o = idx[::-1], fg[::-1]
    else:
        fg_o = fg
    for corner in range(3):
        np.add.at(ds, idx[:, corner], fg_o[:, corner])
        if with_bound:
            np.add.at(M, R["faces"][R["keep"]][:, corner], mfg[:, corner])
            np.add.at(ex, R["faces"][R["keep"]][:, corner], exf[:, corner])
    out = dict(d_screen=ds, fgrad=fg)
    if with_bound:
        out["bound"] = {"d_screen": (ds, K_BOUND * U * M + ex, U * M, ex)}
    return out


# ---- the body-model adjoint ------------------------------------------------------------------------------------------------------
def body_bwd_ref(body, betas, pose, transl, d_verts, dtype=np.float64, assoc="root", reverse=False):
    """ia_sil_body_bwd: the lower half of keypoint_refs.kp_bwd_ref with the vertex cotangent handed in and none of the joints"""
    dt = dtype
    F = np.asarray(pose).reshape(-1, 72).shape[0]
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = kr.kp_fwd_ref(body, betas, pose, transl, eye, np.zeros((F, 25, 3)), kr.THRESHOLD, np.zeros(kr.N_KPV, np.int64), dt, assoc, reverse)
    b, V = r["b"], r["V"]
    dvert = np.asarray(d_verts, np.float32).reshape(F, V, 3).astype(dt)
    T, vp, w = r["T"], r["vp"], b["lbs_weights"]
    dT = np.zeros((F, V, 4, 4), dt)
    dT[..., :3, :3] = dvert[..., :, None] * vp[..., None, :]
    dT[..., :3, 3] = dvert
    dvp = T[..., 0, :3] * dvert[..., 0, None] + T[..., 1, :3] * dvert[..., 1, None] + T[..., 2, :3] * dvert[..., 2, None]
    order = slice(None, None, -1) if reverse else slice(None)
    dA = (np.ascontiguousarray(w[order].T) @ dT[:, order].reshape(F, V, 16)).reshape(F, sr.N_J, 4, 4)
    flat = dvp[:, order].reshape(F, V * 3)
    pd = b["posedirs"].reshape(207, V, 3)[:, order].reshape(207, V * 3)
    dpf = flat @ pd.T if r["has_pd"] else np.zeros((F, 207), dt)
    sd = b["shapedirs"][order].reshape(V * 3, 10)
    db_shape, m_db_shape = flat @ sd, np.abs(flat) @ np.abs(sd)
    djoint = np.zeros((F, sr.N_J, 3), dt)
    d_transl, m_d_transl = dvert[:, order].sum(1), np.abs(dvert).sum(1)
    dL, dJ, m_dL = kr._chain_bwd(dA, djoint, r["L"], r["G"], r["C"], b["parents"])
    dR, m_dR = dL[..., :3, :3].copy(), m_dL[..., :3, :3].copy()
    dR[:, 1:] = dR[:, 1:] + dpf.reshape(F, 23, 3, 3)
    m_dR[:, 1:] = m_dR[:, 1:] + np.abs(dpf).reshape(F, 23, 3, 3)
    d_pose = sr._rodrigues_bwd(r["rod"], dR.reshape(F * sr.N_J, 3, 3), -1).reshape(F, 72)
    m_d_pose = sr._rodrigues_bwd(sr._abs_rod(r["rod"]), m_dR.reshape(F * sr.N_J, 3, 3), +1).reshape(F, 72)
    db_f = (b["JS"] * dJ[..., None]).sum((1, 2)) + db_shape
    m_db_f = (np.abs(b["JS"]) * np.abs(dJ)[..., None]).sum((1, 2)) + m_db_shape
    return dict(d_betas=db_f[order].sum(0), d_pose=d_pose, d_transl=d_transl, m_d_betas=m_db_f.sum(0), m_d_pose=m_d_pose, m_d_transl=m_d_transl,
                verts=r["verts"])


def body_bwd_bound(body, betas, pose, transl, d_verts):
    """{group: (ref, allow, E32, M)} in the groups and with the K of keypoint_refs (allow = K max(E32, u M))"""
    a = (body, betas, pose, transl, d_verts)
    R64, R32 = body_bwd_ref(*a), body_bwd_ref(*a, dtype=np.float32)
    return sr._allow(kr.bwd_groups(R64), kr.bwd_groups(R32), kr.bwd_groups(R64, "m_d_"), K=kr.K_BOUND), R64


# ---- seeded cases --------------------------------------------------------------------------------------------------------------
def tube_mesh(g, n_tubes=3, sides=6, rings=7, size=1.0):
    """closed tubes with seeded axes, radii and a bend (world units ~ size): n_tubes * (sides rings + 2) vertices,
    n_tubes * 2 sides rings faces (3 x 6 x 7: 132 vertices, 252 faces)"""
    V, Fc = [], []
    for _ in range(n_tubes):
        a, b = g.uniform(-size, size, 3) * [1, 1, 0.3], g.uniform(-size, size, 3) * [1, 1, 0.3]
        ax = (b - a) / np.linalg.norm(b - a)
        u = np.cross(ax, [0.3, 0.2, 1.0]); u /= np.linalg.norm(u)
        w = np.cross(ax, u)
        rad, bend, phi0 = g.uniform(0.08, 0.25) * size, g.uniform(-0.3, 0.3) * size, g.uniform(0, 2 * np.pi)
        base = len(V)
        for i in range(rings):
            s = i / (rings - 1)
            c = a + (b - a) * s + bend * np.sin(np.pi * s) * u
            for k in range(sides):
                ang = phi0 + 2 * np.pi * k / sides
                V.append(c + rad * (np.cos(ang) * u + np.sin(ang) * w))
        c0, c1 = len(V), len(V) + 1
        V.extend([a, b])
        for k in range(sides):
            k1 = (k + 1) % sides
            for i in range(rings - 1):
                p, q = base + i * sides, base + (i + 1) * sides
                Fc.extend([(p + k, p + k1, q + k1), (p + k, q + k1, q + k)])
            Fc.extend([(c0, base + k1, base + k), (c1, base + (rings - 1) * sides + k, base + (rings - 1) * sides + k1)])
    return np.asarray(V, np.float32), np.asarray(Fc, np.int32)


def camera(g, H, W, depth=4.0, focal=None):
    """(w2c [4,4] fp32 with a small seeded rotation, (fx, fy, cx, cy, near))"""
    Rc = sr._rodrigues(np.concatenate([g.standard_normal(3) * 0.1, np.zeros(69)]).astype(np.float32), np.float64)["R"][0]
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = Rc, [0.05, -0.03, depth]
    f = float(focal if focal is not None else 1.3 * min(H, W))
    return w2c.astype(np.float32), (f, f * 1.02, (W - 1) / 2 + 0.3, (H - 1) / 2 - 0.2, 0.05)


#: name: (seed, H, W, sigma, kind)
CASES = {
    "tubes-40x48":        (3, 40, 48, 1e-3, "tubes"),
    "tubes-33x70":        (1, 33, 70, 1e-3, "tubes"),
    "tubes-70x33":        (2, 70, 33, 1e-3, "tubes"),
    "tubes-64x64-s1e-4":  (3, 64, 64, 1e-4, "tubes"),
    "one-triangle":       (4, 24, 31, 1e-3, "triangle"),
    "edge-cases":         (5, 40, 48, 1e-3, "edges"),
    "no-faces":           (6, 17, 19, 1e-3, "empty"),
}
DEFECT_CASE = "tubes-33x70"      # not square: max(H, W) and H * H differ from min(H, W) and H * W


@functools.lru_cache(maxsize=None)
def inputs(name):
    """the arrays of one case as the C entries take them; treat as read-only"""
    seed, H, W, sigma, kind = CASES[name]
    g = np.random.default_rng(8100 + seed)
    w2c, cam = camera(g, H, W)
    if kind == "triangle":       # covers the whole image and more
        verts = np.array([[-6, -4, 0], [6, -5, 0.2], [0.4, 8, -0.2]], np.float32)
        faces = np.array([[0, 1, 2]], np.int32)
    elif kind == "empty":
        verts, faces = tube_mesh(g, 1)[0], np.zeros((0, 3), np.int32)
    else:
        verts, faces = tube_mesh(g)
    if kind == "edges":
        verts, faces = verts.copy(), faces.copy()
        nv = len(verts)
        far = tube_mesh(g, 1)[0] + np.float32([40, 0, 0])          # a tube wholly off-screen
        off_faces = tube_mesh(np.random.default_rng(1), 1)[1] + nv
        verts = np.concatenate([verts, far]).astype(np.float32)
        faces = np.concatenate([faces, off_faces]).astype(np.int32)
        verts[5:9, 2] = -10.0                                        # behind the camera: their faces are skipped
        verts[20, 2] = -4.0 + 0.01                                    # in front of the camera but closer than near
        faces[10] = (faces[10, 0], faces[10, 1], faces[10, 1])      # A == 0
        faces[30, 2] = len(verts)                                     # index out of range
        faces[31, 0] = -1
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rr = np.hypot(xs - W * 0.45, ys - H * 0.55) / (0.35 * min(H, W))
    mask = (np.round(np.clip(1.3 - rr, 0, 1) * 255) / 255).astype(np.float32).reshape(-1)
    return dict(verts=verts, faces=faces, w2c=w2c, cam=cam, H=H, W=W, sigma=np.float32(sigma), blur=np.float32(default_blur(sigma)), mask=mask)


def vertex_faces(faces, nv):
    """(vf_start [nv+1], vf_corner [n]) int32: the corners 3 f + c of every vertex, by ascending corner; faces with an index out of
    range are left out"""
    faces = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    ok = ((faces >= 0) & (faces < nv)).all(1)
    corner = (np.arange(len(faces))[:, None] * 3 + np.arange(3))[ok].reshape(-1)
    vert = faces[ok].reshape(-1)
    order = np.argsort(vert, kind="stable")
    start = np.zeros(nv + 1, np.int64)
    np.add.at(start, vert + 1, 1)
    return np.cumsum(start).astype(np.int32), corner[order].astype(np.int32)


def check(got, bound, what, lines=None):
    """every element of `got` [name -> array] against {name: (ref, allow, u M, extra)}: prints one "SILREF" line per output, returns
    ({name: worst error / allow} of the outputs over the bound, the worst (error - extra) / (u M))"""
    over, worst = {}, 0.0
    for k, (ref, allow, uM, extra) in bound.items():
        g = np.asarray(got[k], np.float64).reshape(np.shape(ref))
        err = np.where(np.isfinite(g), np.abs(g - ref), np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(uM > 0, np.maximum(err - extra, 0) / uM, np.where(err > extra, np.inf, 0)), initial=0.0))
        bad = err > allow
        line = "SILREF %-34s %-9s worst err/(u M) %.3f%s" % (what, k, ratio, "  OVER in %d elements" % bad.sum() if bad.any() else "")
        print(line)
        if lines is not None:
            lines.append(line)
        worst = max(worst, ratio)
        if bad.any():
            with np.errstate(divide="ignore", invalid="ignore"):
                over[k] = float(np.max(np.where(bad, err / np.maximum(allow, 1e-300), 0)))
    return over, worst
