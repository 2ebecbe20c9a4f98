"""float64 / float32 restatement of `ia_scene_receive`, written from the text of include/instantavatar_hip_scene.h (DESIGN.md
section 4, "scene composition"): `receive`.  It follows the header step by step -- "fp64" steps on Python floats (IEEE doubles, one
operation at a time, math.sqrt correctly rounded), "fp32" steps on numpy float32 scalars -- and loops over pixels, layers and taps,
so its results are meant to be compared with the kernel's BYTES.

Where a discrete choice of a pixel-layer sits within 2^-40 (relative) of flipping, a last-bit difference in a division or a square
root could change the result by a whole tap; such pixel-layers are reported as not `clear`:
  * a tap with m > 0 whose comparison has |s - (rho - bias) m| <= 2^-40 max(|s|, |rho m|),
  * a tap whose (u + dx) + 0.5 or (v + dy) + 0.5 lies within 2^-40 max(1, |.|) of an integer (a rounding boundary of the floor),
  * a border clause within that of equality: zl against near, u and v against 0 and S - 1,
  * cosv within 2^-40 of cos0 or cos1."""
import math

import numpy as np

EPS = 2.0 ** -40
MAX_LAYERS = 8
NAN = float("nan")


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _near(x, y, scale=None):
    """|x - y| <= 2^-40 max(|x|, |y|) (or `scale`)"""
    return abs(x - y) <= EPS * (max(abs(x), abs(y)) if scale is None else scale)


def receive(rays_o, rays_d, c, a, d, nrm, maps_a, maps_d, proj, light, radius=1, strength=0.6, near=0.05, bias_other=0.02,
            bias_self=0.05, cos0=0.0, cos1=0.25):
    """rays_o, rays_d [R,3]; c [K,R,3], a, d [K,R]; nrm None or [K,R,3]; maps_a, maps_d [K,S,S]; proj [K,3,4]; light [3]
    -> dict(shade [K,R] fp32, c_out [K,R,3] fp32, receives [K,R] bool, clear [K,R] bool, abar [K(j),K(k),R] fp32,
            cosv [K,R] fp64 (NaN: no facing term), g [K,R] fp32, X [K,R,3] fp64, rho [K,R] fp64, uv [K(j),K(k),R,2] fp64 (NaN: not
            projected), inside [K(j),K(k),R] bool (the caster's map was tapped))"""
    f32 = lambda x: np.ascontiguousarray(np.asarray(x, np.float32))
    o, dr, c, a, d = f32(rays_o).reshape(-1, 3), f32(rays_d).reshape(-1, 3), f32(c), f32(a), f32(d)
    maps_a, maps_d, proj = f32(maps_a), f32(maps_d), f32(proj)
    K, R = a.shape
    S = maps_a.shape[1]
    assert 1 <= K <= MAX_LAYERS and c.shape == (K, R, 3) and d.shape == (K, R) and o.shape == (R, 3) and dr.shape == (R, 3)
    assert maps_a.shape == (K, S, S) and maps_d.shape == (K, S, S) and proj.shape == (K, 3, 4)
    if nrm is not None:
        nrm = f32(nrm)
        assert nrm.shape == (K, R, 3)
    r = int(radius)
    strength = np.float32(strength)
    one = np.float32(1.0)
    L = [float(np.float32(v)) for v in np.asarray(light).reshape(3)]
    near, bias_other, bias_self, cos0, cos1 = (float(np.float32(v)) for v in (near, bias_other, bias_self, cos0, cos1))
    dcos = cos1 - cos0
    hi = float(S - 1)
    taps = float((2 * r + 1) ** 2)
    # everything the loops read, as Python floats (the fp32 values converted exactly)
    o64, d64, a64, dd64 = o.astype(np.float64).tolist(), dr.astype(np.float64).tolist(), a.astype(np.float64).tolist(), d.astype(np.float64).tolist()
    ma64, md64, M64 = maps_a.astype(np.float64).tolist(), maps_d.astype(np.float64).tolist(), proj.astype(np.float64).tolist()
    n64 = None if nrm is None else nrm.astype(np.float64).tolist()
    with np.errstate(all="ignore"):
        receives = (a > 0) & np.isfinite(a) & np.isfinite(d) & np.isfinite(c).all(-1)
    shade = np.ones((K, R), np.float32)
    c_out = c.copy()
    clear = np.ones((K, R), bool)
    abar_all = np.zeros((K, K, R), np.float32)
    cosv_all = np.full((K, R), NAN)
    g_all = np.zeros((K, R), np.float32)
    X_all = np.full((K, R, 3), NAN)
    rho_all = np.full((K, R), NAN)
    uv = np.full((K, K, R, 2), NAN)
    inside = np.zeros((K, K, R), bool)
    for px in range(R):
        for j in range(K):
            if not receives[j, px]:
                continue
            ok_clear = True
            z = dd64[j][px] / a64[j][px]
            X = [o64[px][i] + z * d64[px][i] for i in range(3)]
            q = [X[i] - L[i] for i in range(3)]
            rho = math.sqrt(_dot(q, q)) if _dot(q, q) == _dot(q, q) else NAN
            X_all[j, px], rho_all[j, px] = X, rho
            sh = one
            for k in range(K):
                M = M64[k]
                x = [((M[i][0] * X[0] + M[i][1] * X[1]) + M[i][2] * X[2]) + M[i][3] for i in range(3)]
                zl = x[2]
                abar = np.float32(0.0)
                if _near(zl, near):
                    ok_clear = False
                if zl > near:
                    u, v = x[0] / zl, x[1] / zl
                    uv[j, k, px] = (u, v)
                    for w in (u, v):
                        if _near(w, 0.0, 1.0) or _near(w, hi, max(1.0, hi)):
                            ok_clear = False
                    if 0.0 <= u <= hi and 0.0 <= v <= hi:
                        inside[j, k, px] = True
                        bias = bias_self if k == j else bias_other
                        total = 0.0
                        for dy in range(-r, r + 1):
                            ty = (v + float(dy)) + 0.5
                            yi = int(min(max(math.floor(ty), 0.0), hi))
                            if _near(ty, float(round(ty)), max(1.0, abs(ty))):
                                ok_clear = False
                            for dx in range(-r, r + 1):
                                tx = (u + float(dx)) + 0.5
                                xi = int(min(max(math.floor(tx), 0.0), hi))
                                if _near(tx, float(round(tx)), max(1.0, abs(tx))):
                                    ok_clear = False
                                m, s = ma64[k][yi][xi], md64[k][yi][xi]
                                if m > 0.0:
                                    rhs = (rho - bias) * m
                                    if s < rhs:
                                        total += m
                                    if s == s and rhs == rhs and abs(s - rhs) <= EPS * max(abs(s), abs(rho * m)):
                                        ok_clear = False
                        abar = np.float32(total / taps)
                abar_all[j, k, px] = abar
                with np.errstate(all="ignore"):
                    sh = np.float32(sh * np.float32(one - np.float32(strength * abar)))
            g = np.float32(0.0)
            if n64 is not None:
                n = n64[j][px]
                if any(t != 0.0 for t in n) and all(math.isfinite(t) for t in n):
                    l = [L[i] - X[i] for i in range(3)]
                    ll = _dot(l, l)
                    if ll == ll and ll > 0.0:
                        cosv = _dot(n, l) / math.sqrt(ll)
                    else:
                        cosv = NAN                                      # 0 / 0, or NaN in the rays
                    if cosv == cosv:
                        cosv_all[j, px] = cosv
                        t = (cosv - cos0) / dcos
                        f = min(max(t, 0.0), 1.0)
                        g = np.float32(1.0 - f)
                        if abs(cosv - cos0) <= EPS or abs(cosv - cos1) <= EPS:
                            ok_clear = False
            g_all[j, px] = g
            with np.errstate(all="ignore"):
                sh = np.float32(sh * np.float32(one - np.float32(strength * g)))
                shade[j, px] = sh
                c_out[j, px] = c[j, px] * sh
            clear[j, px] = ok_clear
    return dict(shade=shade, c_out=c_out, receives=receives, clear=clear, abar=abar_all, cosv=cosv_all, g=g_all, X=X_all, rho=rho_all,
                uv=uv, inside=inside)
