"""Float64 restatements of the SMPL body-model entries of the C ABI -- ia_smpl_lbs_fwd / ia_smpl_lbs_bwd (csrc/ia_smpl_lbs.hip)
and ia_smpl_tfs / ia_smpl_tfs_bwd (csrc/ia_snarf.hip) -- with the seeded inputs and the per-group error bound that
tests/test_gpu_smpl_kernels.py holds the kernels to and tests/test_cpu_smpl_refs.py validates on the CPU.  numpy only, no
product import; every reference takes the arrays the C entry takes.

What is restated (include/instantavatar_hip.h; the header comment of ia_smpl_lbs.hip), not how the kernels schedule it:

    J        = J0 + JS beta                                                           (lbs.py:185-190, regressor folded)
    R_j      = I + sin(a) K + (1 - cos a) K^2,  a = |theta_j + 1e-8f|,  K = hat(theta_j / a)              (lbs.py:295-329)
    G_0      = [R_0 | J_0],  G_i = G_parent(i) [R_i | J_i - J_parent(i)]                                 (lbs.py:345-401)
    A_j      = Tr(transl) G_j Tr(-J_j)                                            (lbs.py:396-399, body_models.py:353-357)
    po       = vec(R_1..23 - I) . posedirs,  vs = v_template + shapedirs beta,  T_v = sum_j w_vj A_j      (lbs.py:211-230)
    s2w      = A_0,  w2s = s2w^-1,  M_v = T_v^-1 s2w  with  M_v.t += po_t[v] - po[v],  T_inv[v] = T_t[v] M_v
    verts[v] = w2s T_v (vs + po),  verts_t[v] = T_t[v] (vs + po_t)                                 (smpl_deformer.py:66-76)
    tfs_j    = w2s A_j B_j,  B = tfs_inv_t                                                        (snarf_deformer.py:79-86)

All matrices are 4 x 4 homogeneous here (the kernels carry 3 x 4 blocks); a product with the constant row (0, 0, 0, 1) adds
exact zeros, so in either precision the arithmetic is that of the blocks.

The backward is derived on the 4 x 4 matrices, for L = <D, T_inv> + <D_w, w2s> (rows 0..2 of D are read).  With P(X) = X with
its fourth row zeroed (the fourth row of an affine matrix is a constant, nothing flows into it):

    T_inv = T_t M          dT_t = P(D M^T),  dM = P(T_t^T D),  d po[v] = -dM[:3, 3]
    M     = T^-1 S + ..    dTi = P(dM S^T),  dS += P(Ti^T dM),  dT = -P(Ti^T dTi Ti^T)
    w2s   = S^-1           dS += -P(W^T D_w W^T)
    T     = sum_j w A_j    dA_j = sum_v w_vj dT_v,  dA_t,j = sum_v w_vj dT_t,v,  dA_0 += dS,  d pf = posedirs . d po
    A_j   = Tr G_j C_j     d transl = sum_j dA_j[:3, 3],  dG_j = P(dA_j C_j^T),  dJ_j -= (G_j^T dA_j)[:3, 3]      (C_j = Tr(-J_j))
    G_i   = G_p L_i        (children first)  dG_p += P(dG_i L_i^T),  dL_i = P(G_p^T dG_i),  dL_0 = dG_0
    L_i   = [R_i | J_i - J_p]   dR_i = dL_i[:3, :3] (+ d pf's block for the posed chain, i >= 1),  dJ_i += dL_i[:3, 3],  dJ_p -= ...
    R(theta)   with K^2 = d d^T - (d.d) I (d = theta / a is not a unit vector), ax(X) = (X21 - X12, X02 - X20, X10 - X01):
                   g_d = sin(a) ax(dR) + (1 - cos a) ((dR + dR^T) d - 2 tr(dR) d)
                   g_a = cos(a) d.ax(dR) + sin(a) (d^T dR d - (d.d) tr dR)
                   d theta = g_d / a + (g_a - g_d.theta / a^2) (theta + 1e-8f) / a
    beta           d beta = JS^T dJ            (T_inv does not depend on vs: the shape offsets of the two bodies cancel)

The bound, per output group g (forward: rotation block and translation block of T_inv / w2s / tfs / A, verts, verts_t;
backward: d_pose of each joint, d_betas, d_transl):

    allow(g) = K . max( E32(g), u . M(g) ),     u = 2^-24

E32 is the max-norm difference between this reference evaluated op by op in float32 and in float64 on the same case, M the
group's condition magnitude: for a sum, the same sum with every term replaced by its absolute value, the terms being the real
float64 intermediates -- one level per reduction, nothing compounds (lbs_bwd_ref lists them: sum_v |w| |dT| for d_A_j, likewise
d_pf, d_S, d_transl; sum |JS| |dJ| for d_betas; for d_pose of a joint the absolute terms of its final assembly from the real
dA / dS / dpf and the real dG of its children); for a forward output the largest |entry| of the group.  E32 governs wherever
it is the larger, which is in about half of the backward groups (E32 / u M runs from 0.1 to 1.8 at V = 6 890).  K covers the
kernels evaluating the same real expressions in another association (the 256-lane tree over the
vertices against numpy's sums, lane-per-element chains, Gauss-Jordan against the cofactor inverse).  Nothing in the bound
comes from a kernel's output.  d_transl of ia_smpl_tfs_bwd, and of ia_smpl_lbs_bwd without d_w2s, is analytically zero (the
translation cancels in w2s . A and in T^-1 . s2w): there the bound is the floor K . u . M alone.

The skinning weights of the seeded bodies are multiples of 2^-10 that sum to 1 exactly: with rows that sum to 1 only up to
fp32 rounding, the float64 d_transl of the cancelling cases is 1e-8 . M, not zero, and that case could not be asserted.

measured (MI355X, tests/test_gpu_smpl_kernels.py with K = 8): kernel_error / (allow / K) of every case and group; the fourth
rows of all matrix outputs are exact everywhere.  "-d_w2s" is the rerun of a case without d_w2s.
    lbs_fwd         chain-same-257     T_inv.R 0.77  T_inv.t 0.81  w2s.R 0.71  w2s.t 1.07  verts 1.00  verts_t 1.17
    lbs_fwd         chain-zero-255     T_inv.R 0.62  T_inv.t 1.00  w2s.R 0.00  w2s.t 0.00  verts 1.00  verts_t 1.00
    lbs_fwd         smpl-bigroot-6890  T_inv.R 1.05  T_inv.t 1.17  w2s.R 1.00  w2s.t 1.00  verts 1.23  verts_t 0.95
    lbs_fwd         smpl-extreme-255   T_inv.R 0.91  T_inv.t 1.09  w2s.R 1.00  w2s.t 0.84  verts 1.00  verts_t 0.75
    lbs_fwd         smpl-mixed-6890    T_inv.R 1.03  T_inv.t 0.94  w2s.R 0.97  w2s.t 0.81  verts 0.65  verts_t 0.99
    lbs_fwd         smpl-random-257    T_inv.R 0.95  T_inv.t 2.08  w2s.R 0.70  w2s.t 1.33  verts 0.71  verts_t 1.18
    lbs_fwd         star-hand-257      T_inv.R 0.99  T_inv.t 1.03  w2s.R 1.00  w2s.t 1.00  verts 1.00  verts_t 1.00
    lbs_fwd         star-mixed-1       T_inv.R 0.79  T_inv.t 1.52  w2s.R 1.00  w2s.t 0.73  verts 1.51  verts_t 0.43
    lbs_bwd         chain-same-257     d_pose[0..23] 0.36 0.34 0.53 1.01 0.59 0.36 0.47 0.43 0.52 0.84 0.54 0.50 0.50 0.52 0.49 0.73 1.00 0.67 1.71 1.31 1.65 0.62 1.62 0.93  d_transl 0.08  d_betas 1.16
    lbs_bwd -d_w2s  chain-same-257     d_pose[0..23] 0.48 0.34 0.53 1.01 0.59 0.36 0.47 0.43 0.52 0.84 0.54 0.50 0.50 0.52 0.49 0.73 1.00 0.67 1.71 1.31 1.65 0.62 1.62 0.93  d_transl 0.00  d_betas 1.09
    lbs_bwd         chain-zero-255     d_pose[0..23] 0.80 0.54 0.65 0.95 0.95 0.70 0.17 0.39 0.36 0.35 0.55 0.21 0.34 0.18 0.47 1.43 0.53 0.91 0.90 1.22 0.55 0.32 0.59 0.92  d_transl 0.21  d_betas 1.00
    lbs_bwd         smpl-bigroot-6890  d_pose[0..23] 0.11 0.27 0.34 0.24 0.35 0.23 0.25 0.45 0.07 0.33 0.32 0.62 0.41 0.08 0.17 0.93 0.20 0.17 0.21 0.16 0.54 0.17 0.49 1.25  d_transl 0.04  d_betas 0.83
    lbs_bwd         smpl-extreme-255   d_pose[0..23] 0.23 0.25 0.21 0.30 0.33 0.04 0.58 0.21 0.15 0.62 0.34 0.43 0.14 0.20 0.29 0.21 0.36 0.21 0.22 0.71 0.17 0.17 0.33 0.46  d_transl 0.51  d_betas 1.61
    lbs_bwd         smpl-mixed-6890    d_pose[0..23] 0.20 0.16 0.17 0.39 0.24 0.45 0.27 1.23 0.39 0.26 0.98 0.55 0.66 0.51 0.78 0.49 0.34 0.34 0.14 0.20 1.03 1.61 0.85 2.12  d_transl 0.08  d_betas 1.00
    lbs_bwd -d_w2s  smpl-mixed-6890    d_pose[0..23] 0.18 0.16 0.17 0.39 0.24 0.45 0.27 1.23 0.39 0.26 0.98 0.55 0.66 0.51 0.78 0.49 0.34 0.34 0.14 0.20 1.03 1.61 0.85 2.12  d_transl 0.06  d_betas 0.66
    lbs_bwd         smpl-random-257    d_pose[0..23] 0.13 0.32 0.20 0.27 0.29 0.24 0.18 0.27 0.25 0.43 0.40 0.36 0.20 0.26 0.44 0.27 0.35 0.43 0.08 0.35 0.17 0.20 0.32 0.70  d_transl 0.18  d_betas 1.05
    lbs_bwd -d_w2s  smpl-random-257    d_pose[0..23] 0.15 0.32 0.20 0.27 0.29 0.24 0.18 0.27 0.25 0.43 0.40 0.36 0.20 0.26 0.44 0.27 0.35 0.43 0.08 0.35 0.17 0.20 0.32 0.70  d_transl 0.23  d_betas 0.86
    lbs_bwd         star-hand-257      d_pose[0..23] 0.10 0.15 0.06 0.15 0.83 0.21 0.29 0.06 0.18 0.54 0.88 0.13 0.62 0.38 0.19 0.10 0.33 0.14 0.11 0.67 0.12 0.25 0.17 0.19  d_transl 0.00  d_betas 2.83
    lbs_bwd         star-mixed-1       d_pose[0..23] 0.24 0.19 0.37 0.34 0.66 0.17 0.63 0.90 0.36 0.47 1.38 0.93 0.75 0.12 0.25 0.26 0.38 0.38 0.64 0.38 0.67 0.48 0.74 0.43  d_transl 1.00  d_betas 1.00
    lbs_bwd -d_w2s  star-mixed-1       d_pose[0..23] 0.22 0.19 0.37 0.34 0.66 0.17 0.63 0.90 0.36 0.47 1.38 0.93 0.75 0.12 0.25 0.26 0.38 0.38 0.64 0.38 0.67 0.48 0.74 0.43  d_transl 0.00  d_betas 1.00
    tfs             chain-bigroot      tfs.R 1.16  tfs.t 0.94  w2s.R 0.79  w2s.t 0.64  A.R 1.33  A.t 1.00
    tfs_bwd         chain-bigroot      d_pose[0..23] 0.15 0.12 0.25 0.24 0.31 0.36 0.75 0.13 0.27 0.41 0.16 0.33 0.16 0.15 0.08 0.37 0.25 0.27 0.60 0.29 0.10 0.56 0.60 0.59  d_transl 0.74
    tfs             chain-zero         tfs.R 0.00  tfs.t 1.00  w2s.R 0.00  w2s.t 0.00  A.R 0.00  A.t 1.00
    tfs_bwd         chain-zero         d_pose[0..23] 1.00 1.01 1.00 1.00 1.00 1.00 0.66 1.17 0.99 0.73 0.28 0.30 0.27 0.27 0.46 0.83 1.06 1.17 0.78 0.71 0.38 0.56 0.74 0.69  d_transl 0.61
    tfs             smpl-extreme       tfs.R 1.10  tfs.t 0.84  w2s.R 1.48  w2s.t 1.38  A.R 0.83  A.t 0.77
    tfs_bwd         smpl-extreme       d_pose[0..23] 0.40 0.00 0.00 0.26 0.00 0.00 0.47 0.00 0.00 0.36 0.00 0.00 0.00 0.17 0.00 0.00 0.09 0.00 0.23 0.00 0.34 0.00 0.27 0.00  d_transl 0.00
    tfs             smpl-random        tfs.R 1.09  tfs.t 0.92  w2s.R 1.50  w2s.t 0.36  A.R 0.81  A.t 0.94
    tfs_bwd         smpl-random        d_pose[0..23] 0.13 0.08 0.16 0.70 0.24 0.28 0.20 0.12 0.30 0.08 0.12 0.17 0.34 0.15 0.13 0.17 0.17 0.08 0.28 0.22 0.15 0.28 0.62 0.22  d_transl 0.53
    tfs             star-mixed         tfs.R 1.76  tfs.t 1.00  w2s.R 0.95  w2s.t 1.00  A.R 1.00  A.t 1.00
    tfs_bwd         star-mixed         d_pose[0..23] 0.05 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 0.00 1.02  d_transl 0.00
The largest per entry: ia_smpl_lbs_fwd 2.08 (T_inv.t of smpl-random-257), ia_smpl_lbs_bwd 2.83 (d_betas of star-hand-257; 2.12
for d_pose[23] of smpl-mixed-6890), ia_smpl_tfs 1.76 (tfs.R of star-mixed), ia_smpl_tfs_bwd 1.17 (d_pose[17] of chain-zero).
Where a ratio is exactly 1.00 the kernel and the float32 evaluation of this file round alike.  The largest ratio is 2.83, so
K = 8 is the smallest power of two that leaves a factor 2 above it (4 would leave 1.4) and stays.
"""
import functools

import numpy as np

U = 2.0 ** -24
#: the largest measured kernel_error / (allow / K) per entry (see the docstring); K_BOUND >= 2 x the largest of them
MEASURED = {"ia_smpl_lbs_fwd": 2.08, "ia_smpl_lbs_bwd": 2.83, "ia_smpl_tfs": 1.76, "ia_smpl_tfs_bwd": 1.17}
K_BOUND = 8
EPS32 = np.float32(1e-8)
N_J = 24
SMPL_PARENTS = np.array([-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21], np.int32)
HAND = 22          # a leaf joint of SMPL's table (left hand)
ROW3_FILL = 1e30   # the fourth row of every upstream-gradient matrix: large, finite, never read
BODY_KEYS = ("v_template", "shapedirs", "posedirs", "lbs_weights", "J0", "JS", "parents")


# ---- 4 x 4 helpers, every operation in the dtype of its operands -------------------------------------------------------
def _mm(X, Y):
    out = X[..., :, 0, None] * Y[..., 0, None, :]
    for k in range(1, X.shape[-1]):
        out = out + X[..., :, k, None] * Y[..., k, None, :]
    return out


def _t(X):
    return np.swapaxes(X, -1, -2)


def _P(X):
    X = np.array(X)
    X[..., 3, :] = 0
    return X


def _affine(R, t):
    X = np.zeros(R.shape[:-2] + (4, 4), R.dtype)
    X[..., :3, :3], X[..., :3, 3], X[..., 3, 3] = R, t, 1
    return X


def _apply(X, p):
    return X[..., :3, 0] * p[..., 0, None] + X[..., :3, 1] * p[..., 1, None] + X[..., :3, 2] * p[..., 2, None] + X[..., :3, 3]


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _affine_inv(X):
    """[R | t]^-1 = [R^-1 | -R^-1 t], R^-1 = adj(R) / det(R)"""
    R, t = X[..., :3, :3], X[..., :3, 3]
    r0, r1, r2 = R[..., 0, :], R[..., 1, :], R[..., 2, :]
    c0, c1, c2 = np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)
    det = _dot3(r0, c0)[..., None]
    Ri = np.stack([c0 / det, c1 / det, c2 / det], -1)
    ti = -(Ri[..., :, 0] * t[..., 0, None] + Ri[..., :, 1] * t[..., 1, None] + Ri[..., :, 2] * t[..., 2, None])
    return _affine(Ri, ti)


def _hat(d):
    K = np.zeros(d.shape[:-1] + (3, 3), d.dtype)
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -d[..., 2], d[..., 1], d[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -d[..., 0], -d[..., 1], d[..., 0]
    return K


def _vsum(x, reverse=False):
    """sum over the leading (vertex) axis, made the contiguous last one"""
    if reverse:
        x = x[::-1]
    return np.ascontiguousarray(np.moveaxis(x, 0, -1)).sum(-1)


def _tap(tap, name, x, idx=None):
    return x if tap is None else tap(name, x, idx)


# ---- forward pieces ----------------------------------------------------------------------------------------------------
def _rodrigues(theta, dt):
    th = np.asarray(theta).reshape(N_J, 3).astype(dt)
    e = dt(EPS32)
    a = th + e
    ang = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])
    d = th / ang[:, None]
    K = _hat(d)
    s, c = np.sin(ang), np.cos(ang)
    omc = dt(1) - c
    R = np.eye(3, dtype=dt) + s[:, None, None] * K + omc[:, None, None] * _mm(K, K)
    return dict(th=th, the=a, ang=ang, d=d, s=s, c=c, omc=omc, R=R)


def _chain(R, J, parents, transl, assoc):
    dt = R.dtype
    rel = J.copy()
    rel[1:] = J[1:] - J[parents[1:]]
    L = _affine(R, rel)
    G = np.zeros_like(L)
    G[0] = L[0]
    for i in range(1, N_J):
        if assoc == "root":          # from the root down, as lbs.py does
            G[i] = _mm(G[parents[i]], L[i])
        else:                        # the same product associated from the leaf up
            acc, q = L[i], parents[i]
            while q >= 0:
                acc, q = _mm(L[q], acc), parents[q]
            G[i] = acc
    C = _affine(np.broadcast_to(np.eye(3, dtype=dt), (N_J, 3, 3)), -J)
    A = _mm(G, C)
    if transl is not None:
        A[:, :3, 3] = A[:, :3, 3] + transl
    return L, G, C, A


def _cast_body(body, dt):
    b = {k: np.asarray(body[k]).astype(dt) for k in BODY_KEYS[:-1]}
    b["parents"] = np.asarray(body["parents"]).astype(np.int64)
    assert (b["parents"][1:] < np.arange(1, N_J)).all() and (b["parents"][1:] >= 0).all()
    return b


def lbs_fwd_ref(body, betas, pose, transl, pose_t, po_t, dtype=np.float64, assoc="root"):
    """ia_smpl_lbs_fwd: -> dict with T_inv [V,4,4], verts [V,3], verts_t [V,3], w2s [4,4] and the intermediates the backward
    needs.  body: dict of the ia_smpl_body arrays (BODY_KEYS).  dtype=np.float32 evaluates the same expressions op by op in
    float32; assoc="leaf" is the equally valid second association of the chain products (from the leaf up)."""
    dt = dtype
    b = _cast_body(body, dt)
    V = b["v_template"].shape[0]
    betas, po_t = np.asarray(betas).reshape(10).astype(dt), np.asarray(po_t).reshape(V, 3).astype(dt)
    tr = None if transl is None else np.asarray(transl).reshape(3).astype(dt)
    J = b["J0"] + (b["JS"] * betas).sum(-1)
    rod, rod_t = _rodrigues(pose, dt), _rodrigues(pose_t, dt)
    L, G, Cm, A = _chain(rod["R"], J, b["parents"], tr, assoc)
    Lt, Gt, _, At = _chain(rod_t["R"], J, b["parents"], None, assoc)
    S = A[0].copy()
    W = _affine_inv(S)
    pf = (rod["R"][1:] - np.eye(3, dtype=dt)).reshape(207)
    po = (pf @ b["posedirs"]).reshape(V, 3)
    so = (b["shapedirs"] * betas).sum(-1)
    vs = b["v_template"] + so
    w = b["lbs_weights"]
    T, Tt = np.tensordot(w, A, 1), np.tensordot(w, At, 1)
    T[:, 3], Tt[:, 3] = (0, 0, 0, 1), (0, 0, 0, 1)
    Ti = _affine_inv(T)
    M = _mm(Ti, S)
    M[:, :3, 3] = M[:, :3, 3] + (po_t - po)
    T_inv = _mm(Tt, M)
    x = _apply(T, vs + po)
    return dict(T_inv=T_inv, verts=_apply(W, x), verts_t=_apply(Tt, vs + po_t), w2s=W,
                J=J, rod=rod, rod_t=rod_t, L=L, G=G, C=Cm, A=A, Lt=Lt, Gt=Gt, At=At, S=S, W=W, pf=pf, po=po, so=so, vs=vs, T=T, Tt=Tt,
                Ti=Ti, M=M, x_world=x, joints_posed=G[:, :3, 3] + (0 if tr is None else tr))


# ---- backward pieces -----------------------------------------------------------------------------------------------------
def _rodrigues_bwd(r, dR, sgn=-1, tap=None):
    """dR [24,3,3] -> d theta [24,3].  sgn = +1 with |r| and |dR|: the same assembly with every term replaced by its absolute
    value (each subtraction an addition)"""
    num = _tap(tap, "dir_numerator", r["th"])
    d = r["d"] if num is r["th"] else num / r["ang"][:, None]
    ang, s, c, omc = r["ang"][:, None], r["s"][:, None], r["c"][:, None], r["omc"][:, None]
    ax = np.stack([dR[:, 2, 1] + sgn * dR[:, 1, 2], dR[:, 0, 2] + sgn * dR[:, 2, 0], dR[:, 1, 0] + sgn * dR[:, 0, 1]], -1)
    Sy = dR + _t(dR)
    tr = (dR[:, 0, 0] + dR[:, 1, 1] + dR[:, 2, 2])[:, None]
    Sd = Sy[:, :, 0] * d[:, 0, None] + Sy[:, :, 1] * d[:, 1, None] + Sy[:, :, 2] * d[:, 2, None]
    Rd = dR[:, :, 0] * d[:, 0, None] + dR[:, :, 1] * d[:, 1, None] + dR[:, :, 2] * d[:, 2, None]
    g_d = s * ax + omc * (Sd + sgn * (2 * tr * d))
    g_a = c * _dot3(d, ax)[:, None] + s * (_dot3(d, Rd)[:, None] + sgn * (_dot3(d, d)[:, None] * tr))
    return g_d / ang + (g_a + sgn * (_dot3(g_d, r["th"])[:, None] / (ang * ang))) * r["the"] / ang


def _chain_bwd(dA, L, G, Cm, parents, tap=None, m_dA=None):
    """dA [24,4,4] -> dL [24,4,4] (gradient of the local transforms), dJ [24,3], m_dL: per joint the sums that assemble dL_i
    -- dG_i = dA_i C_i^T + sum over the children c of dG_c L_c^T, then G_p^T dG_i -- with each term replaced by its absolute
    value, the terms themselves (dA_i, dG_c) being the real ones: one level, nothing compounds along the chain.  m_dA: |dA|
    where a caller knows dA_i as a sum of its own (the root: vertices + s2w paths)."""
    dG = _P(_mm(dA, _t(Cm)))
    m_dG = _P(_mm(np.abs(dA) if m_dA is None else m_dA, np.abs(_t(Cm))))
    dJ = _tap(tap, "dJ_from_A", -_mm(_t(G), dA)[:, :3, 3])
    dL, m_dL = np.zeros_like(dG), np.zeros_like(dG)
    for i in range(N_J - 1, 0, -1):
        p = parents[i]
        dG[p] = dG[p] + _tap(tap, "dG_to_parent", _P(_mm(dG[i], _t(L[i]))), i)
        m_dG[p] = m_dG[p] + _P(_mm(np.abs(dG[i]), np.abs(_t(L[i]))))
        dL[i] = _P(_mm(_t(G[p]), dG[i]))
        m_dL[i] = _P(_mm(np.abs(_t(G[p])), m_dG[i]))
        dJ[i] = dJ[i] + dL[i, :3, 3]
        dJ[p] = dJ[p] - dL[i, :3, 3]
    dL[0], m_dL[0] = dG[0], m_dG[0]
    dJ[0] = dJ[0] + dL[0, :3, 3]
    return dL, dJ, m_dL


def _abs_rod(r):
    return {k: np.abs(v) for k, v in r.items()}


def _upstream(D, dt):
    return _P(np.asarray(D).astype(dt))


def lbs_bwd_ref(body, betas, pose, transl, pose_t, po_t, d_T_inv, d_w2s, dtype=np.float64, assoc="root", reverse=False, tap=None):
    """ia_smpl_lbs_bwd: -> dict with d_betas [10], d_pose [72], d_transl [3] and the condition magnitudes: each output that is
    a sum, again with every term replaced by its absolute value, the terms being this evaluation's real intermediates (one
    level, per reduction):
        m_dA[j] = sum_v |w_vj| |dT_v|,  m_dAt,  m_dS = sum_v |dS_v| (+ |the w2s path|),  m_dpf = |posedirs| . |d po|
        m_d_transl = sum_j m_dA[j][:3, 3] + m_dS[:3, 3]          m_d_betas = sum |JS| |dJ|
        m_d_pose   = Rodrigues' backward assembled from absolute terms, on |G_p^T| m_dG_j + |d pf_j| (see _chain_bwd; the
                     root's dA_0 enters as |sum_v w dT| + |sum_v dS_v| + |w2s path|)
    reverse=True takes the vertex sums in reversed order.  `tap(name, array, index)` may edit a named intermediate (tests
    seed defects through it)."""
    dt = dtype
    F = lbs_fwd_ref(body, betas, pose, transl, pose_t, po_t, dt, assoc)
    b = _cast_body(body, dt)
    D = _upstream(d_T_inv, dt)
    Dw = None if d_w2s is None else _upstream(d_w2s, dt)
    V = D.shape[0]
    dTt = _P(_mm(D, _t(F["M"])))
    dM = _P(_mm(_t(F["Tt"]), D))
    dpo = -dM[:, :3, 3]
    dTi = _P(_mm(dM, _t(F["S"])))
    dSv = _P(_mm(_t(F["Ti"]), dM))
    dT = _tap(tap, "dT", -_P(_mm(_mm(_t(F["Ti"]), dTi), _t(F["Ti"]))))
    w = b["lbs_weights"]
    dA = _vsum(w[:, :, None, None] * dT[:, None], reverse)
    dAt = _vsum(w[:, :, None, None] * dTt[:, None], reverse)
    dS = _vsum(dSv, reverse)
    pd = b["posedirs"].reshape(207, V, 3)
    dpf = (pd[:, ::-1].reshape(207, -1) @ dpo[::-1].reshape(-1)) if reverse else b["posedirs"] @ dpo.reshape(-1)
    dpf = _tap(tap, "dpf", dpf)
    m_dA, m_dAt = _vsum(w[:, :, None, None] * np.abs(dT)[:, None]), _vsum(w[:, :, None, None] * np.abs(dTt)[:, None])
    m_dS, m_dpf = _vsum(np.abs(dSv)), np.abs(b["posedirs"]) @ np.abs(dpo).reshape(-1)
    m_root = np.abs(dA[0]) + np.abs(dS)
    if Dw is not None:
        dSw = _tap(tap, "dS_w2s", -_P(_mm(_mm(_t(F["W"]), Dw), _t(F["W"]))))
        dS, m_dS, m_root = dS + dSw, m_dS + np.abs(dSw), m_root + np.abs(dSw)
    dA[0] = dA[0] + dS
    d_transl = dA[:, :3, 3].sum(0)
    m_in = np.abs(dA)
    m_in[0] = m_root
    dL, dJ, m_dL = _chain_bwd(dA, F["L"], F["G"], F["C"], b["parents"], tap, m_in)
    _, dJt, _ = _chain_bwd(dAt, F["Lt"], F["Gt"], F["C"], b["parents"], tap)
    dJ = dJ + dJt
    dR, m_dR = dL[:, :3, :3].copy(), m_dL[:, :3, :3].copy()
    dR[1:] = dR[1:] + dpf.reshape(23, 3, 3)
    m_dR[1:] = m_dR[1:] + np.abs(dpf).reshape(23, 3, 3)
    return dict(d_pose=_rodrigues_bwd(F["rod"], dR, -1, tap).reshape(72), d_betas=(b["JS"] * dJ[:, :, None]).sum((0, 1)), d_transl=d_transl,
                m_d_pose=_rodrigues_bwd(_abs_rod(F["rod"]), m_dR, +1).reshape(72), m_d_betas=(np.abs(b["JS"]) * np.abs(dJ)[:, :, None]).sum((0, 1)),
                m_d_transl=m_dA[:, :3, 3].sum(0) + m_dS[:3, 3], m_dA=m_dA, m_dAt=m_dAt, m_dS=m_dS, m_dpf=m_dpf, dJ=dJ)


def tfs_fwd_ref(joints_rest, parents, pose, transl, tfs_inv_t, dtype=np.float64, assoc="root"):
    """ia_smpl_tfs: -> dict with tfs [24,4,4], w2s [4,4], A [24,4,4] and the intermediates"""
    dt = dtype
    J = np.asarray(joints_rest).reshape(N_J, 3).astype(dt)
    par = np.asarray(parents).astype(np.int64)
    B = np.asarray(tfs_inv_t).reshape(N_J, 4, 4).astype(dt)
    tr = None if transl is None else np.asarray(transl).reshape(3).astype(dt)
    rod = _rodrigues(pose, dt)
    L, G, Cm, A = _chain(rod["R"], J, par, tr, assoc)
    W = _affine_inv(A[0])
    return dict(tfs=_mm(_mm(W, A), B), w2s=W, A=A, rod=rod, L=L, G=G, C=Cm, W=W, B=B, parents=par)


def tfs_bwd_ref(joints_rest, parents, pose, transl, tfs_inv_t, d_tfs, dtype=np.float64, assoc="root", tap=None):
    """ia_smpl_tfs_bwd: -> dict with d_pose [72], d_transl [3] (analytically zero), m_d_pose, m_d_transl: as lbs_bwd_ref, with
    dA_j = W^T E_j and the root's dA_0 entering as |W^T E_0| + |W^T dW W^T|;  m_d_transl = sum_j |dA_j[:3, 3]| over those terms"""
    F = tfs_fwd_ref(joints_rest, parents, pose, transl, tfs_inv_t, dtype, assoc)
    D = _upstream(d_tfs, dtype)
    E = _mm(D, _t(F["B"]))
    dA = _P(_mm(_t(F["W"]), E))
    dW = _P(_mm(E, _t(F["A"])).sum(0))
    back = _P(_mm(_mm(_t(F["W"]), dW), _t(F["W"])))
    m_in = np.abs(dA)
    m_in[0] = m_in[0] + np.abs(back)
    dA[0] = dA[0] - back
    dL, _, m_dL = _chain_bwd(dA, F["L"], F["G"], F["C"], F["parents"], tap, m_in)
    return dict(d_pose=_rodrigues_bwd(F["rod"], dL[:, :3, :3], -1, tap).reshape(72), d_transl=dA[:, :3, 3].sum(0),
                m_d_pose=_rodrigues_bwd(_abs_rod(F["rod"]), m_dL[:, :3, :3], +1).reshape(72), m_d_transl=m_in[:, :3, 3].sum(0))


# ---- seeded inputs -----------------------------------------------------------------------------------------------------
def parents_table(kind):
    if kind == "smpl":
        return SMPL_PARENTS.copy()
    p = np.arange(-1, N_J - 1, dtype=np.int32) if kind == "chain" else np.zeros(N_J, np.int32)
    p[0] = -1
    return p


def make_body(V, kind, seed=0, hot=None):
    """synthetic body tables at the scales of tests/golden/make_lbs_golden.py: shapedirs ~0.02, posedirs ~0.01, dense JS; every
    vertex is weighted to 1..4 joints (a joint and its ancestors, the joint itself with at least 5/8), weights are multiples of
    2^-10 that sum to 1 exactly.  hot = (vertex, joint): that vertex is weighted to that joint alone."""
    g = np.random.default_rng(1000 + seed)
    par = parents_table(kind)
    w = np.zeros((V, N_J), np.float32)
    for v in range(V):
        j = int(g.integers(N_J))
        js = [j]
        while par[js[-1]] >= 0 and len(js) < 4:
            js.append(int(par[js[-1]]))
        if j == 0:
            js = [0, 1, 2, 3]
        js = js[:int(g.integers(1, len(js) + 1))]
        rest = 384
        for q in js[1:]:
            k = int(g.integers(1, rest // 2 + 1))
            w[v, q] = k / 1024.0
            rest -= k
        w[v, j] = 1.0 - w[v].sum()
    if hot is not None:
        w[hot[0]] = 0
        w[hot[0], hot[1]] = 1.0
    assert (w.astype(np.float64).sum(1) == 1.0).all() and (w >= 0).all() and ((w > 0).sum(1) <= 4).all()
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    return dict(v_template=f(V, 3) * np.float32(0.4), shapedirs=f(V, 3, 10) * np.float32(0.02), posedirs=f(207, V * 3) * np.float32(0.01),
                lbs_weights=w, J0=f(N_J, 3) * np.float32(0.3), JS=f(N_J, 3, 10) * np.float32(0.02), parents=par)


def _axis_angle(g, n, lo, hi):
    d = g.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * g.uniform(lo, hi, (n, 1))


ZERO_JOINTS = (7, 8, 10, 11, 20, 21, 22, 23)     # feet, toes, wrists, hands: what a real fit leaves at exactly zero


def make_pose(kind, seed=0):
    """-> (pose [72], transl [3] or None by the caller's choice: see LBS_CASES).  kinds: random (|theta| in 0.1..1.2), zero, mixed
    (ZERO_JOINTS exactly 0), extreme (joint 5 at pi - 1e-3, joint 16 at 4.0), bigroot (root at 2.5)"""
    g = np.random.default_rng(2000 + seed)
    p = _axis_angle(g, N_J, 0.1, 1.2)
    if kind == "zero":
        p[:] = 0.0
    elif kind == "mixed":
        p[list(ZERO_JOINTS)] = 0.0
    elif kind == "extreme":
        p[5] *= (np.pi - 1e-3) / np.linalg.norm(p[5])
        p[16] *= 4.0 / np.linalg.norm(p[16])
    elif kind == "bigroot":
        p[0] *= 2.5 / np.linalg.norm(p[0])
    else:
        assert kind in ("random", "same")
    return p.reshape(72).astype(np.float32)


def template_pose():
    """the product's template: legs apart (smpl_deformer.py:33-35)"""
    p = np.zeros(72, np.float32)
    p[3 + 2], p[3 + 5] = np.pi / 6, -np.pi / 6
    return p


def pose_offsets_f32(body, pose):
    """po_t as the product hands it over: the template pose's pose blend, an fp32 array"""
    R = _rodrigues(pose, np.float64)["R"]
    return ((R[1:] - np.eye(3)).reshape(207) @ body["posedirs"].astype(np.float64)).reshape(-1, 3).astype(np.float32)


def make_upstream(n, kind, seed=0, hot=0):
    """upstream gradient [n,4,4]: dense (both signs, magnitudes over ten binades), onehot (matrix `hot` only), last (the last
    matrix only); the fourth row of EVERY matrix holds ROW3_FILL"""
    g = np.random.default_rng(3000 + seed)
    D = (g.standard_normal((n, 4, 4)) * 2.0 ** g.integers(-6, 4, (n, 4, 4))).astype(np.float32)
    keep = np.ones(n, bool) if kind == "dense" else np.arange(n) == (hot if kind == "onehot" else n - 1)
    assert kind in ("dense", "onehot", "last")
    D[~keep] = 0
    D[:, 3] = ROW3_FILL
    return D


#: name: (V, parents, pose, betas non-zero, transl: None | "small" | "large", upstream, d_w2s present)
LBS_CASES = {
    "smpl-random-257":    (257, "smpl", "random", True, "small", "dense", True),
    "chain-zero-255":     (255, "chain", "zero", False, None, "dense", False),
    "star-mixed-1":       (1, "star", "mixed", True, "small", "onehot", True),
    "smpl-extreme-255":   (255, "smpl", "extreme", True, "small", "last", False),
    "chain-same-257":     (257, "chain", "same", True, None, "last", True),
    "star-hand-257":      (257, "star", "random", False, "small", "onehot", False),
    "smpl-bigroot-6890":  (6890, "smpl", "bigroot", True, "large", "dense", False),
    "smpl-mixed-6890":    (6890, "smpl", "mixed", True, "small", "dense", True),
}
HOT_VERTEX = 131      # the one-hot vertex of star-hand-257, weighted to HAND alone

#: name: (parents, pose, transl, upstream)
TFS_CASES = {
    "smpl-random":   ("smpl", "random", "small", "dense"),
    "chain-zero":    ("chain", "zero", None, "dense"),
    "star-mixed":    ("star", "mixed", "small", "last"),
    "smpl-extreme":  ("smpl", "extreme", "small", "onehot"),
    "chain-bigroot": ("chain", "bigroot", "large", "dense"),
}


def _transl(kind, g):
    if kind is None:
        return None
    return (g.standard_normal(3) * 0.3 if kind == "small" else np.array([2.1, -1.7, 3.0])).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lbs_inputs(name):
    """the arrays of one LBS case, as the C entries take them (fp32 / int32); treat as read-only"""
    V, kind, pose_kind, nz_betas, tr_kind, up_kind, has_dw = LBS_CASES[name]
    seed = sorted(LBS_CASES).index(name)
    g = np.random.default_rng(4000 + seed)
    hot = HOT_VERTEX if name == "star-hand-257" else 0
    body = make_body(V, kind, seed, hot=(hot, HAND) if name == "star-hand-257" else None)
    pose = make_pose(pose_kind, seed)
    pose_t = pose.copy() if pose_kind == "same" else template_pose()
    betas = (g.uniform(-2, 2, 10) if nz_betas else np.zeros(10)).astype(np.float32)
    d_w2s = make_upstream(1, "dense", seed + 50)[0] if has_dw else None
    return dict(body=body, betas=betas, pose=pose, transl=_transl(tr_kind, g), pose_t=pose_t, po_t=pose_offsets_f32(body, pose_t),
                d_T_inv=make_upstream(V, up_kind, seed, hot), d_w2s=d_w2s)


def random_affine(g, n):
    """general affine transforms: rotation . (I + 0.1 N), translation ~0.3; fourth row (0, 0, 0, 1)"""
    R = _rodrigues(_axis_angle(g, N_J, 0.2, 2.0).astype(np.float32), np.float64)["R"][:n]
    X = _affine(R @ (np.eye(3) + 0.1 * g.standard_normal((n, 3, 3))), 0.3 * g.standard_normal((n, 3)))
    return X.astype(np.float32)


@functools.lru_cache(maxsize=None)
def tfs_inputs(name):
    kind, pose_kind, tr_kind, up_kind = TFS_CASES[name]
    seed = 100 + sorted(TFS_CASES).index(name)
    g = np.random.default_rng(4000 + seed)
    joints = (g.standard_normal((N_J, 3)) * 0.3).astype(np.float32)
    return dict(joints_rest=joints, parents=parents_table(kind), pose=make_pose(pose_kind, seed), transl=_transl(tr_kind, g),
                tfs_inv_t=random_affine(g, N_J), d_tfs=make_upstream(N_J, up_kind, seed, hot=HAND))


# ---- groups and the bound ------------------------------------------------------------------------------------------------
def _mat_groups(name, X):
    return {name + ".R": X[..., :3, :3], name + ".t": X[..., :3, 3], name + ".row3": X[..., 3, :]}


def fwd_groups(r, entry):
    """{group: array} of a forward result (a reference's dict or the kernel's outputs under the same names)"""
    g = {}
    for k in (("T_inv", "w2s") if entry == "lbs" else ("tfs", "w2s", "A")):
        g.update(_mat_groups(k, np.asarray(r[k])))
    if entry == "lbs":
        g.update(verts=np.asarray(r["verts"]), verts_t=np.asarray(r["verts_t"]))
    return g


def bwd_groups(r):
    g = {"d_pose[%02d]" % j: np.asarray(r["d_pose"]).reshape(N_J, 3)[j] for j in range(N_J)}
    g["d_transl"] = np.asarray(r["d_transl"])
    if "d_betas" in r:
        g["d_betas"] = np.asarray(r["d_betas"])
    return g


def _allow(r64, r32, mags, cancel=(), K=None):
    """{group: (float64 reference, allowance, E32, M)}"""
    K = K_BOUND if K is None else K
    out = {}
    for k, ref in r64.items():
        e32 = float(np.abs(r32[k].astype(np.float64) - ref).max())
        M = float(np.max(mags[k]))
        if k.endswith(".row3"):                       # the constant row: exact
            out[k] = (ref, 0.0, 0.0, M)
        else:
            out[k] = (ref, K * (U * M if k in cancel else max(e32, U * M)), e32, M)
    return out


def _fwd_case(entry, fwd, args):
    r64, r32 = fwd_groups(fwd(*args), entry), fwd_groups(fwd(*args, dtype=np.float32), entry)
    return _allow(r64, r32, {k: np.abs(v) for k, v in r64.items()})


def _bwd_case(bwd, args, cancel):
    R64, R32 = bwd(*args), bwd(*args, dtype=np.float32)
    mags = bwd_groups({k[2:]: v for k, v in R64.items() if k in ("m_d_pose", "m_d_betas", "m_d_transl")})
    return _allow(bwd_groups(R64), bwd_groups(R32), mags, cancel), R64


def lbs_args(i, bwd=False):
    a = (i["body"], i["betas"], i["pose"], i["transl"], i["pose_t"], i["po_t"])
    return a + (i["d_T_inv"], i["d_w2s"]) if bwd else a


def tfs_args(i, bwd=False):
    a = (i["joints_rest"], i["parents"], i["pose"], i["transl"], i["tfs_inv_t"])
    return a + (i["d_tfs"],) if bwd else a


@functools.lru_cache(maxsize=None)
def lbs_fwd_bound(name):
    return _fwd_case("lbs", lbs_fwd_ref, lbs_args(lbs_inputs(name)))


@functools.lru_cache(maxsize=None)
def lbs_bwd_bound(name):
    """({group: (ref, allow, E32, M)}, the float64 result).  d_transl is a pure cancellation when the case has no d_w2s."""
    i = lbs_inputs(name)
    return _bwd_case(lbs_bwd_ref, lbs_args(i, True), ("d_transl",) if i["d_w2s"] is None else ())


@functools.lru_cache(maxsize=None)
def tfs_fwd_bound(name):
    return _fwd_case("tfs", tfs_fwd_ref, tfs_args(tfs_inputs(name)))


@functools.lru_cache(maxsize=None)
def tfs_bwd_bound(name):
    return _bwd_case(tfs_bwd_ref, tfs_args(tfs_inputs(name), True), ("d_transl",))


def compare(got, bound, what, lines=None):
    """every group of `got` against {group: (ref, allow, E32, M)}: prints one line per group (max error, allowance, and the
    ratio error / (allow / K) the MEASURED block records), returns ({group: error / allow}, worst ratio to allow / K)"""
    over, worst = {}, 0.0
    for k, (ref, allow, e32, M) in bound.items():
        g = np.asarray(got[k], np.float64)
        assert g.shape == ref.shape, (what, k, g.shape, ref.shape)
        err = float(np.abs(g - ref).max()) if np.isfinite(g).all() else np.inf
        ratio = 0.0 if err == 0 else np.inf if allow == 0 else err / (allow / K_BOUND)
        line = "SMPLREF %-34s %-11s err %.3e  allow %.3e  (E32 %.3e  u.M %.3e)  err/(allow/K) %.3f" % (what, k, err, allow, e32, U * M, ratio)
        print(line)
        if lines is not None:
            lines.append(line)
        worst = max(worst, ratio)
        if not err <= allow:
            over[k] = err / allow if allow else np.inf
    return over, worst
