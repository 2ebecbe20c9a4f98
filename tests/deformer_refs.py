"""float64 restatements of the deformer precompute and gradient kernels of csrc/ia_snarf.hip, their seeded input sets, and
the error bounds the GPU tests apply (numpy only: no GPU, no product import, no oracle import).

Every reference takes the arrays the C entry takes (include/instantavatar_hip.h) and returns float64 results together with
what its bound needs.  A bound is |got - ref| <= K u M + A with u = 2^-24:

  M   the condition magnitude: the same expression with every summed term replaced by its absolute value;
  K   the fp32 roundings a term meets on its way into the output, counted from the kernel source next to each bound below
      (the library is built with -ffp-contract=off: one rounding per spelled operation, none inside a spelled fma);
  A   the first-order allowance for the sampled skinning weights.  The continuous voxel index is itself a rounded fp32
      expression, c = ((scale (x + offset) + 1) / 2) (size - 1): four roundings (the halving is exact), the first two on
      g = scale (x + offset) BEFORE the cancelling + 1, so the index carries an absolute error of up to
      INDEX_K u (|g| + 1) / 2 (size - 1) =: delta (equal to INDEX_K u |c| for g >= 0).  A weight moves by
      delta |dw_n / dc| per axis; dw_n / dc is the difference of the two face interpolants of the float64 reference, taken
      as the larger of its values at c - delta, c, c + delta (the interpolant is piecewise linear: a point on a voxel node
      may be sampled in either cell).  An index that stays clamped under +-delta has no allowance: both sides hold the
      border value exactly.  The allowance is carried through every sum that consumes w.

Nothing is excluded: trilinear interpolation and the border clamp are continuous, so every element of every output is
compared.  tests/test_cpu_deformer_refs.py shows that the references are right, that plain fp32 stays inside the bounds
in two association orders and that eleven seeded defects do not.
"""
import functools

import numpy as np

U = 2.0 ** -24
NB = 24                       # bones
TILE = 256                    # IA_ID_THREADS: entries per LDS tile of k_implicit_bwd
MAX_BLOCKS = 1024             # ia_implicit_blocks caps the launch
BIG_N = MAX_BLOCKS * TILE + 300      # 262 444: the smallest count at which some workgroups take a second trip
INDEX_K = 4                   # x + offset, scale *, + 1, * (size - 1)
WEIGHT_K = 13                 # up to three (1 - f), two products of the corner weight, eight accumulating fmas


class Grid:
    """ia_snarf_grid as plain values: D, H, W, offset fp32 [3], scale fp32 [3] (x, y, z)"""

    def __init__(self, D, H, W, offset, scale):
        self.D, self.H, self.W = int(D), int(H), int(W)
        self.offset, self.scale = np.asarray(offset, np.float32), np.asarray(scale, np.float32)

    @property
    def sizes(self):          # voxels along x, y, z
        return (self.W, self.H, self.D)

    @property
    def n(self):
        return self.D * self.H * self.W


# ---------------------------------------------------------------------------------------------------------------------
# association orders of the plain-fp32 evaluations
# ---------------------------------------------------------------------------------------------------------------------
class _Acc:
    """adds arrays one at a time, sequentially or pairwise (binary-counter merging), in the arrays' own dtype"""

    def __init__(self, order):
        self.order, self.stack = order, []

    def add(self, t):
        if self.order == "seq":
            self.stack = [(0, t if not self.stack else self.stack[0][1] + t)]
            return
        self.stack.append((0, t))
        while len(self.stack) > 1 and self.stack[-1][0] == self.stack[-2][0]:
            (l, b), (_, a) = self.stack.pop(), self.stack.pop()
            self.stack.append((l + 1, a + b))

    def total(self):
        s = self.stack[-1][1]
        for _, a in self.stack[-2::-1]:
            s = a + s
        return s


def _sum0(t, order):
    """sum over axis 0 in the dtype of t: 'seq' strictly in order, 'pair' by halving"""
    if t.dtype == np.float64:
        return t.sum(0)
    if order == "seq":
        return np.cumsum(t, axis=0, dtype=t.dtype)[-1] if len(t) else np.zeros(t.shape[1:], t.dtype)
    while len(t) > 1:
        h = len(t) // 2
        s = t[0:2 * h:2] + t[1:2 * h:2]
        t = np.concatenate([s, t[2 * h:]]) if len(t) % 2 else s
    return t[0] if len(t) else np.zeros(t.shape[1:], t.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# the trilinear sample of the skinning weights (deformer_torch.py:190-202: grid_sample, align_corners, border padding)
# ---------------------------------------------------------------------------------------------------------------------
def channel_last(voxel_w, grid):
    v = np.asarray(voxel_w)
    if v.shape == (NB, grid.D, grid.H, grid.W):
        return np.moveaxis(v, 0, -1)
    assert v.shape == (grid.D, grid.H, grid.W, NB), (v.shape, "neither [24,D,H,W] nor [D,H,W,24]")
    return v


def voxel_index(grid, x, dtype=np.float64, defect=None):
    """(g, c): normalised coordinate and continuous voxel index per axis [n,3], NOT clamped; dtype=np.float32 forms them op by op
    as id_border_index does"""
    ft = np.dtype(dtype).type
    x = np.asarray(x, np.float32).astype(dtype)
    size = np.array(grid.sizes).astype(dtype)
    g = grid.scale.astype(dtype) * (x + grid.offset.astype(dtype))
    if defect == "align_corners_false":
        return g, ((g + ft(1)) * size - ft(1)) / ft(2)
    return g, ((g + ft(1)) / ft(2)) * (size - ft(1))


def _trilinear(V, c, sizes, order="seq", zero_pad=False, want_dw=True):
    """V [D,H,W,24], c [n,3] -> w [n,24], dw [n,3,24] = d w / d c per axis (difference of the two face interpolants)"""
    ft = V.dtype.type
    hi = np.array(sizes, np.int64)
    if zero_pad:
        base = np.floor(c).astype(np.int64)
    else:
        c = np.minimum(np.maximum(c, ft(0)), (hi - 1).astype(V.dtype))
        base = np.minimum(np.floor(c).astype(np.int64), hi - 2)     # (the top node: fraction 1 of the last cell)
    f = (c - base.astype(V.dtype)).astype(V.dtype)
    one = ft(1)
    w, dw = _Acc(order), [_Acc(order) for _ in range(3)]
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                idx = base + np.array([cx, cy, cz])
                inside = ((idx >= 0) & (idx < hi)).all(1)
                idx = np.clip(idx, 0, hi - 1)
                v = V[idx[:, 2], idx[:, 1], idx[:, 0]] * inside[:, None].astype(V.dtype)
                wx, wy, wz = (f[:, 0] if cx else one - f[:, 0]), (f[:, 1] if cy else one - f[:, 1]), (f[:, 2] if cz else one - f[:, 2])
                w.add((wx * wy * wz)[:, None] * v)
                if want_dw:
                    sx, sy, sz = (one if cx else -one), (one if cy else -one), (one if cz else -one)
                    dw[0].add((sx * wy * wz)[:, None] * v)
                    dw[1].add((wx * sy * wz)[:, None] * v)
                    dw[2].add((wx * wy * sz)[:, None] * v)
    return w.total(), (np.stack([d.total() for d in dw], 1) if want_dw else None)


def sample_weights_ref(voxel_w, grid, x, dtype=np.float64, order="seq", defect=None, want_allow=True):
    """w [n,24], dw [n,3,24] and `allow` [n,24] = sum_axis delta_axis max|dw| (the index allowance A of one weight).
    dtype=np.float32: the same expressions op by op in fp32 (no dw, no allowance)."""
    V = channel_last(voxel_w, grid).astype(dtype)
    if defect and defect.startswith("shift_bone"):       # one bone's plane one voxel further along W
        V = V.copy()
        V[..., 7] = np.roll(V[..., 7], 1, axis=2)
    x = np.asarray(x, np.float32).reshape(-1, 3)
    g, c = voxel_index(grid, x, dtype, defect)
    zp = defect == "zero_padding"
    if np.dtype(dtype) != np.float64:
        return _trilinear(V, c, grid.sizes, order, zp, want_dw=False)[0], None, None
    w, dw = _trilinear(V, c, grid.sizes, zero_pad=zp)
    if not want_allow:
        return w, dw, None
    top = np.array(grid.sizes, np.float64) - 1
    delta = INDEX_K * U * (np.abs(g) + 1) / 2 * top
    free = (c + delta >= 0) & (c - delta <= top)         # an index that stays clamped has nothing to differ by
    lo = _trilinear(V, c - delta, grid.sizes)[1]
    up = _trilinear(V, c + delta, grid.sizes)[1]
    slope = np.maximum(np.abs(dw), np.maximum(np.abs(lo), np.abs(up)))
    allow = ((delta * free)[:, :, None] * slope).sum(1)
    return w, dw, allow


def weight_error(w, allow):
    """|w_got - w_ref| of one sampled weight: WEIGHT_K roundings on non-negative terms (their magnitude is w) + the index allowance"""
    return WEIGHT_K * U * np.abs(w) + allow


# ---------------------------------------------------------------------------------------------------------------------
# a3: precompute (precompute.cu:24-71)
# ---------------------------------------------------------------------------------------------------------------------
def precompute_variant(D, H, W):
    """the host rule of ia_precompute_ws: (threads, workgroups, 'lds' | 'direct')"""
    n_thr = D * H * W // 4
    blocks = min((n_thr + 255) // 256, 8192)
    return n_thr, blocks, ("lds" if n_thr % 64 == 0 and n_thr % (blocks * 256) == 0 else "direct")


def precompute_ref(voxel_w, tfs, grid, dtype=np.float64, order="seq", defect=None):
    """voxel_J [D,H,W,12], voxel_d [3,D,H,W], bbox [6] (mins, then maxes) and the bounds b_J, b_d, b_box.
    Only the first 12 numbers of a bone are read."""
    ft = np.dtype(dtype).type
    D, H, W = grid.D, grid.H, grid.W
    V = channel_last(voxel_w, grid).astype(dtype)                      # [D,H,W,24]
    T = np.asarray(tfs, np.float32).reshape(NB, 16)[:, :12].astype(dtype)
    acc, mag = _Acc(order), _Acc("seq")
    for j in range(NB):
        acc.add(V[..., j, None] * T[j])
        mag.add(np.abs(V[..., j, None] * T[j]))
    J, MJ = acc.total(), mag.total()
    # voxel centres ((i / (size - 1)) 2 - 1) / scale - offset
    cs, mc = [], []
    for a, size in enumerate(grid.sizes):
        t = np.arange(size).astype(dtype) / ft(size - 1)
        b = t * ft(2) - ft(1)
        c = b / ft(grid.scale[a]) - ft(grid.offset[a])
        cs.append(c)
        # |error of c| <= u Mc: t one rounding (it reaches b as 2 t u), b one, the division one, the subtraction one
        mc.append((2 * t + 2 * np.abs(b)) / abs(float(grid.scale[a])) + np.abs(c))
    cz, cy, cx = np.meshgrid(cs[2], cs[1], cs[0], indexing="ij")
    mz, my, mx = np.meshgrid(mc[2], mc[1], mc[0], indexing="ij")
    C3, MC3 = np.stack([cx, cy, cz], -1), np.stack([mx, my, mz], -1)   # [D,H,W,3]
    Jr, MJr = J.reshape(D, H, W, 3, 4), MJ.reshape(D, H, W, 3, 4)
    if order == "seq":
        d = ((Jr[..., 0] * C3[..., None, 0] + Jr[..., 1] * C3[..., None, 1]) + Jr[..., 2] * C3[..., None, 2]) + Jr[..., 3]
    else:
        d = (Jr[..., 0] * C3[..., None, 0] + Jr[..., 1] * C3[..., None, 1]) + (Jr[..., 2] * C3[..., None, 2] + Jr[..., 3])
    d = np.moveaxis(d, -1, 0)                                          # [3,D,H,W]
    out = dict(voxel_J=J, voxel_d=d)
    live = np.ones(D * H * W, bool)
    if defect == "box_ragged_wave":                                    # the lanes of the ragged last wave never reach the box
        n_thr = D * H * W // 4
        live[(n_thr // 64) * 64 * 4:] = False
    dl = d.reshape(3, -1)[:, live]
    out["bbox"] = np.concatenate([dl.min(1), dl.max(1)]) if live.any() else np.array([np.inf] * 3 + [-np.inf] * 3)
    if np.dtype(dtype) == np.float64:
        # voxel_J: 24 terms, one rounding per accumulating fma: K = 24
        out["b_J"] = 24 * U * MJ
        # voxel_d = fma(J2, cz, fma(J1, cy, J0 cx)) + J3: four terms, four roundings (K = 4) on sum |J c| + |J3|; every J carries
        # its own 24 u MJ, every centre its u Mc
        absC = np.abs(C3)
        b_d = (24 * U * ((MJr[..., :3] * absC[..., None, :]).sum(-1) + MJr[..., 3])
               + U * (np.abs(Jr[..., :3]) * MC3[..., None, :]).sum(-1)
               + 4 * U * ((np.abs(Jr[..., :3]) * absC[..., None, :]).sum(-1) + np.abs(Jr[..., 3])))
        out["b_d"] = np.moveaxis(b_d, -1, 0)
        # min and max are 1-Lipschitz in the sup norm: the box moves by no more than the worst voxel of its component
        out["b_box"] = np.tile(out["b_d"].reshape(3, -1).max(1), 2)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a7: the gradients through the roots
# ---------------------------------------------------------------------------------------------------------------------
def implicit_blocks(n):
    return max(1, min((n + TILE - 1) // TILE, MAX_BLOCKS))


def sum_depth(n):
    """the roundings a term meets in the fixed-order reduction of k_implicit_bwd + k_implicit_bwd_reduce: the fmas of its tile
    (at most 256), one `acc += a` per trip of the workgroup, the lane's walk over the partials (blocks / 64), six shuffle
    steps, the `+=` into d_tfs.  (The any-order count, n, would be blind to a dropped tile at n = 262 444.)"""
    blocks = implicit_blocks(n)
    trips = (n + blocks * TILE - 1) // (blocks * TILE)
    return min(n, TILE) + trips + (blocks + 63) // 64 + 6 + 1


def entry_keep(n_loop, defect):
    """which entry positions reach the sum under a seeded reduction defect"""
    keep = np.ones(n_loop, bool)
    if defect == "drop_last_partial_block":
        keep[(n_loop // TILE) * TILE:] = False
    elif defect == "second_tile_overwrites":
        tiles, blocks = (n_loop + TILE - 1) // TILE, implicit_blocks(n_loop)
        t = np.arange(n_loop) // TILE
        keep[t + blocks < tiles] = False
    return keep


def _outer_sum(w, vh, dtype, order, chunk=4096):
    """sum_i w[i,n] vh[i,q] -> [24,12]"""
    if np.dtype(dtype) == np.float64:
        return w.T @ vh
    acc = _Acc(order)
    for s in range(0, len(w), chunk):
        t = (w[s:s + chunk, :, None] * vh[s:s + chunk, None, :]).reshape(-1, NB * 12)
        acc.add(_sum0(t, order))
    return (acc.total() if acc.stack else np.zeros(NB * 12, dtype)).reshape(NB, 12)


def _finish(d12, prefill, dtype, defect):
    """rows 0..2 of the 4x4 receive the sums ON TOP of what d_tfs held; row 3 keeps it"""
    out = np.zeros((NB, 4, 4), dtype) if prefill is None else np.asarray(prefill, np.float32).astype(dtype).copy()
    if defect == "overwrite":
        out[:, :3, :] = 0
    out[:, :3, :] += d12.reshape(NB, 3, 4)
    return out


def _pad12(a):
    out = np.zeros((NB, 4, 4))
    out[:, :3, :] = a.reshape(NB, 3, 4)
    return out


def implicit_bwd_ref(xc, J_inv, live, grad, voxel_w, grid, prefill=None, dtype=np.float64, order="seq", defect=None):
    """d_tfs[n][c][k] = prefill + sum_live w_n v_c h_k, v = -J_inv^T g, h = (x, 1); M = the same sum with |w_n|,
    sum_r |J_inv[r][c]| |g_r| and |h_k|; A = the index allowance of w carried through the sum.  `live` [n] bool."""
    live = np.asarray(live, bool).copy()
    xc, J, g = np.asarray(xc, np.float32).reshape(-1, 3), np.asarray(J_inv, np.float32).reshape(-1, 3, 3), np.asarray(grad, np.float32).reshape(-1, 3)
    if defect == "read_past_live":           # one row past the live ones is read, and happens to hold finite numbers
        i = int(np.nonzero(~live)[0][0])
        xc, J, g = xc.copy(), J.copy(), g.copy()
        xc[i], J[i], g[i], live[i] = (0.05, -0.1, 0.02), np.eye(3), (0.5, -0.25, 1.0), True
    n_loop = int(np.nonzero(live)[0].max()) + 1 if live.any() else 0
    live[:n_loop] &= entry_keep(n_loop, defect)
    i = np.nonzero(live)[0]
    x, Jm, gm = xc[i].astype(dtype), J[i].astype(dtype), g[i].astype(dtype)
    w, _, allow = sample_weights_ref(voxel_w, grid, xc[i], dtype, order, defect)
    if defect == "J_not_transposed":
        v = -((Jm[:, :, 0] * gm[:, 0, None] + Jm[:, :, 1] * gm[:, 1, None]) + Jm[:, :, 2] * gm[:, 2, None])
    else:
        v = -((Jm[:, 0, :] * gm[:, 0, None] + Jm[:, 1, :] * gm[:, 1, None]) + Jm[:, 2, :] * gm[:, 2, None])
    h = np.concatenate([x, np.full((len(i), 1), 0 if defect == "h_without_one" else 1, dtype)], 1)
    vh = (v[:, :, None] * h[:, None, :]).reshape(-1, 12)
    out = dict(d_tfs=_finish(_outer_sum(w, vh, dtype, order), prefill, dtype, defect))
    if np.dtype(dtype) == np.float64:
        VH = ((np.abs(Jm) * np.abs(gm)[:, :, None]).sum(1)[:, :, None] * np.abs(h)[:, None, :]).reshape(-1, 12)
        out["M"] = _pad12(np.abs(w).T @ VH) + (0 if prefill is None else np.abs(np.asarray(prefill, np.float64)))
        out["A"] = _pad12(allow.T @ VH)
        out["n"] = n_loop
    return out


# v = -(J0c g0 + J3c g1 + J6c g2): each term its product and two additions (3); v h (1); the weight (WEIGHT_K); the reduction
def bound_implicit(ref, n):
    b = (sum_depth(n) + 3 + 1 + WEIGHT_K) * U * ref["M"] + ref["A"]
    b[:, 3, :] = 0                           # row 3 keeps the caller's numbers bit for bit
    return b


def entry_points(n, n_init=None, cand_pt=None):
    return np.arange(n) // n_init if cand_pt is None else np.asarray(cand_pt, np.int64)[:n]


def inverse_skinning_ref(xc, xd, pt, live, voxel_w, grid, tfs, grad=None, prefill=None, dtype=np.float64, order="seq", defect=None):
    """Version 2 (deformer_torch.py:68-75): out [n,3] = R^T (x_d - t) with T = sum_n w_n(x_c*) tfs_n for the live entries, 0
    elsewhere; with `grad` [n,3] also d_tfs (prefill + gradient, rows 0..2), d_xd [n,3] = R g (0 where not live) and the
    bounds.  `pt` [n]: the sample point of every entry (entry_points); dense and compact layouts differ only in it."""
    ft = np.dtype(dtype).type
    f64 = np.dtype(dtype) == np.float64
    live = np.asarray(live, bool).copy()
    n = len(live)
    xc = np.asarray(xc, np.float32).reshape(-1, 3)
    gr = None if grad is None else np.asarray(grad, np.float32).reshape(-1, 3)
    pt = np.asarray(pt, np.int64).copy()
    if defect == "read_past_live":
        k = int(np.nonzero(~live)[0][0])
        xc = xc.copy()
        xc[k], live[k], pt[k] = (0.05, -0.1, 0.02), True, 0
        if gr is not None:
            gr = gr.copy()
            gr[k] = (0.5, -0.25, 1.0)
    n_loop = int(np.nonzero(live)[0].max()) + 1 if live.any() else 0
    keep = live.copy()
    keep[:n_loop] &= entry_keep(n_loop, defect)
    i = np.nonzero(live)[0]
    T12 = np.asarray(tfs, np.float32).reshape(NB, 16)[:, :12].astype(dtype)
    w, _, allow = sample_weights_ref(voxel_w, grid, xc[i], dtype, order, defect)
    acc = _Acc(order)
    for b in range(NB):
        acc.add(w[:, b, None] * T12[b])
    T = acc.total().reshape(-1, 3, 4) if len(i) else np.zeros((0, 3, 4), dtype)
    X = np.asarray(xd, np.float32)[pt[i]].astype(dtype)
    a = X - T[:, :, 3]
    val = (a[:, 0, None] * T[:, 0, :3] + a[:, 1, None] * T[:, 1, :3]) + a[:, 2, None] * T[:, 2, :3]
    out = dict(out=np.zeros((n, 3), dtype))
    out["out"][i] = val
    if f64:
        ew = weight_error(w, allow)
        MT = (np.abs(w) @ np.abs(T12)).reshape(-1, 3, 4)
        eT = 24 * U * MT + (ew @ np.abs(T12)).reshape(-1, 3, 4)        # 24 accumulating fmas + the weights' own error
        A_ = np.abs(X) + MT[:, :, 3]                                    # magnitude of a = x_d - t
        ea = eT[:, :, 3] + U * A_                                       # one subtraction
        # out_j = a0 T0j + a1 T4j + a2 T8j: three terms, each its product and two additions (3)
        b_out = np.zeros((n, 3))
        b_out[i] = ((3 * U * A_ + ea)[:, :, None] * MT[:, :, :3] + A_[:, :, None] * eT[:, :, :3]).sum(1)
        out["b_out"] = b_out
    if gr is None:
        return out
    g = gr[i].astype(dtype)
    vh = np.zeros((len(i), 3, 4), dtype)
    vh[:, :, :3] = a[:, :, None] * g[:, None, :]
    Rg = (T[:, :, 0] * g[:, 0, None] + T[:, :, 1] * g[:, 1, None]) + T[:, :, 2] * g[:, 2, None]
    vh[:, :, 3] = Rg if defect == "v2_translation_sign" else -Rg
    k = keep[i]
    out["d_tfs"] = _finish(_outer_sum(w[k], vh[k].reshape(-1, 12), dtype, order), prefill, dtype, defect)
    out["d_xd"] = np.zeros((n, 3), dtype)
    out["d_xd"][i] = Rg
    if f64:
        ag = np.abs(g)
        VH, eVH = np.zeros((len(i), 3, 4)), np.zeros((len(i), 3, 4))
        VH[:, :, :3] = A_[:, :, None] * ag[:, None, :]
        eVH[:, :, :3] = (ea + U * A_)[:, :, None] * ag[:, None, :]      # a g: the error of a and one product
        VH[:, :, 3] = (MT[:, :, :3] * ag[:, None, :]).sum(2)
        eVH[:, :, 3] = ((3 * U * MT[:, :, :3] + eT[:, :, :3]) * ag[:, None, :]).sum(2)      # three terms, product + two additions
        out["M"] = _pad12(np.abs(w).T @ VH.reshape(-1, 12)) + (0 if prefill is None else np.abs(np.asarray(prefill, np.float64)))
        out["A"] = _pad12(ew.T @ VH.reshape(-1, 12) + np.abs(w).T @ eVH.reshape(-1, 12))     # (the weights' K is inside ew)
        out["b_d_xd"] = np.zeros((n, 3))
        out["b_d_xd"][i] = eVH[:, :, 3]
        out["n"] = n_loop
    return out


def bound_inverse_bwd(ref, n):
    b = sum_depth(n) * U * ref["M"] + ref["A"]
    b[:, 3, :] = 0
    return b


def expand_candidate_points_ref(pt_off, pt_cnt, P, n_pts, cap, cand_pt):
    """cand_pt[pt_off[p] + j] = p for j < pt_cnt[p] below cap, over the first min(P, n_pts) points; the rest untouched"""
    out = np.array(cand_pt, np.int32)
    for p in range(P if n_pts is None else min(P, int(n_pts))):
        o, c = int(pt_off[p]), int(pt_cnt[p])
        for j in range(c):
            if o + j < cap:
                out[o + j] = p
    return out


# ---------------------------------------------------------------------------------------------------------------------
# seeded input sets, shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
# the z scale is `ratio` (4) times the others, as ForwardDeformer's descriptor; nothing dyadic
OFFSET = np.array([0.0371, -0.2113, 0.0158], np.float32)
SCALE = np.array([0.8731, 0.8731, 0.8731 * 4], np.float32)

# (D, H, W) -> the variant the host rule of ia_precompute_ws picks (asserted from precompute_variant on the CPU)
PRECOMPUTE_GRIDS = (
    ((2, 2, 4), "direct"),      # 4 threads of one wave
    ((3, 5, 12), "direct"),     # 45 threads: lanes without a trip take part in the reductions
    ((4, 8, 40), "direct"),     # 320 threads: whole waves, not whole launches; the second workgroup is ragged
    ((5, 16, 20), "direct"),    # 400 threads: ragged last wave
    ((4, 8, 64), "lds"),        # 512 threads, two workgroups
    ((8, 32, 32), "lds"),       # the suite's own grid
)
SAMPLE_VOLUMES = ((3, 5, 8), (4, 6, 16))
ENTRY_COUNTS = (1, 255, 257, 785)


def make_grid(D, H, W):
    return Grid(D, H, W, OFFSET, SCALE)


def make_volume(grid, seed=0):
    """channel-major [24,D,H,W] and channel-last [D,H,W,24] copies of the same values: random non-negative weights that sum
    to 1 per voxel (in float64, then rounded), a few voxels with a single weight of exactly 1"""
    rng = np.random.RandomState(7000 + seed + grid.n)
    w = rng.rand(grid.D, grid.H, grid.W, NB) ** 4              # a few bones carry a voxel, the others little
    w[rng.rand(*w.shape) < 0.3] = 0
    w[..., 0] += 1e-3
    w = (w / w.sum(-1, keepdims=True)).astype(np.float32)
    flat = w.reshape(-1, NB)
    for v in rng.choice(len(flat), max(2, len(flat) // 40), replace=False):
        flat[v] = 0
        flat[v, rng.randint(NB)] = 1
    return np.ascontiguousarray(np.moveaxis(w, -1, 0)), np.ascontiguousarray(w)


def make_tfs(seed=0):
    """24 rigid transforms, translations up to +-1; row 3 is NaN: nobody may read it"""
    rng = np.random.RandomState(7100 + seed)
    t = np.full((NB, 4, 4), np.nan, np.float32)
    for b in range(NB):
        q, r = np.linalg.qr(rng.randn(3, 3))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        t[b, :3, :3], t[b, :3, 3] = q, rng.uniform(-1, 1, 3)
    return t


def make_prefill(seed=0):
    rng = np.random.RandomState(7200 + seed)
    p = rng.randn(NB, 4, 4).astype(np.float32)
    return np.where(np.abs(p) < 0.05, np.float32(0.05), p)


def _x_of(grid, g):
    """the fp32 point nearest to the normalised coordinates g"""
    return (np.asarray(g, np.float64) / grid.scale.astype(np.float64) - grid.offset.astype(np.float64)).astype(np.float32)


def _x_with_index(grid, axis, target, other_g, rng):
    """a point whose fp32 voxel index along `axis` is exactly `target` (searched among the neighbours of the nearest fp32 point)"""
    size = grid.sizes[axis]
    g = np.array(other_g, np.float64)
    g[axis] = 2.0 * target / (size - 1) - 1
    x = _x_of(grid, g)
    for k in range(0, 64):
        for s in ((0,) if k == 0 else (1, -1)):
            y = x.copy()
            for _ in range(k):
                y[axis] = np.nextafter(y[axis], np.float32(s * np.inf))
            if voxel_index(grid, y[None], np.float32)[1][0, axis] == np.float32(target):
                return y
    return None


def _x_on_node(grid, axis, targets, other_g, rng):
    """the first of `targets` that some fp32 point attains exactly (near the low face the cancelling + 1 leaves the attainable
    indices too sparse for some nodes)"""
    for t in targets:
        y = _x_with_index(grid, axis, int(t), other_g, rng)
        if y is not None:
            return y
    raise AssertionError(("no fp32 point with an index among", axis, list(targets)))


def query_points(grid, n, seed=0):
    """n points: interior ones, points exactly on voxel nodes (fraction 0 along one or all axes), on each of the six faces
    (normalised coordinate exactly -1 or +1, i.e. fp32 index exactly 0 or size - 1), and outside by up to 3: the structured
    points first (returned: their number), every one of them live in the input sets below"""
    rng = np.random.RandomState(7300 + seed + n)
    pts = []
    for axis in range(3):                                     # the six faces
        for target in (0, grid.sizes[axis] - 1):
            pts.append(_x_on_node(grid, axis, [target], rng.uniform(-0.9, 0.9, 3), rng))
    for axis in range(3):                                     # interior nodes along one axis
        for _ in range(2):
            pts.append(_x_on_node(grid, axis, 1 + rng.permutation(grid.sizes[axis] - 2), rng.uniform(-0.9, 0.9, 3), rng))
    for _ in range(4):                                        # a node along all three
        y = _x_of(grid, np.zeros(3))
        for axis in range(3):
            y[axis] = _x_on_node(grid, axis, rng.permutation(grid.sizes[axis]), np.zeros(3), rng)[axis]
        pts.append(y)
    for j in range(12):                                       # outside on one, two or three axes
        g = rng.uniform(-0.9, 0.9, 3)
        axes = rng.permutation(3)[:1 + j % 3]
        g[axes] = rng.choice([-1, 1], len(axes)) * rng.uniform(1.0, 4.0, len(axes))
        pts.append(_x_of(grid, g))
    pts = np.array(pts, np.float32)
    if n <= len(pts):
        return _x_of(grid, rng.uniform(-0.9, 0.9, (n, 3))), 0
    return np.concatenate([pts, _x_of(grid, rng.uniform(-0.98, 0.98, (n - len(pts), 3)))]), len(pts)


def _spread(rng, shape):
    """both signs, magnitudes over seven binades"""
    return (rng.randn(*shape) * 2.0 ** rng.randint(-3, 4, shape[:1] + (1,) * (len(shape) - 1))).astype(np.float32)


def candidate_lists(n, seed=0):
    """point lists whose counts (0..13, some 0, some 13) add up to exactly n: pt_off, pt_cnt, P"""
    rng = np.random.RandomState(7400 + seed + n)
    cnt = []
    while sum(cnt) < n:
        r = rng.rand()
        cnt.append(0 if r < 0.2 else (13 if r < 0.35 else int(rng.randint(1, 13))))
    cnt[-1] -= sum(cnt) - n
    cnt = np.array(cnt, np.uint8)
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))[:-1]]).astype(np.int32)
    return off, cnt, len(cnt)


@functools.lru_cache(maxsize=None)
def sampling_inputs(dims, n, layout, n_init=13, live_rule="default", seed=0):
    """One input set of the sampling kernels.  layout 'dense': a validity mask with about 30 % zeros, entry e belongs to point
    e // n_init; 'compact': the first n_cand rows are live (n_cand well below cap = n), entry e belongs to cand_pt[e].  Every
    row that is not live holds NaN in xc, J_inv and grad.  live_rule: 'over' (*n_cand > cap), 'zero' (*n_cand = 0),
    'nearly_all' (the large cases: the second trip must find live rows)."""
    grid = make_grid(*dims)
    rng = np.random.RandomState(7500 + seed + 3 * n + (layout == "compact"))
    cm, cl = make_volume(grid, seed)
    xc, n_struct = query_points(grid, n, seed)
    J_inv, grad = _spread(rng, (n, 3, 3)), _spread(rng, (n, 3))
    if n > 8:
        grad[rng.choice(n, 5, replace=False)] = 0
        grad[rng.choice(n, 5, replace=False), rng.randint(0, 3, 5)] = 0
    inp = dict(grid=grid, cm=cm, cl=cl, n=n, layout=layout, tfs=make_tfs(seed), prefill=make_prefill(seed))
    if layout == "dense":
        valid = (rng.rand(n) >= (0.3 if n > 1 else 0.0)).astype(np.uint8)
        valid[:n_struct] = 1
        if live_rule == "nearly_all":
            valid[-TILE:] = 1
        live = valid.astype(bool)
        P = (n + n_init - 1) // n_init
        inp.update(valid=valid, n_cand=None, n_init=n_init, cand_pt=None, pt=entry_points(n, n_init), P=P)
    else:
        n_cand = {"default": max(1, (n * 3) // 5) if n > 1 else 1, "over": n + 37, "zero": 0, "nearly_all": n - 14}[live_rule]
        live = np.arange(n) < n_cand
        off, cnt, P = candidate_lists(n, seed)
        cand_pt = expand_candidate_points_ref(off, cnt, P, None, n, np.full(n, -1, np.int32))
        inp.update(valid=None, n_cand=n_cand, n_init=0, cand_pt=cand_pt, pt=entry_points(n, cand_pt=cand_pt), P=P, pt_off=off, pt_cnt=cnt)
    xc[~live], J_inv[~live], grad[~live] = np.nan, np.nan, np.nan
    inp.update(xc=xc, J_inv=J_inv.reshape(n, 9), grad=grad, live=live, xd=rng.uniform(-1, 1, (P, 3)).astype(np.float32))
    return inp


def expand_inputs(P, seed=0):
    """lists with empty and full (13) counts; cap cuts one list in the middle; n_pts below P (and None: all P)"""
    rng = np.random.RandomState(7600 + seed + P)
    cnt = rng.randint(0, 14, P).astype(np.uint8)
    cnt[rng.rand(P) < 0.25] = 0
    cnt[rng.rand(P) < 0.15] = 13
    if P == 1:
        cnt[0] = 13
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))[:-1]]).astype(np.int32)
    total = int(cnt.sum())
    cut = next(p for p in range(P - 1, -1, -1) if cnt[p] >= 2)
    cap = int(off[cut]) + int(cnt[cut]) // 2                   # the list of point `cut` is cut in the middle
    return dict(pt_off=off, pt_cnt=cnt, P=P, total=total, cap=cap, n_pts=max(1, P - 9) if P > 1 else 1)
