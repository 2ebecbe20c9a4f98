"""References, seeded bodies and point sets, and comparators for the nearest-vertex kernels of csrc/ia_smpl_nn.hip
(`ia_smpl_nn_deform`, `ia_smpl_nn_compact` on the brute-force and on the grid route, `ia_smpl_nn_grid_build`,
`ia_smpl_deform_query`).  numpy only: no GPU, no torch, no product import, no oracle.

Two layers.

EXACT (`nn_exact`): what the kernels must reproduce bit for bit.  The library is built with -ffp-contract=off and the
kernels spell their fused operations, so for float32 inputs
    d       = fl(p - v) per axis
    dist    = fma32(dz, dz, fma32(dy, dy, fl(dx dx)))           (fma32 of train_step_refs: one rounding)
    winner  = smallest dist, lowest vertex index among equals; a NaN distance never wins; nothing wins -> index 0
    valid   = dist < fl(thr thr), strictly
    cano_r  = fl(fma32(T_r2, pz, fma32(T_r1, py, fl(T_r0 px))) + T_r3),  T = T_inv[winner], r = 0..2
NaN results are compared as NaN (the payload of a NaN is not pinned by IEEE 754 and differs between the host and the
device); every other value, signed zeros and infinities included, by its bits.

FLOAT64 (`check64`): what makes the exact layer a reference and not a copy of the kernel.  Squared distances and the affine
map in float64 from the same float32 inputs, u = 2^-24:
    |dist32 - dist64| <= 6 u dist64     one rounding on each difference (doubled by the square), at most three more on the
                                        path of the dx^2 term (product, two fused sums), second order inside the slack
    |cano32 - cano64| <= 4 u (sum_c |T_rc p_c| + |T_r3|)        product, two fused sums, the final sum
so (1) for every finite point dist64(p, v_winner) <= (1 + 12 u) min_v dist64(p, v): the chosen vertex is a true nearest up
to rounding; (2) valid equals dist64 < thr2 wherever |dist64 - thr2| > 6 u thr2, thr2 the float32 product fl(thr thr) that
the entry itself compares with; (3) cano is within its bound of T_inv[winner] applied in float64.  No point is excluded:
the float64 layer constrains every point, the exact layer decides what it leaves open (ties, the band around thr2,
non-finite coordinates).

`GridEmu` restates k_nn_grid_header, the cell function, the clamped binning and the 27-cell query in float32 numpy, with
switches for the seeded defects of tests/test_cpu_smpl_nn_refs.py.  It serves the CPU file only: the GPU tests treat the grid
as a black box and never read the buffer.

Bodies: the nine seeded ones of the issue and `margin`, a directed two-vertex body that only cells wider than the threshold
serve correctly (see MARGIN_THR).
"""
import functools

import numpy as np

from train_step_refs import fma32

U = 2.0 ** -24
F = np.float32
SENT_F = F(-7777.0)        # prefill of float outputs
SENT_I = np.int32(-12345)  # prefill of int32 outputs
SENT_B = np.uint8(0xA5)    # prefill of uint8 outputs
NN_THREADS = 256           # points per workgroup of k_smpl_nn / k_smpl_nn_grid
NN_UNROLL = 4              # unroll factor of the brute-force vertex loop
MAX_DIM = 64               # IA_NNG_MAX_DIM
MAX_VERTS = 13312          # n_verts * 12 <= 160 KB - 4 KB: the largest the entries accept (156 KB of LDS)
P_CAP = 4096


def _fma(a, b, c):
    """fma32 that keeps overflow and non-finite operands as IEEE does (the round-to-odd step is for finite sums only)"""
    with np.errstate(all="ignore"):
        a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
        plain = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        r = fma32(a, b, c)
        return np.where(np.isfinite(plain), r, plain.astype(F)).astype(F)


def same_bits(a, b):
    """elementwise: equal bits, or both NaN"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def thr2_of(thr):
    return F(F(thr) * F(thr))


# =====================================================================================================================
# exact layer
# =====================================================================================================================
def dist32(pts, verts, fused=True):
    """[P, V] float32 squared distances in the kernels' operation order (fused=False: plain products and sums)"""
    p, v = np.asarray(pts, F), np.asarray(verts, F)
    with np.errstate(all="ignore"):
        dx, dy, dz = (p[:, None, c] - v[None, :, c] for c in range(3))
        if fused:
            return _fma(dz, dz, _fma(dy, dy, dx * dx))
        return ((dx * dx + dy * dy) + dz * dz).astype(F)


def transform32(T, pts, translation=True):
    """[P, 3]: rows 0..2 of T [P, 4, 4] applied to pts in the kernels' operation order"""
    T, p = np.asarray(T, F), np.asarray(pts, F)
    with np.errstate(all="ignore"):
        out = np.empty((len(p), 3), F)
        for r in range(3):
            acc = _fma(T[:, r, 2], p[:, 2], _fma(T[:, r, 1], p[:, 1], T[:, r, 0] * p[:, 0]))
            out[:, r] = acc + T[:, r, 3] if translation else acc
        return out


def nn_exact(pts, verts, T_inv, thr, mutant=None, chunk=512):
    """-> dict(idx int32 [P], valid bool [P], cano float32 [P, 3], best float32 [P], ties int [P]: vertices at the winning
    distance).  mutant: one of the seeded defects of the brute-force kernel (None: the reference)."""
    pts, verts, T_inv = np.asarray(pts, F).reshape(-1, 3), np.asarray(verts, F).reshape(-1, 3), np.asarray(T_inv, F)
    P, V = len(pts), len(verts)
    use = V - V % NN_UNROLL if mutant == "skip_tail" else V
    idx, best, ties = np.zeros(P, np.int32), np.full(P, np.inf, F), np.zeros(P, np.int64)
    for s in range(0, P, chunk):
        d = dist32(pts[s:s + chunk], verts[:use], fused=mutant != "unfused") if use else np.full((len(pts[s:s + chunk]), 1), np.inf, F)
        d = np.where(np.isnan(d), np.inf, d).astype(F)
        bi = np.argmin(d, 1)                                   # the first minimum: the lowest index among equals
        b = d[np.arange(len(d)), bi]
        idx[s:s + chunk], best[s:s + chunk] = bi, b
        ties[s:s + chunk] = np.where(np.isfinite(b), (d == b[:, None]).sum(1), 0)
    t2 = thr2_of(thr)
    valid = best <= t2 if mutant == "le" else best < t2
    cano = transform32(T_inv[idx], pts, translation=mutant != "no_translation")
    return dict(idx=idx, valid=valid, cano=cano, best=best, ties=ties)


# =====================================================================================================================
# float64 layer
# =====================================================================================================================
def check64(pts, verts, T_inv, thr, idx, valid, cano, chunk=512):
    """The float64 comparator on the outputs (idx, valid, cano) of all P points -> dict(nn, cano: worst value / bound,
    valid_wrong: points whose validity contradicts float64 outside the band, decided: points outside the band)."""
    pts, verts = np.asarray(pts, F).reshape(-1, 3), np.asarray(verts, F).reshape(-1, 3)
    p64, v64, T64 = pts.astype(np.float64), verts.astype(np.float64), np.asarray(T_inv, F).astype(np.float64)
    idx, valid, cano = np.asarray(idx, np.int64), np.asarray(valid).astype(bool), np.asarray(cano, F)
    P = len(pts)
    assert idx.shape == (P,) and valid.shape == (P,) and cano.shape == (P, 3)
    assert ((idx >= 0) & (idx < len(verts))).all(), "a vertex index outside [0, n_verts)"
    finite = np.isfinite(pts).all(1)
    t2 = float(thr2_of(thr))
    r_nn, wrong, decided = 0.0, 0, 0
    with np.errstate(all="ignore"):
        for s in range(0, P, chunk):
            d = ((p64[s:s + chunk, None, :] - v64[None]) ** 2).sum(-1)
            mn = d.min(1)
            own = d[np.arange(len(d)), idx[s:s + chunk]]
            f = finite[s:s + chunk]
            # (1) a true nearest up to rounding; a distance of exactly zero admits only zero
            ex = np.where(mn > 0, (own / np.where(mn > 0, mn, 1.0) - 1.0) / (12 * U), np.where(own == 0, 0.0, np.inf))
            if f.any():
                r_nn = max(r_nn, float(ex[f].max()))
            # (2) validity outside the band (non-finite points: never valid)
            clear = np.abs(own - t2) > 6 * U * t2
            want = own < t2
            v = valid[s:s + chunk]
            wrong += int((clear & f & (v != want)).sum()) + int((~f & ~np.isfinite(own) & v).sum())
            decided += int((clear & f).sum())
        # (3) the affine map of the chosen vertex
        T = T64[idx]
        ref = (T[:, :3, :3] * p64[:, None, :]).sum(-1) + T[:, :3, 3]
        bound = 4 * U * (np.abs(T[:, :3, :3] * p64[:, None, :]).sum(-1) + np.abs(T[:, :3, 3]))
        err = np.abs(cano.astype(np.float64) - ref)
        err = np.where(np.isnan(err), np.inf, err)
        r_cano = float((err[finite] / bound[finite]).max()) if finite.any() else 0.0
    return dict(nn=r_nn, cano=r_cano, valid_wrong=wrong, decided=decided)


def passes64(r):
    return r["nn"] <= 1.0 and r["cano"] <= 1.0 and r["valid_wrong"] == 0


def agree_exact(got, ref, live=None):
    """number of points at which (idx, valid, cano) differ from the exact layer's"""
    bad = (np.asarray(got["idx"]) != ref["idx"]) | (np.asarray(got["valid"]).astype(bool) != ref["valid"]) | ~same_bits(got["cano"], ref["cano"]).all(1)
    return int(bad.sum() if live is None else bad[:live].sum())


# =====================================================================================================================
# compaction
# =====================================================================================================================
def compact_ref(ref, n_live):
    """the compaction of the first n_live points in point order: dict(n_cand, pt_cnt [n_live] uint8, pt_off [n_live] (the
    exclusive count of valid points), cand_pt [n_cand], cand_xc [n_cand, 3])"""
    v = ref["valid"][:n_live]
    off = (np.cumsum(v) - v).astype(np.int32)
    pt = np.flatnonzero(v).astype(np.int32)
    return dict(n_cand=int(v.sum()), pt_cnt=v.astype(np.uint8), pt_off=off, cand_pt=pt, cand_xc=ref["cano"][:n_live][v])


def check_compact(out, ref, n_live, route):
    """Asserts the outputs of ia_smpl_nn_compact (host arrays of the full buffers, prefilled with the sentinels) against the
    exact layer.  Workgroups reserve their ranges with one atomic each, so blocks of 256 points may be permuted among
    themselves: everything is compared per point, never by position."""
    assert all(len(out[k]) >= n_live for k in ("pt_cnt", "pt_off", "idx", "cand_pt", "cand_xc")), "buffers shorter than the live count"
    v = ref["valid"][:n_live]
    n = int(v.sum())
    assert int(out["n_cand"]) == n, ("n_cand", int(out["n_cand"]), n)
    assert np.array_equal(out["pt_cnt"][:n_live], v.astype(np.uint8)), "pt_cnt is not the validity"
    off = out["pt_off"][:n_live].astype(np.int64)
    ov = off[v]
    assert np.array_equal(np.sort(ov), np.arange(n)), "pt_off of the valid points is not a bijection onto [0, n_cand)"
    where = np.flatnonzero(v)
    for b in range(0, n_live, NN_THREADS):
        m = (where >= b) & (where < b + NN_THREADS)
        o = ov[m]
        if len(o):
            assert (np.diff(o) == 1).all(), ("block %d: offsets not increasing and contiguous" % (b // NN_THREADS))
    assert np.array_equal(out["cand_pt"][ov], where), "cand_pt[pt_off[i]] != i"
    assert same_bits(out["cand_xc"][ov], ref["cano"][:n_live][v]).all(), "cand_xc differs from the exact canonical point"
    if route == "brute":
        assert np.array_equal(out["idx"][:n_live], ref["idx"][:n_live]), "idx differs (brute force: every live point)"
    else:
        assert np.array_equal(out["idx"][:n_live][v], ref["idx"][:n_live][v]) and (out["idx"][:n_live][~v] == -1).all(), "idx differs (grid route)"
    # prefill: slots at or past n_cand, rows at or past the live count
    assert (out["cand_pt"][n:] == SENT_I).all() and (out["cand_xc"][n:] == SENT_F).all(), "a candidate slot at or past n_cand was written"
    assert (out["idx"][n_live:] == SENT_I).all() and (out["pt_off"][n_live:] == SENT_I).all() and (out["pt_cnt"][n_live:] == SENT_B).all(), \
        "a row at or past the live count was written"


# =====================================================================================================================
# the grid, restated
# =====================================================================================================================
class GridEmu:
    """k_nn_grid_header + k_nn_grid_count / _fill (clamped binning) in float32, and the query of k_smpl_nn_grid.
    defect: None | "cell_thr" | "cell_half" | "own_cell" | "corner" | "slot_ties" | "upper_face" """

    def __init__(self, verts, thr, defect=None):
        v = self.verts = np.asarray(verts, F).reshape(-1, 3)
        self.defect = defect
        factor = {"cell_thr": F(1.0), "cell_half": F(0.5)}.get(defect, F(1.001))
        min_cell = F(F(thr) * factor)
        mn, mx = v.min(0), v.max(0)
        ext = F(max(F(0), (mx - mn).max()))
        h = F(max(min_cell, F(F(ext / F(MAX_DIM - 2)) * F(1.0001))))
        if not h > 0:
            h = F(1)
        self.h, self.inv_h = h, F(F(1) / h)
        self.origin = (mn - h).astype(F)
        self.dims = np.minimum(MAX_DIM, np.floor(((mx - self.origin) * self.inv_h).astype(F)).astype(np.int64) + 2)
        raw = self.cell_float(v)
        self.in_grid = np.ones(len(v), bool)
        if defect == "upper_face":                         # a vertex on the upper face of the box is not binned
            self.in_grid = ~(v == mx).any(1)
        self.vcell = np.clip(raw, 0, self.dims - 1).astype(np.int64)

    def cell_float(self, x):
        with np.errstate(all="ignore"):
            return np.floor(((np.asarray(x, F) - self.origin) * self.inv_h).astype(F))

    def query(self, pts, T_inv, thr, chunk=512):
        """-> dict(idx (-1 where not valid), valid, cano (0 where not valid))"""
        pts = np.asarray(pts, F).reshape(-1, 3)
        P = len(pts)
        idx, valid = np.full(P, -1, np.int32), np.zeros(P, bool)
        t2 = thr2_of(thr)
        reach = 0 if self.defect == "own_cell" else 1
        for s in range(0, P, chunk):
            p = pts[s:s + chunk]
            pc = self.cell_float(p)
            with np.errstate(all="ignore"):
                inside = ((pc >= -1) & (pc <= self.dims)).all(1)             # NaN fails
                pci = np.where(np.isfinite(pc), np.clip(pc, -4, MAX_DIM + 4), -4).astype(np.int64)
            delta = self.vcell[None, :, :] - pci[:, None, :]
            near = (np.abs(delta) <= reach).all(-1) & inside[:, None] & self.in_grid[None]
            if self.defect == "corner":
                near &= ~(delta == 1).all(-1)
            d = dist32(p, self.verts)
            d = np.where(np.isnan(d) | ~near, np.inf, d).astype(F)
            if self.defect == "slot_ties":                                   # arrival order taken as descending index
                bi = d.shape[1] - 1 - np.argmin(d[:, ::-1], 1)
            else:
                bi = np.argmin(d, 1)
            b = d[np.arange(len(d)), bi]
            ok = np.isfinite(b) & (b < t2)
            idx[s:s + chunk] = np.where(ok, bi, -1)
            valid[s:s + chunk] = ok
        cano = np.where(valid[:, None], transform32(np.asarray(T_inv, F)[np.maximum(idx, 0)], pts), F(0)).astype(F)
        return dict(idx=idx, valid=valid, cano=cano)


def agree_grid(got, ref):
    """points at which a grid-route result differs from the exact layer: validity; index and canonical point where valid"""
    v = ref["valid"]
    bad = got["valid"] != v
    bad |= v & ((got["idx"] != ref["idx"]) | ~same_bits(got["cano"], ref["cano"]).all(1))
    bad |= ~v & (got["idx"] != -1)
    return int(bad.sum())


# =====================================================================================================================
# bodies
# =====================================================================================================================
BODIES = ("cloud257", "aniso1031", "lattice400", "sheet", "line500", "coincident5", "one", "far", "doubled100", "margin")
TIE_BODIES = ("lattice400", "coincident5", "doubled100")
STAGING_SIZES = (1, 3, 5, 64, 5461, 5462, 6890, MAX_VERTS)      # 5461 / 5462: 65 532 / 65 544 bytes of dynamic LDS
STAGING_P = 300
P_PREFIXES = (1, 63, 64, 65, 255, 256, 257, 1000)


def _lattice(rng, n, side):
    """n distinct points of the lattice k / 64, 0 <= k < side"""
    flat = rng.choice(side ** 3, n, replace=False)
    return (np.stack([flat // side ** 2, flat // side % side, flat % side], 1) / 64.0).astype(F)


def make_body(name):
    """-> (verts float32 [V, 3], thr)"""
    rng = np.random.RandomState(4100 + BODIES.index(name))
    if name == "cloud257":
        return (rng.randn(257, 3) * 0.05).astype(F), 0.05
    if name == "aniso1031":
        return (rng.randn(1031, 3) * (0.2, 0.5, 0.12)).astype(F), 0.05
    if name == "lattice400":
        return _lattice(rng, 400, 40), 5.0 / 64.0
    if name == "sheet":
        v = rng.uniform(-0.5, 0.5, (600, 3))
        v[:, 2] = 0
        return v.astype(F), 0.05
    if name == "line500":
        v = np.zeros((500, 3))
        v[:, 0] = np.linspace(-1, 1, 500)
        return v.astype(F), 0.01
    if name == "coincident5":
        return np.tile(np.array([[0.1, -0.2, 0.3]], F), (5, 1)), 0.05
    if name == "one":
        return np.array([[-0.3, 0.25, 0.1]], F), 0.05
    if name == "far":
        return (rng.randn(257, 3) * 0.05 + (1000.0, -500.0, 250.0)).astype(F), 0.05
    if name == "doubled100":
        v = _lattice(rng, 100, 24)
        return np.concatenate([v, v])[rng.permutation(200)], 5.0 / 64.0
    if name == "margin":
        return np.array([[0, 0, 0], [MARGIN_V1, 0, 0]], F), MARGIN_THR
    raise KeyError(name)


# The directed body for the margin of the cell width (cells 1.001 thr wide, not thr).  Two vertices on the x axis, the second a
# hair above 4 thr, so that the grid is 6 cells long and the cell is set by the threshold.  The cell coordinate of a position is
# fl(fl(x - origin) * inv_h): the subtraction rounds too.  With cells exactly thr wide the second vertex's coordinate rounds UP to
# 5.0 while a point pred(thr) below it, a valid point, stays under 4.0 -- two cells apart, so the 27-cell search misses the vertex.
# Found by scanning thresholds in [0.02, 0.1] and vertices within 40 ulp of 4 thr (the thresholds 0.05, 5 / 64 and 0.01 of the
# other bodies have no such vertex); fixed here.
MARGIN_THR, MARGIN_V1, MARGIN_STEPS = F(0.05067532), F(0.20270127), 60


def margin_points():
    """x = v +- d on the axis for both vertices v and thr and the MARGIN_STEPS floats below it as d"""
    d = [F(MARGIN_THR)]
    for _ in range(MARGIN_STEPS):
        d.append(np.nextafter(d[-1], F(0)))
    d = np.array(d, F)
    x = np.concatenate([F(MARGIN_V1) - d, F(MARGIN_V1) + d, -d, d]).astype(F)
    pts = np.zeros((len(x), 3), F)
    pts[:, 0] = x
    return pts


def staging_body(n_verts):
    rng = np.random.RandomState(4300 + n_verts % 997)
    return (rng.randn(n_verts, 3) * (0.3, 0.6, 0.2)).astype(F), 0.05


def make_T_inv(n_verts, seed):
    """[V, 4, 4]: a perturbed identity and a translation per vertex, nothing dyadic; row 3 is (0, 0, 0, 1)"""
    rng = np.random.RandomState(4500 + seed)
    T = np.zeros((n_verts, 4, 4), F)
    T[:, :3, :3] = np.eye(3) + rng.randn(n_verts, 3, 3) * 0.2
    T[:, :3, 3] = rng.randn(n_verts, 3) * 0.15
    T[:, 3, 3] = 1
    return T


PERMS_340 = np.array([(3, 4, 0), (4, 3, 0), (3, 0, 4), (4, 0, 3), (0, 3, 4), (0, 4, 3)], np.float64) / 5.0
SPECIALS = (np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -0.0)


def make_points(verts, thr, seed, scale=1.0, extra=None):
    """the point kinds of the issue, concatenated and then interleaved by one seeded permutation so that every prefix mixes the
    kinds; float32 [P, 3], P <= P_CAP at scale 1"""
    rng = np.random.RandomState(4700 + seed)
    v64 = np.asarray(verts, np.float64)
    V = len(v64)
    k = lambda n: max(1, int(n * scale))
    pick = lambda n: v64[rng.randint(0, V, n)]
    if scale >= 1.0:
        own = np.arange(V)                                                             # every vertex itself
    else:                                                                              # (the 300-point sets of the staging sizes:
        own = np.unique(np.concatenate([np.arange(min(V, 4)), np.arange(max(V - 4, 0), V), v64.argmin(0), v64.argmax(0),   # both ends, the
                                        rng.permutation(V)[:k(400)]]))                 # extreme ones and a sample)
    sets = [v64[own]]
    sets.append(pick(k(600)) + rng.randn(k(600), 3) * 0.7 * thr)                       # around the vertices
    axis = np.eye(3)[rng.randint(0, 3, k(300))] * rng.choice([-1.0, 1.0], (k(300), 1))
    sets.append(pick(k(300)) + thr * axis)                                             # at the threshold along one axis
    sets.append(pick(k(300)) + 0.999 * thr / np.sqrt(3.0) * rng.choice([-1.0, 1.0], (k(300), 3)))   # the corner cells of the 27
    sets.append(pick(k(300)) + thr * PERMS_340[rng.randint(0, 6, k(300))] * rng.choice([-1.0, 1.0], (k(300), 3)))   # |.| = thr off the axes
    u = rng.randn(k(600), 3)
    sets.append(pick(k(600)) + thr * u / np.linalg.norm(u, axis=1, keepdims=True))     # on the threshold sphere, three inexact squares
    sets.append(0.5 * (pick(k(200)) + pick(k(200))))                                   # midpoints of vertex pairs
    sets.append(rng.uniform(-3, 3, (k(300), 3)))
    lo, hi = v64.min(0), v64.max(0)
    cell = max(1.001 * thr, (hi - lo).max() / (MAX_DIM - 2) * 1.0001)
    out = rng.uniform(lo - cell, hi + cell, (k(300), 3))                               # up to three cells outside each face
    face = rng.randint(0, 6, len(out))
    depth = rng.uniform(0, 3, len(out)) * cell
    for i, (f, d) in enumerate(zip(face, depth)):
        out[i, f % 3] = lo[f % 3] - d if f < 3 else hi[f % 3] + d
    sets.append(out)
    sp = []
    for s in SPECIALS:
        for c in range(3):
            p = v64[rng.randint(0, V)].copy()
            p[c] = s
            sp.append(p)
    sp += [np.full(3, np.nan), np.full(3, -0.0), np.array([np.inf, -np.inf, 1e30])]
    sets.append(np.array(sp))
    with np.errstate(over="ignore"):
        pts = np.concatenate(sets).astype(F)
    if extra is not None:
        pts = np.concatenate([np.asarray(extra, F), pts])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


def _assert_discriminating(name, pts, verts, thr, ref, ties, threshold_hits):
    share = float(ref["valid"].mean())
    assert 0.05 < share < 0.95, (name, "valid share", share)
    if ties:
        assert int((ref["valid"] & (ref["ties"] > 1)).sum()) > 0, (name, "no valid point with an exact winner tie")
    if threshold_hits:
        assert int((ref["best"] == thr2_of(thr)).sum()) > 0, (name, "no point at dist == thr^2")


@functools.lru_cache(maxsize=None)
def case(name):
    """one body with its transforms, points and exact reference: dict(verts, thr, T_inv, pts, ref)"""
    verts, thr = make_body(name)
    T_inv = make_T_inv(len(verts), BODIES.index(name))
    pts = make_points(verts, thr, BODIES.index(name), extra=margin_points() if name == "margin" else None)
    assert len(pts) <= P_CAP
    ref = nn_exact(pts, verts, T_inv, thr)
    _assert_discriminating(name, pts, verts, thr, ref, name in TIE_BODIES, name == "lattice400")
    for a in (verts, T_inv, pts) + tuple(ref.values()):
        a.setflags(write=False)
    return dict(name=name, verts=verts, thr=thr, T_inv=T_inv, pts=pts, ref=ref)


@functools.lru_cache(maxsize=None)
def staging_case(n_verts, P=STAGING_P):
    verts, thr = staging_body(n_verts)
    T_inv = make_T_inv(n_verts, 100 + n_verts % 89)
    pts = make_points(verts, thr, 200 + n_verts % 89, scale=P / 2800.0)
    pts = np.ascontiguousarray(np.concatenate([verts[-3:], pts])[:P])    # the tail of the unrolled loop owns a nearest vertex
    ref = nn_exact(pts, verts, T_inv, thr)
    assert ref["valid"].any() and not ref["valid"].all(), n_verts
    for a in (verts, T_inv, pts) + tuple(ref.values()):
        a.setflags(write=False)
    return dict(name="staging%d" % n_verts, verts=verts, thr=thr, T_inv=T_inv, pts=pts, ref=ref)


@functools.lru_cache(maxsize=None)
def big_case(name, P):
    """the body `name` with at least P points (the sharded-encoder case of the fused query)"""
    verts, thr = make_body(name)
    T_inv = make_T_inv(len(verts), BODIES.index(name))
    pts = make_points(verts, thr, 50 + BODIES.index(name), scale=P / 2600.0)
    assert len(pts) >= P, len(pts)
    pts = np.ascontiguousarray(pts[:P])
    ref = nn_exact(pts, verts, T_inv, thr)
    return dict(name=name, verts=verts, thr=thr, T_inv=T_inv, pts=pts, ref=ref)
