"""References, seeded cases and bounds for the once-per-frame and once-per-subject kernels (numpy only: no GPU, no product import):

  A  ia_density_grid_init        the probe points in the grid's own [x][y][z] order, operation for operation in float32, and a
                                 restatement of the kernels' index plumbing (ia_probe_cell, the cell-major probe order, the jitter index,
                                 both workspace routes) on a seeded hash as the per-point density
  B  the occupancy post-process  flag word, bounds words and bit words of a boolean grid
  C  ia_voxelise_weights         the 30 nearest under the order (d, index) exactly in float32, the blend in float64 with a counted bound,
                                 the smoothing passes bit for bit in float32
  D  ia_grid_cell_centres,       cell centres bit for bit; closed shapes on a dyadic lattice whose interior is known in closed form (integers),
     ia_mesh_signed_distance     a float64 closest-point distance and the bound on the kernel's float32 one

The library is built with -ffp-contract=off and `/` is the IEEE division, so float32 numpy with one rounding per spelled operation
restates every + - * / of these kernels bit for bit.  sqrtf is taken at 1 ulp (2 u relative) from the HIP math table, as in
tests/train_step_refs.py.  Every bound below is counted from the kernel source; nothing in a bound comes from a kernel's output.
tests/test_cpu_setup_refs.py shows that the references are right and that the seeded mutants fail; tests/test_gpu_setup_kernels.py runs
the entries."""
import numpy as np

U = 2.0 ** -24
F = np.float32
SENT_F = F(-7777.0)
SENT_B = 0xA5                       # prefill of byte buffers and workspaces
SENT_W = np.int32(0x5A5A5A5A)       # prefill of the bit grid
IA_ERR_WORKSPACE = -3


# ======================================================================================================================
# A. ia_density_grid_init
# ======================================================================================================================
DENSITY_CASES = ((64, 1), (64, 2), (16, 5), (12, 3))     # (G, iters)
DENSITY_MUTANTS = ("small_scatter_p", "jitter_p_over_iters", "morton_xz_max", "no_accumulate", "sum_then_div")
ONE_BELOW = np.nextafter(F(1), F(0))                     # 0.99999994


def probe_cell(c, G, swap_xz=False):
    """ia_probe_cell: cell (grid index [x][y][z], z fastest) of the c-th cell in probe order -- Morton for G = 64, x fastest otherwise"""
    c = np.asarray(c, np.int64)
    if G == 64:
        x, y, z = np.zeros_like(c), np.zeros_like(c), np.zeros_like(c)
        for b in range(6):
            z |= ((c >> (3 * b)) & 1) << b
            y |= ((c >> (3 * b + 1)) & 1) << b
            x |= ((c >> (3 * b + 2)) & 1) << b
        if swap_xz:
            x, z = z, x
        return (x * G + y) * G + z
    x, y, z = c % G, c // G % G, c // (G * G)
    return (x * G + y) * G + z


def cell_index3(i, G):
    i = np.asarray(i, np.int64)
    return np.stack([i // (G * G), i // G % G, i % G], -1)


def _denorm(idx3, jit, G, aabb, fused_div=False):
    """c0 = fl(idx / G); c = fl(c0 + fl(jit / G)); p = fl(fl(c * fl(hi - lo)) + lo)"""
    aabb = np.asarray(aabb, F).reshape(6)
    lo, hi = aabb[:3], aabb[3:]
    idx = idx3.astype(F)
    g = F(G)
    if fused_div:
        c = (idx + jit) / g
    else:
        c0 = idx / g
        c = c0 + jit / g
    out = c * (hi - lo) + lo
    assert out.dtype == F
    return out


def probe_points_grid(jit, G, aabb):
    """the probe points of every set in the grid's own order: [iters, G^3, 3] float32"""
    jit = np.asarray(jit, F)
    n = G ** 3
    assert jit.shape[1:] == (n, 3)
    return _denorm(cell_index3(np.arange(n), G)[None], jit, G, aabb)


def density_jitter(G, iters):
    """seeded jitter in [0, 1) with entries set to 0.0 and to 0.99999994"""
    rng = np.random.RandomState(1000 * G + iters)
    jit = rng.rand(iters, G ** 3, 3).astype(F)
    jit[jit >= 1] = ONE_BELOW
    flat = jit.reshape(-1)
    pick = rng.permutation(flat.size)[:max(64, flat.size // 50)]
    flat[pick[0::2]] = F(0)
    flat[pick[1::2]] = ONE_BELOW
    return jit


def hash_density(pts):
    """a seeded per-point density from the point's float32 bits (CPU stand-in for search + field): about a quarter positive"""
    b = np.ascontiguousarray(pts, F).reshape(-1, 3).view(np.uint32).astype(np.uint64)
    m = np.uint64(0xffffffff)
    h = ((b[:, 0] * np.uint64(0x9E3779B1)) & m) ^ ((b[:, 1] * np.uint64(0x85EBCA77)) & m) ^ ((b[:, 2] * np.uint64(0xC2B2AE3D)) & m)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & m
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & m
    h ^= h >> np.uint64(15)
    val = ((h & np.uint64(0xffff)).astype(np.float64) / 65536.0 * 300.0 + 0.5).astype(F)
    return np.where(((h >> np.uint64(16)) & np.uint64(3)) == 0, val, F(0)).astype(F)


def density_from_sets(per_set):
    """density_ref = max(0, max over the sets); per_set [iters, n]"""
    d = np.zeros(per_set.shape[1], F)
    for s in per_set:
        d = np.maximum(d, np.asarray(s, F))
    return d


def density_ref_hash(jit, G, aabb):
    pts = probe_points_grid(jit, G, aabb)
    per_set = np.stack([hash_density(p) for p in pts])
    return density_from_sets(per_set), per_set


def sets_that_win_strictly(per_set):
    """for every probe set: the number of cells whose maximum comes strictly from that set"""
    per_set = np.asarray(per_set)
    out = []
    for s in range(len(per_set)):
        others = np.delete(per_set, s, 0)
        rest = np.maximum(others.max(0), 0) if len(others) else np.zeros(per_set.shape[1], per_set.dtype)
        out.append(int((per_set[s] > rest).sum()))
    return out


def density_init_emulated(jit, G, aabb, route, dens_fn=hash_density, mutant=None):
    """k_probe_points -> per-point density -> k_probe_max as ia_density_grid_init launches them on its two workspace routes"""
    assert route in ("batched", "small") and mutant in (None,) + DENSITY_MUTANTS
    jit = np.asarray(jit, F)
    iters, n = jit.shape[:2]
    density = np.full(n, SENT_F, F)

    def k_probe_points(jitter, iters_k):          # jitter [iters_k][n cells][3]
        p = np.arange(n * iters_k)
        it, i = p % iters_k, probe_cell(p // iters_k, G)
        jcell = p // iters_k if mutant == "jitter_p_over_iters" else i
        return _denorm(cell_index3(i, G), jitter[it, jcell], G, aabb, fused_div=mutant == "sum_then_div")

    def k_probe_max(sig, iters_k, accumulate, scatter_p=False):
        c = np.arange(n)
        i = c if scatter_p else probe_cell(c, G, swap_xz=mutant == "morton_xz_max")
        m = density[i].copy() if accumulate else np.zeros(n, F)
        for it in range(iters_k):
            m = np.maximum(m, sig[c * iters_k + it])
        density[i] = m

    if route == "batched":
        k_probe_max(dens_fn(k_probe_points(jit, iters)), iters, False)
    else:
        density[:] = 0
        for it in range(iters):
            k_probe_max(dens_fn(k_probe_points(jit[it:it + 1], 1)), 1, mutant != "no_accumulate", scatter_p=mutant == "small_scatter_p")
    return density


# ======================================================================================================================
# B. occupancy words
# ======================================================================================================================
def pack_with_tail(occ):
    """bit words of a boolean [G,G,G] grid (bit b of word w = cell 32 w + b), the flag word (1 = no border cell occupied) and the six
    bounds words {x_min, x_max, y_min, y_max, z_min, z_max} (min > max when nothing is occupied): int32 [G^3 / 32 + 7]"""
    occ = np.asarray(occ).astype(bool)
    G = occ.shape[0]
    words = (occ.reshape(-1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)
    border = occ.copy()
    border[1:-1, 1:-1, 1:-1] = False
    cells = np.argwhere(occ)
    bounds = [v for c in range(3) for v in ((int(cells[:, c].min()), int(cells[:, c].max())) if len(cells) else (0x7fffffff, -1))]
    tail = np.array([0 if border.any() else 1] + bounds, np.int64).astype(np.uint32)
    return np.concatenate([words, tail]).view(np.int32)


def unpack_words(words, G):
    w = np.asarray(words).view(np.uint32)[:G ** 3 // 32]
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(G, G, G).astype(bool)


def occupancy_cases(G):
    """adversarial densities for a small grid: name -> float32 [G,G,G]"""
    rng = np.random.RandomState(40 + G)
    out = {}
    if G == 4:
        d = np.zeros((G, G, G), F); out["empty"] = d
        d = np.zeros((G, G, G), F); d[0, 0, 0] = 80; out["corner"] = d
        d = np.zeros((G, G, G), F); d[3, 3, 3] = 80; d[0, 0, 0] = 60; out["two corners"] = d
        out["dense"] = (rng.rand(G, G, G) * 100).astype(F)
        return out
    a, b = 2, G // 3
    d = np.zeros((G, G, G), F)
    d[a:b, a:b + 1, a:b + 1] = rng.rand(b - a, b - a + 1, b - a + 1) * 100 + 20            # a blob ...
    d[G - 3, G - 3, G - 3] = 70                                                             # ... and a smaller component
    out["blob + small"] = d
    for axis in range(3):
        for side in (0, 1):
            d = np.zeros((G, G, G), F)
            sl = [slice(a, b)] * 3
            sl[axis] = slice(0, 2) if side == 0 else slice(G - 2, G)
            d[tuple(sl)] = 90
            d[(G - 3 if side == 0 else 2,) * 3] = 50                                        # a smaller one in the far corner
            out["face %d%s" % (axis, "-+"[side])] = d
    d = np.zeros((G, G, G), F); d[2, 2, 2] = 50; d[G - 3, G - 3, G - 3] = 50; out["tie"] = d
    out["empty"] = np.zeros((G, G, G), F)
    out["dense"] = (rng.rand(G, G, G) * 100).astype(F)
    return out


def pack_cases_128():
    """G = 128 through ia_occupancy_pack: n_words / 4 = 16384 > 2 x 1024 threads of k_occ_bounds' power-of-two route"""
    G = 128
    out = {}
    o = np.zeros((G, G, G), bool); out["nowhere"] = o
    o = np.zeros((G, G, G), bool); o.reshape(-1)[-32:] = [1, 0, 0, 1] * 8; out["last word"] = o
    o = np.zeros((G, G, G), bool); o.reshape(-1)[:32] = [0, 1, 1, 0] * 8; out["first word"] = o
    o = np.zeros((G, G, G), bool); o[5, 77, 40:45] = True; o[100, 3, 127] = True; out["two runs"] = o
    return out


# ======================================================================================================================
# C. ia_voxelise_weights
# ======================================================================================================================
KNN_K = 30
KNN_CHUNK = 2048
VOX_GRIDS = ((3, 3, 3), (3, 4, 5), (5, 8, 12))
VOX_NVERTS = (30, 31, 2048, 2049, 4100)
VOX_NSMOOTH = (0, 1, 2, 5)
KNN_MUTANTS = ("evict_smallest_index", "insert_le", "sort_desc_index")
SMOOTH_MUTANTS = ("lerp_03", "mean_mul_sixth", "border_as_interior", "renorm_first")
CLAMP_LO = float(F(0.0001))
# bound of the blend, K u M with M = sum_k w_k |a_kj| of the reference:
#   dd = sqrtf(d)             1 ulp = 2 u relative; the clamp to [1e-4f, 1] is monotone and 1-Lipschitz, it adds nothing
#   w = 1 / dd                u                                             -> 3 u on w
#   wsum                      29 roundings of a sum of positive terms       -> 3 u + 29 u = 32 u on wsum
#   w / wsum                  u                                             -> 36 u on the normalised weight
#   w * a                     u                                             -> 37 u on a term
#   acc += ...                30 terms from 0: the first addition is exact, 29 roundings of partial sums <= M
K_BLEND = 37 + 29


def _weight_rows(rng, n):
    """skinning-like rows [n,24]: four non-zero columns per vertex out of 24, well separated between vertices"""
    vw = np.zeros((n, 24), F)
    for v in range(n):
        cols = rng.permutation(24 if v % 7 == 0 else 20)[:4]      # (the last four columns are rare: some outputs are exactly 0)
        x = rng.rand(4) + 0.2
        vw[v, cols] = (x / x.sum()).astype(F)
    return vw


def voxel_case(grid, n_verts):
    """seeded query points [d*h*w,3], vertices [n_verts,3] and weight rows; at 2049 vertices index 2048 is some voxel's nearest, at
    4100 the four vertices of the third LDS chunk lie beside one voxel"""
    d, h, w = grid
    n = d * h * w
    rng = np.random.RandomState(7 * n + n_verts)
    pts = (rng.rand(n, 3) * 1.6 - 0.8).astype(F)
    verts = (rng.rand(n_verts, 3) * 2.4 - 1.2).astype(F)
    if n_verts > 2048:
        verts[2048] = pts[n // 2] + F(0.001)
    if n_verts > 4096:
        for k, v in enumerate(range(4096, n_verts)):
            verts[v] = pts[n - 1] + np.array([0.002 * (k + 1), -0.001 * k, 0.0015], F)
    return dict(pts=pts, verts=verts, vw=_weight_rows(rng, n_verts), grid=grid)


def tie_case():
    """exact ties: vertices on the lattice {0, 0.5, 1, 1.5}^3 in shuffled order with 24 positions duplicated under other indices and
    weights; 3 x 4 x 5 query points on the same lattice (some on a vertex: clamp at 1e-4; corner points reach d > 1: clamp at 1)"""
    rng = np.random.RandomState(77)
    lat = np.stack(np.meshgrid(*[np.arange(4)] * 3, indexing="ij"), -1).reshape(-1, 3)
    allv = np.concatenate([lat, lat[rng.permutation(64)[:24]]])
    verts = (allv[rng.permutation(len(allv))] * 0.5).astype(F)
    z, y, x = np.meshgrid(np.arange(3), np.arange(4), np.arange(5) - 1, indexing="ij")
    pts = (np.stack([x, y, z], -1).reshape(-1, 3) * 0.5).astype(F)
    return dict(pts=pts, verts=verts, vw=_weight_rows(rng, len(verts)), grid=(3, 4, 5))


def sqdist32(pts, verts):
    """d = fl(fl(fl(dx*dx) + fl(dy*dy)) + fl(dz*dz)) for every pair: [N,V] float32"""
    p, v = np.asarray(pts, F), np.asarray(verts, F)
    dx, dy, dz = (p[:, None, k] - v[None, :, k] for k in range(3))
    return (dx * dx + dy * dy) + dz * dz


def knn_ref(pts, verts, K=KNN_K):
    """the K smallest under the order (d, index), ascending: (d [N,K] float32, index [N,K])"""
    d = sqdist32(pts, verts)
    order = np.argsort(d, axis=1, kind="stable")[:, :K]
    return np.take_along_axis(d, order, 1), order


def knn_emulated(pts, verts, K=KNN_K, mutant=None):
    """k_knn_blend's streaming selection: replace the entry to evict when d < worst, then find the next one to evict (largest d, among
    equals the largest index); selection sort at the end"""
    assert mutant in (None,) + KNN_MUTANTS
    d = sqdist32(pts, verts)
    N, V = d.shape
    sd, si = np.full((N, K), np.inf, F), np.zeros((N, K), np.int64)
    worst, worst_k = np.full(N, np.inf, F), np.zeros(N, np.int64)
    for v in range(V):
        ins = d[:, v] <= worst if mutant == "insert_le" else d[:, v] < worst
        r = np.nonzero(ins)[0]
        if not len(r):
            continue
        sd[r, worst_k[r]] = d[r, v]
        si[r, worst_k[r]] = v
        sub_d, sub_i = sd[r], si[r]
        wmax = sub_d.max(1)
        cand = sub_d == wmax[:, None]
        if mutant == "evict_smallest_index":
            k = np.where(cand, sub_i, 1 << 40).argmin(1)
        else:
            k = np.where(cand, sub_i, -1).argmax(1)
        worst[r], worst_k[r] = wmax, k
    key_i = -si if mutant == "sort_desc_index" else si
    order = np.stack([np.lexsort((key_i[q], sd[q])) for q in range(N)])
    return np.take_along_axis(sd, order, 1), np.take_along_axis(si, order, 1)


def blend_ref64(d30, i30, vw):
    """float64: distance = sqrt(d) clamped to [1e-4f, 1], weights = reciprocals normalised over the 30, output [24,N] and the bound's M"""
    dist = np.clip(np.sqrt(d30.astype(np.float64)), CLAMP_LO, 1.0)
    w = 1.0 / dist
    w /= w.sum(1, keepdims=True)
    rows = np.asarray(vw, np.float64)[i30]
    return np.einsum("nk,nkj->jn", w, rows), np.einsum("nk,nkj->jn", w, np.abs(rows))


def blend_bound(M):
    return K_BLEND * U * M * (1 + K_BLEND * U)


def blend_fp32(d30, i30, vw):
    """plain float32 restatement of k_knn_blend's arithmetic (np.sqrt is correctly rounded)"""
    dd = np.sqrt(d30.astype(F))
    dd = np.where(dd < F(0.0001), F(0.0001), np.where(dd > F(1), F(1), dd)).astype(F)
    w = F(1) / dd
    wsum = np.zeros(len(w), F)
    for k in range(w.shape[1]):
        wsum = wsum + w[:, k]
    acc = np.zeros((len(w), 24), F)
    rows = np.asarray(vw, F)[i30]
    for k in range(w.shape[1]):
        acc = acc + (w[:, k] / wsum)[:, None] * rows[:, k]
    return acc.T.copy()


def voxelise_ref(case, mutant=None):
    """(float64 blend [24,N], bound [24,N]) of a case, neighbours from knn_ref (or a mutant of the selection)"""
    d30, i30 = knn_ref(case["pts"], case["verts"]) if mutant is None else knn_emulated(case["pts"], case["verts"], mutant=mutant)
    ref, M = blend_ref64(d30, i30, case["vw"])
    return ref, blend_bound(M)


def smooth_ref32(w0, grid, n_smooth, mutant=None):
    """k_smooth x n_smooth in float32 from [24, d*h*w]: interior voxels (val - mean) * 0.7f + mean with mean = the six neighbours added
    in the kernel's order (z+1, z-1, y+1, y-1, x+1, x-1) / 6.0f; every voxel divided by its sum taken in channel order"""
    assert mutant in (None,) + SMOOTH_MUTANTS
    d, h, w = grid
    n = d * h * w
    a = np.array(w0, F).reshape(24, n)
    i = np.arange(n)
    z, y, x = i // (h * w), i // w % h, i % w
    interior = (z > 0) & (z < d - 1) & (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    if mutant == "border_as_interior":
        interior = np.ones(n, bool)
    pad = h * w
    for _ in range(n_smooth):
        if mutant == "renorm_first":
            s = np.zeros(n, F)
            for c in range(24):
                s = s + a[c]
            a = a / s
        p = np.zeros((24, n + 2 * pad), F)
        p[:, pad:pad + n] = a
        nb = lambda o: p[:, pad + o:pad + o + n]
        tot = ((((nb(h * w) + nb(-h * w)) + nb(w)) + nb(-w)) + nb(1)) + nb(-1)
        mean = tot * F(1.0 / 6.0) if mutant == "mean_mul_sixth" else tot / F(6.0)
        moved = a * F(0.7) + mean * F(0.3) if mutant == "lerp_03" else (a - mean) * F(0.7) + mean
        v = np.where(interior[None], moved, a).astype(F)
        s = np.zeros(n, F)
        for c in range(24):
            s = s + v[c]
        a = v / s
        assert a.dtype == F
    return a


# ======================================================================================================================
# D. ia_grid_cell_centres, ia_mesh_signed_distance
# ======================================================================================================================
CENTRE_GS = (5, 12, 33)
CENTRE_AABB = np.array([-1.3, -0.7, 0.1, 0.9, 2.3, 1.7], F)       # anisotropic, non-dyadic
SDF_NS = (1, 255, 257)
SDF_MUTANTS = ("closed_edges", "no_orientation_flip", "x_ge", "drop_partial_stage")
IA_MESH_CHUNK = 1024
LATTICE = 17                # integer coordinates 0 .. 16; the float32 coordinate of k is (k - 8) / 8


def cell_centres_ref(G, aabb):
    """fl(fl(fl(idx / G) + fl(0.5 / G)) * fl(hi - lo)) + lo, float32"""
    aabb = np.asarray(aabb, F).reshape(6)
    idx = cell_index3(np.arange(G ** 3), G).astype(F)
    c = idx / F(G) + F(0.5) / F(G)
    out = c * (aabb[3:] - aabb[:3]) + aabb[:3]
    assert out.dtype == F
    return out


def lattice_to_float(k):
    return ((np.asarray(k, np.float64) - 8.0) / 8.0).astype(F)


def lattice_points():
    g = np.arange(LATTICE)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


CUBE_CUTS = {1: (1, 15), 4: (1, 4, 8, 12, 15), 10: (1, 2, 4, 5, 7, 8, 9, 11, 12, 14, 15), 14: tuple(range(1, 16))}


def cube_mesh(k):
    """the cube [1, 15]^3 (lattice units) with each face split k x k along CUBE_CUTS[k]: 12 k^2 faces, shared vertices"""
    cuts = CUBE_CUTS[k]
    assert len(cuts) == k + 1
    index, faces = {}, []

    def vid(p):
        return index.setdefault(tuple(p), len(index))

    for axis in (2, 1, 0):                  # (the faces that the +x rays cross come last: a dropped last stage changes the parity)
        u, v = [a for a in range(3) if a != axis]
        for side in (cuts[0], cuts[-1]):
            for a in range(k):
                for b in range(k):
                    def P(s, t):
                        p = [0, 0, 0]
                        p[axis], p[u], p[v] = side, cuts[s], cuts[t]
                        return vid(p)
                    q = [P(a, b), P(a + 1, b), P(a + 1, b + 1), P(a, b + 1)]
                    if (a + b) & 1:
                        faces += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
                    else:
                        faces += [[q[0], q[1], q[3]], [q[1], q[2], q[3]]]
    verts = np.array(sorted(index, key=index.get), np.int64)
    return verts, np.array(faces, np.int32)


def _classify_box(p, lo, hi):
    """-1 strictly inside, 0 on the boundary, +1 outside of the closed box [lo, hi] (integers)"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    inside = ((p > lo) & (p < hi)).all(-1)
    closed = ((p >= lo) & (p <= hi)).all(-1)
    return np.where(inside, -1, np.where(closed, 0, 1))


OCTA_C, OCTA_R = 8, 6
PRISM_L = ((2, 2), (14, 2), (14, 8), (8, 8), (8, 14), (2, 14))     # the L in (x, y), extruded over z in [3, 13]
PRISM_Z = (3, 13)


def octahedron_mesh():
    c, r = OCTA_C, OCTA_R
    verts = np.array([[c + r, c, c], [c - r, c, c], [c, c + r, c], [c, c - r, c], [c, c, c + r], [c, c, c - r]], np.int64)
    faces = [[x, y, z] for x in (0, 1) for y in (2, 3) for z in (4, 5)]
    return verts, np.array(faces, np.int32)


def prism_mesh():
    """L-shaped prism, the union of the boxes [2,14]x[2,8] and [2,8]x[2,14] over z in [3,13]: 20 faces without T-junctions"""
    z0, z1 = PRISM_Z
    verts = np.array([[x, y, z] for z in (z0, z1) for x, y in PRISM_L], np.int64)
    cap = [[0, 1, 2], [0, 2, 3], [0, 3, 5], [5, 3, 4]]            # vertex 0 = (2,2), 3 = (8,8), 5 = (2,14): the L as four triangles
    faces = [t for t in cap] + [[a + 6, b + 6, c + 6] for a, b, c in cap]
    for e in range(6):
        a, b = e, (e + 1) % 6
        faces += [[a, b, b + 6], [a, b + 6, a + 6]]
    return verts, np.array(faces, np.int32)


def classify(shape, p2, scale=1):
    """exact inside test in integers: -1 inside, 0 on the surface, +1 outside.  `p2` are lattice coordinates times `scale`"""
    p = np.asarray(p2, np.int64)
    s = scale
    if shape.startswith("cube"):
        return _classify_box(p, [1 * s] * 3, [15 * s] * 3)
    if shape == "octahedron":
        m = np.abs(p - OCTA_C * s).sum(-1)
        return np.sign(m - OCTA_R * s).astype(np.int64)
    if shape == "prism":
        z0, z1 = PRISM_Z
        a = _classify_box(p, [2 * s, 2 * s, z0 * s], [14 * s, 8 * s, z1 * s])
        b = _classify_box(p, [2 * s, 2 * s, z0 * s], [8 * s, 14 * s, z1 * s])
        closed = (a <= 0) | (b <= 0)
        # strictly inside the union: inside a box, or on the wall the boxes share (y = 8, 2 < x < 8, z inside)
        shared = (p[..., 1] == 8 * s) & (p[..., 0] > 2 * s) & (p[..., 0] < 8 * s) & (p[..., 2] > z0 * s) & (p[..., 2] < z1 * s)
        inside = (a < 0) | (b < 0) | shared
        return np.where(inside, -1, np.where(closed, 0, 1))
    raise KeyError(shape)


SDF_SHAPES = ("cube1", "cube10", "cube14", "octahedron", "prism")


def shape_mesh(shape):
    if shape.startswith("cube"):
        return cube_mesh(int(shape[4:]))
    return octahedron_mesh() if shape == "octahedron" else prism_mesh()


def coarse_mesh(shape):
    """the same surface with the fewest faces (for the float64 distance)"""
    return cube_mesh(1) if shape.startswith("cube") else shape_mesh(shape)


def mesh_variants(verts, faces):
    """the same surface: as built, every face reversed, every face's vertices rotated, the faces permuted"""
    rng = np.random.RandomState(len(faces))
    return dict(plain=faces, reversed=faces[:, ::-1].copy(), rotated=np.roll(faces, 1, axis=1).copy(),
                permuted=faces[rng.permutation(len(faces))].copy())


def dist_ref64(pts, verts, faces):
    """closest-point distance in float64 by another route than the kernel's region tests: the foot of the perpendicular where it
    falls inside the triangle, else the nearest of the three edges (clamped segment parameter): [N]"""
    p = np.asarray(pts, np.float64)[:, None, :]
    t = np.asarray(verts, np.float64)[np.asarray(faces)]
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(-1)
    h = ((p - a) * nrm).sum(-1) / nn
    foot = p - h[..., None] * nrm
    def side(u, v):
        return (np.cross(v - u, foot - u) * nrm).sum(-1)
    inside = (side(a, b) >= 0) & (side(b, c) >= 0) & (side(c, a) >= 0)
    best = np.where(inside, np.abs(h) * np.sqrt(nn), np.inf)
    for u, v in ((a, b), (b, c), (c, a)):
        e = v - u
        s = np.clip(((p - u) * e).sum(-1) / (e * e).sum(-1), 0.0, 1.0)
        q = u + s[..., None] * e
        best = np.minimum(best, np.sqrt(((p - q) ** 2).sum(-1)))
    return best.min(1)


# bound of the float32 distance on the lattice.  Coordinates are k / 8 with |k| <= 8, so differences are multiples of 1/8 below 2, dot
# products multiples of 1/64 below 12, the products d_i d_j multiples of 1/4096 below 144 and va, vb, vc and their sum below 2^21 / 4096:
# all exact in float32, so the kernel picks the exact region.  What rounds:
#   edge regions   v = d / (d - d')  u;  v * ab  u |ab| <= 2 u each;  a + ...  u |q| <= u                -> 5 u per component of q
#   face region    denom u, vb * denom u, ab * v u (3 u of |ab v| <= 2: 6 u), the same for ac * w (6 u),
#                  a + ab v  u (|a| + |ab v|) <= 3 u,  + ac w  u |q| <= u                                 -> 16 u per component of q
#   p - q          u |p - q| <= 2 u                                                                       -> 18 u per component
#   the norm moves by at most the length of that perturbation, sqrt(3) 18 u; three squares, two additions (3 u on d^2, 1.5 u on d) and
#   sqrtf at 1 ulp (2 u) are relative to the distance.  The minimum over the triangles keeps the bound.
K_SDF_ABS = np.sqrt(3.0) * 18
K_SDF_REL = 3.5


def sdf_bound(dist):
    return (K_SDF_ABS + K_SDF_REL * np.asarray(dist, np.float64)) * U * (1 + 2.0 ** -10)


def sdf_expectation(shape):
    """queries (float32 [17^3,3]) and what is asserted about them:
      sign      -1 / +1 off the surface, 0 on it (exact, integers)
      zero_sign on the surface: the sign bit the half-open rule must give (-1: inside, +1: outside) = the side of the point half a
                lattice step along +x, which the ray enters first (x > p[0] does not count the surface at the point itself); 0 where
                that point lies on the surface too (the ray runs along a face) and nothing is asserted
      dist      float64 closest-point distance"""
    lat = lattice_points()
    sign = classify(shape, lat)
    ahead = classify(shape, 2 * lat + np.array([1, 0, 0]), scale=2)
    zero_sign = np.where(sign == 0, ahead, 0)
    verts, faces = coarse_mesh(shape)
    pts = lattice_to_float(lat)
    dist = dist_ref64(pts, lattice_to_float(verts), faces)
    assert ((dist == 0) == (sign == 0)).all()
    return dict(lat=lat, pts=pts, sign=sign, zero_sign=zero_sign, dist=dist)


def sdf_compare(sdf, exp, sel=None):
    """the assertions of D on a kernel's (or a twin's) output; returns (max error, its allowance, worst error / allowance)"""
    sdf = np.asarray(sdf, F)
    sel = np.arange(len(exp["sign"])) if sel is None else sel
    sign, zs, dist = exp["sign"][sel], exp["zero_sign"][sel], exp["dist"][sel]
    assert sdf.shape == sign.shape and np.isfinite(sdf).all()
    got_sign = np.where(np.signbit(sdf), -1, 1)
    off = sign != 0
    bad = off & (got_sign != sign)
    assert not bad.any(), ("sign off the surface", int(bad.sum()), exp["lat"][sel][bad][:5].tolist())
    badz = (zs != 0) & (got_sign != zs)
    assert not badz.any(), ("sign bit on the surface", int(badz.sum()), exp["lat"][sel][badz][:5].tolist())
    err, allow = np.abs(np.abs(sdf).astype(np.float64) - dist), sdf_bound(dist)
    k = int(np.argmax(err / allow))
    assert (err <= allow).all(), ("distance", float(err[k]), float(allow[k]), exp["lat"][sel][k].tolist())
    return float(err.max()), float(allow[k]), float(err[k] / allow[k])


def sign_emulated(pts, verts, faces, mutant=None):
    """ray_x_crosses in float64 numpy, the crossing parity as -1 (odd) / +1: [N]"""
    assert mutant in (None,) + SDF_MUTANTS
    faces = np.asarray(faces)
    if mutant == "drop_partial_stage":
        faces = faces[:len(faces) // IA_MESH_CHUNK * IA_MESH_CHUNK]
    p = np.asarray(pts, np.float64)
    if not len(faces):
        return np.ones(len(p), np.int64)
    t = np.asarray(verts, np.float64)[faces]
    a, b, c = t[None, :, 0], t[None, :, 1], t[None, :, 2]
    px, py, pz = p[:, None, 0], p[:, None, 1], p[:, None, 2]

    def edge(u, v):
        e = (v[..., 1] - u[..., 1]) * (pz - u[..., 2]) - (v[..., 2] - u[..., 2]) * (py - u[..., 1])
        tl = np.where(v[..., 2] == u[..., 2], v[..., 1] < u[..., 1], v[..., 2] < u[..., 2])
        return e, tl

    (e0, t0), (e1, t1), (e2, t2) = edge(a, b), edge(b, c), edge(c, a)
    area = (b[..., 1] - a[..., 1]) * (c[..., 2] - a[..., 2]) - (b[..., 2] - a[..., 2]) * (c[..., 1] - a[..., 1])
    s = np.where(area > 0, 1.0, -1.0)
    e0, e1, e2 = e0 * s, e1 * s, e2 * s
    if mutant != "no_orientation_flip":
        t0, t1, t2 = (np.where(area < 0, ~tl, tl) for tl in (t0, t1, t2))
    if mutant == "closed_edges":
        inn = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
    else:
        inn = ((e0 > 0) | ((e0 == 0) & t0)) & ((e1 > 0) | ((e1 == 0) & t1)) & ((e2 > 0) | ((e2 == 0) & t2))
    inn &= area != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (e1 * a[..., 0] + e2 * b[..., 0] + e0 * c[..., 0]) / np.abs(area)
    cross = inn & ((x >= px) if mutant == "x_ge" else (x > px))
    return np.where(cross.sum(1) & 1, -1, 1)
