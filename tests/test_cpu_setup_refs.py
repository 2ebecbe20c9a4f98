"""tests/setup_refs.py on the CPU: the references of the occupancy build, the occupancy words, the skinning-weight voxelisation and the
mesh signed distance are right (against the oracle and against plain restatements of the kernels), the conditions that keep the GPU
comparisons from passing vacuously hold on the references alone, and every seeded mutant fails the comparison the GPU test makes."""
import numpy as np
import pytest

import setup_refs as sr

F = np.float32
AABB = np.array([-0.83, -1.21, -0.37, 0.91, 0.77, 0.52], F)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- A ---------------------------------------------------------------------------------------------------------------
def test_probe_cell_is_a_permutation_and_morton_at_64():
    for G in (64, 16, 12, 4):
        perm = sr.probe_cell(np.arange(G ** 3), G)
        assert np.array_equal(np.sort(perm), np.arange(G ** 3))
        assert not np.array_equal(perm, np.arange(G ** 3))
    # Morton: the first 8 cells are the 2 x 2 x 2 block at the origin, z moving first
    assert sr.probe_cell(np.arange(8), 64).tolist() == [0, 1, 64, 65, 4096, 4097, 4160, 4161]
    assert sr.probe_cell(np.arange(3), 12).tolist() == [0, 144, 288]          # x fastest


def test_probe_points_follow_the_oracle_formula(oracle):
    G = 12
    jit = sr.density_jitter(G, 3)
    assert (jit == 0).sum() > 10 and (jit == sr.ONE_BELOW).sum() > 10 and jit.max() < 1
    pts = sr.probe_points_grid(jit, G, AABB)
    idx = np.arange(G, dtype=F)
    c0 = (np.stack(np.meshgrid(idx, idx, idx, indexing="ij"), -1).reshape(-1, 3) / F(G)).astype(F)       # oracle.density_grid_initialize
    for it in range(3):
        want = (c0 + jit[it] / F(G)) * (AABB[3:] - AABB[:3]) + AABB[:3]
        assert np.array_equal(_bits(pts[it]), _bits(want))


@pytest.mark.parametrize("G,iters", sr.DENSITY_CASES)
def test_density_init_emulation_equals_the_grid_order_reference(G, iters):
    jit = sr.density_jitter(G, iters)
    ref, per_set = sr.density_ref_hash(jit, G, AABB)
    assert (ref > 0).any() and all(c > 0 for c in sr.sets_that_win_strictly(per_set))
    for route in ("batched", "small"):
        got = sr.density_init_emulated(jit, G, AABB, route)
        assert np.array_equal(_bits(got), _bits(ref)), route
    for mutant in sr.DENSITY_MUTANTS:
        for route in ("batched", "small"):
            on_small_only = mutant in ("small_scatter_p", "no_accumulate")
            if (on_small_only and route == "batched") or (mutant == "morton_xz_max" and G != 64) or (mutant == "no_accumulate" and iters == 1) \
                    or (mutant == "sum_then_div" and G & (G - 1) == 0):     # (a division by a power of two commutes with the rounding)
                continue
            got = sr.density_init_emulated(jit, G, AABB, route, mutant=mutant)
            assert not np.array_equal(_bits(got), _bits(ref)), (mutant, route)


def test_every_density_mutant_is_killed_somewhere():
    killed = set()
    for G, iters in sr.DENSITY_CASES:
        for m in sr.DENSITY_MUTANTS:
            if not (m == "morton_xz_max" and G != 64) and not (m == "no_accumulate" and iters == 1) and not (m == "sum_then_div" and G & (G - 1) == 0):
                killed.add(m)
    assert killed == set(sr.DENSITY_MUTANTS)


# ---- B ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (4, 12, 20))
def test_occupancy_cases_are_not_vacuous(oracle, G):
    cases = sr.occupancy_cases(G)
    n_on = {}
    for what, dens in cases.items():
        occ = oracle.occupancy_from_density(dens, G).astype(bool)
        words = sr.pack_with_tail(occ)
        assert np.array_equal(sr.unpack_words(words, G), occ) and len(words) == G ** 3 // 32 + 7
        n_on[what] = int(occ.sum())
        if what.startswith("face"):
            axis, side = int(what[5]), what[6]
            cells = np.argwhere(occ)
            assert words[G ** 3 // 32] == 0 and (cells[:, axis].min() == 0 if side == "-" else cells[:, axis].max() == G - 1), what
    assert n_on["empty"] == 0 and n_on["dense"] > 0
    if G != 4:
        assert (G ** 3) % 256 != 0
        assert 0 < n_on["blob + small"] < G ** 3 and n_on["tie"] == 27
        d = cases["blob + small"]
        big = oracle.occupancy_from_density(d, G).astype(bool)
        assert not big[G - 3, G - 3, G - 3] and d[G - 3, G - 3, G - 3] > 0           # the smaller component is dropped
        assert sr.pack_with_tail(big)[G ** 3 // 32] == 1


def test_pack_cases_128():
    cases = sr.pack_cases_128()
    n_words = 128 ** 3 // 32
    assert n_words // 4 > 2 * 1024
    w = sr.pack_with_tail(cases["nowhere"])
    assert not w[:n_words].any() and w[n_words:].tolist() == [1, 0x7fffffff, -1, 0x7fffffff, -1, 0x7fffffff, -1]
    w = sr.pack_with_tail(cases["last word"])
    assert not w[:n_words - 1].any() and w[n_words - 1] != 0 and w[n_words:].tolist() == [0, 127, 127, 127, 127, 96, 127]
    w = sr.pack_with_tail(cases["first word"])
    assert not w[1:n_words].any() and w[0] != 0 and w[n_words:].tolist() == [0, 0, 0, 0, 0, 1, 30]


# ---- C ---------------------------------------------------------------------------------------------------------------
def _tie_fraction(case):
    d = np.sort(sr.sqdist32(case["pts"], case["verts"]), axis=1)
    return float((d[:, sr.KNN_K - 1] == d[:, sr.KNN_K]).mean())


def test_knn_reference_against_the_oracle_and_the_streaming_selection(oracle):
    cases = [sr.tie_case(), sr.voxel_case((3, 4, 5), 31), sr.voxel_case((3, 3, 3), 2049), sr.voxel_case((3, 4, 5), 4100)]
    for case in cases:
        d, i = sr.knn_ref(case["pts"], case["verts"])
        do, io = oracle.knn(case["pts"], case["verts"])
        assert np.array_equal(i, io) and np.array_equal(_bits(d), _bits(do))
        de, ie = sr.knn_emulated(case["pts"], case["verts"])
        assert np.array_equal(i, ie) and np.array_equal(_bits(d), _bits(de))


def test_voxel_cases_reach_what_they_are_for():
    tie = sr.tie_case()
    assert _tie_fraction(tie) >= 0.25
    d, i = sr.knn_ref(tie["pts"], tie["verts"])
    assert (d[:, 0] == 0).any() and (d[:, -1] > 1).any()                   # both clamps
    assert len(np.unique(tie["verts"], axis=0)) == 64 and len(tie["verts"]) == 88
    for grid in sr.VOX_GRIDS:
        _, i = sr.knn_ref(**{k: sr.voxel_case(grid, 2049)[k] for k in ("pts", "verts")})
        assert (i[:, 0] == 2048).any(), grid
        _, i = sr.knn_ref(**{k: sr.voxel_case(grid, 4100)[k] for k in ("pts", "verts")})
        chunks = i // sr.KNN_CHUNK
        assert any(set(row) == {0, 1, 2} for row in chunks.tolist()), grid
    assert [g[0] * g[1] * g[2] for g in sr.VOX_GRIDS] == [27, 60, 480]


def test_blend_bound_holds_for_the_float32_restatement_and_sees_one_wrong_neighbour():
    worst = 0.0
    for case in (sr.tie_case(), sr.voxel_case((5, 8, 12), 31), sr.voxel_case((3, 4, 5), 2049), sr.voxel_case((3, 3, 3), 30)):
        d, i = sr.knn_ref(case["pts"], case["verts"])
        ref, M = sr.blend_ref64(d, i, case["vw"])
        bound = sr.blend_bound(M)
        got = sr.blend_fp32(d, i, case["vw"])
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= bound).all() and (got[bound == 0] == 0).all() and (bound == 0).any()
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert abs(ref.sum(0) - 1).max() < 1e-6
        # one wrong neighbour (the 30th replaced by the 31st where there is one): far outside the bound
        if len(case["verts"]) > sr.KNN_K:
            d31, i31 = sr.knn_ref(case["pts"], case["verts"], K=31)
            i_bad = i.copy(); i_bad[:, -1] = i31[:, -1]
            bad, _ = sr.blend_ref64(d, i_bad, case["vw"])
            assert (np.abs(bad - ref) > 20 * bound).any(axis=0).mean() > 0.9
    print("RATIO blend fp32 restatement %.3f" % worst)
    assert 0 < worst <= 1


@pytest.mark.parametrize("mutant", sr.KNN_MUTANTS)
def test_knn_mutants_fail(mutant):
    case = sr.tie_case()
    d, i = sr.knn_ref(case["pts"], case["verts"])
    dm, im = sr.knn_emulated(case["pts"], case["verts"], mutant=mutant)
    assert not np.array_equal(i, im)                # the neighbour lists differ ...
    assert np.array_equal(_bits(d), _bits(dm))      # ... and only in which of the equally distant vertices they hold
    ref, bound = sr.voxelise_ref(case)
    got, _ = sr.voxelise_ref(case, mutant=mutant)
    out_of_bound = (np.abs(got - ref) > bound).any()
    if mutant == "sort_desc_index":
        # the same SET in another order: the blend is a sum over the set, so no comparison of the entry's output can (or need) see it;
        # it is the returned order that differs from knn_points', which the comparison of the lists above rejects
        assert np.array_equal(np.sort(i, 1), np.sort(im, 1)) and not out_of_bound
    else:
        assert out_of_bound


@pytest.mark.parametrize("mutant", sr.SMOOTH_MUTANTS)
def test_smooth_mutants_fail(mutant):
    for grid in sr.VOX_GRIDS:
        case = sr.voxel_case(grid, 31)
        w0 = sr.blend_fp32(*sr.knn_ref(case["pts"], case["verts"]), case["vw"])
        for n_smooth in (1, 2, 5):
            ref = sr.smooth_ref32(w0, grid, n_smooth)
            assert not np.array_equal(_bits(sr.smooth_ref32(w0, grid, n_smooth, mutant=mutant)), _bits(ref)), (grid, n_smooth)


def test_smoothing_reference_against_float64_and_at_the_border():
    grid = (5, 8, 12)
    case = sr.voxel_case(grid, 2048)
    w0 = sr.blend_fp32(*sr.knn_ref(case["pts"], case["verts"]), case["vw"])
    assert np.array_equal(_bits(sr.smooth_ref32(w0, grid, 0)), _bits(w0))
    a = w0.astype(np.float64).reshape(24, *grid)
    for _ in range(2):                              # deformer_torch.py:237-243 in float64
        mean = (a[:, 2:, 1:-1, 1:-1] + a[:, :-2, 1:-1, 1:-1] + a[:, 1:-1, 2:, 1:-1] + a[:, 1:-1, :-2, 1:-1] + a[:, 1:-1, 1:-1, 2:] + a[:, 1:-1, 1:-1, :-2]) / 6
        a = a.copy()
        a[:, 1:-1, 1:-1, 1:-1] = (a[:, 1:-1, 1:-1, 1:-1] - mean) * 0.7 + mean
        a = a / a.sum(0, keepdims=True)
    got = sr.smooth_ref32(w0, grid, 2).reshape(24, *grid)
    assert np.abs(got - a).max() < 40 * sr.U
    one = sr.smooth_ref32(w0, grid, 1).reshape(24, *grid)
    border = np.ones(grid, bool); border[1:-1, 1:-1, 1:-1] = False
    s = np.zeros(grid, F)
    for c in range(24):
        s = s + w0.reshape(24, *grid)[c]
    assert np.array_equal(_bits(one[:, border]), _bits((w0.reshape(24, *grid) / s)[:, border]))       # border voxels: renormalised only


# ---- D ---------------------------------------------------------------------------------------------------------------
def test_cell_centres_reference():
    for G in sr.CENTRE_GS:
        c = sr.cell_centres_ref(G, sr.CENTRE_AABB)
        lo, hi = sr.CENTRE_AABB[:3].astype(np.float64), sr.CENTRE_AABB[3:].astype(np.float64)
        want = (sr.cell_index3(np.arange(G ** 3), G) + 0.5) / G * (hi - lo) + lo
        assert c.dtype == F and np.abs(c - want).max() < 8 * sr.U * 2.3
    # the two-division form is not the fused one bit for bit
    G = 33
    idx = sr.cell_index3(np.arange(G ** 3), G).astype(F)
    fused = ((idx + F(0.5)) / F(G)) * (sr.CENTRE_AABB[3:] - sr.CENTRE_AABB[:3]) + sr.CENTRE_AABB[:3]
    assert not np.array_equal(_bits(fused), _bits(sr.cell_centres_ref(G, sr.CENTRE_AABB)))


def test_shapes_are_closed_and_sized():
    for shape, n_faces in (("cube1", 12), ("cube10", 1200), ("cube14", 2352), ("octahedron", 8), ("prism", 20)):
        verts, faces = sr.shape_mesh(shape)
        assert len(faces) == n_faces and faces.max() == len(verts) - 1
        e = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
        key, count = np.unique(np.sort(e, 1), axis=0, return_counts=True)
        assert (count == 2).all(), shape                                   # every edge shared by exactly two faces
        v = verts[faces].astype(np.float64)
        assert (np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1) > 0).all()
        assert (classify_on_surface(shape, verts)).all()
    assert sr.IA_MESH_CHUNK < 1200 < 2 * sr.IA_MESH_CHUNK < 2352 < 3 * sr.IA_MESH_CHUNK


def classify_on_surface(shape, p):
    return sr.classify(shape, p) == 0


_EXP = {}


def _exp(shape):
    if shape not in _EXP:
        _EXP[shape] = sr.sdf_expectation(shape)
    return _EXP[shape]


@pytest.mark.parametrize("shape", ("cube1", "cube4", "cube10", "octahedron", "prism"))
def test_the_kernels_twin_gives_the_analytic_sign_and_distance(oracle, shape):
    exp = _exp(shape)
    verts, faces = sr.shape_mesh(shape)
    fv = sr.lattice_to_float(verts)
    n_off, n_on, n_zs = int((exp["sign"] != 0).sum()), int((exp["sign"] == 0).sum()), int((exp["zero_sign"] != 0).sum())
    assert n_off > 3500 and n_on > 100 and n_zs > 50 and (exp["sign"] < 0).sum() > 100
    assert (exp["zero_sign"] < 0).any() and (exp["zero_sign"] > 0).any()
    for name, f in sr.mesh_variants(verts, faces).items():
        sdf = oracle.mesh_signed_distance(exp["pts"], fv, f)
        err, allow, ratio = sr.sdf_compare(sdf, exp)
        assert ratio <= 1
        assert np.array_equal(sr.sign_emulated(exp["pts"], fv, f), np.where(np.signbit(sdf), -1, 1)), name
    print("RATIO sdf twin %s: %d off, %d on the surface, max error %.3g allowance %.3g ratio %.3f" % (shape, n_off, n_on, err, allow, ratio))


@pytest.mark.parametrize("mutant", sr.SDF_MUTANTS)
def test_sdf_mutants_fail(mutant):
    killed = 0
    for shape in ("cube1", "cube10", "octahedron", "prism"):
        exp = _exp(shape)
        verts, faces = sr.shape_mesh(shape)
        fv = sr.lattice_to_float(verts)
        for name, f in sr.mesh_variants(verts, faces).items():
            sign = sr.sign_emulated(exp["pts"], fv, f, mutant=mutant)
            dist = exp["dist"]
            if mutant == "drop_partial_stage" and len(f) < sr.IA_MESH_CHUNK:      # (no face left: the distance stays at its start value)
                dist = np.full(len(sign), 3.0e38)
            sdf = (sign * dist).astype(F)
            sdf[(dist == 0) & (sign < 0)] = F(-0.0)
            try:
                sr.sdf_compare(sdf, exp)
            except AssertionError:
                killed += 1
    print("mutant %s: rejected on %d of 16 meshes" % (mutant, killed))
    assert killed >= (16 if mutant == "drop_partial_stage" else 4), killed


def test_ray_edge_cases_are_on_the_lattice():
    """the lattice puts rays through vertices, along edges and through shared interior edges: count the off-surface queries whose
    +x ray meets a mesh vertex or an edge's (y, z) projection exactly"""
    for shape in ("cube10", "octahedron", "prism"):
        exp = _exp(shape)
        verts, faces = sr.shape_mesh(shape)
        off = exp["lat"][exp["sign"] != 0]
        vy = {(int(v[1]), int(v[2])) for v in verts}
        through_vertex = sum((int(p[1]), int(p[2])) in vy and (verts[(verts[:, 1] == p[1]) & (verts[:, 2] == p[2]), 0] > p[0]).any() for p in off)
        assert through_vertex > 10, (shape, through_vertex)
