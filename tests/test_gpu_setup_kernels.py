"""The once-per-frame and once-per-subject entries, each called through the C ABI on plain device tensors against tests/setup_refs.py:

  A  ia_density_grid_init       density BIT FOR BIT against max(0, max over the probe sets) of ia_deform_query on probe points computed on the
                                host in the grid's own order; occ_bool / occ_bits (flag and bounds words included) against the oracle and against
                                ia_occupancy_from_density on that density; both workspace routes, the sizes one byte short of each, occ_bool = NULL
  B  the occupancy post-process at G = 4, 12, 20 (ragged last workgroup, less than one workgroup); ia_occupancy_pack at G = 128
  C  ia_voxelise_weights        the blend against float64 within a counted bound (exact ties included), the smoothing passes bit for bit
  D  ia_grid_cell_centres bit for bit; ia_mesh_signed_distance against exact inside tests and a float64 distance on a dyadic lattice

Every output carries a sentinel tail and every workspace is handed exactly the bytes its *_workspace_bytes function returns, with a
sentinel tail behind them: nothing may be written there.  tests/test_cpu_setup_refs.py shows on the CPU that the references are right
and which mutants these comparisons reject.  Each bounded check prints the worst error, its allowance and their ratio ("RATIO ...",
NOTES.md)."""
import numpy as np
import pytest
import torch

import setup_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
TAIL = 256


def _lib():
    from instantavatar_amd import _lib as L
    return L


def _dev(a):
    return torch.as_tensor(np.array(a, order="C")).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _f32_out(n):
    return torch.full((n + TAIL,), float(sr.SENT_F), device=DEV)


def _u8_out(n):
    return torch.full((n + TAIL,), sr.SENT_B, dtype=torch.uint8, device=DEV)


def _words_out(G):
    return torch.full((G ** 3 // 32 + 8 + TAIL,), int(sr.SENT_W), dtype=torch.int32, device=DEV)


def _tail_intact(t, n, what):
    tail = _np(t[n:])
    fill = {torch.float32: sr.SENT_F, torch.uint8: sr.SENT_B, torch.int32: sr.SENT_W}[t.dtype]
    assert len(tail) >= TAIL and (tail == fill).all(), ("written behind the end", what)


# ---- A ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gw():
    import world as W
    from instantavatar_amd.pipeline import make_batch
    model, body, fp, init = W.build(DEV, 64, 16)
    poses, tr = W.poses()
    model.deformer.prepare_deformer(make_batch(DEV, 64, poses[3], tr[3]))
    bb = model.deformer.get_bbox_deformed()
    aabb = torch.cat([bb[0].reshape(3), bb[1].reshape(3)]).float().contiguous().clone()
    return model, aabb


def _deformer_args(model):
    dfm = model.deformer
    k = len(dfm.deformer.init_bones)
    return dfm.deformer.voxel_J_cl, dfm.tfs.detach().float().contiguous(), dfm.deformer._bones_c, k, dfm.deformer.grid_desc()


def _query_sigma(model, pts):
    """ia_deform_query on [P,3] host points: sigma [P] (max over the candidates, 0 where there is none)"""
    L = _lib()
    vj, tfs, bones, k, grid = _deformer_args(model)
    P = len(pts)
    ws = _u8_out(L.call("ia_query_workspace_bytes", P, k))
    sigma = _f32_out(P)
    L.call("ia_deform_query", _dev(pts), P, None, vj, tfs, bones, k, grid, model.net_coarse.field_desc(P * k), None, sigma, None, ws, ws.numel() - TAIL)
    torch.cuda.synchronize()
    _tail_intact(sigma, P, "ia_deform_query sigma")
    _tail_intact(ws, ws.numel() - TAIL, "ia_deform_query workspace")
    return _np(sigma[:P])


def _grid_init(model, aabb, jit_dev, iters, G, ws_bytes, with_bool=True, expect_error=False):
    """one call of ia_density_grid_init with a workspace of exactly ws_bytes (+ sentinel tail); returns (density, words, occ_bool or
    None) as numpy after checking every tail.  expect_error: the call must raise, with nothing written anywhere; returns the message"""
    L = _lib()
    vj, tfs, bones, k, grid = _deformer_args(model)
    n = G ** 3
    ws = _u8_out(ws_bytes)
    density, words, occ = _f32_out(n), _words_out(G), (_u8_out(n) if with_bool else None)
    args = (jit_dev, iters, G, aabb, vj, tfs, bones, k, grid, model.net_coarse.field_desc(n * k * iters), density, words, occ, ws, ws_bytes)
    if expect_error:
        with pytest.raises(L.IAError) as e:
            L.call("ia_density_grid_init", *args)
        torch.cuda.synchronize()
        for t, name in ((ws, "workspace"), (density, "density"), (words, "occ_bits"), (occ, "occ_bool")):
            _tail_intact(t, 0, name + " after an error return")
        return str(e.value)
    L.call("ia_density_grid_init", *args)
    torch.cuda.synchronize()
    _tail_intact(ws, ws_bytes, "workspace")
    _tail_intact(density, n, "density")
    _tail_intact(words, n // 32 + 8, "occ_bits")
    if with_bool:
        _tail_intact(occ, n, "occ_bool")
    return _np(density[:n]), _np(words[:n // 32 + 7]), (_np(occ[:n]) if with_bool else None)


def _occupancy(G, dens):
    """ia_occupancy_from_density with exactly its workspace: (occ_bool [G,G,G], words [G^3/32 + 7])"""
    L = _lib()
    n = G ** 3
    nbytes = L.call("ia_occupancy_workspace_bytes", G)
    ws, words, occ = _u8_out(nbytes), _words_out(G), _u8_out(n)
    L.call("ia_occupancy_from_density", _dev(np.asarray(dens, F).reshape(-1)), G, words, occ, ws, nbytes)
    torch.cuda.synchronize()
    _tail_intact(ws, nbytes, "occupancy workspace")
    _tail_intact(words, n // 32 + 8, "occ_bits")
    _tail_intact(occ, n, "occ_bool")
    got = _np(occ[:n])
    assert set(np.unique(got).tolist()) <= {0, 1}
    return got.astype(bool).reshape(G, G, G), _np(words[:n // 32 + 7])


@pytest.mark.parametrize("G,iters", sr.DENSITY_CASES)
def test_density_grid_init_bit_for_bit(oracle, gw, G, iters):
    model, aabb = gw
    L = _lib()
    n = G ** 3
    k = len(model.deformer.deformer.init_bones)
    jit = sr.density_jitter(G, iters)
    assert (jit == 0).any() and (jit == sr.ONE_BELOW).any()
    # the reference: probe points on the host (the aabb's bits read back from the tensor passed in), every set through ia_deform_query
    pts = sr.probe_points_grid(jit, G, _np(aabb))
    per_set = np.stack([_query_sigma(model, pts[it]) for it in range(iters)])
    density_ref = sr.density_from_sets(per_set)
    wins = sr.sets_that_win_strictly(per_set)
    occ_ref = oracle.occupancy_from_density(density_ref, G).astype(bool)
    words_ref = sr.pack_with_tail(occ_ref)
    print("density init G %d iters %d: %d cells > 0, %d occupied, strict winners per set %s" % (G, iters, int((density_ref > 0).sum()), int(occ_ref.sum()), wins))
    assert (density_ref > 0).any() and all(c > 0 for c in wins)
    if G == 64:
        assert occ_ref.sum() > 500
    occ_gpu, words_gpu = _occupancy(G, density_ref)
    assert np.array_equal(occ_gpu, occ_ref) and np.array_equal(words_gpu, words_ref)

    small = L.call("ia_density_init_workspace_bytes", G, k)
    batched = L.call("ia_density_init_workspace_bytes_batched", G, k, iters)
    assert batched >= small and (batched > small) == (iters > 1)
    jit_dev = _dev(jit)
    runs = [("batched", batched, True), ("small", small, True), ("batched, occ_bool = NULL", batched, False)]
    if batched - 1 >= small:
        runs.append(("batched - 1 byte (small route)", batched - 1, True))
    for what, nbytes, with_bool in runs:
        density, words, occ = _grid_init(model, aabb, jit_dev, iters, G, nbytes, with_bool)
        bad = np.nonzero(_bits(density) != _bits(density_ref))[0]
        assert not len(bad), (what, len(bad), bad[:5].tolist(), density[bad[:5]].tolist(), density_ref[bad[:5]].tolist())
        assert np.array_equal(words, words_ref), what
        if with_bool:
            assert np.array_equal(occ.astype(bool).reshape(G, G, G), occ_ref) and occ.max() <= 1, what
    # one byte short of the small workspace: IA_ERR_WORKSPACE, nothing written anywhere
    msg = _grid_init(model, aabb, jit_dev, iters, G, small - 1, expect_error=True)
    assert "(%d)" % sr.IA_ERR_WORKSPACE in msg and "workspace" in msg


# ---- B ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", (4, 12, 20))
def test_occupancy_postprocess_small_and_ragged_grids(oracle, G):
    n = G ** 3
    assert n % 64 == 0 and (G == 4 or n % 256 != 0)
    for what, dens in sr.occupancy_cases(G).items():
        ref = oracle.occupancy_from_density(dens, G).astype(bool)
        got, words = _occupancy(G, dens)
        assert np.array_equal(got, ref), (G, what, int(got.sum()), int(ref.sum()))                 # field against the oracle
        assert np.array_equal(sr.unpack_words(words, G), got), (G, what)                           # bits unpacked
        border = got.copy(); border[1:-1, 1:-1, 1:-1] = False
        assert int(words[n // 32]) == (0 if border.any() else 1), (G, what)                        # flag word
        cells = np.argwhere(got)
        want = [v for c in range(3) for v in ((int(cells[:, c].min()), int(cells[:, c].max())) if len(cells) else (0x7fffffff, -1))]
        assert words[n // 32 + 1:n // 32 + 7].tolist() == want, (G, what, want)                    # bounds words
        assert np.array_equal(words, sr.pack_with_tail(ref)), (G, what)
        # ia_occupancy_pack on the same field: the same words
        packed = _words_out(G)
        _lib().call("ia_occupancy_pack", _dev(got.astype(np.uint8).reshape(-1)), G, packed)
        torch.cuda.synchronize()
        _tail_intact(packed, n // 32 + 8, "ia_occupancy_pack")
        assert np.array_equal(_np(packed[:n // 32 + 7]), words), (G, what)


def test_occupancy_pack_128_bounds_loop():
    """k_occ_bounds' power-of-two route with n_words / 4 = 16384 quads for 1024 threads: eight trips of the two-quad loop"""
    G = 128
    n_words = G ** 3 // 32
    for what, occ in sr.pack_cases_128().items():
        words = _words_out(G)
        _lib().call("ia_occupancy_pack", _dev(occ.astype(np.uint8).reshape(-1)), G, words)
        torch.cuda.synchronize()
        _tail_intact(words, n_words + 8, what)
        got, want = _np(words[:n_words + 7]), sr.pack_with_tail(occ)
        assert np.array_equal(got[:n_words], want[:n_words]), what
        assert got[n_words:].tolist() == want[n_words:].tolist(), (what, got[n_words:].tolist(), want[n_words:].tolist())


# ---- C ---------------------------------------------------------------------------------------------------------------
def _voxelise(case, n_smooth, ws_short=0):
    L = _lib()
    d, h, w = case["grid"]
    n = d * h * w
    nbytes = L.call("ia_voxelise_workspace_bytes", d, h, w)
    ws, out = _u8_out(nbytes), _f32_out(24 * n)
    try:
        L.call("ia_voxelise_weights", _dev(case["pts"]), _dev(case["verts"]), len(case["verts"]), _dev(case["vw"]), d, h, w, n_smooth, out, ws,
               nbytes - ws_short)
    finally:
        torch.cuda.synchronize()
        _tail_intact(ws, nbytes - ws_short, "voxelise workspace")
        _tail_intact(out, 0 if ws_short else 24 * n, "voxel_w")
    return _np(out[:24 * n]).reshape(24, n)


def _check_blend(case, what):
    got = _voxelise(case, 0)
    ref, bound = sr.voxelise_ref(case)
    err = np.abs(got.astype(np.float64) - ref)
    zero = bound == 0
    assert (got[zero] == 0).all(), what
    ratio = float((err[~zero] / bound[~zero]).max())
    k = np.unravel_index(np.argmax(np.where(zero, 0, err / np.where(zero, 1, bound))), err.shape)
    print("RATIO voxelise blend %s: max error %.3g allowance %.3g ratio %.3f (%d outputs exactly 0)" % (what, err[k], bound[k], ratio, int(zero.sum())))
    assert (err <= bound).all(), (what, float(err[k]), float(bound[k]))
    return got


@pytest.mark.parametrize("n_verts", sr.VOX_NVERTS)
def test_voxelise_weights_blend_and_smoothing(n_verts):
    for grid in sr.VOX_GRIDS:
        case = sr.voxel_case(grid, n_verts)
        w0 = _check_blend(case, "grid %s, %d vertices" % (grid, n_verts))
        for n_smooth in sr.VOX_NSMOOTH[1:]:
            got = _voxelise(case, n_smooth)                                   # (either ping-pong parity: the result lands in voxel_w)
            ref = sr.smooth_ref32(w0, grid, n_smooth)
            bad = np.argwhere(_bits(got) != _bits(ref))
            assert not len(bad), (grid, n_verts, n_smooth, len(bad), bad[:4].tolist())


def test_voxelise_weights_exact_ties():
    case = sr.tie_case()
    w0 = _check_blend(case, "ties")
    for n_smooth in (1, 2):
        assert np.array_equal(_bits(_voxelise(case, n_smooth)), _bits(sr.smooth_ref32(w0, case["grid"], n_smooth)))


def test_voxelise_weights_workspace_one_byte_short():
    L = _lib()
    with pytest.raises(L.IAError) as e:
        _voxelise(sr.voxel_case((3, 4, 5), 31), 1, ws_short=1)
    assert "(%d)" % sr.IA_ERR_WORKSPACE in str(e.value)


# ---- D ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", sr.CENTRE_GS)
def test_grid_cell_centres_bit_for_bit(G):
    n = G ** 3
    out = _f32_out(n * 3)
    _lib().call("ia_grid_cell_centres", G, _dev(sr.CENTRE_AABB), out)
    torch.cuda.synchronize()
    _tail_intact(out, n * 3, "cell centres")
    assert np.array_equal(_bits(_np(out[:n * 3]).reshape(n, 3)), _bits(sr.cell_centres_ref(G, sr.CENTRE_AABB)))


def _sdf(pts, verts, faces):
    N = len(pts)
    out = _f32_out(N)
    _lib().call("ia_mesh_signed_distance", _dev(pts), N, _dev(verts), _dev(np.asarray(faces, np.int32)), len(faces), out)
    torch.cuda.synchronize()
    _tail_intact(out, N, "sdf")
    return _np(out[:N])


@pytest.mark.parametrize("shape", sr.SDF_SHAPES)
def test_mesh_signed_distance_exact_sign_on_the_lattice(shape):
    exp = sr.sdf_expectation(shape)
    verts, faces = sr.shape_mesh(shape)
    fv = sr.lattice_to_float(verts)
    n_off, n_on = int((exp["sign"] != 0).sum()), int((exp["sign"] == 0).sum())
    assert n_off > 3500 and n_on > 100
    first = None
    for name, f in sr.mesh_variants(verts, faces).items():
        sdf = _sdf(exp["pts"], fv, f)
        err, allow, ratio = sr.sdf_compare(sdf, exp)
        print("RATIO mesh sdf %s %s (%d faces): %d off, %d on the surface, max error %.3g allowance %.3g ratio %.3f" % (shape, name, len(f), n_off, n_on, err, allow, ratio))
        first = sdf if first is None else first
        assert np.array_equal(np.signbit(sdf), np.signbit(first)), name
    # ragged and single-thread launches: the same answers for the first N queries of a seeded order
    order = np.random.RandomState(3).permutation(len(exp["pts"]))
    for N in sr.SDF_NS:
        sel = order[:N]
        sdf = _sdf(exp["pts"][sel], fv, faces)
        sr.sdf_compare(sdf, exp, sel)
        assert np.array_equal(_bits(sdf), _bits(first[sel])), N
