"""Samples-per-thread shapes of the XCD-sharded encoder k_encode_xcd<L, S>, through the C ABI.

Render route: ia_field_fwd with a descriptor that carries `enc_ws` (V >= 8192) encodes with the render shape
(IA_ENC_S_RENDER samples per thread, tiles of 256 x S samples) and must equal the same call without `enc_ws` -- the fused
route, pinned to the float64 references by test_gpu_mlp_kernels.py -- bit for bit, for 8 and 16 levels and enc_split 0, 2
and 3.  The library decides the shape, so the sizes below are chosen to be the hard ones for EVERY shape a build can
offer (S = 1, 2, 3; checked by the asserts under CASES): V one below, at and one above a common tile multiple, tile counts
4k, 4k + 1, 4k + 2 and 4k + 3 (the second level group is dealt in fours between XCD k and XCD k + 4), a V whose item count
exceeds every shape's grid cap so that workgroups loop, *n_dev below V off a tile boundary, and *n_dev = 0.  Rows at or
past *n_dev keep their prefill.  Training and stand-alone routes (S = 3 behind the same launcher): the record features of
ia_field_fwd_train and the planes of ia_hashgrid_fwd_planes equal ia_hashgrid_fwd bit for bit.
The bound everywhere is zero differing elements: per-sample arithmetic does not depend on the shape."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_refs as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 9.0
SHAPES = (1, 2, 3)                      # ia_field.hip: the values IA_ENC_S_RENDER / IA_ENC_S admit
THREADS = 256                           # IA_ENC_THREADS
WAVES_PER_SIMD = {1: 8, 2: 5, 3: 4}     # 512 VGPRs / allocated VGPRs of the shape (56, 88, 128), at most 8
BIG = (70001, 66667)

#            V, *n_dev
CASES = ((8192, None),          # IA_SHARD_MIN: the first sharded size
         (8193, None),
         (8453, None),
         (8709, None),
         (9215, None),          # 9216 = 36 x 256 = 18 x 512 = 12 x 768
         (9216, None),
         (9217, None),
         (10000, None),
         (10000, 9217),
         BIG,                   # *n_dev below V, off every tile boundary; more work items than any shape's grid holds
         (8192, 0))             # nothing is written


def _tiles(v, s):
    return -(-v // (THREADS * s))


for _s in SHAPES:
    _n = [V if n is None else n for V, n in CASES]
    assert {_tiles(v, _s) % 4 for v in _n if v} == {0, 1, 2, 3}, _s
    assert all(v % (THREADS * _s) in (THREADS * _s - 1, 0, 1) for v in (9215, 9216, 9217)), _s
    assert BIG[1] % (THREADS * _s) not in (0, 1, THREADS * _s - 1)
    # 16 levels, enc_split 2: tiles + 2 * ceil(tiles / 4) items per XCD against 32 CUs x waves per SIMD workgroups
    assert _tiles(BIG[1], _s) + 2 * -(-_tiles(BIG[1], _s) // 4) > 32 * WAVES_PER_SIMD[_s], _s
WS_SAMPLES = max(v for v, _ in CASES) + 11


def _L():
    from instantavatar_amd import _lib as L
    return L


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


class _Field:
    """the synthetic field of the MLP tests (xavier weights, random table, body-sized box); `enc_ws_samples` > 0 adds the
    encoder workspace that selects the sharded encoding"""

    def __init__(self, n_levels, W, table, enc_ws_samples=0, enc_split=0):
        L = _L()
        self.n_levels = n_levels
        self.hd = L.make_hash_desc(n_levels)
        self.t = {k: _dev(np.asarray(W[k], np.float16)) for k in mr.WEIGHT_NAMES}
        self.t["table"] = table
        f = self.f = L.Field()
        f.center[:], f.scale[:] = [float(v) for v in mr.REAL_CENTER], [float(v) for v in mr.REAL_SCALE]
        f.hash = self.hd
        f.table = table.data_ptr()
        f.sig_w1, f.sig_w2 = self.t["W1"].data_ptr(), self.t["W2"].data_ptr()
        f.col_w1, f.col_w2, f.col_w3 = self.t["Wc1"].data_ptr(), self.t["Wc2"].data_ptr(), self.t["Wc3"].data_ptr()
        f.enc_ws, f.enc_ws_samples, f.enc_split = None, 0, enc_split
        self.t["frags"] = torch.zeros(L.lib().ia_field_frags_bytes() // 2, dtype=torch.float16, device=DEV)
        L.check(L.lib().ia_field_prepare(C.byref(f), L.ptr(self.t["frags"]), L.stream()), "ia_field_prepare")
        f.mlp_frags = self.t["frags"].data_ptr()
        if enc_ws_samples:
            self.t["enc_ws"] = torch.zeros(n_levels * enc_ws_samples, dtype=torch.int32, device=DEV)
            f.enc_ws, f.enc_ws_samples = self.t["enc_ws"].data_ptr(), enc_ws_samples


@functools.lru_cache(maxsize=None)
def _table(n_levels):
    L = _L()
    return mr.xavier_weights(n_levels), _dev(mr.real_table(int(L.make_hash_desc(n_levels).offset[n_levels])))


@functools.lru_cache(maxsize=None)
def _field(n_levels, enc_split=None):
    """enc_split None: no workspace (the fused route); else the sharded route with that hint"""
    W, table = _table(n_levels)
    if enc_split is None:
        return _Field(n_levels, W, table)
    return _Field(n_levels, W, table, enc_ws_samples=WS_SAMPLES, enc_split=enc_split)


@functools.lru_cache(maxsize=None)
def _points(V):
    """points uniform in the field's box"""
    u = np.random.RandomState(4100 + V % 977).rand(V, 3)
    return _dev(((u - 0.5) * mr.REAL_SCALE.astype(np.float64) + mr.REAL_CENTER.astype(np.float64)).astype(np.float32))


def _fwd(fd, x, n_dev):
    L = _L()
    V = len(x)
    rgb, sigma = torch.full((V, 3), SENTINEL, device=DEV), torch.full((V,), SENTINEL, device=DEV)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    L.check(L.lib().ia_field_fwd(L.ptr(x), V, L.ptr(nd), C.byref(fd.f), L.ptr(rgb), L.ptr(sigma), L.stream()), "ia_field_fwd")
    torch.cuda.synchronize()
    return _bits(rgb), _bits(sigma)


@functools.lru_cache(maxsize=None)
def _fused(n_levels, V, n_dev):
    """the fused route's bits, computed once per case and shared by the enc_split variants"""
    rgb, sigma = _fwd(_field(n_levels), _points(V), n_dev)
    rgb.setflags(write=False)
    sigma.setflags(write=False)
    return rgb, sigma


@pytest.mark.parametrize("V,n_dev", CASES)
@pytest.mark.parametrize("enc_split", [0, 2, 3])
@pytest.mark.parametrize("n_levels", [8, 16])
def test_render_route_equals_fused_route_bit_for_bit(n_levels, enc_split, V, n_dev):
    n = V if n_dev is None else n_dev
    rgb0, sigma0 = _fused(n_levels, V, n_dev)
    rgb1, sigma1 = _fwd(_field(n_levels, enc_split), _points(V), n_dev)
    sent = np.float32(SENTINEL).view(np.uint32)
    assert (rgb1[n:] == sent).all() and (sigma1[n:] == sent).all(), "rows at or past *n_dev were written"
    assert (rgb0[n:] == sent).all() and (sigma0[n:] == sent).all()
    if n:
        assert (sigma1[:n] != sent).any(), "the render route wrote nothing"
    d_rgb, d_sigma = int((rgb0 != rgb1).sum()), int((sigma0 != sigma1).sum())
    print("DIFF L%d split %d V%d n_dev %s: rgb %d of %d, sigma %d of %d" % (n_levels, enc_split, V, n_dev, d_rgb, rgb0.size, d_sigma, sigma0.size))
    assert d_rgb == 0 and d_sigma == 0


@pytest.mark.parametrize("V,n_dev", [(8193, None), (10000, 9217)])
@pytest.mark.parametrize("n_levels", [8, 16])
def test_training_and_standalone_routes_equal_hashgrid_fwd(n_levels, V, n_dev):
    L = _L()
    fd = _field(n_levels, 2)
    x = _points(V)
    n = V if n_dev is None else n_dev
    feat = torch.zeros((V, 2 * n_levels), dtype=torch.float16, device=DEV)
    L.check(L.lib().ia_hashgrid_fwd(L.ptr(x), V, C.byref(fd.f), L.ptr(feat), L.stream()), "ia_hashgrid_fwd")
    # stand-alone planes: [n_levels][stride] words of packed half2; columns at or past V keep the prefill
    stride = V + 11
    planes = torch.full((n_levels, stride), 0x12345678, dtype=torch.int32, device=DEV)
    L.check(L.lib().ia_hashgrid_fwd_planes(L.ptr(x), V, C.byref(fd.f), L.ptr(planes), stride, L.stream()), "ia_hashgrid_fwd_planes")
    # training forward on the sharded route: the record's first 2L halves are the features
    stride_a = L.lib().ia_field_act_stride(n_levels)
    rgb, sigma = torch.full((V, 3), SENTINEL, device=DEV), torch.full((V,), SENTINEL, device=DEV)
    acts = torch.full((V, stride_a), 0x1234, dtype=torch.int16, device=DEV).view(torch.float16)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    L.check(L.lib().ia_field_fwd_train(L.ptr(x), V, L.ptr(nd), C.byref(fd.f), L.ptr(rgb), L.ptr(sigma), L.ptr(acts), L.stream()),
            "ia_field_fwd_train")
    torch.cuda.synchronize()
    want = feat.cpu().numpy().view(np.uint32)                        # [V, n_levels]
    got_planes = planes.cpu().numpy().view(np.uint32)
    assert np.array_equal(got_planes[:, :V].T, want), "ia_hashgrid_fwd_planes differs from ia_hashgrid_fwd"
    assert (got_planes[:, V:] == 0x12345678).all(), "ia_hashgrid_fwd_planes wrote past V"
    got_acts = acts.cpu().numpy().view(np.uint16)
    assert np.array_equal(np.ascontiguousarray(got_acts[:n, :2 * n_levels]).view(np.uint32), want[:n]), \
        "record features of ia_field_fwd_train differ from ia_hashgrid_fwd"
    assert (got_acts[n:] == 0x1234).all(), "ia_field_fwd_train wrote record rows at or past *n_dev"
    rgb0, sigma0 = _fused(n_levels, V, n_dev)
    assert np.array_equal(_bits(rgb), rgb0) and np.array_equal(_bits(sigma), sigma0), "ia_field_fwd_train differs from ia_field_fwd"
