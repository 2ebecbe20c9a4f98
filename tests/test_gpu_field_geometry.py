"""Launch geometry of the render MLP on the planes route: ia_field_fwd with a descriptor that carries `enc_ws` (V >= 8192:
k_encode_xcd, then k_field<L, false, 0, 4, true> as 256-thread workgroups, at most 3 per CU) against the same call without
`enc_ws` (the fused route at 768 threads, pinned to the float64 references by test_gpu_mlp_kernels.py), bit for bit.  Which
wave of which workgroup runs a tile must not show in the result: the sizes below cover workgroups that exit before staging,
ragged last tiles, *n_dev below V and zero, and a second round of the wave loop.  The bound is zero differing elements."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_refs as mr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 9.0
PLANES_WORKGROUPS, PLANES_WAVES = 256 * 3, 4       # ia_field.hip: IA_FIELD_PLANES_WG_PER_CU, IA_FIELD_PLANES_THREADS / 64
ROUND = PLANES_WORKGROUPS * PLANES_WAVES * 64      # samples of one round of the wave loop over the full grid
assert ROUND + 64 + 5 == 196677 == mr.FWD_V[-1]

#            V, *n_dev
CASES = ((8192, None),            # 128 tiles: fewer tiles than workgroups
         (8193, None),            # ragged last tile, one lane live
         (8192 + 63, None),       # ragged last tile, 63 lanes live
         (8257, 8157),            # rows at or past *n_dev keep the sentinel
         (8192, 0),               # nothing is written
         (ROUND + 64 + 5, None))  # a second round of the wave loop: one full and one ragged tile


def _L():
    from instantavatar_amd import _lib as L
    return L


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


class _Field:
    """the synthetic field of the MLP tests (xavier weights, random table, body-sized box); `enc_ws_samples` > 0 adds the
    encoder workspace that selects the planes route"""

    def __init__(self, n_levels, W, table, enc_ws_samples=0):
        L = _L()
        self.hd = L.make_hash_desc(n_levels)
        self.t = {k: _dev(np.asarray(W[k], np.float16)) for k in mr.WEIGHT_NAMES}
        self.t["table"] = table
        f = self.f = L.Field()
        f.center[:], f.scale[:] = [float(v) for v in mr.REAL_CENTER], [float(v) for v in mr.REAL_SCALE]
        f.hash = self.hd
        f.table = table.data_ptr()
        f.sig_w1, f.sig_w2 = self.t["W1"].data_ptr(), self.t["W2"].data_ptr()
        f.col_w1, f.col_w2, f.col_w3 = self.t["Wc1"].data_ptr(), self.t["Wc2"].data_ptr(), self.t["Wc3"].data_ptr()
        f.enc_ws, f.enc_ws_samples, f.enc_split = None, 0, 0
        self.t["frags"] = torch.zeros(L.lib().ia_field_frags_bytes() // 2, dtype=torch.float16, device=DEV)
        L.check(L.lib().ia_field_prepare(C.byref(f), L.ptr(self.t["frags"]), L.stream()), "ia_field_prepare")
        f.mlp_frags = self.t["frags"].data_ptr()
        if enc_ws_samples:
            self.t["enc_ws"] = torch.zeros(n_levels * enc_ws_samples, dtype=torch.int32, device=DEV)
            f.enc_ws, f.enc_ws_samples = self.t["enc_ws"].data_ptr(), enc_ws_samples


@functools.lru_cache(maxsize=None)
def _fields(n_levels):
    """(fused route, planes route) over the same weights and table, built once per level count"""
    L = _L()
    W = mr.xavier_weights(n_levels)
    table = _dev(mr.real_table(int(L.make_hash_desc(n_levels).offset[n_levels])))
    return _Field(n_levels, W, table), _Field(n_levels, W, table, enc_ws_samples=max(v for v, _ in CASES) + 11)


@functools.lru_cache(maxsize=None)
def _points(V):
    """points uniform in the field's box"""
    u = np.random.RandomState(8300 + V % 977).rand(V, 3)
    return _dev(((u - 0.5) * mr.REAL_SCALE.astype(np.float64) + mr.REAL_CENTER.astype(np.float64)).astype(np.float32))


def _fwd(fd, x, n_dev):
    L = _L()
    V = len(x)
    rgb, sigma = torch.full((V, 3), SENTINEL, device=DEV), torch.full((V,), SENTINEL, device=DEV)
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    L.check(L.lib().ia_field_fwd(L.ptr(x), V, L.ptr(nd), C.byref(fd.f), L.ptr(rgb), L.ptr(sigma), L.stream()), "ia_field_fwd")
    torch.cuda.synchronize()
    return _bits(rgb), _bits(sigma)


@pytest.mark.parametrize("V,n_dev", CASES)
@pytest.mark.parametrize("n_levels", [8, 16])
def test_planes_route_equals_fused_route_bit_for_bit(n_levels, V, n_dev):
    fused, planes = _fields(n_levels)
    x = _points(V)
    n = V if n_dev is None else n_dev
    rgb0, sigma0 = _fwd(fused, x, n_dev)
    rgb1, sigma1 = _fwd(planes, x, n_dev)
    sent = np.float32(SENTINEL).view(np.uint32)
    assert (rgb1[n:] == sent).all() and (sigma1[n:] == sent).all(), "rows at or past *n_dev were written"
    assert (rgb0[n:] == sent).all() and (sigma0[n:] == sent).all()
    if n:
        assert (sigma1[:n] != sent).any(), "the planes route wrote nothing"
    d_rgb, d_sigma = int((rgb0 != rgb1).sum()), int((sigma0 != sigma1).sum())
    print("DIFF L%d V%d n_dev %s: rgb %d of %d, sigma %d of %d" % (n_levels, V, n_dev, d_rgb, rgb0.size, d_sigma, sigma0.size))
    assert d_rgb == 0 and d_sigma == 0
    # the same inputs again give the same bits
    rgb2, sigma2 = _fwd(planes, x, n_dev)
    assert np.array_equal(rgb1, rgb2) and np.array_equal(sigma1, sigma2), "two calls with the same inputs differ"
