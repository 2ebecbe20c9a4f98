"""`_lib.call`, the one checked way into the C ABI, against the hand-written `check(lib().ia_x(ptr(a), ..., stream()))`
idiom it replaces: same bits, and a wrong argument is a Python exception before anything is launched."""
import pytest
import torch

from instantavatar_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _near_far_inputs():
    transl = torch.tensor([0.3, -0.2, 2.5], device=DEV)
    return transl, torch.full((5,), -7.0, device=DEV), torch.full((5,), -7.0, device=DEV)


def test_call_equals_the_old_idiom_with_and_without_the_stream():
    transl, near0, far0 = _near_far_inputs()
    _lib.check(_lib.lib().ia_near_far(_lib.ptr(transl), 5, _lib.ptr(near0), _lib.ptr(far0), _lib.stream()), "ia_near_far")
    _, near1, far1 = _near_far_inputs()
    _lib.call("ia_near_far", transl, 5, near1, far1)
    _, near2, far2 = _near_far_inputs()
    _lib.call("ia_near_far", transl, 5, near2, far2, _lib.stream())
    assert (near0 != -7.0).all() and (far0 - near0 == 2.0).all()
    for near, far in ((near1, far1), (near2, far2)):
        assert torch.equal(near, near0) and torch.equal(far, far0)


@pytest.mark.parametrize("case, param", [("float64", "near_out"), ("strided", "near_out"), ("cpu", "transl"), ("one too many", None)])
def test_call_rejects_a_wrong_argument_before_the_launch(case, param):
    transl, near, far = _near_far_inputs()
    args = {"float64": (transl, 5, near.double(), far),
            "strided": (transl, 3, near[::2], far),
            "cpu": (transl.cpu(), 5, near, far),
            "one too many": (transl, 5, near, far, _lib.stream(), 0)}[case]
    with pytest.raises(_lib.IAError) as e:
        _lib.call("ia_near_far", *args)
    assert "ia_near_far" in str(e.value)
    if param is not None:     # (a surplus argument has no parameter to name)
        assert "`%s`" % param in str(e.value)
    torch.cuda.synchronize()
    assert (near == -7.0).all() and (far == -7.0).all()


@pytest.mark.parametrize("which", ["d_sigma only", "d_rgb only"])
def test_call_passes_none_as_null(which):
    P, n_cand = 3, 4
    g = torch.Generator(device=DEV).manual_seed(3)
    d_rgb = torch.randn((P, 3), device=DEV, generator=g) if which == "d_rgb only" else None
    d_sigma = torch.randn(P, device=DEV, generator=g) if which == "d_sigma only" else None
    arg = torch.tensor([2, -1, 0], dtype=torch.int32, device=DEV)
    old = torch.zeros((n_cand, 3), device=DEV), torch.zeros(n_cand, device=DEV)
    new = torch.zeros((n_cand, 3), device=DEV), torch.zeros(n_cand, device=DEV)
    _lib.check(_lib.lib().ia_candidate_gather_bwd(_lib.ptr(d_rgb), _lib.ptr(d_sigma), _lib.ptr(arg), P, _lib.ptr(old[0]),
                                                  _lib.ptr(old[1]), _lib.stream()), "ia_candidate_gather_bwd")
    _lib.call("ia_candidate_gather_bwd", d_rgb, d_sigma, arg, P, new[0], new[1])
    given, out = (d_rgb, old[0]) if d_rgb is not None else (d_sigma, old[1])
    assert torch.equal(out[2], given[0]) and torch.equal(out[0], given[2]) and (out[1] == 0).all() and (out[3] == 0).all()
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])


def test_call_returns_sizes_and_passes_structs_by_reference():
    import ctypes as C
    L = _lib.lib()
    assert _lib.call("ia_field_act_stride", 16) == L.ia_field_act_stride(16) > 0
    assert _lib.call("ia_occupancy_workspace_bytes", 64) == L.ia_occupancy_workspace_bytes(64) > 0
    grid = _lib.SnarfGrid(D=8, H=32, W=32)
    assert _lib.call("ia_precompute_workspace_bytes", grid) == L.ia_precompute_workspace_bytes(C.byref(grid))
    with pytest.raises(_lib.IAError, match="ia_precompute_workspace_bytes.*`grid`"):
        _lib.call("ia_precompute_workspace_bytes", _lib.OccGrid(G=64))
