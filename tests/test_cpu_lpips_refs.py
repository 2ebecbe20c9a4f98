"""The patch-loss kernels' float64 restatements (tests/lpips_refs.py) against autograd through the torch expressions they restate --
`NGPLoss(fused=False)` and `utils.lpips.LPIPS` -- and the host side of the feature: the header's binding table, the build lists, the
refusals, and that nothing changes for a caller who does not ask for `patch_terms="hip"`."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_refs as lr
from instantavatar_amd.training import NGPLoss

NAMES = ["ia_conv3x3", "ia_conv3x3_pack", "ia_conv3x3_packed_bytes", "ia_conv3x3_workspace_bytes", "ia_lpips_head", "ia_lpips_head_bwd",
         "ia_lpips_head_workspace_bytes", "ia_lpips_prepare", "ia_lpips_prepare_bwd", "ia_maxpool2x2", "ia_maxpool2x2_bwd", "ia_patch_depth_reg"]


def test_header_is_a_table_of_its_own_and_is_built():
    from instantavatar_amd import _lib, build
    d = _lib.declarations("lpips")
    assert sorted(d) == NAMES          # (disjoint from every other header's names: tests/test_cpu_abi_headers.py)
    for name in NAMES:
        if not name.endswith("_bytes"):
            assert d[name].stream, name
    assert len(d["ia_conv3x3"].params) == 14 and len(d["ia_patch_depth_reg"].params) == 8
    assert "ia_lpips.hip" in build.SOURCES and "ia_lpips.hip" in build.source_manifest()
    assert os.path.normpath(_lib.header_path("lpips")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert os.path.exists(os.path.join(build.CSRC, "ia_lpips.hip"))


def test_library_binds_the_entries_and_refuses_bad_arguments():
    from instantavatar_amd import _lib
    assert hasattr(_lib.lib(), "ia_conv3x3") and all(n in _lib._bound for n in NAMES)
    # sizes are closed expressions: K padded to 288 rows per 32 input channels, Cout to 64
    assert _lib.call("ia_conv3x3_packed_bytes", 3, 64) == 288 * 64 * 4 and _lib.call("ia_conv3x3_packed_bytes", 64, 3) == 2 * 288 * 64 * 4
    assert _lib.call("ia_conv3x3_packed_bytes", 512, 512) == 16 * 288 * 512 * 4
    assert _lib.call("ia_conv3x3_packed_bytes", 0, 64) == 0 and _lib.call("ia_conv3x3_packed_bytes", 513, 64) == 0
    assert _lib.call("ia_conv3x3_workspace_bytes", 8, 3, 64, 32, 32) == 256
    assert _lib.call("ia_conv3x3_workspace_bytes", 3, 128, 256, 2, 2) == 4 * 3 * 256 * 4 * 4
    assert _lib.call("ia_lpips_head_workspace_bytes", 4, 1024) == 4 * 64 * 4 and _lib.call("ia_lpips_head_workspace_bytes", 1, 4) == 256
    assert _lib.call("ia_lpips_head_workspace_bytes", 0, 4) == 0 and _lib.call("ia_lpips_head_workspace_bytes", 1, 16 * 65535 + 1) == 0
    assert _lib.call("ia_conv3x3_workspace_bytes", 1, 64, 64, 0, 2) == 0 and _lib.call("ia_conv3x3_workspace_bytes", 1 << 20, 512, 512, 64, 64) == 0
    P = 4096                                                  # (a non-null address that is never read: every call below is refused)
    for args, msg in (((P, None, P, P, 1, 0, 64, 5, 7, 1, P, None, 0, P), "Cin 0"),
                      ((P, None, P, P, 1, 64, 64, 5, 7, 1, P, None, 0, P), "ia_conv3x3_workspace_bytes"),
                      ((None, None, P, P, 1, 3, 64, 5, 7, 1, P, None, 0, P), "are required"),
                      ((P, None, P + 4, P, 1, 3, 64, 5, 7, 1, P, None, 0, P), "16-byte aligned")):
        with pytest.raises(_lib.IAError, match=msg):
            _lib.call("ia_conv3x3", *args)
    with pytest.raises(_lib.IAError, match="H, W >= 2"):
        _lib.call("ia_maxpool2x2", P, 3, 1, 4, P, P)
    with pytest.raises(_lib.IAError, match="ia_conv3x3_packed_bytes"):
        _lib.call("ia_conv3x3_pack", P, 64, 3, 0, P, 16, P)
    with pytest.raises(_lib.IAError, match="n_patch 0"):
        _lib.call("ia_patch_depth_reg", P, P, 0, 4, P, P, P, P)


def test_fused_lpips_refuses_alex_and_the_cpu():
    from instantavatar_amd import _lib
    from instantavatar_amd.lpips_hip import FusedLPIPS, depth_reg
    from instantavatar_amd.utils.lpips import LPIPS
    with pytest.raises(ValueError, match="net='alex'"):
        FusedLPIPS(LPIPS(net="alex"))
    with pytest.raises(TypeError):
        FusedLPIPS(torch.nn.Identity())
    fused = FusedLPIPS(lr.seeded_lpips())
    assert [op[0] for op in fused.plan].count("conv") == 13 and [op[0] for op in fused.plan].count("pool") == 4
    with pytest.raises(_lib.IAError, match="no CPU path"):
        fused.value_and_grad(torch.rand(1, 16, 16, 3), torch.rand(1, 16, 16, 3))
    with pytest.raises(_lib.IAError, match="no CPU path"):
        depth_reg(torch.rand(1, 4, 4), torch.rand(1, 4, 4))
    with pytest.raises(ValueError, match="net='alex'"):
        NGPLoss(dict(w_lpips=0.01), lpips=LPIPS(net="alex"), patch_terms="hip")
    with pytest.raises(ValueError, match="patch_terms"):
        NGPLoss(dict(), patch_terms="cuda")


def _patch_batch(n, P, Q, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    pred, target = lr.whole_term_inputs(n, P, Q, seed)
    predicts = dict(rgb_coarse=pred[None].to(dtype), alpha_coarse=torch.rand(1, n, P, Q, generator=g).to(dtype),
                    weight_coarse=torch.rand(64, generator=g).to(dtype), depth_coarse=(2 + torch.rand(1, n, P, Q, generator=g)).to(dtype))
    targets = dict(rgb=target[None].to(dtype), alpha=(torch.rand(1, n, P, Q, generator=g) > 0.5).to(dtype))
    return predicts, targets


def test_refs_equal_autograd_through_the_torch_loss():
    """prepare + head (+ their gradients) and the depth term, in closed form, against autograd through NGPLoss(fused=False) in float64"""
    m = lr.seeded_lpips(1).double()
    loss = NGPLoss(dict(w_rgb=1.0, w_alpha=0.1, w_reg=0.1, w_lpips=0.01, w_depth_reg=0.01), fused=False, lpips=m)
    assert loss.patch_terms == "torch"
    predicts, targets = _patch_batch(2, 16, 16, 3)
    for k in ("rgb_coarse", "alpha_coarse", "depth_coarse"):
        predicts[k].requires_grad_(True)
    out = loss(predicts, targets)
    # the depth term
    v, d_a, d_d = lr.depth_reg(predicts["alpha_coarse"].detach().reshape(2, -1), predicts["depth_coarse"].detach().reshape(2, -1))
    g_a, g_d = torch.autograd.grad(out["loss_depth_reg"], [predicts["alpha_coarse"], predicts["depth_coarse"]], retain_graph=True)
    assert abs(float(v) - float(out["loss_depth_reg"].detach())) <= 1e-14 * abs(float(v))
    assert torch.allclose(d_a.reshape(g_a.shape), g_a, rtol=1e-12, atol=1e-18) and torch.allclose(d_d.reshape(g_d.shape), g_d, rtol=1e-12, atol=1e-18)
    # LPIPS = prepare -> trunk -> five heads; the trunk is torch's here, prepare and the heads are the restatements
    pred, target = predicts["rgb_coarse"].detach()[0], targets["rgb"][0]
    x = lr.prepare(pred, target, m.scaling_layer.shift.reshape(-1), m.scaling_layer.scale.reshape(-1)).requires_grad_(True)
    feats = m.net(x)
    val = sum(lr.head(f.flatten(2), lin.model[0].weight.reshape(-1)) for f, lin in zip(feats, m.lins))
    assert torch.allclose(val.sum(), out["loss_lpips"], rtol=1e-12)
    g_rgb, = torch.autograd.grad(out["loss_lpips"], predicts["rgb_coarse"])
    # the heads' closed-form gradients, pushed through the trunk by autograd and through prepare by its closed form
    hg = [lr.head_bwd(f.detach().flatten(2), lin.model[0].weight.reshape(-1)).reshape(f[:2].shape) for f, lin in zip(feats, m.lins)]
    gx, = torch.autograd.grad([f[:2] for f in feats], x, hg)
    mine = lr.prepare_bwd(pred, gx[:2], m.scaling_layer.scale.reshape(-1))
    # (NGPLoss hands the module `.float()` inputs, so `2 x - 1` and the gradient's way back are rounded to fp32 there: a perturbation
    #  of 2^-24 of the network's input and of its gradient, seen here at 7e-8 of the largest element; a wrong restatement is off by O(1))
    assert torch.allclose(mine, g_rgb[0], rtol=0, atol=2.0 ** -20 * float(g_rgb.abs().max()))
    assert (mine[pred > 1] == 0).all() and (pred > 1).any()
    # module_value_and_grad is the same thing per image, float64 throughout
    v2, g2 = lr.module_value_and_grad(m, pred, target)
    assert torch.allclose(v2.sum(), out["loss_lpips"], rtol=1e-12) and torch.allclose(mine, g2, rtol=1e-9, atol=1e-10 * float(g2.abs().max()))


def test_pool_refs_equal_torch():
    rng = np.random.RandomState(0)
    for H, W in ((4, 4), (5, 7), (2, 2)):
        x = rng.randn(6, H, W).astype(np.float32)
        x[0, 0, 0] = x[0, 0, 1] = x[0, 1, 1] = 3.0                    # a tie at a positive value: the first in row-major order takes it
        xt = torch.from_numpy(x)[None].requires_grad_(True)
        y = F.max_pool2d(xt, 2, 2)
        dy = torch.from_numpy(rng.randn(*y.shape).astype(np.float32))
        g, = torch.autograd.grad(y, xt, dy)
        mine, arg = lr.pool(x)
        assert mine.tobytes() == y.detach().numpy()[0].tobytes() and arg[0, 0, 0] == 0
        assert lr.pool_bwd(x, dy.numpy()[0]).tobytes() == g.numpy()[0].tobytes()


def test_default_patch_terms_are_todays_torch_expressions():
    """Nothing changes without the new argument: the default is "torch", a CPU batch never reaches the kernels whatever was asked for,
    the driver's defaults are the old ones, and the values are the expressions of loss.py:28-39."""
    from instantavatar_amd.drivers import fit as fit_driver
    assert inspect.signature(NGPLoss.__init__).parameters["patch_terms"].default == "torch"
    sig = inspect.signature(fit_driver.fit_sequence).parameters
    assert sig["patch_terms"].default == "torch" and sig["lpips"].default is None
    m = lr.seeded_lpips(2)
    predicts, targets = _patch_batch(2, 16, 16, 4, torch.float32)
    opt = dict(w_rgb=1.0, w_alpha=0.1, w_reg=0.1, w_lpips=0.01, w_depth_reg=0.01)
    a = NGPLoss(opt, fused=False, lpips=m)(predicts, targets)
    b = NGPLoss(opt, fused=False, lpips=m, patch_terms="hip")(predicts, targets)           # CPU tensors: the torch expressions
    base = NGPLoss(dict(opt, w_lpips=0, w_depth_reg=0), fused=False)(predicts, targets)
    pr = predicts["rgb_coarse"][0][..., [2, 1, 0]].permute(0, 3, 1, 2).clip(max=1)
    tg = targets["rgb"][0][..., [2, 1, 0]].permute(0, 3, 1, 2)
    lp = m(pr, tg).sum()
    al, de = predicts["alpha_coarse"], predicts["depth_coarse"]
    avg = (de * al).sum(dim=(-1, -2)) / (al.sum(dim=(-1, -2)) + 1e-3)
    reg = (al * (de - avg[..., None, None]).abs()).mean()
    assert torch.equal(a["loss_lpips"], lp) and torch.equal(a["loss_depth_reg"], reg)
    assert torch.equal(a["loss"], base["loss"] + 0.01 * lp + 0.01 * reg)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert not NGPLoss(opt, lpips=m).direct_backward_ok(predicts) and not NGPLoss(opt, lpips=m, patch_terms="hip").direct_backward_ok(predicts)
    flat = {k: v.reshape(1, -1, *v.shape[4:]) if v.dim() == 5 else v for k, v in predicts.items()}
    assert "loss_lpips" not in NGPLoss(opt, fused=False, lpips=m, patch_terms="hip")(flat, {k: v.reshape(1, -1, *v.shape[4:]) if v.dim() == 5 else v for k, v in targets.items()})
