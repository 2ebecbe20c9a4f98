"""The patch terms of the fit stage's loss as HIP kernels (csrc/ia_lpips.hip through the C ABI and instantavatar_amd/lpips_hip.py):
the primitives against float64 references with derived bounds, the whole LPIPS term against the float64 torch module with a measured
yardstick, and the training step that uses them (NGPLoss(patch_terms="hip")).  Weights are seeded stand-ins (tests/lpips_refs.py)."""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_refs as lr
from instantavatar_amd import _lib
from instantavatar_amd.drivers import fit as fit_driver
from instantavatar_amd.lpips_hip import FusedLPIPS, depth_reg, depth_reg_value_and_grads
from instantavatar_amd.training import GraphedTrainStep, NGPLoss, configure_optimizer, training_step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- ia_conv3x3
def _conv(x, gate, w, b, relu, transpose_flip=0):
    """ia_conv3x3 on device tensors; w is the torch weight [Cout_w,Cin_w,3,3], packed here"""
    co_w, ci_w = int(w.shape[0]), int(w.shape[1])
    cin, cout = (co_w, ci_w) if transpose_flip else (ci_w, co_w)
    N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    assert x.shape[1] == cin
    nbytes = _lib.call("ia_conv3x3_packed_bytes", cin, cout)
    img = torch.empty(nbytes // 4, device=DEV)
    _lib.call("ia_conv3x3_pack", w, co_w, ci_w, transpose_flip, img, nbytes)
    ws = torch.empty(_lib.call("ia_conv3x3_workspace_bytes", N, cin, cout, H, W), dtype=torch.uint8, device=DEV)
    y = torch.full((N, cout, H, W), float("nan"), device=DEV)
    _lib.call("ia_conv3x3", x, gate, img, b, N, cin, cout, H, W, relu, y, ws, ws.numel())
    return y


def _conv_case(shape, seed=0):
    N, cin, cout, H, W = shape
    g = torch.Generator().manual_seed(seed + 1000 * cin + cout)
    x, gate = torch.randn(N, cin, H, W, generator=g), torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    b = torch.rand(cout, generator=g) * 0.2 - 0.1
    return x, gate, w, b


CONV_SHAPES = [(1, 3, 64, 5, 7), (2, 64, 3, 4, 4), (1, 5, 7, 1, 1), (3, 128, 256, 2, 2), (1, 512, 512, 2, 2)]


@pytest.mark.parametrize("gated", [0, 1], ids=["plain", "gated"])
@pytest.mark.parametrize("relu", [0, 1], ids=["linear", "relu"])
@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_within_the_a_priori_bound(shape, relu, gated):
    """|y - y64| <= (K + 2) 2^-24 (conv(|x|, |w|) + |b|), K = 9 Cin: the bound of ANY fp32 summation order; an indexing error misses it by
    orders of magnitude"""
    x, gate, w, b = _conv_case(shape)
    y = _conv(x.to(DEV), gate.to(DEV) if gated else None, w.to(DEV), b.to(DEV), relu).cpu()
    ref, bound = lr.conv_ref_and_bound(x, gate if gated else None, w, b, relu)
    err = (y.double() - ref).abs()
    print("conv %s relu %d gate %d: max err / bound %.3f, max |y| %.3g" % (shape, relu, gated, float((err / bound.clamp_min(1e-300)).max()), float(ref.abs().max())))
    assert torch.isfinite(y).all() and (err <= bound).all()
    assert float(ref.abs().max()) > 0.1               # (the case says something)


@pytest.mark.parametrize("shape", [(2, 64, 3, 4, 4), (1, 5, 7, 3, 3)], ids=lambda s: "x".join(map(str, s)))
def test_conv3x3_adjoint_pack_is_the_input_gradient(shape):
    """the gated call on the adjoint weight image against autograd's input gradient of relu(conv(x)) in float64; the gate is the
    kernel's own forward output"""
    N, cin, cout, H, W = shape
    x, _, w, b = _conv_case(shape, seed=7)
    up = torch.randn(N, cout, H, W, generator=torch.Generator().manual_seed(3))
    y = _conv(x.to(DEV), None, w.to(DEV), b.to(DEV), 1)
    gx = _conv(up.to(DEV), y, w.to(DEV), None, 0, transpose_flip=1).cpu()
    x64 = x.double().requires_grad_(True)
    pre = F.conv2d(x64, w.double(), b.double(), padding=1)
    assert ((pre > 0) == (y.cpu() > 0)).all()         # both precisions take the same ReLU decisions on this input
    ref, = torch.autograd.grad(F.relu(pre), x64, up.double())
    bound = (9 * cout + 2) * 2.0 ** -24 * F.conv_transpose2d((up.double() * (pre > 0)).abs(), w.double().abs(), padding=1)
    err = (gx.double() - ref).abs()
    print("adjoint %s: max err / bound %.3f" % (shape, float((err / bound.clamp_min(1e-300)).max())))
    assert gx.shape == x.shape and (err <= bound).all() and float(ref.abs().max()) > 0.1


def test_conv3x3_is_deterministic_and_batch_independent():
    shape = (3, 128, 256, 2, 2)
    x, gate, w, b = (t.to(DEV) for t in _conv_case(shape))
    a, b2 = _conv(x, gate, w, b, 1), _conv(x, gate, w, b, 1)
    assert a.cpu().numpy().tobytes() == b2.cpu().numpy().tobytes()
    alone = _conv(x[1:2].contiguous(), gate[1:2].contiguous(), w, b, 1)
    assert alone.cpu().numpy().tobytes() == a[1:2].cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------- pools
@pytest.mark.parametrize("hw", [(4, 4), (5, 7), (2, 2)], ids=lambda s: "%dx%d" % s)
def test_maxpool_and_its_gradient_are_torchs_bytes(hw):
    H, W = hw
    rng = np.random.RandomState(H * 10 + W)
    x = rng.randn(2, 3, H, W).astype(np.float32)
    x[0, 0, 0, 0] = x[0, 0, 0, 1] = x[0, 0, 1, 1] = 3.0        # a tie at a positive value
    xt = torch.from_numpy(x).requires_grad_(True)
    ref = F.max_pool2d(xt, 2, 2)
    dy = torch.from_numpy(rng.randn(*ref.shape).astype(np.float32))
    gref, = torch.autograd.grad(ref, xt, dy)
    xd = torch.from_numpy(x).to(DEV)
    y = torch.full(ref.shape, float("nan"), device=DEV)
    _lib.call("ia_maxpool2x2", xd, 6, H, W, y)
    dx = torch.full(x.shape, float("nan"), device=DEV)
    _lib.call("ia_maxpool2x2_bwd", xd, dy.to(DEV), 6, H, W, dx)
    assert y.cpu().numpy().tobytes() == ref.detach().numpy().tobytes()
    assert dx.cpu().numpy().tobytes() == gref.numpy().tobytes()
    assert float(dx[0, 0, 0, 0]) == float(dy[0, 0, 0, 0]) and float(dx[0, 0, 0, 1]) == 0 and float(dx[0, 0, 1, 1]) == 0
    assert lr.pool_bwd(x.reshape(6, H, W), dy.numpy().reshape(6, H // 2, W // 2)).tobytes() == gref.numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------- depth term
def _depth_ref(alpha, depth):
    """float64 autograd of NGPLoss's own expression (training.py, loss.py:33-39)"""
    a, d = alpha.double()[None].requires_grad_(True), depth.double()[None].requires_grad_(True)
    n, P, Q = alpha.shape
    predicts = dict(rgb_coarse=torch.zeros(1, n, P, Q, 3, dtype=torch.float64), alpha_coarse=a, weight_coarse=torch.rand(8).double(), depth_coarse=d)
    out = NGPLoss(dict(w_depth_reg=0.01), fused=False)(predicts, dict(rgb=torch.zeros(1, n, P, Q, 3).double(), alpha=torch.zeros(1, n, P, Q).double()))
    ga, gd = torch.autograd.grad(out["loss_depth_reg"], [a, d])
    return out["loss_depth_reg"].detach(), ga[0], gd[0]


@pytest.mark.parametrize("shape", [(1, 2, 2), (3, 5, 5), (4, 32, 32)], ids=lambda s: "x".join(map(str, s)))
def test_patch_depth_reg_rounds_once(shape):
    """the kernel accumulates in fp64 and rounds once: |delta| <= 2^-23 |ref| + 2^-40 max |ref| per element, value and both gradients"""
    g = torch.Generator().manual_seed(sum(shape))
    alpha, depth = torch.rand(shape, generator=g), 2 + torch.rand(shape, generator=g)
    v64, ga64, gd64 = _depth_ref(alpha, depth)
    v, ga, gd = depth_reg_value_and_grads(alpha.to(DEV), depth.to(DEV))
    for name, mine, ref in (("value", v.reshape(1), v64.reshape(1)), ("d_alpha", ga, ga64), ("d_depth", gd, gd64)):
        err = (mine.cpu().double() - ref).abs()
        bound = 2.0 ** -23 * ref.abs() + 2.0 ** -40 * ref.abs().max()
        print("depth_reg %s %s: max err / bound %.3f" % (shape, name, float((err / bound).max())))
        assert mine.shape == ref.shape and (err <= bound).all(), name
    # through autograd: the same numbers, scaled
    a, d = alpha.to(DEV).requires_grad_(True), depth.to(DEV).requires_grad_(True)
    (3 * depth_reg(a, d)).backward()
    assert torch.equal(a.grad, ga * 3) and torch.equal(d.grad, gd * 3)


def test_patch_depth_reg_with_an_empty_patch():
    g = torch.Generator().manual_seed(9)
    alpha, depth = torch.rand(2, 5, 5, generator=g), 2 + torch.rand(2, 5, 5, generator=g)
    alpha[1] = 0
    v, ga, gd = depth_reg_value_and_grads(alpha[1:].to(DEV), depth[1:].to(DEV))
    assert float(v) == 0 and torch.isfinite(ga).all() and torch.isfinite(gd).all() and (gd == 0).all()
    v64, ga64, gd64 = _depth_ref(alpha, depth)
    v, ga, gd = depth_reg_value_and_grads(alpha.to(DEV), depth.to(DEV))
    assert abs(float(v) - float(v64)) <= 2.0 ** -22 * float(v64) and torch.isfinite(ga).all() and torch.isfinite(gd).all()
    assert ((ga.cpu().double() - ga64).abs() <= 2.0 ** -23 * ga64.abs() + 2.0 ** -40 * ga64.abs().max()).all()


# ---------------------------------------------------------------------------------------------------------------- the whole term
# (n, P, Q, input seed, small-distance regime).  The seeds are ones for which the float64 run keeps every pre-activation away from zero
# (asserted in _whole_reference): with ~2e6 pre-activations per case about every other seed has one within 1e-6 of its layer's scale
WHOLE_CASES = {"1x16x16": (1, 16, 16, 11, False), "2x16x48": (2, 16, 48, 16, False), "4x32x32": (4, 32, 32, 21, False),
               "4x32x32-close": (4, 32, 32, 70, True)}
FACTOR = 8          # the two fp32 orders of the CPU differ from each other by up to 3.6 times the smaller one: a third order needs more room than 4


@functools.lru_cache(maxsize=None)
def _module():
    return lr.seeded_lpips(0)


@functools.lru_cache(maxsize=None)
def _fused():
    return FusedLPIPS(_module())


@functools.lru_cache(maxsize=None)
def _whole_reference(case):
    """(pred, target, v64, g64, yardstick of the values, yardstick of the gradients): the float64 module under autograd, and the
    deviation of the SAME module in fp32 on the CPU from it, contiguous and channels_last, the larger of the two"""
    n, P, Q, seed, close = WHOLE_CASES[case]
    pred, target = lr.whole_term_inputs(n, P, Q, seed, close)
    pre = []
    v64, g64 = lr.module_value_and_grad(_module(), pred, target, hooks=pre)
    # no ReLU or pool decision can differ between the precisions: no pre-activation of the float64 run lies within 1e-6 of zero
    # relative to its layer's scale (the rms of the layer's pre-activations)
    for k, p in enumerate(pre):
        assert float(p.abs().min()) > 1e-6 * float(p.pow(2).mean().sqrt()), (case, k)
    yv = yg = 0.0
    for fmt in (torch.contiguous_format, torch.channels_last):
        v32, g32 = lr.module_value_and_grad(_module(), pred, target, dtype=torch.float32, memory_format=fmt)
        yv = max(yv, float(((v32.double() - v64).abs() / v64.abs()).max()))
        yg = max(yg, float((g32.double() - g64).abs().max() / g64.abs().max()))
    return pred, target, v64, g64, yv, yg


@pytest.mark.parametrize("case", list(WHOLE_CASES))
def test_fused_lpips_against_the_float64_module(case):
    pred, target, v64, g64, yv, yg = _whole_reference(case)
    assert (pred > 1).any() and not (pred == 1).any()
    v, g = _fused().value_and_grad(pred.to(DEV), target.to(DEV))
    ev = float(((v.cpu().double() - v64).abs() / v64.abs()).max())
    eg = float((g.cpu().double() - g64).abs().max() / g64.abs().max())
    print("lpips %s: value err %.3e (cpu fp32 %.3e, ratio %.2f)  grad err %.3e (cpu fp32 %.3e, ratio %.2f)  launches %d"
          % (case, ev, yv, ev / yv, eg, yg, eg / yg, _fused().launches))
    assert v.shape == (pred.shape[0],) and g.shape == pred.shape and (v64 > 0).all()
    assert ev <= FACTOR * yv and eg <= FACTOR * yg
    assert (g[pred.to(DEV) > 1] == 0).all()
    # the autograd function gives the same numbers
    p = pred.to(DEV).requires_grad_(True)
    w = torch.arange(1, pred.shape[0] + 1, device=DEV, dtype=torch.float32)
    vals = _fused()(p, target.to(DEV))
    (vals * w).sum().backward()
    assert torch.equal(vals.detach(), v) and torch.equal(p.grad, g * w.reshape(-1, 1, 1, 1))


def test_fused_lpips_of_equal_images_is_exactly_zero_and_repeats():
    """target == pred in [0, 1): every value and every gradient element is exactly 0 -- which needs both halves of the batch to get
    identical bytes; and two calls return the same bytes"""
    g = torch.Generator().manual_seed(21)
    pred = torch.rand(4, 32, 32, 3, generator=g).to(DEV)
    v, d = _fused().value_and_grad(pred, pred.clone())
    assert (v == 0).all() and (d == 0).all()
    pred2, target2 = (t.to(DEV) for t in lr.whole_term_inputs(2, 16, 48, 22))
    a = [t.clone() for t in _fused().value_and_grad(pred2, target2)]
    _fused().value_and_grad(pred, pred.clone())                   # (other shapes in between: the buffers are reused)
    b = _fused().value_and_grad(pred2, target2)
    for s, t in zip(a, b):
        assert s.cpu().numpy().tobytes() == t.cpu().numpy().tobytes() and float(s.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------------------------- integration
OPT = dict(w_rgb=1.0, w_alpha=0.1, w_reg=0.1, w_lpips=0.01, w_depth_reg=0.01)


def test_training_step_hip_patch_terms_equal_the_torch_path():
    """one step from identical state and draws: patch_terms="hip" (seeded gradients) against patch_terms="torch" (the same module on the
    device, autograd) -- the two patch terms and every parameter gradient within the whole-term tolerance"""
    tol_v = FACTOR * max(_whole_reference(c)[4] for c in WHOLE_CASES)
    tol_g = FACTOR * max(_whole_reference(c)[5] for c in WHOLE_CASES)
    torch.manual_seed(0)
    dev = torch.device(DEV)
    frames, body_model, true = fit_driver.synthetic_frames(dev, res=96, n_frames=2, noise=0.03, patch=32)
    base = fit_driver.build_fit_model(frames, body_model, dev)
    opt = configure_optimizer(base, lr=1e-2, smpl_lr=1e-4)
    base.train()
    plain = NGPLoss(dict(OPT, w_lpips=0.0))
    for it in range(12):                                   # a formed field and occupancy grid first
        training_step(base, frames.batch(it % 2), opt, plain)
    state = copy.deepcopy(base.state_dict())
    grids = [(g.density_cached.clone(), g.density_field.clone(), g.occ_bits.clone()) for g in base.renderer.density_grid_train_all]
    lp = copy.deepcopy(_module()).to(DEV)
    res = {}
    for terms in ("torch", "hip"):
        model = fit_driver.build_fit_model(frames, body_model, dev)
        model.load_state_dict(state)
        model.net_coarse.mark_updated()
        model.net_coarse.initialize(base.net_coarse.bbox)
        for g, (c, f, b) in zip(model.renderer.density_grid_train_all, grids):
            g.density_cached.copy_(c); g.density_field.copy_(f); g.occ_bits.copy_(b)
        model.global_step = 41                             # not an occupancy-update step
        opt = configure_optimizer(model, lr=1e-3, smpl_lr=1e-4)
        model.train()
        loss_fn = NGPLoss(OPT, lpips=lp, patch_terms=terms)
        batch = frames.batch(0, generator=torch.Generator(device=DEV).manual_seed(5))
        n_rays = batch["rays_o"].numel() // 3
        g = torch.Generator(device=DEV).manual_seed(6)
        draws = dict(ray_jitter=torch.rand((n_rays, 256), device=DEV, generator=g), noise=torch.randn((n_rays, 256), device=DEV, generator=g))
        taken = []
        orig = loss_fn.value_and_grads
        loss_fn.value_and_grads = lambda *a, **k: (taken.append(1), orig(*a, **k))[1]
        out = training_step(model, batch, opt, loss_fn, draws=draws)
        assert bool(taken) == (terms == "hip")             # the seeded-gradient path is taken exactly with the kernels
        res[terms] = ({k: float(v) for k, v in out.items() if torch.is_tensor(v) and v.numel() == 1},
                      {n: p.grad.detach().double().cpu() for n, p in model.named_parameters() if p.grad is not None})
    (l1, g1), (l0, g0) = res["hip"], res["torch"]
    for k in ("loss_lpips", "loss_depth_reg"):
        print("step %s: hip %.9g torch %.9g rel %.3e (tolerance %.3e)" % (k, l1[k], l0[k], abs(l1[k] - l0[k]) / abs(l0[k]), tol_v))
    worst = {n: float((g1[n] - g0[n]).abs().max() / g0[n].abs().max()) for n in g0 if float(g0[n].abs().max()) > 0}
    print("step gradients, max |hip - torch| / max |torch| (tolerance %.3e):" % tol_g, {n: "%.2e" % e for n, e in worst.items()})
    assert sorted(g1) == sorted(g0) and len(worst) >= 5
    for k in ("loss_lpips", "loss_depth_reg"):
        assert l0[k] != 0 and abs(l1[k] - l0[k]) <= tol_v * abs(l0[k]), k
    assert all(e <= tol_g for e in worst.values()), worst


def _fit_setup(patch_terms="hip"):
    torch.manual_seed(0)
    dev = torch.device(DEV)
    frames, body_model, true = fit_driver.synthetic_frames(dev, res=96, n_frames=2, noise=0.0, patch=32)
    model = fit_driver.build_fit_model(frames, body_model, dev)
    opt = configure_optimizer(model, lr=1e-3, smpl_lr=1e-4)
    loss_fn = NGPLoss(OPT, lpips=copy.deepcopy(_module()).to(DEV), patch_terms=patch_terms)
    model.train()
    return frames, model, opt, loss_fn


def test_training_steps_with_hip_patch_terms():
    frames, model, opt, loss_fn = _fit_setup()
    taken = []
    orig = loss_fn.value_and_grads

    def spy(predicts, *a, **k):
        assert loss_fn.direct_backward_ok(predicts)
        losses, grads = orig(predicts, *a, **k)
        taken.append(len(grads))
        return losses, grads
    loss_fn.value_and_grads = spy
    for it in range(3):
        losses = training_step(model, frames.batch(it % 2), opt, loss_fn)
        for k in ("loss", "loss_lpips", "loss_depth_reg", "mse_loss"):
            assert torch.isfinite(losses[k]), k
        assert float(losses["loss_lpips"]) > 0 and float(losses["skipped_non_finite"]) == 0.0
    assert taken == [4, 4]                                  # steps 1 and 2 (step 0 updates the occupancy grid: autograd, by rule)
    assert model.net_coarse.encoder.params.grad.abs().sum() > 0
    for k in ("body_pose", "global_orient", "transl"):
        g = getattr(model.SMPL_param, k).weight.grad
        assert g is not None and torch.isfinite(g).all() and g.abs().sum() > 0, k


def test_graphed_fit_step_with_hip_patch_terms():
    frames, model, opt, loss_fn = _fit_setup()
    stepper = GraphedTrainStep(model, opt, loss_fn)
    assert stepper.enabled
    g = torch.Generator(device=DEV).manual_seed(2)
    for it in range(14):
        out = stepper(frames.batch(it % 2, generator=g, out=stepper.inputs))
        assert all(bool(torch.isfinite(out[k])) for k in ("loss", "loss_lpips", "loss_depth_reg")), it
        assert float(out["skipped_non_finite"]) == 0.0
    assert stepper.capture_error is None, stepper.capture_error
    assert len(stepper.graphs) == 1 and stepper.replays >= 12, (len(stepper.graphs), stepper.replays, stepper.eager_steps)
