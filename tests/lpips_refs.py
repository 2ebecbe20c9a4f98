"""Float64 restatements of the patch-loss kernels (include/instantavatar_hip_lpips.h, DESIGN.md section 4 "patch loss") in closed form
-- the input preparation, the LPIPS head, the pool routing and the depth term with their gradients -- plus the seeded stand-in weights
and inputs the tests share.  tests/test_cpu_lpips_refs.py pins these to autograd through the torch expressions of `NGPLoss(fused=False)`
and `utils.lpips.LPIPS`; tests/test_gpu_lpips.py compares the kernels against them and against the float64 module."""
import copy

import numpy as np
import torch
import torch.nn.functional as F

from instantavatar_amd.utils.lpips import LPIPS


def seeded_lpips(seed=0):
    """LPIPS(net="vgg") with weights of its own (the pretrained ones cannot be fetched): He-normal convolutions, biases uniform in
    +-0.1, `lin` weights uniform in [0, 1) so that the value is a distance."""
    m = LPIPS()
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        with torch.no_grad():
            for mod in m.net.modules():
                if isinstance(mod, torch.nn.Conv2d):
                    torch.nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
                    mod.bias.uniform_(-0.1, 0.1)
            for lin in m.lins:
                lin.model[0].weight.uniform_(0, 1)
    m.weights_loaded = {"trunk": True, "lin": True}
    return m


def whole_term_inputs(n, P, Q, seed, close=False):
    """pred uniform in [0, 1.2) (the clip is exercised, no element exactly 1), target uniform in [0, 1); close: target = pred + 0.02
    noise clipped to [0, 1], the small-distance regime."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.rand(n, P, Q, 3, generator=g) * 1.2
    pred[pred == 1] = 0.5
    if close:
        target = (pred + 0.02 * torch.randn(n, P, Q, 3, generator=g)).clip(0, 1)
    else:
        target = torch.rand(n, P, Q, 3, generator=g)
    return pred, target


def module_value_and_grad(module, pred, target, dtype=torch.float64, memory_format=None, hooks=None):
    """values [n] and d sum(values) / d pred of the torch module under autograd, with NGPLoss's own preparation (training.py: BGR
    order, NCHW, clip).  hooks: a list that receives every convolution's output (the pre-activations)."""
    m = copy.deepcopy(module).to(dtype)       # (nn.Module.to converts in place: the caller's fp32 module stays as it is)
    pr0 = pred.detach().to(dtype).requires_grad_(True)
    pr = pr0[..., [2, 1, 0]].permute(0, 3, 1, 2).clip(max=1)
    tg = target.detach().to(dtype)[..., [2, 1, 0]].permute(0, 3, 1, 2)
    if memory_format is not None:
        pr, tg = pr.contiguous(memory_format=memory_format), tg.contiguous(memory_format=memory_format)
    handles = []
    if hooks is not None:
        for mod in m.net.modules():
            if isinstance(mod, torch.nn.Conv2d):
                handles.append(mod.register_forward_hook(lambda _m, _i, out: hooks.append(out.detach())))
    try:
        v = m(pr, tg).reshape(-1)
        g, = torch.autograd.grad(v.sum(), pr0)
    finally:
        for h in handles:
            h.remove()
    return v.detach(), g.detach()


# ---- closed forms, float64 ------------------------------------------------------------------------------------------------------
def prepare(pred, target, shift, scale):
    """[n,P,Q,3] x 2 -> [2n,3,P,Q], predictions first"""
    both = torch.cat([pred.double().clip(max=1), target.double()])[..., [2, 1, 0]].permute(0, 3, 1, 2)
    return ((2 * both - 1) - shift.double().reshape(1, 3, 1, 1)) / scale.double().reshape(1, 3, 1, 1)


def prepare_bwd(pred, g, scale):
    """g [n,3,P,Q] -> d pred [n,P,Q,3]: passes where pred <= 1"""
    d = (g.double() / scale.double().reshape(1, 3, 1, 1) * 2).permute(0, 2, 3, 1)[..., [2, 1, 0]]
    return torch.where(pred.double() <= 1, d, torch.zeros_like(d))


def head(feat, lin):
    """feat [2n,C,HW], lin [C] -> values [n]"""
    n = feat.shape[0] // 2
    f = feat.double()
    u = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    return ((u[:n] - u[n:]).pow(2) * lin.double().reshape(1, -1, 1)).sum(1).mean(1)


def head_bwd(feat, lin):
    """d sum(values) / d feat[:n], closed form: q / na - (sum_c q_c a_c) a / (na^2 sqrt(sa)), q = 2 lin (u - v) / HW"""
    n, hw = feat.shape[0] // 2, feat.shape[2]
    f = feat.double()
    s = f.pow(2).sum(1, keepdim=True)
    na = s.sqrt() + 1e-10
    u = f / na
    q = 2 * lin.double().reshape(1, -1, 1) * (u[:n] - u[n:]) / hw
    a, ra, nn = f[:n], s[:n].sqrt(), na[:n]
    coef = torch.where(s[:n] > 0, (q * a).sum(1, keepdim=True) / (nn * nn * ra.clamp_min(1e-300)), torch.zeros_like(ra))
    return q / nn - coef * a


def pool(x):
    """[NC,H,W] numpy -> (y [NC,H/2,W/2], arg: index 0..3 of the FIRST maximum of each window in row-major order)"""
    nc, H, W = x.shape
    oh, ow = H // 2, W // 2
    win = np.stack([x[:, 0:2 * oh:2, 0:2 * ow:2], x[:, 0:2 * oh:2, 1:2 * ow:2], x[:, 1:2 * oh:2, 0:2 * ow:2], x[:, 1:2 * oh:2, 1:2 * ow:2]], -1)
    arg = win.argmax(-1)                        # numpy: the first occurrence
    return np.take_along_axis(win, arg[..., None], -1)[..., 0], arg


def pool_bwd(x, dy):
    nc, H, W = x.shape
    _, arg = pool(x)
    dx = np.zeros_like(x)
    oh, ow = H // 2, W // 2
    for k in range(4):
        sel = arg == k
        view = dx[:, (k >> 1):2 * oh:2, (k & 1):2 * ow:2]
        view[sel] = dy[sel]
    return dx


def depth_reg(alpha, depth):
    """alpha, depth [n_patch,PQ] -> (value, d alpha, d depth), float64 (loss.py:33-39 with the paths through avg; sign(0) = 0)"""
    a, d = alpha.double(), depth.double()
    A = a.sum(1, keepdim=True) + 1e-3
    avg = (d * a).sum(1, keepdim=True) / A
    e = d - avg
    sg = torch.sign(e)
    T = (a * sg).sum(1, keepdim=True)
    n = a.numel()
    return (a * e.abs()).sum() / n, (e.abs() - T * e / A) / n, (a * sg - T * a / A) / n


# ---- convolution ----------------------------------------------------------------------------------------------------------------
def conv_ref_and_bound(x, gate, w, b, relu):
    """float64 convolution of the fp32 operands and the a-priori bound (K + 2) 2^-24 (conv(|x|, |w|) + |b|), K = 9 Cin, of any fp32
    summation order, with or without fused multiply-add"""
    x64 = x.double() if gate is None else x.double() * (gate > 0).double()
    w64, b64 = w.double(), (b.double() if b is not None else None)
    y = F.conv2d(x64, w64, b64, padding=1)
    mag = F.conv2d(x64.abs(), w64.abs(), None, padding=1) + (b64.abs().reshape(1, -1, 1, 1) if b is not None else 0)
    K = 9 * x.shape[1]
    return (F.relu(y) if relu else y), (K + 2) * 2.0 ** -24 * mag
