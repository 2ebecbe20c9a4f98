"""The two patch terms of the fit stage's loss as HIP kernels (csrc/ia_lpips.hip, include/instantavatar_hip_lpips.h; definitions in
DESIGN.md section 4, "patch loss"): LPIPS with the frozen VGG-16 trunk -- value and gradient with respect to the prediction -- and
the depth regulariser.  All fp32, deterministic: two calls give the same bits.  There is no fall-back: off the GPU the calls raise.

    fused = FusedLPIPS(utils.lpips.LPIPS(net="vgg") with weights loaded)
    values, d_pred = fused.value_and_grad(pred, target)        # pred, target [n,P,Q,3] RGB in [0, 1]; values [n], d sum(values) / d pred
    values = fused(pred, target)                               # the same through autograd, differentiable in pred only
    value, d_alpha, d_depth = depth_reg_value_and_grads(alpha, depth)
    value = depth_reg(alpha, depth)                            # autograd

The trunk is frozen, so the gradient with respect to a layer's input is the SAME convolution kernel run on the adjoint weight image
(`ia_conv3x3_pack(..., transpose_flip=1)`) with the upstream gradient gated by the layer's stored output."""
import torch

from . import _lib


def _f32(buf, numel):
    return buf[:numel * 4].view(torch.float32)


class FusedLPIPS:
    """LPIPS(VGG-16) of `utils.lpips.LPIPS(net="vgg")` through the C ABI.  Weights are packed twice per layer (forward and adjoint)
    on first use on a device; activation, gradient and workspace buffers are sized on first use (`_lib.scratch`), so a captured graph
    replays with fixed pointers."""

    def __init__(self, module):
        from .utils.lpips import LPIPS
        if not isinstance(module, LPIPS):
            raise TypeError("FusedLPIPS takes a utils.lpips.LPIPS module, got %s" % type(module).__name__)
        if module.pnet_type != "vgg":
            raise ValueError("FusedLPIPS: only net='vgg' (the training loss) runs as HIP kernels; net=%r -- the eval metric's "
                             "11 x 11 stride-4 and 5 x 5 convolutions -- is out of scope, use the torch module" % (module.pnet_type,))
        self.module = module
        # the trunk as a plan: ("conv", index into self.convs) / ("pool",) / ("tap", k)
        self.plan, self.convs = [], []
        for k, s in enumerate((module.net.slice1, module.net.slice2, module.net.slice3, module.net.slice4, module.net.slice5)):
            mods = list(s)
            for i, m in enumerate(mods):
                if isinstance(m, torch.nn.Conv2d):
                    if not (m.kernel_size == (3, 3) and m.padding == (1, 1) and m.stride == (1, 1) and i + 1 < len(mods)
                            and isinstance(mods[i + 1], torch.nn.ReLU)):
                        raise ValueError("FusedLPIPS: the trunk is not 3 x 3 / padding 1 / stride 1 convolutions followed by ReLU")
                    self.plan.append(("conv", len(self.convs)))
                    self.convs.append(m)
                elif isinstance(m, torch.nn.MaxPool2d):
                    self.plan.append(("pool",))
            self.plan.append(("tap", k))
        self._device = None
        self.launches = 0          # kernel launches of the last value_and_grad (tools/time_lpips.py)

    # -- weights ----------------------------------------------------------------------------------------------------------
    def _pack(self, device):
        device = torch.device(device)
        if self._device == device:
            return
        self.fwd, self.adj, self.bias = [], [], []
        for m in self.convs:
            w = m.weight.detach().to(device=device, dtype=torch.float32).contiguous()
            co, ci = int(w.shape[0]), int(w.shape[1])
            images = []
            for tf, (cin, cout) in ((0, (ci, co)), (1, (co, ci))):
                nbytes = _lib.call("ia_conv3x3_packed_bytes", cin, cout)
                img = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
                _lib.call("ia_conv3x3_pack", w, co, ci, tf, img, nbytes)
                images.append(img)
            self.fwd.append(images[0])
            self.adj.append(images[1])
            self.bias.append(m.bias.detach().to(device=device, dtype=torch.float32).contiguous())
        self.lin = [l.model[0].weight.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous() for l in self.module.lins]
        self.shift = self.module.scaling_layer.shift.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        self.scale = self.module.scaling_layer.scale.detach().to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        self._device = device

    # -- one convolution -------------------------------------------------------------------------------------------------
    def _conv(self, x, gate, image, bias, N, cin, cout, H, W, relu, y):
        need = _lib.call("ia_conv3x3_workspace_bytes", N, cin, cout, H, W)
        ws = _lib.scratch(self, "_ws", need, x.device)
        _lib.call("ia_conv3x3", x, gate, image, bias, N, cin, cout, H, W, relu, y, ws, ws.numel())
        self.launches += 2 if cin > 32 else 1      # (more than 32 input channels: the K chunks, then their ordered sum)

    def value_and_grad(self, pred, target):
        """pred, target [n,P,Q,3] -> (values [n], d sum(values) / d pred [n,P,Q,3]).  The 2n images go through the trunk as one batch."""
        _lib.require_cuda(pred, target)
        if pred.dim() != 4 or pred.shape[-1] != 3 or pred.shape != target.shape:
            raise ValueError("FusedLPIPS: pred and target must both be [n,P,Q,3], got %s and %s" % (tuple(pred.shape), tuple(target.shape)))
        dev = pred.device
        self._pack(dev)
        pred = pred.detach().to(torch.float32).contiguous()
        target = target.detach().to(torch.float32).contiguous()
        n, P, Q = int(pred.shape[0]), int(pred.shape[1]), int(pred.shape[2])
        self.launches = 0
        # forward: every activation of the 2n images is kept (the gates and pool routes of the backward pass read the first n)
        x = _f32(_lib.scratch(self, "_act_in", 2 * n * 3 * P * Q * 4, dev), 2 * n * 3 * P * Q)
        _lib.call("ia_lpips_prepare", pred, target, self.shift, self.scale, n, P, Q, x)
        self.launches += 1
        C, H, W = 3, P, Q
        acts = []                  # per plan entry: (input tensor, output tensor, C_in, C_out, H_in, W_in)
        values = torch.empty(n, dtype=torch.float32, device=dev)
        taps = []
        for j, op in enumerate(self.plan):
            if op[0] == "conv":
                m = self.convs[op[1]]
                co = int(m.weight.shape[0])
                y = _f32(_lib.scratch(self, "_act%d" % j, 2 * n * co * H * W * 4, dev), 2 * n * co * H * W)
                self._conv(x, None, self.fwd[op[1]], self.bias[op[1]], 2 * n, C, co, H, W, 1, y)
                acts.append((x, y, C, co, H, W))
                x, C = y, co
            elif op[0] == "pool":
                if H < 2 or W < 2:
                    raise ValueError("FusedLPIPS: patches of %d x %d are too small for the trunk's four 2 x 2 pools" % (P, Q))
                y = _f32(_lib.scratch(self, "_act%d" % j, 2 * n * C * (H // 2) * (W // 2) * 4, dev), 2 * n * C * (H // 2) * (W // 2))
                _lib.call("ia_maxpool2x2", x, 2 * n * C, H, W, y)
                self.launches += 1
                acts.append((x, y, C, C, H, W))
                x, H, W = y, H // 2, W // 2
            else:
                hws = _lib.scratch(self, "_head_ws", _lib.call("ia_lpips_head_workspace_bytes", n, H * W), dev)
                _lib.call("ia_lpips_head", x, self.lin[op[1]], n, C, H * W, 1 if op[1] > 0 else 0, values, hws, hws.numel())
                self.launches += 2                 # (the workgroups' sums, then their ordered sum)
                acts.append((x, x, C, C, H, W))
                taps.append(op[1])
        # backward over the first n images: two gradient buffers, written alternately
        big = max(n * max(a[2], a[3]) * a[4] * a[5] for a in acts)
        gbuf = [_f32(_lib.scratch(self, "_grad%d" % i, big * 4, dev), big) for i in (0, 1)]
        cur = None                 # index of the buffer holding the gradient of the current activation, None before tap 5
        for j in range(len(self.plan) - 1, -1, -1):
            op = self.plan[j]
            xin, y, ci, co, H, W = acts[j]
            if op[0] == "tap":
                dst = 0 if cur is None else cur
                _lib.call("ia_lpips_head_bwd", y, self.lin[op[1]], n, co, H * W, 0 if cur is None else 1, gbuf[dst])
                self.launches += 1
                cur = dst
            elif op[0] == "pool":
                _lib.call("ia_maxpool2x2_bwd", xin, gbuf[cur], n * ci, H, W, gbuf[1 - cur])
                self.launches += 1
                cur = 1 - cur
            else:
                self._conv(gbuf[cur], y, self.adj[op[1]], None, n, co, ci, H, W, 0, gbuf[1 - cur])
                cur = 1 - cur
        d_pred = torch.empty_like(pred)
        _lib.call("ia_lpips_prepare_bwd", pred, gbuf[cur], self.scale, n, P, Q, d_pred)
        self.launches += 1
        return values, d_pred

    def __call__(self, pred, target):
        """values [n], differentiable in `pred` only."""
        return _LPIPSFn.apply(pred, target, self)


class _LPIPSFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, fused):
        values, d_pred = fused.value_and_grad(pred, target)
        ctx.save_for_backward(d_pred)
        ctx.dtype = pred.dtype
        return values

    @staticmethod
    def backward(ctx, g):
        d_pred, = ctx.saved_tensors
        return (d_pred * g.reshape(-1, 1, 1, 1)).to(ctx.dtype), None, None


def depth_reg_value_and_grads(alpha, depth):
    """alpha, depth [..., P, Q] (the leading dimensions count the patches) -> (value [], d value / d alpha, d value / d depth):
    value = mean(alpha |depth - avg|), avg = sum(depth alpha) / (sum alpha + 1e-3) per patch (the reference's loss.py:33-39)."""
    _lib.require_cuda(alpha, depth)
    if alpha.shape != depth.shape or alpha.dim() < 2:
        raise ValueError("depth_reg: alpha and depth must have one shape [..., P, Q], got %s and %s" % (tuple(alpha.shape), tuple(depth.shape)))
    a = alpha.detach().to(torch.float32).contiguous()
    d = depth.detach().to(torch.float32).contiguous()
    pq = int(a.shape[-1]) * int(a.shape[-2])
    value = torch.empty(1, dtype=torch.float32, device=a.device)
    d_a, d_d = torch.empty_like(a), torch.empty_like(d)
    _lib.call("ia_patch_depth_reg", a, d, a.numel() // pq, pq, value, d_a, d_d)
    return value[0], d_a, d_d


class _DepthRegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, depth):
        value, d_a, d_d = depth_reg_value_and_grads(alpha, depth)
        ctx.save_for_backward(d_a, d_d)
        ctx.dtypes = alpha.dtype, depth.dtype
        return value

    @staticmethod
    def backward(ctx, g):
        d_a, d_d = ctx.saved_tensors
        return (d_a * g).to(ctx.dtypes[0]), (d_d * g).to(ctx.dtypes[1])


def depth_reg(alpha, depth):
    """The depth regulariser through autograd (one launch forward, the stored gradients scaled backward)."""
    return _DepthRegFn.apply(alpha, depth)
