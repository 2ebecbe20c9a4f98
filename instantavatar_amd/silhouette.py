"""A differentiable soft silhouette of a triangle mesh, and the refinement of a custom sequence's SMPL poses against its masks with it
(scripts/custom/refine-smpl.py of the reference, its `--silhouette` stage: LBFGS per frame over pose and translation, the loss the MSE
between the mask and a soft silhouette that the reference renders with pytorch3d).  Projection, render, their backward passes and the
body model's adjoint are the HIP kernels of csrc/ia_silhouette.hip and csrc/ia_keypoints.hip (include/instantavatar_hip_silhouette.h);
the optimiser is torch.optim.LBFGS.  Definition: DESIGN.md section 4, "silhouette refinement".  There is no CPU path.

    s = SoftSilhouette(faces, camera, sigma=1e-4, blur_radius=None)      camera: raster.Camera; blur_radius None = log(1 / 1e-4 - 1) sigma
    s.render(verts)                  -> alpha [H,W]
    s.loss_and_grad(verts, mask)     -> (loss, d_verts [nv,3]) of L = mean (alpha - mask)^2
    soft_silhouette(verts, faces, camera, ...)   -> alpha [H,W], differentiable in verts inside a torch graph

    r = SilhouetteRefiner(body_model, faces, camera, masks, sigma, blur_radius)      masks [F,H,W] in [0, 1]
    r.loss(pose, transl, betas, frame) / r.loss_and_grad(...)          pose [F,72], transl [F,3], betas [10]
    r.refine(betas, pose, transl, iters=10)   -> (pose, transl, losses [F,2]: the loss at the start and at the end of each frame)
"""
import math

import numpy as np
import torch

from . import _lib


def default_blur_radius(sigma):
    """refine-smpl.py:59: blur_radius = log(1 / 1e-4 - 1) * sigma"""
    return math.log(1.0 / 1e-4 - 1.0) * float(sigma)


def vertex_faces(faces, nv):
    """The vertex-to-face list `ia_sil_render_bwd` gathers over, built once per topology on the device: (vf_start [nv+1], vf_corner [n])
    int32, the corners 3 f + c of every vertex in ascending order; faces with an index outside [0, nv) are left out."""
    f = faces.reshape(-1, 3).to(torch.int64)
    ok = ((f >= 0) & (f < nv)).all(1)
    corner = (torch.arange(f.shape[0], device=f.device)[:, None] * 3 + torch.arange(3, device=f.device))[ok].reshape(-1)
    vert = f[ok].reshape(-1)
    order = torch.sort(vert, stable=True)[1]
    start = torch.zeros(nv + 1, dtype=torch.int64, device=f.device)
    if vert.numel():
        start[1:] = torch.cumsum(torch.bincount(vert, minlength=nv), 0)
    return start.to(torch.int32).contiguous(), corner[order].to(torch.int32).contiguous()


class SoftSilhouette:
    def __init__(self, faces, camera, sigma=1e-4, blur_radius=None):
        """faces [nf,3] integer tensor on the GPU; camera: raster.Camera (its w2c may change between calls without a host copy)"""
        _lib.require_cuda(faces, camera.w2c)
        self.faces = faces.detach().reshape(-1, 3).to(torch.int32).contiguous()
        self.camera, self.device = camera, self.faces.device
        self.sigma = float(sigma)
        self.blur_radius = default_blur_radius(sigma) if blur_radius is None else float(blur_radius)
        self.nf, self.H, self.W = int(self.faces.shape[0]), camera.H, camera.W
        self._nv = self._vf = self._ws = None

    def _for(self, nv):
        if self._nv != nv:
            need = int(_lib.call("ia_sil_workspace_bytes", nv, self.nf, self.H, self.W))
            if need == 0:
                raise _lib.IAError("SoftSilhouette: %d vertices, %d faces, a %d x %d image: outside 1 <= H, W <= 16384" % (nv, self.nf, self.H, self.W))
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._vf = vertex_faces(self.faces, nv)
            self._nv = nv

    def _verts(self, verts):
        _lib.require_cuda(verts)
        v = verts.detach().reshape(-1, 3).float().contiguous()
        self._for(int(v.shape[0]))
        return v

    def _cam(self):
        c = self.camera
        return (c.w2c, c.fx, c.fy, c.cx, c.cy, c.near)

    def project(self, verts):
        """-> (screen [nv,2] pixels, inv_z [nv]; zeros for an invalid vertex)"""
        v = self._verts(verts)
        screen, inv_z = torch.empty((v.shape[0], 2), device=self.device), torch.empty(v.shape[0], device=self.device)
        _lib.call("ia_sil_project_fwd", v, v.shape[0], *self._cam(), screen, inv_z)
        return screen, inv_z

    def _render(self, screen, inv_z, mask=None, want_alpha=True):
        n = self.H * self.W
        alpha = torch.empty(n, device=self.device) if want_alpha else None
        loss = d_alpha = None
        if mask is not None:
            mask = mask.detach().reshape(-1).float().contiguous()
            if mask.numel() != n:
                raise ValueError("SoftSilhouette: the mask has %d values, the image %d x %d" % (mask.numel(), self.H, self.W))
            loss, d_alpha = torch.empty(1, device=self.device), torch.empty(n, device=self.device)
        _lib.call("ia_sil_render_fwd", screen, inv_z, self._nv, self.faces, self.nf, self.H, self.W, self.sigma, self.blur_radius, mask, alpha, loss,
                  d_alpha, self._ws, self._ws.numel())
        return alpha, loss, d_alpha

    def _backward(self, v, screen, inv_z, alpha, d_alpha):
        d_screen, d_verts = torch.empty_like(screen), torch.empty_like(v)
        _lib.call("ia_sil_render_bwd", screen, inv_z, self._nv, self.faces, self.nf, self.H, self.W, self.sigma, self.blur_radius, alpha, d_alpha,
                  self._vf[0], self._vf[1], d_screen, self._ws, self._ws.numel())
        _lib.call("ia_sil_project_bwd", v, v.shape[0], *self._cam(), d_screen, d_verts)
        return d_verts

    @torch.no_grad()
    def render(self, verts):
        screen, inv_z = self.project(verts)
        return self._render(screen, inv_z)[0].view(self.H, self.W)

    @torch.no_grad()
    def loss_and_grad(self, verts, mask):
        """-> (loss: device scalar, d_verts [nv,3]) of L = sum (alpha - mask)^2 / (H W)"""
        v = self._verts(verts)
        screen, inv_z = self.project(v)
        alpha, loss, d_alpha = self._render(screen, inv_z, mask)
        return loss[0], self._backward(v, screen, inv_z, alpha, d_alpha)


class _SoftSilhouetteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, sil):
        v = sil._verts(verts)
        screen, inv_z = sil.project(v)
        alpha = sil._render(screen, inv_z)[0]
        ctx.save_for_backward(v, screen, inv_z, alpha)
        ctx.sil, ctx.shape = sil, verts.shape
        return alpha.view(sil.H, sil.W)

    @staticmethod
    def backward(ctx, grad):
        v, screen, inv_z, alpha = ctx.saved_tensors
        sil = ctx.sil
        sil._for(int(v.shape[0]))
        d_verts = sil._backward(v, screen, inv_z, alpha, grad.detach().reshape(-1).float().contiguous())
        return d_verts.view(ctx.shape), None


def soft_silhouette(verts, faces, camera, sigma=1e-4, blur_radius=None, renderer=None):
    """alpha [H,W] of the mesh, differentiable in verts.  renderer: a SoftSilhouette to reuse (its topology lists and workspace)"""
    return _SoftSilhouetteFn.apply(verts, renderer if renderer is not None else SoftSilhouette(faces, camera, sigma, blur_radius))


class SilhouetteRefiner:
    def __init__(self, body_model, faces, camera, masks, sigma=1e-4, blur_radius=None):
        """body_model: deformers.smplx.SMPL on the GPU; faces [nf,3] (SMPL.faces_tensor); masks [F,H,W] in [0, 1] (uint8: / 255)"""
        self.body, self._keep = body_model.lbs_constants()
        dev = self._keep["v_template"].device
        if dev.type != "cuda":
            raise _lib.IAError("SilhouetteRefiner: the body model must be on the GPU (got %s); there is no CPU path" % dev)
        self.device, self.V = dev, int(self.body.n_verts)
        faces = torch.as_tensor(np.asarray(faces)) if not torch.is_tensor(faces) else faces
        if faces.numel() == 0:
            raise ValueError("SilhouetteRefiner: the body model has no faces (an SMPL file without `f`, or a synthetic body without triangles)")
        self.sil = SoftSilhouette(faces.to(dev), camera, sigma, blur_radius)
        m = torch.as_tensor(np.asarray(masks)) if not torch.is_tensor(masks) else masks
        m = m.to(dev)
        self.masks = (m.float() / 255 if m.dtype == torch.uint8 else m.float()).contiguous()
        if self.masks.dim() != 3 or tuple(self.masks.shape[1:]) != (camera.H, camera.W):
            raise ValueError("SilhouetteRefiner: masks must be [F,%d,%d], got %s" % (camera.H, camera.W, tuple(self.masks.shape)))
        self.F = int(self.masks.shape[0])
        need_v, need_b = _lib.call("ia_kp_workspace_bytes", 1, self.V), _lib.call("ia_sil_body_workspace_bytes", 1, self.V)
        if need_v == 0 or need_b == 0:
            raise ValueError("SilhouetteRefiner: a body of %d vertices is outside what the body-model kernels take" % self.V)
        self._ws = torch.empty(int(max(need_v, need_b)), dtype=torch.uint8, device=dev)
        self._verts = torch.empty((1, self.V, 3), device=dev)
        # ia_kp_loss_fwd is the forward of vert[f,v]; its keypoint part gets a camera that cannot divide by zero and no live keypoint
        self._proj = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 0, 1.0]], device=dev)
        self._kp, self._kpv = torch.zeros((1, 25, 3), device=dev), torch.zeros(11, dtype=torch.int32, device=dev)

    def _row(self, pose, transl, betas, frame):
        p, t = pose.detach().reshape(-1, 72).float(), transl.detach().reshape(-1, 3).float()
        f = int(frame)
        if not 0 <= f < self.F:
            raise ValueError("SilhouetteRefiner: frame %d outside [0, %d)" % (f, self.F))
        p, t = (x[f if x.shape[0] > 1 else 0].contiguous() for x in (p, t))
        return p, t, betas.detach().reshape(-1)[:10].float().contiguous(), f

    def _posed(self, b, p, t):
        _lib.call("ia_kp_loss_fwd", self.body, b, p, t, 1, self._proj, self._kp, 0.5, self._kpv, self._verts, None, None, None, self._ws, self._ws.numel())
        return self._verts[0]

    @torch.no_grad()
    def loss(self, pose, transl, betas, frame):
        """pose [F,72] (or the frame's [72]), transl [F,3] (or [3]), betas [10] -> the frame's loss, a device scalar"""
        p, t, b, f = self._row(pose, transl, betas, frame)
        v = self._posed(b, p, t)
        screen, inv_z = self.sil.project(v)
        return self.sil._render(screen, inv_z, self.masks[f], want_alpha=False)[1][0]

    @torch.no_grad()
    def loss_and_grad(self, pose, transl, betas, frame, out=None):
        """-> (loss, {"pose": [72], "transl": [3]}); out: a [75] tensor the two gradients are written into instead (pose, then transl)"""
        p, t, b, f = self._row(pose, transl, betas, frame)
        loss, d_verts = self.sil.loss_and_grad(self._posed(b, p, t), self.masks[f])
        g = torch.empty(75, device=self.device) if out is None else out
        _lib.call("ia_sil_body_bwd", self.body, b, p, t, 1, d_verts, None, g[:72], g[72:], self._ws, self._ws.numel())
        return loss, dict(pose=g[:72], transl=g[72:])

    def refine(self, betas, pose, transl, iters=10, log=None, frames=None, trace=None):
        """For each frame in turn (frames: an iterable of frame indices, None = all), torch.optim.LBFGS(line_search_fn="strong_wolfe")
        with torch's defaults takes `iters` calls of .step(closure) on one flat 75-float parameter, the frame's pose and translation
        (refine-smpl.py:220-252: every other gradient of its LBFGS over all parameters is zero; betas stay fixed, :229).
        -> (pose [F,72], transl [F,3], losses [F,2]: the loss at the start and at the end of each refined frame, NaN for the others).
        trace: a list that receives (frame, loss, gradient [75]) of every closure evaluation.  log: callable(str), once per frame."""
        pose, transl = pose.detach().reshape(-1, 72).float().clone(), transl.detach().reshape(-1, 3).float().clone()
        if pose.shape[0] != self.F or transl.shape[0] != self.F:
            raise ValueError("SilhouetteRefiner: pose [%d,72] and transl [%d,3] expected, got %s and %s" % (self.F, self.F, tuple(pose.shape), tuple(transl.shape)))
        b = betas.detach().reshape(-1)[:10].float().contiguous()
        losses = torch.full((self.F, 2), float("nan"), device=self.device)
        for f in (range(self.F) if frames is None else frames):
            x = torch.nn.Parameter(torch.cat([pose[f], transl[f]]))
            x.grad = torch.zeros_like(x)
            opt = torch.optim.LBFGS([x], line_search_fn="strong_wolfe")
            first = []

            def closure():
                loss, _ = self.loss_and_grad(x.data[:72], x.data[72:], b, f, out=x.grad)
                if not first:
                    first.append(loss)
                if trace is not None:
                    trace.append((f, loss, x.grad.clone()))
                return loss

            for _ in range(int(iters)):
                opt.step(closure)
            pose[f], transl[f] = x.data[:72], x.data[72:]
            losses[f, 0] = first[0] if first else self.loss(pose, transl, b, f)
            losses[f, 1] = self.loss(pose, transl, b, f)
            if log is not None:
                log("silhouette refinement: frame %d, %d LBFGS steps, loss %.6f -> %.6f" % (f, iters, float(losses[f, 0]), float(losses[f, 1])))
        return pose, transl, losses
