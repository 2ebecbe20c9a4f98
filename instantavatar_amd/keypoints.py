"""Refinement of a custom sequence's SMPL parameters against 2D keypoints (scripts/custom/refine-smpl.py of the reference, its
keypoint stage): the loss over all frames and its gradient are the HIP kernels of csrc/ia_keypoints.hip (`ia_kp_loss_fwd`,
`ia_kp_loss_bwd`), the optimiser step is `FusedAdam` (`ia_adam_step`).  Definition: DESIGN.md section 4, "keypoint refinement".

    r = KeypointRefiner(body_model, proj, keypoints, threshold=0.2)
    r.loss(betas, pose, transl)            -> {"loss", "loss_kp", "loss_t"} device scalars (+ verts, points, uv)
                                              (verts is the refiner's own buffer: the next call overwrites it)
    r.loss_and_grad(betas, pose, transl)   -> (that dict, {"betas", "pose", "transl"} gradients)
    r.refine(betas, pose, transl)          -> (betas, pose, transl, losses [steps, 3])

betas [10], pose [F,72] (global_orient then body_pose, axis-angle), transl [F,3]; proj [3,4] = intrinsic @ extrinsic[:3];
keypoints [F,25,3] (x, y, confidence; BODY_25 order).  There is no CPU path.  The `--silhouette` stage of the reference (LBFGS per
frame through a soft rasteriser) is instantavatar_amd/silhouette.py.
"""
import numpy as np
import torch

from . import _lib
from .optim import FusedAdam

#: BODY_25 point k is model point BODY25_TO_POINT[k]: the 24 SMPL joints, then the 11 vertices of SMPL_KP_VERTEX (refine-smpl.py:74-84)
BODY25_TO_POINT = (24, 12, 17, 19, 21, 16, 18, 20, 0, 2, 5, 8, 1, 4, 7, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34)
MIDHIP = 8      # not in the loss (refine-smpl.py:133-134)
#: SMPL vertices that stand in for nose, right eye, left eye, right ear, left ear, left big toe, left small toe, left heel, right big
#: toe, right small toe, right heel (smplx's vertex_ids, "smpl")
SMPL_KP_VERTEX = (332, 6260, 2800, 4071, 583, 3216, 3226, 3387, 6617, 6624, 6787)


class KeypointRefiner:
    def __init__(self, body_model, proj, keypoints, threshold=0.2, kp_vertex=SMPL_KP_VERTEX):
        """body_model: deformers.smplx.SMPL on the GPU; proj [3,4]; keypoints [F,25,3]; kp_vertex: 11 vertex indices below V"""
        self.body, self._keep = body_model.lbs_constants()
        dev = self._keep["v_template"].device
        if dev.type != "cuda":
            raise _lib.IAError("KeypointRefiner: the body model must be on the GPU (got %s); there is no CPU path" % dev)
        self.device, self.V = dev, int(self.body.n_verts)
        f32 = lambda a: torch.as_tensor(np.asarray(a, np.float32) if not torch.is_tensor(a) else a).to(device=dev, dtype=torch.float32).contiguous()
        self.proj, self.keypoints = f32(proj), f32(keypoints)
        if tuple(self.proj.shape) != (3, 4):
            raise ValueError("KeypointRefiner: proj must be [3,4], got %s" % (tuple(self.proj.shape),))
        if self.keypoints.dim() != 3 or tuple(self.keypoints.shape[1:]) != (25, 3):
            raise ValueError("KeypointRefiner: keypoints must be [F,25,3], got %s" % (tuple(self.keypoints.shape),))
        kv = [int(v) for v in kp_vertex]
        if len(kv) != 11 or min(kv) < 0 or max(kv) >= self.V:
            raise ValueError("KeypointRefiner: kp_vertex must hold 11 vertex indices in [0, %d), got %s" % (self.V, kv))
        self.kp_vertex = torch.tensor(kv, dtype=torch.int32, device=dev)
        self.F, self.threshold = int(self.keypoints.shape[0]), float(threshold)
        need = _lib.call("ia_kp_workspace_bytes", self.F, self.V)
        if need == 0:
            raise ValueError("KeypointRefiner: %d frames of %d vertices are outside what ia_kp_loss_fwd takes" % (self.F, self.V))
        self._ws = torch.empty(int(need), dtype=torch.uint8, device=dev)
        self._verts = torch.empty((self.F, self.V, 3), device=dev)

    def _args(self, betas, pose, transl):
        b, p, t = (x.detach().float().contiguous() for x in (betas.reshape(-1)[:10], pose.reshape(-1, 72), transl.reshape(-1, 3)))
        if p.shape[0] != self.F or t.shape[0] != self.F or b.numel() != 10:
            raise ValueError("KeypointRefiner: betas [10], pose [%d,72], transl [%d,3] expected, got %s, %s, %s"
                             % (self.F, self.F, tuple(betas.shape), tuple(pose.shape), tuple(transl.shape)))
        return b, p, t

    def _fwd(self, b, p, t, loss, points=None, uv=None):
        _lib.call("ia_kp_loss_fwd", self.body, b, p, t, self.F, self.proj, self.keypoints, self.threshold, self.kp_vertex, self._verts, points, uv,
                  loss, self._ws, self._ws.numel())

    def _bwd(self, b, p, t, d_b, d_p, d_t):
        _lib.call("ia_kp_loss_bwd", self.body, b, p, t, self.F, self.proj, self.keypoints, self.threshold, self.kp_vertex, self._verts, d_b, d_p, d_t,
                  self._ws, self._ws.numel())

    def loss(self, betas, pose, transl):
        b, p, t = self._args(betas, pose, transl)
        loss = torch.empty(3, device=self.device)
        points, uv = torch.empty((self.F, 35, 3), device=self.device), torch.empty((self.F, 25, 2), device=self.device)
        self._fwd(b, p, t, loss, points, uv)
        return dict(loss=loss[0], loss_kp=loss[1], loss_t=loss[2], verts=self._verts, points=points, uv=uv)

    def loss_and_grad(self, betas, pose, transl):
        b, p, t = self._args(betas, pose, transl)
        out = self.loss(b, p, t)
        g = dict(betas=torch.empty(10, device=self.device), pose=torch.empty((self.F, 72), device=self.device), transl=torch.empty((self.F, 3), device=self.device))
        self._bwd(b, p, t, g["betas"], g["pose"], g["transl"])
        return out, g

    def refine(self, betas, pose, transl, steps=200, lr=1e-3, log=None):
        """Adam (torch.optim.Adam's defaults, refine-smpl.py:186) on one tensor each for betas, pose and transl, `steps` steps of the
        plain eager loop.  -> (betas [10], pose [F,72], transl [F,3], losses [steps,3]: L, L_kp, L_t BEFORE each step, one device
        tensor).  log: optional callable(str), called once at the end (the only host read of the loop is made for it)."""
        b, p, t = (torch.nn.Parameter(x.clone()) for x in self._args(betas, pose, transl))
        for x in (b, p, t):
            x.grad = torch.empty_like(x)
        opt = FusedAdam([b, p, t], lr=lr)
        losses = torch.empty((int(steps), 3), device=self.device)
        for i in range(int(steps)):
            self._fwd(b.data, p.data, t.data, losses[i])
            self._bwd(b.data, p.data, t.data, b.grad, p.grad, t.grad)
            opt.step()
        if log is not None and steps > 0:
            h = losses.cpu().numpy()
            log("keypoint refinement: %d steps, loss %.6f -> %.6f (keypoints %.6f -> %.6f, temporal %.6f -> %.6f)"
                % (steps, h[0, 0], h[-1, 0], h[0, 1], h[-1, 1], h[0, 2], h[-1, 2]))
        return b.detach(), p.detach(), t.detach(), losses
