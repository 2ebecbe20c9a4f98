"""SNARFDeformer plugin (drop-in for instant_avatar/deformers/snarf_deformer.py:33).

Same constructor and methods as the reference class so that
`confs/deformer/fast_snarf.yaml` only needs its `_target_` re-pointed:

    SNARFDeformer(model_path, gender, opt)
    .prepare_deformer(smpl_params)   .transform_rays_w2s(rays)
    .get_bbox_deformed()             .__call__(pts, model, eval_mode)
    attributes: bbox, vertices, w2s, tfs, initialized, body_model

Per-frame work runs on the GPU without host synchronisation: the SMPL joint
chain + tfs in `ia_smpl_tfs`, the voxel transforms in `ia_precompute`; the
field query `deformer(pts, net)` is the fused `ia_deform_query` when `net` is
an instantavatar_amd NeRFNGPNet, and the generic masked path (reference
structure, snarf_deformer.py:127-159) for any other callable.
"""
import os

import numpy as np
import torch

from . import _opt
from .. import _lib
from ..training import DeferredCount, field_autograd
from .fast_snarf.forward_deformer import ForwardDeformer
from .smplx import SMPL


def get_predefined_rest_pose(cano_pose, device="cuda"):
    """snarf_deformer.py:6-18"""
    presets = {"da_pose": {2: torch.pi / 6, 5: -torch.pi / 6},
               "a_pose": {2: 0.2, 5: -0.2, 47: -0.8, 50: 0.8}}
    key = cano_pose.lower()
    if key not in presets:
        raise ValueError("Unknown cano_pose: {}".format(cano_pose))
    pose = torch.zeros((1, 69), device=device)
    for i, v in presets[key].items():
        pose[:, i] = v
    return pose


def get_bbox_from_smpl(vs, factor=1.2):
    """snarf_deformer.py:20-31: cube around the vertices, half-size = factor * max half extent."""
    assert vs.shape[0] == 1
    lo, hi = vs.min(dim=1).values, vs.max(dim=1).values
    c = (hi + lo) / 2
    s = ((hi - lo) / 2).max(dim=-1).values * factor
    return torch.cat([c - s[:, None], c + s[:, None]], dim=0)


#: prepare_deformer's backward through `ia_smpl_tfs_bwd` (False: lbs.py-style torch ops under autograd, the kernels' checker)
FUSED_SMPL_BACKWARD = True


def affine_inverse(A):
    """Inverse of affine 4x4 matrices [..., 4, 4] with last row (0, 0, 0, 1): M^-1 = adj(M) / det(M) by cross products of
    the rows of M, translation -M^-1 t.  Differentiable, no solver library, no host synchronisation."""
    M, t = A[..., :3, :3], A[..., :3, 3]
    r0, r1, r2 = M[..., 0, :], M[..., 1, :], M[..., 2, :]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    det = (r0 * c0).sum(-1, keepdim=True)
    Minv = torch.stack([c0, c1, c2], dim=-1) / det[..., None]
    top = torch.cat([Minv, -(Minv @ t[..., None])], dim=-1)
    bottom = torch.zeros_like(top[..., :1, :])
    bottom[..., 0, 3] = 1.0
    return torch.cat([top, bottom], dim=-2)


def _abs_path(p):
    try:
        import hydra
        return hydra.utils.to_absolute_path(p)
    except Exception:
        return os.path.abspath(p) if isinstance(p, str) else p


class _CandidateGatherFn(torch.autograd.Function):
    """rgb / sigma of the winning candidate per point (torch.max + torch.gather of snarf_deformer.py:150-158)."""

    @staticmethod
    def forward(ctx, cand_rgb, cand_sigma, arg, fill):
        cand_rgb, cand_sigma = cand_rgb.contiguous(), cand_sigma.contiguous()
        P = arg.shape[0]
        rgb = torch.empty((P, 3), device=arg.device)
        sigma = torch.empty(P, device=arg.device)
        _lib.call("ia_candidate_gather_fwd", cand_rgb, cand_sigma, arg, P, float(fill), rgb, sigma)
        ctx.save_for_backward(arg)
        ctx.n_cand = cand_sigma.shape[0]
        return rgb, sigma

    @staticmethod
    def backward(ctx, d_rgb, d_sigma):
        (arg,) = ctx.saved_tensors
        c = lambda t: None if t is None else t.float().contiguous()
        d_rgb, d_sigma = c(d_rgb), c(d_sigma)
        d_cand_rgb = torch.zeros((ctx.n_cand, 3), device=arg.device)
        d_cand_sigma = torch.zeros(ctx.n_cand, device=arg.device)
        _lib.call("ia_candidate_gather_bwd", d_rgb, d_sigma, arg, arg.shape[0], d_cand_rgb, d_cand_sigma)
        return d_cand_rgb, d_cand_sigma, None, None


class _SmplTfsFn(torch.autograd.Function):
    """prepare_deformer's tfs / w2s / A (snarf_deformer.py:79-86) from the per-frame kernel `ia_smpl_tfs`, differentiable
    w.r.t. the pose and the translation through `ia_smpl_tfs_bwd` -- what the reference obtains by running lbs.py under
    autograd when the SMPL parameters are optimised (~370 tiny launches per step replaced by two)."""

    @staticmethod
    def forward(ctx, global_orient, body_pose, transl, deformer):
        fo = deformer._frame_out
        pose = torch.cat([global_orient.detach().reshape(1, 3), body_pose.detach().reshape(1, 69)], dim=1).float().contiguous()
        trc = transl.detach().reshape(3).float().contiguous()
        tfs, w2s, A = torch.empty_like(fo["tfs"]), torch.empty_like(fo["w2s"]), torch.empty_like(fo["A"])
        _lib.call("ia_smpl_tfs", deformer._joints_rest, deformer._parents32, pose, trc, deformer.tfs_inv_t, tfs, w2s, A)
        ctx.deformer = deformer
        ctx.shapes = (global_orient.shape, body_pose.shape, transl.shape)
        ctx.save_for_backward(pose, trc)
        ctx.mark_non_differentiable(w2s, A)
        return tfs, w2s, A

    @staticmethod
    def backward(ctx, d_tfs, _d_w2s, _d_A):
        pose, trc = ctx.saved_tensors
        d = ctx.deformer
        d_pose = torch.empty(72, device=pose.device)
        d_tr = torch.empty(3, device=pose.device)
        g = d_tfs.reshape(24, 4, 4).float().contiguous()
        _lib.call("ia_smpl_tfs_bwd", d._joints_rest, d._parents32, pose, trc, d.tfs_inv_t, g, d_pose, d_tr)
        s_go, s_bp, s_tr = ctx.shapes
        return d_pose[:3].reshape(s_go), d_pose[3:].reshape(s_bp), d_tr.reshape(s_tr), None


def _pose72(go, bp):
    """[1,72] axis-angle vector (global orientation, then the 23 body joints) for `ia_smpl_tfs`.  When the two inputs already
    are the adjacent parts of ONE 72-float record (a row of a pose table, pipeline.GraphedRenderer's static inputs) the
    record is used in place; otherwise they are concatenated (one launch)."""
    g, b = go.reshape(-1), bp.reshape(-1)
    if (g.dtype == torch.float32 and b.dtype == torch.float32 and g.numel() == 3 and b.numel() == 69 and g.is_contiguous()
            and b.is_contiguous() and b.data_ptr() == g.data_ptr() + 12
            and g.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()):
        return torch.as_strided(g, (1, 72), (72, 1))
    return torch.cat([go.reshape(1, 3), bp.reshape(1, 69)], dim=1).float().contiguous()


class SNARFDeformer():
    #: capacity (candidates) of one training-mode field call (`query_train_fused`, the probe of DensityGrid.update).
    #: None = points x init bones: every candidate fits by construction, nothing can be dropped (262 144 probe points x 13
    #: = 3.4 M rows, 1.6 GB of fp16 activations for the duration of the call every 20th step -- of 288 GB).  A number
    #: bounds the buffers instead; a call that needs more is then detected one call later (`train_overflow`) and the
    #: capacity doubles.
    train_cand_capacity = None

    def __init__(self, model_path, gender, opt, body_model=None) -> None:
        # body_model: optional pre-built SMPL (e.g. SMPL.from_dict(synthetic.make_body()))
        self.body_model = body_model if body_model is not None else SMPL(_abs_path(model_path), gender=gender)
        self.deformer = ForwardDeformer(opt)
        self.initialized = False
        self.opt = opt
        self.dtype = torch.float32
        self._ws = None
        self._cand_counts = DeferredCount()

    def clone_shared(self):
        """A second deformer for the same subject: body model, weight voxels and rest-pose constants shared by reference,
        per-frame state (tfs, w2s, voxel transforms) its own.  Requires an initialised deformer."""
        assert self.initialized, "clone_shared: initialise the deformer first"
        other = SNARFDeformer.__new__(SNARFDeformer)
        other.body_model, other.opt, other.dtype, other._ws = self.body_model, self.opt, self.dtype, None
        other._cand_counts = DeferredCount()
        other.deformer = self.deformer.clone_shared()
        other.initialized = True
        for k in ("tfs_inv_t", "vs_template", "bbox", "_joints_rest", "_parents32"):
            setattr(other, k, getattr(self, k))
        dev = self.tfs_inv_t.device
        other._frame_out = dict(tfs=torch.empty((1, 24, 4, 4), device=dev), w2s=torch.empty((1, 4, 4), device=dev),
                                A=torch.empty((1, 24, 4, 4), device=dev))
        return other

    # ------------------------------------------------------------------ init
    def initialize(self, betas, device):
        cano = _opt.get(self.opt, "cano_pose", "A_pose")
        if isinstance(cano, str):
            body_pose_t = get_predefined_rest_pose(cano, device=device)
        else:
            body_pose_t = torch.zeros((1, 69), device=device)
            for slot, val in zip((2, 5, 47, 50), cano):
                body_pose_t[:, slot] = val
        rest = self.body_model(betas=betas[:1], body_pose=body_pose_t)
        self.tfs_inv_t = torch.inverse(rest.A.float().detach()).contiguous()
        self.vs_template = rest.vertices
        self.deformer.device = device
        self.deformer.switch_to_explicit(resolution=_opt.get(self.opt, "resolution", 128),
                                         smpl_verts=rest.vertices.float().detach(),
                                         smpl_weights=self.body_model.lbs_weights.clone()[None].detach(),
                                         use_smpl=True)
        self.bbox = get_bbox_from_smpl(rest.vertices.detach())
        # constants of the per-frame kernel
        self._joints_rest = self.body_model.rest_joints(betas[:1].float()).contiguous()
        self._parents32 = self.body_model.parents.to(torch.int32).contiguous()
        self._frame_out = dict(tfs=torch.empty((1, 24, 4, 4), device=device), w2s=torch.empty((1, 4, 4), device=device),
                               A=torch.empty((1, 24, 4, 4), device=device))

    # ------------------------------------------------------------- per frame
    def prepare_deformer(self, smpl_params, want_bbox=True):
        """snarf_deformer.py:71-93.  betas are assumed constant per subject after
        the first call (the reference re-evaluates blend shapes every frame; with
        constant betas the rest joints are identical).
        want_bbox=False (training steps: nothing there reads the box of the deformed voxels, snarf_deformer.py:105-107 is the test
        grid's): the voxel pass writes the blended transforms only -- no voxel_d planes, no extrema, no reduce launch (20 -> 13 us
        and one launch less); `get_bbox_deformed()` computes them on demand."""
        device = smpl_params["betas"].device
        if self.body_model.v_template.device != device:
            self.body_model = self.body_model.to(device)
        if not self.initialized:
            self.initialize(smpl_params["betas"], device)
            self.initialized = True
        go, bp, tr = smpl_params["global_orient"], smpl_params["body_pose"], smpl_params["transl"]
        needs_grad = any(t.requires_grad for t in (go, bp, tr))
        _lib.require_cuda(go)  # no CPU route: the per-frame path is HIP kernels
        if needs_grad and FUSED_SMPL_BACKWARD and self.deformer.version == 1 and torch.is_grad_enabled():
            # SMPL-parameter refinement (config 4), version 1: the joint chain and its backward as two kernels.  (w2s / A carry no
            # gradient: with the implicit differentiation of version 1 nothing downstream of the rays is differentiated,
            # deformer_torch.py:50-67 -- the reference's gradient through transform_rays_w2s is identically zero there.)
            tfs, w2s, A = _SmplTfsFn.apply(go, bp, tr, self)
        elif needs_grad:
            # differentiable route (version 2, or the checker of the kernels above): torch ops under autograd; the voxel
            # precompute / search below still run as kernels, the gradient reaches tfs by implicit differentiation
            out = self.body_model(betas=smpl_params["betas"], body_pose=bp, global_orient=go, transl=tr,
                                  return_verts=False)
            s2w = out.A[:, 0].float()
            # snarf_deformer.py:84 `torch.inverse(s2w)`: the LU route of the library reads its status back to the host (one
            # synchronisation per step) and does not survive HIP-graph capture; s2w = [M t; 0 0 0 1], so the inverse is
            # [M^-1, -M^-1 t] with M^-1 from the cofactors -- plain differentiable tensor ops, equal to the LU inverse to rounding
            w2s = affine_inverse(s2w)
            tfs = (w2s[:, None] @ out.A.float() @ self.tfs_inv_t).type(self.dtype)
            A = out.A
        else:
            fo = self._frame_out
            pose = _pose72(go, bp)
            trc = tr.reshape(3).float().contiguous()
            _lib.call("ia_smpl_tfs", self._joints_rest, self._parents32, pose, trc, self.tfs_inv_t, fo["tfs"], fo["w2s"], fo["A"])
            tfs, w2s, A = fo["tfs"], fo["w2s"], fo["A"]
        self.deformer.precompute(tfs, want_voxel_d=want_bbox, want_bbox=want_bbox)
        self.w2s = w2s
        self.tfs = tfs
        self.A = A
        self.smpl_params = smpl_params
        self._vertices = None

    def release_graph(self):
        """Drop the autograd graph the per-frame attributes hold on to (tfs / w2s / A are non-leaf tensors when the SMPL
        parameters are optimised): called at the end of a training step.  A graph kept alive across steps keeps the
        AccumulateGrad nodes of the SMPL tables alive on the stream they were created on, which breaks a later HIP-graph
        capture of the step on another stream (and holds the step's activations)."""
        for name in ("tfs", "w2s", "A"):
            v = getattr(self, name, None)
            if torch.is_tensor(v) and v.requires_grad:
                setattr(self, name, v.detach())
        p = getattr(self, "smpl_params", None)
        if isinstance(p, dict):
            self.smpl_params = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in p.items()}
        self._vertices = None

    @property
    def vertices(self):
        """posed vertices in the SMPL-root frame (snarf_deformer.py:89); only the
        smpl_init occupancy bootstrap reads them, so they are computed lazily."""
        if self._vertices is None:
            p = self.smpl_params
            out = self.body_model(betas=p["betas"], body_pose=p["body_pose"], global_orient=p["global_orient"],
                                  transl=p["transl"])
            w2s = self.w2s
            self._vertices = (out.vertices @ w2s[:, :3, :3].permute(0, 2, 1)) + w2s[:, None, :3, 3]
        return self._vertices

    def transform_rays_w2s(self, rays):
        """snarf_deformer.py:95-103 (in place on the Rays object)."""
        o, d = rays.o, rays.d
        if o.is_cuda and o.dtype == torch.float32 and not (o.requires_grad or self.w2s.requires_grad):
            oc, dc = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
            R = oc.shape[0]
            o2, d2 = torch.empty_like(oc), torch.empty_like(dc)
            near, far = torch.empty(R, device=o.device), torch.empty(R, device=o.device)
            w2s = self.w2s.reshape(4, 4).float().contiguous()
            _lib.call("ia_transform_rays_w2s", oc, dc, w2s, R, o2, d2, near, far)
            rays.o, rays.d = o2.reshape(o.shape), d2.reshape(d.shape)
            rays.near, rays.far = near.reshape(o.shape[:-1]), far.reshape(o.shape[:-1])
            return
        w2s = self.w2s
        # (the differentiable branch -- w2s under optimisation: fit stage, version 2 -- as broadcast multiply + sum: a [n,3] x [3,3]
        # product is a library GEMM launch here, ~40 us forward and two more backward, and the only BLAS call of a fit step)
        R = w2s[:, :3, :3]
        shp_o, shp_d = o.shape, d.shape
        rays.o = ((o.reshape(1, -1, 1, 3) * R[:, None, :, :]).sum(-1) + w2s[:, None, :3, 3]).reshape(shp_o)
        rays.d = (d.reshape(1, -1, 1, 3) * R[:, None, :, :]).sum(-1).reshape(shp_d).to(d)
        dist = torch.norm(rays.o, dim=-1)
        rays.near, rays.far = dist - 1, dist + 1

    def get_bbox_deformed(self):
        """snarf_deformer.py:105-107; the min/max were reduced inside ia_precompute."""
        if self.deformer.bbox_deformed is None:      # the frame was prepared without it (a training step): one more voxel pass
            self.deformer.precompute(self.tfs.detach(), want_voxel_d=True, want_bbox=True)
        b = self.deformer.bbox_deformed
        return [b[:3], b[3:]]

    # ------------------------------------------------------------ field query
    def deform(self, pts, eval_mode):
        """snarf_deformer.py:109-125: canonical candidates [P,13,3] + validity [P,13]."""
        point_size = pts.shape[0]
        pts_cano, others = self.deformer.forward(pts.reshape(1, -1, 3), cond=None, tfs=self.tfs, eval_mode=eval_mode)
        k = len(self.deformer.init_bones)
        return pts_cano.reshape(point_size, k, 3), others["valid_ids"].reshape(point_size, k)

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self._ws

    def _is_native_field(self, model):
        from ..models.networks.ngp import NeRFNGPNet
        return isinstance(model, NeRFNGPNet)

    @torch.no_grad()
    def deform_test(self, pts, model):
        """snarf_deformer.py:127-141."""
        pts = pts.type(self.dtype)
        if self._is_native_field(model) and pts.is_cuda:
            return self.query_fused(pts, model)
        from .. import dense_routes
        return dense_routes.deform_query(self, pts, model, eval_mode=True)

    @torch.no_grad()
    def query_fused(self, pts, net, dmax=None, want_rgb=True):
        """deform_test as ONE C-ABI call: search + filter + compaction + field on the
        surviving candidates + max over candidates; no host synchronisation."""
        pts = pts.reshape(-1, 3).contiguous()
        P = pts.shape[0]
        k = len(self.deformer.init_bones)
        ws = self._workspace(_lib.call("ia_query_workspace_bytes", P, k), pts.device)
        rgb = torch.empty((P, 3), device=pts.device) if want_rgb else None
        sigma = torch.empty(P, device=pts.device)
        tfs = self.tfs.detach().float().contiguous()
        _lib.call("ia_deform_query", pts, P, None, self.deformer.voxel_J_cl, tfs, self.deformer._bones_c, k, self.deformer.grid_desc(),
                  net.field_desc(P * k), rgb, sigma, dmax, ws, ws.numel())
        return rgb, sigma

    @torch.no_grad()
    def surface_normals(self, rays_o, rays_d, depth, alpha, net, want_roots=False):
        """Normal map of the posed density field for a rendered frame ("surface normals"): rays [R,3] in
        the frame the marcher works in (after `transform_rays_w2s`), depth / alpha [R] as the renderer returned them ->
        [R,3] fp32 in the camera frame: unit length where the pixel has alpha >= 0.5 and a valid canonical root, zero
        elsewhere.  Seven launches behind the frame, no host synchronisation: surface points (compaction in ray order) ->
        candidate search -> sigma and d sigma / d x_c of every candidate in one kernel -> arg-max -> n = -M^{-T} g, rotated back
        with w2s.  The deformer must be prepared for the frame (`prepare_deformer`).
        want_roots: also return copies of what the map was made from -- dict(n [1] the number of surface points, ray [R] their
        rays, root [R,3] / grad [R,3] the winning canonical root and d sigma / d x_c of every point (zeros: no valid candidate)).
        Scratch: sized for the worst case, every pixel a surface point with all k candidates valid -- 28 R k + 44 R bytes, cached
        on the deformer (99 MB at 512^2 with 13 init bones); fixed pointers are what lets the pass be captured in a graph, and a
        smaller candidate capacity would drop candidates silently when a frame exceeds it."""
        _lib.require_cuda(rays_o, rays_d, depth, alpha)
        f32 = lambda t, *shape: t.detach().reshape(*shape).float().contiguous()
        o, d, dep, alp = f32(rays_o, -1, 3), f32(rays_d, -1, 3), f32(depth, -1), f32(alpha, -1)
        R = o.shape[0]
        dev = o.device
        k = len(self.deformer.init_bones)
        cap = R * k
        # one scratch block for everything between the frame and the map (sized on first use: a captured graph keeps its pointers)
        al = lambda n: (int(n) + 255) // 256 * 256
        ws_bytes = int(_lib.call("ia_surface_points_workspace_bytes", R))
        sizes = dict(ws=al(ws_bytes), n=256, pts=al(R * 12), ray=al(R * 4), off=al(R * 4), cnt=al(R), xc=al(cap * 12), sig=al(cap * 4),
                     grad=al(cap * 12), root=al(R * 12), g=al(R * 12))
        buf = _lib.scratch(self, "_ws_normals", sum(sizes.values()), dev)
        part, at = {}, 0
        for name, n in sizes.items():
            part[name] = buf[at:at + n]
            at += n
        i32 = lambda name, n: part[name].view(torch.int32)[:n]
        flt = lambda name, *shape: part[name].view(torch.float32)[:int(np.prod(shape))].view(*shape)
        counts = i32("n", 2)      # [points, candidates]
        pts, ray = flt("pts", R, 3), i32("ray", R)
        _lib.call("ia_surface_points", o, d, dep, alp, R, pts, ray, counts[0:1], part["ws"], ws_bytes)
        pt_off, pt_cnt, cand_xc = i32("off", R), part["cnt"][:R], flt("xc", cap, 3)
        tfs = self.tfs.detach().float().contiguous()
        _lib.call("ia_snarf_search_compact", pts, R, counts[0:1], self.deformer.voxel_J_cl, tfs, self.deformer._bones_c, k,
                  self.deformer.grid_desc(), 1e-5, 1e-1, cand_xc, cap, pt_off, pt_cnt, counts[1:2], 1)
        sig, grad = flt("sig", cap), flt("grad", cap, 3)
        _lib.call("ia_field_sigma_grad", cand_xc, cap, counts[1:2], net.field_desc(), sig, grad)
        root, g = flt("root", R, 3), flt("g", R, 3)
        _lib.call("ia_candidate_select", sig, cand_xc, grad, cap, pt_off, pt_cnt, R, counts[0:1], root, g, None)
        normals = torch.empty((R, 3), device=dev)
        w2s = self.w2s.detach().reshape(4, 4).float().contiguous()
        _lib.call("ia_normals_from_gradient", root, g, ray, R, counts[0:1], self.deformer.voxel_J_cl, self.deformer.grid_desc(), w2s, R,
                  normals)
        if want_roots:
            return normals, dict(n=counts[0:1].clone(), ray=ray.clone(), root=root.clone(), grad=g.clone())
        return normals

    def search_compact(self, pts, n_pts_dev=None, cap=None, want_J_inv=False, n_cand_out=None):
        """Search + filter + compaction (`ia_snarf_search_compact`): returns a dict with
        cand_xc [cap,3], pt_off [P], pt_cnt [P] and n_cand (device int32[1]); with `want_J_inv`
        (`ia_snarf_search_compact_jinv`) also cand_Jinv [cap,3,3], the Broyden J_inv of every
        surviving root -- the input of the implicit differentiation when tfs carries a gradient."""
        pts = pts.detach().reshape(-1, 3).float().contiguous()
        P = pts.shape[0]
        k = len(self.deformer.init_bones)
        dev = pts.device
        cap = P * k if cap is None else min(int(cap), P * k)
        out = dict(cand_xc=torch.empty((cap, 3), device=dev), pt_off=torch.empty(P, dtype=torch.int32, device=dev),
                   pt_cnt=torch.empty(P, dtype=torch.uint8, device=dev),
                   # (n_cand_out: a ZERO-FILLED device int32[1] of the caller's, e.g. half of its counter pair)
                   n_cand=n_cand_out if n_cand_out is not None else torch.zeros(1, dtype=torch.int32, device=dev),
                   pts=pts, n_pts_dev=n_pts_dev)
        tfs = self.tfs.detach().float().contiguous()
        head = (pts, P, n_pts_dev, self.deformer.voxel_J_cl, tfs, self.deformer._bones_c, k, self.deformer.grid_desc(), 1e-5, 1e-1,
                out["cand_xc"])
        tail = (cap, out["pt_off"], out["pt_cnt"], out["n_cand"], 0)
        if want_J_inv:
            out["cand_Jinv"] = torch.empty((cap, 3, 3), device=dev)
            # J_inv of the valid solves before compaction (P x 13 x 36 B)
            ws = _lib.scratch(self, "_ws_jinv", int(_lib.call("ia_snarf_search_jinv_workspace_bytes", P, k)), dev)
            _lib.call("ia_snarf_search_compact_jinv", *head, out["cand_Jinv"], *tail, ws, ws.numel())
        else:
            _lib.call("ia_snarf_search_compact", *head, *tail)
        return out

    def candidates_with_grad(self, sc):
        """The compact candidate positions of `search_compact`, carrying -- when the bone transforms are under
        optimisation (`tfs.requires_grad`: SMPL refinement, DNeRF.py:113-128) -- the gradient of the implicit
        differentiation of deformer_torch.py:50-67 (`ia_snarf_implicit_bwd_compact`); plain tensor otherwise."""
        if self.deformer.version != 1:
            # `version: 2` (deformer_torch.py:68-75): in training every root is REPLACED by its closed-form inverse skinning
            # x_c = R^T (x_d - t) -- another value, not only another gradient -- whether or not tfs is under optimisation
            from .fast_snarf.forward_deformer import _InverseSkinningFn
            P = sc["pts"].shape[0]
            cand_pt = torch.empty(sc["cand_xc"].shape[0], dtype=torch.int32, device=sc["pts"].device)
            _lib.call("ia_expand_candidate_points", sc["pt_off"], sc["pt_cnt"], P, sc["n_pts_dev"], cand_pt, cand_pt.numel())
            return _InverseSkinningFn.apply(self.tfs, sc["cand_xc"], sc["pts"], None, cand_pt, sc["n_cand"], self.deformer)
        if "cand_Jinv" not in sc:
            return sc["cand_xc"]
        from .fast_snarf.forward_deformer import _ImplicitDiffCompactFn
        return _ImplicitDiffCompactFn.apply(self.tfs, sc["cand_xc"], sc["cand_Jinv"], sc["n_cand"], self.deformer)

    def fused_train_route(self):
        """True when the fused training route covers the current state: always for version 1 (implicit differentiation of the
        roots on the compact candidate list) and for version 2 (closed-form inverse skinning, deformer_torch.py:68-75) as long
        as the SMPL parameters are not under optimisation -- with them, version 2's x_c = R^T (x_d - t) also sends a gradient
        through the sample points x_d into the ray frame w2s (snarf_deformer.py:95-103), which only the dense route's autograd
        over the rays carries (its inverse skinning is the same kernel pair, in the dense layout)."""
        if getattr(self, "force_dense_train", False):   # tests: the route that keeps the reference's dense structure
            return False
        return self.deformer.version == 1 or not self.tfs.requires_grad

    #: number of `query_train_fused` calls whose candidates exceeded the capacity (they were dropped in compaction order --
    #: the densities had holes); the capacity doubles after every such call (deferred check, `_cand_count_check`)
    train_overflow = 0

    def _cand_count_check(self):
        """Deferred overflow check of the previous `query_train_fused` call (no stall: that call has long finished)."""
        self._cand_counts.check(self)

    @property
    def last_cand_count(self):
        """candidates of the last `query_train_fused` call looked at, None before the first"""
        return self._cand_counts.last[0] if self._cand_counts.last else None

    def query_train_fused(self, pts, net):
        """deform_train (snarf_deformer.py:143-159) without the dense [P,13,*] temporaries:
        compacted candidates -> field under autograd -> arg-max gather (`ia_candidate_gather_*`, whose
        backward is a unique scatter: no index sort).  No host synchronisation: the field runs on a
        capacity-sized candidate buffer with the device-side count; the count is inspected one call later
        (`train_overflow`, growing `train_cand_capacity`)."""
        P = pts.shape[0]
        k = len(self.deformer.init_bones)
        self._cand_count_check()
        cap = P * k if self.train_cand_capacity is None else min(P * k, self.train_cand_capacity)
        want_J_inv = self.tfs.requires_grad and torch.is_grad_enabled() and self.deformer.version == 1
        with torch.no_grad():
            sc = self.search_compact(pts, cap=cap, want_J_inv=want_J_inv)
        rgb_c, sig_c = field_autograd(net, self.candidates_with_grad(sc), n_dev=sc["n_cand"])
        self._cand_counts.post(sc["n_cand"], cap)
        arg = torch.empty(P, dtype=torch.int32, device=pts.device)
        sig_d = sig_c.detach().float().contiguous()
        _lib.call("ia_candidate_argmax", sig_d, cap, sc["pt_off"], sc["pt_cnt"], P, k, arg)
        return _CandidateGatherFn.apply(rgb_c.float(), sig_c.float(), arg, -1e5)

    def deform_train(self, pts, model):
        """snarf_deformer.py:143-159."""
        if self._is_native_field(model) and pts.is_cuda and self.fused_train_route():
            return self.query_train_fused(pts.type(self.dtype), model)
        from .. import dense_routes
        return dense_routes.deform_query(self, pts.type(self.dtype), model, eval_mode=False)

    def __call__(self, pts, model, eval_mode=True):
        if eval_mode:
            return self.deform_test(pts, model)
        return self.deform_train(pts, model)
