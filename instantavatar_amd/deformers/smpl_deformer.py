"""SMPLDeformer plugin (drop-in for instant_avatar/deformers/smpl_deformer.py:20-137), the second
deformer behind the `confs/deformer` surface (`confs/deformer/smpl.yaml`): a point is moved to
canonical space by the inverse transform of its NEAREST posed SMPL vertex if that vertex is closer
than `threshold`.

    SMPLDeformer(model_path, gender, threshold=0.05, k=1)
    .initialize(betas, device)   .prepare_deformer(smpl_params)   .transform_rays_w2s(rays)
    .get_bbox_deformed()         .deform(pts) -> (pts_cano, valid)
    .deform_test / .deform_train / __call__(pts, model, eval_mode)
    attributes: bbox, vertices, w2s, T_inv, initialized, body_model

The nearest-vertex search (pytorch3d knn_points in the reference) and the per-point transform are
the HIP kernel `ia_smpl_nn_deform`; `deformer(pts, net)` is the fused `ia_smpl_deform_query`
(search + compaction + field + scatter, no host synchronisation) when `net` is an
instantavatar_amd NeRFNGPNet, and the reference's masked structure for any other callable.
Only k = 1 is supported (the reference squeezes the neighbour axis: "we use the nearest neighbor
only", smpl_deformer.py:98-100).
"""
import torch

from .. import _lib
from .smplx import SMPL
from .snarf_deformer import _abs_path, get_bbox_from_smpl


#: the body model of `prepare_deformer` as the fused kernels `ia_smpl_lbs_fwd / _bwd` (csrc/ia_smpl_lbs.hip); False = the
#: lbs.py-style torch ops under autograd (the checker of the kernels: tests/test_gpu_smpl_deformer.py)
FUSED_LBS = True


class _SmplLbsFn(torch.autograd.Function):
    """`SMPLDeformer.initialize` + `prepare_deformer` (smpl_deformer.py:32-77) as two launches, differentiable w.r.t. betas, pose and
    translation through four more -- what the reference obtains by running smplx's SMPL.forward twice under autograd (fit stage:
    DNeRF.py:113-128).  Outputs: T_inv [1,V,4,4], vertices [1,V,3] (SMPL-root frame), w2s [1,4,4], template vertices [1,V,3]."""

    @staticmethod
    def forward(ctx, betas, body_pose, global_orient, transl, deformer):
        smpl = deformer.body_model
        body, keep = smpl.lbs_constants()
        dev = keep["v_template"].device
        V = body.n_verts
        b = betas.detach().reshape(-1)[:10].float().contiguous()
        pose = torch.cat([global_orient.detach().reshape(3), body_pose.detach().reshape(69)]).float().contiguous()
        tr = transl.detach().reshape(3).float().contiguous() if transl is not None else None
        pose_t, po_t = deformer._template_constants(dev)
        ws = _lib.scratch(deformer, "_lbs_ws", _lib.call("ia_smpl_lbs_workspace_bytes", V), dev)
        T_inv, verts = torch.empty((1, V, 4, 4), device=dev), torch.empty((1, V, 3), device=dev)
        verts_t, w2s = torch.empty((1, V, 3), device=dev), torch.empty((1, 4, 4), device=dev)
        _lib.call("ia_smpl_lbs_fwd", body, b, pose, tr, pose_t, po_t, T_inv, verts, verts_t, w2s, ws, ws.numel())
        ctx.deformer = deformer
        ctx.shapes = (betas.shape, body_pose.shape, global_orient.shape, None if transl is None else transl.shape)
        ctx.save_for_backward(b, pose, tr if tr is not None else torch.empty(0, device=dev))
        ctx.has_tr = tr is not None
        ctx.mark_non_differentiable(verts, verts_t)     # nearest-vertex search and bounding boxes only (smpl_deformer.py:45-48,90)
        ctx.set_materialize_grads(False)
        return T_inv, verts, w2s, verts_t

    @staticmethod
    def backward(ctx, d_T_inv, _d_verts, d_w2s, _d_verts_t):
        b, pose, tr = ctx.saved_tensors
        d = ctx.deformer
        body, keep = d.body_model.lbs_constants()
        dev = b.device
        V = body.n_verts
        s_b, s_bp, s_go, s_tr = ctx.shapes
        if d_T_inv is None and d_w2s is None:
            return None, None, None, None, None
        g = d_T_inv.reshape(V, 4, 4).float().contiguous() if d_T_inv is not None else torch.zeros((V, 4, 4), device=dev)
        gw = d_w2s.reshape(4, 4).float().contiguous() if d_w2s is not None else None
        pose_t, po_t = d._template_constants(dev)
        ws = _lib.scratch(d, "_lbs_ws", _lib.call("ia_smpl_lbs_workspace_bytes", V), dev)
        d_b, d_pose, d_tr = torch.empty(10, device=dev), torch.empty(72, device=dev), torch.empty(3, device=dev)
        _lib.call("ia_smpl_lbs_bwd", body, b, pose, tr if ctx.has_tr else None, pose_t, po_t, g, gw, d_b, d_pose, d_tr, ws, ws.numel())
        gb = torch.zeros(s_b, device=dev)
        gb.reshape(-1)[:10] = d_b      # (betas [1,10]: the row in use)
        return gb, d_pose[3:].reshape(s_bp), d_pose[:3].reshape(s_go), (d_tr.reshape(s_tr) if ctx.has_tr else None), None


class SMPLDeformer():
    def __init__(self, model_path, gender, threshold=0.05, k=1, body_model=None) -> None:
        # body_model: optional pre-built SMPL (e.g. SMPL.from_dict(synthetic.make_body()))
        self.body_model = body_model if body_model is not None else SMPL(_abs_path(model_path), gender=gender)
        if k != 1:
            raise NotImplementedError("SMPLDeformer: only k = 1 (nearest vertex) is implemented, as used by the reference")
        self.k = k
        self.threshold = threshold
        self.strategy = "nearest_neighbor"
        self.initialized = False
        self._ws = None

    def initialize(self, betas, device):
        """smpl_deformer.py:32-45: template pose (legs apart), its per-vertex transforms and offsets."""
        batch_size = betas.shape[0]
        body_pose_t = torch.zeros((batch_size, 69), device=device)
        body_pose_t[:, 2] = torch.pi / 6
        body_pose_t[:, 5] = -torch.pi / 6
        out = self.body_model(betas=betas, body_pose=body_pose_t)
        self.bbox = get_bbox_from_smpl(out.vertices[0:1].detach())
        self.T_template = out.T
        self.vs_template = out.vertices
        self.pose_offset_t = out.pose_offsets
        self.shape_offset_t = out.shape_offsets
        self._init_betas = betas.detach()

    def _template_constants(self, device):
        """(template pose [72], its pose-corrective offsets po_t [V,3]) on `device`: the template pose of :33-35 is a constant, so
        its pose blend (pose_feature_t x posedirs) is one per subject"""
        c = getattr(self, "_tmpl_const", None)
        if c is None or c[0].device != torch.device(device):
            from .smplx import batch_rodrigues
            with torch.no_grad():
                pose_t = torch.zeros(72, device=device)
                pose_t[3 + 2], pose_t[3 + 5] = torch.pi / 6, -torch.pi / 6
                rot = batch_rodrigues(pose_t.view(-1, 3))
                pf = (rot[1:] - torch.eye(3, device=device)).reshape(1, -1)
                po_t = torch.matmul(pf, self.body_model.posedirs.to(device)).view(-1, 3).float().contiguous()      # lbs.py:216-219
            c = self._tmpl_const = (pose_t.contiguous(), po_t)
        return c

    def _fused_lbs_ok(self, betas):
        """the fused kernels evaluate template and posed body with the SAME betas -- what the reference does (it re-initialises every
        frame, smpl_deformer.py:57-61).  A caller who froze a template (`initialized = True`) with other betas gets the torch route."""
        if not (FUSED_LBS and betas.is_cuda):
            return False
        if not self.initialized:
            return True
        ib = getattr(self, "_init_betas", None)
        if ib is None:
            return False
        key = (betas.data_ptr(), betas._version, ib.data_ptr())
        if getattr(self, "_betas_ok_key", None) != key:
            self._betas_ok = bool(ib.shape == betas.shape and torch.equal(ib, betas.detach()))   # (host read: once per betas tensor)
            self._betas_ok_key = key
        return self._betas_ok

    def get_bbox_deformed(self):
        return get_bbox_from_smpl(self.vertices[0:1].detach())

    #: tests: keep the reference's dense structure for the training render (dense_routes.render_train + deform_train)
    force_dense_train = False

    def fused_train_route(self):
        """the training render over compact samples (Raymarcher.render_train_fused): one frame per step, on the GPU"""
        return not self.force_dense_train and torch.is_tensor(getattr(self, "vertices", None)) and self.vertices.is_cuda and self.vertices.shape[0] == 1

    def prepare_deformer(self, smpl_params):
        """smpl_deformer.py:50-77"""
        device = smpl_params["betas"].device
        if next(self.body_model.buffers()).device != device:
            self.body_model = self.body_model.to(device)
        if self._fused_lbs_ok(smpl_params["betas"]):
            _lib.require_cuda(smpl_params["body_pose"])
            T_inv, verts, w2s, verts_t = _SmplLbsFn.apply(smpl_params["betas"], smpl_params["body_pose"], smpl_params["global_orient"],
                                                          smpl_params["transl"], self)
            if not self.initialized:     # `initialize` (the reference re-runs it every frame: betas may change)
                self.bbox = get_bbox_from_smpl(verts_t.detach())
            self.T_inv, self.vertices, self.w2s = T_inv, verts, w2s
            self._build_nn_grid()
            return
        if not self.initialized:
            self.initialize(smpl_params["betas"], device)  # the reference re-initialises every frame (betas may change)
        out = self.body_model(betas=smpl_params["betas"], body_pose=smpl_params["body_pose"],
                              global_orient=smpl_params["global_orient"], transl=smpl_params["transl"], small_ops=True)
        s2w = out.A[:, 0]
        # (smpl_deformer.py:69-70 uses torch.inverse twice: the LU route reads its status back to the host and, for the 6 890
        # per-vertex transforms, is a chain of library kernels; both matrices are affine -- closed form, differentiable)
        from .snarf_deformer import affine_inverse
        from .smplx import small_matmul
        w2s = affine_inverse(s2w)
        T_inv = small_matmul(affine_inverse(out.T.float()), s2w[:, None])
        T_inv[..., :3, 3] += self.pose_offset_t - out.pose_offsets   # remove & re-apply the blend shapes
        T_inv[..., :3, 3] += self.shape_offset_t - out.shape_offsets
        self.T_inv = small_matmul(self.T_template, T_inv).float().contiguous()
        self.vertices = ((out.vertices @ w2s[:, :3, :3].permute(0, 2, 1)) + w2s[:, None, :3, 3]).float().contiguous()
        self.w2s = w2s
        self._build_nn_grid()

    #: the fused queries look for the nearest vertex in a per-frame vertex grid (`ia_smpl_nn_grid_build`) instead of testing
    #: all vertices; False = brute force (the checker: tests/test_gpu_smpl_deformer.py)
    use_nn_grid = True

    def _build_nn_grid(self):
        """bin this frame's posed vertices (four small launches, no host read); the buffer is per deformer and reused"""
        self._nn_grid_ok = False
        if not (self.use_nn_grid and torch.is_tensor(self.vertices) and self.vertices.is_cuda and self.vertices.shape[0] == 1):
            return
        V = self.vertices.shape[1]
        buf = _lib.scratch(self, "_nn_grid_buf", _lib.call("ia_smpl_nn_grid_bytes", V), self.vertices.device)
        v = self.vertices.detach()
        _lib.call("ia_smpl_nn_grid_build", v, V, float(self.threshold), buf, buf.numel())
        self._nn_grid_ok = True
        self._nn_grid_key = (self.vertices.data_ptr(), self.vertices._version, float(self.threshold))

    def nn_grid_ptr(self):
        """device pointer of the vertex grid of the CURRENT vertices, or None (brute force)"""
        if not (getattr(self, "_nn_grid_ok", False) and self.use_nn_grid):
            return None
        v = self.vertices     # (somebody replaced or rewrote the vertices, or changed the threshold, after prepare_deformer: brute force)
        if self._nn_grid_key != (v.data_ptr(), v._version, float(self.threshold)):
            return None
        return self._nn_grid_buf.data_ptr()     # (a raw address for `call`: the buffer lives on the deformer)

    def release_graph(self):
        """drop the autograd graph held by the per-frame attributes (see SNARFDeformer.release_graph)"""
        # (the template quantities of `initialize` carry the betas' graph on the torch route: the reference recomputes them every frame)
        for name in ("T_inv", "vertices", "w2s", "T_template", "vs_template", "pose_offset_t", "shape_offset_t"):
            v = getattr(self, name, None)
            if torch.is_tensor(v) and v.requires_grad:
                setattr(self, name, v.detach())

    def transform_rays_w2s(self, rays):
        """smpl_deformer.py:79-86 (same as SNARFDeformer.transform_rays_w2s): fused kernel."""
        from .snarf_deformer import SNARFDeformer
        return SNARFDeformer.transform_rays_w2s(self, rays)

    # ------------------------------------------------------------------ queries
    def _check_batch(self):
        if self.vertices.shape[0] != 1:
            raise NotImplementedError("SMPLDeformer: batch size 1 (one frame per step, peoplesnapshot.py:171)")

    def deform(self, pts):
        """smpl_deformer.py:88-110 -> (pts_cano [P,3], valid [P] bool)"""
        self._check_batch()
        _lib.require_cuda(pts)
        x = pts.detach().reshape(-1, 3).float().contiguous()
        P = x.shape[0]
        cano = torch.empty((P, 3), device=x.device)
        valid = torch.empty(P, dtype=torch.uint8, device=x.device)
        need_grad = torch.is_grad_enabled() and (self.T_inv.requires_grad or pts.requires_grad)
        idx = torch.empty(P, dtype=torch.int32, device=x.device) if need_grad else None
        if P:
            _lib.call("ia_smpl_nn_deform", x, P, None, self.vertices.detach(), self.T_inv.detach(), self.vertices.shape[1],
                      float(self.threshold), cano, valid, idx)
        if need_grad and P:
            # SMPL refinement with this deformer (SNARF_NGP_refine + deformer=smpl): the reference's pts_cano
            # (smpl_deformer.py:100-107) is differentiable w.r.t. the per-vertex transforms; the nearest-vertex
            # index comes from the kernel, the affine map is re-applied in torch so that autograd reaches T_inv
            # (index_select: its backward is an index_add, not the sort-based indexing backward of T_inv[0][idx] -- 250 us a call;
            # the 3 x 3 products as multiply + sum: a batched GEMM over ~10^5 tiny matrices is 260 us forward and twice that back)
            T = torch.index_select(self.T_inv[0], 0, idx.long())
            xh = pts.reshape(-1, 3).float()
            cano = (T[:, :3, :3] * xh[:, None, :]).sum(-1) + T[:, :3, 3]
        return cano, valid.bool()

    def _workspace(self, nbytes, device):
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != device:
            self._ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self._ws

    def _query_fused(self, pts, net, fill, nan_to_num):
        self._check_batch()
        x = pts.detach().reshape(-1, 3).float().contiguous()
        P = x.shape[0]
        rgb = torch.zeros((P, 3), device=x.device)
        sigma = torch.full((P,), float(fill), device=x.device)
        if P == 0:
            return rgb, sigma
        ws = self._workspace(_lib.call("ia_smpl_query_workspace_bytes", P), x.device)
        _lib.call("ia_smpl_deform_query", x, P, None, self.vertices, self.T_inv, self.vertices.shape[1], float(self.threshold),
                  net.field_desc(P), float(fill), int(nan_to_num), rgb, sigma, ws, ws.numel(), self.nn_grid_ptr())
        return rgb, sigma

    @staticmethod
    def _native(model):
        from ..models.networks.ngp import NeRFNGPNet
        return isinstance(model, NeRFNGPNet)

    def surface_normals(self, rays_o, rays_d, depth, alpha, net):
        """Normal maps need the canonical roots and the blended transforms of the SNARF deformer; not built for this one."""
        raise NotImplementedError("surface normals are implemented for the SNARF deformer (deformers.snarf_deformer.SNARFDeformer) "
                                  "only; SMPLDeformer has no normal pass")

    def deform_test(self, pts, model):
        """smpl_deformer.py:122-131: invalid points -> rgb 0, sigma 0"""
        if self._native(model) and not torch.is_grad_enabled():
            return self._query_fused(pts, model, 0.0, 0)
        from .. import dense_routes
        return dense_routes.deform_query_single(self, pts, model, eval_mode=True)

    def deform_train(self, pts, model):
        """smpl_deformer.py:112-120: invalid or non-finite -> rgb 0, sigma -1e5"""
        from .. import dense_routes
        return dense_routes.deform_query_single(self, pts, model, eval_mode=False)

    def __call__(self, pts, model, eval_mode=True):
        return self.deform_test(pts, model) if eval_mode else self.deform_train(pts, model)
