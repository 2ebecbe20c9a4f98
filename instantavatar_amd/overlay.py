"""Looking at a custom sequence on the GPU (csrc/ia_overlay.hip, include/instantavatar_hip_overlay.h; definitions in DESIGN.md section
4, "sequence inspection"): overlay the posed SMPL body, the mask outline and the 2D skeleton on the frames, and measure per frame how
well the poses fit -- silhouette IoU against the masks and pixel error against the 2D keypoints.  What scripts/visualize-SMPL.py of the
reference shows through aitviewer and an OpenGL context; `drivers/inspect_sequence.py` is the command line around it.

    blend(images, layer, opacity=128)                  images [n,H,W,3] u8, layer [n,H,W,4] u8, opacity in 0 .. 256 -> [n,H,W,3] u8
    outline(images, masks, thickness=2, rgb=...)       in place: the inner border of masks > 0, `thickness` pixels wide
    face_shade(face_id, verts, faces, w2c, tint)       [H,W] int32 face ids -> a flat-shaded layer [H,W,4] u8
    draw_skeleton(images, points, segments, ...)       in place: capsules and discs with exact integer geometry in quarter pixels
    mask_stats(a, b)                                   -> MaskStats(inter, union, a_area, b_area, iou), one row per frame

    SequenceInspector(body_model, K, extrinsic, H, W, keypoints=None, masks=None)
        .report(betas, pose, transl)                   -> per-frame device tensors (iou, kp_err_px, ...)
        .overlay(images, frame_indices, betas, pose, transl) -> the frames with body, outline, skeleton and model points drawn in

Everything stays on the device.  There is no CPU route."""
import collections
import colorsys

import numpy as np
import torch

from . import _lib
from .keypoints import MIDHIP, SMPL_KP_VERTEX, KeypointRefiner
from .masks import _owner, _side_stream

#: the 24 limb pairs OpenPose publishes for BODY_25 (its pose-render pairs), as indices into the 25 points
BODY25_SEGMENTS = ((1, 8), (1, 2), (1, 5), (2, 3), (3, 4), (5, 6), (6, 7), (8, 9), (9, 10), (10, 11), (8, 12), (12, 13), (13, 14), (1, 0),
                   (0, 15), (15, 17), (0, 16), (16, 18), (14, 19), (19, 20), (14, 21), (11, 22), (22, 23), (11, 24))
#: one colour per limb: this project's own table, a hue ramp by limb index at saturation 0.85 and full value
LIMB_COLOURS = tuple(tuple(int(round(255 * c)) for c in colorsys.hsv_to_rgb(i / 24.0, 0.85, 1.0)) for i in range(24))
BODY_TINT = (90, 170, 255)         # the body layer
OUTLINE_COLOUR = (255, 255, 255)   # the mask outline
DETECTION_COLOUR = (255, 255, 255)  # the detected points: joints as wide as the limbs between them
HALF_WIDTH_Q, DETECTION_RADIUS_Q, MODEL_RADIUS_Q = 6, 6, 8      # of `SequenceInspector.overlay`, in quarter pixels
MODEL_POINT_COLOUR = (255, 255, 0)  # the projected model points (fully saturated: no colour of the ramp above)

#: inter, union, a_area, b_area: int32 [n] pixel counts of a > 0 & b > 0, a > 0 | b > 0, a > 0, b > 0; iou: float32 [n] = inter / union, and 0
#: where union == 0 (two empty masks are NOT called a perfect fit: an empty frame should show up among the worst)
MaskStats = collections.namedtuple("MaskStats", "inter union a_area b_area iou")


def _u8(t, what, shape_tail=None):
    if not torch.is_tensor(t):
        raise TypeError("%s is a uint8 tensor on the GPU, got %s" % (what, type(t).__name__))
    _lib.require_cuda(t)
    if t.dtype not in (torch.uint8, torch.bool):
        raise _lib.IAError("%s is uint8, got %s" % (what, t.dtype))
    if shape_tail is not None and (t.dim() < 1 or t.shape[-1] != shape_tail):
        raise _lib.IAError("%s has %d channels last, got shape %s" % (what, shape_tail, tuple(t.shape)))
    return t


def _rgb(c, what):
    c = tuple(int(v) for v in c)
    if len(c) != 3:
        raise ValueError("%s is (r, g, b), got %r" % (what, c))
    return c


@torch.no_grad()
def blend(images, layer, opacity=128, out=None):
    """images uint8 [n,H,W,3] (or [H,W,3]), layer uint8 [n,H,W,4] (r, g, b, alpha) -> the images with the layer blended in at `opacity`
    (an integer in 0 .. 256; 256 with alpha 255 is the layer itself).  out: None (a new tensor) or a contiguous tensor of the images'
    shape, which may be `images` itself."""
    _u8(images, "blend: images", 3)
    _u8(layer, "blend: layer", 4)
    if images.dim() not in (3, 4) or tuple(images.shape[:-1]) != tuple(layer.shape[:-1]):
        raise _lib.IAError("blend: images [n,H,W,3] and layer [n,H,W,4], got %s and %s" % (tuple(images.shape), tuple(layer.shape)))
    if out is None:
        images = images.contiguous()
        out = torch.empty_like(images)
    elif out.shape != images.shape or out.dtype != torch.uint8 or not out.is_contiguous() or not images.is_contiguous():
        raise _lib.IAError("blend: out is a contiguous uint8 tensor of the shape of (contiguous) images")
    layer = layer.contiguous()
    H, W = images.shape[-3:-1]
    n = 1 if images.dim() == 3 else images.shape[0]
    with torch.cuda.device(images.device), _side_stream(images.device):
        _lib.call("ia_overlay_blend", images, layer, n, H, W, int(opacity), out)
    return out


@torch.no_grad()
def outline(images, masks, thickness=2, rgb=OUTLINE_COLOUR):
    """In place on images uint8 [n,H,W,3] (or [H,W,3]), contiguous: every pixel with masks > 0 that has a pixel of the image with masks == 0
    within Chebyshev distance `thickness` (1 .. 8) takes `rgb`.  The image border is not an edge.  -> images"""
    _u8(images, "outline: images", 3)
    _u8(masks, "outline: masks")
    if images.dim() not in (3, 4) or tuple(images.shape[:-1]) != tuple(masks.shape) or not images.is_contiguous():
        raise _lib.IAError("outline: contiguous images [n,H,W,3] and masks [n,H,W], got %s and %s" % (tuple(images.shape), tuple(masks.shape)))
    r, g, b = _rgb(rgb, "outline: rgb")
    H, W = masks.shape[-2:]
    n = 1 if masks.dim() == 2 else masks.shape[0]
    with torch.cuda.device(images.device), _side_stream(images.device):
        _lib.call("ia_overlay_outline", masks.contiguous(), n, H, W, int(thickness), r, g, b, images)
    return images


@torch.no_grad()
def face_shade(face_id, verts, faces, w2c, tint=BODY_TINT):
    """face_id int32 [H,W] (`raster.rasterize(...).face_id`; -1 = empty), verts [nv,3] fp32, faces [nf,3] int32, w2c [4,4] -> layer uint8
    [H,W,4]: tint * (0.25 + 0.75 |n_z|) with n the face's unit normal in the camera frame and alpha 255 on covered pixels, zeros elsewhere."""
    _lib.require_cuda(face_id, verts, faces, w2c)
    if face_id.dtype != torch.int32 or face_id.dim() != 2:
        raise _lib.IAError("face_shade: face_id is int32 [H,W], got %s %s" % (face_id.dtype, tuple(face_id.shape)))
    verts = verts.detach().reshape(-1, 3).float().contiguous()
    faces = faces.detach().reshape(-1, 3).to(torch.int32).contiguous()
    w2c = w2c.detach().reshape(4, 4).float().contiguous()
    r, g, b = _rgb(tint, "face_shade: tint")
    H, W = face_id.shape
    layer = torch.empty((H, W, 4), dtype=torch.uint8, device=face_id.device)
    with torch.cuda.device(face_id.device), _side_stream(face_id.device):
        _lib.call("ia_overlay_face_shade", face_id.contiguous(), H, W, verts, verts.shape[0], faces, faces.shape[0], w2c, r, g, b, layer)
    return layer


@torch.no_grad()
def draw_skeleton(images, points, segments=BODY25_SEGMENTS, segment_rgb=LIMB_COLOURS, point_rgb=MODEL_POINT_COLOUR, threshold=0.2,
                  half_width_q=HALF_WIDTH_Q, radius_q=MODEL_RADIUS_Q):
    """In place on images uint8 [n,H,W,3] (or [H,W,3]), contiguous.  points [n,K,3] fp32 (x, y, confidence), K <= 64; segments: S <= 64
    index pairs (a sequence or an int32 tensor [S,2]; S = 0: discs only) and as many colours; half_width_q (1 .. 64) and radius_q
    (0 .. 128) in quarter pixels.  A point is drawn when its confidence is ABOVE the threshold, a segment when both of its ends are;
    discs lie over segments, a higher segment index over a lower.  -> images"""
    _u8(images, "draw_skeleton: images", 3)
    _lib.require_cuda(points)
    if images.dim() not in (3, 4) or not images.is_contiguous():
        raise _lib.IAError("draw_skeleton: contiguous images [n,H,W,3], got %s" % (tuple(images.shape),))
    H, W = images.shape[-3:-1]
    n = 1 if images.dim() == 3 else images.shape[0]
    points = points.detach().float().reshape(n, -1, 3).contiguous()
    dev = images.device
    if torch.is_tensor(segments):
        seg = segments.detach().to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    else:
        seg = torch.as_tensor(np.asarray(segments, np.int64).reshape(-1, 2).astype(np.int32), device=dev)
    S = int(seg.shape[0])
    if torch.is_tensor(segment_rgb):
        col = segment_rgb.detach().to(device=dev, dtype=torch.uint8).reshape(-1, 3)[:S].contiguous()
    else:
        col = torch.as_tensor(np.asarray(segment_rgb, np.int64).reshape(-1, 3)[:S].astype(np.uint8), device=dev)
    if col.shape[0] != S:
        raise _lib.IAError("draw_skeleton: %d segments but %d colours" % (S, col.shape[0]))
    r, g, b = _rgb(point_rgb, "draw_skeleton: point_rgb")
    with torch.cuda.device(dev), _side_stream(dev):
        _lib.call("ia_overlay_skeleton", points, n, points.shape[1], seg if S else None, col if S else None, S, r, g, b, float(threshold),
                  int(half_width_q), int(radius_q), H, W, images)
    return images


@torch.no_grad()
def mask_stats(a, b):
    """a, b: uint8 or bool [n,H,W] (or [H,W]) on the GPU -> MaskStats of the pixels that are non-zero.  iou = inter / union, and 0 where
    the union is empty."""
    _u8(a, "mask_stats: a")
    _u8(b, "mask_stats: b")
    if a.shape != b.shape or a.dim() not in (2, 3):
        raise _lib.IAError("mask_stats: two masks [n,H,W] of one shape, got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    single = a.dim() == 2
    a, b = a.contiguous(), b.contiguous()
    H, W = a.shape[-2:]
    n = 1 if single else a.shape[0]
    dev = a.device
    out = torch.empty((n, 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev), _side_stream(dev):
        nb = int(_lib.call("ia_overlay_stats_workspace_bytes", n, H, W))
        if nb == 0:
            raise _lib.IAError("mask_stats: %d frames of %d x %d: outside 1 <= n <= 65535, H, W >= 1, H * W < 2^31" % (n, H, W))
        ws = _lib.scratch(_owner(dev), "_overlay_ws", nb, dev)
        _lib.call("ia_overlay_stats", a, b, n, H, W, out, ws, ws.numel())
    inter, union = out[:, 0], out[:, 1]
    iou = torch.where(union > 0, inter.float() / union.clamp(min=1).float(), torch.zeros((), device=dev))
    if single:
        return MaskStats(inter[0], union[0], out[0, 2], out[0, 3], iou[0])
    return MaskStats(inter, union, out[:, 2], out[:, 3], iou)


def worst_frames(report, count):
    """indices of the `count` worst frames of a `SequenceInspector.report`: lowest IoU first where there are masks, else highest keypoint
    error first; ties go to the earlier frame.  One host read."""
    if "iou" in report:
        key = report["iou"].detach().cpu().numpy().astype(np.float64)
    elif "kp_err_px" in report:
        key = -report["kp_err_px"].detach().cpu().numpy().astype(np.float64)
    else:
        return []
    return [int(i) for i in np.argsort(key, kind="stable")[:max(int(count), 0)]]


class SequenceInspector:
    """body_model: deformers.smplx.SMPL on the GPU (with faces); K [3,3] and extrinsic [4,4] (or [3,4]): the host arrays of cameras.npz;
    H, W: the size of the frames; keypoints [F,25,3] (x, y, confidence in BODY_25 order) or None; masks [F,H,W] (uint8, bool or float:
    foreground is > 0) on the GPU or None; kp_vertex: the 11 vertices that stand in for the face and foot points."""
    CHUNK = 32      # frames whose silhouettes are held at a time

    def __init__(self, body_model, K, extrinsic, H, W, keypoints=None, masks=None, threshold=0.2, kp_vertex=SMPL_KP_VERTEX):
        from .raster import Camera
        if keypoints is None and masks is None:
            raise ValueError("SequenceInspector: neither keypoints nor masks: nothing to measure the poses against")
        self.faces = body_model.faces_tensor
        if self.faces.numel() == 0:
            raise ValueError("SequenceInspector: the body model has no faces (an SMPL file with `f`, or synthetic.make_mesh_body)")
        dev = self.faces.device
        if dev.type != "cuda":
            raise _lib.IAError("SequenceInspector: the body model must be on the GPU (got %s); there is no CPU path" % dev)
        self.device, self.H, self.W, self.threshold = dev, int(H), int(W), float(threshold)
        self.faces = self.faces.to(torch.int32).contiguous()
        K = np.asarray(K, np.float64).reshape(3, 3)
        E = np.asarray(extrinsic, np.float64)
        E = np.vstack([E.reshape(3, 4), [0, 0, 0, 1]]) if E.size == 12 else E.reshape(4, 4)
        self.camera = Camera(K, torch.as_tensor(E.astype(np.float32), device=dev), self.H, self.W)
        self.has_keypoints, self.has_masks = keypoints is not None, masks is not None
        if masks is not None:
            _lib.require_cuda(masks)
            if masks.dim() != 3 or tuple(masks.shape[1:]) != (self.H, self.W):
                raise ValueError("SequenceInspector: masks must be [F,%d,%d], got %s" % (self.H, self.W, tuple(masks.shape)))
            self.masks = (masks if masks.dtype in (torch.uint8, torch.bool) else masks > 0).contiguous()
        if keypoints is not None and not torch.is_tensor(keypoints):
            keypoints = np.asarray(keypoints, np.float32)
        F = int(masks.shape[0]) if keypoints is None else int(keypoints.shape[0])
        if masks is not None and masks.shape[0] != F:
            raise ValueError("SequenceInspector: %d rows of keypoints but %d masks" % (F, masks.shape[0]))
        kp = np.zeros((F, 25, 3), np.float32) if keypoints is None else keypoints
        self.refiner = KeypointRefiner(body_model, (K @ E[:3]).astype(np.float32), kp, threshold=threshold, kp_vertex=kp_vertex)
        self.keypoints, self.F = self.refiner.keypoints, F

    def _posed(self, betas, pose, transl):
        """-> verts [F,V,3] (the refiner's own buffer: the next call overwrites it), uv [F,25,2]"""
        out = self.refiner.loss(betas, pose, transl)
        return out["verts"], out["uv"]

    @torch.no_grad()
    def report(self, betas, pose, transl):
        """-> dict of device tensors [F].  With masks: inter, union, mask_area, sil_area (int32 pixel counts; the silhouette is
        `raster.rasterize(verts_f, faces, camera).mask`, the masks are thresholded > 0) and iou (float32; 0 where the union is empty).
        With keypoints: n_confident (int32: BODY_25 points with confidence > threshold, MidHip excluded as in the refiner) and kp_err_px
        (float32: the mean pixel distance between the projected model points and the detections over those points; 0 where there are none)."""
        from .raster import rasterize
        verts, uv = self._posed(betas, pose, transl)
        out = {}
        if self.has_masks:
            rows = []
            for f0 in range(0, self.F, self.CHUNK):
                f1 = min(f0 + self.CHUNK, self.F)
                sil = torch.stack([rasterize(verts[f], self.faces, self.camera).mask for f in range(f0, f1)])
                rows.append(mask_stats(self.masks[f0:f1], sil))
            out["inter"], out["union"], out["mask_area"], out["sil_area"], out["iou"] = (torch.cat([getattr(r, k) for r in rows])
                                                                                           for k in MaskStats._fields)
        if self.has_keypoints:
            sel = self.keypoints[..., 2] > self.threshold
            sel[:, MIDHIP] = False
            dist = (uv - self.keypoints[..., :2]).square().sum(-1).sqrt()
            n = sel.sum(1)
            out["n_confident"] = n.to(torch.int32)
            out["kp_err_px"] = torch.where(sel, dist, torch.zeros((), device=self.device)).sum(1) / n.clamp(min=1).float()
        return out

    @torch.no_grad()
    def overlay(self, images_u8, frame_indices, betas, pose, transl, opacity=0.5):
        """images_u8 [m,H,W,3] uint8 on the GPU: the frames `frame_indices` (m indices into the sequence) -> a new tensor with, in this
        order, the flat-shaded body blended in at `opacity` (0 .. 1), the mask outline, the detected skeleton in limb colours (points
        above the threshold) and the 25 projected model points as discs in one contrasting colour (the same kernel with S = 0)."""
        from .raster import rasterize
        idx = [int(i) for i in frame_indices]
        _u8(images_u8, "overlay: images_u8", 3)
        if tuple(images_u8.shape) != (len(idx), self.H, self.W, 3) or any(not 0 <= i < self.F for i in idx):
            raise ValueError("SequenceInspector.overlay: images [%d,%d,%d,3] and frame indices in [0, %d), got %s and %s"
                             % (len(idx), self.H, self.W, self.F, tuple(images_u8.shape), idx))
        if not idx:
            return images_u8.clone()
        verts, uv = self._posed(betas, pose, transl)
        layer = torch.stack([face_shade(rasterize(verts[f], self.faces, self.camera).face_id, verts[f], self.faces, self.camera.w2c) for f in idx])
        out = blend(images_u8, layer, int(round(float(opacity) * 256)))
        sel = torch.as_tensor(idx, device=self.device)
        if self.has_masks:
            outline(out, self.masks[sel])
        if self.has_keypoints:
            draw_skeleton(out, self.keypoints[sel], point_rgb=DETECTION_COLOUR, threshold=self.threshold, radius_q=DETECTION_RADIUS_Q)
        model = torch.cat([uv[sel], torch.ones((len(idx), 25, 1), device=self.device)], -1)
        draw_skeleton(out, model, segments=(), segment_rgb=(), threshold=0.5, radius_q=MODEL_RADIUS_Q)
        return out
