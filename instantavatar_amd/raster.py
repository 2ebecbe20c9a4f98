"""Pictures of triangle meshes: a deterministic z-buffer rasteriser on the GPU (csrc/ia_raster.hip,
include/instantavatar_hip_raster.h; definition in DESIGN.md section 4, "rasteriser").  `rasterize` gives face ids, depth and
interpolated vertex attributes per pixel; `render` (`Mesh.render`, `AvatarModel.render_mesh`) packs colour, normal and shaded
8-bit images of a `mesh.Mesh` with the kernels the volumetric frames are packed with.  Everything stays on the device.

The camera is the OpenCV pinhole of `drivers/animate.make_rays` sampled at integer pixel positions, so a raster frame of a
posed mesh overlays the volumetric frame of the same batch."""
import collections

import numpy as np
import torch

from . import _lib

#: face_id [H,W] int32 (-1: empty), depth [H,W] fp32 (camera z, 0: empty), attrs [H,W,C] fp32 or None, mask [H,W] bool;
#: counts: device int32 [2] = faces skipped (invalid vertex, degenerate, culled), covered pixels
RasterFrame = collections.namedtuple("RasterFrame", "face_id depth attrs mask counts")


class Camera:
    """K: host 3x3 intrinsics (fx, fy, cx, cy are read and rounded to fp32, which is how the C ABI takes them; no skew);
    w2c: DEVICE [4,4] world -> camera (x right, y down, z forward);
    H, W: image size; near: vertices closer than this (camera z) are invalid, and so are their faces."""

    def __init__(self, K, w2c, H, W, near=0.05):
        K = np.asarray(K, np.float64)
        if K.shape != (3, 3) or K[0, 1] != 0:
            raise ValueError("Camera: K must be a 3x3 pinhole matrix without skew")
        self.K = K
        self.fx, self.fy, self.cx, self.cy = (float(np.float32(v)) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
        if not torch.is_tensor(w2c):
            raise TypeError("Camera: w2c is a device tensor [4,4] (it may change per frame without a host copy)")
        self.w2c = w2c.detach().reshape(4, 4).float().contiguous()
        self.H, self.W, self.near = int(H), int(W), float(near)
        self._rays = None

    @classmethod
    def from_sequence(cls, seq, near=0.05):
        """the camera of a `drivers.animate.AnimateSequence`: its K, c2w = I, its image size"""
        return seq.camera(near=near)

    def rays_d(self):
        """[H*W,3] unit ray directions K^-1 [x, y, 1] in the CAMERA frame (what `ia_pack_normals8` lights along), built once"""
        if self._rays is None or self._rays.device != self.w2c.device:
            dev = self.w2c.device
            x = (torch.arange(self.W, device=dev, dtype=torch.float32) - self.cx) / self.fx
            y = (torch.arange(self.H, device=dev, dtype=torch.float32) - self.cy) / self.fy
            d = torch.stack([x[None, :].expand(self.H, self.W), y[:, None].expand(self.H, self.W), torch.ones(self.H, self.W, device=dev)], -1)
            self._rays = (d / d.norm(dim=-1, keepdim=True)).reshape(-1, 3).contiguous()
        return self._rays


def look_at_box(lo, hi, size, device, fill=0.9):
    """The camera of `extract_mesh --render`: on the -z side of the box [lo, hi], on the axis through its centre, looking along
    +z at the centre, world +y up in the image (so world +x points LEFT: the view is from behind a body that faces +z).  Square
    image of `size` pixels, focal length = size, at the distance at which the box's nearest face fills `fill` of the image."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, e = (lo + hi) / 2, hi - lo
    dist = max(e[0], e[1]) / fill + e[2] / 2            # nearest face at dist - e_z / 2, where an extent e spans f e / z pixels
    R = np.diag([-1.0, -1.0, 1.0])                      # x_cam = -x, y_cam = -y (down), z_cam = z: a proper rotation
    eye = c - np.array([0.0, 0.0, dist])
    w2c = np.eye(4)
    w2c[:3, :3], w2c[:3, 3] = R, -R @ eye
    K = np.array([[float(size), 0, (size - 1) / 2], [0, float(size), (size - 1) / 2], [0, 0, 1]])
    return Camera(K, torch.as_tensor(w2c, dtype=torch.float32, device=device), size, size, near=min(0.05, dist / 100))


@torch.no_grad()
def rasterize(verts, faces, camera, attrs=None, cull=False):
    """verts [nv,3] fp32, faces [nf,3] int32, attrs [nv,C] fp32 (1 <= C <= 8) or None -> RasterFrame.  Three entry points
    (project, visibility, resolve), no host read."""
    _lib.require_cuda(verts, faces, camera.w2c, attrs)
    verts = verts.detach().reshape(-1, 3).float().contiguous()
    faces = faces.detach().reshape(-1, 3).to(torch.int32).contiguous()
    nv, nf, H, W = verts.shape[0], faces.shape[0], camera.H, camera.W
    dev = verts.device
    C = 0
    if attrs is not None:
        attrs = attrs.detach().reshape(nv, -1).float().contiguous()
        C = attrs.shape[1]
    nb = int(_lib.call("ia_raster_workspace_bytes", nv, nf, H, W))
    if nb == 0:
        raise _lib.IAError("rasterize: %d vertices, %d faces, a %d x %d image: outside 1 <= H, W <= 16384" % (nv, nf, H, W))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    xy, inv_z = torch.empty((nv, 2), dtype=torch.int32, device=dev), torch.empty(nv, device=dev)
    vis = torch.empty(H * W, dtype=torch.int64, device=dev)
    face_id, depth = torch.empty((H, W), dtype=torch.int32, device=dev), torch.empty((H, W), device=dev)
    out = torch.empty((H, W, C), device=dev) if C else None
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call("ia_raster_project", verts, nv, camera.w2c, camera.fx, camera.fy, camera.cx, camera.cy, camera.near, xy, inv_z)
    _lib.call("ia_raster_visibility", xy, inv_z, nv, faces, nf, H, W, int(bool(cull)), vis, ws, nb)
    _lib.call("ia_raster_resolve", xy, inv_z, nv, faces, nf, vis, H, W, attrs, C, ws, nb, face_id, depth, out, counts)
    return RasterFrame(face_id, depth, out, face_id >= 0, counts)


@torch.no_grad()
def render(mesh, camera, light=None, cull=True):
    """`Mesh.render`: dict of device tensors -- rgba8 [H,W,4] uint8 (vertex colours in the MODEL's channel order, as the frames
    `drivers.animate.write_frames` takes; alpha = covered), normal8 [H,W,4] ((n + 1) / 2 in the camera frame, covered), shaded8
    [H,W,4] (max(0, n . l); light: device float [3] in the camera frame, None = towards the camera along the pixel's ray), depth
    [H,W] fp32 (camera z, 0 = empty), mask [H,W] bool, face_id [H,W] int32.  Colour and normal go through ONE resolve (6 channels);
    the interpolated normal is renormalised by `ia_unit_negative`; packing is `ia_pack_rgba8` / `ia_pack_normals8`."""
    _lib.require_cuda(mesh.verts, mesh.faces, mesh.normals, mesh.colors, camera.w2c, light)
    H, W = camera.H, camera.W
    dev = mesh.verts.device
    n_cam = mesh.normals.detach().float() @ camera.w2c[:3, :3].T           # world -> camera frame (a rotation)
    frame = rasterize(mesh.verts, mesh.faces, camera, torch.cat([mesh.colors.detach().float(), n_cam], 1), cull)
    R = H * W
    rgb = frame.attrs[..., :3].reshape(R, 3).contiguous()
    minus_n = (-frame.attrs[..., 3:]).reshape(R, 3).contiguous()
    normal = torch.empty((R, 3), device=dev)
    _lib.call("ia_unit_negative", minus_n, R, normal)                        # -(-n) / |n|; zero stays zero (empty pixels)
    rgba8, normal8, shaded8 = (torch.empty((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(3))
    _lib.call("ia_pack_rgba8", rgb, frame.mask.reshape(R).float(), R, rgba8)
    _lib.call("ia_pack_normals8", normal, camera.rays_d(), light, R, normal8, shaded8)
    return dict(rgba8=rgba8, normal8=normal8, shaded8=shaded8, depth=frame.depth, mask=frame.mask, face_id=frame.face_id)


@torch.no_grad()
def render_textured(mesh, camera, light=None, cull=True):
    """`Mesh.render` of a mesh with a `texture`: the dict of `render` with rgba8 holding the atlas colours filtered at the
    interpolated corner coordinates (ia_tex_sample), plus uv [H,W,2] fp32 (continuous texel coordinates, 0 = empty).  Texture
    coordinates belong to corners, not vertices, so the unshared copy verts[faces] is rasterised with faces = arange: the same
    position bits in the same face order, hence the face_id and depth of `render`.  One resolve of 5 channels: uv and the
    camera-frame normal."""
    from . import texture as texture_mod
    tex = mesh.texture
    if tex is None:
        raise _lib.IAError("render_textured: the mesh has no texture (AvatarModel.bake_texture / texture.bake make one)")
    _lib.require_cuda(mesh.verts, mesh.faces, mesh.normals, tex.atlas, tex.uv, camera.w2c, light)
    H, W = camera.H, camera.W
    dev = mesh.verts.device
    verts = mesh.verts.detach().reshape(-1, 3).float()
    faces = mesh.faces.detach().reshape(-1, 3).long()
    nv, nf = verts.shape[0], faces.shape[0]
    if tex.uv.shape[0] != nf:
        raise _lib.IAError("render_textured: the texture was baked over %d faces, the mesh has %d" % (tex.uv.shape[0], nf))
    n_cam = mesh.normals.detach().float() @ camera.w2c[:3, :3].T           # world -> camera frame (a rotation)
    # a face with an index outside [0, nv) is skipped by `render`: here its corners become invalid vertices
    bad = ((faces < 0) | (faces >= nv)).any(1, keepdim=True).expand(nf, 3).reshape(-1)
    idx = faces.clamp(0, max(nv - 1, 0)).reshape(-1)
    corners = torch.where(bad[:, None], torch.full((1, 3), float("nan"), device=dev), verts[idx]) if nv else verts.new_zeros((0, 3))
    attrs = torch.cat([tex.uv.reshape(-1, 2).float(), n_cam[idx]], 1) if nv else verts.new_zeros((0, 5))
    frame = rasterize(corners, torch.arange(3 * nf, dtype=torch.int32, device=dev).reshape(-1, 3), camera, attrs, cull)
    R = H * W
    uv = frame.attrs[..., :2].contiguous()
    mask = frame.mask.reshape(R).float()
    rgb = texture_mod.sample(tex, uv.reshape(R, 2), mask)
    minus_n = (-frame.attrs[..., 2:]).reshape(R, 3).contiguous()
    normal = torch.empty((R, 3), device=dev)
    _lib.call("ia_unit_negative", minus_n, R, normal)
    rgba8, normal8, shaded8 = (torch.empty((H, W, 4), dtype=torch.uint8, device=dev) for _ in range(3))
    _lib.call("ia_pack_rgba8", rgb, mask, R, rgba8)
    _lib.call("ia_pack_normals8", normal, camera.rays_d(), light, R, normal8, shaded8)
    return dict(rgba8=rgba8, normal8=normal8, shaded8=shaded8, depth=frame.depth, mask=frame.mask, face_id=frame.face_id, uv=uv)
