"""A photo texture: the frames a sequence was recorded with, projected back onto the texture atlas of a mesh
(csrc/ia_phototex.hip, include/instantavatar_hip_phototex.h; definition in DESIGN.md section 4, "photo texture").  `bake` takes the
posed mesh, the camera, the image, the mask and the raster depth map of every frame and returns a `texture.Texture` with the layout
of `texture.bake` plus `seen`, the number of frames that saw every texel; `coverage_image` paints that count.  Everything stays on
the device; `bake` reads nothing back.

A texel takes a frame only when the frame looks at its face from the front (cosine above `cos_min`) and all four pixels of its
bilinear footprint lie inside the image, inside the mask and on the surface the posed mesh shows there (raster depth within
`depth_tol` of the texel's own depth); the frames are averaged with the weights cosine^`power`.  The defaults (0.3, 2, 0.02 m, 1
frame) are this project's choices."""
import torch

from . import _lib, texture


def _flush(pending, verts_shape, faces, nf, B, T, n, chunk, acc, stride, cos_min, power, depth_tol):
    """one accumulate call per range of texels for the frames in `pending` (same camera intrinsics, image size, masks or none)"""
    cam = pending[0][1]
    F, nv = len(pending), verts_shape
    verts = torch.stack([p[0] for p in pending]).contiguous()
    w2c = torch.stack([p[1].w2c for p in pending]).contiguous()
    images = torch.stack([p[2] for p in pending]).contiguous()
    masks = None if pending[0][3] is None else torch.stack([p[3] for p in pending]).contiguous()
    depth = torch.stack([p[4] for p in pending]).contiguous()
    for first in range(0, n, chunk):
        count = min(chunk, n - first)
        _lib.call("ia_phototex_accumulate", verts, nv, faces, nf, B, T, first, count, F, w2c, cam.fx, cam.fy, cam.cx, cam.cy, cam.near,
                  images, masks, depth, cam.H, cam.W, cos_min, power, depth_tol, acc[first * stride:(first + count) * stride])


@torch.no_grad()
def bake(mesh, frames_iter, block=8, base=None, cos_min=0.3, power=2.0, depth_tol=0.02, min_frames=1, chunk_frames=16, chunk=1 << 21):
    """Project frames onto the atlas of `mesh` -> (Texture, seen [T,T] int32).

    frames_iter yields, per frame, (posed_verts [nv,3] fp32, camera (`raster.Camera`), image_u8 [H,W,3] uint8 in the model's channel
    order, mask [H,W] fp32 or None, depth [H,W] fp32: the raster depth of the posed mesh under that camera).  `mesh` gives the faces
    and, through its own vertices, the owner of every texel.  base: the atlas [T,T,3] (or a Texture of the same layout) a texel seen
    by fewer than `min_frames` frames falls back to; None: zero.  chunk_frames: frames per launch; chunk: texels per launch (the
    result depends on neither).  The Texture's `unsnapped` is the device count of owned texels that no frame saw (also `unseen`)."""
    _lib.require_cuda(mesh.verts, mesh.faces)
    verts = mesh.verts.detach().reshape(-1, 3).float().contiguous()
    faces = mesh.faces.detach().reshape(-1, 3).to(torch.int32).contiguous()
    nv, nf, B = int(verts.shape[0]), int(faces.shape[0]), int(block)
    cos_min, power, depth_tol, min_frames = float(cos_min), float(power), float(depth_tol), int(min_frames)
    if not 0 <= cos_min < 1:
        raise _lib.IAError("phototex.bake: cos_min = %r outside [0, 1)" % (cos_min,))
    if not (power >= 0 and power != float("inf")):
        raise _lib.IAError("phototex.bake: power = %r must be finite and not negative" % (power,))
    if not (depth_tol >= 0 and depth_tol != float("inf")):
        raise _lib.IAError("phototex.bake: depth_tol = %r must be finite and not negative" % (depth_tol,))
    if min_frames < 1 or int(chunk_frames) < 1:
        raise _lib.IAError("phototex.bake: min_frames and chunk_frames must be at least 1")
    T = texture.atlas_size(nf, B)
    dev = verts.device
    n = T * T
    chunk = max(1, min(int(chunk), n))
    if isinstance(base, texture.Texture):
        if (base.block, base.size) != (B, T):
            raise _lib.IAError("phototex.bake: the base texture has blocks of %d in an atlas of %d, the mesh needs %d in %d"
                               % (base.block, base.size, B, T))
        base = base.atlas
    if base is not None:
        _lib.require_cuda(base)
        if base.numel() != 3 * n:
            raise _lib.IAError("phototex.bake: the base atlas has %d values, the atlas of the mesh %d x %d x 3" % (base.numel(), T, T))
        base = base.detach().reshape(n, 3).float().contiguous()
    stride = int(_lib.call("ia_phototex_acc_bytes", 1))
    acc = torch.empty(int(_lib.call("ia_phototex_acc_bytes", n)), dtype=torch.uint8, device=dev)
    _lib.call("ia_phototex_zero", acc, n)
    pending, key = [], None
    for posed, cam, image, mask, depth in frames_iter:
        _lib.require_cuda(posed, cam.w2c, image, mask, depth)
        posed = posed.detach().reshape(-1, 3).float()
        if posed.shape[0] != nv:
            raise _lib.IAError("phototex.bake: a frame has %d posed vertices, the mesh %d" % (posed.shape[0], nv))
        if image.dtype != torch.uint8 or tuple(image.shape) != (cam.H, cam.W, 3):
            raise _lib.IAError("phototex.bake: a frame's image is %s %s, the camera needs uint8 (%d, %d, 3)"
                               % (image.dtype, tuple(image.shape), cam.H, cam.W))
        if tuple(depth.shape) != (cam.H, cam.W) or (mask is not None and tuple(mask.shape) != (cam.H, cam.W)):
            raise _lib.IAError("phototex.bake: a frame's depth map or mask is not %d x %d" % (cam.H, cam.W))
        k = (cam.fx, cam.fy, cam.cx, cam.cy, cam.near, cam.H, cam.W, mask is None)
        if pending and (k != key or len(pending) == int(chunk_frames)):
            _flush(pending, nv, faces, nf, B, T, n, chunk, acc, stride, cos_min, power, depth_tol)
            pending = []
        key = k
        pending.append((posed, cam, image, None if mask is None else mask.detach().float(), depth.detach().float()))
    if pending:
        _flush(pending, nv, faces, nf, B, T, n, chunk, acc, stride, cos_min, power, depth_tol)
    atlas = torch.empty((n, 3), device=dev)
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    seen = torch.empty(n, dtype=torch.int32, device=dev)
    unseen = torch.zeros((), dtype=torch.int32, device=dev)
    pts = torch.empty((chunk, 3), device=dev)
    for first in range(0, n, chunk):
        count = min(chunk, n - first)
        own = owner[first:first + count]
        _lib.call("ia_tex_texel_points", verts, nv, faces, nf, B, T, first, count, None, 0.0, pts[:count], None, own)
        _lib.call("ia_phototex_resolve", acc[first * stride:(first + count) * stride], None if base is None else base[first:first + count],
                  own, count, min_frames, atlas[first:first + count], seen[first:first + count], unseen)
    rgba8 = torch.empty((T, T, 4), dtype=torch.uint8, device=dev)
    _lib.call("ia_pack_rgba8", atlas, (owner >= 0).float(), n, rgba8)
    tex = texture.Texture(atlas.view(T, T, 3), rgba8, texture.corner_uv(nf, B, dev), B, T, unseen)
    tex.unseen = unseen
    return tex, seen.view(T, T)


@torch.no_grad()
def coverage_image(seen, owner, top=None):
    """rgba8 [T,T,4] uint8 in the model's channel order: the count `seen` [T,T] on the ramp of `meshdist.heat` turned round -- red: no
    frame, green: half of `top`, blue: `top` frames or more (None: the largest count, at least 1, which costs one host read); alpha =
    owned (`owner` [T,T]: the face of every texel or -1, or a bool mask)."""
    from . import meshdist
    _lib.require_cuda(seen, owner)
    T = int(seen.shape[0])
    n = T * T
    s = seen.detach().reshape(n).float()
    if top is None:
        top = max(1.0, float(s.max())) if n else 1.0
    rgb = meshdist.heat(float(top) - s, float(top)).contiguous()
    owned = owner.detach().reshape(n)
    owned = (owned if owned.dtype == torch.bool else owned >= 0).float().contiguous()
    rgba8 = torch.empty((T, T, 4), dtype=torch.uint8, device=seen.device)
    _lib.call("ia_pack_rgba8", rgb, owned, n, rgba8)
    return rgba8
