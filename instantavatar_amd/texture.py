"""A texture atlas over a triangle mesh: the colour field baked into one half of a square block of texels per face
(csrc/ia_texture.hip, include/instantavatar_hip_texture.h; definition in DESIGN.md section 4, "texture atlas").  `bake` evaluates any
`sample(points) -> (rgb, sigma)` at the surface point of every texel, optionally after snapping the point onto the level set along
the face normal; `sample` filters the atlas bilinearly at interpolated coordinates (`raster.render_textured`).  `Mesh.to_obj_textured`
writes the result as OBJ + MTL + PNG.  Everything stays on the device; `bake` reads nothing back.

The layout needs no unwrapping: face f lies in block f >> 1, half f & 1, with its corners on texel centres three texels short of the
block edge, so that bilinear filtering inside a face's triangle only ever reads texels that face owns."""
import numpy as np
import torch

from . import _lib

DEFAULT_LEVEL = 10.0      # (= mesh.DEFAULT_LEVEL)
MIN_BLOCK, MAX_BLOCK, MAX_SIZE = 4, 64, 16384


class Texture:
    """atlas [T,T,3] fp32 in the MODEL's channel order (B, G, R), zero where no face owns the texel; rgba8 [T,T,4] uint8 (alpha = owned,
    packed by ia_pack_rgba8); uv [nf,3,2] fp32 continuous texel coordinates of the corners (texel centre i at i + 0.5); block, size =
    B, T; unsnapped: device int32 scalar, the owned texels for which the snap found no crossing."""

    def __init__(self, atlas, rgba8, uv, block, size, unsnapped):
        self.atlas, self.rgba8, self.uv, self.block, self.size, self.unsnapped = atlas, rgba8, uv, int(block), int(size), unsnapped

    def vt(self):
        """[nf,3,2] float64 host array of OBJ texture coordinates: (x / T, 1 - y / T) of the corners' continuous coordinates (x, y)
        (PNG row 0 is y = 0, OBJ's v runs upwards)"""
        uv = self.uv.detach().cpu().numpy().astype(np.float64)
        return np.stack([uv[..., 0] / self.size, 1.0 - uv[..., 1] / self.size], -1)


def atlas_size(nf, block):
    """T, the atlas edge in texels, for `nf` faces in blocks of `block` texels; raises outside 4 <= block <= 64, T <= 16384"""
    nf, block = int(nf), int(block)
    T = int(_lib.call("ia_tex_atlas_size", nf, block))
    if T == 0:
        raise _lib.IAError("texture: %d faces in blocks of %d: the block edge must lie in [%d, %d] and the atlas edge cannot exceed %d"
                           % (nf, block, MIN_BLOCK, MAX_BLOCK, MAX_SIZE))
    return T


def corner_uv(nf, block, device="cuda"):
    """[nf,3,2] fp32 device tensor: the continuous texel coordinates of every face's corners"""
    T = atlas_size(nf, block)
    uv = torch.empty((int(nf), 3, 2), device=device)
    _lib.call("ia_tex_corner_uv", int(nf), int(block), T, uv)
    return uv


def snap_offsets(steps, dist):
    """t_k [steps] float32 = (k - (steps-1)/2) h with h = 2 dist / (steps-1), formed in fp32 as ia_tex_snap forms them"""
    h = np.float32(np.float32(2) * np.float32(dist)) / np.float32(steps - 1)
    return ((np.arange(steps) - (steps - 1) // 2).astype(np.float32) * h).astype(np.float32)


@torch.no_grad()
def bake(mesh, sample, block=8, snap=0.0, level=DEFAULT_LEVEL, steps=9, chunk=1 << 21):
    """Bake `sample(points [n,3] cuda fp32) -> (rgb [n,3], sigma [n])` into an atlas over `mesh` -> Texture.

    block: texels per block edge; snap: the distance along the face normal, on either side, within which every texel's point is
    moved onto sigma = level (0: the points stay on the faces) from `steps` (odd, 3 .. 17) density samples; chunk: texels per call
    of `sample` (the result does not depend on it).  `steps` + 1 calls of `sample` per chunk with a snap, one without."""
    _lib.require_cuda(mesh.verts, mesh.faces)
    verts = mesh.verts.detach().reshape(-1, 3).float().contiguous()
    faces = mesh.faces.detach().reshape(-1, 3).to(torch.int32).contiguous()
    nv, nf, B, K = int(verts.shape[0]), int(faces.shape[0]), int(block), int(steps)
    snap = float(snap)
    if not (snap >= 0 and np.isfinite(snap)):
        raise _lib.IAError("texture.bake: snap = %r must be finite and not negative" % (snap,))
    if K % 2 == 0 or not 3 <= K <= 17:
        raise _lib.IAError("texture.bake: steps = %d must be odd and in [3, 17]" % K)
    T = atlas_size(nf, B)
    dev = verts.device
    n = T * T
    chunk = max(1, min(int(chunk), n))
    atlas = torch.empty((n, 3), device=dev)
    owner = torch.empty(n, dtype=torch.int32, device=dev)
    unsnapped = torch.zeros((), dtype=torch.int32, device=dev)
    pts = torch.empty((chunk, 3), device=dev)
    if snap > 0:
        offsets = snap_offsets(K, snap)
        sig, t = torch.empty((K, chunk), device=dev), torch.empty(chunk, device=dev)
    for first in range(0, n, chunk):
        count = min(chunk, n - first)
        own = owner[first:first + count]
        p = pts[:count]
        if snap > 0:
            s = sig.reshape(-1)[:K * count].view(K, count)
            for k in range(K):
                _lib.call("ia_tex_texel_points", verts, nv, faces, nf, B, T, first, count, None, float(offsets[k]), p, None, own)
                s[k].copy_(sample(p)[1].reshape(count))
            _lib.call("ia_tex_snap", s, K, count, float(level), snap, own, t, unsnapped)
            _lib.call("ia_tex_texel_points", verts, nv, faces, nf, B, T, first, count, t, 0.0, p, None, None)
        else:
            _lib.call("ia_tex_texel_points", verts, nv, faces, nf, B, T, first, count, None, 0.0, p, None, own)
        rgb = sample(p)[0].reshape(count, 3).float()
        atlas[first:first + count] = torch.where((own >= 0)[:, None], rgb, torch.zeros_like(rgb))
    rgba8 = torch.empty((T, T, 4), dtype=torch.uint8, device=dev)
    _lib.call("ia_pack_rgba8", atlas, (owner >= 0).float(), n, rgba8)
    return Texture(atlas.view(T, T, 3), rgba8, corner_uv(nf, B, dev), B, T, unsnapped)


@torch.no_grad()
def sample(texture, uv, mask=None):
    """The atlas of `texture` filtered bilinearly at uv [...,2] (continuous texel coordinates, as `Texture.uv` interpolated over a
    face) -> [...,3] fp32; rows whose `mask` [...] is 0 or whose uv is not finite give 0 (ia_tex_sample)."""
    _lib.require_cuda(texture.atlas, uv, mask)
    shape = tuple(uv.shape[:-1])
    uv = uv.detach().reshape(-1, 2).float().contiguous()
    R = int(uv.shape[0])
    if mask is not None:
        mask = mask.detach().reshape(-1).float().contiguous()
        if mask.numel() != R:
            raise _lib.IAError("texture.sample: %d mask values for %d coordinates" % (mask.numel(), R))
    out = torch.empty((R, 3), device=uv.device)
    _lib.call("ia_tex_sample", texture.atlas, texture.size, uv, mask, R, out)
    return out.view(*shape, 3)
