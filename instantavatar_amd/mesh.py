"""Triangle meshes of the avatar: the isosurface of the canonical density field by marching tetrahedra on the GPU
(csrc/ia_isosurface.hip, include/instantavatar_hip_mesh.h; definition in DESIGN.md section 4, "isosurface"), its largest
connected component, per-vertex colours and normals from the field, forward skinning into a posed frame, and PLY / OBJ
writers (numpy only).  `AvatarModel.extract_mesh` / `AvatarModel.pose_mesh` are the public entry points.  `simplify`, `smooth` and
`vertex_normals` process a mesh afterwards (csrc/ia_meshops.hip, include/instantavatar_hip_meshops.h; DESIGN.md section 4, "mesh
simplification"): vertex clustering with quadrics, Taubin smoothing, normals from the faces.  A mesh may carry a texture atlas baked
from the colour field (`texture`, `AvatarModel.bake_texture`; DESIGN.md section 4, "texture atlas"): `pose` keeps it, `smooth` and
`simplify` return meshes without one, since the atlas belongs to the faces and positions it was baked over.  `Mesh.to_glb` writes
the mesh, a rig (`rig.Rig`) and a pose track as one glTF binary ("rigged export").  `Mesh.distance_to` and
`Mesh.compare` measure the distance to another mesh, `Mesh.raycast`, `Mesh.contains` and `Mesh.signed_distance_to` ask where a ray meets
the mesh and on which side of it a point lies ("ray queries"), `Mesh.from_ply` / `Mesh.from_obj` read the written files back (`meshdist`;
DESIGN.md section 4, "surface distance").

The level is OURS: the reference ships a marching-cubes helper it never calls, whose default level 0 is meant for signed
distances; sigma = 10 is a density at which a 1 cm step is already ~10 % opaque.  It is a parameter."""
import time

import numpy as np
import torch

from . import _lib

DEFAULT_LEVEL = 10.0


class Mesh:
    """verts [nv,3] fp32, faces [nf,3] int32, normals [nv,3] fp32 (unit length or zero), colors [nv,3] fp32 in [0, 1] in the
    MODEL's channel order (B, G, R: the cv2.imread order of the training images) -- device tensors."""

    def __init__(self, verts, faces, normals, colors):
        self.verts, self.faces, self.normals, self.colors = verts, faces, normals, colors
        #: a `texture.Texture` baked over these faces (`AvatarModel.bake_texture`), or None: the mesh carries vertex colours only
        self.texture = None

    def render(self, camera, light=None, cull=True):
        """8-bit pictures of the mesh under `camera` (`raster.Camera`) by the GPU rasteriser: a dict of device tensors rgba8,
        normal8, shaded8 [H,W,4] uint8, depth [H,W], mask [H,W] (and face_id) -- see `raster.render`.  A mesh with a texture is
        drawn with it (`raster.render_textured`, which adds `uv`)."""
        from . import raster
        if self.texture is not None:
            return raster.render_textured(self, camera, light, cull)
        return raster.render(self, camera, light, cull)

    def simplify(self, cell, box=None, reg=1e-3):
        """`simplify(self, cell, box, reg)`: one vertex per occupied cell of edge `cell`"""
        return simplify(self, cell, box, reg)

    def smooth(self, iters=10, lam=0.5, mu=-0.53):
        """`smooth(self, iters, lam, mu)`: Taubin smoothing of the positions"""
        return smooth(self, iters, lam, mu)

    def distance_to(self, other):
        """per vertex of this mesh the closest point of `other` (`meshdist.closest`): a dict of dist [nv], face [nv], bary [nv,3] and
        point [nv,3]; a vertex with a non-finite coordinate gets dist = NaN and face = -1"""
        from . import meshdist
        return meshdist.closest(self.verts, other)

    def compare(self, other, samples=100000, taus=(), signed=False):
        """`meshdist.compare(self, other, samples, taus, signed)`: distances both ways, Chamfer, Hausdorff, normal consistency, F-scores;
        signed: also on which side of the other mesh the samples lie"""
        from . import meshdist
        return meshdist.compare(self, other, samples, taus, signed)

    def raycast(self, origins, dirs, t_min=None, t_max=None):
        """the first hit of the rays origins + t dirs with this mesh (`meshdist.TriangleGrid.raycast`; the grid is built for this one
        call): a dict of t [P] (+inf: none), face [P], bary [P,3] and point [P,3]"""
        from . import meshdist
        return meshdist.TriangleGrid(self).raycast(origins, dirs, t_min, t_max)

    def contains(self, points):
        """[P] bool: the points inside this mesh, which must be a closed surface (`meshdist.TriangleGrid.contains`)"""
        from . import meshdist
        return meshdist.TriangleGrid(self).contains(points)

    def signed_distance_to(self, other):
        """`distance_to(other)` with dist negative for the vertices inside `other` (a closed surface), and `inside` [nv] bool"""
        from . import meshdist
        return meshdist.TriangleGrid(other).signed_distance(self.verts)

    @classmethod
    def from_ply(cls, path, device):
        """a Mesh on `device` from a PLY file: what `to_ply` writes (verts, faces and normals come back with the same bytes; colours in
        their 8-bit steps), or a plain binary little-endian / ASCII PLY (`meshdist.read_ply`)"""
        from . import meshdist
        if not str(path).lower().endswith(".ply"):
            raise _lib.IAError("from_ply: %s is not a .ply file" % path)
        return meshdist.load_mesh(path, device)

    @classmethod
    def from_obj(cls, path, device):
        """a Mesh on `device` from a Wavefront OBJ: what `to_obj` / `to_obj_textured` write (without the texture), or a plain OBJ with
        `v` / `f` lines (`meshdist.read_obj`)"""
        from . import meshdist
        if not str(path).lower().endswith(".obj"):
            raise _lib.IAError("from_obj: %s is not a .obj file" % path)
        return meshdist.load_mesh(path, device)

    def _host(self):
        f = lambda t: t.detach().cpu().numpy()
        rgb = f(self.colors).astype(np.float32)[:, ::-1]          # model order -> RGB, as drivers/animate.write_frames
        rgb8 = (np.clip(rgb, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)   # quantised as ia_pack_rgba8
        return f(self.verts).astype("<f4"), f(self.faces).astype("<i4"), f(self.normals).astype("<f4"), rgb8

    def to_ply(self, path):
        """binary little-endian PLY: vertex = float x y z nx ny nz, uchar red green blue; face = list uchar int32"""
        v, f, n, c = self._host()
        vert = np.empty(len(v), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                       ("red", "u1"), ("green", "u1"), ("blue", "u1")])
        for k, name in enumerate(("x", "y", "z")):
            vert[name] = v[:, k]
            vert["n" + name] = n[:, k]
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
        face = np.empty(len(f), dtype=[("n", "u1"), ("v", "<i4", (3,))])
        face["n"] = 3
        face["v"] = f
        header = ("ply\nformat binary_little_endian 1.0\ncomment instantavatar_amd mesh\nelement vertex %d\n"
                  "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %d\n"
                  "property list uchar int vertex_indices\nend_header\n" % (len(v), len(f)))
        with open(path, "wb") as out:
            out.write(header.encode("ascii"))
            out.write(vert.tobytes())
            out.write(face.tobytes())

    def to_obj(self, path):
        """Wavefront OBJ: `v x y z r g b` (colours in [0, 1], 8-bit steps), `vn`, `f a//a b//b c//c` (1-based)"""
        v, f, n, c = self._host()
        with open(path, "w") as out:
            out.write("# instantavatar_amd mesh: %d vertices, %d faces\n" % (len(v), len(f)))
            np.savetxt(out, np.concatenate([v.astype(np.float64), c.astype(np.float64) / 255.0], 1), fmt="v %.9g %.9g %.9g %.6g %.6g %.6g")
            np.savetxt(out, n.astype(np.float64), fmt="vn %.9g %.9g %.9g")
            g = f.astype(np.int64) + 1
            np.savetxt(out, np.stack([g[:, 0], g[:, 0], g[:, 1], g[:, 1], g[:, 2], g[:, 2]], 1), fmt="f %d//%d %d//%d %d//%d")

    def to_obj_textured(self, path, mtllib=None):
        """Wavefront OBJ with the baked texture: `path` holds `mtllib`, `v x y z`, `vn`, three `vt` per face (corner (x, y) in
        continuous texels -> (x / T, 1 - y / T)), `usemtl` and `f a/ta/a b/tb/b c/tc/c` (1-based); `<stem>.mtl` next to it names
        `<stem>.png`, the atlas in RGB order without alpha, row 0 = y = 0.  mtllib: the .mtl of another mesh in the same directory;
        only the OBJ is written then and names it -- posed meshes share the canonical mesh's material and picture."""
        import os
        if self.texture is None:
            raise _lib.IAError("to_obj_textured: the mesh has no texture (AvatarModel.bake_texture / texture.bake make one)")
        v, f, n, _ = self._host()
        if len(f) != self.texture.uv.shape[0]:
            raise _lib.IAError("to_obj_textured: the texture was baked over %d faces, the mesh has %d" % (self.texture.uv.shape[0], len(f)))
        mtl = os.path.splitext(path if mtllib is None else mtllib)[0] + ".mtl"
        if mtllib is None:
            from PIL import Image
            png = os.path.splitext(path)[0] + ".png"
            Image.fromarray(np.ascontiguousarray(self.texture.rgba8.detach().cpu().numpy()[..., 2::-1]), "RGB").save(png)
            with open(mtl, "w") as out:
                out.write("# instantavatar_amd texture: %d x %d texels, blocks of %d\nnewmtl avatar\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 1\n"
                          "map_Kd %s\n" % (self.texture.size, self.texture.size, self.texture.block, os.path.basename(png)))
        with open(path, "w") as out:
            out.write("# instantavatar_amd mesh: %d vertices, %d faces, textured\nmtllib %s\n" % (len(v), len(f), os.path.basename(mtl)))
            np.savetxt(out, v.astype(np.float64), fmt="v %.9g %.9g %.9g")
            np.savetxt(out, n.astype(np.float64), fmt="vn %.9g %.9g %.9g")
            np.savetxt(out, self.texture.vt().reshape(-1, 2), fmt="vt %.9g %.9g")
            out.write("usemtl avatar\n")
            g = f.astype(np.int64) + 1
            t = np.arange(3 * len(f), dtype=np.int64).reshape(-1, 3) + 1
            np.savetxt(out, np.stack([g[:, 0], t[:, 0], g[:, 0], g[:, 1], t[:, 1], g[:, 1], g[:, 2], t[:, 2], g[:, 2]], 1),
                       fmt="f %d/%d/%d %d/%d/%d %d/%d/%d")

    def to_glb(self, path, rig=None, animation=None, fps=30):
        """glTF 2.0 binary (`gltf.write_glb`; DESIGN.md section 4, "rigged export"): the mesh with its texture when it carries one
        (un-indexed, the atlas embedded as the PNG `to_obj_textured` writes) and with its vertex colours otherwise; rig: a
        `rig.Rig` of this (canonical) mesh -> a skin of 24 joints; animation: (quat [F,24,4], root_t [F,3]) of `rig.track` -> the
        pose track as key frames i / fps.  Zero normals are replaced by `vertex_normals` of the mesh."""
        from . import gltf
        v, f, n, rgb8 = self._host()
        if rig is None and animation is not None:
            raise _lib.IAError("to_glb: an animation needs a rig (AvatarModel.rig_mesh / rig.build make one)")
        kw = {}
        if not (np.isfinite(n).all() and (np.abs(n).max(1, initial=0.0) > 0).all()) and self.verts.is_cuda:
            kw["fallback_normals"] = vertex_normals(self.verts, self.faces).cpu().numpy()
        if self.texture is not None:
            if len(f) != self.texture.uv.shape[0]:
                raise _lib.IAError("to_glb: the texture was baked over %d faces, the mesh has %d" % (self.texture.uv.shape[0], len(f)))
            vt = self.texture.vt()
            kw["corner_uv"] = np.stack([vt[..., 0], 1.0 - vt[..., 1]], -1)       # glTF's origin is top-left, as the PNG's
            kw["image"] = np.ascontiguousarray(self.texture.rgba8.detach().cpu().numpy()[..., 2::-1])
        else:
            kw["colors8"] = rgb8
        if rig is not None:
            host = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
            if rig.joints.shape[0] != len(v):
                raise _lib.IAError("to_glb: the rig has %d vertices, the mesh %d" % (rig.joints.shape[0], len(v)))
            kw.update(joints=host(rig.joints), weights=host(rig.weights), parents=rig.parents, rest_translation=rig.rest_translation,
                      cano_quat=rig.cano_quat, inverse_bind=rig.inverse_bind)
            if animation is not None:
                kw.update(animation=tuple(host(a) for a in animation), fps=fps)
        gltf.write_glb(path, v, f, n, **kw)


def field_box(net):
    """(lo, hi) fp32 [3] of the box the field normalises to the unit cube: center -/+ scale / 2, formed in fp32"""
    center, scale = (np.asarray(t, np.float32) for t in net._center_scale_host())
    half = scale / np.float32(2)
    return center - half, center + half


def lattice_desc(N, lo, hi):
    d = _lib.OccGrid()
    d.G = int(N)
    d.aabb_min[:], d.aabb_max[:] = [float(x) for x in lo], [float(x) for x in hi]
    return d


def lattice_sigma(net, lat, chunk=1 << 21):
    """sigma [N^3] of `net` (ia_field_fwd, canonical space, no deformer) on the lattice, evaluated `chunk` points at a time"""
    N = lat.G
    n = N ** 3
    dev = net.center.device
    chunk = max(1, min(int(chunk), n))
    sigma = torch.empty(n, device=dev)
    pts, rgb = torch.empty((chunk, 3), device=dev), torch.empty((chunk, 3), device=dev)
    for first in range(0, n, chunk):
        count = min(chunk, n - first)
        _lib.call("ia_iso_lattice_points", lat, first, count, pts)
        _lib.call("ia_field_fwd", pts, count, None, net.field_desc(count), rgb, sigma[first:first + count])
    return sigma


def isosurface(sigma, lat, level=DEFAULT_LEVEL, cap=True):
    """marching tetrahedra on a device lattice sigma [N^3] -> (verts [nv,3] fp32, faces [nf,3] int32).  One host read: the two counts."""
    _lib.require_cuda(sigma)
    N = lat.G
    sigma = sigma.detach().reshape(-1).float().contiguous()
    if sigma.numel() != N ** 3:
        raise _lib.IAError("isosurface: %d samples for a lattice of %d^3" % (sigma.numel(), N))
    dev = sigma.device
    nb = int(_lib.call("ia_iso_workspace_bytes", N))
    if nb == 0:
        raise _lib.IAError("isosurface: resolution %d outside [2, 564]" % N)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call("ia_iso_count", sigma, N, float(level), int(bool(cap)), ws, nb, counts)
    nv, nf = counts.tolist()
    verts, faces = torch.empty((nv, 3), device=dev), torch.empty((nf, 3), dtype=torch.int32, device=dev)
    _lib.call("ia_iso_emit", sigma, lat, float(level), int(bool(cap)), ws, nb, verts, nv, faces, nf)
    return verts, faces


def largest_component(verts, faces, area_unit):
    """-> (verts, faces, vert_src [nv_out] int32) of the component with the largest surface area; order preserved"""
    _lib.require_cuda(verts, faces)
    nv, nf = verts.shape[0], faces.shape[0]
    dev = verts.device
    nb = int(_lib.call("ia_mesh_component_workspace_bytes", nv, nf))
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.call("ia_mesh_largest_count", verts, faces, nv, nf, float(area_unit), ws, nb, counts)
    nv2, nf2 = counts.tolist()
    v2, f2 = torch.empty((nv2, 3), device=dev), torch.empty((nf2, 3), dtype=torch.int32, device=dev)
    src = torch.empty(nv2, dtype=torch.int32, device=dev)
    _lib.call("ia_mesh_largest_emit", verts, faces, nv, nf, ws, nb, v2, nv2, f2, nf2, src)
    return v2, f2, src


def box_area_unit(lo, hi):
    """the largest face area of the box: the unit of the component filter's fixed-point areas"""
    e = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return float(max(e[0] * e[1], e[1] * e[2], e[0] * e[2]))


@torch.no_grad()
def extract(net, resolution=256, level=DEFAULT_LEVEL, largest=True, cap=True, chunk=1 << 21, timings=None):
    """The canonical mesh of the field `net` (NeRFNGPNet): `AvatarModel.extract_mesh`.
    timings: a dict that receives the wall time in seconds of `field` (lattice sigma), `isosurface` (count + emit),
    `component` (the filter) and `attributes` (colours, normals); measuring synchronises after every stage."""
    _lib.require_cuda(net.center)
    clock = None
    if timings is not None:
        def clock(name, t0):
            torch.cuda.synchronize()
            timings[name] = time.perf_counter() - t0
            return time.perf_counter()
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    lo, hi = field_box(net)
    lat = lattice_desc(resolution, lo, hi)
    sigma = lattice_sigma(net, lat, chunk)
    if clock:
        t0 = clock("field", t0)
    verts, faces = isosurface(sigma, lat, level, cap)
    del sigma
    if clock:
        t0 = clock("isosurface", t0)
    if largest:
        verts, faces, _ = largest_component(verts, faces, box_area_unit(lo, hi))
    if clock:
        t0 = clock("component", t0)
    nv = verts.shape[0]
    dev = verts.device
    colors, normals = torch.empty((nv, 3), device=dev), torch.empty((nv, 3), device=dev)
    if nv:
        sig, grad = torch.empty(nv, device=dev), torch.empty((nv, 3), device=dev)
        _lib.call("ia_field_fwd", verts, nv, None, net.field_desc(nv), colors, sig)
        _lib.call("ia_field_sigma_grad", verts, nv, None, net.field_desc(), sig, grad)
        _lib.call("ia_unit_negative", grad, nv, normals)
    if clock:
        clock("attributes", t0)
    return Mesh(verts, faces, normals, colors)


@torch.no_grad()
def pose(deformer, mesh, batch):
    """The canonical `mesh` in the frame of `batch` (SMPL parameters): `AvatarModel.pose_mesh`.  Positions by forward
    skinning (ia_forward_skin), normals by ia_normals_from_gradient with one "ray" per vertex; faces and colours are shared."""
    from .deformers.snarf_deformer import SNARFDeformer
    if not isinstance(deformer, SNARFDeformer):
        raise NotImplementedError("pose_mesh is implemented for the SNARF deformer (deformers.snarf_deformer.SNARFDeformer), whose "
                                  "transform grid forward skinning reads; SMPLDeformer has none")
    _lib.require_cuda(mesh.verts)
    deformer.prepare_deformer(batch, want_bbox=False)
    nv = mesh.verts.shape[0]
    dev = mesh.verts.device
    verts = mesh.verts.detach().float().contiguous()
    s2w = deformer.A.detach().reshape(-1, 4, 4)[0].float().contiguous()
    w2s = deformer.w2s.detach().reshape(4, 4).float().contiguous()
    xd, normals = torch.empty((nv, 3), device=dev), torch.zeros((nv, 3), device=dev)
    if nv:
        vJ, grid = deformer.deformer.voxel_J_cl, deformer.deformer.grid_desc()
        _lib.call("ia_forward_skin", verts, nv, vJ, grid, s2w, xd)
        # n = -M^{-T} g with g = -n_c: only the direction of the gradient enters
        idx = torch.arange(nv, dtype=torch.int32, device=dev)
        _lib.call("ia_normals_from_gradient", verts, (-mesh.normals).contiguous(), idx, nv, None, vJ, grid, w2s, nv, normals)
    out = Mesh(xd, mesh.faces, normals, mesh.colors)
    out.texture = mesh.texture          # the faces are shared, so one bake serves every pose
    return out


# ---- processing of a mesh: csrc/ia_meshops.hip --------------------------------------------------------------------------------------
MAX_CLUSTER_CELLS = 1 << 27


class Adjacency:
    """the per-vertex face and neighbour lists of (verts, faces), built once on the device (ia_mesh_adjacency_build) and read by
    `taubin` and `normals`; the lists depend on the faces and on which vertices are finite, not on the positions"""

    def __init__(self, verts, faces):
        _lib.require_cuda(verts, faces)
        self.faces = faces.detach().to(torch.int32).contiguous()
        self.nv, self.nf = int(verts.shape[0]), int(self.faces.shape[0])
        self.nbytes = int(_lib.call("ia_mesh_adjacency_workspace_bytes", self.nv, self.nf))
        if self.nbytes == 0:
            raise _lib.IAError("mesh adjacency: %d faces are more than %d" % (self.nf, (2 ** 31 - 1) // 6))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=verts.device)
        _lib.call("ia_mesh_adjacency_build", _f32(verts), self.faces, self.nv, self.nf, self.ws, self.nbytes)

    def taubin(self, verts, iters, lam, mu):
        out = torch.empty((self.nv, 3), device=verts.device)
        _lib.call("ia_mesh_taubin", _f32(verts), self.nv, self.nf, self.ws, self.nbytes, float(lam), float(mu), int(iters), out)
        return out

    def normals(self, verts):
        out = torch.empty((self.nv, 3), device=verts.device)
        _lib.call("ia_mesh_vertex_normals", _f32(verts), self.faces, self.nv, self.nf, self.ws, self.nbytes, out)
        return out


def _f32(t):
    return t.detach().reshape(-1, 3).float().contiguous()


@torch.no_grad()
def vertex_normals(verts, faces):
    """normals [nv,3] fp32 from the faces: per vertex the sum of the cross products (twice the area vectors) of its valid faces in
    ascending face order, in fp64, normalised; the zero vector for a vertex without a valid face"""
    _lib.require_cuda(verts, faces)
    return Adjacency(verts, faces).normals(verts)


@torch.no_grad()
def smooth(m, iters=10, lam=0.5, mu=-0.53):
    """Taubin smoothing of `m`: `iters` times a step lam towards the mean of the neighbours and a step mu (negative: away from it),
    which damps the lattice's staircase and the hash grid's noise without the shrinkage of plain Laplacian smoothing.  -> a Mesh
    with new positions, normals from the faces, and the faces and colours of `m`."""
    _lib.require_cuda(m.verts, m.faces)
    if int(iters) < 0:
        raise _lib.IAError("smooth: iters = %d < 0" % iters)
    adj = Adjacency(m.verts, m.faces)
    verts = adj.taubin(m.verts, iters, lam, mu)
    return Mesh(verts, m.faces, adj.normals(verts), m.colors)


def cluster_grid(lo, hi, cell):
    """cells per axis of the clustering grid, max(1, ceil((hi - lo) / cell)) in float64 on the fp32 values, as the library forms them"""
    lo, hi = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    h = np.float64(np.float32(cell))
    if not (h > 0 and np.isfinite(h)):
        raise _lib.IAError("simplify: the cell edge %r must be positive and finite" % (cell,))
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise _lib.IAError("simplify: the box is not finite")
    n = np.maximum(np.ceil((hi - lo) / h), 1.0)
    if n.prod() > MAX_CLUSTER_CELLS:
        raise _lib.IAError("simplify: a grid of %.0f x %.0f x %.0f cells is more than 2^27: enlarge the cell" % tuple(n))
    return [int(x) for x in n]


@torch.no_grad()
def simplify(m, cell, box=None, reg=1e-3):
    """Vertex clustering of `m` on a grid of edge `cell` over `box` = (lo, hi) (default: the bounding box of the finite vertices,
    which costs a second host read): one vertex per occupied cell at the minimiser of the cell's quadric pulled towards the
    members' mean with weight reg * trace, faces with two corners in one cell dropped, colours averaged, normals from the faces.
    -> a Mesh with the extra attribute `vert_cluster` [nv] int32 (the output vertex of every input vertex, -1 without one).
    One host read: the two counts."""
    _lib.require_cuda(m.verts, m.faces, m.colors)
    verts, colors = _f32(m.verts), _f32(m.colors)
    faces = m.faces.detach().to(torch.int32).contiguous()
    nv, nf = int(verts.shape[0]), int(faces.shape[0])
    dev = verts.device
    if box is None:
        if nv == 0:
            lo = hi = np.zeros(3, np.float32)
        else:
            fin = torch.isfinite(verts).all(1, keepdim=True)
            both = torch.stack([torch.where(fin, verts, torch.full_like(verts, float("inf"))).amin(0),
                                torch.where(fin, verts, torch.full_like(verts, float("-inf"))).amax(0)]).cpu().numpy()
            lo, hi = (both[0], both[1]) if np.isfinite(both).all() else (np.zeros(3, np.float32), np.zeros(3, np.float32))
    else:
        lo, hi = np.asarray(box[0], np.float32).reshape(3), np.asarray(box[1], np.float32).reshape(3)
    n = cluster_grid(lo, hi, cell)
    h = np.float32(cell)
    inv_h = np.float32(1.0 / np.float64(h))
    if not (float(reg) > 0 and np.isfinite(float(reg))):
        raise _lib.IAError("simplify: reg = %r must be positive and finite" % (reg,))
    nb = int(_lib.call("ia_mesh_cluster_workspace_bytes", nv, nf, n[0] * n[1] * n[2]))
    if nb == 0:
        raise _lib.IAError("simplify: %d faces are more than %d" % (nf, (2 ** 31 - 1) // 6))
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    geo = [float(x) for x in lo] + [float(x) for x in hi] + [float(h), float(inv_h)]
    _lib.call("ia_mesh_cluster_count", verts, faces, nv, nf, *geo, ws, nb, counts)
    nv2, nf2 = counts.tolist()
    v2, c2 = torch.empty((nv2, 3), device=dev), torch.empty((nv2, 3), device=dev)
    f2 = torch.empty((nf2, 3), dtype=torch.int32, device=dev)
    vmap = torch.empty(nv, dtype=torch.int32, device=dev)
    _lib.call("ia_mesh_cluster_emit", verts, faces, colors, nv, nf, *geo, float(reg), ws, nb, v2, nv2, f2, nf2, c2, vmap)
    out = Mesh(v2, f2, Adjacency(v2, f2).normals(v2), c2)
    out.vert_cluster = vmap
    return out
