"""The standard rig of a canonical mesh (csrc/ia_rig.hip, include/instantavatar_hip_rig.h; definition in DESIGN.md section 4, "rigged
export"): per-vertex joint indices and weights sampled from the deformer's skinning-weight volume (`build`), the bone matrices,
joint quaternions and root translations of a whole pose track (`track`), and linear-blend skinning of the mesh over every frame of
the track in one launch (`skin`).  `AvatarModel.rig_mesh` / `AvatarModel.skin_rigged` are the public entry points, `Mesh.to_glb`
writes the rig into a glTF file (`gltf.write_glb`).

`AvatarModel.pose_mesh` skins through the per-frame grid of blended transforms, voxel_J = sum_j w_j tfs_j per voxel; trilinear
interpolation is linear, so it equals linear-blend skinning with the trilinearly interpolated weights: a rig with all 24 influences
reproduces it up to rounding (inside the weight volume: outside it the transform grid is padded with zeros, the weights with their
border values), one with fewer deviates by what `deviation` reports.  SNARF deformer only; there is no CPU route."""
import numpy as np
import torch

from . import _lib

N_JOINTS = 24


class Rig:
    """joints [n,K] uint8 and weights [n,K] fp32 on the device; host arrays (float64, computed once): parents [24] int,
    rest_translation [24,3] (node j's local translation J_j - J_parent, the root's J_0), cano_quat [24,4] (the canonical pose's local
    rotations, xyzw), inverse_bind [24,4,4] (inv(G_j(canonical pose)) = T(-J_j) . tfs_inv_t_j, row-major)."""

    def __init__(self, joints, weights, parents, rest_translation, cano_quat, inverse_bind):
        self.joints, self.weights, self.parents = joints, weights, parents
        self.rest_translation, self.cano_quat, self.inverse_bind = rest_translation, cano_quat, inverse_bind

    @property
    def influences(self):
        return int(self.joints.shape[1])


def quaternions(pose72):
    """[..., 24, 4] float64 unit quaternions (x, y, z, w) of axis-angle poses [..., 72], from Rodrigues as the project defines it:
    ang = |theta + 1e-8|, dir = theta / ang, q = normalise(dir sin(ang / 2), cos(ang / 2))"""
    th = np.asarray(pose72, np.float64)
    th = th.reshape(th.shape[:-1] + (N_JOINTS, 3))
    ang = np.linalg.norm(th + 1e-8, axis=-1, keepdims=True)
    q = np.concatenate([th / ang * np.sin(ang / 2), np.cos(ang / 2)], -1)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _snarf(deformer, who):
    from .deformers.snarf_deformer import SNARFDeformer
    if not isinstance(deformer, SNARFDeformer):
        raise NotImplementedError("%s is implemented for the SNARF deformer (deformers.snarf_deformer.SNARFDeformer), whose skinning-"
                                  "weight volume it samples; SMPLDeformer has none" % who)
    if not deformer.initialized:
        raise _lib.IAError("%s: the deformer is not initialised (no canonical pose, no weight volume yet)" % who)
    return deformer


def cano_pose72(deformer):
    """the canonical pose of `SNARFDeformer.initialize` as a [72] float64 host vector (global orientation zero)"""
    from .deformers import _opt
    from .deformers.snarf_deformer import get_predefined_rest_pose
    cano = _opt.get(deformer.opt, "cano_pose", "A_pose")
    pose = np.zeros(72)
    if isinstance(cano, str):
        pose[3:] = get_predefined_rest_pose(cano, device="cpu").reshape(69).double().numpy()
    else:
        for slot, val in zip((2, 5, 47, 50), cano):
            pose[3 + slot] = float(val)
    return pose


@torch.no_grad()
def weights(deformer, points, influences=4, full=False):
    """(joints [n,K] uint8, weights [n,K] fp32[, full [n,24] fp32]) of canonical points [n,3]: ia_rig_weights on the channel-last
    copy of the weight volume"""
    deformer = _snarf(deformer, "rig.weights")
    _lib.require_cuda(points)
    K = int(influences)
    if not 1 <= K <= N_JOINTS:
        raise _lib.IAError("rig: influences = %d outside [1, %d]" % (K, N_JOINTS))
    pts = points.detach().reshape(-1, 3).float().contiguous()
    n, dev = pts.shape[0], pts.device
    fd = deformer.deformer
    j, w = torch.empty((n, K), dtype=torch.uint8, device=dev), torch.empty((n, K), device=dev)
    f = torch.empty((n, N_JOINTS), device=dev) if full else None
    _lib.call("ia_rig_weights", pts, n, fd.lbs_voxel_channel_last(), 1, fd.grid_desc(), K, j, w, f)
    return (j, w, f) if full else (j, w)


@torch.no_grad()
def build(deformer, mesh, influences=4):
    """The rig of the canonical `mesh` -> Rig.  Two small host reads (tfs_inv_t, the rest joints) for the float64 constants."""
    deformer = _snarf(deformer, "rig.build")
    j, w = weights(deformer, mesh.verts, influences)
    J = deformer._joints_rest.detach().reshape(N_JOINTS, 3).double().cpu().numpy()
    B = deformer.tfs_inv_t.detach().reshape(N_JOINTS, 4, 4).double().cpu().numpy()
    parents = deformer._parents32.detach().cpu().numpy().astype(np.int64)
    rest = J.copy()
    rest[1:] = J[1:] - J[parents[1:]]
    ibm = B.copy()
    ibm[:, :3, 3] -= J                               # T(-J_j) . tfs_inv_t_j
    return Rig(j, w, parents, rest, quaternions(cano_pose72(deformer)), ibm)


@torch.no_grad()
def track(deformer, poses72, transl=None):
    """(bones [F,24,4,4], quat [F,24,4], root_t [F,3]) on the device for poses [F,72] and translations [F,3] (None: 0): ia_rig_track,
    one launch for the whole track"""
    deformer = _snarf(deformer, "rig.track")
    _lib.require_cuda(poses72, transl)
    poses = poses72.detach().reshape(-1, 72).float().contiguous()
    F, dev = poses.shape[0], poses.device
    tr = None if transl is None else transl.detach().reshape(-1, 3).float().contiguous()
    if tr is not None and tr.shape[0] != F:
        raise _lib.IAError("rig.track: %d translations for %d poses" % (tr.shape[0], F))
    bones, quat, root = torch.empty((F, N_JOINTS, 4, 4), device=dev), torch.empty((F, N_JOINTS, 4), device=dev), torch.empty((F, 3), device=dev)
    _lib.call("ia_rig_track", deformer._joints_rest, deformer._parents32, poses, tr, deformer.tfs_inv_t, F, bones, quat, root)
    return bones, quat, root


@torch.no_grad()
def skin(rig, mesh, bones, chunk=None):
    """(verts [F,n,3], normals [F,n,3]) of `mesh` under the bone matrices `bones` [F,24,4,4]: ia_rig_skin.  chunk=None: one launch,
    the results stay on the device (24 F n bytes).  chunk=c: c frames per launch through two device buffers of c frames, the results
    are collected in host memory -- for tracks whose skinned frames do not fit on the device at once; the values are the same."""
    _lib.require_cuda(mesh.verts, mesh.normals, bones, rig.joints, rig.weights)
    verts, nrm = mesh.verts.detach().reshape(-1, 3).float().contiguous(), mesh.normals.detach().reshape(-1, 3).float().contiguous()
    n, K, dev = verts.shape[0], rig.influences, verts.device
    if rig.joints.shape[0] != n or rig.weights.shape != rig.joints.shape:
        raise _lib.IAError("rig.skin: the rig has %d vertices, the mesh %d" % (rig.joints.shape[0], n))
    b = bones.detach().reshape(-1, N_JOINTS, 4, 4).float().contiguous()
    F = b.shape[0]
    if chunk is None:
        xv, xn = torch.empty((F, n, 3), device=dev), torch.empty((F, n, 3), device=dev)
        _lib.call("ia_rig_skin", verts, nrm, n, rig.joints, rig.weights, K, b, F, xv, xn)
        return xv, xn
    c = int(chunk)
    if c < 1:
        raise _lib.IAError("rig.skin: chunk = %d < 1" % c)
    xv, xn = torch.empty((F, n, 3)), torch.empty((F, n, 3))
    dv, dn = torch.empty((min(c, F), n, 3), device=dev), torch.empty((min(c, F), n, 3), device=dev)
    for first in range(0, F, c):
        count = min(c, F - first)
        _lib.call("ia_rig_skin", verts, nrm, n, rig.joints, rig.weights, K, b[first:first + count], count, dv, dn)
        xv[first:first + count].copy_(dv[:count])
        xn[first:first + count].copy_(dn[:count])
    return xv, xn


@torch.no_grad()
def deviation(a, b):
    """(max [F], mean [F]) of the distances between corresponding points of a and b [F,n,3] (a report: plain tensor operations)"""
    d = (a.double() - b.double().to(a.device)).norm(dim=-1)
    if d.shape[-1] == 0:
        return d.new_zeros(d.shape[0]), d.new_zeros(d.shape[0])
    return d.amax(-1), d.mean(-1)
