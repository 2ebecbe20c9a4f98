"""float64 numpy references of the surface-normal pass (include/instantavatar_hip_normals.h),
built on tests/backward_refs.py's hash-grid restatement.  Shared by tests/test_gpu_normals.py and tests/test_cpu_normals.py."""
import numpy as np

import backward_refs as br

#: test 1 (sigma gradient): points, seed, and the share of points that may be left out
SG_POINTS, SG_SEED, SG_MAX_EXCLUDED = 4096, 42, 0.05


# ---- the synthetic field ----------------------------------------------------------------------------------------------
def synthetic_field(n_levels, seed=42, device="cpu"):
    """The field `pipeline.build_synthetic_model(seed)` loads, without the deformer (whose set-up needs the GPU): canonical
    joints and bounding box from the synthetic body posed with the canonical pose -> `synthetic.make_field` -> (field dict,
    Levels)."""
    import torch
    from instantavatar_amd import synthetic as syn
    from instantavatar_amd.deformers.smplx import SMPL
    from instantavatar_amd.deformers.snarf_deformer import get_bbox_from_smpl
    smpl = SMPL.from_dict(syn.make_body(seed)).to(device)
    betas = torch.zeros(1, 10, device=device)
    pose = torch.as_tensor(syn.cano_pose("A_pose"), device=device)[None]
    rest = smpl(betas=betas, body_pose=pose)
    bbox = get_bbox_from_smpl(rest.vertices.detach()).cpu().numpy()
    fp = syn.make_field(rest.joints[0].detach().cpu().numpy(), bbox, seed=seed, n_levels=n_levels)
    return fp, levels_of(fp)


def levels_of(fp):
    return br.Levels(fp["level_scale"], fp["level_res"], fp["level_offset"])


def box_points(fp, n=SG_POINTS, seed=SG_SEED):
    """n points uniform in the field's box (fp32)"""
    rng = np.random.RandomState(seed)
    u = rng.uniform(0.0, 1.0, (n, 3))
    return ((u - 0.5) * fp["scale"].astype(np.float64) + fp["center"].astype(np.float64)).astype(np.float32)


# ---- sigma and its gradient -------------------------------------------------------------------------------------------
def sigma_grad_ref(x, fp, lv):
    """float64 sigma network on the fp16 table and fp16 weights: features by exact trilinear interpolation, layer-1
    pre-activations h1 [V,64], mask = h1 > 0 (from ITS OWN pre-activations), sigma = W2[0] relu(h1),
    grad = d sigma / d x [V,3] through `hashgrid_bwd_ref`'s dx (analytic derivative of the interpolation, 0 on a clamped axis)."""
    x = np.asarray(x, np.float32)
    feat, _ = br.hashgrid_fwd_ref(x, fp["center"], fp["scale"], lv, fp["table"])
    W1 = np.asarray(fp["sig_w1"]).astype(np.float64)             # [64, 2L]
    w2 = np.asarray(fp["sig_w2"]).astype(np.float64)[0]          # [64]
    h1 = feat @ W1.T
    mask = h1 > 0
    sigma = (np.where(mask, h1, 0.0) * w2[None]).sum(1)
    dF = (mask * w2[None]) @ W1                                   # [V, 2L]
    dx = br.hashgrid_bwd_ref(x, None, fp["center"], fp["scale"], lv, dF, table=fp["table"])["dx"]
    return dict(sigma=sigma, grad=dx, h1=h1)


def sigma_grad_excluded(x, fp, lv, h1):
    """the rows test 1 leaves out: `near_cell_face` (one rounding of the normalisation may move the point into the neighbouring
    cell), or a layer-1 pre-activation whose magnitude is below the half rounding step of its value (the forward's half-rounded
    hidden unit is then zero while the float64 one is not)"""
    face = br.near_cell_face(x, fp["center"], fp["scale"], lv)
    a = np.abs(h1)
    with np.errstate(over="ignore"):
        step = np.spacing(a.astype(np.float16)).astype(np.float64)
    tiny = ((a > 0) & (a < step)).any(1)
    return face | tiny


# ---- surface points ---------------------------------------------------------------------------------------------------
def surface_points_ref(o, d, depth, alpha):
    """(points [n,3] float64, ray index [n]) of the pixels with alpha >= 0.5 and a finite fp32 depth / alpha, in ray order;
    t is the fp32 quotient (what the kernel forms), o + t d is evaluated exactly"""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    depth, alpha = np.asarray(depth, np.float32).reshape(-1), np.asarray(alpha, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        t = (depth / alpha).astype(np.float32)
        hit = (alpha >= np.float32(0.5)) & np.isfinite(t)
    idx = np.nonzero(hit)[0]
    pts = o[idx].astype(np.float64) + t[idx].astype(np.float64)[:, None] * d[idx].astype(np.float64)
    return pts, idx.astype(np.int32)


# ---- normals from gradients -------------------------------------------------------------------------------------------
def blend_M_ref(root, voxel_J, grid):
    """linear part [n,3,3] of the trilinear blend of voxel_J [D,H,W,12] at the roots (grid_sample, align_corners, corners
    outside the grid with weight 0), float64.  grid: dict(D, H, W, offset [3], scale [3]).  The normalised coordinate and the
    source index are formed in fp32 as the kernel forms them (which cell a root falls into is decided there)."""
    root = np.asarray(root, np.float32)
    D, H, W = grid["D"], grid["H"], grid["W"]
    off, scl = np.asarray(grid["offset"], np.float32), np.asarray(grid["scale"], np.float32)
    gn = (scl[None] * (root + off[None]).astype(np.float32)).astype(np.float32)        # x -> W, y -> H, z -> D
    n = len(root)
    M = np.zeros((n, 3, 3))
    sizes = (W, H, D)
    with np.errstate(all="ignore"):
        ix = [(((gn[:, a] + np.float32(1)) / np.float32(2)).astype(np.float32) * np.float32(sizes[a] - 1)).astype(np.float32) for a in range(3)]
    ix = [np.where(np.abs(v) <= 2147483648.0, v, np.float32(-100.0)).astype(np.float32) for v in ix]
    i0 = [np.floor(v).astype(np.int64) for v in ix]
    fr = [v.astype(np.float64) - f for v, f in zip(ix, i0)]
    vJ = np.asarray(voxel_J, np.float64).reshape(D, H, W, 3, 4)[..., :3]
    for c in range(8):
        cx, cy, cz = i0[0] + (c & 1), i0[1] + ((c >> 1) & 1), i0[2] + ((c >> 2) & 1)
        wx = fr[0] if c & 1 else 1 - fr[0]
        wy = fr[1] if c & 2 else 1 - fr[1]
        wz = fr[2] if c & 4 else 1 - fr[2]
        ok = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H) & (cz >= 0) & (cz < D)
        w = np.where(ok, wx * wy * wz, 0.0)
        M += w[:, None, None] * vJ[np.clip(cz, 0, D - 1), np.clip(cy, 0, H - 1), np.clip(cx, 0, W - 1)]
    return M


def normals_ref(root, grad, voxel_J, grid, w2s):
    """n = -M^{-T} g / |M^{-T} g| rotated with the transpose of w2s' rotation [n,3] float64; zero where g = 0 or M is
    singular.  Also returns |det M| (the tests treat a blend that is singular only up to rounding as undecided)."""
    M = blend_M_ref(root, voxel_J, grid)
    g = np.asarray(grad, np.float64)
    r0, r1, r2 = M[:, 0], M[:, 1], M[:, 2]
    C = np.stack([np.cross(r1, r2), np.cross(r2, r0), np.cross(r0, r1)], 1)         # cof(M) = det(M) M^{-T}
    det = (r0 * C[:, 0]).sum(1)
    v = -np.sign(det)[:, None] * np.einsum("nij,nj->ni", C, g)
    u = v @ np.asarray(w2s, np.float64)[:3, :3]                                     # R^T v, row-vector form
    ln = np.linalg.norm(u, axis=1)
    ok = (det != 0) & (ln > 0) & np.isfinite(ln)
    out = np.where(ok[:, None], u / np.where(ok, ln, 1.0)[:, None], 0.0)
    return out, np.abs(det)
