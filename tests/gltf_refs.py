"""Float64 numpy references of the rigged export ("rigged export"), independent of the product: a GLB reader, a
scene evaluator (what a glTF viewer computes: node globals at a time t, joint matrices, skinned positions and normals), restatements
of the definitions (weights of a canonical point, top-K selection, bones / quaternions / root translation of a frame through
smpl_refs.tfs_fwd_ref, blended-matrix skinning), and the error bounds tests/test_gpu_rig.py holds csrc/ia_rig.hip to.  Validated on
hand-checkable cases in tests/test_cpu_gltf_refs.py.

Bounds.  u = 2^-24; a chain of n fp32 operations on non-negative terms has relative error <= n u (1 + O(u)), written G(n) below.

  index      the kernel forms g = scl (x + off) (2 roundings, |g| <= 1 inside the volume), c = ((g + 1) / 2) (size - 1) (2 more):
             |dc| <= u (size - 1) ((ops + 2) / 2 + 1) with ops = 2; the fraction c - floor(c) is exact, 1 - fraction adds u.  The
             interpolant is continuous and piecewise linear with slope <= vmax (the largest |difference| of neighbouring voxels,
             <= the largest value for values in [0, vmax]) per unit index, so an axis contributes vmax (|dc| + u).
  full       8 corner terms, each the product of three factors in [0, 1] (2 roundings) times a value (fma), accumulated: G(11) on
             non-negative terms, <= 11 u vmax.  full_bound = vmax u (11 + sum_axes ((size - 1) ((ops + 2) / 2 + 1) + 1)).
             Against torch's grid_sample on the same volume (ForwardDeformer.query_weights: (x - offset) / scale * ratio, and
             scale_kernel = 1 / scale rounded once more) both sides get ops = 4.
  top-K      kept weights w_k (each within E = full_bound of the reference), s = their fp32 sum in slot order (K - 1 additions), one
             division: |d(w_k / s)| <= (E + (w_k / s) (K E + (K - 1) u s)) / (s - K E) + u <= E (1 + K) / (s - K E) + (K + 1) u.
             Two weights closer than 2 E may be ordered either way: the index comparison skips a point whose K-th and (K+1)-th
             reference weights are that close, and accepts in slot k any joint whose reference weight is within 2 E of the k-th.
  skinning   against float64 on the same fp32 inputs: M = K fmaf, x' = 3 fmaf / products + 1 addition: (K + 4) u (1 + 2^-10) times
             (sum_k |w_k| |B_jk|) [|x|; 1].  Normal: m = M_3x3 n with error dm <= (K + 3) u (..) |n|; normalising a vector with
             componentwise error dm moves the unit vector by at most 2 sqrt(3) max(dm) / |m|, and the three products, two sums, the
             square root and the division add 4 u.
  quaternion ang: three (theta + 1e-8)^2 summed and a root, 3 u relative; dir = theta / ang 4 u; sin / cos of ang / 2 within 2 ulp
             (4 u) of an argument off by 3 u h: a component is off by <= 9 u + 3 u h <= 15.3 u for h <= 2.1, normalising adds the
             length's error (<= 18 u) times the component and one division: E_Q = 40 u.
  Rodrigues  R = I + sin K + (1 - cos) K^2 with K = hat(dir) and |dir| = 1 + e, |e| <= sqrt(3) 1e-8 / |theta|, is not the rotation
             that the joint's quaternion stores (entries differ by less than 3 |e| -- the quaternion is built on the same non-unit axis,
             so most of it cancels -- and by nothing for theta = 0): `rodrigues_gap` evaluates
             both in float64 and returns the row-sum norm of their difference, a function of the pose alone.
  bones      as smpl_refs: K_BOUND max(E32, u M) per group, E32 from the same float64 code run in float32.
"""
import json
import struct

import numpy as np

import smpl_refs as sr

U = 2.0 ** -24
E_Q = 40 * U
N_J = 24
_NP = {5120: "i1", 5121: "u1", 5122: "<i2", 5123: "<u2", 5125: "<u4", 5126: "<f4"}
_NC = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT2": 4, "MAT3": 9, "MAT4": 16}


def G(n):
    return n * U * (1 + 2.0 ** -10)


# ---- the container ---------------------------------------------------------------------------------------------------------------
def read_glb(src):
    """(json document, binary chunk) of a .glb given as a path or as bytes; checks the header and the chunk structure"""
    blob = src if isinstance(src, (bytes, bytearray)) else open(src, "rb").read()
    magic, version, total = struct.unpack_from("<4sII", blob, 0)
    assert magic == b"glTF" and version == 2 and total == len(blob) and total % 4 == 0, (magic, version, total, len(blob))
    n0, t0 = struct.unpack_from("<I4s", blob, 12)
    assert t0 == b"JSON" and n0 % 4 == 0
    doc = json.loads(bytes(blob[20:20 + n0]).decode("utf-8"))
    binary = b""
    if 20 + n0 < total:
        n1, t1 = struct.unpack_from("<I4s", blob, 20 + n0)
        assert t1 == b"BIN\0" and n1 % 4 == 0 and 20 + n0 + 8 + n1 == total
        binary = bytes(blob[28 + n0:28 + n0 + n1])
    return doc, binary


def chunk_padding(src):
    """(the JSON chunk's bytes, the BIN chunk's bytes) as stored, padding included"""
    blob = src if isinstance(src, (bytes, bytearray)) else open(src, "rb").read()
    n0 = struct.unpack_from("<I", blob, 12)[0]
    n1 = struct.unpack_from("<I", blob, 20 + n0)[0]
    return bytes(blob[20:20 + n0]), bytes(blob[28 + n0:28 + n0 + n1])


def accessor(doc, binary, index):
    """the accessor's elements as an array [count, components] of its component type (byteStride and byteOffset honoured)"""
    a = doc["accessors"][index]
    v = doc["bufferViews"][a["bufferView"]]
    dt = np.dtype(_NP[a["componentType"]])
    nc = _NC[a["type"]]
    start = v.get("byteOffset", 0) + a.get("byteOffset", 0)
    stride = v.get("byteStride", dt.itemsize * nc)
    count, tight = a["count"], dt.itemsize * nc
    assert start % dt.itemsize == 0, (index, start)
    assert count == 0 or a.get("byteOffset", 0) + (count - 1) * stride + tight <= v["byteLength"], index
    assert v.get("byteOffset", 0) + v["byteLength"] <= len(binary), index
    if stride == tight:
        return np.frombuffer(binary, dt, count * nc, start).reshape(count, nc).copy()
    return np.stack([np.frombuffer(binary, dt, nc, start + i * stride) for i in range(count)]) if count else np.empty((0, nc), dt)


# ---- the scene evaluator ---------------------------------------------------------------------------------------------------------
def quat_matrix(q):
    x, y, z, w = (np.asarray(q, np.float64) / np.linalg.norm(q)).tolist()
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def slerp(q0, q1, s):
    """spherical interpolation of the two keys AS STORED (linear when nearly parallel): no sign is changed here, so keys with a
    negative dot product go the long way round -- the writer's sign continuity is what the evaluation then shows"""
    q0, q1 = np.asarray(q0, np.float64), np.asarray(q1, np.float64)
    d = float(np.clip(q0 @ q1, -1.0, 1.0))
    if d > 0.9995:
        q = q0 + s * (q1 - q0)
        return q / np.linalg.norm(q)
    a = np.arccos(d)
    return (np.sin((1 - s) * a) * q0 + np.sin(s * a) * q1) / np.sin(a)


def animated(doc, binary, t, anim=0):
    """{(node, path): value} of animation `anim` at time t: LINEAR interpolation, slerp for rotations, clamped outside the keys"""
    out = {}
    a = doc["animations"][anim]
    for ch in a["channels"]:
        smp = a["samplers"][ch["sampler"]]
        assert smp.get("interpolation", "LINEAR") == "LINEAR"
        times = accessor(doc, binary, smp["input"])[:, 0].astype(np.float64)
        vals = accessor(doc, binary, smp["output"]).astype(np.float64)
        assert (np.diff(times) > 0).all() and len(vals) == len(times)
        if t <= times[0] or len(times) == 1:
            v = vals[0]
        elif t >= times[-1]:
            v = vals[-1]
        else:
            i = int(np.searchsorted(times, t, side="right")) - 1
            s = (t - times[i]) / (times[i + 1] - times[i])
            v = slerp(vals[i], vals[i + 1], s) if ch["target"]["path"] == "rotation" else vals[i] + s * (vals[i + 1] - vals[i])
        out[(ch["target"]["node"], ch["target"]["path"])] = v
    return out


def node_globals(doc, binary=b"", t=None, anim=0):
    """[N,4,4] global transforms of all nodes (default TRS, or the animation's values at time t)"""
    nodes = doc["nodes"]
    over = animated(doc, binary, t, anim) if t is not None else {}
    local = []
    for i, nd in enumerate(nodes):
        if "matrix" in nd:
            local.append(np.array(nd["matrix"], np.float64).reshape(4, 4).T)
            continue
        T = np.asarray(over.get((i, "translation"), nd.get("translation", (0, 0, 0))), np.float64)
        Q = np.asarray(over.get((i, "rotation"), nd.get("rotation", (0, 0, 0, 1))), np.float64)
        S = np.asarray(over.get((i, "scale"), nd.get("scale", (1, 1, 1))), np.float64)
        M = np.eye(4)
        M[:3, :3] = quat_matrix(Q) * S[None, :]
        M[:3, 3] = T
        local.append(M)
    parent = {c: i for i, nd in enumerate(nodes) for c in nd.get("children", ())}
    out = [None] * len(nodes)

    def glob(i):
        if out[i] is None:
            out[i] = local[i] if i not in parent else glob(parent[i]) @ local[i]
        return out[i]
    return np.stack([glob(i) for i in range(len(nodes))])


def joint_matrices(doc, binary, skin=0, t=None, anim=0):
    """[J,4,4] global(joint node) . inverseBindMatrix (stored column-major)"""
    sk = doc["skins"][skin]
    ibm = accessor(doc, binary, sk["inverseBindMatrices"]).astype(np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
    g = node_globals(doc, binary, t, anim)
    return np.stack([g[j] @ ibm[k] for k, j in enumerate(sk["joints"])])


def primitive(doc, binary, mesh=0, prim=0):
    """{attribute: array} of a primitive, plus "indices" ([nf,3], or arange for an un-indexed one)"""
    p = doc["meshes"][mesh]["primitives"][prim]
    out = {k: accessor(doc, binary, i) for k, i in p["attributes"].items()}
    n = len(out["POSITION"])
    out["indices"] = (accessor(doc, binary, p["indices"])[:, 0].astype(np.int64) if "indices" in p else np.arange(n)).reshape(-1, 3)
    return out


def skinned(doc, binary, t=None, anim=0):
    """(positions [n,3], normals [n,3]) of mesh 0 under skin 0 at time t, over all JOINTS_n / WEIGHTS_n sets: the blended matrix
    applied to the position, its 3 x 3 block to the normal, normalised"""
    at = primitive(doc, binary)
    jm = joint_matrices(doc, binary, 0, t, anim)
    pos, nrm = at["POSITION"].astype(np.float64), at["NORMAL"].astype(np.float64)
    M = np.zeros((len(pos), 4, 4))
    s = 0
    while "JOINTS_%d" % s in at:
        j, w = at["JOINTS_%d" % s].astype(np.int64), at["WEIGHTS_%d" % s].astype(np.float64)
        M += (w[:, :, None, None] * jm[j]).sum(1)
        s += 1
    assert s > 0
    p = np.einsum("nab,nb->na", M[:, :3, :3], pos) + M[:, :3, 3]
    m = np.einsum("nab,nb->na", M[:, :3, :3], nrm)
    return p, m / np.linalg.norm(m, axis=1, keepdims=True)


# ---- the definitions -------------------------------------------------------------------------------------------------------------
def weights_full_ref(xc, vol, offset, scale):
    """[n,C] trilinear sample of vol [C,D,H,W] at xc [n,3]: g = scale (x + offset), index ((g + 1) / 2) (size - 1) clamped to the
    volume (border padding), x <-> W, y <-> H, z <-> D"""
    vol = np.asarray(vol, np.float64)
    C, D, H, W = vol.shape
    x = np.asarray(xc, np.float64).reshape(-1, 3)
    g = np.asarray(scale, np.float64) * (x + np.asarray(offset, np.float64))
    out = np.zeros((len(x), C))
    idx = [np.clip((g[:, a] + 1) / 2 * (size - 1), 0, size - 1) for a, size in enumerate((W, H, D))]
    lo = [np.minimum(np.floor(c).astype(np.int64), size - 1) for c, size in zip(idx, (W, H, D))]
    fr = [c - l for c, l in zip(idx, lo)]
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                wt = (fr[0] if cx else 1 - fr[0]) * (fr[1] if cy else 1 - fr[1]) * (fr[2] if cz else 1 - fr[2])
                xi, yi, zi = np.minimum(lo[0] + cx, W - 1), np.minimum(lo[1] + cy, H - 1), np.minimum(lo[2] + cz, D - 1)
                out += wt[:, None] * vol[:, zi, yi, xi].T
    return out


def topk_ref(full, K):
    """-> (joints [n,K] int, weights [n,K] float64 normalised, kept [n,K] unnormalised, order [n,24]): descending, ties to the lower
    joint, a slot with weight exactly 0 names joint 0; a row that is not finite or whose kept sum is 0: joint 0 with weight 1"""
    full = np.asarray(full, np.float64)
    order = np.argsort(-np.where(np.isnan(full), -np.inf, full), axis=1, kind="stable")
    kept = np.take_along_axis(full, order[:, :K], 1)
    kept = np.where(np.isnan(kept), 0.0, kept)
    joints = np.where(kept == 0, 0, order[:, :K])
    s = np.zeros(len(full))
    for k in range(K):
        s = s + kept[:, k]
    ok = np.isfinite(full).all(1) & (s != 0) & np.isfinite(s)
    w = np.zeros_like(kept)
    w[ok] = kept[ok] / s[ok, None]
    w[~ok, 0] = 1.0
    joints[~ok] = 0
    return joints, w, kept, order


def rig_weights_ref(xc, vol, offset, scale, K):
    """the whole of ia_rig_weights: (joints, weights, full, kept, order); a point with a non-finite coordinate has full = 0 and
    joint 0 with weight 1"""
    x = np.asarray(xc, np.float64).reshape(-1, 3)
    fin = np.isfinite(x).all(1)
    full = np.zeros((len(x), np.asarray(vol).shape[0]))
    full[fin] = weights_full_ref(x[fin], vol, offset, scale)
    j, w, kept, order = topk_ref(full, K)
    j[~fin], w[~fin] = 0, 0
    w[~fin, 0] = 1
    return j, w, full, kept, order


def quaternions_ref(poses):
    """[..., 24, 4] x, y, z, w: ang = |theta + 1e-8f|, dir = theta / ang, q = normalise(dir sin(ang / 2), cos(ang / 2))"""
    th = np.asarray(poses, np.float64)
    th = th.reshape(th.shape[:-1] + (N_J, 3))
    ang = np.linalg.norm(th + np.float64(sr.EPS32), axis=-1, keepdims=True)
    q = np.concatenate([th / ang * np.sin(ang / 2), np.cos(ang / 2)], -1)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def track_ref(joints_rest, parents, poses, transl, tfs_inv_t, dtype=np.float64):
    """ia_rig_track over F frames: dict bones [F,24,4,4] = A . tfs_inv_t, quat [F,24,4], root_t [F,3], A [F,24,4,4] (tfs_fwd_ref's)"""
    poses = np.asarray(poses).reshape(-1, 72)
    F = len(poses)
    tr = np.zeros((F, 3), np.float32) if transl is None else np.asarray(transl).reshape(F, 3)
    A = np.stack([sr.tfs_fwd_ref(joints_rest, parents, poses[f], tr[f], tfs_inv_t, dtype)["A"] for f in range(F)])
    B = np.asarray(tfs_inv_t).reshape(N_J, 4, 4).astype(dtype)
    J0 = np.asarray(joints_rest).reshape(N_J, 3)[0].astype(dtype)
    return dict(bones=sr._mm(A, B[None]), quat=quaternions_ref(poses), root_t=J0[None] + tr.astype(dtype), A=A)


def track_bound(joints_rest, parents, poses, transl, tfs_inv_t):
    """{group: (float64 reference, allowance)} for bones.R, bones.t (K_BOUND max(E32, u M), as smpl_refs._allow), quat (E_Q) and
    root_t (one addition: u times the magnitude)"""
    r64 = track_ref(joints_rest, parents, poses, transl, tfs_inv_t)
    r32 = track_ref(joints_rest, parents, poses, transl, tfs_inv_t, np.float32)
    out = {}
    for name, sl in (("bones.R", (Ellipsis, slice(0, 3), slice(0, 3))), ("bones.t", (Ellipsis, slice(0, 3), 3))):
        ref = r64["bones"][sl]
        e32 = float(np.abs(r32["bones"][sl].astype(np.float64) - ref).max())
        out[name] = (ref, sr.K_BOUND * max(e32, U * float(np.abs(ref).max())))
    out["bones.row3"] = (r64["bones"][..., 3, :], 0.0)
    out["quat"] = (r64["quat"], E_Q)
    out["root_t"] = (r64["root_t"], 2 * U * float(np.abs(r64["root_t"]).max() + 1e-30))
    return out


def lbs_ref(verts, normals, joints, weights, bones):
    """(positions [F,n,3], normals [F,n,3] or None): M = sum_k w_k B_jk, x' = M [x; 1], n' = normalise(M_3x3 n), zero where that is
    zero or not finite"""
    x, w = np.asarray(verts, np.float64), np.asarray(weights, np.float64)
    B = np.asarray(bones, np.float64).reshape(-1, N_J, 4, 4)
    j = np.minimum(np.asarray(joints, np.int64), N_J - 1)
    M = np.einsum("nk,fnkab->fnab", w, B[:, j])
    p = np.einsum("fnab,nb->fna", M[..., :3, :3], x) + M[..., :3, 3]
    if normals is None:
        return p, None
    m = np.einsum("fnab,nb->fna", M[..., :3, :3], np.asarray(normals, np.float64))
    length = np.linalg.norm(m, axis=-1, keepdims=True)
    ok = np.isfinite(length) & (length > 0)
    return p, np.where(ok, m / np.where(ok, length, 1.0), 0.0)


# ---- the bounds --------------------------------------------------------------------------------------------------------------------
def index_error(size, ops=2):
    return U * (size - 1) * ((ops + 2) / 2.0 + 1)


def full_bound(dims, vmax=1.0, ops=2):
    """allowance of one sampled weight on a volume of dims (D, H, W) with values in [0, vmax]"""
    return vmax * (G(11) + sum(index_error(s, ops) + U for s in dims))


def topk_weight_bound(E, kept_sum, K):
    """[n] allowance of a normalised weight, from the reference's kept sum s"""
    s = np.asarray(kept_sum, np.float64)
    return E * (1 + K) / np.maximum(s - K * E, 1e-300) + (K + 1) * U


def skin_bound(verts, normals, joints, weights, bones):
    """(allowance [F,n,3] of the positions, allowance [F,n,1] of the normals or None)"""
    x, w = np.abs(np.asarray(verts, np.float64)), np.abs(np.asarray(weights, np.float64))
    B = np.asarray(bones, np.float64).reshape(-1, N_J, 4, 4)
    j = np.minimum(np.asarray(joints, np.int64), N_J - 1)
    K = w.shape[1]
    Mabs = np.einsum("nk,fnkab->fnab", w, np.abs(B[:, j]))
    pos = G(K + 4) * (np.einsum("fnab,nb->fna", Mabs[..., :3, :3], x) + Mabs[..., :3, 3])
    if normals is None:
        return pos, None
    nn = np.asarray(normals, np.float64)
    dm = G(K + 3) * np.einsum("fnab,nb->fna", Mabs[..., :3, :3], np.abs(nn))
    m = np.einsum("fnab,nb->fna", np.einsum("nk,fnkab->fnab", np.asarray(weights, np.float64), B[:, j])[..., :3, :3], nn)
    length = np.linalg.norm(m, axis=-1, keepdims=True)
    return pos, 2 * np.sqrt(3.0) * dm.max(-1, keepdims=True) / np.maximum(length, 1e-300) + 4 * U


def rodrigues_gap(poses):
    """[F,24] row-sum norm of (Rodrigues as the project defines it) - (the rotation matrix of the joint's quaternion), both in
    float64: the distance between two definitions, a function of the pose alone"""
    th = np.asarray(poses, np.float64).reshape(-1, 72)
    out = np.zeros((len(th), N_J))
    for f in range(len(th)):
        R = sr._rodrigues(th[f], np.float64)["R"]
        Q = np.stack([quat_matrix(q) for q in quaternions_ref(th[f])])
        out[f] = np.abs(R - Q).sum(-1).max(-1)
    return out


def chain_sum(per_joint, parents):
    """[..., 24] -> the largest sum of `per_joint` over a joint and its ancestors"""
    p = np.asarray(parents, np.int64)
    acc = np.array(per_joint, np.float64)
    for j in range(1, N_J):
        acc[..., j] = acc[..., j] + acc[..., p[j]]
    return acc.max(-1)


# ---- seeded inputs shared by tests/test_gpu_rig.py and tests/test_cpu_gltf_refs.py ---------------------------------------------------
WEIGHT_DIMS = (2, 3, 5)                                       # D, H, W
WEIGHT_SIZES = (1, 63, 64, 65, 257)
WEIGHT_KS = (1, 4, 8, 24)
WEIGHT_OFFSET = np.array([0.1, -0.2, 0.05], np.float32)
WEIGHT_SCALE = np.array([0.8, 1.1, 2.0], np.float32)


def weight_volume():
    """[24,2,3,5] fp32 in [0, 1)"""
    return np.random.default_rng(7).random((N_J,) + WEIGHT_DIMS, np.float32)


def tie_volume():
    """0.25 on joints 3, 7, 11 and 20 at every voxel, 0 elsewhere: with K = 2 the rule picks joints 3 and 7, 0.5 each, exactly"""
    v = np.zeros((N_J,) + WEIGHT_DIMS, np.float32)
    v[[3, 7, 11, 20]] = 0.25
    return v


def weight_points(n):
    """[n,3] fp32: a third inside the volume, a third with one coordinate on a face of it (g = -1 or 1 up to fp32 rounding), a
    third outside (|g| up to 1.6 on every axis)"""
    rng = np.random.default_rng(100 + n)
    g = rng.uniform(-1, 1, (n, 3))
    k = np.arange(n)
    face = k % 3 == 1
    g[face, rng.integers(0, 3, n)[face]] = rng.choice([-1.0, 1.0], n)[face]
    out = k % 3 == 2
    g[out] = rng.uniform(-1.6, 1.6, (int(out.sum()), 3))
    return (g / WEIGHT_SCALE.astype(np.float64) - WEIGHT_OFFSET.astype(np.float64)).astype(np.float32)


def index_skips(kept, order, full, K, E):
    """[n] bool: the points whose index comparison is skipped -- the K-th and the (K+1)-th largest reference weights are closer
    than 2 E (with K = 24 there is no (K+1)-th: nothing is skipped)"""
    if K >= full.shape[1]:
        return np.zeros(len(full), bool)
    nxt = np.take_along_axis(full, order[:, K:K + 1], 1)[:, 0]
    return kept[:, K - 1] - nxt < 2 * E


# ---- the invariant: a rig with all 24 influences against the transform grid's skinning ---------------------------------------------
def _max_allow(bounds, names):
    return max(bounds[k][1] for k in names)


def invariant_terms(verts, full, joints_rest, parents, pose, transl, tfs_inv_t):
    """What separates `pose_mesh` (ia_smpl_tfs -> ia_precompute -> ia_forward_skin) from the exact linear-blend skinning with the
    reference weights `full` [n,24] (float64, from weights_full_ref) normalised to sum 1, for one frame.  Both kernels form the
    fractional voxel coordinates of a vertex with the same fp32 operations (g = scl (x + off), ((g + 1) / 2) (size - 1), floor), so
    inside the volume the corner weights start from the same bits and no index term enters.  All in the infinity norm:

      pose    voxel_J = 24 fmaf of w tfs, 8 corner terms (2 products + fmaf each: G(11)), J [x; 1] (G(4)), all on the root-frame
              magnitude mag_root = max (sum_j w_j |tfs_j|) [|x|; 1]; tfs itself within smpl_refs' allowance (a_R on 3 |x|, a_t);
              then s2w: G(4) on (S mag_root + |t|) with S = the largest row sum of |s2w_R|, and s2w within A's allowance
      renorm  pose_mesh blends with the weights as sampled, the rig divides them by their sum s: |s - 1| mag_world
      rig     weights G(11) relative (non-negative terms), their sum 23 additions, one division; M = 24 fmaf, x' G(4): G(64) on
              mag_world = max (sum_j w_j |B_j|) [|x|; 1]; the bones within track_bound's allowance
    -> dict(pose, renorm, rig, mag_world, xmax, bones_allow)"""
    x = np.abs(np.asarray(verts, np.float64))
    s = np.asarray(full, np.float64).sum(1)
    w = np.asarray(full, np.float64) / s[:, None]
    args = (joints_rest, parents, pose, transl, tfs_inv_t)
    r = sr.tfs_fwd_ref(*args)
    b = sr._fwd_case("tfs", sr.tfs_fwd_ref, args)
    tb = track_bound(joints_rest, parents, np.asarray(pose)[None], None if transl is None else np.asarray(transl)[None], tfs_inv_t)
    bones = tb["bones.R"][0][0], tb["bones.t"][0][0]
    xh = np.concatenate([x, np.ones((len(x), 1))], 1)
    mag_root = float(np.einsum("nj,jab,nb->na", w, np.abs(r["tfs"][:, :3, :]), xh).max())
    Babs = np.concatenate([np.abs(bones[0]), np.abs(bones[1])[..., None]], -1)
    mag_world = float(np.einsum("nj,jab,nb->na", w, Babs, xh).max())
    S, ts, xmax = float(np.abs(r["A"][0, :3, :3]).sum(1).max()), float(np.abs(r["A"][0, :3, 3]).max()), float(x.max())
    pose_err = (S * (G(24 + 11 + 4) * mag_root + 3 * b["tfs.R"][1] * xmax + b["tfs.t"][1]) + G(4) * (S * mag_root + ts)
                + 3 * b["A.R"][1] * mag_root + b["A.t"][1])
    bones_allow = 3 * tb["bones.R"][1] * xmax + tb["bones.t"][1]
    return dict(pose=pose_err, renorm=float(np.abs(s - 1).max()) * mag_world, rig=G(64) * mag_world + bones_allow,
                mag_world=mag_world, xmax=xmax, bones_allow=bones_allow)


def glb_terms(verts, joints, weights, inverse_bind, rest_translation, parents, poses):
    """[F] what separates the file evaluated in float64 from the exact skinning with the bones of the definition, in the infinity
    norm.  A joint's stored quaternion is within E_Q per component of the definition's; the rotation's entries are sums of
    products 2 q_a q_b (the evaluator normalises q), off by <= 4 sqrt(2) E_Q each, 12 sqrt(2) E_Q per row; the quaternion's
    rotation is `rodrigues_gap` away from the Rodrigues matrix the bones are built on.  A perturbation rho of joint a's rotation
    moves whatever hangs below a by <= rho times its distance from a, which rigid bones keep below `reach` = the longest
    root-to-leaf path of rest offsets + the largest canonical distance between a vertex and a joint that influences it; the
    perturbations of a joint and its ancestors add up (`chain_sum`).  Translations and inverse bind matrices are rounded to fp32
    once: u on the chain's offsets and on |IBM| [|x|; 1]."""
    x = np.asarray(verts, np.float64)
    ibm = np.asarray(inverse_bind, np.float64).reshape(N_J, 4, 4)
    jpos = np.linalg.inv(ibm)[:, :3, 3]                                   # the canonical joints
    rest = np.abs(np.asarray(rest_translation, np.float64)).max(1)
    rest[0] = 0
    path = chain_sum(rest, parents)
    j, w = np.asarray(joints, np.int64), np.asarray(weights, np.float64)
    dist = np.where(w > 0, np.abs(x[:, None, :] - jpos[j]).max(-1), 0.0).max()
    reach = path + float(dist)
    rho = 12 * np.sqrt(2.0) * E_Q + rodrigues_gap(poses)
    xh = np.concatenate([np.abs(x).max(0), [1.0]])
    stored = U * (path + float((np.abs(ibm[:, :3, :]) @ xh).max()))
    return reach * chain_sum(rho, parents) + stored
