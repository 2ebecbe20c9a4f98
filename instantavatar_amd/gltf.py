"""glTF 2.0 binary (.glb) writer for a rigged avatar mesh: one mesh, one skin of 24 joint nodes, one unlit material (a texture atlas or
vertex colours) and, optionally, a pose track as an animation.  numpy and PIL only: nothing here touches the GPU; `Mesh.to_glb`
brings the tensors to the host and calls `write_glb`.  Definitions: DESIGN.md section 4, "rigged export".

With node j's local rotation R_j, local translation J_j - J_parent (the root: J_0 + transl) and the inverse bind matrix
inv(G_j(canonical pose)), a viewer's joint matrix global(node_j) . IBM_j is the bone matrix B_j = A_j . tfs_inv_t_j of `rig.track`,
and what it draws is `rig.skin`: M = sum_k w_k B_{j_k}, x' = M [x; 1], n' = normalise(M_3x3 n)."""
import io
import json
import struct

import numpy as np

FLOAT, UBYTE, UINT = 5126, 5121, 5125
ARRAY_BUFFER, ELEMENT_ARRAY_BUFFER = 34962, 34963
_COMPONENTS = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}
_DTYPES = {FLOAT: "<f4", UBYTE: "u1", UINT: "<u4"}


class _Buffer:
    """the binary chunk under construction: every view starts on a multiple of 4 bytes"""

    def __init__(self):
        self.blob, self.views, self.accessors = bytearray(), [], []

    def view(self, data, target=None):
        self.blob.extend(b"\0" * (-len(self.blob) % 4))
        v = {"buffer": 0, "byteOffset": len(self.blob), "byteLength": len(data)}
        if target is not None:
            v["target"] = target
        self.blob.extend(data)
        self.views.append(v)
        return len(self.views) - 1

    def accessor(self, array, ctype, kind, target=None, minmax=False, normalized=False, view=None, offset=0):
        a = np.ascontiguousarray(array, _DTYPES[ctype]).reshape(-1, _COMPONENTS[kind])
        if view is None:
            view = self.view(a.tobytes(), target)
        acc = {"bufferView": view, "componentType": ctype, "count": int(a.shape[0]), "type": kind}
        if offset:
            acc["byteOffset"] = int(offset)
        if normalized:
            acc["normalized"] = True
        if minmax and a.shape[0]:
            acc["min"], acc["max"] = [float(x) for x in a.min(0)], [float(x) for x in a.max(0)]
        self.accessors.append(acc)
        return len(self.accessors) - 1


def unit_normals(normals, fallback=None):
    """[n,3] float32 unit normals: a normal that is zero or not finite is replaced by `fallback`'s (where that is neither), else by
    (0, 0, 1); normalised in float64"""
    n = np.array(normals, np.float64).reshape(-1, 3)
    length = np.linalg.norm(n, axis=1)
    bad = ~(np.isfinite(length) & (length > 0))
    if bad.any() and fallback is not None:
        n[bad] = np.asarray(fallback, np.float64).reshape(-1, 3)[bad]
        length = np.linalg.norm(n, axis=1)
        bad = ~(np.isfinite(length) & (length > 0))
    n[bad] = (0.0, 0.0, 1.0)
    length[bad] = 1.0
    return (n / length[:, None]).astype(np.float32)


def continuous_quaternions(quat):
    """quat [F,J,4] with q_f replaced by -q_f wherever dot(q_f, q_{f-1}) < 0 (q_{f-1} after its own flip), so that a LINEAR
    (spherical) interpolation between two keys takes the short way"""
    q = np.array(quat, np.float64)
    for f in range(1, q.shape[0]):
        flip = (q[f] * q[f - 1]).sum(-1) < 0
        q[f][flip] = -q[f][flip]
    return q


def pad_influences(joints, weights):
    """(joints [n,4s] uint8, weights [n,4s] float32): K padded with (joint 0, weight 0) to a multiple of four"""
    j, w = np.asarray(joints, np.uint8), np.asarray(weights, np.float32)
    n, K = j.shape
    pad = -K % 4
    return np.concatenate([j, np.zeros((n, pad), np.uint8)], 1), np.concatenate([w, np.zeros((n, pad), np.float32)], 1)


def write_glb(path, verts, faces, normals, colors8=None, corner_uv=None, image=None, fallback_normals=None, joints=None, weights=None,
              parents=None, rest_translation=None, cano_quat=None, inverse_bind=None, animation=None, fps=30):
    """Write a glTF 2.0 binary.

    verts [nv,3], faces [nf,3], normals [nv,3] (made unit length: `unit_normals` with `fallback_normals`).
    Vertex colours: colors8 [nv,3] uint8 in R, G, B order -> an indexed primitive with COLOR_0 as normalised ubyte VEC4 (alpha 255).
    Texture: corner_uv [nf,3,2] (glTF coordinates: origin top-left, i.e. (u, 1 - v) of the OBJ's `vt`) and image [T,T,3] uint8 RGB,
      row 0 on top -> the primitive is un-indexed to 3 nf vertices (the atlas has per-corner coordinates), the picture is embedded
      as a PNG buffer view and drawn through baseColorTexture.  Either way the material is unlit, metallic 0, roughness 1.
    Rig (all or none): joints [nv,K] uint8, weights [nv,K], parents [24], rest_translation [24,3], cano_quat [24,4] xyzw,
      inverse_bind [24,4,4] row-major -> JOINTS_n / WEIGHTS_n in sets of four, 24 joint nodes whose default TRS is the canonical
      pose, inverseBindMatrices column-major.
    animation: (quat [F,24,4] xyzw, root_t [F,3]) -> one rotation channel per joint and a translation channel on the root, key
      times i / fps, LINEAR interpolation, quaternion signs made continuous.  Needs the rig."""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    n = unit_normals(normals, fallback_normals)
    if n.shape != v.shape:
        raise ValueError("write_glb: %d normals for %d vertices" % (n.shape[0], v.shape[0]))
    if f.size and (f.min() < 0 or f.max() >= len(v)):
        raise ValueError("write_glb: a face index lies outside [0, %d)" % len(v))
    textured = corner_uv is not None
    if textured == (colors8 is not None) or textured != (image is not None):
        raise ValueError("write_glb: give either colors8 or corner_uv with image")
    rig = [joints, weights, parents, rest_translation, cano_quat, inverse_bind]
    rigged = joints is not None
    if any((x is not None) != rigged for x in rig):
        raise ValueError("write_glb: the rig's six arrays are given together or not at all")
    if animation is not None and not rigged:
        raise ValueError("write_glb: an animation needs the rig")
    if rigged:
        jp, wp = pad_influences(joints, weights)
        if jp.shape[0] != len(v) or wp.shape != jp.shape or jp.max(initial=0) >= 24:
            raise ValueError("write_glb: joints / weights do not fit the %d vertices and 24 joints" % len(v))
    pick = f.reshape(-1) if textured else slice(None)            # un-index: one vertex per face corner
    buf = _Buffer()
    attributes = {"POSITION": buf.accessor(v[pick], FLOAT, "VEC3", ARRAY_BUFFER, minmax=True),
                  "NORMAL": buf.accessor(n[pick], FLOAT, "VEC3", ARRAY_BUFFER)}
    primitive = {"attributes": attributes, "material": 0, "mode": 4}
    material = {"pbrMetallicRoughness": {"metallicFactor": 0.0, "roughnessFactor": 1.0}, "extensions": {"KHR_materials_unlit": {}}}
    doc = {"asset": {"version": "2.0", "generator": "instantavatar_amd"}, "extensionsUsed": ["KHR_materials_unlit"]}
    if textured:
        uv = np.asarray(corner_uv, np.float32)
        if uv.shape != (len(f), 3, 2):
            raise ValueError("write_glb: corner_uv %r for %d faces" % (uv.shape, len(f)))
        attributes["TEXCOORD_0"] = buf.accessor(uv.reshape(-1, 2), FLOAT, "VEC2", ARRAY_BUFFER)
    else:
        c = np.asarray(colors8, np.uint8).reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError("write_glb: %d colours for %d vertices" % (len(c), len(v)))
        rgba = np.concatenate([c, np.full((len(c), 1), 255, np.uint8)], 1)
        attributes["COLOR_0"] = buf.accessor(rgba, UBYTE, "VEC4", ARRAY_BUFFER, normalized=True)
        primitive["indices"] = buf.accessor(f.reshape(-1), UINT, "SCALAR", ELEMENT_ARRAY_BUFFER)
    if rigged:
        for s in range(jp.shape[1] // 4):
            attributes["JOINTS_%d" % s] = buf.accessor(jp[pick, 4 * s:4 * s + 4], UBYTE, "VEC4", ARRAY_BUFFER)
            attributes["WEIGHTS_%d" % s] = buf.accessor(wp[pick, 4 * s:4 * s + 4], FLOAT, "VEC4", ARRAY_BUFFER)
    if textured:
        from PIL import Image
        png = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(np.asarray(image, np.uint8)), "RGB").save(png, format="PNG")
        doc["images"] = [{"bufferView": buf.view(png.getvalue()), "mimeType": "image/png"}]
        doc["samplers"] = [{"magFilter": 9729, "minFilter": 9729, "wrapS": 33071, "wrapT": 33071}]      # LINEAR, CLAMP_TO_EDGE: no mip levels
        doc["textures"] = [{"sampler": 0, "source": 0}]
        material["pbrMetallicRoughness"]["baseColorTexture"] = {"index": 0}
    doc["materials"] = [material]
    doc["meshes"] = [{"primitives": [primitive]}]
    if not rigged:
        doc["nodes"] = [{"mesh": 0, "name": "avatar"}]
        doc["scenes"] = [{"nodes": [0]}]
    else:
        par = np.asarray(parents, np.int64).reshape(24)
        rest, q0 = np.asarray(rest_translation, np.float64).reshape(24, 3), np.asarray(cano_quat, np.float64).reshape(24, 4)
        nodes = []
        for j in range(24):
            node = {"name": "joint_%d" % j, "translation": [float(x) for x in rest[j]], "rotation": [float(x) for x in q0[j]]}
            kids = [int(k) for k in np.nonzero(par[1:] == j)[0] + 1]
            if kids:
                node["children"] = kids
            nodes.append(node)
        ibm = np.asarray(inverse_bind, np.float64).reshape(24, 4, 4).transpose(0, 2, 1)                   # column-major
        doc["skins"] = [{"joints": list(range(24)), "skeleton": 0, "inverseBindMatrices": buf.accessor(ibm, FLOAT, "MAT4")}]
        nodes.append({"mesh": 0, "skin": 0, "name": "avatar"})
        doc["nodes"] = nodes
        doc["scenes"] = [{"nodes": [0, 24]}]
    doc["scene"] = 0
    if animation is not None:
        quat, root_t = animation
        q = continuous_quaternions(np.asarray(quat, np.float64).reshape(-1, 24, 4))
        t = np.asarray(root_t, np.float32).reshape(-1, 3)
        F = q.shape[0]
        if F < 1 or t.shape[0] != F or not float(fps) > 0:
            raise ValueError("write_glb: the animation needs F >= 1 frames of both arrays and fps > 0")
        times = buf.accessor(np.arange(F, dtype=np.float64) / float(fps), FLOAT, "SCALAR", minmax=True)
        rot_view = buf.view(np.ascontiguousarray(q.transpose(1, 0, 2), "<f4").tobytes())                  # [24][F][4]: a joint's keys together
        samplers, channels = [], []
        for j in range(24):
            out = buf.accessor(q[:, j], FLOAT, "VEC4", view=rot_view, offset=j * F * 16)
            samplers.append({"input": times, "output": out, "interpolation": "LINEAR"})
            channels.append({"sampler": j, "target": {"node": j, "path": "rotation"}})
        samplers.append({"input": times, "output": buf.accessor(t, FLOAT, "VEC3"), "interpolation": "LINEAR"})
        channels.append({"sampler": 24, "target": {"node": 0, "path": "translation"}})
        doc["animations"] = [{"name": "track", "samplers": samplers, "channels": channels}]
    buf.blob.extend(b"\0" * (-len(buf.blob) % 4))
    doc["buffers"] = [{"byteLength": len(buf.blob)}]
    doc["bufferViews"], doc["accessors"] = buf.views, buf.accessors
    text = json.dumps(doc, separators=(",", ":")).encode("utf-8")
    text += b" " * (-len(text) % 4)
    with open(path, "wb") as out:
        out.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(text) + 8 + len(buf.blob)))
        out.write(struct.pack("<I4s", len(text), b"JSON"))
        out.write(text)
        out.write(struct.pack("<I4s", len(buf.blob), b"BIN\0"))
        out.write(bytes(buf.blob))
