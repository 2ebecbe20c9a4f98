"""tests/gltf_refs.py, the float64 reference of the rigged export ("rigged export"), is itself checked here on
cases that can be verified by hand: a two-bone GLB assembled byte by byte, the weight sampling against torch's grid_sample, an exact
tie.  Then `gltf.write_glb` on numpy inputs (structure, round trip, the textured layout, quaternion signs), the binding table of
include/instantavatar_hip_rig.h and what is refused before anything is launched.  No GPU."""
import json
import os
import struct

import numpy as np
import pytest
import torch

import gltf_refs as gr
import smpl_refs as sr
import texture_refs as tx

NAMES = ["ia_rig_skin", "ia_rig_track", "ia_rig_weights"]


# ---- the reader and the evaluator ----------------------------------------------------------------------------------------------------
def _two_bone_glb():
    """joint 0 at the origin, joint 1 one unit up; three vertices: on joint 0, on joint 1 (two units up), and half / half through a
    SECOND influence set; joint 1 turns by 90 degrees about z between t = 0 and t = 1"""
    f32 = lambda *v: struct.pack("<%df" % len(v), *v)
    u8 = lambda *v: bytes(v)
    parts, views = [], []

    def add(data):
        off = sum(len(p) for p in parts)
        parts.append(data + b"\0" * (-len(data) % 4))
        views.append({"buffer": 0, "byteOffset": off, "byteLength": len(data)})
        return len(views) - 1
    h = np.sqrt(0.5)
    v_pos = add(f32(0, 0, 0, 0, 2, 0, 0, 1.5, 0))
    v_nrm = add(f32(1, 0, 0, 1, 0, 0, 0, 1, 0))
    v_j0 = add(u8(0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0))
    v_w0 = add(f32(1, 0, 0, 0, 1, 0, 0, 0, 0.5, 0, 0, 0))
    v_j1 = add(u8(0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0))
    v_w1 = add(f32(0, 0, 0, 0, 0, 0, 0, 0, 0, 0.5, 0, 0))
    v_idx = add(struct.pack("<3H", 0, 1, 2))
    ibm = [np.eye(4), np.eye(4)]
    ibm[1][1, 3] = -1
    v_ibm = add(b"".join(f32(*m.T.reshape(-1)) for m in ibm))                     # column-major
    v_t = add(f32(0, 1))
    v_q = add(f32(0, 0, 0, 1, 0, 0, h, h))
    acc = lambda view, ctype, count, kind, **kw: dict(bufferView=view, componentType=ctype, count=count, type=kind, **kw)
    doc = {"asset": {"version": "2.0"}, "scene": 0, "scenes": [{"nodes": [0, 2]}],
           "nodes": [{"children": [1]}, {"translation": [0, 1, 0]}, {"mesh": 0, "skin": 0}],
           "meshes": [{"primitives": [{"attributes": {"POSITION": 0, "NORMAL": 1, "JOINTS_0": 2, "WEIGHTS_0": 3, "JOINTS_1": 4, "WEIGHTS_1": 5},
                                       "indices": 6}]}],
           "skins": [{"joints": [0, 1], "inverseBindMatrices": 7}],
           "animations": [{"samplers": [{"input": 8, "output": 9, "interpolation": "LINEAR"}],
                           "channels": [{"sampler": 0, "target": {"node": 1, "path": "rotation"}}]}],
           "accessors": [acc(v_pos, 5126, 3, "VEC3", min=[0, 0, 0], max=[0, 2, 0]), acc(v_nrm, 5126, 3, "VEC3"), acc(v_j0, 5121, 3, "VEC4"),
                         acc(v_w0, 5126, 3, "VEC4"), acc(v_j1, 5121, 3, "VEC4"), acc(v_w1, 5126, 3, "VEC4"), acc(v_idx, 5123, 3, "SCALAR"),
                         acc(v_ibm, 5126, 2, "MAT4"), acc(v_t, 5126, 2, "SCALAR", min=[0], max=[1]), acc(v_q, 5126, 2, "VEC4")]}
    binary = b"".join(parts)
    doc["buffers"], doc["bufferViews"] = [{"byteLength": len(binary)}], views
    text = json.dumps(doc).encode()
    text += b" " * (-len(text) % 4)
    return (struct.pack("<4sII", b"glTF", 2, 28 + len(text) + len(binary)) + struct.pack("<I4s", len(text), b"JSON") + text
            + struct.pack("<I4s", len(binary), b"BIN\0") + binary)


def test_reader_and_evaluator_on_a_two_bone_file_written_by_hand():
    doc, binary = gr.read_glb(_two_bone_glb())
    at = gr.primitive(doc, binary)
    assert at["POSITION"].tolist() == [[0, 0, 0], [0, 2, 0], [0, 1.5, 0]] and at["indices"].tolist() == [[0, 1, 2]]
    assert at["JOINTS_1"].tolist()[2] == [0, 1, 0, 0] and at["WEIGHTS_0"].dtype == np.float32
    # the bind pose: every joint matrix is the identity, the mesh stands as stored
    assert np.abs(gr.joint_matrices(doc, binary) - np.eye(4)).max() < 1e-15
    p, n = gr.skinned(doc, binary)
    assert np.abs(p - at["POSITION"]).max() < 1e-15 and np.abs(n - at["NORMAL"]).max() < 1e-15
    # t = 1: joint 1 has turned (x, y) -> (-y, x) about its own origin (0, 1, 0)
    p, n = gr.skinned(doc, binary, 1.0)
    assert np.abs(p - [[0, 0, 0], [-1, 1, 0], [-0.25, 1.25, 0]]).max() < 1e-7          # (sqrt(1/2) is stored in fp32)
    assert np.abs(n[:2] - [[1, 0, 0], [0, 1, 0]]).max() < 1e-7
    assert np.abs(n[2] - np.array([-0.5, 0.5, 0]) / np.sqrt(0.5)).max() < 1e-7        # (0,1,0) -> half itself, half (-1,0,0)
    # t = 0.5: 45 degrees; beyond the last key the value holds
    p = gr.skinned(doc, binary, 0.5)[0]
    s = np.sqrt(0.5)
    assert np.abs(p - [[0, 0, 0], [-s, 1 + s, 0], [-s / 4, 1.25 + s / 4, 0]]).max() < 1e-7
    assert np.array_equal(gr.skinned(doc, binary, 7.0)[0], gr.skinned(doc, binary, 1.0)[0])
    g = gr.node_globals(doc, binary, 1.0)
    assert np.abs(g[1] - [[0, -1, 0, 0], [1, 0, 0, 1], [0, 0, 1, 0], [0, 0, 0, 1]]).max() < 1e-7


# ---- the weights of a canonical point --------------------------------------------------------------------------------------------------
def test_weight_reference_equals_grid_sample_inside_on_the_faces_and_outside():
    vol = gr.weight_volume().astype(np.float64)
    for n in gr.WEIGHT_SIZES:
        x = gr.weight_points(n).astype(np.float64)
        ref = gr.weights_full_ref(x, vol, gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE)
        g = gr.WEIGHT_SCALE.astype(np.float64) * (x + gr.WEIGHT_OFFSET.astype(np.float64))
        if n >= 63:
            assert (np.abs(g).max(1) < 1).any() and (np.abs(g).max(1) > 1.2).any() and (np.abs(np.abs(g) - 1).min(1) < 1e-6).any()
        t = torch.nn.functional.grid_sample(torch.as_tensor(vol)[None], torch.as_tensor(g)[None, :, None, None], mode="bilinear",
                                            padding_mode="border", align_corners=True)
        assert np.abs(t[0, :, :, 0, 0].T.numpy() - ref).max() < 1e-12


def test_top_k_takes_the_lower_joint_on_an_exact_tie_and_names_joint_0_for_zero():
    x = gr.weight_points(65)
    j, w, full, kept, order = gr.rig_weights_ref(x, gr.tie_volume(), gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE, 2)
    assert np.array_equal(j, np.tile([3, 7], (65, 1))) and np.array_equal(w, np.full((65, 2), 0.5))
    j, w = gr.rig_weights_ref(x, gr.tie_volume(), gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE, 6)[:2]
    assert np.array_equal(j, np.tile([3, 7, 11, 20, 0, 0], (65, 1))) and np.array_equal(w, np.tile([0.25] * 4 + [0, 0], (65, 1)))
    # a descending order, sums of one, and the rule for points that have no weights
    j, w, full, kept, order = gr.rig_weights_ref(x, gr.weight_volume(), gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE, 8)
    assert (np.diff(w, axis=1) <= 0).all() and np.abs(w.sum(1) - 1).max() < 1e-15
    assert all(len(set(r)) == 8 for r in j.tolist())
    bad = x.copy()
    bad[0, 1], bad[1, 2] = np.nan, np.inf
    j, w, full = gr.rig_weights_ref(bad, gr.weight_volume(), gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE, 4)[:3]
    assert j[:2].tolist() == [[0] * 4] * 2 and w[:2].tolist() == [[1, 0, 0, 0]] * 2 and not full[:2].any() and w[2:].min() > 0
    j, w = gr.topk_ref(np.zeros((3, 24)), 4)[:2]
    assert not j.any() and w.tolist() == [[1, 0, 0, 0]] * 3


def test_the_index_comparison_of_the_gpu_test_skips_at_most_one_point_in_a_hundred():
    """with the reference alone, on the seeded inputs tests/test_gpu_rig.py uses"""
    vol, E = gr.weight_volume(), gr.full_bound(gr.WEIGHT_DIMS)
    assert 30 * gr.U < E < 40 * gr.U                           # 11 + (3 * 1 + 1) + (3 * 2 + 1) + (3 * 4 + 1) = 35 roundings
    total = skipped = 0
    for n in gr.WEIGHT_SIZES:
        for K in gr.WEIGHT_KS:
            j, w, full, kept, order = gr.rig_weights_ref(gr.weight_points(n), vol, gr.WEIGHT_OFFSET, gr.WEIGHT_SCALE, K)
            total, skipped = total + n, skipped + int(gr.index_skips(kept, order, full, K, E).sum())
    assert total == 4 * sum(gr.WEIGHT_SIZES) and skipped <= total // 100, (skipped, total)


# ---- the writer ------------------------------------------------------------------------------------------------------------------
def _rig_inputs(nv=37, nf=20, K=6, F=4, seed=0):
    """a random mesh with a random rig over SMPL's joint tree; everything that goes into the file is fp32-exact"""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    verts, normals = f32(rng.standard_normal((nv, 3))), rng.standard_normal((nv, 3))
    normals[3] = 0                                             # replaced by the fallback
    normals[5] = np.nan                                        # no fallback either: (0, 0, 1)
    fallback = rng.standard_normal((nv, 3))
    fallback[5] = 0
    faces = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int32)
    joints = np.stack([rng.permutation(24)[:K] for _ in range(nv)]).astype(np.uint8)
    w = rng.random((nv, K)).astype(np.float32)
    weights = f32(w / w.sum(1, keepdims=True))
    parents = sr.SMPL_PARENTS.copy()
    J = f32(rng.standard_normal((24, 3)) * 0.3)
    rest = J.copy()
    rest[1:] = J[1:] - J[parents[1:]]
    rest = f32(rest)
    cano = f32(gr.quaternions_ref(rng.standard_normal(72) * 0.3))
    quat = f32(gr.quaternions_ref(rng.standard_normal((F, 72)) * 0.8))
    root_t = f32(rng.standard_normal((F, 3)))
    ibm = np.linalg.inv(_globals(parents, cano, rest))
    ibm[:, 3] = (0, 0, 0, 1)
    return dict(verts=verts, faces=faces, normals=normals, fallback=fallback, joints=joints, weights=weights, parents=parents,
                rest=rest, cano=cano, ibm=f32(ibm), quat=quat, root_t=root_t, colors=rng.integers(0, 256, (nv, 3)).astype(np.uint8))


def _globals(parents, quat, trans):
    """[24,4,4] chain of the local transforms [R(q_j) | t_j], written out directly"""
    G = np.zeros((24, 4, 4))
    for j in range(24):
        L = np.eye(4)
        L[:3, :3], L[:3, 3] = gr.quat_matrix(quat[j]), trans[j]
        G[j] = L if j == 0 else G[parents[j]] @ L
    return G


def _write(tmp_path, d, name="a.glb", **kw):
    from instantavatar_amd import gltf
    path = str(tmp_path / name)
    args = dict(fallback_normals=d["fallback"], joints=d["joints"], weights=d["weights"], parents=d["parents"], rest_translation=d["rest"],
                cano_quat=d["cano"], inverse_bind=d["ibm"])
    args.update(kw)
    gltf.write_glb(path, d["verts"], d["faces"], d["normals"], **args)
    return path


def _check_structure(path):
    doc, binary = gr.read_glb(path)
    text, blob = gr.chunk_padding(path)
    assert len(text) % 4 == 0 and len(blob) % 4 == 0 and text.rstrip(b" ") == json.dumps(doc, separators=(",", ":")).encode()
    assert doc["buffers"] == [{"byteLength": len(binary)}] and doc["asset"]["version"] == "2.0"
    ends = 0
    for v in doc["bufferViews"]:
        assert v["byteOffset"] % 4 == 0 and v["byteOffset"] >= ends and not any(binary[ends:v["byteOffset"]])       # zero padding
        ends = v["byteOffset"] + v["byteLength"]
    assert ends <= len(binary) and not any(binary[ends:])
    for i, a in enumerate(doc["accessors"]):
        size = np.dtype(gr._NP[a["componentType"]]).itemsize
        assert (doc["bufferViews"][a["bufferView"]]["byteOffset"] + a.get("byteOffset", 0)) % size == 0 and a.get("byteOffset", 0) % size == 0
        if "min" in a:
            got = gr.accessor(doc, binary, i).astype(np.float64)
            assert a["min"] == got.min(0).tolist() and a["max"] == got.max(0).tolist()
    prim = doc["meshes"][0]["primitives"][0]
    assert len(doc["meshes"]) == 1 and len(doc["meshes"][0]["primitives"]) == 1 and len(doc["materials"]) == 1 and prim["material"] == 0
    assert "min" in doc["accessors"][prim["attributes"]["POSITION"]]
    m = doc["materials"][0]
    assert m["pbrMetallicRoughness"]["metallicFactor"] == 0 and m["pbrMetallicRoughness"]["roughnessFactor"] == 1
    assert "KHR_materials_unlit" in m["extensions"] and doc["extensionsUsed"] == ["KHR_materials_unlit"]
    at = gr.primitive(doc, binary)
    assert at["NORMAL"].dtype == np.float32 and np.abs(np.linalg.norm(at["NORMAL"].astype(np.float64), axis=1) - 1).max() < 2e-7
    if "skins" in doc:
        sk = doc["skins"][0]
        assert sk["joints"] == list(range(24)) and doc["accessors"][sk["inverseBindMatrices"]]["type"] == "MAT4"
        assert doc["nodes"][24] == {"mesh": 0, "skin": 0, "name": "avatar"} and doc["scenes"][0]["nodes"] == [0, 24]
        sets = sorted(k for k in at if k.startswith("JOINTS_"))
        assert sets == ["JOINTS_%d" % s for s in range(len(sets))] and all(at[k].dtype == np.uint8 and at[k].shape[1] == 4 for k in sets)
        assert all(at["WEIGHTS_%d" % s].dtype == np.float32 for s in range(len(sets)))
    for an in doc.get("animations", []):
        for smp in an["samplers"]:
            assert smp["interpolation"] == "LINEAR" and "min" in doc["accessors"][smp["input"]] and "max" in doc["accessors"][smp["input"]]
    return doc, binary, at


def test_write_glb_vertex_colours_rig_and_animation_round_trip(tmp_path):
    d = _rig_inputs()
    fps = 25.0
    path = _write(tmp_path, d, colors8=d["colors"], animation=(d["quat"], d["root_t"]), fps=fps)
    doc, binary, at = _check_structure(path)
    nv, K = d["joints"].shape
    # the indexed, vertex-coloured layout
    assert np.array_equal(at["POSITION"], d["verts"].astype(np.float32)) and np.array_equal(at["indices"], d["faces"])
    acc = doc["accessors"][doc["meshes"][0]["primitives"][0]["attributes"]["COLOR_0"]]
    assert acc["componentType"] == 5121 and acc["type"] == "VEC4" and acc["normalized"] is True
    assert np.array_equal(at["COLOR_0"][:, :3], d["colors"]) and (at["COLOR_0"][:, 3] == 255).all()
    # normals: unit, the zero one from the fallback, the hopeless one (0, 0, 1)
    keep = np.ones(nv, bool)
    keep[[3, 5]] = False
    n64 = d["normals"][keep] / np.linalg.norm(d["normals"][keep], axis=1, keepdims=True)
    assert np.abs(at["NORMAL"][keep] - n64).max() < 1e-7
    assert np.abs(at["NORMAL"][3] - d["fallback"][3] / np.linalg.norm(d["fallback"][3])).max() < 1e-7 and at["NORMAL"][5].tolist() == [0, 0, 1]
    # K = 6 is padded to two sets of four with (joint 0, weight 0)
    assert sorted(k for k in at if k.startswith(("JOINTS", "WEIGHTS"))) == ["JOINTS_0", "JOINTS_1", "WEIGHTS_0", "WEIGHTS_1"]
    jj, ww = np.concatenate([at["JOINTS_0"], at["JOINTS_1"]], 1), np.concatenate([at["WEIGHTS_0"], at["WEIGHTS_1"]], 1)
    assert np.array_equal(jj[:, :K], d["joints"]) and np.array_equal(ww[:, :K], d["weights"].astype(np.float32)) and not jj[:, K:].any() and not ww[:, K:].any()
    # the skeleton: default TRS = the canonical pose, inverse bind matrices column-major; the bind pose leaves the mesh where it is
    for j, nd in enumerate(doc["nodes"][:24]):
        assert nd["translation"] == d["rest"][j].tolist() and nd["rotation"] == d["cano"][j].tolist()
        assert sorted(nd.get("children", [])) == [k for k in range(1, 24) if d["parents"][k] == j]
    stored = gr.accessor(doc, binary, doc["skins"][0]["inverseBindMatrices"]).reshape(24, 4, 4)
    assert np.array_equal(stored.transpose(0, 2, 1), d["ibm"].astype(np.float32))
    assert np.abs(gr.skinned(doc, binary)[0] - d["verts"]).max() < 1e-5           # (the inverse was rounded to fp32)
    # the animation: 24 rotation channels and the root's translation, keys at i / fps
    an = doc["animations"][0]
    assert [(c["target"]["node"], c["target"]["path"]) for c in an["channels"]] == [(j, "rotation") for j in range(24)] + [(0, "translation")]
    F = len(d["quat"])
    times = gr.accessor(doc, binary, an["samplers"][0]["input"])[:, 0]
    assert np.array_equal(times, (np.arange(F) / fps).astype(np.float32)) and len({s["input"] for s in an["samplers"]}) == 1
    # read back and evaluated at every key = numpy linear-blend skinning of the inputs, the chain written out directly
    for f in range(F):
        rest = d["rest"].copy()
        rest[0] = d["root_t"][f]
        Bm = _globals(d["parents"], d["quat"][f], rest) @ d["ibm"]
        M = (d["weights"][:, :, None, None] * Bm[d["joints"].astype(int)]).sum(1)
        want = np.einsum("nab,nb->na", M[:, :3, :3], d["verts"]) + M[:, :3, 3]
        got, got_n = gr.skinned(doc, binary, float(times[f]))
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), f
        m = np.einsum("nab,nb->na", M[:, :3, :3], at["NORMAL"].astype(np.float64))
        assert np.abs(got_n - m / np.linalg.norm(m, axis=1, keepdims=True)).max() < 1e-12
        lp, ln = gr.lbs_ref(d["verts"], at["NORMAL"], d["joints"], d["weights"], Bm[None])
        assert np.abs(lp[0] - want).max() <= 1e-12 * np.abs(want).max() and np.abs(ln[0] - got_n).max() < 1e-12


def test_write_glb_textured_layout_is_unindexed_with_v_flipped(tmp_path):
    from PIL import Image
    import io
    d = _rig_inputs(seed=1, K=4)
    nf, B = len(d["faces"]), 5
    T = tx.atlas_size(nf, B)
    uv = tx.corner_uv(nf, B)                                                 # continuous texels (x, y), y = 0 in the PNG's top row
    vt = np.stack([uv[..., 0] / T, 1 - uv[..., 1] / T], -1)                  # what Texture.vt() gives the OBJ
    image = np.random.default_rng(3).integers(0, 256, (T, T, 3)).astype(np.uint8)
    path = _write(tmp_path, d, corner_uv=np.stack([vt[..., 0], 1 - vt[..., 1]], -1), image=image)
    doc, binary, at = _check_structure(path)
    prim = doc["meshes"][0]["primitives"][0]
    assert "indices" not in prim and "COLOR_0" not in prim["attributes"] and len(at["POSITION"]) == 3 * nf
    pick = d["faces"].reshape(-1)
    assert np.array_equal(at["POSITION"], d["verts"].astype(np.float32)[pick]) and np.array_equal(at["JOINTS_0"], d["joints"][pick])
    assert np.array_equal(at["WEIGHTS_0"], d["weights"].astype(np.float32)[pick])
    assert np.array_equal(at["TEXCOORD_0"], (uv / T).astype(np.float32).reshape(-1, 2))                    # (u, 1 - v) = (x / T, y / T)
    assert np.abs(at["TEXCOORD_0"][:, 1] - (1 - vt[..., 1].reshape(-1))).max() < 1e-7
    img = doc["images"][0]
    assert img["mimeType"] == "image/png" and doc["textures"] == [{"sampler": 0, "source": 0}]
    assert doc["materials"][0]["pbrMetallicRoughness"]["baseColorTexture"] == {"index": 0}
    v = doc["bufferViews"][img["bufferView"]]
    png = Image.open(io.BytesIO(binary[v["byteOffset"]:v["byteOffset"] + v["byteLength"]]))
    assert png.mode == "RGB" and np.array_equal(np.asarray(png), image)
    assert np.abs(gr.skinned(doc, binary)[0] - d["verts"][pick]).max() < 1e-5
    # without a rig: one node, no skin; and the refusals
    from instantavatar_amd import gltf
    gltf.write_glb(str(tmp_path / "plain.glb"), d["verts"], d["faces"], d["normals"], colors8=d["colors"])
    doc = _check_structure(str(tmp_path / "plain.glb"))[0]
    assert "skins" not in doc and doc["nodes"] == [{"mesh": 0, "name": "avatar"}] and "animations" not in doc
    for kw in (dict(), dict(colors8=d["colors"], corner_uv=uv, image=image), dict(corner_uv=uv), dict(colors8=d["colors"], joints=d["joints"]),
               dict(colors8=d["colors"], animation=(d["quat"], d["root_t"]))):
        with pytest.raises(ValueError):
            gltf.write_glb(str(tmp_path / "bad.glb"), d["verts"], d["faces"], d["normals"], **kw)


def test_quaternion_signs_are_made_continuous_where_the_angle_passes_pi(tmp_path):
    """joint 1 turns about z by 0.95 pi, then by 1.05 pi written as -0.95 pi: the two quaternions have a negative dot product, and
    interpolating them as they are would go the long way round, through the identity"""
    from instantavatar_amd import gltf, rig
    poses = np.zeros((3, 72))
    poses[:, 5] = [0.9 * np.pi, 0.95 * np.pi, -0.95 * np.pi]
    q = gr.quaternions_ref(poses)
    assert np.abs(rig.quaternions(poses) - q).max() < 1e-15 and np.abs(np.linalg.norm(q, axis=-1) - 1).max() < 1e-15
    assert (q[2, 1] * q[1, 1]).sum() < 0
    c = gltf.continuous_quaternions(q)
    assert ((c[1:] * c[:-1]).sum(-1) >= 0).all() and np.array_equal(c[2, 1], -q[2, 1]) and np.array_equal(c[:2], q[:2]) and np.array_equal(c[2, 0], q[2, 0])
    d = _rig_inputs(seed=2, K=4)
    path = _write(tmp_path, d, colors8=d["colors"], animation=(q, np.zeros((3, 3))), fps=1.0)
    doc, binary = gr.read_glb(path)
    an = doc["animations"][0]
    stored = gr.accessor(doc, binary, an["samplers"][1]["output"]).astype(np.float64)
    assert ((stored[1:] * stored[:-1]).sum(-1) > 0).all()
    mid = gr.animated(doc, binary, 1.5)[(1, "rotation")]                     # half way between 0.95 pi and 1.05 pi: pi about z
    assert np.abs(gr.quat_matrix(mid) - np.diag([-1.0, -1.0, 1.0])).max() < 1e-6
    # the quaternion against Rodrigues as smpl_refs states it: the gap the non-unit axis opens stays below 3 |e|, |e| <= sqrt(3) 1e-8 / |theta|
    pose = sr.make_pose("extreme", 3).astype(np.float64)
    gap = gr.rodrigues_gap(pose)[0]
    size = np.linalg.norm(pose.reshape(24, 3), axis=1)
    assert (gap > 0).all() and (gap <= 3.5 * 3 * np.sqrt(3) * 1e-8 / size).all() and gap.max() < 1e-6
    small = np.zeros(72)
    small[3] = 1e-4
    assert gr.rodrigues_gap(small)[0, 1] < 3 * 1e-4 * 1e-4                   # |e| = 1e-4, and sin(ang) = 1e-4 scales the difference
    assert gr.rodrigues_gap(np.zeros(72)).max() == 0 and np.array_equal(gr.quaternions_ref(np.zeros(72)), np.tile([0, 0, 0, 1.0], (24, 1)))


def test_track_reference_is_the_chain_of_the_node_settings():
    """global(node_j) . IBM_j with the node settings of the definition equals B_j = A_j . tfs_inv_t_j of tfs_fwd_ref"""
    i = sr.tfs_inputs("smpl-random")
    J, par = i["joints_rest"].astype(np.float64), i["parents"]
    cano = sr.make_pose("mixed", 9)
    cano[:3] = 0
    B = sr._affine_inv(sr.tfs_fwd_ref(J, par, cano, None, np.tile(np.eye(4), (24, 1, 1)))["A"])           # tfs_inv_t of that canonical pose
    ref = gr.track_ref(J, par, i["pose"][None], i["transl"][None], B)
    rest = J.copy()
    rest[1:] = J[1:] - J[par[1:]]
    ibm = B.copy()
    ibm[:, :3, 3] -= J
    assert np.abs(_globals(par, gr.quaternions_ref(cano), rest) @ ibm - np.eye(4)).max() < 1e-7          # = inv(G(cano)), up to the Rodrigues gap
    rest[0] = ref["root_t"][0]
    got = _globals(par, ref["quat"][0], rest) @ ibm
    assert np.abs(got - ref["bones"][0]).max() < 1e-6
    b = gr.track_bound(J, par, i["pose"][None], i["transl"][None], B.astype(np.float32))
    assert set(b) == {"bones.R", "bones.t", "bones.row3", "quat", "root_t"} and 0 < b["bones.R"][1] < 1e-4 and b["quat"][1] == gr.E_Q


def test_skinning_bound_covers_an_fp32_evaluation():
    rng = np.random.default_rng(5)
    n, K, F = 50, 8, 2
    x, nn = rng.standard_normal((n, 3)).astype(np.float32), rng.standard_normal((n, 3)).astype(np.float32)
    j = rng.integers(0, 24, (n, K)).astype(np.uint8)
    w = rng.random((n, K)).astype(np.float32)
    w /= w.sum(1, keepdims=True)
    B = np.tile(np.eye(4, dtype=np.float32), (F, 24, 1, 1))
    B[..., :3, :] = rng.standard_normal((F, 24, 3, 4)).astype(np.float32)
    p, m = gr.lbs_ref(x, nn, j, w, B)
    bp, bn = gr.skin_bound(x, nn, j, w, B)
    M = np.zeros((F, n, 3, 4), np.float32)
    for k in range(K):
        M = M + w[None, :, k, None, None] * B[:, j[:, k].astype(int), :3, :]
    p32 = ((M[..., 0] * x[:, 0, None] + M[..., 1] * x[:, 1, None]) + M[..., 2] * x[:, 2, None]) + M[..., 3]
    assert (np.abs(p32.astype(np.float64) - p) <= bp).all() and (bp < 1e-5).all() and (bn < 1e-4).all()


# ---- the binding -------------------------------------------------------------------------------------------------------------------
def test_rig_header_is_bound():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    d = _lib.declarations("rig")
    assert sorted(d) == NAMES
    assert len(_lib.declarations()) == 89
    for name in NAMES:
        assert d[name].stream, name                                                # every entry point launches and takes a stream
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
    assert "ia_rig.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_rig.hip"))
    assert os.path.normpath(_lib.header_path("rig")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_rig.hip" in build.source_manifest() and "ia_rig.hip" in build.library_manifest()
    with pytest.raises(_lib.IAError, match=r"instantavatar_hip_rig\.h"):
        _lib.call("ia_rig_export")


def test_host_side_argument_errors():
    """what the entry points decide before any launch"""
    from instantavatar_amd import _lib
    P = 4096                                                  # (a non-null address that is never read: every call below is refused)
    grid = _lib.SnarfGrid()
    grid.D, grid.H, grid.W = 2, 3, 5
    for K in (0, 25, -1):
        with pytest.raises(_lib.IAError, match="K = %d" % K):
            _lib.call("ia_rig_weights", P, 8, P, 0, grid, K, P, P, None, None)
        with pytest.raises(_lib.IAError, match="K = %d" % K):
            _lib.call("ia_rig_skin", P, None, 8, P, P, K, P, 2, P, None, None)
    with pytest.raises(_lib.IAError, match="n = -1"):
        _lib.call("ia_rig_weights", P, -1, P, 0, grid, 4, P, P, None, None)
    with pytest.raises(_lib.IAError, match="n = -1"):
        _lib.call("ia_rig_skin", P, None, -1, P, P, 4, P, 2, P, None, None)
    for F in (-1,):
        with pytest.raises(_lib.IAError, match="F = -1"):
            _lib.call("ia_rig_track", P, P, P, None, P, F, P, None, None, None)
        with pytest.raises(_lib.IAError, match="F = -1"):
            _lib.call("ia_rig_skin", P, None, 8, P, P, 4, P, F, P, None, None)
    with pytest.raises(_lib.IAError, match="together"):
        _lib.call("ia_rig_skin", P, P, 8, P, P, 4, P, 2, P, None, None)
    with pytest.raises(_lib.IAError, match="together"):
        _lib.call("ia_rig_skin", P, None, 8, P, P, 4, P, 2, P, P, None)
    with pytest.raises(_lib.IAError, match="16-byte"):
        _lib.call("ia_rig_skin", P, None, 8, P, P, 4, P + 4, 2, P, None, None)
    with pytest.raises(_lib.IAError, match="16-byte"):
        _lib.call("ia_rig_weights", P, 8, P + 4, 1, grid, 4, P, P, None, None)
    bad = _lib.SnarfGrid()
    with pytest.raises(_lib.IAError, match="bad grid"):
        _lib.call("ia_rig_weights", P, 8, P, 0, bad, 4, P, P, None, None)
    for args in ((None, 8, P, 0, grid, 4, P, P), (P, 8, None, 0, grid, 4, P, P), (P, 8, P, 0, grid, 4, None, P), (P, 8, P, 0, grid, 4, P, None)):
        with pytest.raises(_lib.IAError, match="null pointer"):
            _lib.call("ia_rig_weights", *args, None, None)
    for args in ((None, P, P, None, P, 2, P), (P, None, P, None, P, 2, P), (P, P, None, None, P, 2, P), (P, P, P, None, None, 2, P), (P, P, P, None, P, 2, None)):
        with pytest.raises(_lib.IAError, match="null pointer"):
            _lib.call("ia_rig_track", *args, None, None, None)
    for args in ((None, None, 8, P, P, 4, P, 2, P), (P, None, 8, None, P, 4, P, 2, P), (P, None, 8, P, None, 4, P, 2, P), (P, None, 8, P, P, 4, None, 2, P),
                 (P, None, 8, P, P, 4, P, 2, None)):
        with pytest.raises(_lib.IAError, match="null pointer"):
            _lib.call("ia_rig_skin", *args, None, None)
    # empty work is accepted without a launch
    assert _lib.call("ia_rig_weights", None, 0, None, 0, None, 4, None, None, None, None) == 0
    assert _lib.call("ia_rig_track", None, None, None, None, None, 0, None, None, None, None) == 0
    assert _lib.call("ia_rig_skin", None, None, 0, None, None, 4, None, 2, None, None, None) == 0
    assert _lib.call("ia_rig_skin", None, None, 8, None, None, 4, None, 0, None, None, None) == 0


def test_cpu_tensors_and_bad_arguments_raise_in_python():
    from instantavatar_amd import _lib, mesh, rig
    from instantavatar_amd.pipeline import AvatarModel
    f = lambda *s: torch.zeros(s)
    b = lambda *s: torch.zeros(s, dtype=torch.uint8)
    grid = _lib.SnarfGrid()
    grid.D, grid.H, grid.W = 2, 3, 5
    calls = {
        "ia_rig_weights": (f(8, 3), 8, f(24, 2, 3, 5), 0, grid, 4, b(8, 4), f(8, 4), None),
        "ia_rig_track": (f(24, 3), torch.zeros(24, dtype=torch.int32), f(2, 72), None, f(24, 4, 4), 2, f(2, 24, 4, 4), None, None),
        "ia_rig_skin": (f(8, 3), None, 8, b(8, 4), f(8, 4), 4, f(2, 24, 4, 4), 2, f(2, 8, 3), None),
    }
    assert sorted(calls) == NAMES
    for name, args in calls.items():
        with pytest.raises(_lib.IAError, match="GPU"):
            _lib.call(name, *args, None)
    m = mesh.Mesh(f(8, 3), torch.zeros((4, 3), dtype=torch.int32), f(8, 3), f(8, 3))
    r = rig.Rig(b(8, 4), f(8, 4), None, None, None, None)
    assert r.influences == 4
    with pytest.raises(_lib.IAError, match="GPU"):
        rig.skin(r, m, f(2, 24, 4, 4))
    with pytest.raises(_lib.IAError, match="animation needs a rig"):
        m.to_glb("unused.glb", animation=(f(2, 24, 4), f(2, 3)))

    class Other:
        initialized = True
    for call in (lambda: rig.build(Other(), m), lambda: rig.track(Other(), f(2, 72)), lambda: AvatarModel(Other(), None, None).rig_mesh(m)):
        with pytest.raises(NotImplementedError, match="SNARF"):
            call()
    mx, mean = rig.deviation(torch.tensor([[[0.0, 0, 0], [1, 0, 0]]]), torch.tensor([[[0.0, 3, 4], [1, 0, 0]]]))
    assert mx.tolist() == [5.0] and mean.tolist() == [2.5]


def test_the_driver_refuses_bad_rig_flags_before_it_touches_a_device():
    from instantavatar_amd.drivers import extract_mesh as drv
    for argv in (["--synthetic", "--rig", "25"], ["--synthetic", "--rig", "-1"], ["--synthetic", "--rig", "4", "--fps", "0"],
                 ["--synthetic", "--fps", "nan"]):
        with pytest.raises(SystemExit):
            drv.main(argv)
