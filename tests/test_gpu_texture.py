"""csrc/ia_texture.hip against tests/texture_refs.py (float64 numpy, validated in tests/test_cpu_texture_refs.py): each entry point
alone at the smallest shapes where it can go wrong, then whole bakes with an analytic field -- a sphere whose texels must all land on
it, and meshes whose textured pictures must show the field's colour at every covered pixel -- then `AvatarModel.bake_texture`, the
OBJ writer and the extract_mesh driver on the synthetic model.

Tolerances.  owner and the corner uv are integers and half-integers: exact.  pts / normal: the kernel and numpy evaluate the same
fp64 expressions, whose results differ by ~1e-16 (association, contraction); rounding to fp32 adds half an ulp of the value, so 1 ulp
of the largest coordinate magnitude.  t: the kernel's fp32 operation sequence is the reference's, 4 ulp of `dist` allows a division or
multiplication rounded differently.  Sampling: three lerps of one subtraction and one fma each on values in [0, 1], plus the two
weights: 8 ulp of 1 against float64."""
import os

import numpy as np
import pytest
import torch

import texture_refs as tx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP1 = float(np.spacing(np.float32(1)))
LEVEL, RADIUS = 10.0, 0.5


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _ulp(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def _mesh(v, f):
    from instantavatar_amd.mesh import Mesh
    nv = len(v)
    return Mesh(_dev(v, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3), torch.zeros((nv, 3), device=DEV),
                torch.zeros((nv, 3), device=DEV))


def _case_mesh(nf):
    """random vertices; from 7 faces on: face 1 without area, face 2 with a NaN vertex, faces 3 and 4 with an index outside [0, nv)"""
    rng = np.random.default_rng(nf)
    nv = 12
    v = (rng.standard_normal((nv, 3)) * 3).astype(np.float32)
    f = np.stack([rng.permutation(nv - 1)[:3] for _ in range(nf)]).astype(np.int32)        # (vertex nv - 1 is kept for the NaN)
    if nf >= 7:
        v[nv - 1, 1] = np.nan
        f[1] = [f[1, 0], f[1, 1], f[1, 0]]
        f[2, 2] = nv - 1
        f[3, 0] = nv
        f[4, 1] = -1
    return v, f


@pytest.fixture(scope="module")
def sphere():
    v, f = tx.octasphere(2, RADIUS)
    return v, f, tx.max_sag(v, f, RADIUS)


# ---- the entry points, one at a time ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [4, 5, 8])
@pytest.mark.parametrize("nf", [1, 2, 3, 7, 33])
def test_corner_uv_and_texel_points_against_reference(nf, B):
    from instantavatar_amd import _lib, texture
    v, f = _case_mesh(nf)
    T = tx.atlas_size(nf, B)
    assert texture.atlas_size(nf, B) == T
    uv = texture.corner_uv(nf, B, DEV)
    again = texture.corner_uv(nf, B, DEV)
    assert uv.dtype == torch.float32 and np.array_equal(_np(uv).astype(np.float64), tx.corner_uv(nf, B)) and torch.equal(uv, again)
    n = T * T
    rng = np.random.default_rng(100 * nf + B)
    t = (rng.standard_normal(n) * 0.1).astype(np.float32)
    t_scalar = float(np.float32(0.37))
    ref = tx.texel_points(v, f, B, t.astype(np.float64) + t_scalar)
    if nf >= 7:
        assert {-1, 0, 1, 5} <= set(ref["owner"].tolist()) and not {2, 3, 4} & set(ref["owner"].tolist())
    vd, fd, td = _dev(v), _dev(f), _dev(t)
    # the whole atlas, and a range whose ends are no multiples of a wave
    for first, count in ((0, n), (5, min(131, n - 5))):
        outs = []
        for _ in range(2):
            pts, nrm = torch.full((count, 3), 7.0, device=DEV), torch.full((count, 3), 7.0, device=DEV)
            own = torch.full((count,), 7, dtype=torch.int32, device=DEV)
            _lib.call("ia_tex_texel_points", vd, len(v), fd, nf, B, T, first, count, td[first:first + count].contiguous(), t_scalar, pts, nrm, own)
            outs.append((pts, nrm, own))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(*outs)), "two calls differ"
        pts, nrm, own = (_np(a) for a in outs[0])
        sl = slice(first, first + count)
        assert np.array_equal(own, ref["owner"][sl])
        assert np.isfinite(pts).all() and np.isfinite(nrm).all()
        assert np.abs(pts - ref["pts"][sl]).max() <= _ulp(ref["pts"])
        assert np.abs(nrm - ref["normal"][sl]).max() <= ULP1
    # without t, normal and owner: the points on the faces
    pts = torch.empty((n, 3), device=DEV)
    _lib.call("ia_tex_texel_points", vd, len(v), fd, nf, B, T, 0, n, None, 0.0, pts, None, None)
    base = tx.texel_points(v, f, B)
    assert np.abs(_np(pts) - base["pts"]).max() <= _ulp(base["pts"])
    cuv = tx.corner_uv(nf, B)                                    # the corner texels hold the vertices' bits
    for face in set(base["owner"].tolist()) - {-1}:
        for k in range(3):
            x, y = (cuv[face, k] - 0.5).astype(int)
            assert np.array_equal(_np(pts)[y * T + x], v[f[face, k]])


@pytest.mark.parametrize("K", [3, 9, 17])
@pytest.mark.parametrize("n", [131, 1000])
def test_snap_against_reference(n, K):
    from instantavatar_amd import _lib
    rng = np.random.default_rng(n + K)
    dist = 0.07
    sigma = (LEVEL + rng.standard_normal((K, n)) * 5).astype(np.float32)
    sigma[:, :20] = LEVEL + 3 + rng.random((K, 20)).astype(np.float32)                       # no crossing
    sigma[rng.integers(0, K, 40), rng.integers(20, n, 40)] = np.nan
    sigma[rng.integers(0, K, 10), rng.integers(20, n, 10)] = np.inf
    sigma[rng.integers(0, K, 10), rng.integers(20, n, 10)] = LEVEL                             # s = 0
    sigma[:, 21] = LEVEL + np.where(np.arange(K) % (K - 1) == 0, -1, 1)                        # a tie at the two ends
    owner = np.where(rng.random(n) < 0.15, -1, np.arange(n)).astype(np.int32)
    owner[:5] = -1
    owner[21] = 21
    for own in (owner, None):
        want_t, want_miss = tx.snap(sigma, LEVEL, dist, own)
        assert 0 < want_miss < n
        outs = []
        for _ in range(2):
            t = torch.full((n,), 7.0, device=DEV)
            cnt = torch.full((1,), 3, dtype=torch.int32, device=DEV)                           # accumulated onto what is there
            _lib.call("ia_tex_snap", _dev(sigma), K, n, LEVEL, dist, None if own is None else _dev(own), t, cnt)
            outs.append((t, cnt))
        torch.cuda.synchronize()
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        assert int(outs[0][1]) == 3 + want_miss
        assert np.abs(_np(outs[0][0]) - want_t).max() <= 4 * _ulp(np.float32(dist))
    if K == 3:
        assert want_t[21] == -np.float32(dist) / 2               # -h / 2 and +h / 2 tie exactly: the smaller k
    t, cnt = torch.full((n,), 7.0, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.call("ia_tex_snap", _dev(sigma), K, n, LEVEL, 0.0, None, t, cnt)                        # dist = 0: no snap, nothing counted
    assert not t.any() and int(cnt) == 0


@pytest.mark.parametrize("T,R", [(4, 131), (25, 1000)])
def test_sample_against_reference(T, R):
    from instantavatar_amd import _lib
    rng = np.random.default_rng(T)
    atlas = rng.random((T, T, 3)).astype(np.float32)
    uv = (rng.random((R, 2)) * (T + 2) - 1).astype(np.float32)                                 # also outside the atlas
    centres = np.array([[x + 0.5, y + 0.5] for y in range(min(T, 4)) for x in range(T)], np.float32)
    uv[:len(centres)] = centres
    uv[len(centres)] = [np.nan, 1.5]
    uv[len(centres) + 1] = [1.5, np.inf]
    uv[len(centres) + 2] = [-1e30, 1e30]
    mask = (rng.random(R) < 0.8).astype(np.float32)
    mask[:len(centres) + 3] = 1
    for m in (mask, None):
        outs = []
        for _ in range(2):
            out = torch.full((R, 3), 7.0, device=DEV)
            _lib.call("ia_tex_sample", _dev(atlas), T, _dev(uv), None if m is None else _dev(m), R, out)
            outs.append(out)
        torch.cuda.synchronize()
        assert torch.equal(*outs)
        got = _np(outs[0])
        assert np.abs(got - tx.sample(atlas, uv, m)).max() <= 8 * ULP1
        assert np.array_equal(got[:len(centres)], atlas[:min(T, 4)].reshape(-1, 3))            # a texel centre returns the texel's bits
        assert not got[len(centres):len(centres) + 2].any()
        assert np.array_equal(got[len(centres) + 2], atlas[T - 1, 0])
        if m is not None:
            assert not got[m == 0].any()


# ---- whole bakes with an analytic field -----------------------------------------------------------------------------------------------
def _field(A, b):
    A, b = _dev(A, torch.float32), _dev(b, torch.float32)

    def sample(p):
        return p @ A.T + b, LEVEL + 50 * (RADIUS - p.norm(dim=1))
    return sample


def test_bake_snaps_every_texel_of_a_sphere_onto_it(sphere):
    """sigma - level = 50 (r - |x|) along a line x(t) = p + t n is 50 (r - rho(t)) with rho'' = g^2 / rho^3 <= 1 / rho, g the distance of
    the line to the centre.  Linear interpolation with step h of a function whose second derivative is at most M errs by at most
    h^2 M / 8, so at the root t* of the interpolant |rho(t*) - r| <= h^2 / (8 rho_min): the distance of the snapped point to the
    sphere.  rho_min >= g_min := r - sag - dist bounds every sample point from below: the faces lie within `sag` under the sphere,
    the samples within `dist` of the faces (texels extrapolated past an edge lie further out, not further in)."""
    from instantavatar_amd import texture
    v, f, sag = sphere
    dist, K, B = 2 * sag, 9, 8
    # colour = position: the atlas holds the snapped points themselves
    tex = texture.bake(_mesh(v, f), _field(np.eye(3), np.zeros(3)), block=B, snap=dist, level=LEVEL, steps=K)
    again = texture.bake(_mesh(v, f), _field(np.eye(3), np.zeros(3)), block=B, snap=dist, level=LEVEL, steps=K, chunk=1000)
    torch.cuda.synchronize()
    assert tex.size == 64 and tex.block == B and tex.atlas.shape == (64, 64, 3) and tex.rgba8.shape == (64, 64, 4) and tex.uv.shape == (128, 3, 2)
    assert tex.unsnapped.dtype == torch.int32 and tex.unsnapped.is_cuda
    assert int(tex.unsnapped) == 0
    assert torch.equal(tex.atlas, again.atlas) and torch.equal(tex.rgba8, again.rgba8) and int(again.unsnapped) == 0      # chunks do not matter
    h = 2 * dist / (K - 1)
    g_min = RADIUS - sag - dist
    bound = h * h / (8 * g_min) + 16 * float(np.finfo(np.float32).eps) * RADIUS       # + fp32: the point, |x| and sigma are rounded
    off = np.abs(np.linalg.norm(_np(tex.atlas).reshape(-1, 3).astype(np.float64), axis=1) - RADIUS)
    print("sphere bake: largest distance of a snapped texel to the sphere %.3e, bound %.3e (sag %.4f, snap %.4f)" % (off.max(), bound, sag, dist))
    assert off.max() <= bound
    assert (_np(tex.rgba8)[..., 3] == 255).all()
    # without a snap the texels stay on the faces: up to `sag` under the sphere, and the count stays 0
    flat = texture.bake(_mesh(v, f), _field(np.eye(3), np.zeros(3)), block=B, snap=0.0)
    d = RADIUS - np.linalg.norm(_np(flat.atlas).reshape(-1, 3).astype(np.float64), axis=1)
    assert int(flat.unsnapped) == 0 and 0.5 * sag < d.max() <= sag + 1e-6
    # a snap that cannot reach: every texel of the face interiors stays unsnapped, and none is moved
    short = texture.bake(_mesh(v, f), _field(np.eye(3), np.zeros(3)), block=B, snap=sag * 1e-3)
    assert 0 < int(short.unsnapped) <= 64 * 64


def _pictures_show_the_field(v, f, B, box, cull):
    """bake A x + b without a snap, draw the mesh at 64^2, and compare every covered pixel with A x + b at the surface point the
    rasteriser interpolates there.  A = s I with s such that half a texel of the SMALLEST face edge changes a channel by 0.02."""
    from instantavatar_amd import raster, texture
    vv = v.astype(np.float64)
    edges = np.concatenate([np.linalg.norm(vv[f[:, k]] - vv[f[:, (k + 1) % 3]], axis=1) for k in range(3)])
    half_texel = edges.min() / (B - 3) / 2
    A, b = np.eye(3) * (0.02 / half_texel), np.array([0.5, 0.4, 0.6])
    m = _mesh(v, f)
    m.normals = _dev(v / np.linalg.norm(v, axis=1, keepdims=True), torch.float32) if cull else torch.tensor([[0.0, 0.0, -1.0]], device=DEV).expand(len(v), 3).contiguous()
    plain = raster.render(m, raster.look_at_box(*box, 64, DEV), None, cull)
    m.texture = texture.bake(m, _field(A, b), block=B, snap=0.0)
    cam = raster.look_at_box(*box, 64, DEV)
    out = m.render(cam, None, cull)                              # delegates to render_textured
    assert set(out) == set(plain) | {"uv"} and out["uv"].shape == (64, 64, 2)
    corners = m.verts[m.faces.long()].reshape(-1, 3)
    frame = raster.rasterize(corners, torch.arange(len(corners), dtype=torch.int32, device=DEV).reshape(-1, 3), cam, corners, cull)
    torch.cuda.synchronize()
    assert torch.equal(out["face_id"], plain["face_id"]) and torch.equal(out["depth"], plain["depth"]) and torch.equal(out["mask"], plain["mask"])
    assert torch.equal(out["normal8"], plain["normal8"]) and torch.equal(out["shaded8"], plain["shaded8"])
    assert torch.equal(frame.face_id, out["face_id"])
    mask = _np(out["mask"])
    assert mask.sum() > 500
    rgb = _np(texture.sample(m.texture, out["uv"], out["mask"]))
    want = _np(frame.attrs).astype(np.float64) @ A.T + b
    err = np.abs(rgb - want)[mask]
    print("B = %d, %d faces: %d covered pixels, largest colour error %.3e (half a texel: 0.02)" % (B, len(f), mask.sum(), err.max()))
    assert err.max() <= 0.002
    assert not rgb[~mask].any() and not _np(out["uv"])[~mask].any()
    # the 8-bit picture is that colour quantised as ia_pack_rgba8 quantises, alpha = covered
    q = (np.clip(rgb, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)
    rgba = _np(out["rgba8"])
    assert np.array_equal(rgba[..., :3], q) and np.array_equal(rgba[..., 3], np.where(mask, 255, 0))


@pytest.mark.parametrize("B", [4, 8])
def test_textured_picture_of_a_quad(B):
    v = np.float32([[-0.4, -0.4, 0], [0.4, -0.4, 0], [0.4, 0.4, 0], [-0.4, 0.4, 0]])
    f = np.int32([[0, 2, 1], [0, 3, 2]])                         # normal -z: towards the camera of look_at_box
    _pictures_show_the_field(v, f, B, (np.float32([-0.5] * 3), np.float32([0.5] * 3)), cull=False)


def test_textured_picture_of_the_sphere(sphere):
    v, f, _ = sphere
    _pictures_show_the_field(v, f, 8, (np.float32([-0.6] * 3), np.float32([0.6] * 3)), cull=True)


def test_faces_the_rasteriser_skips_are_skipped_with_a_texture_too(sphere):
    from instantavatar_amd import raster, texture
    v, f, _ = sphere
    v = np.concatenate([v, np.float32([[np.nan, 0, 0]])])
    f = np.concatenate([np.int32([[0, 1, len(v) - 1], [0, 1, len(v)], [-1, 2, 3]]), f])
    m = _mesh(v, f)
    m.normals = torch.nan_to_num(m.verts / m.verts.norm(dim=1, keepdim=True)).contiguous()
    cam = raster.look_at_box(np.float32([-0.6] * 3), np.float32([0.6] * 3), 64, DEV)
    plain = raster.render(m, cam)
    m.texture = texture.bake(m, _field(np.eye(3), np.full(3, 0.5)), block=5)
    out = raster.render_textured(m, cam)
    torch.cuda.synchronize()
    assert torch.equal(out["face_id"], plain["face_id"]) and torch.equal(out["depth"], plain["depth"])
    assert int(out["face_id"].max()) > 2 and not bool(((out["face_id"] >= 0) & (out["face_id"] < 3)).any())
    owner_alpha = _np(m.texture.rgba8)[..., 3]
    own = tx.texel_points(v, f, 5)["owner"].reshape(owner_alpha.shape)
    assert np.array_equal(owner_alpha != 0, own >= 0) and np.isfinite(_np(m.texture.atlas)).all()


# ---- the synthetic model -------------------------------------------------------------------------------------------------------------
def _parse_obj(path):
    out = {"v": [], "vn": [], "vt": [], "f": [], "mtllib": None, "usemtl": None}
    for line in open(path):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] in ("v", "vn", "vt"):
            out[w[0]].append([float(x) for x in w[1:]])
        elif w[0] == "f":
            out["f"].append([[int(x) for x in c.split("/")] for c in w[1:]])
        elif w[0] in ("mtllib", "usemtl"):
            out[w[0]] = w[1]
    return {k: (np.array(x) if isinstance(x, list) else x) for k, x in out.items()}


def test_bake_the_model_mesh_pose_it_and_write_it(tmp_path):
    import world
    from PIL import Image
    from instantavatar_amd import mesh as M, raster
    from instantavatar_amd.pipeline import make_batch
    model = world.build(DEV, 64, 16)[0]
    base = model.extract_mesh(resolution=64)
    lo, hi = M.field_box(model.net_coarse)
    small = model.simplify_mesh(base, 4 * float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / 63)
    assert base.texture is None and small.texture is None
    out = model.bake_texture(small, block=8)
    tex = out.texture
    nf = small.faces.shape[0]
    T = tx.atlas_size(nf, 8)
    torch.cuda.synchronize()
    assert small.texture is None and out.verts is small.verts and out.faces is small.faces
    assert tex.size == T and tex.atlas.shape == (T, T, 3) and tex.uv.shape == (nf, 3, 2)
    owned = int((tex.rgba8[..., 3] != 0).sum())
    assert owned == int((tx.texel_owner(nf, 8)[0] >= 0).sum())
    print("synthetic model at resolution 64, simplify 4: %d faces, atlas %d^2, %d of %d owned texels unsnapped (%.2f %%)"
          % (nf, T, int(tex.unsnapped), owned, 100.0 * int(tex.unsnapped) / owned))
    assert 0 <= int(tex.unsnapped) <= owned
    a = _np(tex.atlas)
    assert np.isfinite(a).all() and a.min() >= 0 and a.max() <= 1 and a.std() > 0
    assert torch.equal(model.bake_texture(small, block=8).texture.atlas, tex.atlas)
    # pose keeps the texture, smooth and simplify drop it
    poses, tr = world.poses(8)
    posed = model.pose_mesh(out, make_batch(DEV, 8, poses[5], tr[5]))
    assert posed.texture is tex and posed.faces is out.faces
    assert model.smooth_mesh(out, 1).texture is None and out.simplify(0.2).texture is None
    img = out.render(raster.look_at_box(lo, hi, 64, DEV))
    assert "uv" in img and int(img["mask"].sum()) > 50 and "uv" not in small.render(raster.look_at_box(lo, hi, 64, DEV))
    # the three files
    out.to_obj_textured(str(tmp_path / "a.obj"))
    assert sorted(os.listdir(tmp_path)) == ["a.mtl", "a.obj", "a.png"]
    obj = _parse_obj(str(tmp_path / "a.obj"))
    assert obj["mtllib"] == "a.mtl" and obj["usemtl"] == "avatar"
    assert obj["vt"].shape == (3 * nf, 2) and obj["vt"].min() >= 0 and obj["vt"].max() <= 1
    assert obj["v"].shape == (small.verts.shape[0], 3) and obj["vn"].shape == obj["v"].shape and obj["f"].shape == (nf, 3, 3)
    assert np.array_equal(obj["f"][..., 0] - 1, _np(small.faces)) and np.array_equal(obj["f"][..., 2], obj["f"][..., 0])
    assert np.array_equal(obj["f"][..., 1].reshape(-1), np.arange(3 * nf) + 1)
    assert np.abs(obj["vt"].reshape(nf, 3, 2) - tex.vt()).max() < 1e-8
    mtl = open(tmp_path / "a.mtl").read()
    assert "newmtl avatar" in mtl and "map_Kd a.png" in mtl
    png = Image.open(tmp_path / "a.png")
    assert png.size == (T, T) and png.mode == "RGB"
    assert np.array_equal(np.asarray(png), _np(tex.rgba8)[..., 2::-1])
    posed.to_obj_textured(str(tmp_path / "p.obj"), mtllib="a.mtl")
    assert sorted(os.listdir(tmp_path)) == ["a.mtl", "a.obj", "a.png", "p.obj"] and _parse_obj(str(tmp_path / "p.obj"))["mtllib"] == "a.mtl"


def test_extract_mesh_driver_with_and_without_a_texture(tmp_path, capsys):
    import re
    import world
    from PIL import Image
    from instantavatar_amd.drivers import extract_mesh as drv
    poses, tr = world.poses(8)
    np.savez(tmp_path / "track.npz", poses=poses[:2], trans=tr[:2])
    common = ["--synthetic", "--resolution", "48", "--simplify", "4", "--poses", str(tmp_path / "track.npz"), "--render", "64"]
    assert drv.main(common + ["--out", str(tmp_path / "plain")]) == 0
    said = capsys.readouterr().out
    # what the driver wrote before it knew of textures
    before = sorted(["canonical.ply", "canonical_front.png"] + ["%s%d.%s" % (p, i, e) for i in range(2) for p, e in (("posed_", "ply"), ("posed_", "png"), ("posed_shaded_", "png"))])
    assert sorted(os.listdir(tmp_path / "plain")) == before and "texture" not in said
    assert drv.main(common + ["--texture", "8", "--out", str(tmp_path / "tex")]) == 0
    said = capsys.readouterr().out
    new = ["canonical_textured.obj", "canonical_textured.mtl", "canonical_textured.png", "canonical_front_textured.png",
           "posed_0_textured.obj", "posed_1_textured.obj", "posed_textured_0.png", "posed_textured_1.png"]
    assert sorted(os.listdir(tmp_path / "tex")) == sorted(before + new)
    for name in before:
        assert open(tmp_path / "plain" / name, "rb").read() == open(tmp_path / "tex" / name, "rb").read(), name
    m = re.search(r"texture: atlas (\d+) x \1 texels in blocks of 8, snap [\d.e+-]+, (\d+) of (\d+) owned texels \(([\d.]+) %\) without", said)
    assert m, said[-2000:]
    T, miss, owned = int(m.group(1)), int(m.group(2)), int(m.group(3))
    assert Image.open(tmp_path / "tex" / "canonical_textured.png").size == (T, T) and 0 <= miss <= owned
    canon, posed = _parse_obj(str(tmp_path / "tex" / "canonical_textured.obj")), _parse_obj(str(tmp_path / "tex" / "posed_1_textured.obj"))
    assert canon["mtllib"] == posed["mtllib"] == "canonical_textured.mtl"
    assert np.array_equal(canon["vt"], posed["vt"]) and np.array_equal(canon["f"], posed["f"]) and not np.array_equal(canon["v"], posed["v"])
    assert T == tx.atlas_size(len(canon["f"]), 8) and owned == int((tx.texel_owner(len(canon["f"]), 8)[0] >= 0).sum())
    front = np.asarray(Image.open(tmp_path / "tex" / "canonical_front_textured.png"))
    plain = np.asarray(Image.open(tmp_path / "tex" / "canonical_front.png"))
    assert front.shape == (64, 64, 4) and np.array_equal(front[..., 3], plain[..., 3]) and (front[..., 3] != 0).sum() > 50
