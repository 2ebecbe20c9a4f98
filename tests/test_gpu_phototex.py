"""csrc/ia_phototex.hip against tests/phototex_refs.py (float64 numpy, validated in tests/test_cpu_phototex_refs.py): the entry
points at the smallest shapes where they can go wrong, with depth maps GIVEN to both sides; byte equality across every way of
splitting the work; whole bakes through `phototex.bake` with the real rasteriser on a convex mesh, where the result is known
without a reference; then `AvatarModel.bake_photo_texture` and the extract_mesh driver on the synthetic model.

Tolerances.  Decisions and `seen` are compared exactly on every texel-frame pair that the reference DECIDES (no margin below 1e-9
relative, see phototex_refs); at most 1 % of the owned pairs may be undecided (measured on the committed scenes: none).  The atlas
holds fp32(S / W) with S / W in [0, 1]: both sides round an fp64 quotient once and the kernel's fp64 error is orders of magnitude
smaller, so 4 fp32 ulps of 1 (4.8e-7); a constant colour comes back to 1 ulp of itself."""
import functools
import os

import numpy as np
import pytest
import torch

import phototex_refs as pr
import texture_refs as tx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ULP1 = float(np.spacing(np.float32(1)))
TOL = 4 * ULP1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _mesh(v, f):
    from instantavatar_amd.mesh import Mesh
    nv = len(v)
    return Mesh(_dev(v, torch.float32).reshape(-1, 3), _dev(f, torch.int32).reshape(-1, 3), torch.zeros((nv, 3), device=DEV),
                torch.zeros((nv, 3), device=DEV))


def run_entries(case, B, frame_chunks, texel_ranges, base=None, min_frames=1, options=pr.KERNEL_OPTIONS):
    """the three entry points alone: zero, one accumulate per (chunk of frames, range of texels), resolve.
    -> (atlas [n,3], seen [n], unseen, the accumulator's bytes) as numpy"""
    from instantavatar_amd import _lib
    verts, faces = _dev(case["verts"], torch.float32), _dev(case["faces"], torch.int32)
    nv, nf = verts.shape[0], faces.shape[0]
    T = tx.atlas_size(nf, B)
    n = T * T
    fx, fy, cx, cy, near = case["intr"]
    H, W = case["images"].shape[1:3]
    stride = _lib.call("ia_phototex_acc_bytes", 1)
    acc = torch.full((_lib.call("ia_phototex_acc_bytes", n),), 0xA5, dtype=torch.uint8, device=DEV)
    _lib.call("ia_phototex_zero", acc, n)
    for f0, f1 in frame_chunks:
        posed, w2c = _dev(case["posed"][f0:f1], torch.float32), _dev(case["w2c"][f0:f1], torch.float32)
        images, depth = _dev(case["images"][f0:f1]), _dev(case["depth"][f0:f1], torch.float32)
        masks = None if case["masks"] is None else _dev(case["masks"][f0:f1], torch.float32)
        for first, count in texel_ranges(n):
            _lib.call("ia_phototex_accumulate", posed, nv, faces, nf, B, T, first, count, f1 - f0, w2c, fx, fy, cx, cy, near, images, masks,
                      depth, H, W, options["cos_min"], options["power"], options["depth_tol"], acc[first * stride:(first + count) * stride])
    pts, owner = torch.empty((n, 3), device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    _lib.call("ia_tex_texel_points", verts, nv, faces, nf, B, T, 0, n, None, 0.0, pts, None, owner)
    atlas = torch.full((n, 3), float("nan"), device=DEV)
    seen = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    unseen = torch.zeros((), dtype=torch.int32, device=DEV)
    for first, count in texel_ranges(n):
        _lib.call("ia_phototex_resolve", acc[first * stride:(first + count) * stride], None if base is None else base[first:first + count],
                  owner[first:first + count], count, min_frames, atlas[first:first + count], seen[first:first + count], unseen)
    torch.cuda.synchronize()
    return _np(atlas), _np(seen), int(unseen), _np(acc)


whole = lambda n: [(0, n)]


def pieces(n):
    """ranges whose boundaries are no multiples of 64 (nor of a row of the atlas), the last one short"""
    out, first, k = [], 0, 0
    while first < n:
        count = min((37, 101, 5, 250)[k % 4], n - first)
        out.append((first, count))
        first, k = first + count, k + 1
    return out


@functools.lru_cache(maxsize=None)
def kernel_ref(nf, B, F):
    case = pr.kernel_case(nf, B, F)
    T = tx.atlas_size(nf, B)
    base = np.random.RandomState(nf + B + F).rand(T * T, 3).astype(np.float32)
    return case, base, pr.bake(case["verts"], case["faces"], B, case["frames"], base=base, **pr.KERNEL_OPTIONS)


@pytest.mark.parametrize("nf,B,F", pr.KERNEL_CASES)
def test_kernel_against_the_reference(nf, B, F):
    case, base, ref = kernel_ref(nf, B, F)
    own = ref["owner"].reshape(-1) >= 0
    undecided = int((~ref["decided"][:, own]).sum())
    print("nf %d B %d F %d: %d owned texels, %d of %d pairs accepted, %d undecided" % (nf, B, F, own.sum(), ref["ok"].sum(), F * own.sum(), undecided))
    assert undecided <= 0.01 * F * own.sum()
    # the decision of every frame alone: a fresh accumulator per frame, seen is 0 or 1
    for f in range(F):
        seen_f = run_entries(case, B, [(f, f + 1)], whole)[1]
        assert set(np.unique(seen_f).tolist()) <= {0, 1}
        d = ref["decided"][f]
        assert np.array_equal(seen_f[d] == 1, ref["ok"][f][d]), (f, np.flatnonzero((seen_f == 1) != ref["ok"][f]))
    atlas, seen, unseen, _ = run_entries(case, B, [(0, F)], whole, base=_dev(base))
    sure = ref["decided"].all(0)
    assert np.array_equal(seen[sure], ref["seen"].reshape(-1)[sure])
    err = np.abs(atlas.astype(np.float64) - ref["atlas"].reshape(-1, 3))[sure]
    print("  atlas: max error %.3g (bound %.3g) over %d texels, %d seen" % (err.max(), TOL, sure.sum(), (seen > 0).sum()))
    assert err.max() <= TOL
    assert (atlas[~own] == 0).all() and (seen[~own] == 0).all()
    never = own & (seen == 0)
    assert np.array_equal(atlas[never], base[never])                      # the fallback, byte for byte
    if sure.all():
        assert unseen == ref["unseen"]


def test_min_frames_and_a_missing_base():
    case, base, ref = kernel_ref(20, 8, 3)
    want = pr.bake(case["verts"], case["faces"], 8, case["frames"], base=None, min_frames=2, **pr.KERNEL_OPTIONS)
    atlas, seen, unseen, _ = run_entries(case, 8, [(0, 3)], whole, base=None, min_frames=2)
    sure = want["decided"].all(0)
    assert (seen == 1).any() and (seen >= 2).any()
    assert np.array_equal(seen[sure], want["seen"].reshape(-1)[sure])
    assert np.abs(atlas.astype(np.float64) - want["atlas"].reshape(-1, 3))[sure].max() <= TOL
    assert (atlas[seen < 2] == 0).all() and unseen == want["unseen"]


@pytest.mark.parametrize("nf,B,F", [(20, 8, 3), (3, 5, 3), (20, 4, 3)])
def test_bytes_do_not_depend_on_how_the_work_is_split(nf, B, F):
    case, base, _ = kernel_ref(nf, B, F)
    b = _dev(base)
    one = run_entries(case, B, [(0, F)], whole, base=b)
    for name, chunks, ranges in (("a second identical call", [(0, F)], whole),
                                 ("one launch per frame", [(f, f + 1) for f in range(F)], whole),
                                 ("frames 2 + 1", [(0, 2), (2, 3)], whole),
                                 ("texel pieces", [(0, F)], pieces),
                                 ("frames and texels split", [(f, f + 1) for f in range(F)], pieces)):
        other = run_entries(case, B, chunks, ranges, base=b)
        assert np.array_equal(one[3], other[3]), name                    # the fp64 sums themselves
        assert one[0].tobytes() == other[0].tobytes() and np.array_equal(one[1], other[1]) and one[2] == other[2], name
    assert (one[1] > 0).any()


def test_masks_may_be_missing():
    case, _, _ = kernel_ref(20, 8, 3)
    bare = dict(case, masks=None, frames=[(p, w, i, im, None, d) for p, w, i, im, _, d in case["frames"]])
    want = pr.bake(bare["verts"], bare["faces"], 8, bare["frames"], **pr.KERNEL_OPTIONS)
    atlas, seen, unseen, _ = run_entries(bare, 8, [(0, 3)], whole)
    assert want["decided"].all() and np.array_equal(seen, want["seen"].reshape(-1)) and unseen == want["unseen"]
    assert seen.sum() > kernel_ref(20, 8, 3)[2]["seen"].sum()              # the holes of the masks had rejected some
    assert np.abs(atlas.astype(np.float64) - want["atlas"].reshape(-1, 3)).max() <= TOL


# ---- whole bakes with the real rasteriser ---------------------------------------------------------------------------------------------
SPH_H, SPH_W = 80, 96
SPH_COLOUR = np.array([37, 190, 101], np.uint8)


def sphere_ramp():
    j, i = np.meshgrid(np.arange(SPH_H), np.arange(SPH_W), indexing="ij")
    return np.stack([5 + 2 * i, 240 - i - j, 20 + 2 * j], -1).astype(np.uint8)


def sphere_ramp_at(u, v):
    return np.stack([5 + 2 * u, 240 - u - v, 20 + 2 * v], -1) / 255.0


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """an octasphere of 128 faces (convex) seen by four cameras around it; depth maps by `raster.rasterize`; the reference of the
    ramp-image bake on the same depth maps, computed once"""
    from instantavatar_amd import raster
    verts, faces = tx.octasphere(2, 0.5)
    mesh = _mesh(verts, faces)
    K = np.array([[140.0, 0, 47.5], [0, 140.0, 39.5], [0, 0, 1]])
    cams, depths = [], []
    for k in range(4):
        a = 2 * np.pi * k / 4 + 0.3
        w2c = pr.look_at((2.0 * np.sin(a), 0.4 * (-1) ** k, 2.0 * np.cos(a)), (0, 0, 0))
        cam = raster.Camera(K, _dev(w2c), SPH_H, SPH_W, near=0.05)
        cams.append(cam)
        depths.append(raster.rasterize(mesh.verts, mesh.faces, cam).depth)
    torch.cuda.synchronize()
    intr = lambda c: (c.fx, c.fy, c.cx, c.cy, c.near)
    frames = [(verts, _np(c.w2c), intr(c), sphere_ramp(), None, _np(d)) for c, d in zip(cams, depths)]
    T = tx.atlas_size(len(faces), 8)
    base = np.random.RandomState(3).rand(T, T, 3).astype(np.float32)
    ref = pr.bake(verts, faces, 8, frames, base=base)
    return mesh, cams, depths, base, ref


def sphere_bake(image, **kw):
    from instantavatar_amd import phototex
    mesh, cams, depths, base, _ = sphere_scene()
    img = _dev(image)
    ones = torch.ones((SPH_H, SPH_W), device=DEV)
    tex, seen = phototex.bake(mesh, ((mesh.verts, c, img, ones, d) for c, d in zip(cams, depths)), 8, base=_dev(base), **kw)
    torch.cuda.synchronize()
    return tex, seen


def test_a_constant_colour_comes_back_and_unseen_texels_keep_the_base():
    mesh, cams, depths, base, ref = sphere_scene()
    tex, seen = sphere_bake(np.broadcast_to(SPH_COLOUR, (SPH_H, SPH_W, 3)).copy(), chunk_frames=3, chunk=1000)
    atlas, seen = _np(tex.atlas), _np(seen)
    own = ref["owner"] >= 0
    assert tex.size == ref["size"] and tex.block == 8 and atlas.shape == (tex.size, tex.size, 3) and seen.dtype == np.int32
    assert np.array_equal(_np(tex.uv), tx.corner_uv(128, 8).astype(np.float32))
    assert np.array_equal(_np(tex.rgba8)[..., 3] != 0, own)
    c = (SPH_COLOUR.astype(np.float64) / 255).astype(np.float32)
    hit = seen > 0
    assert hit.sum() > 1000 and (own & ~hit).sum() > 0
    assert (np.abs(atlas[hit] - c) <= np.spacing(c)).all()
    assert np.array_equal(atlas[own & ~hit], base[own & ~hit]) and (atlas[~own] == 0).all()
    assert int(tex.unsnapped) == int(tex.unseen) == (own & ~hit).sum()
    assert ref["decided"].all() and np.array_equal(seen, ref["seen"])     # (the decisions do not depend on the image)


def test_a_ramp_image_comes_back_at_the_projected_points():
    mesh, cams, depths, base, ref = sphere_scene()
    tex, seen = sphere_bake(sphere_ramp())
    atlas, seen = _np(tex.atlas).reshape(-1, 3), _np(seen).reshape(-1)
    # from the reference only the projected points, the decisions and the weights are taken: the colour is the ramp there
    S, Wt = np.zeros((len(seen), 3)), np.zeros(len(seen))
    for r in ref["per_frame"]:
        S += np.where(r["ok"][:, None], r["weight"][:, None] * sphere_ramp_at(r["uv"][:, 0], r["uv"][:, 1]), 0)
        Wt += np.where(r["ok"], r["weight"], 0)
    hit = seen > 0
    assert np.array_equal(seen, ref["seen"].reshape(-1)) and hit.sum() > 1000
    err = np.abs(atlas[hit] - S[hit] / Wt[hit][:, None])
    print("ramp: max error %.3g (bound %.3g) over %d seen texels" % (err.max(), TOL, hit.sum()))
    assert err.max() <= TOL
    assert np.abs(atlas.astype(np.float64) - ref["atlas"].reshape(-1, 3)).max() <= TOL


def test_what_faces_a_camera_of_a_convex_mesh_is_seen():
    """every owned non-gutter texel that a frame looks at with c > cos_min and whose footprint lies inside the image is seen in that
    frame, unless its footprint straddles the silhouette (or, at this resolution, a pixel of its footprint lies further than
    depth_tol away in depth on a steep face): the exceptions are counted and may not exceed the reference's on the same input"""
    from instantavatar_amd import phototex
    mesh, cams, depths, base, ref = sphere_scene()
    owner, w = pr.texel_weights(128, 8)
    inner = (owner >= 0) & (w >= 0).all(1)
    ones = torch.ones((SPH_H, SPH_W), device=DEV)
    img = _dev(sphere_ramp())
    missed = missed_ref = eligible = 0
    for k, r in enumerate(ref["per_frame"]):
        seen_k = _np(phototex.bake(mesh, [(mesh.verts, cams[k], img, ones, depths[k])], 8)[1]).reshape(-1)
        m = r["margins"]
        want = inner & (m["facing"] > 0) & (m["near"] > 0) & (np.minimum(np.minimum(m["left"], m["right"]), np.minimum(m["top"], m["bottom"])) > 0)
        eligible += int(want.sum())
        missed += int((want & (seen_k == 0)).sum())
        missed_ref += int((want & ~r["ok"]).sum())
        assert np.array_equal(seen_k == 1, r["ok"])
    print("convex mesh, 4 cameras: %d eligible texel-frame pairs, %d not seen (reference: %d)" % (eligible, missed, missed_ref))
    assert eligible > 2000 and missed <= missed_ref < 0.5 * eligible


def test_coverage_image():
    from instantavatar_amd import phototex
    mesh, cams, depths, base, ref = sphere_scene()
    seen = _dev(ref["seen"].astype(np.int32))
    owner = _dev(ref["owner"].astype(np.int32))
    img = _np(phototex.coverage_image(seen, owner))
    T = ref["size"]
    assert img.shape == (T, T, 4) and img.dtype == np.uint8
    assert np.array_equal(img[..., 3] != 0, ref["owner"] >= 0)
    top = ref["seen"].max()
    assert top >= 2
    own = ref["owner"] >= 0
    assert (img[own & (ref["seen"] == 0)][:, :3] == [0, 0, 255]).all()     # B, G, R: red where no frame saw the texel
    assert (img[own & (ref["seen"] == top)][:, :3] == [255, 0, 0]).all()   # blue at the largest count
    assert np.array_equal(img, _np(phototex.coverage_image(seen, owner >= 0, top=top)))


def test_bake_refuses_what_does_not_fit():
    from instantavatar_amd import _lib, phototex
    mesh, cams, depths, base, ref = sphere_scene()
    img = _dev(sphere_ramp())
    frame = (mesh.verts, cams[0], img, None, depths[0])
    for kw, what in ((dict(cos_min=1.0), "cos_min"), (dict(cos_min=-0.1), "cos_min"), (dict(power=-1.0), "power"), (dict(depth_tol=float("nan")), "depth_tol"),
                     (dict(min_frames=0), "min_frames"), (dict(base=torch.zeros((8, 8, 3), device=DEV)), "base atlas")):
        with pytest.raises(_lib.IAError, match=what):
            phototex.bake(mesh, [frame], 8, **kw)
    with pytest.raises(_lib.IAError, match="posed vertices"):
        phototex.bake(mesh, [(mesh.verts[:-1], cams[0], img, None, depths[0])], 8)
    with pytest.raises(_lib.IAError, match="uint8"):
        phototex.bake(mesh, [(mesh.verts, cams[0], img.float(), None, depths[0])], 8)
    with pytest.raises(_lib.IAError, match="depth map or mask"):
        phototex.bake(mesh, [(mesh.verts, cams[0], img, None, depths[0][:-1])], 8)
    tex, seen = phototex.bake(mesh, [], 8)                                 # no frames: nothing is seen, nothing is launched for them
    assert int(seen.max()) == 0 and float(tex.atlas.abs().max()) == 0 and int(tex.unseen) == int((ref["owner"] >= 0).sum())


def test_the_camera_of_a_loaded_sequence_projects_every_pixel_ray_back_onto_its_pixel(tmp_path):
    """`DeviceFrames.camera()` (K, c2w^-1) against the rays the same object trains with, on a directory whose extrinsic is no identity"""
    import sequence_fixture as fx
    from instantavatar_amd.datasets import sequence_dir as sd
    from instantavatar_amd.datasets.device_frames import DeviceFrames
    fx.write_sequence(tmp_path / "seq", "peoplesnapshot")
    frames = DeviceFrames.from_directory(sd.read_sequence(tmp_path / "seq", "peoplesnapshot", "train", dict(start=0, end=3, downscale=1)), None, DEV)
    cam = frames.camera()
    assert (cam.H, cam.W) == (frames.H, frames.W) and not torch.equal(cam.w2c, torch.eye(4, device=DEV))
    p = _np(frames.rays_o.reshape(cam.H, cam.W, 3) + 2.5 * frames.rays_d.reshape(cam.H, cam.W, 3)).astype(np.float64)
    w2c = _np(cam.w2c).astype(np.float64)
    x = p @ w2c[:3, :3].T + w2c[:3, 3]
    j, i = np.meshgrid(np.arange(cam.H), np.arange(cam.W), indexing="ij")
    assert (x[..., 2] > 0).all()
    assert np.abs(cam.fx * x[..., 0] / x[..., 2] + cam.cx - i).max() < 1e-3 and np.abs(cam.fy * x[..., 1] / x[..., 2] + cam.cy - j).max() < 1e-3


# ---- the synthetic model -------------------------------------------------------------------------------------------------------------
def _psnr(a, b, sel):
    mse = float(((a - b) ** 2)[sel].mean())
    return -10.0 * np.log10(mse)


def test_bake_photo_texture_of_the_model():
    """the photo texture of the synthetic model from 8 teacher frames through a full turn: layout, counts, fallback, and its quality at
    a held-out pose against the field-baked texture (the gate is PSNR_photo >= PSNR_field - 3 dB: a factor 2 in MSE, meant to catch
    a swapped channel, a flipped axis or a wrong pose; the figures are printed and kept in profiles/phototex_quality.txt)"""
    import world
    from instantavatar_amd import mesh as M
    from instantavatar_amd.drivers import eval as eval_driver
    model = world.build(DEV, 64, 16)[0]
    res, n_frames = 128, 8
    base_mesh = model.extract_mesh(resolution=64)
    lo, hi = M.field_box(model.net_coarse)
    small = model.simplify_mesh(base_mesh, 4 * float((hi.astype(np.float64) - lo.astype(np.float64)).max()) / 63)
    frames = eval_driver.synthetic_photo_set(DEV, model, res, n_frames)
    assert len(frames) == n_frames and frames.images.shape == (n_frames, res, res, 3) and frames.images.dtype == torch.uint8
    cam = frames.camera()
    assert (cam.H, cam.W) == (res, res) and torch.equal(cam.w2c, torch.eye(4, device=DEV))
    field = model.bake_texture(small, block=8)
    photo, seen = model.bake_photo_texture(small, frames, block=8)
    torch.cuda.synchronize()
    tex, ftex = photo.texture, field.texture
    assert small.texture is None and photo.verts is small.verts and photo.faces is small.faces
    assert (tex.size, tex.block) == (ftex.size, ftex.block) and torch.equal(tex.uv, ftex.uv) and torch.equal(tex.rgba8[..., 3], ftex.rgba8[..., 3])
    assert seen.shape == (tex.size, tex.size) and seen.dtype == torch.int32 and 0 <= int(seen.min()) and int(seen.max()) <= n_frames
    owned = tex.rgba8[..., 3] != 0
    unseen = owned & (seen == 0)
    assert torch.equal(tex.atlas[seen == 0], ftex.atlas[seen == 0])        # byte for byte the field-baked atlas
    share = float((owned & (seen > 0)).sum()) / float(owned.sum())
    assert share > 0 and int(tex.unseen) == int(unseen.sum())
    assert torch.equal(model.bake_photo_texture(small, frames, block=8, chunk_frames=3, chunk=777)[0].texture.atlas, tex.atlas)
    none = model.bake_photo_texture(small, frames, block=8, base=None)[0].texture
    assert float(none.atlas[seen == 0].abs().max()) == 0 and torch.equal(none.atlas[seen > 0], tex.atlas[seen > 0])
    # quality at a held-out pose, against the existing path
    held = eval_driver.synthetic_photo_set(DEV, model, res, n_frames, held_out=True)
    p = held.smpl_params
    k = 3
    pose72 = torch.cat([p["global_orient"][k], p["body_pose"][k]]).cpu().numpy()
    from instantavatar_amd.pipeline import make_batch
    batch = make_batch(DEV, res, pose72, p["transl"][k].cpu().numpy())
    with torch.no_grad():
        rgb, _, alpha, _ = model.render_image_fast(batch, (res, res))
    truth, alpha = rgb[0], alpha[0]
    psnr = {}
    for name, m in (("photo", photo), ("field", field)):
        img = model.pose_mesh(m, batch).render(cam)
        mask = img["rgba8"][..., 3] != 0
        inner = -torch.nn.functional.max_pool2d(-mask.float()[None, None], 5, 1, 2)[0, 0] > 0          # eroded by 2 pixels
        sel = inner & (alpha > 0.5)
        assert int(sel.sum()) > 200
        psnr[name] = _psnr(img["rgba8"][..., :3].float() / 255, truth, sel)
    line = ("synthetic model, resolution 64, simplify 4 (%d faces), block 8, %d teacher frames at %d^2 through a full turn: %.1f %% of the owned "
            "texels seen, at most %d frames per texel; held-out pose: PSNR photo texture %.2f dB, field texture %.2f dB"
            % (small.faces.shape[0], n_frames, res, 100 * share, int(seen.max()), psnr["photo"], psnr["field"]))
    print(line)
    path = os.path.join(ROOT, "profiles", "phototex_quality.txt")
    if not os.path.exists(path):
        try:
            with open(path, "w") as out:
                out.write(line + "\n")
        except OSError:
            pass                                                           # a read-only checkout: the line above was printed
    assert psnr["photo"] >= psnr["field"] - 3.0, psnr


def test_extract_mesh_driver_with_and_without_photo(tmp_path, capsys):
    import re
    from PIL import Image
    from instantavatar_amd.drivers import extract_mesh as drv
    common = ["--synthetic", "--resolution", "64", "--simplify", "4", "--texture", "8", "--render", "64", "--rig", "4"]
    assert drv.main(common + ["--out", str(tmp_path / "tex")]) == 0
    said = capsys.readouterr().out
    before = sorted(["canonical.ply", "canonical_textured.obj", "canonical_textured.mtl", "canonical_textured.png", "canonical_front.png",
                     "canonical_front_textured.png", "avatar.glb"])
    assert sorted(os.listdir(tmp_path / "tex")) == before and "photo" not in said
    assert drv.main(common + ["--photo", "--photo-frames", "4", "--photo-res", "96", "--out", str(tmp_path / "photo")]) == 0
    said = capsys.readouterr().out
    new = ["canonical_phototextured.obj", "canonical_phototextured.mtl", "canonical_phototextured.png", "coverage.png",
           "canonical_front_phototextured.png"]
    assert sorted(os.listdir(tmp_path / "photo")) == sorted(before + new)
    for name in before:
        same = open(tmp_path / "tex" / name, "rb").read() == open(tmp_path / "photo" / name, "rb").read()
        assert same == (name != "avatar.glb"), name                         # with --photo the glTF carries the photo texture
    assert "avatar.glb with" in said and ", photo-textured" in said
    front = np.asarray(Image.open(tmp_path / "photo" / "canonical_front_phototextured.png"))
    plain = np.asarray(Image.open(tmp_path / "photo" / "canonical_front_textured.png"))
    assert front.shape == (64, 64, 4) and np.array_equal(front[..., 3], plain[..., 3]) and not np.array_equal(front, plain)
    m = re.search(r"photo texture: 4 frames, (\d+) of (\d+) owned texels \(([\d.]+) %\) seen at least once, median (\d+) frames per seen texel", said)
    assert m, said[-2000:]
    n_seen, owned, median = int(m.group(1)), int(m.group(2)), int(m.group(4))
    assert 0 < n_seen <= owned and 1 <= median <= 4
    T = Image.open(tmp_path / "photo" / "canonical_textured.png").size[0]
    png, cov = Image.open(tmp_path / "photo" / "canonical_phototextured.png"), Image.open(tmp_path / "photo" / "coverage.png")
    assert png.size == (T, T) and png.mode == "RGB" and cov.size == (T, T) and cov.mode == "RGBA"
    assert (np.asarray(cov)[..., 3] != 0).sum() == owned
    assert not np.array_equal(np.asarray(png), np.asarray(Image.open(tmp_path / "photo" / "canonical_textured.png")))
    with pytest.raises(SystemExit) as e:
        drv.main(["--synthetic", "--photo", "--out", str(tmp_path / "no")])
    assert e.value.code == 2 and not os.path.exists(tmp_path / "no")
