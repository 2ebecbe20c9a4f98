"""`ia_scene_receive` (csrc/ia_scene.hip, include/instantavatar_hip_scene_receive.h) against tests/scene_receive_refs.py on the inputs
of tests/scene_receive_cases.py (both held to their own conditions in tests/test_cpu_scene_receive_refs.py), then
`instantavatar_amd.scene` and the driver end to end on the synthetic two-avatar scene of tests/test_gpu_scene.py (its helpers, its
SIZE = 32, shadow maps of 64^2, one fixed occupancy jitter).

Bounds.  The definition is separate IEEE operations in a fixed order on both sides, so on `clear` pixel-layers (no discrete choice
within 2^-40 of flipping, see the reference) shade and c_out are compared as BYTES; on the others a tap may fall on the other side,
which moves a factor of the product by at most `strength`: |shade - ref| <= strength.  Nothing here is a tolerance to widen."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_receive_cases as cases
import scene_receive_refs as srr
import test_gpu_scene as tgs

pytestmark = pytest.mark.gpu
DEV = tgs.DEV
ROOT = tgs.ROOT
SIZE = tgs.SIZE
NAN = float("nan")


def _dev(x):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(DEV)


def run_receive(case, fill=NAN, **override):
    """-> (shade [K,R], c_out [K,R,3]) as numpy arrays; outputs pre-filled with `fill`"""
    from instantavatar_amd import _lib
    p = dict(case, **override)
    K, R, S = p["K"], p["R"], p["S"]
    c_out, shade = torch.full((K, R, 3), fill, device=DEV), torch.full((K, R), fill, device=DEV)
    try:
        _lib.call("ia_scene_receive", _dev(p["rays_o"]), _dev(p["rays_d"]), R, _dev(p["c"]), _dev(p["a"]), _dev(p["d"]), _dev(p["nrm"]),
                  _dev(p["maps_a"]), _dev(p["maps_d"]), _dev(p["proj"]), K, S, *[float(v) for v in p["light"]], int(p["radius"]),
                  float(p["strength"]), float(p["near"]), float(p["bias_other"]), float(p["bias_self"]), float(p["cos0"]), float(p["cos1"]),
                  c_out, shade)
    finally:
        torch.cuda.synchronize()
        run_receive.last = (shade.cpu().numpy(), c_out.cpu().numpy())
    return run_receive.last


def _compare(shade, c_out, ref, c_in, strength, what):
    """the comparison of the module docstring; prints its figures before it asserts"""
    rec, clear = ref["receives"], ref["clear"]
    same_shade = shade.view(np.uint32) == ref["shade"].view(np.uint32)
    same_c = (c_out.view(np.uint32) == ref["c_out"].view(np.uint32)).all(-1)
    diff = np.abs(shade.astype(np.float64) - ref["shade"].astype(np.float64))
    print("%s: %d pixel-layers, %d receive, %d unclear; shade differs in %d (max %.3g), c_out in %d"
          % (what, rec.size, rec.sum(), (~clear).sum(), (~same_shade).sum(), float(diff.max()), (~same_c).sum()))
    assert same_shade[clear].all() and same_c[clear].all()
    assert (diff[~clear] <= float(strength)).all()
    assert (shade[~rec] == 1).all() and c_out[~rec].tobytes() == np.ascontiguousarray(c_in[~rec]).tobytes()      # bit for bit, NaNs included


# ---- 1. the kernel against the reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_receive_against_the_reference(name):
    case, ref = cases.case_and_reference(name)
    shade, c_out = run_receive(case)
    assert not np.isnan(shade).any()                                                   # every shade written
    assert not np.isnan(c_out[ref["receives"]]).any() and np.array_equal(np.isnan(c_out), np.isnan(case["c"]))
    _compare(shade, c_out, ref, case["c"], case["strength"], name)
    again = run_receive(case, fill=-1.0)
    assert again[0].tobytes() == shade.tobytes() and again[1].tobytes() == c_out.tobytes()


# ---- 2. bad arguments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("override, message", [
    (dict(K=0), "K = 0 outside"), (dict(K=9), "K = 9 outside"), (dict(radius=4), "PCF radius 4"), (dict(S=0), "S = 0 outside"),
    (dict(strength=1.5), "strength"), (dict(cos0=0.25, cos1=0.25), "cos0"), (dict(cos0=0.5, cos1=0.25), "cos0"),
    (dict(bias_other=-0.01), "biases"), (dict(bias_self=-0.01), "biases"), (dict(maps_d=None), "null pointer"), (dict(maps_a=None), "null pointer"),
    (dict(near=0.0), "near"), (dict(light=(NAN, 0.0, 0.0)), "light"), (dict(radius=-1), "PCF radius -1"), (dict(cos0=-1.5), "cos0"),
    (dict(bias_self=float("inf")), "biases")])
def test_receive_rejects_bad_arguments_and_writes_nothing(override, message):
    from instantavatar_amd import _lib
    case = cases.make_one_ray()
    with pytest.raises(_lib.IAError, match=message):
        run_receive(case, **override)
    shade, c_out = run_receive.last
    assert np.isnan(shade).all() and np.isnan(c_out).all()


# ---- 3. nothing else moved -----------------------------------------------------------------------------------------------------------------
def _two(offsets, frames=4):
    return [tgs._model(42), tgs._model(43)], [tgs._seq(offsets[0], frames), tgs._seq(offsets[1], frames)]


def test_receive_with_strength_zero_returns_the_bytes_of_a_scene_without_it():
    from instantavatar_amd import scene
    models, seqs = _two(((-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)))
    ground = scene.ground_under(models, seqs, color2=(0.4, 0.4, 0.4), cell=0.5)
    opts = dict(ground=ground, light=(-2.0, -4.0, 2.0), shadow_size=64, jitter=tgs._jitter(), shadow_strength=0.0)
    plain = scene.Scene(models, seqs, receive=False, **opts).render(1)
    with_it = scene.Scene(models, seqs, receive=True, **opts).render(1)
    assert "layer_shade" not in plain and sorted(plain) == ["alpha", "contested", "depth", "rgb", "rgba8", "shade"]
    for key in ("rgb", "alpha", "depth", "rgba8", "shade"):
        assert torch.equal(plain[key], with_it[key]), key
    assert with_it["layer_shade"].shape == (2, SIZE, SIZE) and bool((with_it["layer_shade"] == 1).all())
    assert float(plain["alpha"].max()) == 1.0 and float(plain["rgb"].max()) > 0.1


def test_receive_needs_a_light():
    from instantavatar_amd import _lib, scene
    models, seqs = _two(((-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)))
    with pytest.raises(_lib.IAError, match="needs a light"):
        scene.Scene(models, seqs, receive=True)
    s = scene.Scene(models, seqs, receive=True, light=(-2.0, -4.0, 2.0))
    assert s.lit and not s.shadows and not scene.Scene(models, seqs, light=(-2.0, -4.0, 2.0)).lit


# ---- 4. end to end: one avatar shadows the other ------------------------------------------------------------------------------------------
def _render_spied(monkeypatch, sc, i):
    """sc.render(i) and the arguments `composite` was given"""
    from instantavatar_amd import scene
    seen = {}
    real = scene.composite

    def spy(layers, rays_o, rays_d, **kw):
        seen.update(layers=layers, rays_o=rays_o, rays_d=rays_d, **kw)
        return real(layers, rays_o, rays_d, **kw)
    monkeypatch.setattr(scene, "composite", spy)
    out = sc.render(i)
    monkeypatch.setattr(scene, "composite", real)
    return out, seen


def _reference_of(seen):
    from instantavatar_amd import scene
    h = lambda t: t.detach().float().cpu().numpy()
    rc = seen["receive"]
    K = len(seen["layers"])
    R = seen["layers"][0][1].numel()
    nrm = None if rc["normals"] is None else np.stack([h(n).reshape(R, 3) for n in rc["normals"]])
    return srr.receive(h(seen["rays_o"]).reshape(R, 3), h(seen["rays_d"]).reshape(R, 3), np.stack([h(l[0]).reshape(R, 3) for l in seen["layers"]]),
                       np.stack([h(l[1]).reshape(R) for l in seen["layers"]]), np.stack([h(l[2]).reshape(R) for l in seen["layers"]]), nrm,
                       h(rc["maps_a"]), h(rc["maps_d"]), np.stack([scene.light_rays_projection(cm) for cm in rc["cams"]]), rc["light"],
                       radius=rc["radius"], strength=rc["strength"], near=min(cm.near for cm in rc["cams"]), bias_other=rc["bias_other"],
                       bias_self=rc["bias_self"]), K, R


def test_an_avatar_between_the_light_and_another_shadows_it(monkeypatch):
    from instantavatar_amd import scene
    models, seqs = _two(((-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)))
    roots = [s.transl[1].double().cpu().numpy() for s in seqs]
    along = (roots[1] - roots[0]) / np.linalg.norm(roots[1] - roots[0])
    assert abs(np.linalg.norm(roots[1] - roots[0]) - 1.0) < 1e-5                       # one metre apart
    means = {}
    for side, light in (("left", roots[0] - 2.0 * along), ("right", roots[1] + 2.0 * along)):
        sc = scene.Scene(models, seqs, light=light, shadow_size=64, jitter=tgs._jitter(), receive=True)
        out, seen = _render_spied(monkeypatch, sc, 1)
        ref, K, R = _reference_of(seen)
        assert out["shade"] is None and seen["receive"]["normals"] is not None
        got = out["layer_shade"].cpu().numpy().reshape(K, R)
        clear = ref["clear"]
        same = got.view(np.uint32) == ref["shade"].view(np.uint32)
        print("%s: %d of %d pixel-layers unclear, shade differs in %d" % (side, (~clear).sum(), K * R, (~same).sum()))
        assert (~clear).sum() <= 0.01 * K * R and same[clear].all()
        alpha = np.stack([l[1].cpu().numpy().reshape(R) for l in seen["layers"]])
        solid = alpha >= 0.5
        assert solid[0].sum() > 20 and solid[1].sum() > 20
        means[side] = [float(got[k][solid[k]].mean()) for k in range(2)]
        if side == "left":
            flat = scene.Scene(models, seqs, light=light, shadow_size=64, jitter=tgs._jitter(), receive=True, receive_normals=False)
            out_flat, seen_flat = _render_spied(monkeypatch, flat, 1)
            assert seen_flat["receive"]["normals"] is None
            near_flat = float(out_flat["layer_shade"].cpu().numpy().reshape(K, R)[0][solid[0]].mean())
            print("near avatar, mean shade: %.4f with the facing term, %.4f without" % (means[side][0], near_flat))
            assert near_flat >= means[side][0]
    print("mean shade (avatar 0, avatar 1): light on the left %s, on the right %s" % (means["left"], means["right"]))
    assert means["left"][1] < means["left"][0]                                         # the far one is darker ...
    assert means["right"][0] < means["right"][1]                                       # ... whichever end the light stands at


# ---- 5. the light view measures what the receiver measures: metres from the light --------------------------------------------------------
def test_a_lit_surface_finds_itself_in_its_own_light_view():
    """The pixels of one avatar that the camera sees solid (alpha >= 0.99) and that face the light (cosv > cos1): X from the camera's
    depth, projected into the avatar's own light view, lands on the body (m >= 0.5 at the nearest tap, for 90 % at least) at the
    distance the light view recorded -- median |rho - s / m| below bias_self.  If the second fails the default bias is wrong for this
    model."""
    from instantavatar_amd import scene
    model, seq = tgs._model(42), tgs._seq()
    root = seq.transl[1].double().cpu().numpy()
    light = root + np.array([-0.3, -0.5, -2.0])                                        # in front of it, a little up and to the side
    sc = scene.Scene([model], [seq], light=light, shadow_size=64, jitter=tgs._jitter(), receive=True)
    batch = seq.batch(1)
    batch["bg_color"] = sc._zero_bg
    with torch.no_grad():
        rgb, depth, alpha, _, nrm = model.render_image_fast(batch, (SIZE, SIZE), jitter=tgs._jitter(), normals=True)
    m, s, cam = sc.light_view_maps(0, 1, batch)
    h = lambda t: t.detach().double().cpu().numpy()
    a, d, n = h(alpha).reshape(-1), h(depth).reshape(-1), h(nrm).reshape(-1, 3)
    o, dr = h(seq.rays_o).reshape(-1, 3), h(seq.rays_d).reshape(-1, 3)
    m, s = h(m), h(s)
    with np.errstate(all="ignore"):
        X = o + (d / a)[:, None] * dr
        l = light[None] - X
        rho = np.linalg.norm(l, axis=1)
        cosv = (n * l).sum(1) / rho
        pick = (a >= 0.99) & (cosv > 0.25)
    assert pick.sum() > 20
    P = scene.light_rays_projection(cam).astype(np.float64)
    x = X[pick] @ P[:, :3].T + P[:, 3]
    u, v = x[:, 0] / x[:, 2], x[:, 1] / x[:, 2]
    assert (x[:, 2] > cam.near).all() and (u >= 0).all() and (u <= 63).all() and (v >= 0).all() and (v <= 63).all()
    ui, vi = np.floor(u + 0.5).astype(int), np.floor(v + 0.5).astype(int)
    on_body = m[vi, ui] >= 0.5
    print("%d lit solid pixels, %.1f %% of them on the body in the light view" % (pick.sum(), 100.0 * on_body.mean()))
    assert on_body.mean() >= 0.9
    gap = np.abs(rho[pick][on_body] - s[vi, ui][on_body] / m[vi, ui][on_body])
    print("median |rho - s / m| = %.4f m (90th percentile %.4f m); bias_self = %.2f m" % (np.median(gap), np.percentile(gap, 90), sc.bias_self))
    assert np.median(gap) < sc.bias_self


# ---- 6. the driver -------------------------------------------------------------------------------------------------------------------------
def _drive(extra, out):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "instantavatar_amd.drivers.scene", "--synthetic", "--seeds", "42", "43", "--size", "32", "--max-frames", "2",
           "--receive-shadows", "--jitter-seed", "1", "--no-gif", "--out", out] + extra
    return subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)


def test_scene_driver_receives_shadows_reproducibly(tmp_path):
    outs = []
    for name in ("one", "two"):
        out = str(tmp_path / name)
        r = _drive(["--light", "-2", "-4", "2"], out)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "avatar pixels in shadow:" in r.stdout and "frames/s" in r.stdout
        assert sorted(os.listdir(out)) == ["0.png", "1.png"]
        outs.append(out)
    for f in ("0.png", "1.png"):
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f


def test_scene_driver_asks_for_a_light(tmp_path):
    r = _drive([], str(tmp_path / "none"))
    assert r.returncode != 0 and "--receive-shadows needs --light" in r.stderr and "Traceback" not in r.stderr
