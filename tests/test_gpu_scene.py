"""csrc/ia_scene.hip against tests/scene_refs.py (float64 numpy, validated in tests/test_cpu_scene_refs.py) on the inputs of
tests/scene_cases.py -- 5 x 7 and 33 x 65 pixels, K = 1, 2, 3, 8, layers that do not take part, exact ties, rejected rays, a
checker, the disc edge, PCF radii 0 .. 3 on maps of 4^2 and 17^2 -- then `instantavatar_amd.scene` and the driver end to end on the
synthetic model at 32 x 32 with one fixed occupancy jitter on both sides.

Preconditions (asserted from the reference's report): distinct keys of a pixel differ by more than 1e-3 relative and checker
coordinates lie more than 1e-4 cells from a border, so no discrete choice can flip between fp32 and fp64.

Bounds (derived, not tuned).  Colour, alpha and shade: absolute 5e-6 -- at most 10 fp32 steps (a product and a sum per contributor,
the background, the shade) on values in [0, 1], each within 2^-24 = 6e-8, with a factor of about four of slack; the shadow's taps
are three fp32 lerps each and their mean is taken in fp64.  depth, t_g and P: relative 5e-6 (the geometric part is fp64 on both
sides and rounded once; depth is the same fp32 chain on values of a few metres).  `contested` is exact; a second call gives the
same bytes.

`rgb_coarse` of `render_image_fast` is premultiplied only when the batch carries a zero `bg_color` (without one the renderer puts
the frame on white: C + T), so that is what both sides of the one-avatar test render with."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_cases as sc
import scene_refs as sr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABS, REL = 5e-6, 5e-6


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _close_rel(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    bound = REL * np.abs(want)
    print("%s: max relative error %.3g" % (what, float(np.max(err / np.maximum(np.abs(want), 1e-30))) if err.size else 0.0))
    assert (err <= bound).all(), (what, float(err.max()))


def _close_abs(got, want, what):
    err = np.abs(got.astype(np.float64) - want)
    print("%s: max absolute error %.3g" % (what, float(err.max()) if err.size else 0.0))
    assert (err <= ABS).all(), (what, float(err.max()))


# ---- the entry points -----------------------------------------------------------------------------------------------------------------
def run_composite(case, fill=float("nan")):
    from instantavatar_amd import _lib
    K, R = case["K"], case["R"]
    c, a, d = _dev(case["c"]), _dev(case["a"]), _dev(case["d"])
    g = [None] * 4 if case["ground"] is None else [_dev(x) for x in case["ground"]]
    bg = _dev(case["background"])
    rgb, alpha, depth = (torch.full(s, fill, device=DEV) for s in ((R, 3), (R,), (R,)))
    contested = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    _lib.call("ia_scene_zero", contested, 1)
    _lib.call("ia_scene_composite", c, a, d, K, R, *g, bg, int(bg is not None and bg.numel() == 3), case["contact"], rgb, alpha, depth, contested)
    torch.cuda.synchronize()
    return _np(rgb), _np(alpha), _np(depth), int(contested)


@pytest.mark.parametrize("name", sorted(sc.COMPOSITE))
def test_composite_against_the_reference(name):
    case = sc.COMPOSITE[name]()
    ref = sr.composite(case["c"], case["a"], case["d"], ground=case["ground"], background=case["background"], contact=case["contact"])
    assert ref["report"]["key_gap"] > 1e-3 and sc.contact_margin(case) > 1e-3                   # preconditions
    rgb, alpha, depth, contested = run_composite(case)
    assert np.isfinite(rgb).all() and np.isfinite(alpha).all() and np.isfinite(depth).all()      # every pixel written, no NaN let through
    _close_abs(rgb, ref["rgb"], "rgb")
    _close_abs(alpha, ref["alpha"], "alpha")
    _close_rel(depth, ref["depth"], "depth")
    assert contested == ref["contested"]
    if case["close"]:
        assert 0 < contested < case["R"]
    again = run_composite(case, fill=-1.0)
    assert again[0].tobytes() == rgb.tobytes() and again[1].tobytes() == alpha.tobytes() and again[2].tobytes() == depth.tobytes()
    assert again[3] == contested


def test_composite_accumulates_the_counter_and_rejects_bad_layer_counts():
    from instantavatar_amd import _lib
    case = sc.COMPOSITE["large_K2_close"]()
    K, R = case["K"], case["R"]
    c, a, d = _dev(case["c"]), _dev(case["a"]), _dev(case["d"])
    out = [torch.empty((R, 3), device=DEV), torch.empty(R, device=DEV), torch.empty(R, device=DEV)]
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    for _ in range(2):
        _lib.call("ia_scene_composite", c, a, d, K, R, None, None, None, None, None, 0, case["contact"], *out, counter)
    want = sr.composite(case["c"], case["a"], case["d"], contact=case["contact"])["contested"]
    assert int(counter) == 2 * want and want > 0
    for bad in (0, 9):
        with pytest.raises(_lib.IAError, match="K = %d outside" % bad):
            _lib.call("ia_scene_composite", c, a, d, bad, R, None, None, None, None, None, 0, case["contact"], *out, counter)
    from instantavatar_amd import scene
    layer = (out[0], out[1], out[2])
    for n in (0, 9):
        with pytest.raises(_lib.IAError, match="%d layers" % n):
            scene.composite([layer] * n, None, None)


def run_ground(case):
    from instantavatar_amd import _lib
    p = case["plane"]
    o, d = _dev(case["rays_o"]), _dev(case["rays_d"])
    R = o.shape[0]
    t_g, a_g, c_g, P = (torch.full(s, float("nan"), device=DEV) for s in ((R,), (R,), (R, 3), (R, 3)))
    _lib.call("ia_scene_ground", o, d, R, *[float(v) for v in p["normal"]], float(p["h"]), *p["g0"], *p["g1"], float(p["cell"]),
              *[float(v) for v in p["centre"]], p["r0"], p["r1"], t_g, a_g, c_g, P)
    torch.cuda.synchronize()
    return _np(t_g), _np(a_g), _np(c_g), _np(P)


@pytest.mark.parametrize("name", sorted(sc.GROUND))
def test_ground_against_the_reference(name):
    case = sc.GROUND[name]()
    ref = sr.ground(case["rays_o"], case["rays_d"], **case["plane"])
    assert ref["report"]["cell_margin"] > 1e-4                                                   # precondition
    hit = ref["hit"]
    assert hit.any() and (~hit[:4]).all()                                                        # the four rejected rays
    t_g, a_g, c_g, P = run_ground(case)
    assert np.array_equal(t_g != 0, hit)
    for arr in (t_g, a_g, c_g, P):
        assert (arr[~hit] == 0).all()
    _close_rel(t_g, ref["t_g"], "t_g")
    _close_rel(P, ref["P"], "P")
    _close_abs(a_g, ref["a_g"], "a_g")
    assert np.array_equal(c_g, ref["c_g"].astype(np.float32))                                    # one of the two colours, exactly
    if case["plane"]["cell"] > 0:
        assert len(np.unique(c_g[hit], axis=0)) == 2
    if case["plane"]["r1"] > case["plane"]["r0"]:
        assert (a_g[hit] == 0).any() and ((a_g > 0) & (a_g < 1)).any()                            # outside and on the ramp
        assert (a_g[hit] == 1).any() or case["plane"]["r0"] == 0                                  # inside
    again = run_ground(case)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, (t_g, a_g, c_g, P)))


def run_shadow(case):
    from instantavatar_amd import _lib
    P, a_g, maps, proj = _dev(case["P"]), _dev(case["a_g"]), _dev(case["maps"]), _dev(case["proj"])
    R = P.shape[0]
    shade = torch.full((R,), float("nan"), device=DEV)
    _lib.call("ia_scene_shadow", P, a_g, R, maps, proj, case["K"], case["S"], case["radius"], float(case["strength"]), float(case["near"]), shade)
    torch.cuda.synchronize()
    return _np(shade)


@pytest.mark.parametrize("name", sorted(sc.SHADOW))
def test_shadow_against_the_reference(name):
    case = sc.SHADOW[name]()
    ref = sr.shadow(case["P"], case["a_g"], case["maps"], case["proj"], case["radius"], case["strength"], case["near"])
    assert ref["inside"].any() and (~ref["inside"]).any() and ref["report"]["border_margin"] < 1.0
    shade = run_shadow(case)
    _close_abs(shade, ref["shade"], "shade")
    assert (shade[case["a_g"] == 0] == 1).all() and (shade[::9][case["a_g"][::9] != 0] == 1).all()   # no ground; behind every light
    assert (shade < 1).any()
    assert run_shadow(case).tobytes() == shade.tobytes()


# ---- end to end on the synthetic model ------------------------------------------------------------------------------------------------
SIZE = 32


@functools.lru_cache(maxsize=None)
def _model(seed):
    from instantavatar_amd.pipeline import build_synthetic_model
    model, _, _ = build_synthetic_model(torch.device(DEV), seed=seed)
    model.eval()
    return model


@functools.lru_cache(maxsize=None)
def _jitter():
    from instantavatar_amd.drivers import animate
    return animate.fixed_jitter(1, DEV)


def _seq(offset=(0.0, 0.0, 0.0), frames=4):
    from instantavatar_amd import scene, synthetic
    from instantavatar_amd.drivers import animate
    poses, trans = synthetic.procedural_pose_track(64)
    seq = animate.AnimateSequence(poses[:frames], trans[:frames], np.zeros(10, np.float32), torch.device(DEV), size=SIZE)
    return scene.place(seq, offset)


def _single(model, seq, i):
    """render_image_fast of one avatar with a zero background colour: premultiplied rgb, alpha, depth sum"""
    batch = seq.batch(i)
    batch["bg_color"] = torch.zeros((1, SIZE * SIZE, 3), device=DEV)
    with torch.no_grad():
        rgb, depth, alpha, _ = model.render_image_fast(batch, (SIZE, SIZE), jitter=_jitter())
    return rgb[0].clone(), alpha[0].clone(), depth[0].clone()


def test_scene_of_one_avatar_returns_the_bytes_of_render_image_fast():
    from instantavatar_amd import scene
    model, seq = _model(42), _seq()
    rgb, alpha, depth = _single(model, seq, 1)
    out = scene.Scene([model], [seq], jitter=_jitter()).render(1)
    assert float(alpha.max()) > 0.9 and float(alpha.min()) == 0.0                      # the avatar is in the frame and does not fill it
    assert torch.equal(out["rgb"], rgb) and torch.equal(out["alpha"], alpha) and torch.equal(out["depth"], depth)
    assert out["shade"] is None and int(out["contested"]) == 0
    want = torch.empty((SIZE, SIZE, 4), dtype=torch.uint8, device=DEV)
    from instantavatar_amd import _lib
    _lib.call("ia_pack_rgba8", rgb.contiguous(), alpha.contiguous(), SIZE * SIZE, want)
    assert torch.equal(out["rgba8"], want)
    # without a `bg_color` the renderer composites onto white: the same frame over a white background, up to rounding
    with torch.no_grad():
        white = model.render_image_fast(seq.batch(1), (SIZE, SIZE), jitter=_jitter())[0][0]
    over = scene.Scene([model], [seq], jitter=_jitter(), background=(1.0, 1.0, 1.0)).render(1)
    assert float((over["rgb"] - white).abs().max()) <= 2e-7 and bool((over["alpha"] == 1).all())


def test_two_avatars_side_by_side():
    from instantavatar_amd import scene
    ma, mb = _model(42), _model(43)
    sa, sb = _seq((-0.75, 0.0, 0.0)), _seq((0.75, 0.0, 0.0))
    ra, rb = _single(ma, sa, 2), _single(mb, sb, 2)
    assert float(ra[1].max()) > 0.9 and float(rb[1].max()) > 0.9
    ab = scene.Scene([ma, mb], [sa, sb], jitter=_jitter()).render(2)
    ba = scene.Scene([mb, ma], [sb, sa], jitter=_jitter()).render(2)
    for key in ("rgb", "alpha", "depth", "rgba8"):
        assert torch.equal(ab[key], ba[key]), key                                      # the order of the list changes nothing
    only_a, only_b = rb[1] == 0, ra[1] == 0
    assert bool((only_a & (ra[1] > 0)).any()) and bool((only_b & (rb[1] > 0)).any())
    for (rgb, alpha, depth), where in ((ra, only_a), (rb, only_b)):
        assert torch.equal(ab["rgb"][where], rgb[where]) and torch.equal(ab["alpha"][where], alpha[where])
        assert torch.equal(ab["depth"][where], depth[where])


def test_an_avatar_behind_another_is_hidden():
    from instantavatar_amd import scene
    ma, mb = _model(42), _model(43)
    front, back = _seq(), _seq((0.0, 0.0, 2.0))
    rf = _single(ma, front, 0)
    out = scene.Scene([mb, ma], [back, front], jitter=_jitter()).render(0)
    solid = rf[1] >= 0.99
    assert int(solid.sum()) > 20
    # behind alpha >= 0.99 the transmittance is at most 0.01, and the hidden layer's colour at most 1
    assert float((out["rgb"][solid] - rf[0][solid]).abs().max()) <= 0.01
    rb = _single(mb, back, 0)
    assert bool((solid & (rb[1] > 0.5)).any())                                         # there is something to hide


def test_ground_shadows_fall_where_the_light_sees_the_avatar():
    from instantavatar_amd import scene
    ma, mb = _model(42), _model(43)
    sa, sb = _seq((-0.5, 0.0, 0.0)), _seq((0.5, 0.0, 0.0))
    ground = scene.ground_under([ma, mb], [sa, sb], color2=(0.4, 0.4, 0.4), cell=0.5)
    assert ground.normal == (0.0, -1.0, 0.0) and 0.5 < -ground.offset < 2.0             # the feet are about a metre below the root, +y down
    light = (-2.0, -4.0, 2.0)
    s = scene.Scene([ma, mb], [sa, sb], ground=ground, light=light, shadow_size=64, jitter=_jitter())
    out = s.render(1)
    plain = scene.Scene([ma, mb], [sa, sb], jitter=_jitter()).render(1)
    shade = out["shade"]
    assert bool((out["alpha"] >= plain["alpha"]).all()) and float(out["alpha"].max()) == 1.0
    # the ground pixels, their points and where those fall in avatar 0's light map
    first = s.seqs[0]
    R = SIZE * SIZE
    t_g, a_g, c_g, P = (torch.empty(n, device=DEV) for n in ((R,), (R,), (R, 3), (R, 3)))
    from instantavatar_amd import _lib
    _lib.call("ia_scene_ground", first.rays_o.reshape(-1, 3).contiguous(), first.rays_d.reshape(-1, 3).contiguous(), R, *ground.normal,
              ground.offset, *ground.color, *ground.color2, ground.cell, *ground.centre, ground.r0, ground.r1, t_g, a_g, c_g, P)
    on_ground = a_g > 0
    assert int(on_ground.sum()) > 50
    assert bool((shade.reshape(-1)[on_ground] < 1).any()) and bool((shade.reshape(-1)[~on_ground] == 1).all())
    lit, dark = [], []
    for k in range(2):
        idx = 1 % len(s.seqs[k])
        batch = s.seqs[k].batch(idx)
        batch["bg_color"] = s._zero_bg
        with torch.no_grad():
            s.models[k].render_image_fast(batch, (SIZE, SIZE), jitter=_jitter())
        m, cam = s.light_view(k, idx, batch)
        proj = torch.as_tensor(scene.light_rays_projection(cam), device=DEV).double()
        x = torch.cat([P.double(), torch.ones(R, 1, device=DEV, dtype=torch.float64)], 1) @ proj.T
        u, v = (x[:, 0] / x[:, 2]).round().long(), (x[:, 1] / x[:, 2]).round().long()
        inside = on_ground & (x[:, 2] > 0.05) & (u >= 0) & (u < 64) & (v >= 0) & (v < 64)
        a = m[v.clamp(0, 63), u.clamp(0, 63)]
        lit.append(inside & (a >= 0.5))
        dark.append(~inside | (a == 0))
    shadowed, free = lit[0] | lit[1], dark[0] & dark[1] & on_ground
    assert int(shadowed.sum()) > 5 and int(free.sum()) > 5
    flat = shade.reshape(-1)
    assert float(flat[shadowed].mean()) < float(flat[free].mean())
    assert float(flat[shadowed].mean()) < 0.9


def test_scene_driver_writes_reproducible_frames(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = []
    for name in ("one", "two"):
        out = str(tmp_path / name)
        cmd = [sys.executable, "-m", "instantavatar_amd.drivers.scene", "--synthetic", "--seeds", "42", "43", "--size", "32", "--max-frames", "2",
               "--ground", "--light", "-2", "-4", "2", "--jitter-seed", "1", "--out", out]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "frames/s" in r.stdout and "contested pixels:" in r.stdout
        assert sorted(os.listdir(out)) == ["0.png", "1.png", "scene.gif"]
        outs.append(out)
    for f in ("0.png", "1.png", "scene.gif"):
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f
    from PIL import Image
    im = np.asarray(Image.open(os.path.join(outs[0], "1.png")))
    assert im.shape == (32, 32, 4) and (im[..., 3] == 255).mean() > 0.1                 # the ground covers part of the frame
