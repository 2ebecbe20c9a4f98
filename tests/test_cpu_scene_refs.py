"""tests/scene_refs.py, the float64 reference of the scene composition ("scene composition"), is itself checked
here by properties that can be verified by hand; then the binding table of include/instantavatar_hip_scene.h, what the entry points
refuse before anything is launched, the host-side pieces of `instantavatar_amd.scene` (the ground's axes, the light camera), and
that the inputs of the GPU test (`scene_cases`) meet the preconditions its bounds rest on.  No GPU."""
import os

import numpy as np
import pytest

import scene_refs as sr

NAMES = ["ia_scene_composite", "ia_scene_ground", "ia_scene_shadow", "ia_scene_zero"]


def _layer(R, rgb, a, z):
    """a layer of constant UNpremultiplied colour, opacity a and depth z over R pixels -> (c, a, d) as the renderer gives them"""
    a = np.full(R, a, np.float64)
    return np.asarray(rgb, np.float64)[None] * a[:, None], a, a * z


def _stack(layers):
    return np.stack([l[0] for l in layers]), np.stack([l[1] for l in layers]), np.stack([l[2] for l in layers])


# ---- composite ------------------------------------------------------------------------------------------------------------------------
def test_one_layer_gives_the_inputs_back():
    rng = np.random.default_rng(0)
    a = rng.uniform(0.0, 1.0, 12).astype(np.float32)
    a[3] = 0.0
    c = (rng.uniform(0, 1, (12, 3)) * a[:, None]).astype(np.float32)
    d = (a * rng.uniform(3, 6, 12)).astype(np.float32)
    out = sr.composite(c[None], a[None], d[None])
    keep = a > 0
    np.testing.assert_allclose(out["rgb"][keep], c[keep], rtol=0, atol=1e-15)
    np.testing.assert_allclose(out["alpha"][keep], a[keep], rtol=0, atol=1e-15)
    np.testing.assert_allclose(out["depth"][keep], d[keep], rtol=0, atol=1e-15)
    assert (out["rgb"][~keep] == 0).all() and out["alpha"][3] == 0 and out["depth"][3] == 0      # a = 0 does not take part
    assert out["contested"] == 0 and out["report"]["key_gap"] == np.inf


def test_the_nearer_of_two_opaque_layers_wins_whichever_is_listed_first():
    near, far = _layer(4, (1, 0, 0), 1.0, 3.0), _layer(4, (0, 1, 0), 1.0, 5.0)
    for pair in ([near, far], [far, near]):
        out = sr.composite(*_stack(pair))
        assert np.array_equal(out["rgb"], np.tile([1.0, 0, 0], (4, 1))) and (out["alpha"] == 1).all() and (out["depth"] == 3).all()


def test_half_transparent_front_layer_closed_form():
    front, back = _layer(3, (1.0, 0.5, 0.0), 0.5, 2.0), _layer(3, (0.0, 0.25, 1.0), 1.0, 4.0)
    out = sr.composite(*_stack([back, front]))
    np.testing.assert_allclose(out["rgb"], np.tile([0.5 * 1.0, 0.5 * 0.5 + 0.5 * 0.25, 0.5 * 1.0], (3, 1)), rtol=0, atol=1e-15)
    np.testing.assert_allclose(out["alpha"], 1.0)
    np.testing.assert_allclose(out["depth"], 0.5 * 2.0 + 0.5 * 4.0)
    assert out["order"][0] == [1, 0]


def test_invariant_under_permuting_layers_with_different_keys():
    rng = np.random.default_rng(1)
    R, K = 9, 4
    layers = [_layer(R, rng.uniform(0, 1, 3), a, z) for a, z in zip((0.3, 0.8, 0.6, 1.0), (2.0, 3.0, 4.5, 6.0))]
    ref = sr.composite(*_stack(layers))
    assert ref["report"]["key_gap"] > 0.1
    for perm in ([3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 3, 1]):
        out = sr.composite(*_stack([layers[p] for p in perm]))
        for key in ("rgb", "alpha", "depth"):
            assert np.array_equal(out[key], ref[key]), (perm, key)


def test_an_exact_tie_resolves_by_index():
    a, b = _layer(2, (1, 0, 0), 0.5, 3.0), _layer(2, (0, 0, 1), 0.5, 3.0)
    ab, ba = sr.composite(*_stack([a, b])), sr.composite(*_stack([b, a]))
    assert ab["order"][0] == [0, 1] and ba["order"][0] == [0, 1]
    assert np.allclose(ab["rgb"][0], [0.5, 0, 0.25]) and np.allclose(ba["rgb"][0], [0.25, 0, 0.5])
    # the ground has index K: a tie with a layer goes to the avatar
    g = (np.full(2, 3.0), np.ones(2), np.tile([0.0, 1.0, 0.0], (2, 1)), np.ones(2))
    out = sr.composite(*_stack([a]), ground=g)
    assert out["order"][0] == [0, 1] and np.allclose(out["rgb"][0], [0.5, 0.5, 0.0])
    assert out["report"]["key_gap"] == np.inf                                        # equal keys are not a gap


def test_layers_that_do_not_take_part():
    good = _layer(5, (0.2, 0.4, 0.6), 0.7, 3.0)
    for field, value in ((0, np.nan), (0, np.inf), (1, np.nan), (1, np.inf), (2, np.nan), (2, -np.inf), (1, 0.0), (1, -0.5)):
        bad = [x.copy() for x in _layer(5, (1, 1, 1), 1.0, 1.0)]
        if field == 0:
            bad[0][:, 1] = value
        else:
            bad[field][:] = value
        out = sr.composite(*_stack([bad, good]))
        ref = sr.composite(*_stack([good]))
        for key in ("rgb", "alpha", "depth"):
            assert np.array_equal(out[key], ref[key]), (field, value, key)


def test_the_background_fills_exactly_the_transmittance():
    layers = [_layer(6, (1, 0, 0), 0.25, 2.0), _layer(6, (0, 1, 0), 0.5, 3.0)]
    plain = sr.composite(*_stack(layers))
    T = 0.75 * 0.5
    np.testing.assert_allclose(plain["transmittance"], T)
    np.testing.assert_allclose(plain["alpha"], 1 - T)
    bg = np.random.default_rng(2).uniform(0, 1, (6, 3))
    out = sr.composite(*_stack(layers), background=bg)
    np.testing.assert_allclose(out["rgb"] - plain["rgb"], T * bg.astype(np.float32).astype(np.float64), rtol=0, atol=1e-15)
    assert (out["alpha"] == 1).all() and np.array_equal(out["depth"], plain["depth"])
    const = sr.composite(*_stack(layers), background=(0.5, 0.25, 1.0))
    np.testing.assert_allclose(const["rgb"] - plain["rgb"], np.tile([T * 0.5, T * 0.25, T], (6, 1)), rtol=0, atol=1e-15)


def test_contested_counts_a_close_pair_and_not_a_distant_one():
    R = 7
    a = _layer(R, (1, 0, 0), 0.9, 5.0)
    close, distant, faint = _layer(R, (0, 1, 0), 0.8, 5.2), _layer(R, (0, 1, 0), 0.8, 5.4), _layer(R, (0, 1, 0), 0.4, 5.1)
    assert sr.composite(*_stack([a, close]), contact=0.3)["contested"] == R
    assert sr.composite(*_stack([a, distant]), contact=0.3)["contested"] == 0
    assert sr.composite(*_stack([a, faint]), contact=0.3)["contested"] == 0          # below a = 0.5
    # one pixel counts once, however many pairs it has, and the ground is no avatar
    g = (np.full(R, 5.05), np.ones(R), np.ones((R, 3)), np.ones(R))
    out = sr.composite(*_stack([a, close, _layer(R, (0, 0, 1), 1.0, 5.1)]), ground=g, contact=0.3)
    assert out["contested"] == R and out["contested_mask"].all()
    assert sr.composite(*_stack([a]), ground=g, contact=0.3)["contested"] == 0
    with pytest.raises(ValueError):
        sr.composite(np.zeros((9, 2, 3)), np.zeros((9, 2)), np.zeros((9, 2)))


# ---- ground -----------------------------------------------------------------------------------------------------------------------------
FLOOR = dict(normal=(0.0, -1.0, 0.0), h=-1.0, g0=(0.8, 0.7, 0.6), g1=(0.1, 0.2, 0.3))          # the plane y = 1, +y down


def _pinhole(H, W, f, eye=(0.0, 0.0, 0.0)):
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(i - (W - 1) / 2) / f, (j - (H - 1) / 2) / f, np.ones_like(i, float)], -1).reshape(-1, 3)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(np.asarray(eye, np.float32), (H * W, 1)), d.astype(np.float32)


def test_ground_closed_form_under_an_analytic_camera():
    o, d = _pinhole(9, 7, 8.0)
    out = sr.ground(o, d, cell=0.0, centre=(0, 1, 4), r0=100.0, r1=200.0, **FLOOR)
    dd = d.astype(np.float64)
    down = dd[:, 1] > 0
    assert np.array_equal(out["hit"], down) and down.any() and (~down).any()
    np.testing.assert_allclose(out["t_g"][down], 1.0 / dd[down, 1], rtol=1e-14)       # y = 1 from the origin: t = 1 / d_y
    np.testing.assert_allclose(out["P"][down], dd[down] / dd[down, 1:2], rtol=1e-14)
    assert (out["a_g"][down] == 1).all() and np.array_equal(out["c_g"][down], np.tile(np.float32(FLOOR["g0"]).astype(float), (down.sum(), 1)))
    for key in ("t_g", "a_g", "c_g", "P"):
        assert (out[key][~down] == 0).all()


def test_ground_rejected_rays():
    o = np.zeros((4, 3), np.float32)
    d = np.array([[0, 0, 1], [0, -1, 0], [0, 1, 0], [0, 1, 0]], np.float32)       # parallel, away from the plane, towards it, towards it
    o[3] = (0, 2, 0)                                                               # a camera below the floor
    out = sr.ground(o, d, cell=0.0, centre=(0, 1, 0), r0=1.0, r1=2.0, **FLOOR)
    assert out["hit"].tolist() == [False, False, True, False]
    # a hit behind the origin: the camera above the plane looking up has t < 0 and is rejected by n . d < 0 as well as by t > 0
    assert out["t_g"].tolist() == [0, 0, 1, 0]
    # t beyond fp32: no hit
    far = sr.ground(np.zeros((1, 3), np.float32), np.array([[1, 1e-45, 0]], np.float32), cell=0.0, centre=(0, 1, 0), r0=1.0, r1=2.0, **FLOOR)
    assert not far["hit"][0]


def test_disc_opacity_at_r0_midpoint_and_r1():
    # straight down from above the points at distance r0, (r0 + r1) / 2, r1 and beyond, exactly representable
    xs = np.array([0.0, 2.0, 3.0, 4.0, 5.0], np.float32)
    o = np.stack([xs, np.zeros(5, np.float32), np.zeros(5, np.float32)], 1)
    d = np.tile(np.float32([0, 1, 0]), (5, 1))
    out = sr.ground(o, d, cell=0.0, centre=(0, 1, 0), r0=2.0, r1=4.0, **FLOOR)
    assert out["hit"].all() and out["a_g"].tolist() == [1.0, 1.0, 0.5, 0.0, 0.0]
    assert (out["t_g"] == 1).all()                                                   # outside the disc the hit is still reported
    same = sr.ground(o, d, cell=0.0, centre=(0, 1, 0), r0=3.0, r1=3.0, **FLOOR)      # r0 == r1: a hard edge
    assert same["a_g"].tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]


def test_checker_axes_and_parity():
    e1, e2 = sr.plane_axes(FLOOR["normal"])
    assert e1.tolist() == [1.0, 0.0, 0.0] and e2.tolist() == [0.0, 0.0, 1.0]          # least aligned axis of (0, -1, 0): x (lowest index)
    for n in ((0.6, 0.0, 0.8), (0.48, -0.6, 0.64), (-1.0, 0.0, 0.0)):
        n = np.float32(n).astype(np.float64)
        a, b = sr.plane_axes(n)
        assert abs(a @ n) < 1e-7 and abs(b @ n) < 1e-7 and abs(a @ b) < 1e-7 and abs(a @ a - 1) < 1e-12 and abs(b @ b - 1) < 1e-6
    xs, zs = np.meshgrid(np.arange(-2, 3) * 0.5 + 0.25, np.arange(-2, 3) * 0.5 + 0.25)
    o = np.stack([xs.ravel(), np.zeros(25), zs.ravel()], 1).astype(np.float32)
    d = np.tile(np.float32([0, 1, 0]), (25, 1))
    out = sr.ground(o, d, cell=0.5, centre=(0, 1, 0), r0=10.0, r1=20.0, **FLOOR)
    odd = ((np.floor(xs.ravel() / 0.5) + np.floor(zs.ravel() / 0.5)).astype(int) & 1) == 1
    assert odd.any() and (~odd).any()
    assert np.array_equal(out["c_g"], np.where(odd[:, None], np.float32(FLOOR["g1"]).astype(float), np.float32(FLOOR["g0"]).astype(float)))
    assert out["report"]["cell_margin"] == pytest.approx(0.5)
    assert sr.ground(o, d, cell=0.0, centre=(0, 1, 0), r0=10.0, r1=20.0, **FLOOR)["report"]["cell_margin"] == np.inf


# ---- shadow -----------------------------------------------------------------------------------------------------------------------------
def _top_light(S, f=4.0, height=3.0):
    """a light `height` above the floor y = 1 at (0, 1 - height, 0) looking straight down: camera x = world x, camera y = world z"""
    w2c = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, -(1 - height)]], np.float64)
    K = np.array([[f, 0, (S - 1) / 2], [0, f, (S - 1) / 2], [0, 0, 1]], np.float64)
    return (K @ w2c).astype(np.float32)


def test_shadow_of_a_constant_map_and_outside_the_map():
    S = 9
    proj = _top_light(S)[None]
    P = np.array([[0, 1, 0], [0.5, 1, -0.5], [2.9, 1, 0], [3.1, 1, 0], [0, 4.5, 0], [0, 1, 0]], np.float32)   # u = 4 + 4 x / 3
    a_g = np.array([1, 1, 0.5, 1, 1, 0], np.float32)
    for r in (0, 1, 3):
        out = sr.shadow(P, a_g, np.full((1, S, S), 0.75, np.float32), proj, r, 0.5, 0.05)
        assert out["inside"][0].tolist() == [True, True, True, False, True, False]
        np.testing.assert_allclose(out["shade"], [1 - 0.5 * 0.75] * 3 + [1.0] + [1 - 0.5 * 0.75] + [1.0], rtol=0, atol=1e-15)
    # behind the light (z <= near) contributes nothing
    up = sr.shadow(np.array([[0, -3, 0]], np.float32), np.ones(1, np.float32), np.ones((1, S, S), np.float32), proj, 1, 1.0, 0.05)
    assert up["shade"][0] == 1 and not up["inside"][0, 0]


def test_shadow_bilinear_pcf_and_the_product_over_layers():
    S = 5
    m = np.zeros((2, S, S), np.float32)
    m[0, :, 3:] = 1.0                              # a step in u between pixels 2 and 3
    m[1] = 0.5
    proj = np.stack([_top_light(S, f=3.0), _top_light(S, f=3.0)])          # u = 2 + x
    P = np.array([[0.25, 1, 0], [0.5, 1, 0.0], [-1.0, 1, 0]], np.float32)  # u = 2.25, 2.5, 1
    r0 = sr.shadow(P, np.ones(3, np.float32), m[:1], proj[:1], 0, 1.0, 0.05)
    np.testing.assert_allclose(r0["abar"][0], [0.25, 0.5, 0.0], atol=1e-15)
    r1 = sr.shadow(P[2:], np.ones(1, np.float32), m[:1], proj[:1], 1, 1.0, 0.05)     # taps at u = 0, 1, 2: all 0
    assert r1["abar"][0, 0] == 0
    r1 = sr.shadow(P[1:2], np.ones(1, np.float32), m[:1], proj[:1], 1, 1.0, 0.05)    # taps at u = 1.5, 2.5, 3.5: 0, 0.5, 1
    np.testing.assert_allclose(r1["abar"][0, 0], 0.5, atol=1e-15)
    both = sr.shadow(P, np.ones(3, np.float32), m, proj, 0, 0.8, 0.05)
    np.testing.assert_allclose(both["shade"], (1 - np.float64(np.float32(0.8)) * np.array([0.25, 0.5, 0.0])) * (1 - np.float64(np.float32(0.8)) * 0.5), atol=1e-15)
    # a tap beyond the border clamps to the edge: at u = 4 (the last pixel) with r = 1 the taps are 3, 4, 4
    edge = sr.shadow(np.array([[2.0, 1, 0]], np.float32), np.ones(1, np.float32), m[:1], proj[:1], 1, 1.0, 0.05)
    assert edge["abar"][0, 0] == 1.0 and edge["report"]["border_margin"] == 0.0


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_scene_header_is_bound():
    """(that its names are disjoint from every other header's: tests/test_cpu_abi_headers.py)"""
    from instantavatar_amd import _lib, build
    d = _lib.declarations("scene")
    assert sorted(d) == NAMES
    assert len(_lib.declarations()) == 89
    for name in NAMES:
        assert d[name].stream, name                                       # every entry point launches and takes a stream
        assert hasattr(_lib.lib(), name) and name in _lib._bound, name
    assert "ia_scene.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ia_scene.hip"))
    assert os.path.normpath(_lib.header_path("scene")) in [os.path.normpath(h) for h in build.SHARED_HEADERS]
    assert "ia_scene.hip" in build.source_manifest() and "ia_scene.hip" in build.library_manifest()
    with pytest.raises(_lib.IAError, match=r"instantavatar_hip_scene\.h"):
        _lib.call("ia_scene_nothing")
    with open(_lib.header_path("scene")) as f:
        assert "#define IA_SCENE_MAX_LAYERS %d" % sr.MAX_LAYERS in f.read()


def test_host_side_argument_errors():
    """what the entry points decide before any launch"""
    from instantavatar_amd import _lib
    P = 4096                                                  # (a non-null address that is never read: every call below is refused)

    def comp(K=2, R=4, ground=(None,) * 4, contact=0.3, c=P, out=P):
        return _lib.call("ia_scene_composite", c, P, P, K, R, *ground, None, 0, contact, out, P, P, P, None)
    for K in (0, 9, -1):
        with pytest.raises(_lib.IAError, match="K = %d outside" % K):
            comp(K=K)
    with pytest.raises(_lib.IAError, match="R = -1"):
        comp(R=-1)
    with pytest.raises(_lib.IAError, match="contact"):
        comp(contact=-0.1)
    with pytest.raises(_lib.IAError, match="or none of them"):
        comp(ground=(P, P, None, P))
    with pytest.raises(_lib.IAError, match="null pointer"):
        comp(c=None)
    assert comp(R=0, c=None, out=None) == 0                    # nothing to do: nothing is read

    def gnd(n=(0.0, -1.0, 0.0), cell=0.5, r=(1.0, 2.0), R=4, o=P):
        return _lib.call("ia_scene_ground", o, P, R, *n, 0.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, cell, 0.0, 0.0, 0.0, *r, P, P, P, P, None)
    with pytest.raises(_lib.IAError, match="unit length"):
        gnd(n=(0.0, -2.0, 0.0))
    with pytest.raises(_lib.IAError, match="unit length"):
        gnd(n=(float("nan"), 0.0, 0.0))
    with pytest.raises(_lib.IAError, match="cell"):
        gnd(cell=-1.0)
    with pytest.raises(_lib.IAError, match="radii"):
        gnd(r=(2.0, 1.0))
    with pytest.raises(_lib.IAError, match="null pointer"):
        gnd(o=None)

    def shd(K=1, S=8, radius=1, strength=0.5, near=0.05, R=4, maps=P):
        return _lib.call("ia_scene_shadow", P, P, R, maps, P, K, S, radius, strength, near, P, None)
    for K in (0, 9):
        with pytest.raises(_lib.IAError, match="K = %d outside" % K):
            shd(K=K)
    with pytest.raises(_lib.IAError, match="S = 0"):
        shd(S=0)
    for r in (-1, 4):
        with pytest.raises(_lib.IAError, match="PCF radius %d" % r):
            shd(radius=r)
    for s in (-0.1, 1.5, float("nan")):
        with pytest.raises(_lib.IAError, match="strength"):
            shd(strength=s)
    with pytest.raises(_lib.IAError, match="near"):
        shd(near=0.0)
    with pytest.raises(_lib.IAError, match="null pointer"):
        shd(maps=None)
    with pytest.raises(_lib.IAError, match="n = -1"):
        _lib.call("ia_scene_zero", P, -1, None)


# ---- the host side of instantavatar_amd.scene ------------------------------------------------------------------------------------------
def test_light_camera_looks_at_its_target_and_fills_the_map():
    from instantavatar_amd import scene
    light, target = np.array([-2.0, -4.0, 2.0]), np.array([0.3, 0.15, 5.0])
    cam = scene.light_camera(light, target, extent=2.4, size=64, device="cpu")
    w2c = cam.w2c_host
    R = w2c[:3, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-14)
    assert np.linalg.det(R) == pytest.approx(1.0)
    dist = np.linalg.norm(target - light)
    np.testing.assert_allclose(w2c[:3, :3] @ target + w2c[:3, 3], [0, 0, dist], atol=1e-12)          # the target is on the axis
    np.testing.assert_allclose(w2c[:3, :3] @ light + w2c[:3, 3], 0, atol=1e-12)
    assert R[1] @ np.array([0.0, 1.0, 0.0]) > 0                                                       # world down is down in the map
    o, d, proj = scene.light_rays(cam)
    assert o.shape == d.shape == (64 * 64, 3) and proj.shape == (3, 4) and proj.dtype == np.float32
    np.testing.assert_allclose(o, np.tile(light, (64 * 64, 1)), atol=1e-5)
    # `extent` metres across the target's plane span the map: a point extent / 2 to the side of the target lands size / 2 pixels from the centre
    side = target + 1.2 * R[0]
    x = proj.astype(np.float64) @ np.append(side, 1.0)
    assert x[0] / x[2] == pytest.approx(31.5 + 32.0, abs=1e-4) and x[1] / x[2] == pytest.approx(31.5, abs=1e-4)
    # a ray through a pixel projects back onto that pixel: the rays and the projection are one camera
    k = 17 * 64 + 40
    x = proj.astype(np.float64) @ np.append(o[k] + 3.0 * d[k], 1.0)
    assert x[0] / x[2] == pytest.approx(40.0, abs=1e-3) and x[1] / x[2] == pytest.approx(17.0, abs=1e-3)
    # a light straight above: the up rule switches to world +z
    top = scene.light_camera([0.0, -5.0, 5.0], [0.0, 0.0, 5.0], size=16, device="cpu")
    assert np.isfinite(top.w2c_host).all() and np.allclose(top.w2c_host[2, :3], [0, 1, 0])


def test_ground_object():
    from instantavatar_amd import _lib, scene
    g = scene.Ground(normal=(0, -2, 0), offset=-1.0, color=(0.1, 0.2, 0.3))
    assert g.normal == (0.0, -1.0, 0.0) and g.centre == (0.0, 1.0, 0.0) and g.cell == 0.0 and g.color2 == g.color
    g = scene.Ground(offset=-1.0, color2=(0, 0, 0), cell=0.5, centre=(1, 1, 4), r0=1, r1=2)
    assert g.cell == 0.5 and g.centre == (1.0, 1.0, 4.0)
    with pytest.raises(_lib.IAError, match="radii"):
        scene.Ground(r0=3, r1=2)


# ---- the GPU test's inputs meet its preconditions --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(__import__("scene_cases").COMPOSITE))
def test_composite_cases_have_no_close_keys(name):
    import scene_cases as sc
    case = sc.COMPOSITE[name]()
    out = sr.composite(case["c"], case["a"], case["d"], ground=case["ground"], background=case["background"], contact=case["contact"])
    assert out["report"]["key_gap"] > 1e-3, out["report"]
    # no pair of opaque layers sits near the `contact` threshold either: |z_i - z_j| stays 1e-3 away from it (relative to contact)
    assert sc.contact_margin(case) > 1e-3
    if case.get("expect_contested") is not None:
        assert out["contested"] == case["expect_contested"]
    if case.get("expect_ties"):
        assert any(len(o) > 1 for o in out["order"])


@pytest.mark.parametrize("name", sorted(__import__("scene_cases").GROUND))
def test_ground_cases_stay_off_the_cell_borders(name):
    import scene_cases as sc
    case = sc.GROUND[name]()
    out = sr.ground(case["rays_o"], case["rays_d"], **case["plane"])
    assert out["report"]["cell_margin"] > 1e-4, out["report"]
    assert out["hit"].any() and not out["hit"][:4].any()           # the four rays that must be rejected are


@pytest.mark.parametrize("name", sorted(__import__("scene_cases").SHADOW))
def test_shadow_cases_cover_what_they_are_meant_to(name):
    import scene_cases as sc
    case = sc.SHADOW[name]()
    out = sr.shadow(case["P"], case["a_g"], case["maps"], case["proj"], case["radius"], case["strength"], case["near"])
    assert out["inside"].any() and (~out["inside"]).any()
    assert (out["shade"] < 1).any()
    assert out["report"]["border_margin"] < 1.0                     # some centre tap is within a pixel of the border: the clamp is exercised
