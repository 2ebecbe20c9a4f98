"""tests/scene_receive_refs.py -- the yardstick of tests/test_gpu_scene_receive.py -- held to analytic facts, and the conditions the
inputs of tests/scene_receive_cases.py must meet for that comparison to mean something.  No GPU.

The analytic set-ups put the light at (0, 0, -1) looking along +z with an identity rotation, so that a point (x, y, z) projects to
u = f x / (z + 1) + (S - 1) / 2 and its distance from the light is sqrt(x^2 + y^2 + (z + 1)^2): both are recomputed here with
numpy, independently of the reference's loops."""
import numpy as np
import pytest

import scene_receive_cases as cases
import scene_receive_refs as srr

F32 = np.float32
STRENGTH = F32(0.6)
FULL = F32(1.0) - STRENGTH * F32(1.0)          # the shade of a pixel-layer under one fully occluding caster


def _axis_projection(S, f, K=1):
    P = np.array([[f, 0, (S - 1) / 2.0, (S - 1) / 2.0], [0, f, (S - 1) / 2.0, (S - 1) / 2.0], [0, 0, 1.0, 1.0]], np.float32)
    return np.stack([P] * K)


def _plane_scene(depth, S=16, f=24.0, n=12):
    """receiver: layer 0, the plane z = `depth` seen along an n x n fan of rays; caster: layer 1, invisible to the camera (a = 0),
    whose map holds an opaque square of texels 5 .. 10 at 2 m from the light; layer 0's own map is empty"""
    o, dr = cases.fan(n * n, spread=0.4)
    dr[0] = dr[1]                               # (ray 0 of a fan is the axis itself, which projects onto a texel boundary)
    z =(depth / dr[:, 2].astype(np.float64)).astype(np.float32)
    a = np.stack([np.ones(n * n, np.float32), np.zeros(n * n, np.float32)])
    c = np.stack([np.full((n * n, 3), 0.5, np.float32), np.zeros((n * n, 3), np.float32)])
    maps_a = np.zeros((2, S, S), np.float32)
    maps_a[1, 5:11, 5:11] = 1.0
    maps_d = maps_a * F32(2.0)
    args = dict(rays_o=o, rays_d=dr, c=c, a=a, d=a * z[None], nrm=None, maps_a=maps_a, maps_d=maps_d, proj=_axis_projection(S, f, 2),
                light=cases.AXIS_LIGHT, radius=0, strength=STRENGTH)
    X = dr.astype(np.float64) * z.astype(np.float64)[:, None]
    u, v = f * X[:, 0] / (X[:, 2] + 1.0) + (S - 1) / 2.0, f * X[:, 1] / (X[:, 2] + 1.0) + (S - 1) / 2.0
    return args, X, u, v


def test_an_opaque_square_darkens_exactly_the_receivers_under_it():
    args, X, u, v = _plane_scene(3.0)
    out = srr.receive(**args)
    ui, vi = np.floor(u + 0.5), np.floor(v + 0.5)
    under = (ui >= 5) & (ui <= 10) & (vi >= 5) & (vi <= 10)
    assert 10 < under.sum() < under.size - 10 and out["clear"].all()
    assert (np.abs(u + 0.5 - np.round(u + 0.5)) > 1e-6).all()                           # no receiver on a texel boundary
    assert np.array_equal(out["shade"][0] == FULL, under) and np.array_equal(out["shade"][0] == 1, ~under)
    assert np.array_equal(out["c_out"][0], args["c"][0] * out["shade"][0][:, None])
    assert (out["shade"][1] == 1).all() and not out["receives"][1].any()               # the invisible caster does not receive
    rho = np.sqrt(X[:, 0] ** 2 + X[:, 1] ** 2 + (X[:, 2] + 1.0) ** 2)
    assert np.allclose(out["rho"][0], rho, rtol=1e-12) and rho.min() > 2.5              # behind the occluder at 2 m
    # a PCF radius of 1 softens the edge: fractions of ninths, full only where all nine taps are under the square
    soft = srr.receive(**dict(args, radius=1))["shade"][0]
    inner = (ui >= 6) & (ui <= 9) & (vi >= 6) & (vi <= 9)
    assert (soft[inner] == FULL).all() and ((soft > FULL) & (soft < 1)).any()


def test_a_receiver_in_front_of_the_occluder_stays_lit():
    args, X, _, _ = _plane_scene(0.5)
    rho = np.sqrt(X[:, 0] ** 2 + X[:, 1] ** 2 + (X[:, 2] + 1.0) ** 2)
    assert rho.max() < 1.9                                                              # nearer to the light than the 2 m of the square
    out = srr.receive(**args)
    assert (out["shade"] == 1).all() and out["inside"][0, 1].any()                      # tapped, and not occluded


@pytest.mark.parametrize("gap, bias_self, dark", [(0.03, 0.05, False), (0.07, 0.05, True), (0.03, 0.02, True), (0.03, 0.03, False)])
def test_bias_self_decides_a_self_tap_by_the_stated_inequality(gap, bias_self, dark):
    """one ray along +z, one layer at z = 3 (rho = 4 exactly) whose own map is opaque at 4 - gap metres: s < (rho - bias_self) m"""
    o, dr = cases.fan(1)
    S = 4
    maps_a = np.ones((1, S, S), np.float32)
    maps_d = np.full((1, S, S), 4.0 - gap, np.float32)
    out = srr.receive(rays_o=o, rays_d=dr, c=np.full((1, 1, 3), 0.5, np.float32), a=np.ones((1, 1), np.float32), d=np.full((1, 1), 3.0, np.float32),
                      nrm=None, maps_a=maps_a, maps_d=maps_d, proj=_axis_projection(S, 2.0), light=cases.AXIS_LIGHT, radius=0,
                      strength=STRENGTH, bias_other=0.0, bias_self=bias_self)
    assert out["rho"][0, 0] == 4.0 and out["inside"][0, 0, 0]
    assert (float(F32(4.0 - gap)) < (4.0 - float(F32(bias_self))) * 1.0) == dark        # the inequality, on the fp32 values
    assert out["shade"][0, 0] == (FULL if dark else 1)


def test_the_one_ray_case_shadows_itself_only_when_its_own_map_is_held_to_bias_other():
    case = cases.make_one_ray()
    out = srr.receive(**cases.arguments(case))
    assert out["shade"][0, 0] == FULL and out["shade"][1, 0] == 1 and out["shade"][2, 0] == 1
    assert out["abar"][0, 1, 0] == 1 and out["abar"][0, 0, 0] == 0 and out["abar"][1, 1, 0] == 0 and out["inside"][1, 1, 0]
    same = srr.receive(**dict(cases.arguments(case), bias_self=case["bias_other"]))
    assert same["abar"][1, 1, 0] == 1 and same["shade"][1, 0] == FULL                   # only bias_self suppressed it


@pytest.mark.parametrize("n, g", [((1.0, 0.0, 0.0), 1.0), ((0.9, 0.0, -0.25), 0.5), ((0.8, 0.0, -0.5), 0.0), ((0.0, 0.0, -1.0), 0.0),
                                   ((0.0, 0.0, 1.0), 1.0), ((0.0, 0.0, 0.0), 0.0), ((np.nan, 0.0, -1.0), 0.0)])
def test_the_facing_ramp(n, g):
    """receiver (0, 0, 3), light (0, 0, -1): l = (0, 0, -4), so cosv = -n_z exactly; cos0 = 0, cos1 = 0.5: g = 1, 1/2, 0 at cos0,
    halfway and cos1, clamped beyond; no term for a zero or a non-finite normal"""
    o, dr = cases.fan(1)
    S = 4
    out = srr.receive(rays_o=o, rays_d=dr, c=np.full((1, 1, 3), 0.5, np.float32), a=np.ones((1, 1), np.float32), d=np.full((1, 1), 3.0, np.float32),
                      nrm=np.asarray(n, np.float32).reshape(1, 1, 3), maps_a=np.zeros((1, S, S), np.float32), maps_d=np.zeros((1, S, S), np.float32),
                      proj=_axis_projection(S, 2.0), light=cases.AXIS_LIGHT, radius=1, strength=STRENGTH, cos0=0.0, cos1=0.5)
    assert out["g"][0, 0] == F32(g)
    assert out["shade"][0, 0] == F32(1.0) - STRENGTH * F32(g)
    if np.isfinite(n).all() and any(n):
        assert out["cosv"][0, 0] == -n[2]


def test_strength_zero_leaves_every_layer_as_it_is():
    case = cases.CASES["R65_K3_S16_r3_zero_rows"]()
    out = srr.receive(**dict(cases.arguments(case), strength=0.0))
    assert (out["shade"] == 1).all()
    rec = out["receives"]
    assert np.array_equal(out["c_out"][rec], case["c"][rec])
    assert out["c_out"].tobytes() == case["c"].tobytes()                                # and the others bit for bit, NaNs included


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_every_case_holds_what_the_gpu_test_needs(name):
    case, ref = cases.case_and_reference(name)
    K, R = case["K"], case["R"]
    rec, shade = ref["receives"], ref["shade"]
    unclear = int((~ref["clear"]).sum())
    print("%s: %d of %d pixel-layers unclear, %d receive, %d shaded below 1" % (name, unclear, K * R, rec.sum(), (shade[rec] < 1).sum()))
    assert unclear <= 0.01 * K * R
    assert not rec.all()                                                                # a pixel-layer that does not receive
    assert (shade[~rec] == 1).all() and ref["c_out"][~rec].tobytes() == case["c"][~rec].tobytes()
    assert (shade[rec] == 1).any()                                                      # one that receives and stays lit
    if float(case["strength"]) > 0:
        assert (shade[rec] < 1).any()
    else:
        # strength 0 shades nothing by definition: what the case must hold is something that WOULD be shaded
        assert (shade == 1).all() and ((ref["abar"] > 0).any(1)[rec].any() or (ref["g"][rec] > 0).any())


def test_the_cases_cover_the_listed_edge_inputs():
    seen = set()
    for name in sorted(cases.CASES):
        case, ref = cases.case_and_reference(name)
        a, c, d, rec = case["a"], case["c"], case["d"], ref["receives"]
        K = case["K"]
        with np.errstate(all="ignore"):
            seen |= {"a0"} if (a == 0).any() else set()
            seen |= {"a_neg"} if (a < 0).any() else set()
            seen |= {"bad_c"} if (~np.isfinite(c)).any() else set()
            seen |= {"bad_a"} if (~np.isfinite(a)).any() else set()
            seen |= {"bad_d"} if (~np.isfinite(d)).any() else set()
        proj = case["proj"].astype(np.float64)
        X = ref["X"]
        zl = np.einsum("kc,jrc->jkr", proj[:, 2, :3], np.nan_to_num(X)) + proj[:, 2, 3][None, :, None]
        behind = rec[:, None, :] & (zl <= float(case["near"]))
        seen |= {"behind_near"} if behind.any() else set()
        seen |= {"outside_every_map"} if (rec & ~ref["inside"].any(1) & ~behind.any(1)).any() else set()
        seen |= {"m0"} if (case["maps_a"] == 0).any() and ref["inside"].any() else set()
        seen |= {"s_nan"} if (np.isnan(case["maps_d"]) & (case["maps_a"] > 0)).any() else set()
        seen |= {"strength%g" % float(case["strength"])}
        seen |= {"normals_" + ("null" if case["nrm"] is None else "zero_rows" if (case["nrm"] == 0).all(-1).any() else "given")}
        seen |= {"R%d" % case["R"], "K%d" % K, "S%d" % case["S"], "r%d" % case["radius"]}
    want = {"a0", "a_neg", "bad_c", "bad_a", "bad_d", "behind_near", "outside_every_map", "m0", "s_nan", "strength0", "strength1",
            "normals_null", "normals_zero_rows", "normals_given", "R1", "R65", "R200", "K1", "K2", "K3", "K8", "S1", "S8", "S16",
            "r0", "r1", "r2", "r3"}
    assert want <= seen, sorted(want - seen)
