"""`ia_scene_deep_composite` (csrc/ia_scene_deep.hip, include/instantavatar_hip_scene_deep.h) against tests/scene_deep_refs.py on the
inputs of tests/scene_deep_cases.py (both held to their own conditions in tests/test_cpu_scene_deep_refs.py), then the recorder
`dense_routes.render_test_deep` and `scene.Scene(exact=True)` end to end on the synthetic model at 32 x 32 with one fixed occupancy
jitter, and the driver.

Bounds: the reference's own propagated error bound per output (`deep_compare`, one RATIO line per case), on the pixels where no
threshold decision lies within its error; the count of interleaved pixels is exact.  Against the renderer's fused route the gate is
`world.rays_within`'s default (1e-3 on all but max(2, 1e-4 n) rays), the one the closure route is held to."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_deep_cases as cases
import scene_deep_refs as sdr
from world import rays_within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def run_deep(case, fill=float("nan")):
    from instantavatar_amd import _lib
    K, S, n = case["z"].shape
    g = (None,) * 4 if case["ground"] is None else tuple(_dev(x) for x in case["ground"])
    bg = _dev(case["bg"])
    rgb, alpha, depth = (torch.full(s, fill, device=DEV) for s in ((n, 3), (n,), (n,)))
    count = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    _lib.call("ia_scene_zero", count, 1)
    _lib.call("ia_scene_deep_composite", _dev(case["z"]), _dev(case["delta"]), _dev(case["sigma"]), _dev(case["rgb"]), K, S, n,
              _dev(case["factor"]), *g, bg, int(bg is not None and bg.numel() == 3), float(case["thresh"]), rgb, alpha, depth, count)
    return dict(rgb=_np(rgb), alpha=_np(alpha), depth=_np(depth), interleaved=int(count))


def _same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("rgb", "alpha", "depth")) and a["interleaved"] == b["interleaved"]


# ---- the kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.NAMES)
def test_kernel_against_the_reference(name):
    case, ref = cases.case_and_ref(name)
    got = run_deep(case)
    assert np.isfinite(got["rgb"]).all() and np.isfinite(got["alpha"]).all() and np.isfinite(got["depth"]).all()
    sdr.deep_compare(got, ref, name)
    if not ref["undecidable"].any():
        assert got["interleaved"] == ref["interleaved"]
    assert _same_bytes(run_deep(case, fill=0.0), got)                                    # a second call gives the same bytes


@pytest.mark.parametrize("name", ["k1_n1_s1", "k1_n70_s37"])
def test_one_list_gives_the_bytes_of_ia_composite_test(name):
    from instantavatar_amd import _lib
    case, _ = cases.case_and_ref(name)
    got = run_deep(case)
    _, S, n = case["z"].shape
    rows = lambda a: _dev(np.moveaxis(a[0], 0, 1))                                      # [S,n,..] -> the dense [n,S,..] blocks
    color, depth, trans = torch.zeros((n, 3), device=DEV), torch.zeros(n, device=DEV), torch.ones(n, device=DEV)
    _lib.call("ia_composite_test", rows(case["rgb"]), rows(case["sigma"]), rows(case["delta"]), rows(case["z"]),
              torch.arange(n, device=DEV), n, S, color, depth, trans, float(case["thresh"]))
    assert got["rgb"].tobytes() == _np(color).tobytes() and got["depth"].tobytes() == _np(depth).tobytes()
    assert got["alpha"].tobytes() == _np(1 - trans).tobytes()
    assert n == 1 or (got["alpha"] > 0.5).any()


@pytest.mark.parametrize("name", [n for n in cases.NO_TIES if not n.startswith("k1")])
def test_a_permutation_of_the_layers_changes_no_byte(name):
    case, _ = cases.case_and_ref(name)
    got = run_deep(case)
    K = case["K"]
    for perm in (np.arange(K)[::-1], np.random.default_rng(7).permutation(K)):
        assert _same_bytes(run_deep(cases.permuted(case, perm)), got), perm


def test_bad_arguments_are_refused_and_nothing_is_written():
    from instantavatar_amd import _lib
    K, S, n = 2, 4, 5
    z, rgb = torch.zeros((K, S, n), device=DEV), torch.zeros((K, S, n, 3), device=DEV)
    out = [torch.full(s, 3.0, device=DEV) for s in ((n, 3), (n,), (n,))]
    count = torch.full((1,), 5, dtype=torch.int32, device=DEV)

    def deep(K=K, S=S, n=n, ground=(None,) * 4, thresh=0.01, z=z):
        return _lib.call("ia_scene_deep_composite", z, z, z, rgb, K, S, n, None, *ground, None, 0, thresh, *out, count)
    for kw in (dict(K=0), dict(K=9), dict(S=0), dict(S=1025), dict(n=-1), dict(thresh=-1.0), dict(thresh=float("nan")),
               dict(ground=(out[1], out[1], None, out[1])), dict(z=None)):
        with pytest.raises(_lib.IAError, match=r"\(-\d+\)"):
            deep(**kw)
    assert deep(n=0) == 0
    torch.cuda.synchronize()
    assert all(bool((o == 3.0).all()) for o in out) and int(count) == 5


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


@functools.lru_cache(maxsize=None)
def _vivid_model(seed):
    """a synthetic model whose colours are far from grey: the last layer of the colour network (the trailing 16 x 64 weights, in
    front of the sigmoid) times 8.  The synthetic fields' colours all lie within about 0.08 of one another (a Xavier-initialised
    network in front of a sigmoid: about 0.5 everywhere), and the difference between two orders of compositing is bounded by the
    contrast between the avatars times the weight that changes place -- two avatars that look alike cannot show it."""
    from instantavatar_amd.pipeline import build_synthetic_model
    model, _, _ = build_synthetic_model(torch.device(DEV), seed=seed)
    model.eval()
    with torch.no_grad():
        model.net_coarse.color_net.params[-16 * 64:].mul_(8.0)
    return model


def _seq(offset=(0.0, 0.0, 0.0), frames=4):
    from instantavatar_amd import scene, synthetic
    from instantavatar_amd.drivers import animate
    poses, trans = synthetic.procedural_pose_track(64)
    seq = animate.AnimateSequence(poses[:frames], trans[:frames], np.zeros(10, np.float32), torch.device(DEV), size=SIZE)
    return scene.place(seq, offset)


def _rows_case(deep, cols=None, **kw):
    """the recorded lists (device, [K,S,n]) as a case of scene_deep_refs"""
    pick = (lambda t: _np(t)) if cols is None else (lambda t: np.ascontiguousarray(_np(t)[:, :, cols]))
    return dict(z=pick(deep["z"]), delta=pick(deep["delta"]), sigma=pick(deep["sigma"]), rgb=pick(deep["rgb"]), thresh=sdr.THRESH,
                factor=kw.get("factor"), ground=kw.get("ground"), bg=kw.get("bg"))


def test_render_test_deep_records_what_the_fused_render_composites():
    from instantavatar_amd import dense_routes, scene
    from instantavatar_amd.models.structures.utils import Rays
    model, seq = _model(42), _seq()
    batch = seq.batch(1)
    batch["bg_color"] = torch.zeros((1, SIZE * SIZE, 3), device=DEV)
    with torch.no_grad():
        rgb, depth, alpha, _ = model.render_image_fast(batch, (SIZE, SIZE), jitter=_jitter())
    rgb, depth, alpha = rgb.reshape(-1, 3).clone(), depth.reshape(-1).clone(), alpha.reshape(-1).clone()
    rays = Rays(o=batch["rays_o"], d=batch["rays_d"], near=batch["near"], far=batch["far"])
    model.deformer.transform_rays_w2s(rays)
    field = lambda x, _: model.deformer(x, model.net_coarse, True)
    alive0 = torch.nonzero(alpha > 0).reshape(-1)
    n, S = int(alive0.numel()), model.renderer.MAX_SAMPLES
    assert n > 40

    def record(chunk, first=n):
        deep = scene.deep_buffers(1, S, n, DEV)
        rec = {k: v[0] for k, v in deep.items()}
        cols = torch.arange(n, device=DEV)
        outs = [dense_routes.render_test_deep(model.renderer, rays, field, alive0[c0:min(c0 + chunk, first)], rec, cols=cols[c0:min(c0 + chunk, first)])
                for c0 in range(0, first, chunk)]
        return deep, [torch.cat([o[j] for o in outs]) for j in range(3)]
    deep, (c_d, d_d, a_d) = record(4096)
    # the dense route itself is the fused one on these rays (the gate of the closure route)
    rays_within(_np((c_d - rgb[alive0]).abs().max(1).values), "render_test_deep rgb against the fused layer")
    rays_within(_np((a_d - alpha[alive0]).abs()), "render_test_deep alpha against the fused layer")
    # the recorded rows, composited alone by the float64 reference, are the fused layer on those rays
    ref = sdr.deep_ref(_rows_case(deep))
    rays_within(np.abs(ref["rgb"] - _np(rgb[alive0]).astype(np.float64)).max(1), "recorded rows (float64) rgb against the fused layer")
    rays_within(np.abs(ref["alpha"] - _np(alpha[alive0]).astype(np.float64)), "recorded rows (float64) alpha against the fused layer")
    rays_within(np.abs(ref["depth"] - _np(depth[alive0]).astype(np.float64)), "recorded rows (float64) depth against the fused layer")
    assert ref["interleaved"] == 0 and float(ref["alpha"].max()) > 0.9
    filled = _np(deep["delta"][0]) > 0
    assert filled.any() and (np.cumprod(filled, 0).astype(bool) == filled).all()        # a filled prefix per ray
    # the rows do not depend on the chunk
    deep7, _ = record(7)
    for key in ("z", "delta", "sigma", "rgb"):
        assert torch.equal(deep7[key], deep[key]), key
    deep1, _ = record(1, first=40)
    for key in ("z", "delta", "sigma", "rgb"):
        assert torch.equal(deep1[key][:, :, :40], deep[key][:, :, :40]) and not bool(deep1[key][:, :, 40:].any()), key


def _same_result(a, b, keys=("rgb", "alpha", "depth", "rgba8", "contested")):
    return all(torch.equal(a[k], b[k]) for k in keys)


def test_exact_scene_of_one_avatar_is_the_layered_one():
    from instantavatar_amd import scene
    model, seq = _model(42), _seq()
    plain = scene.Scene([model], [seq], jitter=_jitter()).render(1)
    exact = scene.Scene([model], [seq], jitter=_jitter(), exact=True).render(1)
    assert set(exact) == set(plain) | {"overlap", "interleaved"}
    assert _same_result(exact, plain) and exact["shade"] is None
    assert int(exact["overlap"]) == 0 and int(exact["interleaved"]) == 0 and exact["overlap"].dtype == torch.int32


def test_exact_scene_with_one_avatar_behind_the_other_equals_the_layered_one():
    from instantavatar_amd import scene
    ma, mb = _model(42), _model(43)
    front, back = _seq(), _seq((0.0, 0.0, 1.5))
    plain = scene.Scene([ma, mb], [front, back], jitter=_jitter()).render(0)
    sc = scene.Scene([ma, mb], [front, back], jitter=_jitter(), exact=True)
    exact = sc.render(0)
    assert int(exact["interleaved"]) == 0 and int(exact["overlap"]) > 0
    assert int(exact["overlap"]) == int(sc.last_active.numel())
    flat = lambda t: _np(t.reshape(SIZE * SIZE, -1).float())
    rays_within(np.abs(flat(exact["rgb"]) - flat(plain["rgb"])).max(1), "exact against layered, disjoint supports: rgb")
    rays_within(np.abs(flat(exact["alpha"]) - flat(plain["alpha"])).max(1), "exact against layered, disjoint supports: alpha")
    rays_within(np.abs(flat(exact["depth"]) - flat(plain["depth"])).max(1), "exact against layered, disjoint supports: depth")
    outside = torch.ones(SIZE * SIZE, dtype=torch.bool, device=DEV)
    outside[sc.last_active] = False
    for key in ("rgb", "alpha", "depth", "rgba8"):
        a, b = exact[key].reshape(SIZE * SIZE, -1), plain[key].reshape(SIZE * SIZE, -1)
        assert torch.equal(a[outside], b[outside]), key
    assert torch.equal(exact["contested"], plain["contested"])


def _against_reference(sc, exact, what):
    """the exact frame on the active pixels against the float64 reference evaluated on the recorded rows and the gathered ground,
    shade and background: pins the gathers, the scatter and the arguments of the merge"""
    rows, active = sc.last_rows, sc.last_active
    n = int(active.numel())
    take = lambda t: _np(t[active])
    case = _rows_case(sc.last_deep, factor=None if rows["factor"] is None else _np(rows["factor"][:, active]),
                      ground=None if rows["ground"] is None else tuple(take(x) for x in rows["ground"]),
                      bg=None if rows["bg"] is None else (_np(rows["bg"]) if rows["bg_const"] else take(rows["bg"].reshape(-1, 3))))
    ref = sdr.deep_ref(case)
    got = dict(rgb=take(exact["rgb"].reshape(-1, 3)), alpha=take(exact["alpha"].reshape(-1)), depth=take(exact["depth"].reshape(-1)),
               interleaved=int(exact["interleaved"]))
    sdr.deep_compare(got, ref, what)
    assert int(exact["overlap"]) == n
    return ref


def test_exact_scene_of_two_intertwined_avatars():
    from instantavatar_amd import scene
    # half a period of the pose track apart, so that limbs of one cross the other's body, and colours that differ
    ma, mb = _vivid_model(42), _vivid_model(43)
    sa, sb = _seq(frames=64), _seq((0.0, 0.0, 0.1), frames=64)
    kw = dict(jitter=_jitter(), phases=[0, 32], background=(0.2, 0.5, 0.9))
    plain = scene.Scene([ma, mb], [sa, sb], **kw).render(0)
    sc = scene.Scene([ma, mb], [sa, sb], exact=True, **kw)
    exact = sc.render(0)
    assert int(exact["interleaved"]) > 0 and int(exact["overlap"]) >= int(exact["interleaved"])
    ref = _against_reference(sc, exact, "two intertwined avatars, background")
    inter = sc.last_active[torch.as_tensor(ref["interleaved_mask"], device=DEV)]
    diff = (exact["rgb"].reshape(-1, 3)[inter] - plain["rgb"].reshape(-1, 3)[inter]).abs().max()
    rows = sc.last_rows
    contrast = (rows["c"][0][inter] / rows["a"][0][inter, None] - rows["c"][1][inter] / rows["a"][1][inter, None]).abs().max()
    print("largest difference between the two avatars' colours at an interleaved pixel: %.3f" % float(contrast))
    print("largest difference between the exact and the layered frame at an interleaved pixel: %.3f" % float(diff))
    assert float(diff) > 0.05
    assert _same_result(sc.render(0), exact, ("rgb", "alpha", "depth", "rgba8", "overlap", "interleaved"))
    # ground + light + receive: the colour factor is live; exact_ground adds the pixels where one avatar meets the ground
    ground = scene.ground_under([ma, mb], [sa, sb], color2=(0.4, 0.4, 0.4), cell=0.5)
    lit = dict(jitter=_jitter(), phases=[0, 32], ground=ground, light=(-2.0, -4.0, 2.0), shadow_size=64, receive=True)
    plain = scene.Scene([ma, mb], [sa, sb], **lit).render(0)
    sc = scene.Scene([ma, mb], [sa, sb], exact=True, exact_ground=True, **lit)
    exact = sc.render(0)
    assert set(exact) == set(plain) | {"overlap", "interleaved"} and torch.equal(exact["layer_shade"], plain["layer_shade"])
    assert bool((sc.last_rows["factor"][:, sc.last_active] < 1).any())
    ref = _against_reference(sc, exact, "two intertwined avatars, ground, light, receive, exact_ground")
    assert any(2 in o for o in ref["owners"]) and int(exact["interleaved"]) > 0
    two = scene.Scene([ma, mb], [sa, sb], exact=True, **lit).render(0)
    assert 0 < int(two["overlap"]) < int(exact["overlap"])


def test_the_budget_is_enforced():
    from instantavatar_amd import _lib, scene
    ma, mb = _model(42), _model(43)
    with pytest.raises(_lib.IAError, match=r"deep_budget = 1\b"):
        scene.Scene([ma, mb], [_seq(), _seq((0.0, 0.0, 0.1))], jitter=_jitter(), exact=True, deep_budget=1).render(0)


def test_scene_driver_exact_writes_reproducible_frames(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = []
    for name in ("one", "two"):
        out = str(tmp_path / name)
        cmd = [sys.executable, "-m", "instantavatar_amd.drivers.scene", "--synthetic", "--seeds", "42", "43", "--spacing", "0.1", "--size", "32",
               "--max-frames", "2", "--jitter-seed", "1", "--exact", "--out", out]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        assert "overlap pixels:" in r.stdout and "interleaved pixels:" in r.stdout and "warning" not in r.stdout
        assert sorted(os.listdir(out)) == ["0.png", "1.png", "scene.gif"]
        outs.append(out)
    for f in ("0.png", "1.png", "scene.gif"):
        assert open(os.path.join(outs[0], f), "rb").read() == open(os.path.join(outs[1], f), "rb").read(), f
