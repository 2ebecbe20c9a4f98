"""Seeded inputs of `ia_scene_receive` for tests/test_gpu_scene_receive.py and tests/test_cpu_scene_receive_refs.py, as fp32 numpy
arrays, at the smallest shapes at which the kernel can still go wrong: R = 1 (one thread), 65 (a wavefront plus one) and 200 (a
partial workgroup), K = 1, 2, 3, 8, maps of 1^2, 8^2 and 16^2 texels, PCF radii 0 .. 3, normals given / given with zero rows / NULL.

Geometry of the seeded cases: a fan of unit rays from the origin around +z (ray 0 is +z itself), layer j about 2 + 0.4 j metres
along them, a light above and behind the camera whose K cameras look at the middle of the layers with slightly different focal
lengths, so that the fan is wider than every map (receivers outside every map).  A map's left third carries a depth far behind
every receiver (never occluding), its right third one right in front of the light (always occluding), the middle third depths in
the receivers' range; a quarter of the texels has m = 0, a quarter m = 1, a few depth sums are NaN.  Every seventh pixel holds a
layer that must not receive (a = 0, a < 0, NaN or inf in c, a, d), every eleventh a layer with a negative depth sum: a receiver
behind the camera and behind the light's near plane.  tests/test_cpu_scene_receive_refs.py asserts what every case must contain."""
import functools

import numpy as np

import scene_receive_refs as srr

LIGHT =(0.4, -1.5, -0.5)
AXIS_LIGHT = (0.0, 0.0, -1.0)


def look_at(eye, target, S, f):
    """K [R | t] [3,4] fp32 of a camera at `eye` looking at `target` with focal length f and the principal point at (S - 1) / 2"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    down = np.array([0.0, 1.0, 0.0]) if abs(z[1]) <= 0.99 else np.array([0.0, 0.0, 1.0])
    x = np.cross(down, z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    Km = np.array([[f, 0, (S - 1) / 2], [0, f, (S - 1) / 2], [0, 0, 1.0]])
    return (Km @ np.concatenate([Rm, (-Rm @ eye)[:, None]], 1)).astype(np.float32)


def fan(R, spread=0.25, shift=0.0):
    """R unit rays from the origin around +z (shifted sideways by `shift`); ray 0 is (0, 0, 1) exactly"""
    n = int(np.ceil(np.sqrt(R)))
    g = np.stack(np.meshgrid(np.linspace(-spread, spread, n), np.linspace(-spread, spread, n), indexing="xy"), -1).reshape(-1, 2)[:R] + shift
    d = np.concatenate([g, np.ones((R, 1))], 1)
    d[0] = (0.0, 0.0, 1.0)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.zeros((R, 3), np.float32), d.astype(np.float32)


def make(R, K, S, radius, seed, normals="given", strength=0.6, cos=(0.0, 0.25), bias=(0.02, 0.05), light=LIGHT):
    rng = np.random.default_rng(seed)
    # (S = 1: no ray but ray 0 may have a coordinate of exactly 0, which is the border of a one-texel map)
    o, dr = fan(R, shift=0.013 if S == 1 else 0.0)
    px = np.arange(R)
    z = (2.0 + 0.4 * np.arange(K)[:, None] + rng.uniform(-0.1, 0.1, (K, R))).astype(np.float32)
    a = rng.uniform(0.05, 1.0, (K, R)).astype(np.float32)
    a[rng.uniform(size=(K, R)) < 0.3] = 1.0
    col = rng.uniform(0, 1, (K, R, 3)).astype(np.float32)
    behind = px % 11 == 5                                                              # behind the camera and the light's near plane
    z[0, behind] = -3.0
    c, d = col * a[..., None], a * z
    kinds = [("a", 0.0), ("a", -0.25), ("c", np.nan), ("a", np.inf), ("d", np.nan), ("d", -np.inf), ("c", np.inf), ("a", np.nan)]
    for n, r in enumerate(range(3 if R > 3 else 0, R, 7)):                            # layers that must not receive
        name, v = kinds[n % len(kinds)]
        k = n % K
        if name == "c":
            c[k, r, n % 3] = v
        else:
            dict(a=a, d=d)[name][k, r] = v
    L = np.asarray(light, np.float64)
    if S == 1:          # one texel: only a receiver on the optical axis lies inside it (u = v = 0 exactly), so the light is on ray 0
        proj = np.stack([look_at(light, (0.0, 0.0, 3.0), 1, 1.0 + k) for k in range(K)])
    else:
        proj = np.stack([look_at(light, (0.0, 0.0, 2.0 + 0.2 * K), S, (S - 1) / 2.0 * 4.0 / (0.5 + 0.05 * k)) for k in range(K)])
    maps_a = rng.uniform(0.05, 1.0, (K, S, S)).astype(np.float32)
    maps_a[rng.uniform(size=(K, S, S)) < 0.25] = 1.0
    maps_a[rng.uniform(size=(K, S, S)) < 0.25] = 0.0
    mean = rng.uniform(2.5, 5.5, (K, S, S))
    if S > 1:
        mean[:, :, : S // 3] = 40.0
        mean[:, :, S - S // 3:] = 0.5
        maps_a[:, S // 2, S // 2] = 0.0                                                 # m = 0 next to the centre, whatever the seed
        maps_a[:, S // 2, S // 2 - 1] = 0.75
    else:
        maps_a[:] = 1.0
        mean[:] = 0.5 + 2.4 * (np.arange(K) % 2)[:, None, None]                        # right at the light, and between layers 0 and 1
    maps_d = (maps_a * mean).astype(np.float32)
    if S > 1:
        maps_d[:, S // 2, S // 2 - 1] = np.nan                                          # a NaN depth sum under m > 0
        maps_d[rng.uniform(size=(K, S, S)) < 0.03] = np.nan
    nrm = None
    if normals != "null":
        X = o[None].astype(np.float64) + z[..., None].astype(np.float64) * dr[None].astype(np.float64)
        n = L[None, None] - X
        n = n / np.linalg.norm(n, axis=-1, keepdims=True) + rng.normal(0, 0.6, (K, R, 3))
        away = rng.uniform(size=(K, R)) < 0.3
        n[away] = -n[away]
        nrm = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
        if normals == "zero_rows":
            nrm[:, px % 3 == 1] = 0.0
            nrm[0, px % 13 == 2, 1] = np.nan                                           # not finite: no facing term either
    return dict(rays_o=o, rays_d=dr, c=c.astype(np.float32), a=a, d=d.astype(np.float32), nrm=nrm, maps_a=maps_a, maps_d=maps_d, proj=proj,
                light=np.asarray(light, np.float32), radius=radius, strength=np.float32(strength), near=np.float32(0.05),
                bias_other=np.float32(bias[0]), bias_self=np.float32(bias[1]), cos0=np.float32(cos[0]), cos1=np.float32(cos[1]),
                K=K, R=R, S=S)


def make_one_ray(bias=(0.02, 0.05)):
    """One ray, three layers.  Layer 1 stands at 2.0 m, layer 0 at 2.6 m behind it, layer 2 has a = 0 and an empty map.  The maps of
    layers 0 and 1 are opaque everywhere at their own distance from the light minus 3 cm: against bias_self = 5 cm neither shadows
    itself, against bias_other = 2 cm layer 1 shadows layer 0 -- and would shadow itself if its own map were held to bias_other."""
    S = 8
    o, dr = fan(1)
    L = np.asarray(LIGHT, np.float64)
    z = np.array([[2.6], [2.0], [2.3]], np.float32)
    a = np.array([[0.9], [0.8], [0.0]], np.float32)
    col = np.array([[[0.2, 0.5, 0.8]], [[0.9, 0.4, 0.1]], [[0.3, 0.3, 0.3]]], np.float32)
    X = z[..., None].astype(np.float64) * dr[None].astype(np.float64)
    rho = np.linalg.norm(X - L, axis=-1)[:, 0]
    proj = np.stack([look_at(LIGHT, (0.0, 0.0, 2.3), S, (S - 1) / 2.0 * 3.0 / (1.0 + 0.1 * k)) for k in range(3)])
    maps_a = np.ones((3, S, S), np.float32)
    maps_a[2] = 0.0
    maps_d = (maps_a * (rho - 0.03)[:, None, None]).astype(np.float32)
    return dict(rays_o=o, rays_d=dr, c=col * a[..., None], a=a, d=a * z, nrm=None, maps_a=maps_a, maps_d=maps_d, proj=proj,
                light=np.asarray(LIGHT, np.float32), radius=1, strength=np.float32(0.6), near=np.float32(0.05),
                bias_other=np.float32(bias[0]), bias_self=np.float32(bias[1]), cos0=np.float32(0.0), cos1=np.float32(0.25), K=3, R=1, S=S)


CASES = {
    "R1_K3_S8_r1_self_bias": make_one_ray,
    "R65_K1_S8_r1_normals": lambda: make(65, 1, 8, 1, 11),
    "R65_K2_S16_r2_zero_rows_strength1": lambda: make(65, 2, 16, 2, 12, normals="zero_rows", strength=1.0),
    "R200_K3_S8_r3_null": lambda: make(200, 3, 8, 3, 13, normals="null"),
    "R65_K8_S16_r1_ramp": lambda: make(65, 8, 16, 1, 14, cos=(-0.2, 0.6), bias=(0.0, 0.1)),
    "R200_K2_S16_r0_strength0": lambda: make(200, 2, 16, 0, 15, normals="zero_rows", strength=0.0),
    "R200_K2_S1_r1_axis": lambda: make(200, 2, 1, 1, 16, normals="null", light=AXIS_LIGHT),
    "R65_K3_S16_r3_zero_rows": lambda: make(65, 3, 16, 3, 17, normals="zero_rows"),
}


@functools.lru_cache(maxsize=None)
def case_and_reference(name):
    """(the case, scene_receive_refs.receive of it), computed once per process and shared: read, never written"""
    case = CASES[name]()
    return case, srr.receive(**arguments(case))


def arguments(case):
    """the arguments of scene_receive_refs.receive"""
    return dict(rays_o=case["rays_o"], rays_d=case["rays_d"], c=case["c"], a=case["a"], d=case["d"], nrm=case["nrm"], maps_a=case["maps_a"],
                maps_d=case["maps_d"], proj=case["proj"], light=case["light"], radius=case["radius"], strength=case["strength"],
                near=case["near"], bias_other=case["bias_other"], bias_self=case["bias_self"], cos0=case["cos0"], cos1=case["cos1"])
