"""The inputs of tests/test_gpu_scene.py for the three scene-composition entry points, as fp32 numpy arrays, built so that no
discrete choice can flip between the kernels' fp32 and the reference's fp64: the keys of a pixel sit on a ladder with 0.6 m between
its rungs (distinct keys differ by more than 1e-3 relative, opaque pairs stay away from the `contact` threshold), checker
coordinates stay more than 1e-4 cells from a cell border.  tests/test_cpu_scene_refs.py checks on the CPU that they do.
Shapes: 5 x 7 and 33 x 65 pixels (neither a multiple of a wavefront; the second more than one workgroup)."""
import numpy as np

import scene_refs as sr

SHAPES = {"small": (5, 7), "large": (33, 65)}
CONTACT = 0.3


def make_composite(shape, K, seed, ground=False, background=None, bad=False, ties=False, close=False):
    H, W = SHAPES[shape]
    R = H * W
    rng = np.random.default_rng(seed)
    px = np.arange(R)
    # rung s of the ladder: z = 2 + 0.6 s +- 0.05; every pixel deals the rungs to its layers and the ground in another order
    slots = np.stack([rng.permutation(K + 1) for _ in range(R)], 1)                          # [K+1,R]
    z = (2.0 + 0.6 * slots + rng.uniform(-0.05, 0.05, (K + 1, R))).astype(np.float32)
    a = rng.uniform(0.05, 1.0, (K, R)).astype(np.float32)
    a[np.abs(a - 0.5) < 0.01] = 0.6                                                          # (the a >= 0.5 test of `contested`)
    a[rng.uniform(size=(K, R)) < 0.2] = 1.0
    a[rng.uniform(size=(K, R)) < 0.15] = 0.0
    if close and K >= 2:                                                                     # two opaque layers 0.1 m apart
        sel = px % 4 == 1
        a[0, sel] = a[1, sel] = 0.9
        z[1, sel] = z[0, sel] + np.float32(0.1)
    col = rng.uniform(0, 1, (K, R, 3)).astype(np.float32)
    c = col * a[..., None]
    d = a * z[:K]
    g = None
    if ground:
        t_g = z[K].copy()
        a_g = rng.uniform(0.05, 1.0, R).astype(np.float32)
        a_g[px % 3 == 0] = 1.0
        miss = px % 11 == 5
        t_g[miss], a_g[miss] = 0.0, 0.0
        c_g = rng.uniform(0, 1, (R, 3)).astype(np.float32)
        c_g[miss] = 0.0
        shade = rng.uniform(0.3, 1.0, R).astype(np.float32)
        g = [t_g, a_g, c_g, shade]
        if ties:                                                                             # layer 0 exactly at the ground's depth
            sel = (px % 7 == 3) & ~miss
            a[0, sel] = 1.0
            d[0, sel] = t_g[sel]
            c[0, sel] = col[0, sel]
    if ties and K >= 2:                                                                      # two layers with identical bit patterns of a and d
        sel = px % 5 == 0
        a[K - 1, sel], d[K - 1, sel] = a[0, sel], d[0, sel]
        c[K - 1, sel] = col[K - 1, sel] * a[K - 1, sel, None]
    if bad:                                                                                  # layers that must not take part
        kinds = [(c, np.nan), (c, np.inf), (a, np.nan), (a, np.inf), (d, np.nan), (d, -np.inf), (a, -0.25)]
        for r in range(0, R, 3):
            arr, v = kinds[(r // 3) % len(kinds)]
            k = (r // 3) % K
            if arr is c:
                c[k, r, (r // 3) % 3] = v
            else:
                arr[k, r] = v
        if g is not None:
            g[3][px % 13 == 2] = np.nan                                                      # a ground that does not take part
            g[0][px % 13 == 6] = np.inf
    bg = None
    if background == "image":
        bg = rng.uniform(0, 1, (R, 3)).astype(np.float32)
    elif background == "const":
        bg = np.array([0.25, 0.5, 0.75], np.float32)
    return dict(c=c, a=a, d=d, ground=g, background=bg, contact=CONTACT, K=K, R=R,
                expect_ties=ties, expect_contested=None, close=bool(close and K >= 2))


def contact_margin(case):
    """the smallest | |z_i - z_j| - contact | / contact over the pairs of layers that take part with a >= 0.5 (inf: none)"""
    c, a, d = (np.asarray(x, np.float64) for x in (case["c"], case["a"], case["d"]))
    K = a.shape[0]
    with np.errstate(all="ignore"):
        ok = (a > 0) & np.isfinite(a) & np.isfinite(d) & np.isfinite(c).all(-1) & (a >= 0.5)
        z = d / a
    best = np.inf
    for i in range(K):
        for j in range(i + 1, K):
            both = ok[i] & ok[j]
            if both.any():
                best = min(best, float(np.min(np.abs(np.abs(z[i, both] - z[j, both]) - case["contact"]))) / case["contact"])
    return best


COMPOSITE = {
    "small_K1": lambda: make_composite("small", 1, 1),
    "small_K2_bad_bg": lambda: make_composite("small", 2, 2, background="const", bad=True),
    "small_K3_ground_ties": lambda: make_composite("small", 3, 3, ground=True, ties=True),
    "small_K8_all": lambda: make_composite("small", 8, 4, ground=True, background="image", bad=True, ties=True, close=True),
    "large_K1_ground_bad": lambda: make_composite("large", 1, 5, ground=True, bad=True, ties=True),
    "large_K2_close": lambda: make_composite("large", 2, 6, close=True, ties=True),
    "large_K3_bg": lambda: make_composite("large", 3, 7, background="image", bad=True, close=True),
    "large_K8_all": lambda: make_composite("large", 8, 8, ground=True, background="const", bad=True, ties=True, close=True),
}


def _pinhole(H, W, f, eye, pitch):
    """rays of a pinhole at `eye` pitched down by `pitch` radians (+y is down), unit directions, fp32"""
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(i - (W - 1) / 2) / f, (j - (H - 1) / 2) / f, np.ones_like(i, float)], -1).reshape(-1, 3)
    cp, sp = np.cos(pitch), np.sin(pitch)
    d = d @ np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]]).T                              # y' = cp y + sp z: forward tips towards +y
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(np.asarray(eye, np.float32), (H * W, 1)), d.astype(np.float32)


def make_ground(shape, normal, cell, seed, r0, r1, pitch=0.35):
    H, W = SHAPES[shape]
    n = np.asarray(normal, np.float64)
    n = (n / np.linalg.norm(n)).astype(np.float32)
    o, d = _pinhole(H, W, 0.9 * W, (0.1, -0.4, 0.2), pitch)
    # the first four rays must not hit: parallel to the plane, away from it, from below it, and with the plane behind the origin
    e1, _ = sr.plane_axes(n)
    d[0] = e1.astype(np.float32)
    d[1] = n
    o[2] = (o[2].astype(np.float64) - 5.0 * n).astype(np.float32)
    up = n.astype(np.float64) + 0.3 * e1                      # the plane lies behind this ray's origin: t < 0
    d[3] = (up / np.linalg.norm(up)).astype(np.float32)
    plane = dict(normal=n, h=np.float32(-1.0), g0=(0.8, 0.7, 0.6), g1=(0.15, 0.2, 0.3), cell=np.float32(cell), centre=(0.2, 0.0, 3.0), r0=r0, r1=r1)
    plane["centre"] = tuple(np.float32(np.asarray(plane["centre"]) - (np.asarray(plane["centre"]) @ n.astype(np.float64) + 1.0) * n.astype(np.float64)))
    if cell > 0:                                              # rays whose checker coordinates come too close to a border become misses
        near = sr.ground(o, d, **plane)["cell_margins"] < 1e-3
        d[near] = n
    return dict(rays_o=o, rays_d=d, plane=plane, expect_misses=True)


GROUND = {
    "small_floor_checker": lambda: make_ground("small", (0, -1, 0), 0.37, 1, 2.0, 4.0),
    "small_tilted_plain": lambda: make_ground("small", (0.3, -0.9, 0.1), 0.0, 2, 1.0, 1.0),
    "large_floor_checker": lambda: make_ground("large", (0, -1, 0), 0.21, 3, 1.5, 6.0),
    "large_tilted_checker": lambda: make_ground("large", (-0.2, -0.95, 0.25), 0.5, 4, 0.0, 3.0, pitch=0.5),
}


def _look_at(eye, target, S, f):
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross([0.0, 0.0, 1.0], z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    Rm = np.stack([x, y, z])
    K = np.array([[f, 0, (S - 1) / 2], [0, f, (S - 1) / 2], [0, 0, 1.0]])
    return (K @ np.concatenate([Rm, (-Rm @ eye)[:, None]], 1)).astype(np.float32)


def make_shadow(shape, K, S, radius, seed):
    """ground points on the floor y = 1 under K lights about 3 m above it; the maps cover about 2 m, the points 3 m: some fall
    outside, some within a pixel of the border; a few points lie above the lights (behind their cameras)"""
    H, W = SHAPES[shape]
    R = H * W
    rng = np.random.default_rng(seed)
    P = np.stack([rng.uniform(-1.5, 1.5, R), np.ones(R), rng.uniform(-1.5, 1.5, R)], 1).astype(np.float32)
    P[::9, 1] = -6.0
    a_g = rng.uniform(0.1, 1.0, R).astype(np.float32)
    a_g[::5] = 0.0
    maps = rng.uniform(0, 1, (K, S, S)).astype(np.float32)
    maps[:, : S // 2] = np.round(maps[:, : S // 2])                                      # hard edges in one half, soft values in the other
    proj = np.stack([_look_at((0.4 * k - 0.3, -2.0 - 0.2 * k, 0.3 - 0.2 * k), (0.1 * k, 1.0, 0.0), S, (S - 1) / 2.0 * 3.0 / 1.0)
                     for k in range(K)])
    return dict(P=P, a_g=a_g, maps=maps, proj=proj, radius=radius, strength=np.float32(0.6 + 0.1 * (seed % 4)), near=np.float32(0.05), K=K, S=S)


SHADOW = {
    "small_K1_S4_r0": lambda: make_shadow("small", 1, 4, 0, 1),
    "small_K2_S17_r3": lambda: make_shadow("small", 2, 17, 3, 2),
    "large_K3_S4_r3": lambda: make_shadow("large", 3, 4, 3, 3),
    "large_K1_S17_r0": lambda: make_shadow("large", 1, 17, 0, 4),
    "large_K8_S17_r1": lambda: make_shadow("large", 8, 17, 1, 5),
}
