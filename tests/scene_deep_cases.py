"""Seeded inputs of `ia_scene_deep_composite` for tests/test_gpu_scene_deep.py and tests/test_cpu_scene_deep_refs.py, as fp32 numpy
arrays in the kernel's slot-major layout (z, delta, sigma [K,S,n], rgb [K,S,n,3]).  K in {1, 2, 3, 8}, n in {1, 70} (a wave plus a
ragged tail), S in {1, 4, 37}.  Per pixel and list the slots are a filled prefix like the renderer's: a constant step, z on the
lattice z0 + j step at the occupied j.  The lists are empty, full, partly filled, cut by their own stop (opaque samples that take
T_k below 1e-4 with filled slots behind) or carry samples under the threshold.  `mode`:
  interleaved  every list covers the same depth range on its own lattice (offset by a fraction of a step): A B A B
  ties         all lists share ONE lattice, so equal keys across lists are exact
  disjoint     list k covers a depth block of its own, the blocks in a per-pixel order and separated by gaps
Ground: None, or per pixel in front of everything, between samples (inside the depth range; between the blocks when disjoint),
behind, or not taking part (a_g = 0).  Background none, one colour or per pixel; with and without `factor`; `bad`: non-finite
sigma, rgb, z and delta sprinkled in (a non-finite z or delta ends its list: a filled prefix).
tests/test_cpu_scene_deep_refs.py asserts what every case must contain."""
import functools

import numpy as np

import scene_deep_refs as sdr

F = np.float32

#        name              K   n   S  mode           ground  bg       factor bad
CASES = (("k1_n1_s1", 1, 1, 1, "interleaved", False, None, False, False),
         ("k1_n70_s37", 1, 70, 37, "interleaved", False, None, False, False),
         ("k1_ground_bg", 1, 70, 4, "interleaved", True, "const", True, False),
         ("k2_inter", 2, 70, 37, "interleaved", False, None, False, False),
         ("k2_inter_full", 2, 70, 37, "interleaved", True, "pixel", True, False),
         ("k2_ties", 2, 70, 4, "ties", True, "const", False, False),
         ("k2_disjoint", 2, 70, 37, "disjoint", True, None, True, False),
         ("k3_inter_bad", 3, 70, 37, "interleaved", True, "pixel", True, True),
         ("k3_ties_s1", 3, 70, 1, "ties", False, None, False, False),
         ("k3_disjoint", 3, 70, 4, "disjoint", True, "const", False, False),
         ("k8_inter", 8, 70, 4, "interleaved", True, None, True, False),
         ("k8_ties_bad", 8, 70, 37, "ties", True, "const", True, True),
         ("k8_disjoint", 8, 70, 4, "disjoint", False, "pixel", False, False),
         ("k8_n1", 8, 1, 37, "interleaved", True, "const", True, False))
NAMES = tuple(c[0] for c in CASES)
DISJOINT = tuple(c[0] for c in CASES if c[4] == "disjoint")
NO_TIES = tuple(c[0] for c in CASES if c[4] != "ties")


def make(name):
    _, K, n, S, mode, with_ground, bg_kind, with_factor, bad = next(c for c in CASES if c[0] == name)
    rng = np.random.default_rng(1000 + NAMES.index(name))
    z, dl = np.zeros((K, S, n), F), np.zeros((K, S, n), F)
    sg, rgb = np.zeros((K, S, n), F), rng.uniform(0, 1, (K, S, n, 3)).astype(F)
    near, depth_range = F(2.0), F(2.0)
    block = F(depth_range / K)
    step = F(block * 0.8 / S) if mode == "disjoint" else F(depth_range / S)
    kinds = np.empty((K, n), object)
    order = np.zeros((K, n), np.int64)
    for p in range(n):
        order[:, p] = rng.permutation(K)
        for k in range(K):
            kind = ("empty", "full", "part", "stop", "faint", "mixed")[int(rng.integers(0, 6))] if n > 1 else "mixed"
            kinds[k, p] = kind
            cnt = dict(empty=0, full=S).get(kind, int(rng.integers(1, S + 1)))
            if kind == "stop":
                cnt = S
            j = np.sort(rng.choice(S, size=cnt, replace=False))
            if mode == "disjoint":
                z0 = F(near + block * F(order[k, p]))
            elif mode == "ties":
                z0 = near
            else:
                z0 = F(near + step * F((k + 1) / (K + 2.0)))
            z[k, :cnt, p] = (z0 + j.astype(F) * step).astype(F)
            dl[k, :cnt, p] = step
            x = rng.uniform(0.02, 1.2, cnt)                         # sigma delta: alpha from 0.02 to 0.7
            if kind == "stop":
                x = rng.uniform(1.4, 1.8, cnt)                       # tau about 0.2: T_k < 1e-4 after six samples, filled slots behind
            elif kind == "faint":
                x = rng.uniform(0.0, 0.008, cnt)                     # all under the threshold
            elif kind == "mixed":
                x = np.where(rng.uniform(size=cnt) < 0.3, rng.uniform(0.0, 0.008, cnt), x)
            sg[k, :cnt, p] = (x / float(step)).astype(F)
    case = dict(name=name, K=K, S=S, n=n, mode=mode, z=z, delta=dl, sigma=sg, rgb=rgb, thresh=sdr.THRESH, kinds=kinds, factor=None,
                ground=None, bg=None, ground_where=None)
    if bad:
        for arr, vals in ((sg, (np.nan, np.inf, -np.inf)), (rgb, (np.nan, np.inf)), (z, (np.nan, np.inf, -np.inf)), (dl, (np.nan, -np.inf))):
            flat = arr.reshape(-1)
            at = rng.choice(flat.size, size=max(3, flat.size // 200), replace=False)
            flat[at] = rng.choice(vals, size=at.size).astype(F)
    if with_factor:
        case["factor"] = rng.uniform(0.4, 1.0, (K, n)).astype(F)
    if with_ground:
        where = np.array(["front", "between", "behind", "absent"])[np.arange(n) % 4] if n > 1 else np.array(["between"])
        t_g = np.zeros(n, F)
        for p in range(n):
            if where[p] == "between" and mode == "disjoint":
                t_g[p] = F(near + block * F(int(rng.integers(1, K)) if K > 1 else 1) - block * F(0.1))      # in the gap before a block
            else:
                t_g[p] = dict(front=F(1.0), behind=F(10.0), absent=F(3.0)).get(where[p], F(near + depth_range * F(rng.uniform(0.2, 0.8))))
        a_g = np.where(where == "absent", 0, rng.uniform(0.3, 1.0, n)).astype(F)
        case["ground"] = (t_g, a_g, rng.uniform(0, 1, (n, 3)).astype(F), rng.uniform(0.4, 1.0, n).astype(F))
        case["ground_where"] = where
    if bg_kind == "const":
        case["bg"] = np.array([0.2, 0.5, 0.9], F)
    elif bg_kind == "pixel":
        case["bg"] = rng.uniform(0, 1, (n, 3)).astype(F)
    return case


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    """(the case, scene_deep_refs.deep_ref of it), computed once per process and shared: read, never written"""
    case = make(name)
    return case, sdr.deep_ref(case)


def permuted(case, perm):
    """the same case with its lists in another order"""
    perm = np.asarray(perm)
    out = dict(case)
    for key in ("z", "delta", "sigma", "rgb"):
        out[key] = np.ascontiguousarray(case[key][perm])
    if case["factor"] is not None:
        out["factor"] = np.ascontiguousarray(case["factor"][perm])
    return out


def single(case, k):
    """list k of a case alone: no factor, ground or background"""
    out = dict(case, K=1, factor=None, ground=None, bg=None)
    for key in ("z", "delta", "sigma", "rgb"):
        out[key] = np.ascontiguousarray(case[key][k:k + 1])
    return out
