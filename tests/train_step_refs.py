"""References, seeded input sets and bounds for the forward half of a training step: the compacting marcher
(`ia_march_train_compact`), the fused loss (`ia_nerf_loss`), the ray set-up (`ia_transform_rays_w2s`) and the frame
statistics (`ia_frame_stats`).  numpy only: no GPU, no product import.

The marcher is pinned BIT FOR BIT.  The library is built with -ffp-contract=off, the kernel spells its one FMA (the cell
position), the oracle's `orc_raymarch_train` spells the same one, and nothing on the path is a transcendental: the dense
depths of the oracle, compacted here in plain float32 with one rounding per spelled operation, are what a correct kernel
writes.  `march_train_compact_emulated` restates the KERNEL's algorithm (lane-owned runs, running-sum replay, two exclusive
scans, slot cap, kept count); tests/test_cpu_train_step_refs.py shows that it equals the reference on every input set and
that one-line mutants of it do not pass `march_compare`, the comparison the GPU test makes.

The other three are float64 references with bounds |got - ref| <= K u M, u = 2^-24, K counted from the kernel source next
to each definition.  Nothing in a bound comes from a kernel's output.  Device expf and logf are taken at 1 ulp (= 2 u
relative), sqrtf at 1 ulp, as the HIP math API documents them ("HIP math API", single precision floating-point functions:
expf 1, logf 1, sqrtf 1 ULP); tests/mlp_refs.py and tests/backward_refs.py take expf from the same table.
"""
import ctypes as C
import functools

import numpy as np

U = 2.0 ** -24
F = np.float32
IA_MT_RAYS = 8            # rays (waves) per workgroup of k_march_train_compact
SPL_MAX = 8               # steps per lane the kernel holds in registers
SENT_F = F(-7777.0)       # prefill of the float outputs
SENT_I = np.int32(-12345)  # prefill of s_slot


# =====================================================================================================================
# marcher
# =====================================================================================================================
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding: the product of two float32 is exact in float64; the float64 sum is rounded to odd
    (TwoSum gives its error; an inexact sum with an even last bit moves to its odd neighbour on the side of the true value),
    and a round-to-odd float64 rounds to float32 as the exact value does (53 >= 24 + 2 bits)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    s = np.ascontiguousarray(s)
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F)


def running_sum(near, dt, K):
    """t_0 = near, t_{k+1} = fl(t_k + dt): the float32 values of the reference loop's `t += dt`, [n, K]"""
    ts = np.empty((len(near), K), F)
    t = np.asarray(near, F).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            ts[:, k] = t
            t = (t + dt).astype(F)
    return ts


def step_size(near, far, max_samples):
    with np.errstate(invalid="ignore"):
        return ((np.asarray(far, F) - np.asarray(near, F)) / F(max_samples)).astype(F)


def loop_steps(near, far, max_samples, extra=8):
    """how many steps `while (t < far) t += dt` takes when no slot cap stops it (counted up to max_samples + extra)"""
    ts = running_sum(near, step_size(near, far, max_samples), max_samples + extra)
    with np.errstate(invalid="ignore"):
        return np.logical_and.accumulate(ts < np.asarray(far, F)[:, None], axis=1).sum(1)      # the loop ends at the first failed test


def cell_occupied(t, o, d, occ_bool, aabb, fma=True):
    """occupancy of the points o + t d (t [n, ...], o / d [n, 3]) as raymarcher.cu:49-52 tests it: position by one FMA,
    (x - min) * (G / (max - min)) in float32, clamped to [0, G - 1], truncated.  Non-finite t gives an arbitrary cell."""
    G = occ_bool.shape[0]
    aabb = np.asarray(aabb, F)
    sc = (F(G) / (aabb[1] - aabb[0])).astype(F)
    shp = (len(o),) + (1,) * (t.ndim - 1)
    idx = []
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            da, oa = d[:, a].reshape(shp), o[:, a].reshape(shp)
            x = fma32(t, da, oa) if fma else ((t * da).astype(F) + oa).astype(F)
            f = ((x - aabb[0, a]).astype(F) * sc[a]).astype(F)
            f = np.fmax(F(0), np.fmin(f, F(G - 1)))
            idx.append(np.nan_to_num(f, nan=0.0).astype(np.int64))
    return occ_bool[idx[0], idx[1], idx[2]]


def dense_depths_oracle(orc, o, d, near, far, occ_bool, aabb, max_samples):
    """[n, max_samples] depths of the oracle's raymarch_train (zeros where no sample), step = fl32((far - near) / max_samples)"""
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    near, far = np.ascontiguousarray(near, F), np.ascontiguousarray(far, F)
    aabb = np.asarray(aabb, F)
    step = np.ascontiguousarray(step_size(near, far, max_samples))
    offset, scale = np.ascontiguousarray(aabb[0]), np.ascontiguousarray(aabb[1] - aabb[0])
    occ8 = np.ascontiguousarray(occ_bool, np.uint8)
    z = np.zeros((len(o), max_samples), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    orc.lib().orc_raymarch_train(p(o), p(d), p(near), p(far), C.c_long(len(o)), p(occ8), int(occ8.shape[0]), p(scale), p(offset),
                                 p(step), int(max_samples), p(z))
    return z


def compact_from_dense(z, o, d, near, far, max_samples, jitter):
    """The compaction of dense depths in the kernel's order, float32, one rounding per operation: per ray the slots with
    z > 0 in slot order; s_slot = the dense slot; s_z = fl(t + fl(j dt)); s_pts = fl(fl(s_z d) + o).  Samples of ray n sit
    at [ray_start[n], ray_start[n] + ray_cnt[n]) of the returned arrays (ray order)."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    dt = step_size(near, far, max_samples)
    keep = z > 0
    ray, slot = np.nonzero(keep)
    j = F(0.5) if jitter is None else np.asarray(jitter, F).reshape(len(o), max_samples)[ray, slot]
    s_z = (z[ray, slot] + (j * dt[ray]).astype(F)).astype(F)
    s_pts = ((s_z[:, None] * d[ray]).astype(F) + o[ray]).astype(F)
    cnt = keep.sum(1).astype(np.int32)
    start = (np.cumsum(cnt) - cnt).astype(np.int64)
    return dict(ray_cnt=cnt, ray_start=start, s_slot=slot.astype(np.int32), s_z=s_z, s_pts=s_pts.reshape(-1, 3), n_samples=int(cnt.sum()))


def march_train_compact_ref(o, d, near, far, occ_bool, aabb, max_samples, jitter, orc=None):
    """What `ia_march_train_compact` must write, exactly (see the module text)."""
    if orc is None:
        from oracle import oracle as orc
    z = dense_depths_oracle(orc, o, d, near, far, occ_bool, aabb, max_samples)
    ref = compact_from_dense(z, o, d, near, far, max_samples, jitter)
    ref["dense"] = z
    return ref


MARCH_MUTANTS = ("lane_mul", "no_cap", "keep_ge", "jitter_compact", "spl_short", "no_fma", "kept_as_slot", "no_dt_guard")


def march_train_compact_emulated(o, d, near, far, occ_bool, aabb, max_samples, jitter, mutant=None, sample_cap=None, size=None):
    """k_march_train_compact in numpy, float32: one wave per ray, lane l owns the `spl` consecutive steps from l * spl,
    reached by replaying the running sum; occupied steps take slots (exclusive scan over the lanes), slots >= max_samples
    are dropped (and no step counts unless dt > 0: with far < near the sum falls below far), the kept ones (t > 0) take compact positions (second exclusive scan); jitter is read by slot.  Workgroups
    take their ranges in index order (one of the orders the atomic allows).  Returns the kernel's outputs, buffers of
    `size` elements prefilled with the sentinels and written below `sample_cap` only.
    mutant: one of MARCH_MUTANTS
      lane_mul        lane start t0 + (lane spl) dt by multiplication
      no_cap          no slot cap
      keep_ge         kept test t >= 0
      jitter_compact  jitter indexed by the compact position
      spl_short       spl = ceil(max_samples / 64)
      no_fma          cell position as fl(fl(t d) + o)
      kept_as_slot    the kept count written as the slot index
      no_dt_guard     steps of a falling running sum (far < near, dt < 0) admitted: the kernel before this file existed"""
    assert mutant is None or mutant in MARCH_MUTANTS
    o, d, near, far = np.asarray(o, F), np.asarray(d, F), np.asarray(near, F), np.asarray(far, F)
    n, ms = len(o), int(max_samples)
    spl = (ms + 63) // 64 if mutant == "spl_short" else (ms + 2 + 63) // 64
    assert 1 <= spl <= SPL_MAX
    dt = step_size(near, far, ms)
    lane = np.arange(64)
    with np.errstate(invalid="ignore", over="ignore"):
        if mutant == "lane_mul":
            t = (near[:, None] + ((lane * spl).astype(F)[None, :] * dt[:, None]).astype(F)).astype(F)
        else:
            t = running_sum(near, dt, 63 * spl + 1)[:, lane * spl]
        tk = np.zeros((n, 64, SPL_MAX), F)
        occf = np.zeros((n, 64, SPL_MAX), bool)
        for q in range(SPL_MAX):
            tk[:, :, q] = t
            if q < spl:
                fwd = np.ones_like(dt, bool) if mutant == "no_dt_guard" else dt > 0
                occf[:, :, q] = fwd[:, None] & (t < far[:, None]) & cell_occupied(t, o, d, occ_bool, aabb, fma=mutant != "no_fma")
            t = (t + dt[:, None]).astype(F)
        c = occf.sum(2)
        excl_c = np.cumsum(c, 1) - c
        sl = excl_c.copy()
        kcnt = np.zeros((n, 64), np.int64)
        keep = np.zeros_like(occf)
        for q in range(SPL_MAX):
            f = occf[:, :, q].copy()
            if mutant != "no_cap":
                occf[:, :, q] = f & (sl < ms)
            sl = sl + f
            keep[:, :, q] = occf[:, :, q] & ((tk[:, :, q] >= 0) if mutant == "keep_ge" else (tk[:, :, q] > 0))
            kcnt += keep[:, :, q]
    excl_k = np.cumsum(kcnt, 1) - kcnt
    tot_k = kcnt.sum(1)
    base = np.cumsum(tot_k) - tot_k
    total = int(tot_k.sum())
    size = max(total, 1) if size is None else int(size)
    cap = size if sample_cap is None else int(sample_cap)
    assert cap <= size
    s_pts, s_z, s_slot = np.full((size, 3), SENT_F, F), np.full(size, SENT_F, F), np.full(size, SENT_I, np.int32)
    jit = None if jitter is None else np.asarray(jitter, F).reshape(-1)
    sl, kept = excl_c.copy(), excl_k.copy()
    rows = np.arange(n)[:, None] * np.ones((1, 64), np.int64)
    for q in range(SPL_MAX):
        pos = base[:, None] + kept
        w = keep[:, :, q] & (pos < cap)
        if w.any():
            r, p, tt, s, k = rows[w], pos[w], tk[:, :, q][w], sl[w], kept[w]
            if jit is None:
                j = F(0.5)
            else:
                j = jit[np.minimum(r * ms + (k if mutant == "jitter_compact" else s), len(jit) - 1)]
            zj = (tt + (j * dt[r]).astype(F)).astype(F)
            s_z[p] = zj
            s_slot[p] = k if mutant == "kept_as_slot" else s
            s_pts[p] = ((zj[:, None] * d[r]).astype(F) + o[r]).astype(F)
        kept = kept + keep[:, :, q]
        sl = sl + occf[:, :, q]
    return dict(s_pts=s_pts, s_z=s_z, s_slot=s_slot, ray_off=base.astype(np.int32), ray_cnt=tot_k.astype(np.int32), n_samples=total)


def march_compare(got, ref, sample_cap=None):
    """The comparison of the GPU test.  got: the kernel's outputs (s_pts [size, 3], s_z, s_slot [size], ray_off, ray_cnt [n],
    n_samples), buffers prefilled with the sentinels; ref: `march_train_compact_ref`.  Asserts: n_samples and ray_cnt exact;
    the ranges [ray_off, ray_off + ray_cnt) of the rays that have samples tile [0, n_samples) disjointly in any order; every
    position below min(n_samples, sample_cap) holds, bit for bit, the reference sample its ray_off assigns to it; every other
    position holds the sentinel."""
    total = ref["n_samples"]
    assert int(got["n_samples"]) == total, ("n_samples", int(got["n_samples"]), total)
    cnt, off = np.asarray(got["ray_cnt"], np.int64), np.asarray(got["ray_off"], np.int64)
    bad = np.nonzero(cnt != ref["ray_cnt"])[0]
    assert bad.size == 0, ("ray_cnt differs", bad[:8].tolist(), cnt[bad[:8]].tolist(), ref["ray_cnt"][bad[:8]].tolist())
    has = np.nonzero(cnt > 0)[0]
    order = has[np.argsort(off[has], kind="stable")]
    ends = off[order] + cnt[order]
    assert (off[order] == np.concatenate([[0], ends[:-1]])).all() and (ends[-1] if order.size else 0) == total, \
        ("the rays' ranges do not tile [0, n_samples)", off[order][:8].tolist(), cnt[order][:8].tolist())
    size = len(got["s_z"])
    cap = size if sample_cap is None else int(sample_cap)
    assert min(total, cap) <= size
    ray = np.repeat(np.arange(len(cnt)), cnt)
    pos = off[ray] + (np.arange(total) - ref["ray_start"][ray])
    m = pos < cap
    for k, sent in (("s_slot", SENT_I), ("s_z", SENT_F), ("s_pts", SENT_F)):
        g = np.ascontiguousarray(got[k])
        want = np.full(g.shape, sent, g.dtype)
        want[pos[m]] = ref[k][m]
        diff = np.nonzero((g.view(np.uint32) != want.view(np.uint32)).reshape(size, -1).any(1))[0]
        if diff.size:
            p = int(diff[0])
            raise AssertionError((k, "differs at %d of %d positions, first %d" % (diff.size, size, p), "got", g[p].tolist(), "want", want[p].tolist(),
                                  "n_samples", total, "cap", cap))


# ---- input sets ------------------------------------------------------------------------------------------------------
MARCH_MS = (1, 2, 62, 63, 64, 126, 127, 190, 256, 510)
MARCH_NRAYS = (1, 7, 8, 9, 203)       # 8 = rays per workgroup; 203 = 25 workgroups and a ragged tail of 3
MARCH_G = (64, 24)                    # 24^3 = 432 words: a bit word spans z-columns
MARCH_GRIDS = ("block", "full", "border")
MARCH_AABB = np.array([[-1.25, -1.55, -1.05], [1.25, 0.95, 1.30]], F)   # not a cube; the origin lies inside the block
ONE_BELOW = np.nextafter(F(1), F(0))


@functools.lru_cache(maxsize=None)
def march_occupancy(G, kind):
    """bool [G, G, G]: 'block' = cells [0.3 G, 0.7 G)^3 plus 3 % random cells; 'full'; 'border' = exactly the cells with an
    index 0 or G - 1 (a point outside the box clamps to one of them, so a ray that misses the box still samples)"""
    occ = np.zeros((G, G, G), bool)
    if kind == "block":
        a, b = int(0.3 * G), int(0.7 * G)
        occ[a:b, a:b, a:b] = True
        occ |= np.random.default_rng(1000 + G).random((G, G, G)) < 0.03
    elif kind == "full":
        occ[:] = True
    else:
        assert kind == "border"
        occ[0], occ[-1], occ[:, 0], occ[:, -1], occ[:, :, 0], occ[:, :, -1] = True, True, True, True, True, True
    occ.setflags(write=False)
    return occ


def pack_occupancy(occ_bool):
    """the marcher's bit grid: bit (i & 31) of word (i >> 5) for cell i = (x G + y) G + z, and the 8 tail words behind it
    (flag 0 = border cells may be occupied: the training marcher does not read them)"""
    bits = np.packbits(np.ascontiguousarray(occ_bool).reshape(-1), bitorder="little")
    assert bits.size % 4 == 0
    return np.concatenate([bits.view(np.uint32), np.zeros(8, np.uint32)]).view(np.int32)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _norm32(o):
    o = np.asarray(o, F)
    return np.sqrt(((o[:, 0] * o[:, 0]).astype(F) + (o[:, 1] * o[:, 1]).astype(F) + (o[:, 2] * o[:, 2]).astype(F)).astype(F)).astype(F)


def march_ray_kinds(max_samples, n_rays):
    """the class of every ray of a set.  Seven classes are in every set of 7 rays and more; the two degenerate pairs
    (far == near / far < near, NaN near / NaN far) alternate with the parity of max_samples at 7 rays and are both there
    from 8 and 9 rays on."""
    even = max_samples % 2 == 0
    seven = ["block", "miss", "inner", "zero", "eq" if even else "lt", "nan_near" if even else "nan_far", "large"]
    if n_rays < 7:
        return ["block", "blockg", "inner", "miss", "zero", "large"][:n_rays]
    kinds = seven + ["lt" if even else "eq", "nan_far" if even else "nan_near", "zero0", "fmaedge"]
    fill = ["block", "blockg", "miss", "inner", "large", "blockg"]
    while len(kinds) < n_rays:
        kinds.append(fill[len(kinds) % len(fill)])
    return kinds[:n_rays]


def _fma_edge_ray(rng, max_samples, tries=512):
    """a ray from |o| = 60 whose step k = max_samples // 2 sits on the low-x face of the block of the 64^3 'block' grid, its
    direction moved by a few ulp until fl(t d + o) with one rounding and with two fall into cells of different occupancy
    (t d cancels against o: the unfused product is rounded at magnitude 60, 2e-6, the face is one float32 wide)"""
    occ, G = march_occupancy(64, "block"), 64
    mn, mx = MARCH_AABB.astype(np.float64)
    o = (60.0 * _unit(rng, tries)).astype(F)
    dist = _norm32(o)
    near, far = (dist - F(1)).astype(F), (dist + F(1)).astype(F)
    t = running_sum(near, step_size(near, far, max_samples), max_samples // 2 + 1)[:, -1:]
    P = mn + (mx - mn) * np.array([int(0.3 * G) / G, 0.5, 0.5])
    d0 = ((P - o.astype(np.float64)) / t.astype(np.float64)).astype(F)
    for j in range(-6, 7):
        d = d0.copy()
        d[:, 0] = (d0[:, 0].view(np.int32) + j).view(F)
        hit = np.nonzero(cell_occupied(t, o, d, occ, MARCH_AABB, True)[:, 0] != cell_occupied(t, o, d, occ, MARCH_AABB, False)[:, 0])[0]
        if hit.size:
            i = int(hit[0])
            return o[i], d[i], near[i], far[i]
    raise AssertionError("no fused / unfused cell difference found")


@functools.lru_cache(maxsize=None)
def march_rays(max_samples, n_rays):
    """One seeded ray set: o, d [n, 3], near, far [n], jitter [n, max_samples] (uniform draws; row 1 exact zeros, row 2 the
    largest float below 1) and the class of every ray:
      block     from outside at the occupied block, near / far = |o| -+ 1 (what training feeds)
      blockg    the same geometry with a general near / far that ends inside the block
      miss      never enters the box (|o| = 3, direction perpendicular to o)
      inner     |o| < 1: near < 0, the leading slots are masked
      zero      o = 0, near = -1, far = 1: at a power-of-two max_samples a step lands on t == 0 exactly
      zero0     near = 0 exactly, inside the block: step 0 is a t == 0 slot at every max_samples
      eq / lt   far == near, far < near: no step
      nan_near / nan_far   no step (origin and direction stay finite)
      large     |o| = 60 through the box
      fmaedge   |o| = 60, aimed so that step max_samples // 2 lands on a face of the block of the 64^3 'block' grid where the
                fused and the unfused cell position fall into cells of different occupancy (found by `_fma_edge_ray`)"""
    rng = np.random.default_rng(7919 * max_samples + n_rays)
    kinds = march_ray_kinds(max_samples, n_rays)
    n = n_rays
    o, d, near, far = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, F), np.zeros(n, F)
    mn, mx = MARCH_AABB.astype(np.float64)
    for i, k in enumerate(kinds):
        u, v = _unit(rng, 2)
        if k in ("block", "blockg", "eq", "lt", "nan_near", "nan_far"):
            o[i] = u * rng.uniform(1.8, 2.6)
            target = mn + (mx - mn) * rng.uniform(0.35, 0.65, 3)
            d[i] = (target - o[i]) / np.linalg.norm(target - o[i]) * rng.uniform(0.9, 1.1)
        elif k == "miss":
            o[i] = 3.0 * u
            w = np.cross(u, v)
            d[i] = w / np.linalg.norm(w)
        elif k == "inner":
            o[i], d[i] = u * rng.uniform(0.2, 0.9), v
        elif k == "zero":
            o[i], d[i] = 0.0, v
        elif k == "zero0":
            o[i], d[i] = 0.1 * u, v
        elif k == "fmaedge":
            continue
        else:
            assert k == "large"
            o[i] = 60.0 * u
            w = -u + 0.005 * v
            d[i] = w / np.linalg.norm(w)
    o, d = o.astype(F), d.astype(F)
    dist = _norm32(o)
    near[:], far[:] = dist - F(1), dist + F(1)
    for i, k in enumerate(kinds):
        if k == "fmaedge":
            o[i], d[i], near[i], far[i] = _fma_edge_ray(rng, max_samples)
        elif k == "blockg":
            t_hit = np.linalg.norm((mn + mx) / 2 - o[i].astype(np.float64)) / np.linalg.norm(d[i].astype(np.float64))
            far[i] = F(t_hit + rng.uniform(-0.15, 0.15))
            near[i] = far[i] - F(rng.uniform(1.2, 2.2))
        elif k == "zero":
            near[i], far[i] = -1.0, 1.0
        elif k == "zero0":
            near[i], far[i] = 0.0, 1.0
        elif k == "eq":
            near[i], far[i] = 1.5, 1.5
        elif k == "lt":
            near[i], far[i] = 2.0, 1.0
        elif k == "nan_near":
            near[i], far[i] = np.nan, 3.0
        elif k == "nan_far":
            near[i], far[i] = 1.0, np.nan
    # a positive step must move t everywhere on the ray, or the reference loop would not end
    dt = step_size(near, far, max_samples)
    with np.errstate(invalid="ignore"):
        live = near < far
    assert ((near[live] + dt[live]).astype(F) > near[live]).all() and ((far[live] + dt[live]).astype(F) > far[live]).all()
    jitter = rng.random((n, max_samples), dtype=F)
    if n > 1:
        jitter[1] = 0.0
    if n > 2:
        jitter[2] = ONE_BELOW
    assert jitter.max() < 1 and jitter.min() >= 0
    for a in (o, d, near, far, jitter):
        a.setflags(write=False)
    return dict(o=o, d=d, near=near, far=far, jitter=jitter, kinds=tuple(kinds), max_samples=max_samples, n_rays=n)


def march_cases(max_samples):
    """every (n_rays, G, grid, with_jitter) of one max_samples"""
    return [(n, G, g, j) for n in MARCH_NRAYS for G in MARCH_G for g in MARCH_GRIDS for j in (True, False)]


@functools.lru_cache(maxsize=None)
def march_reference(max_samples, n_rays, G, grid, with_jitter):
    """the reference of one input set, computed once and shared (read-only)"""
    r = march_rays(max_samples, n_rays)
    ref = march_train_compact_ref(r["o"], r["d"], r["near"], r["far"], march_occupancy(G, grid), MARCH_AABB, max_samples,
                                  r["jitter"] if with_jitter else None)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# =====================================================================================================================
# loss (instant_avatar/utils/loss.py:53-77 as csrc/ia_loss.hip evaluates it)
# =====================================================================================================================
LOSS_OFFSET = float(F(0.313262))      # the kernel's constant is a float32 literal
LOSS_SIZES = ((1, 0), (1, 1), (5, 7), (64, 64 * 256), (1000, 7000), (300, 128 * 1024 * 2 + 4), (300, 128 * 1024 * 2 + 5))
LOSS_WEIGHTS = ((1.0, 0.1, 0.1), (0.5, 0.0, 0.25))
LOSS_CAP = 1000
LOSS_POISON = (None, 0.0, 1.0)
LOSS_OVERFLOW = (None, LOSS_CAP - 1, LOSS_CAP, LOSS_CAP + 1)      # only the last poisons
LOSS_MUTANTS = ("inv_n", "no_offset", "de_sign", "over_ge", "dw_unpoisoned", "skip_tail")


@functools.lru_cache(maxsize=None)
def loss_inputs(N, M):
    """seeded inputs with the edges in them: weights rand^4 with exact 0 and 1, alpha exactly 0, 0.5 and 1, targets 0 and 1"""
    rng = np.random.default_rng(31 * N + M)
    rgb, tgt_rgb = rng.random((N, 3), dtype=F), rng.random((N, 3), dtype=F)
    tgt_rgb.reshape(-1)[0::5] = 0.0
    tgt_rgb.reshape(-1)[1::5] = 1.0
    alpha = rng.random(N, dtype=F)
    alpha[1::7], alpha[2::7], alpha[0::7] = 0.0, 1.0, 0.5
    tgt_alpha = (rng.random(N) > 0.5).astype(F)
    weight = rng.random(M, dtype=F) ** 4
    weight[3::11], weight[5::13] = 0.0, 1.0
    weight = weight.astype(F)
    for a in (rgb, tgt_rgb, alpha, tgt_alpha, weight):
        a.setflags(write=False)
    return dict(rgb=rgb, tgt_rgb=tgt_rgb, alpha=alpha, tgt_alpha=tgt_alpha, weight=weight)


def _ent64(v):
    a, b = np.exp(-v), np.exp(v - 1.0)
    return -np.log(a + b), (a - b) / (a + b)


def loss_poisoned(poison, overflow_count, overflow_cap):
    over = overflow_count is not None and int(overflow_count) > int(overflow_cap)
    return bool((poison is not None and float(poison) > 0) or over), over


def nerf_loss_ref(rgb, tgt_rgb, alpha, tgt_alpha, weight, w_rgb, w_alpha, w_reg, poison=None, overflow_count=None, overflow_cap=0,
                  out_pre=None):
    """float64.  out[0..4] = the caller's contents + {loss, mse, loss_alpha, reg_alpha + OFFSET, reg_density + OFFSET} (an
    empty weight array has reg_density 0); out[5] = 1 / 0 for *overflow_count > overflow_cap, the caller's content without a
    counter.  Poisoned (poison > 0 or the counter above the cap): out[0] and every gradient element NaN, out[1..4] as usual.
    Also returns the magnitudes the bounds use (`mag`) and the unpoisoned gradients (`clean`)."""
    f8 = lambda a: np.asarray(a, F).astype(np.float64)
    rgb, tgt_rgb, alpha, tgt_alpha, weight = f8(rgb).reshape(-1), f8(tgt_rgb).reshape(-1), f8(alpha), f8(tgt_alpha), f8(weight)
    w_rgb, w_alpha, w_reg = float(F(w_rgb)), float(F(w_alpha)), float(F(w_reg))
    N, M = len(alpha), len(weight)
    pre = np.zeros(6) if out_pre is None else np.asarray(out_pre, np.float64)
    d3, da = rgb - tgt_rgb, alpha - tgt_alpha
    ea, dea = _ent64(alpha)
    ew, dew = _ent64(weight)
    mse, la, ra = (d3 * d3).mean(), (da * da).mean(), ea.mean()
    rd = ew.mean() if M else 0.0
    loss = w_rgb * mse + w_alpha * la + w_reg * ra + w_reg * rd + 2.0 * w_reg * LOSS_OFFSET
    poisoned, over = loss_poisoned(poison, overflow_count, overflow_cap)
    out = pre + np.array([loss, mse, la, ra + LOSS_OFFSET, rd + LOSS_OFFSET, 0.0])
    out[5] = pre[5] if overflow_count is None else float(over)
    t1 = w_alpha * 2.0 * da / N
    clean = dict(d_rgb=w_rgb * 2.0 * d3 / (3.0 * N), d_alpha=t1 + w_reg * dea / N, d_weight=w_reg * dew / M if M else np.zeros(0))
    grads = {k: (np.full_like(v, np.nan) if poisoned else v) for k, v in clean.items()}
    if poisoned:
        out[0] = np.nan
    mag = dict(mse=np.abs(d3 * d3).mean(), la=np.abs(da * da).mean(), ra=np.abs(ea).mean(), rd=np.abs(ew).mean() if M else 0.0,
               t1=np.abs(t1), loss_clean=pre[0] + loss)
    return dict(out=out, poisoned=poisoned, clean=clean, mag=mag, N=N, M=M, w=(w_rgb, w_alpha, w_reg), pre=pre, **grads)


def loss_geometry(N, M, vec):
    """launch geometry of ia_nerf_loss and the longest per-thread chain of each sum: workgroups B = clamp(ceil(max(M, 3 N)
    / 1024), 1, 128) of 256 threads; a thread adds every (256 B)-th element to its partial."""
    B = int(min(128, max(1, (max(M, 3 * N) + 1023) // 1024)))
    T = 256 * B
    up = lambda a: -(-a // T)
    # the vector path adds (e0 + e1) + (e2 + e3) to the partial: two more levels per element
    return dict(B=B, T=T, L_rgb=up(3 * N), L_a=up(N), L_w=(up(M // 4) + 2) if vec else up(M))


# K of the gradients, per element (csrc/ia_loss.hip; -ffp-contract=off: one rounding per spelled operation).
#   d_rgb   = w_rgb * 2 * d * inv3n:  d = rgb - tgt (1), (w_rgb * 2) exact, * d (1), inv3n = 1 / (3 * N) (2), * inv3n (1)       = 5
#   de      = (a - b) / (a + b), a = expf(-v) (2 u), b = expf(v - 1) (argument 1 u |v - 1| <= u, expf 2 u: 3 u):
#             |err(a - b)| <= 2 u a + 3 u b + u |a - b|, a + b relative 3 u + u; with the division's own rounding
#             |err(de)| <= 3 u + (1 + 4 + 1) u |de| <= 9 u  AT MAGNITUDE 1 (|de| <= 1; the quotient cancels near v = 0.5)
#   d_weight = w_reg * de * invm:     de (9), two products (2), invm = 1 / M (1)                                            = 12, of w_reg / M
#   d_alpha  = t1 + t2, t1 = w_alpha * 2 * d * invn: d (1), two products (2), invn (1), the sum (1)                         = 5, of |t1|
#              t2 = w_reg * de * invn as d_weight (12), the sum (1)                                                         = 13, of w_reg / N
K_DRGB, K_DW, K_DA_T1, K_DA_T2 = 5, 12, 5, 13
# one more in each for the second-order terms ((1 + u)^K - 1 <= (K + 1) u for these K)
K_2ND = 1
# K of the values.  Every term of a sum passes through its thread's chain (L additions), the 6-step wave tree, the 4 wave
# partials, the product with the reciprocal count (whose own roundings are <= 2) -- L + 6 + 4 + 3 -- on top of its own
# roundings: (rgb - tgt)^2 and (alpha - tgt)^2 3 (the difference counts twice), the entropy 2 (logf at 1 ulp of |e|).  The
# entropy's ARGUMENT a + b is off by 4 u relative (above), which moves the logarithm by 4 u at magnitude 1, not |e|: A = 4 (+ 1
# second order).  Then one atomic per workgroup (and one for the additive constant) onto the caller's content: each add
# rounds at the magnitude of |content| + M (+ OFFSET).
K_TERM = dict(mse=3, la=3, ra=2, rd=2)
K_ARG = dict(mse=0, la=0, ra=5, rd=5)
K_TREE = 6 + 4 + 3
# out[0] = sum over the workgroups of w_rgb mse_b + w_alpha la_b + w_reg ra_b + w_reg rd_b (+ 2 w_reg OFFSET once): a term
# passes through one product and at most four additions (5), then the atomics.
K_TOTAL = 5


def nerf_loss_bounds(ref, vec):
    """dict of bounds (float64 arrays of the outputs' shapes) for one call: see the counts above"""
    N, M, mag = ref["N"], ref["M"], ref["mag"]
    w_rgb, w_alpha, w_reg = (abs(w) for w in ref["w"])
    g = loss_geometry(N, M, vec)
    B, pre = g["B"], np.abs(ref["pre"])
    b = dict(d_rgb=(K_DRGB + K_2ND) * U * np.abs(ref["clean"]["d_rgb"]),
             d_alpha=U * ((K_DA_T1 + K_2ND) * mag["t1"] + (K_DA_T2 + K_2ND) * w_reg / N),
             d_weight=np.full(M, (K_DW + K_2ND) * U * w_reg / max(M, 1)))
    inner, out = {}, np.zeros(6)
    for i, (k, L, off, adds) in enumerate((("mse", g["L_rgb"], 0.0, B), ("la", g["L_a"], 0.0, B), ("ra", g["L_a"], LOSS_OFFSET, B + 1),
                                           ("rd", g["L_w"], LOSS_OFFSET, B + 1))):
        inner[k] = U * ((K_TERM[k] + L + K_TREE) * mag[k] + K_ARG[k] * (1.0 if (k != "rd" or M) else 0.0))
        out[1 + i] = inner[k] + U * adds * (pre[1 + i] + mag[k] + off)
    m0 = w_rgb * mag["mse"] + w_alpha * mag["la"] + w_reg * (mag["ra"] + mag["rd"]) + 2 * w_reg * LOSS_OFFSET
    out[0] = w_rgb * inner["mse"] + w_alpha * inner["la"] + w_reg * (inner["ra"] + inner["rd"]) + U * (K_TOTAL + B) * (pre[0] + m0)
    b["out"] = out           # out[5] has bound 0: exact
    return b


def _exp32(x):
    return np.exp(np.asarray(x, F).astype(np.float64)).astype(F)      # a correctly rounded float32 expf


def _ent32(v, sign=1.0):
    a, b = _exp32(-v), _exp32((v - F(1)).astype(F))
    s = (a + b).astype(F)
    return (-np.log(s.astype(np.float64))).astype(F), (F(sign) * ((a - b).astype(F) / s)).astype(F)


def _thread_partials(terms, T):
    """partial of thread tid = terms[tid] + terms[tid + T] + ... in float32, sequentially"""
    L = max(1, -(-len(terms) // T))
    a = np.zeros(L * T, F)
    a[:len(terms)] = terms
    s = np.zeros(T, F)
    for row in a.reshape(L, T):
        s = (s + row).astype(F)
    return s


def _workgroup_sums(s):
    """[B] float32: the xor-butterfly over the 64 lanes of each wave, then ((0 + w0) + w1) + w2) + w3"""
    v = s.reshape(-1, 4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, lane ^ o]).astype(F)
    p = np.zeros(v.shape[0], F)
    for w in range(4):
        p = (p + v[:, w, 0]).astype(F)
    return p


def nerf_loss_fp32(rgb, tgt_rgb, alpha, tgt_alpha, weight, w_rgb, w_alpha, w_reg, poison=None, overflow_count=None, overflow_cap=0,
                   out_pre=None, vec=None, mutant=None):
    """k_nerf_loss in plain float32 on the host, in the kernel's order (launch geometry, chains, wave tree, wave partials, one
    atomic per workgroup in index order); exp and log correctly rounded.  vec: the 16-byte path (default: M % 4 == 0).
    Returns out [6] and the three gradients (float32).  mutant: one of LOSS_MUTANTS."""
    assert mutant is None or mutant in LOSS_MUTANTS
    rgb, tgt_rgb = np.asarray(rgb, F).reshape(-1), np.asarray(tgt_rgb, F).reshape(-1)
    alpha, tgt_alpha, weight = np.asarray(alpha, F), np.asarray(tgt_alpha, F), np.asarray(weight, F)
    w_rgb, w_alpha, w_reg = F(w_rgb), F(w_alpha), F(w_reg)
    N, M = len(alpha), len(weight)
    vec = (M % 4 == 0) if vec is None else vec
    assert not vec or M % 4 == 0
    g = loss_geometry(N, M, vec)
    over = overflow_count is not None and (overflow_count >= overflow_cap if mutant == "over_ge" else overflow_count > overflow_cap)
    pz = F(np.nan) if ((poison is not None and poison > 0) or over) else F(1)
    out = np.zeros(6, F) if out_pre is None else np.asarray(out_pre, F).copy()
    if overflow_count is not None:
        out[5] = 1.0 if over else 0.0
    invn = F(F(1) / F(N))
    inv3n = invn if mutant == "inv_n" else F(F(1) / F(F(3) * F(N)))
    invm = F(F(1) / F(M)) if M else F(0)
    sign = -1.0 if mutant == "de_sign" else 1.0
    with np.errstate(invalid="ignore"):
        d3 = (rgb - tgt_rgb).astype(F)
        d_rgb = ((((w_rgb * F(2)) * d3).astype(F) * inv3n).astype(F) * pz).astype(F)
        da = (alpha - tgt_alpha).astype(F)
        ea, dea = _ent32(alpha, sign)
        t1 = (((w_alpha * F(2)) * da).astype(F) * invn).astype(F)
        t2 = ((w_reg * dea).astype(F) * invn).astype(F)
        d_alpha = ((t1 + t2).astype(F) * pz).astype(F)
        Mw = (M // 4) * 4 if mutant == "skip_tail" else M
        ew, dew = _ent32(weight[:Mw], sign)
        d_weight = np.zeros(M, F)
        d_weight[:Mw] = (((w_reg * dew).astype(F) * invm).astype(F) * (F(1) if mutant == "dw_unpoisoned" else pz)).astype(F)
    if vec or mutant == "skip_tail":
        q = ew.reshape(-1, 4)
        ew_terms = ((q[:, 0] + q[:, 1]).astype(F) + (q[:, 2] + q[:, 3]).astype(F)).astype(F)
    else:
        ew_terms = ew
    T = g["T"]
    p = [_workgroup_sums(_thread_partials(t, T)) for t in ((d3 * d3).astype(F), (da * da).astype(F), ea, ew_terms)]
    mse, la, ra, rd = (p[0] * inv3n).astype(F), (p[1] * invn).astype(F), (p[2] * invn).astype(F), (p[3] * invm).astype(F)
    total = ((((w_rgb * mse).astype(F) + (w_alpha * la).astype(F)).astype(F) + (w_reg * ra).astype(F)).astype(F) + (w_reg * rd).astype(F)).astype(F)
    off = F(0) if mutant == "no_offset" else F(LOSS_OFFSET)
    with np.errstate(invalid="ignore"):
        for b in range(g["B"]):
            tb = total[b]
            if b == 0:
                tb = F(tb + F((F(2) * w_reg) * off))
                out[3], out[4] = F(out[3] + off), F(out[4] + off)
            out[0] = F(out[0] + F(tb * pz))
            out[1], out[2], out[3], out[4] = F(out[1] + mse[b]), F(out[2] + la[b]), F(out[3] + ra[b]), F(out[4] + rd[b])
    return dict(out=out, d_rgb=d_rgb, d_alpha=d_alpha, d_weight=d_weight)


LOSS_PRE = (2.5, -1.25, 0.5, 4.0, -3.0, 7.0)


def loss_calls():
    """every call the GPU test makes: (N, M, weights, poison, overflow_count, out_pre, vec).  All sizes x the poison / overflow
    matrix (the weight triple alternating), two vector-sized weight arrays given off 16-byte alignment (scalar path), and two
    calls that accumulate onto non-zero contents (one of them without a counter: out[5] keeps its 7)."""
    calls = []
    for i, (N, M) in enumerate(LOSS_SIZES):
        for j, (p, c) in enumerate(loss_matrix()):
            calls.append((N, M, LOSS_WEIGHTS[(i + j) % 2], p, c, None, M % 4 == 0))
    calls.append((64, 64 * 256, LOSS_WEIGHTS[0], None, None, None, False))
    calls.append((300, 128 * 1024 * 2 + 4, LOSS_WEIGHTS[0], None, None, None, False))
    calls.append((1000, 7000, LOSS_WEIGHTS[0], 0.0, LOSS_CAP, LOSS_PRE, True))
    calls.append((5, 7, LOSS_WEIGHTS[1], None, None, LOSS_PRE, False))
    return calls


def loss_matrix():
    """(poison, overflow_count) of the poison / overflow matrix, the capacity being LOSS_CAP"""
    return [(p, c) for p in LOSS_POISON for c in LOSS_OVERFLOW]


# =====================================================================================================================
# ray set-up (snarf_deformer.py:95-103) and frame statistics
# =====================================================================================================================
RAYS_R = (1, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def transform_inputs(R):
    """a general rigid w2s with translation; every fourth origin lands within one unit of the root (near < 0)"""
    rng = np.random.default_rng(500 + R)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = rng.uniform(-1.5, 1.5, 3)
    w2s = np.eye(4)
    w2s[:3, :3], w2s[:3, 3] = q, t
    d = _unit(rng, R) * rng.uniform(0.8, 1.2, (R, 1))
    target = _unit(rng, R) * rng.uniform(1.5, 4.0, (R, 1))
    target[0::4] = _unit(rng, len(target[0::4])) * rng.uniform(0.05, 0.95, (len(target[0::4]), 1))
    o = (target - t) @ q          # w2s o = target
    out = dict(o=o.astype(F), d=d.astype(F), w2s=w2s.astype(F))
    for a in out.values():
        a.setflags(write=False)
    return out


# k_transform_rays, per element, no contraction:
#   o'[a] = ox w0 + oy w1 + oz w2 + w3: a term passes through its product and at most 3 additions: K = 4, M = sum |terms|
#   d'[a] = dx w0 + dy w1 + dz w2:      K = 3
#   dist  = sqrtf(o'0^2 + o'1^2 + o'2^2) from the ROUNDED o': |err| <= sum_a err(o'[a]) (the norm is 1-Lipschitz), plus the
#           squares and two additions (3 u on the sum, halved by the root: 1.5 u) and sqrtf at 1 ulp (2 u): 4 u dist
#   near / far = dist -+ 1: one more rounding at |dist| + 1
K_TO, K_TD, K_DIST = 4, 3, 4


def transform_rays_w2s_ref(o, d, w2s):
    """float64 o', d', near, far and their bounds"""
    o, d, w = np.asarray(o, F).astype(np.float64), np.asarray(d, F).astype(np.float64), np.asarray(w2s, F).astype(np.float64)
    o2, d2 = o @ w[:3, :3].T + w[:3, 3], d @ w[:3, :3].T
    m_o, m_d = np.abs(o) @ np.abs(w[:3, :3]).T + np.abs(w[:3, 3]), np.abs(d) @ np.abs(w[:3, :3]).T
    dist = np.sqrt((o2 * o2).sum(1))
    b_o, b_d = K_TO * U * m_o, K_TD * U * m_d
    b_n = b_o.sum(1) + K_DIST * U * dist + U * (dist + 1.0)
    ref = dict(o=o2, d=d2, near=dist - 1.0, far=dist + 1.0)
    return ref, dict(o=b_o, d=b_d, near=b_n, far=b_n)


def transform_rays_w2s_fp32(o, d, w2s):
    o, d, w = np.asarray(o, F), np.asarray(d, F), np.asarray(w2s, F)
    o2, d2 = np.zeros_like(o), np.zeros_like(d)
    for a in range(3):
        s = ((o[:, 0] * w[a, 0]).astype(F) + (o[:, 1] * w[a, 1]).astype(F)).astype(F)
        o2[:, a] = ((s + (o[:, 2] * w[a, 2]).astype(F)).astype(F) + w[a, 3]).astype(F)
        s = ((d[:, 0] * w[a, 0]).astype(F) + (d[:, 1] * w[a, 1]).astype(F)).astype(F)
        d2[:, a] = (s + (d[:, 2] * w[a, 2]).astype(F)).astype(F)
    dist = _norm32(o2)
    return dict(o=o2, d=d2, near=(dist - F(1)).astype(F), far=(dist + F(1)).astype(F))


STATS_R = (1, 2047, 2048, 2049, 128 * 2048 + 5)      # workgroup-count boundaries, and past the 128-workgroup cap
STATS_PRE = (F(3.25), F(-0.75))


@functools.lru_cache(maxsize=None)
def stats_inputs(R):
    """counter: non-integer values (the sums round); alpha with exact 0.5 (not counted) and NaN (not counted)"""
    rng = np.random.default_rng(900 + R)
    counter = (rng.random(R, dtype=F) * F(256)).astype(F)
    alpha = rng.random(R, dtype=F)
    alpha[0::5] = 0.5
    alpha[3::17] = np.nan
    alpha[4::19] = np.nextafter(F(0.5), F(1))
    counter.setflags(write=False)
    alpha.setflags(write=False)
    return dict(counter=counter, alpha=alpha)


def stats_geometry(R):
    B = int(min(128, -(-R // 2048)))
    return dict(B=B, T=256 * B, L=-(-R // (256 * B)))


# k_frame_stats: acc[k] += sum over the workgroups of (s0 + s1 + s2 + s3) / R.  A term passes through its thread's chain (L),
# the wave tree (6), the three additions of the wave partials and the division: K = L + 6 + 3 + 1; then B atomics at the
# magnitude |content| + M.  The coverage terms are 0 / 1: their sums are exact integers, the same K covers the division.
def frame_stats_ref(counter, alpha, acc_pre):
    counter, a32 = np.asarray(counter, F).astype(np.float64), np.asarray(alpha, F)
    R = len(counter)
    with np.errstate(invalid="ignore"):
        hit = (a32 > F(0.5)).astype(np.float64)
    pre = np.asarray(acc_pre, F).astype(np.float64)
    g = stats_geometry(R)
    ref = pre + np.array([counter.sum() / R, hit.sum() / R])
    mag = np.array([np.abs(counter).sum() / R, hit.sum() / R])
    bound = U * ((g["L"] + 6 + 3 + 1) * mag + g["B"] * (np.abs(pre) + mag))
    return ref, bound


def frame_stats_fp32(counter, alpha, acc_pre):
    counter, alpha = np.asarray(counter, F), np.asarray(alpha, F)
    R = len(counter)
    g = stats_geometry(R)
    with np.errstate(invalid="ignore"):
        hit = (alpha > F(0.5)).astype(F)
    acc = np.asarray(acc_pre, F).copy()
    for k, terms in enumerate((counter, hit)):
        v = _thread_partials(terms, g["T"]).reshape(-1, 4, 64)
        lane = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):
            v = (v + v[:, :, lane ^ o]).astype(F)
        w = v[:, :, 0]
        s = (((w[:, 0] + w[:, 1]).astype(F) + w[:, 2]).astype(F) + w[:, 3]).astype(F)
        for b in range(g["B"]):
            acc[k] = F(acc[k] + F(s[b] / F(R)))
    return acc
