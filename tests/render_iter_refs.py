"""References, seeded input sets, kernel emulations and mutants for ONE iteration of the inference wave-front loop
(`ia_render_test`): `ia_render_init_rays`, `ia_render_march_compact`, `ia_render_composite_compact`, `ia_render_finalize`
(csrc/ia_render.hip).  numpy only: no GPU, no product import.  Builds on tests/train_step_refs.py (`fma32`, `running_sum`,
`cell_occupied`, `march_occupancy`, `pack_occupancy`, the ray kinds of `march_rays`).

MARCHER, bit for bit.  The reference is the plain loop of raymarcher.cu:44-69,
    while (t < far && cnt < N) { if (occupied(t)) cnt++; t += dt; }
in float32, one rounding per spelled operation, the position by one FMA -- no skip, no unrolling (`march_iter_ref`).  The
library is built with -ffp-contract=off and nothing on the path is a transcendental, so per-ray counts, depths, positions,
`near_w` after the call, `counter`, and the record fields are pinned exactly.  A ray without a positive step (far <= near, a NaN
bound, step 0) takes no sample and keeps its near: the reference loop would not end on it, the kernel says so at its `dt > 0`.
`march_iter_emulated` restates the KERNEL's algorithm (slab interval in grid coordinates, margins, skip before and behind the
box, four steps per trip, LDS staging decided per workgroup, one range per wave) and carries one-line mutants of it.

COMPOSITOR, float64 with bounds |got - ref| <= sum K u M (`composite_ref`; the counts are next to it), the same decisions as the
kernel: skip when alpha < thresh, stop when T <= 1e-4, the candidate maximum as cand_max(fill = 0, nan_to_num), survival
T > 1e-4 && cnt == N_steps && s_t[last] > 0.  A ray whose float64 alpha or T comes within its bound of a threshold is undecidable
and left out of the value comparison (at most 2 % of a set, asserted on the reference alone).  `composite_emulated` is the
kernel's loop (four samples per trip) in plain float32 with a correctly rounded exp, and carries mutants.

__expf.  composite_step calls __expf, not expf.  No HIP documentation is installed with this ROCm (only headers), so the
figure is derived from the lowering: clang's __clang_hip_math.h defines
    float __expf(float x) { const float log2_e = 0x1.715476p+0; return __builtin_amdgcn_exp2f(log2_e * x); }
and the gfx950 code of ia_render.hip holds exactly that in k_composite_compact and k_composite_test: v_mul_f32 of sg * dl by
0xbfb8aa3b (-log2 e: the negation of -sg * dl folded into the constant, which is exact) feeding v_exp_f32.  x = fl(-sigma dt) carries u |x|; fl32(log2 e) is off by 0.23 u relative and the product rounds once (u): the
exponent is off by <= 2.23 u |x| relative to x log2 e, i.e. e^x by a FACTOR e^(2.23 u |x|); v_exp_f32 is specified at 1 ulp
(AMD "CDNA3 / CDNA4 Instruction Set Architecture", V_EXP_F32: "base 2 exponent, 1 ULP accuracy, denormals are flushed") = 2 u
relative.  Together TAU_REL(x) = u (3 |x| + 2) + second order (`K_TAU_X`, `K_TAU`); a flushed denormal result (tau < 2^-126) is an
absolute 2^-126, below everything compared here.  Nothing in a bound comes from a kernel's output.
"""
import functools

import numpy as np

import train_step_refs as tr
from train_step_refs import F, U, MARCH_AABB, cell_occupied, fma32, march_occupancy, pack_occupancy, running_sum

SENT_F = tr.SENT_F
SENT_I = np.int32(-12345)
STATE_FIELDS = ("n_alive", "n_samples", "n_cand", "k_before", "iters", "n_step", "n_eff", "pad")      # eight int32 per record
WG, WAVE = 256, 64
THRESH = float(F(0.01))         # the kernel compares float alpha with the float literal 0.01f
T_STOP = 1e-4                   # and (double)T with the double literal 1e-4
INF = F(np.inf)
STATE1_PRE = (0, 0, 0, -1, -1, 55, 66, 77)      # what the tests put into the NEXT record before the march: it writes [3] and [4] only


def schedule(n_alive, k_before, max_samples, max_batch):
    """(n_eff, N_step) of render_schedule: the loop condition `k < MAX_SAMPLES` and max(min(MAX_BATCH // n_alive, MAX_SAMPLES), 1)"""
    na = int(n_alive) if k_before < max_samples else 0
    ns = max(min(max_batch // na, max_samples), 1) if na > 0 else 0
    return na, ns


# =====================================================================================================================
# occupancy grids and their tail words
# =====================================================================================================================
GRIDS = ("empty", "full", "block", "cell", "corners2", "face", "blobs", "slab_x", "slab_y", "slab_z", "rand3")
INTERIOR_GRIDS = ("block", "cell", "corners2", "blobs", "slab_x", "slab_y", "slab_z")      # flag 1: the exact skip is on


@functools.lru_cache(maxsize=None)
def iter_occupancy(G, kind):
    occ = np.zeros((G, G, G), bool)
    a, b, m = int(0.3 * G), int(0.7 * G), G // 2
    if kind == "full":
        occ[:] = True
    elif kind == "block":
        occ[a:b, a:b, a:b] = True
    elif kind == "cell":
        occ[m, m - 1, m + 1] = True
    elif kind == "corners2":
        occ[1, 1, 1] = occ[G - 2, G - 2, G - 2] = True
    elif kind == "face":                     # touches the x = 0 border: flag 0
        occ[0:b, a:b, a:b] = True
    elif kind == "blobs":                    # empty space inside the common bounds
        q = max(G // 8, 1)
        occ[a:a + q, a:a + q, a:a + q] = True
        occ[b - q:b, b - q:b, b - q:b] = True
    elif kind.startswith("slab_"):           # one cell thick, interior
        ax = "xyz".index(kind[-1])
        sl = [slice(1, G - 1)] * 3
        sl[ax] = slice(m, m + 1)
        occ[tuple(sl)] = True
    elif kind == "rand3":                    # the parity test's random 3 % (border cells included: flag 0)
        occ |= np.random.default_rng(1000 + G).random((G, G, G)) < 0.03
    else:
        assert kind == "empty"
    occ.setflags(write=False)
    return occ


def tail_words(occ_bool):
    """the seven tail words behind the bit grid: flag = 1 iff no border cell is occupied, then x_min, x_max, y_min, y_max, z_min,
    z_max of the occupied cells (0x7fffffff, -1 when nothing is occupied), as uint32"""
    occ = np.asarray(occ_bool, bool)
    border = occ[0].any() or occ[-1].any() or occ[:, 0].any() or occ[:, -1].any() or occ[:, :, 0].any() or occ[:, :, -1].any()
    w = [0 if border else 1]
    idx = np.nonzero(occ)
    for a in range(3):
        w += [int(idx[a].min()), int(idx[a].max())] if idx[a].size else [0x7fffffff, -1]
    return np.array(w, np.int64).astype(np.uint32)


def pack_with_tail(occ_bool, flag=None):
    """int32 words of the bit grid + 8 tail words (the eighth is spare); `flag` overrides the border flag"""
    words = pack_occupancy(occ_bool).copy()
    t = tail_words(occ_bool)
    if flag is not None:
        t[0] = flag
    words[-8:-1] = t.view(np.int32)
    return words


# =====================================================================================================================
# rays
# =====================================================================================================================
def _world(G, g):
    """world coordinates of the grid coordinates g [..., 3]"""
    mn, mx = MARCH_AABB.astype(np.float64)
    return mn + np.asarray(g, np.float64) * (mx - mn) / G


def _cells_per_unit(G):
    mn, mx = MARCH_AABB.astype(np.float64)
    return G / (mx - mn)


def _box(G, grid):
    """(lo, hi) of the occupied cells in grid coordinates ([min, max + 1]); the block's for an empty grid"""
    t = tail_words(iter_occupancy(G, grid if grid != "empty" else "block")).view(np.int32)
    return np.array([t[1], t[3], t[5]], np.float64), np.array([t[2], t[4], t[6]], np.float64) + 1.0


EXTRA_KINDS = ("ax+in", "ax-in", "ax+out", "ay+in", "ay-out", "az-in", "az+out", "c13in", "c11out", "bstr_lo_in", "bstr_hi_in", "bstr_lo_out",
               "bstr_hi_out", "inside", "inside_negnear", "behind", "negnear", "dt0", "far60", "far1000",
               "face-0.02", "face+0.02", "face-0.1", "face+0.1", "edge-0.02", "edge+0.02", "edge-0.1", "edge+0.1",
               "corner-0.02", "corner+0.02", "corner-0.1", "corner+0.1")


def _extra_ray(kind, G, grid, rng):
    """(o, d, near, far) in float64 for one of EXTRA_KINDS, placed against the occupied box of the grid"""
    lo, hi = _box(G, grid)
    mid = (lo + hi) / 2
    cpu = _cells_per_unit(G)
    if kind[0] == "a" and kind[1] in "xyz":              # exactly axis-parallel, inside / outside the box in the other axes
        ax, sign, where = "xyz".index(kind[1]), (1.0 if kind[2] == "+" else -1.0), kind[3:]
        p = mid.copy()
        if where == "out":
            p[(ax + 1) % 3] = hi[(ax + 1) % 3] + 3.0
        d = np.zeros(3)
        d[ax] = sign
        return _world(G, p) - 2.0 * d, d, 0.25, 4.0
    if kind in ("c13in", "c11out") or kind.startswith("bstr"):       # x-marching with a tiny y component
        p = mid.copy()
        if kind.endswith("out"):
            p[1] = lo[1] - 2.5
        dy = {"c13in": 1e-13, "c11out": 1e-11}.get(kind)
        if dy is None:                                    # B_y = d_y s_y just below / above the kernel's 1e-12
            dy = (0.9e-12 if "_lo_" in kind else 1.1e-12) / cpu[1]
        return _world(G, p) - np.array([2.0, 0, 0]), np.array([1.0, dy, 0.0]), 0.5, 3.5
    u = rng.standard_normal(3)
    u /= np.linalg.norm(u)
    if kind in ("inside", "inside_negnear"):
        return _world(G, mid + (hi - lo) * rng.uniform(-0.3, 0.3, 3)), u, (-0.7 if kind == "inside_negnear" else 0.0), 2.0
    if kind in ("behind", "negnear", "dt0"):
        o = _world(G, mid) - 2.2 * u
        if kind == "behind":                              # near already past the box
            ext = np.linalg.norm((hi - lo) / cpu)
            return o, u, 2.2 + ext + 0.3, 2.2 + ext + 1.3
        return o, u, (-0.5 if kind == "negnear" else 1.0), 3.5
    if kind in ("far60", "far1000"):
        dist = 60.0 if kind == "far60" else 1000.0
        o = _world(G, mid + (hi - lo) * rng.uniform(-0.4, 0.4, 3)) - dist * u
        return o, u, dist - 1.0, dist + 1.0
    what, off = kind[:-5] if kind[-5] in "+-" else kind[:-4], float(kind[-5:] if kind[-5] in "+-" else kind[-4:])
    # aimed at a face / an edge / a corner of the box, `off` cells inside (+) or outside (-) it, travelling along the feature
    p = mid.copy()
    n_ax = {"face": 1, "edge": 2, "corner": 3}[what]
    p[:n_ax] = lo[:n_ax] + off
    d = np.array([0.0, 0.0, 1.0]) if what == "edge" else (np.array([0.0, 0.6, 0.8]) if what == "face" else np.array([1.0, -1.0, 0.0]) / np.sqrt(2))
    if what == "corner":
        d = np.array([1.0, -1.0, 0.0]) / np.sqrt(2) * 0.999 + np.array([0, 0, 0.04])
    return _world(G, p) - 1.7 * d, d, 0.2, 3.4


@functools.lru_cache(maxsize=None)
def iter_rays(max_samples, R, G, grid):
    """One seeded ray set of R rays: the kinds of train_step_refs.march_rays (through, miss, inner, far < near, far == near, NaN
    bound, |o| = 60, fmaedge), then EXTRA_KINDS placed against the occupied box of (G, grid), cycled until R rays are there; from
    the second cycle on the random kinds draw new directions.  step = fl((far - near) / max_samples) as k_render_init_rays
    computes it, except the 'dt0' rays (step 0 with near < far).  Returns o, d [R, 3], near, far, step [R], kinds."""
    rng = np.random.default_rng(104729 * max_samples + 31 * R + G + 7 * GRIDS.index(grid))
    n_base = min(R, 11)
    base = tr.march_rays(max_samples, n_base)
    o, d = np.zeros((R, 3), F), np.zeros((R, 3), F)
    near, far = np.zeros(R, F), np.zeros(R, F)
    o[:n_base], d[:n_base], near[:n_base], far[:n_base] = base["o"], base["d"], base["near"], base["far"]
    kinds = list(base["kinds"])
    for i in range(n_base, R):
        k = EXTRA_KINDS[(i - n_base) % len(EXTRA_KINDS)]
        oo, dd, nn, ff = _extra_ray(k, G, grid, rng)
        o[i], d[i], near[i], far[i] = oo, dd, nn, ff
        kinds.append(k)
    step = tr.step_size(near, far, max_samples)
    for i, k in enumerate(kinds):
        if k == "dt0":
            step[i] = 0.0
    with np.errstate(invalid="ignore"):
        live = step > 0
    # a positive step must move t everywhere on the ray, or no loop ends
    assert ((near[live] + step[live]).astype(F) > near[live]).all() and ((far[live] + step[live]).astype(F) > far[live]).all()
    out = dict(o=o, d=d, near=near, far=far, step=step)
    for a in out.values():
        a.setflags(write=False)
    out["kinds"] = tuple(kinds)
    return out


# (name, n_alive, R, max_samples, max_batch, k_before) -> N_step
CASES = (("n1", 1, 8, 64, 1, 0),                 # 1
         ("n2", 3, 40, 64, 6, 0),                # 2
         ("n3", 63, 80, 64, 63 * 3 + 5, 3),      # 3
         ("n4", 64, 64, 64, 64 * 4, 0),          # 4
         ("n5", 65, 130, 64, 65 * 5 + 64, 0),    # 5
         ("n7", 200, 256, 128, 200 * 7 + 199, 10),   # 7
         ("n8", 257, 300, 128, 257 * 8, 0),      # 8
         ("n9", 513, 600, 128, 513 * 9 + 1, 0),  # 9
         ("nms", 65, 130, 6, 100000, 0),         # max_samples
         ("small_batch", 200, 256, 64, 150, 0),  # max_batch < n_alive: 1
         ("done", 65, 130, 64, 1000, 64))        # k_before >= max_samples: nothing is processed, nothing is written
CASE_NSTEP = dict(n1=1, n2=2, n3=3, n4=4, n5=5, n7=7, n8=8, n9=9, nms=6, small_batch=1, done=0)
GS = (64, 32, 16)


def case_by_name(name):
    return next(c for c in CASES if c[0] == name)


@functools.lru_cache(maxsize=None)
def iter_inputs(case, G, grid):
    """the input set of one (case, G, grid): rays, the shuffled alive subset (R slots, the first n_alive are alive; the rest hold
    other rays, which the kernels must not touch), the state record and the table of steps shared by reference and emulation"""
    name, n_alive, R, ms, mb, kb = case_by_name(case)
    r = iter_rays(ms, R, G, grid)
    rng = np.random.default_rng(17 * R + n_alive)
    alive = rng.permutation(R).astype(np.int32)
    at = int(np.nonzero(alive == 0)[0][0])
    alive[[0, at]] = alive[at], alive[0]     # ray 0 (a 'block' ray: it has samples) is alive at every n_alive
    counter0 = rng.integers(0, 50, R).astype(F)
    occ = iter_occupancy(G, grid)
    alive.setflags(write=False)
    counter0.setflags(write=False)
    return dict(r, occ=occ, G=G, grid=grid, alive=alive, n_alive=n_alive, R=R, max_samples=ms, max_batch=mb, k_before=kb, counter0=counter0,
                iters0=3, case=name)


# =====================================================================================================================
# the table of steps: t_k and the occupancy of step k for every alive ray
# =====================================================================================================================
def step_table(inp):
    """For the n_eff processed rays (alive order): T [n, K] the running sum from near_w (`inp['near_w']`, default near), L [n] the number of steps with t < far
    (prefix), OCC [n, K] the occupancy of step k (False from L on, and on a ray without a positive step).  K covers L + 1."""
    na, ns = schedule(inp["n_alive"], inp["k_before"], inp["max_samples"], inp["max_batch"])
    ray = inp["alive"][:na].astype(np.int64)
    near = np.asarray(inp.get("near_w", inp["near"]), F)[ray]
    far, dt, o, d = inp["far"][ray], inp["step"][ray], inp["o"][ray], inp["d"][ray]
    K = 8
    while True:
        T = running_sum(near, dt, K)
        with np.errstate(invalid="ignore"):
            ok = np.logical_and.accumulate(T < far[:, None], axis=1) & (dt > 0)[:, None]
        if na == 0 or not ok[:, -1].any():
            break
        K *= 2
        assert K <= 8192, "a ray does not reach far"
    L = ok.sum(1)
    OCC = np.zeros((na, K), bool)
    if na:
        OCC = cell_occupied(T, o, d, inp["occ"], MARCH_AABB) & ok
    return dict(ray=ray, T=T, L=L, OCC=OCC, near=near, far=far, dt=dt, o=o, d=d, n_eff=na, n_step=ns, K=K)


def _points(T_hit, o, d):
    return np.stack([fma32(T_hit, d[:, a], o[:, a]) for a in range(3)], axis=-1)


def _finish_march(inp, tab, cnt, first, t_end, occ_eff, order="index"):
    """the outputs of the march from per-ray counts, the step index the second pass starts at and the final t: the first `cnt`
    occupied steps from `first` on (second pass), compact ranges wave by wave"""
    na, ns, R = tab["n_eff"], tab["n_step"], inp["R"]
    total = int(cnt.sum())
    ray_off, ray_cnt = np.full(R, SENT_I, np.int32), np.full(R, SENT_I, np.int32)
    near_w, counter = np.array(inp.get("near_w", inp["near"]), F), np.array(inp["counter0"], F)
    s_t, s_pts = np.zeros(total, F), np.zeros((total, 3), F)
    off = np.cumsum(cnt) - cnt
    if na:
        ray_off[:na], ray_cnt[:na] = off, cnt
        near_w[tab["ray"]] = t_end
        counter[tab["ray"]] = (counter[tab["ray"]] + cnt.astype(F)).astype(F)
        K = tab["K"]
        k = np.arange(K)[None, :]
        m = occ_eff & (k >= first[:, None])
        rank = np.cumsum(m, 1) - m
        m &= rank < cnt[:, None]
        assert (m.sum(1) == cnt).all(), "second pass finds fewer steps than the first counted"
        rr, kk = np.nonzero(m)
        s_t[:] = tab["T"][rr, kk]
        s_pts[:] = _points(s_t, tab["o"][rr], tab["d"][rr])
    state = np.array([[0] * 8, STATE1_PRE], np.int32)
    state[0] = [inp["n_alive"], total, 0, inp["k_before"], inp["iters0"], ns, na, 0]
    state[1, 3], state[1, 4] = inp["k_before"] + ns, inp["iters0"] + (1 if na > 0 else 0)
    return dict(ray_off=ray_off, ray_cnt=ray_cnt, s_t=s_t, s_pts=s_pts, near_w=near_w, counter=counter, state=state, n_samples=total,
                n_eff=na, n_step=ns, ray_start=off)


def march_iter_ref(inp, tab=None):
    """What ia_render_march_compact must write (samples in alive order; `march_iter_compare` allows the waves' permutation)."""
    tab = step_table(inp) if tab is None else tab
    na, N = tab["n_eff"], tab["n_step"]
    hits = np.cumsum(tab["OCC"], 1)
    total_hits = hits[:, -1] if na else np.zeros(0, np.int64)
    cnt = np.minimum(total_hits, N)
    # the step behind the N-th hit when the cap ended the loop, step L (the first t not below far) otherwise
    full = total_hits >= N
    k_last = np.argmax(hits >= N, axis=1) if na else np.zeros(0, np.int64)
    end = np.where(full, k_last + 1, tab["L"])
    t_end = tab["T"][np.arange(na), np.minimum(end, tab["K"] - 1)]
    assert (end < tab["K"]).all()
    return _finish_march(inp, tab, cnt, np.zeros(na, np.int64), t_end, tab["OCC"])


MARCH_MUTANTS = ("margin0", "no_swap", "parallel_outside", "stage_lt", "skip_behind_full")
# Mutants that cannot change an output, whatever the input (tests/test_cpu_render_iter_refs.py asserts that they equal the
# reference on every set): the skip only REMOVES steps from the march, so a change that widens the marched interval, or moves
# its end among steps outside the grown box, is invisible.
#   loop_lt          `t < t_hi` in the loop: the step at t == t_hi lies 2 steps + 0.05 cell outside the box, it is not occupied
#                    (the same `<=` in the staging test is the killable `stage_lt`: the loop then reads an unstaged grid)
#   no_parallel      no |B| < 1e-12 branch: IEEE division gives -inf / +inf inside the slab and inf / inf (or NaN, dropped by
#                    fminf / fmaxf) outside: the same interval
#   parallel_inside  parallel-and-outside treated as inside: widens
MARCH_EQUIVALENT = ("loop_lt", "no_parallel", "parallel_inside")


def slab_interval(inp, tab, mutant=None):
    """[t_lo, t_hi] of k_march_compact's exact skip, float32 as the kernel spells it; (-inf, inf) when the flag word is not 1"""
    na = tab["n_eff"]
    tail = tail_words(inp["occ"]).view(np.int32)
    flag = inp.get("flag", int(tail[0]))
    t_lo, t_hi = np.full(na, -INF, F), np.full(na, INF, F)
    if flag != 1 or na == 0:
        return t_lo, t_hi
    G = inp["G"]
    mg = F(0.0) if mutant == "margin0" else F(0.05)
    aabb = MARCH_AABB.astype(F)
    sc = (F(G) / (aabb[1] - aabb[0])).astype(F)
    a, b = np.full(na, -INF, F), np.full(na, INF, F)
    with np.errstate(all="ignore"):
        for c in range(3):
            lo = F(F(int(tail[1 + 2 * c])) - mg)
            hi = F(F(int(tail[2 + 2 * c]) + 1) + mg)
            A = ((tab["o"][:, c] - aabb[0, c]).astype(F) * sc[c]).astype(F)
            B = (tab["d"][:, c] * sc[c]).astype(F)
            if not lo <= hi:
                a[:], b[:] = INF, -INF
                continue
            par = np.abs(B) < F(1e-12)
            if mutant == "no_parallel":
                par = np.zeros(na, bool)
            outside = ~((A >= lo) & (A <= hi))
            if mutant == "parallel_inside":
                outside = np.zeros(na, bool)
            if mutant == "parallel_outside":
                outside = np.ones(na, bool)
            t1, t2 = ((lo - A).astype(F) / B).astype(F), ((hi - A).astype(F) / B).astype(F)
            if mutant == "no_swap":
                a2, b2 = np.fmax(a, t1), np.fmin(b, t2)
            else:
                a2, b2 = np.fmax(a, np.fmin(t1, t2)), np.fmin(b, np.fmax(t1, t2))
            a = np.where(par, np.where(outside, INF, a), a2).astype(F)
            b = np.where(par, np.where(outside, -INF, b), b2).astype(F)
        two_dt = F(0) * tab["dt"] if mutant == "margin0" else (F(2) * tab["dt"]).astype(F)
        hit = a <= b
        t_lo = np.where(hit, (a - two_dt).astype(F), INF).astype(F)
        t_hi = np.where(hit, (b + two_dt).astype(F), -INF).astype(F)
    return t_lo, t_hi


def march_iter_emulated(inp, tab=None, mutant=None, lds=True):
    """k_march_compact in numpy.  Per ray: the slab interval; `march_skip` to min(far, t_lo) (steps skipped: the leading k with
    t_k < that); trips of four steps from there, a trip starting only while t <= t_hi, every step inside a trip behind
    `t < far && cnt < N`; behind the loop `march_skip` to far unless cnt == N; the second pass re-marches from the first hit.
    lds: the bit grid is staged per workgroup of 256 alive slots only if one of its rays can reach the box (`s_any`); a
    workgroup that did not stage reads ALL ONES here (the worst content an unwritten LDS can have).
    mutant: one of MARCH_MUTANTS / MARCH_EQUIVALENT
      margin0           box not grown, interval not widened
      no_swap           no min / max swap of the slab's two crossings (negative B)
      parallel_outside  a ray parallel to a slab is taken to miss the box
      stage_lt          staging test `t_start < t_hi`
      skip_behind_full  t runs on to far also when the sample cap ended the loop (near_w wrong for the next iteration)"""
    assert mutant is None or mutant in MARCH_MUTANTS + MARCH_EQUIVALENT
    tab = step_table(inp) if tab is None else tab
    na, N, K = tab["n_eff"], tab["n_step"], tab["K"]
    T, L, far, dt = tab["T"], tab["L"], tab["far"], tab["dt"]
    t_lo, t_hi = slab_interval(inp, tab, mutant)
    k = np.arange(K)[None, :]
    with np.errstate(invalid="ignore"):
        pos = dt > 0
        lim = np.fmin(far, t_lo)                                             # fminf
        k_lo = np.where(pos, np.logical_and.accumulate(T < lim[:, None], axis=1).sum(1), 0)
        beyond = ~(T < t_hi[:, None]) if mutant == "loop_lt" else ~(T <= t_hi[:, None])
        # the first step from k_lo on at which a trip may not start, rounded up to a trip boundary
        k_hi = np.where((beyond & (k >= k_lo[:, None])).any(1), np.argmax(beyond & (k >= k_lo[:, None]), axis=1), K)
        k_end = np.minimum(k_lo + 4 * ((k_hi - k_lo + 3) // 4), L)
        t_start = tab["near"]
        reach = (t_start < t_hi) if mutant == "stage_lt" else (t_start <= t_hi)
        wants = (t_start < far) & (t_lo <= t_hi) & reach
    occ_eff = tab["OCC"]
    if lds and na:
        wg = np.arange(na) // WG
        staged = np.zeros(wg.max() + 1, bool)
        np.logical_or.at(staged, wg, wants)
        ok = np.logical_and.accumulate(T < far[:, None], axis=1) & pos[:, None] if na else occ_eff
        occ_eff = np.where(staged[wg][:, None], occ_eff, ok)
    m = occ_eff & (k >= k_lo[:, None]) & (k < k_end[:, None])
    hits = np.cumsum(m, 1)
    total_hits = hits[:, -1] if na else np.zeros(0, np.int64)
    cnt = np.minimum(total_hits, N)
    full = total_hits >= N
    k_last = np.argmax(hits >= N, axis=1) if na else np.zeros(0, np.int64)
    end = np.where(full & (mutant != "skip_behind_full"), k_last + 1, L)
    t_end = np.where(pos, T[np.arange(na), np.minimum(end, K - 1)], tab["near"])
    first = np.where(total_hits > 0, np.argmax(m, axis=1), 0) if na else np.zeros(0, np.int64)
    # the second pass has no t_hi: it takes the first cnt occupied steps from `first` on, whatever the first pass looked at
    k2 = occ_eff & (k >= first[:, None])
    short = k2.sum(1) < cnt
    assert not short.any()
    return _finish_march(inp, tab, cnt, first, t_end, occ_eff)


def march_iter_compare(got, ref, inp, sample_cap=None):
    """The comparison of the GPU test.  got: ray_off, ray_cnt [R], s_t [size], s_pts [size, 3] (prefilled with the sentinels),
    near_w, counter [R], state [2, 8].  Exact: both state records; ray_cnt; near_w and counter of every ray (untouched rays keep
    their value); the ranges of the rays with samples are disjoint and cover [0, n_samples); inside a wave (64 consecutive alive
    slots) they follow each other in lane order; every sample below min(n_samples, sample_cap) holds the reference's bits;
    slots that are not alive, and every sample position from min(n_samples, cap) on, keep the sentinel."""
    na, total = ref["n_eff"], ref["n_samples"]
    assert np.array_equal(np.asarray(got["state"], np.int32).reshape(2, 8), ref["state"]), ("state", np.asarray(got["state"]).tolist(), ref["state"].tolist())
    cnt, off = np.asarray(got["ray_cnt"], np.int64), np.asarray(got["ray_off"], np.int64)
    bad = np.nonzero(cnt != ref["ray_cnt"])[0]
    assert bad.size == 0, ("ray_cnt differs", bad[:8].tolist(), cnt[bad[:8]].tolist(), ref["ray_cnt"][bad[:8]].tolist())
    assert (off[na:] == SENT_I).all(), "ray_off written behind the alive rays"
    for k in ("near_w", "counter"):
        g, w = np.ascontiguousarray(got[k], F), np.ascontiguousarray(ref[k], F)
        d = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
        assert d.size == 0, (k, "differs at rays", d[:8].tolist(), g[d[:8]].tolist(), w[d[:8]].tolist())
    c, o = cnt[:na], off[:na]
    has = np.nonzero(c > 0)[0]
    order = has[np.argsort(o[has], kind="stable")]
    ends = o[order] + c[order]
    assert (o[order] == np.concatenate([[0], ends[:-1]])).all() and (ends[-1] if order.size else 0) == total, \
        ("the rays' ranges do not tile [0, n_samples)", o[order][:8].tolist(), c[order][:8].tolist())
    for w0 in range(0, na, WAVE):               # one atomic per wave: lane order inside it (rays without samples sit at their place)
        cw, ow = c[w0:w0 + WAVE], o[w0:w0 + WAVE]
        if cw.sum():
            assert (ow == ow[0] + np.cumsum(cw) - cw).all(), ("ranges of wave %d are not contiguous in lane order" % (w0 // WAVE), ow.tolist(), cw.tolist())
    size = len(got["s_t"])
    cap = size if sample_cap is None else int(sample_cap)
    assert min(total, cap) <= size
    slot = np.repeat(np.arange(na), c)
    pos = o[slot] + (np.arange(total) - ref["ray_start"][slot])
    m = pos < cap
    for k in ("s_t", "s_pts"):
        g = np.ascontiguousarray(got[k], F)
        want = np.full(g.shape, SENT_F, F)
        want[pos[m]] = ref[k][m]
        ne = g.view(np.uint32) != want.view(np.uint32)
        diff = np.nonzero(ne if ne.ndim == 1 else ne.any(1))[0]
        if diff.size:
            p = int(diff[0])
            raise AssertionError((k, "differs at %d of %d positions, first %d" % (diff.size, size, p), "got", g[p].tolist(), "want", want[p].tolist(),
                                  "n_samples", total, "cap", cap))


# ---- the two rays that kill margin0 and stage_lt ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def special_inputs(which):
    """'stage': ONE alive ray (so its workgroup stages or not on its word alone) whose near_w is exactly the t_hi the kernel
    computes for it -- with `t_start < t_hi` nothing is staged, and the loop's `t <= t_hi` trip reads the unstaged grid.
    'margin': rays from |o| = 1000 at the 64^3 block, searched (seeded) for one on which the skip WITHOUT margins drops a sample:
    the slab arithmetic rounds at |A| ~ 2e4 cells and t ~ 1000 (1e-3 cell), a step that lands that close behind a face is lost."""
    G, grid, ms = 64, "block", 64
    if which == "stage":
        oo, dd, nn, ff = _extra_ray("behind", G, grid, np.random.default_rng(5))
        o, d = np.array([oo], F), np.array([dd], F)
        near, far = np.array([nn], F), np.array([ff + 2.0], F)
        inp = dict(o=o, d=d, near=near, far=far, step=tr.step_size(near, far, ms), occ=iter_occupancy(G, grid), G=G, grid=grid,
                   alive=np.zeros(1, np.int32), n_alive=1, R=1, max_samples=ms, max_batch=4, k_before=0, counter0=np.zeros(1, F), iters0=0, case="stage")
        _, t_hi = slab_interval(inp, step_table(inp))
        assert np.isfinite(t_hi[0]) and t_hi[0] < far[0]
        inp["near"] = t_hi.astype(F)                      # (step stays: it is an input of its own)
        return inp
    assert which == "margin"
    rng = np.random.default_rng(2024)
    n = 4096
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    lo, hi = _box(G, grid)
    tgt = _world(G, lo + (hi - lo) * rng.uniform(0.05, 0.95, (n, 3)))
    o = (tgt - 1000.0 * u).astype(F)
    d = u.astype(F)
    near, far = np.full(n, 999.0, F), np.full(n, 1001.0, F)
    inp = dict(o=o, d=d, near=near, far=far, step=tr.step_size(near, far, ms), occ=iter_occupancy(G, grid), G=G, grid=grid,
               alive=np.arange(n, dtype=np.int32), n_alive=n, R=n, max_samples=ms, max_batch=n * ms, k_before=0, counter0=np.zeros(n, F), iters0=0,
               case="margin")
    tab = step_table(inp)
    ref, mut = march_iter_ref(inp, tab), march_iter_emulated(inp, tab, "margin0", lds=False)
    lost = np.nonzero(ref["ray_cnt"][:n] != mut["ray_cnt"][:n])[0]
    assert lost.size, "no ray found on which the skip without margins drops a sample"
    keep = np.concatenate([lost[:4], np.arange(60)])      # the killers and 60 ordinary rays from 1000 away: one wave
    m = len(keep)
    out = dict(inp, o=o[keep], d=d[keep], near=near[keep], far=far[keep], step=inp["step"][keep], alive=rng.permutation(m).astype(np.int32),
               n_alive=m, R=m, max_batch=m * ms, counter0=np.zeros(m, F))
    return out


# =====================================================================================================================
# compositor
# =====================================================================================================================
N_INITS = (1, 13)
COMPOSITE_MUTANTS = ("group_once", "m_ignored", "no_cnt_rule", "no_last_rule", "seed_neginf", "skip_attenuates", "first_wins_off")
# seed_neginf changes an output only where a non-positive density composites, i.e. with thresh <= 0: the sets with thresh = -0.5
# are there for it (with thresh = 0.01 a sample whose maximum is <= 0 is skipped under either seed).


@functools.lru_cache(maxsize=None)
def composite_inputs(case, G, grid, n_init, thresh=THRESH):
    """The march reference's samples of (case, G, grid) in alive order with seeded candidate tables: per sample pc in 0 ... n_init
    candidates; densities sigma = s / dt with s drawn from {0, U(0, 0.4), U(0.4, 3)} scaled by 0.5 (0.2 for n_init 13), negated, 25 (ends
    the ray), NaN, +-inf;
    every ray i gets its terminating density at sample i % (N + 1) (position N: none), so rays end at each position of a group
    of four; colours in [0, 1] with NaN / inf among them.  Prior colour / depth / T of every ray as a previous iteration leaves
    them (T in (1e-4, 1], some exactly 1, two rays at 5e-5: already terminated)."""
    inp = iter_inputs(case, G, grid)
    return composite_tables(inp, march_iter_ref(inp), n_init, thresh, 977 * n_init + 13 * inp["R"] + GRIDS.index(grid) + G)


def composite_tables(inp, ref, n_init, thresh, seed, fresh=False, kill_rate=0.7):
    """the tables of `composite_inputs` for any input set and its march reference; fresh: the priors k_render_init_rays leaves;
    kill_rate: the share of the candidates at a ray's terminating sample that carry the terminating density"""
    na, N, R, total = ref["n_eff"], ref["n_step"], inp["R"], ref["n_samples"]
    rng = np.random.default_rng(seed)
    cnt = ref["ray_cnt"][:na].astype(np.int64)
    slot = np.repeat(np.arange(na), cnt)
    j = np.arange(total) - ref["ray_start"][slot]
    ray = inp["alive"][:na].astype(np.int64)[slot]
    dt = inp["step"][ray].astype(np.float64)
    pc = rng.integers(0, n_init + 1, total)
    pc[rng.random(total) < 0.5] = n_init                     # half the samples have every candidate valid (first-wins path)
    pt_off = (np.cumsum(pc) - pc).astype(np.int32)
    C = int(pc.sum())
    cs = rng.random(C)
    s = np.where(cs < 0.15, 0.0, np.where(cs < 0.45, rng.uniform(0, 0.4, C), rng.uniform(0.4, 3.0, C)))
    s *= 0.5 if n_init == 1 else 0.2                        # (so that the maximum over a sample's candidates leaves rays alive behind nine samples)
    s[rng.random(C) < 0.08] *= -1.0
    owner = np.repeat(np.arange(total), pc)
    kill = (j[owner] == slot[owner] % (N + 1)) & (rng.random(C) < kill_rate)
    s[kill] = 25.0
    sigma = (s / dt[owner]).astype(F)
    odd = rng.random(C)
    sigma[odd < 0.02] = np.nan
    sigma[(odd >= 0.02) & (odd < 0.03)] = np.inf
    sigma[(odd >= 0.03) & (odd < 0.04)] = -np.inf
    ties = np.nonzero((pc[owner] == n_init) & (np.arange(C) > pt_off[owner]) & (rng.random(C) < 0.1))[0]
    sigma[ties] = sigma[pt_off[owner[ties]]]                 # a later candidate ties with slot 0: the first wins
    rgb = rng.random((C, 3), dtype=F)
    oddc = rng.random((C, 3))
    rgb[oddc < 0.01] = np.nan
    rgb[(oddc >= 0.01) & (oddc < 0.02)] = np.inf
    T0 = rng.uniform(0.05, 1.0, R).astype(F)
    T0[rng.random(R) < 0.3] = 1.0
    if na >= 4:
        T0[inp["alive"][2:4]] = 5e-5
    color0, depth0 = (rng.random((R, 3)) * (1 - T0[:, None])).astype(F), (rng.random(R) * 3).astype(F)
    if fresh:
        T0, color0, depth0 = np.ones(R, F), np.zeros((R, 3), F), np.zeros(R, F)
    out = dict(inp=inp, march=ref, pt_off=pt_off, pt_cnt=pc.astype(np.uint8), cand_sigma=sigma, cand_rgb=rgb, T0=T0, color0=color0, depth0=depth0,
               n_init=n_init, thresh=float(F(thresh)), slot=slot, j=j)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def candidate_max(pt_off, pt_cnt, cand_sigma, cand_rgb, n_init, dtype=np.float64, mutant=None):
    """cand_max(fill = 0, nan_to_num) per sample: (best [P], rgb [P, 3]).  Non-finite densities and colours count as 0; with an
    invalid slot (pc < n_init) the maximum is seeded 0 and only a greater density takes it (colour 0 otherwise); with every slot
    valid the first candidate seeds it; ties keep the earlier candidate."""
    pc, po = np.asarray(pt_cnt, np.int64), np.asarray(pt_off, np.int64)
    P = len(pc)
    sig = np.asarray(cand_sigma, F).astype(dtype)
    sig = np.where(np.isfinite(sig), sig, 0.0)
    col = np.asarray(cand_rgb, F).astype(dtype)
    col = np.where(np.isfinite(col), col, 0.0)
    seeded = pc < n_init
    best = np.where(seeded, -np.inf if mutant == "seed_neginf" else 0.0, -np.inf).astype(dtype)
    bi = np.full(P, -1, np.int64)
    for c in range(int(pc.max()) if P else 0):
        on = c < pc
        v = np.where(on, sig[np.minimum(po + c, len(sig) - 1)] if len(sig) else 0.0, -np.inf)
        take = on & ((v > best) | ((bi < 0) & ~seeded & (c == 0)))
        if mutant == "first_wins_off":
            take = on & ((v >= best) | ((bi < 0) & ~seeded & (c == 0)))
        best = np.where(take, v, best)
        bi = np.where(take, c, bi)
    rgb = np.where((bi >= 0)[:, None], col[np.clip(po + bi, 0, max(len(col) - 1, 0))] if len(col) else 0.0, 0.0)
    return best.astype(dtype), rgb.astype(dtype)


# K of the compositor (k_composite_compact / composite_step, -ffp-contract=off: one rounding per spelled operation):
#   tau   = __expf(x), x = fl(-sg * dl): relative K_TAU_X |x| + K_TAU (module text)
#   alpha = 1 - tau: the error of tau (absolute tau * rel) + the subtraction (1, of |alpha|)
#   T    *= tau: rel(T_j) = rel(T_j-1) + rel(tau_j) + 1
#   w     = alpha * T: |T| err(alpha) + |w| rel(T) + 1 |w|
#   c    += w * rgb: |rgb| err(w) + 1 |w rgb| (product) + 1 |c| (the sum, at the magnitude of the running total)
#   dep  += w * t:   the same with t
# second order: every relative error here stays below 1e-3 (asserted), so a factor 1.002 on the bound covers the products of two.
K_TAU_X, K_TAU, K_SUB, K_MUL, K_ADD = 3.0, 2.0, 1.0, 1.0, 1.0
SECOND_ORDER = 1.002


def composite_ref(cs, march=None, T0=None, color0=None, depth0=None, prior=None):
    """float64 reference of k_composite_compact on the samples of `march` (default: the set's own) and the tables of `cs`.
    Returns color [R, 3], depth, T [R] (rays that are not processed keep their prior), keep [n_eff] (the survival rule), the
    bounds b_color, b_depth, b_T, `undecidable` [n_eff] (alpha or T within its bound of a threshold at some step, or at the
    survival test) and `survivors` (the alive list of the next iteration, in alive order).
    prior: dict(b_color, b_depth, rel_T) per ray [R], the errors the priors carry already (chained iterations)."""
    inp = cs["inp"]
    march = cs["march"] if march is None else march
    na, N, R = march["n_eff"], march["n_step"], inp["R"]
    thresh = cs["thresh"]
    T0 = np.asarray(cs["T0"] if T0 is None else T0, np.float64)
    color = np.array(cs["color0"] if color0 is None else color0, np.float64)
    depth = np.array(cs["depth0"] if depth0 is None else depth0, np.float64)
    Tout = T0.copy()
    b_color = np.zeros((R, 3)) if prior is None else np.array(prior["b_color"], np.float64)
    b_depth = np.zeros(R) if prior is None else np.array(prior["b_depth"], np.float64)
    rel_T_all = np.zeros(R) if prior is None else np.array(prior["rel_T"], np.float64)
    ray = inp["alive"][:na].astype(np.int64)
    cnt, start = march["ray_cnt"][:na].astype(np.int64), march["ray_start"]
    best, rgb = candidate_max(cs["pt_off"], cs["pt_cnt"], cs["cand_sigma"], cs["cand_rgb"], cs["n_init"])
    dt32 = inp["step"][ray]
    dt = dt32.astype(np.float64)
    T, c, dep = T0[ray].copy(), color[ray].copy(), depth[ray].copy()
    relT, bc, bd = rel_T_all[ray].copy(), b_color[ray].copy(), b_depth[ray].copy()
    und = np.zeros(na, bool)
    with np.errstate(all="ignore"):
        for s in range(int(cnt.max()) if na else 0):
            q = np.minimum(start + s, max(len(best) - 1, 0))
            on = (s < cnt) & (dt32 > 0)
            und |= on & (np.abs(T - T_STOP) <= T * relT * SECOND_ORDER)
            on &= T > T_STOP
            x = -best[q] * dt
            tau = np.exp(x)
            rel_tau = U * (K_TAU_X * np.abs(x) + K_TAU)
            alpha = 1.0 - tau
            e_alpha = tau * rel_tau + K_SUB * U * np.abs(alpha)
            e_alpha = np.where(np.isfinite(e_alpha), e_alpha, 0.0)        # tau = inf: alpha = -inf, skipped under any thresh here
            und |= on & (np.abs(alpha - thresh) <= e_alpha * SECOND_ORDER)
            on &= ~(alpha < thresh)
            w = alpha * T
            e_w = T * e_alpha + np.abs(w) * (relT + K_MUL * U)
            tz = march["s_t"][q].astype(np.float64)
            cn = c + np.where(on[:, None], w[:, None] * rgb[q], 0.0)
            dn = dep + np.where(on, w * tz, 0.0)
            bc = np.where(on[:, None], bc + np.abs(rgb[q]) * e_w[:, None] + U * (K_MUL * np.abs(w[:, None] * rgb[q]) + K_ADD * np.abs(cn)), bc)
            bd = np.where(on, bd + np.abs(tz) * e_w + U * (K_MUL * np.abs(w * tz) + K_ADD * np.abs(dn)), bd)
            c, dep = cn, dn
            relT = np.where(on, relT + rel_tau + K_MUL * U, relT)
            T = np.where(on, T * tau, T)
        assert not na or relT.max() < 1e-3
        und |= np.abs(T - T_STOP) <= T * relT * SECOND_ORDER
        last = march["s_t"][np.clip(start + cnt - 1, 0, max(len(march["s_t"]) - 1, 0))] if len(march["s_t"]) else np.zeros(na, F)
        keep = (T > T_STOP) & (cnt == N) & (cnt > 0) & (last > 0)
    color[ray], depth[ray], Tout[ray] = c, dep, T
    b_color[ray], b_depth[ray], rel_T_all[ray] = bc * SECOND_ORDER, bd * SECOND_ORDER, relT
    b_T = np.zeros(R)
    b_T[ray] = T * relT * SECOND_ORDER
    return dict(color=color, depth=depth, T=Tout, keep=keep, b_color=b_color, b_depth=b_depth, b_T=b_T, rel_T=rel_T_all, undecidable=und,
                survivors=ray[keep].astype(np.int32), n_eff=na)


def _exp32(x):
    with np.errstate(over="ignore"):
        return np.exp(np.asarray(x, F).astype(np.float64)).astype(F)


def composite_emulated(cs, mutant=None, march=None):
    """k_composite_compact in plain float32 (exp correctly rounded): trips of four samples, m = min(4, cnt - s), the candidate
    maximum per sample, every step of a trip behind `j < m && T > 1e-4`; survival T > 1e-4 && cnt == N && s_t[last] > 0; the
    survivors appended wave by wave in lane order.  Returns color, depth, T (float32), alive_next, n_next.
    mutant: one of COMPOSITE_MUTANTS
      group_once       termination tested once per trip
      m_ignored        the tail trip composites four samples (it runs into the next ray's)
      no_cnt_rule      survival without cnt == N_steps
      no_last_rule     survival without s_t[last] > 0
      seed_neginf      the maximum seeded -inf when pc < n_init
      skip_attenuates  a skipped sample (alpha < thresh) still multiplies T
      first_wins_off   a tie takes the later candidate"""
    assert mutant is None or mutant in COMPOSITE_MUTANTS
    inp = cs["inp"]
    march = cs["march"] if march is None else march
    na, N, R = march["n_eff"], march["n_step"], inp["R"]
    thresh = F(cs["thresh"])
    ray = inp["alive"][:na].astype(np.int64)
    cnt, start = march["ray_cnt"][:na].astype(np.int64), march["ray_start"]
    best, rgb = candidate_max(cs["pt_off"], cs["pt_cnt"], cs["cand_sigma"], cs["cand_rgb"], cs["n_init"], F, mutant)
    P = len(best)
    dt = inp["step"][ray]
    color, depth, Tall = np.array(cs["color0"], F), np.array(cs["depth0"], F), np.array(cs["T0"], F)
    T, c, dep = Tall[ray].copy(), color[ray].copy(), depth[ray].copy()
    with np.errstate(all="ignore"):
        n_trips = (int(cnt.max()) + 3) // 4 if na else 0
        for g in range(n_trips):
            s0 = 4 * g
            trip = (s0 < cnt) & (T.astype(np.float64) > T_STOP) & (dt > 0)
            m = np.minimum(4, cnt - s0)
            for jj in range(4):
                inm = np.ones(na, bool) if mutant == "m_ignored" else jj < m
                on = trip & inm
                if mutant != "group_once":
                    on &= T.astype(np.float64) > T_STOP
                q = np.clip(start + s0 + jj, 0, max(P - 1, 0))
                tau = _exp32((-best[q] * dt).astype(F)) if P else np.ones(na, F)
                alpha = (F(1) - tau).astype(F)
                skip = alpha < thresh
                if mutant == "skip_attenuates":
                    T = np.where(on & skip, (T * tau).astype(F), T)
                on &= ~skip
                w = (alpha * T).astype(F)
                tz = march["s_t"][q] if P else np.zeros(na, F)
                c = np.where(on[:, None], (c + (w[:, None] * rgb[q]).astype(F)).astype(F), c) if P else c
                dep = np.where(on, (dep + (w * tz).astype(F)).astype(F), dep)
                T = np.where(on, (T * tau).astype(F), T)
        last = march["s_t"][np.clip(start + cnt - 1, 0, max(P - 1, 0))] if P else np.zeros(na, F)
        keep = T.astype(np.float64) > T_STOP
        if mutant != "no_cnt_rule":
            keep &= (cnt == N)
        if mutant != "no_last_rule":
            keep &= (cnt > 0) & (last > 0)
    color[ray], depth[ray], Tall[ray] = c, dep, T
    nxt = np.full(R, SENT_I, np.int32)
    surv = ray[keep].astype(np.int32)
    nxt[:len(surv)] = surv
    return dict(color=color, depth=depth, T=Tall, alive_next=nxt, n_next=len(surv))


MAX_UNDECIDABLE = 0.02


def composite_compare(got, ref, cs, what, report=print):
    """The comparison of the GPU test.  got: color [R, 3], depth, T [R], alive_next [R] (prefilled with the sentinel), n_next.
    Rays that were not processed keep their prior bits.  On the decidable rays: |got - ref| <= bound for colour, depth and T
    (prints one `RATIO <what> color .. depth .. T ..` line), and the survivor set is the reference's.  alive_next holds every survivor once, only processed
    rays, in alive order inside every wave, the sentinel behind n_next."""
    inp = cs["inp"]
    na, R = ref["n_eff"], inp["R"]
    ray = inp["alive"][:na].astype(np.int64)
    und = ref["undecidable"]
    assert und.sum() <= MAX_UNDECIDABLE * max(na, 1), (what, "undecidable rays", int(und.sum()), na)
    untouched = np.ones(R, bool)
    untouched[ray] = False
    for k, prior in (("color", cs["color0"]), ("depth", cs["depth0"]), ("T", cs["T0"])):
        g = np.ascontiguousarray(got[k], F)
        p = np.ascontiguousarray(ref.get("prior_" + k, prior), F)
        assert np.array_equal(g[untouched].view(np.uint32), p[untouched].view(np.uint32)), (what, k, "a ray that is not alive was written")
    ok = ray[~und]
    worst = {}
    for k, b in (("color", "b_color"), ("depth", "b_depth"), ("T", "b_T")):
        g, r, bound = np.asarray(got[k], np.float64)[ok], ref[k][ok], ref[b][ok]
        assert np.isfinite(g).all(), (what, k, "non-finite output")
        err = np.abs(g - r)
        z = bound == 0
        assert (err[z] == 0).all(), (what, k, "differs where the bound is zero", float(err[z].max()) if z.any() else 0)
        ratio = err[~z] / bound[~z]
        worst[k] = float(ratio.max()) if ratio.size else 0.0
        if worst[k] > 1.0:
            report("RATIO %-60s %s %.3f" % (what, k, worst[k]))
            i = int(np.argmax(np.where(z, 0, err / np.where(z, 1, bound)).reshape(len(ok), -1).max(1)))
            raise AssertionError((what, k, "error / bound", worst[k], "ray", int(ok[i]), "got", g[i].tolist(), "ref", r[i].tolist(), "bound", bound[i].tolist()))
    report("RATIO %-60s color %.3f depth %.3f T %.3f" % (what, worst["color"], worst["depth"], worst["T"]))
    n_next = int(got["n_next"])
    nxt = np.asarray(got["alive_next"], np.int64)
    assert (nxt[n_next:] == SENT_I).all(), (what, "alive_next written behind n_alive of the next record")
    surv = nxt[:n_next]
    assert len(set(surv.tolist())) == n_next, (what, "a survivor appears twice")
    slot_of = np.full(R, -1, np.int64)
    slot_of[ray] = np.arange(na)
    assert (slot_of[surv] >= 0).all(), (what, "a ray that was not processed survives")
    got_keep = np.zeros(na, bool)
    got_keep[slot_of[surv]] = True
    bad = np.nonzero((got_keep != ref["keep"]) & ~und)[0]
    assert bad.size == 0, (what, "survivor set differs at slots", bad[:8].tolist(), "kept by the kernel", got_keep[bad[:8]].tolist())
    sl = slot_of[surv]
    wave = sl // WAVE
    same = wave[1:] == wave[:-1]
    assert (sl[1:][same] > sl[:-1][same]).all(), (what, "survivors of one wave are not in lane order")
    # a wave's survivors are contiguous (one atomic per wave)
    if n_next:
        change = np.nonzero(~same)[0]
        firsts = np.concatenate([[wave[0]], wave[1:][change]])
        assert len(set(firsts.tolist())) == len(firsts), (what, "a wave's survivors are not contiguous")
    return worst


def dense_layout(cs, best, rgb, march=None):
    """the samples of a set in the dense [n_eff, N] layout of ia_composite_test: rgb, sigma, delta (0 = empty slot), depth"""
    inp = cs["inp"]
    march = cs["march"] if march is None else march
    na, N = march["n_eff"], march["n_step"]
    ray = inp["alive"][:na].astype(np.int64)
    d_rgb, d_sig, d_delta, d_depth = np.zeros((na, N, 3), F), np.zeros((na, N), F), np.zeros((na, N), F), np.zeros((na, N), F)
    slot = np.repeat(np.arange(na), march["ray_cnt"][:na])
    j = np.arange(march["n_samples"]) - march["ray_start"][slot]
    d_rgb[slot, j], d_sig[slot, j], d_depth[slot, j] = rgb, best, march["s_t"]
    with np.errstate(invalid="ignore"):
        d_delta[slot, j] = np.where(inp["step"][ray][slot] > 0, inp["step"][ray][slot], 0)
    return d_rgb, d_sig, d_delta, d_depth


# =====================================================================================================================
# init and finalize (exact)
# =====================================================================================================================
def init_rays_ref(near, far, max_samples):
    near, far = np.asarray(near, F), np.asarray(far, F)
    R = len(near)
    with np.errstate(invalid="ignore"):
        step = ((far - near).astype(F) / F(max_samples)).astype(F)
    return dict(near_w=near.copy(), step=step, color=np.zeros((R, 3), F), depth=np.zeros(R, F), nohit=np.ones(R, F), counter=np.zeros(R, F),
                alive=np.arange(R, dtype=np.int32))


def finalize_ref(color, depth, nohit, counter, bg, state_end, max_samples):
    color, nohit = np.asarray(color, F), np.asarray(nohit, F)
    b = np.ones_like(color) if bg is None else np.asarray(bg, F)
    with np.errstate(invalid="ignore", over="ignore"):
        rgb = (color + (nohit[:, None] * b).astype(F)).astype(F)
        alpha = (F(1) - nohit).astype(F)
    na = int(state_end[0]) if state_end[3] < max_samples else 0
    return dict(rgb=rgb, depth=np.asarray(depth, F).copy(), alpha=alpha, counter=np.asarray(counter, F).copy(), n_alive_out=np.array([na, state_end[4]], np.int32))
