"""References, case tables and seeded mutants for the two kernel families that bracket a training step (numpy only: no GPU, no product
import):

  A  ia_adam_step       `adam_ref`: one step of torch/optim/adam.py `_single_tensor_adam` as torch's CPU kernels evaluate it -- both forms of
                        ATen's lerp, addcmul as one FMA, float32 IEEE sqrt and division, Python-double bias corrections -- behind GradScaler's
                        skip rule, with the fp16 copy and the gradient zero-fill.  The FMA is EXACT (`fma32`): the float64 sum of the exact
                        product, and rational arithmetic wherever that sum lands on a float32 tie
  B  ia_nonzero_select  `nonzero_select_ref`: np.nonzero(window != 0) at a rank; without replacement by popping from a Python list
  C  ia_mask_edge,      `erode_ref` / `dilate_ref`: the window [-k//2, k-1-k//2] pixel by pixel, pixels outside the image skipped
     ia_mask_dilate
  D  ia_sample_batch    `sample_batch_ref`: float32(u8 / 255.0) from float64, then one rounding per spelled operation, as numpy evaluates
                        `img * msk + (1 - msk) * bg`
  E  ia_patch_corners, ia_edge_indices, ia_near_far   the index maps in float32 (one rounding per operation, as oracle/data_oracle.py `_rank`)
  F  ia_make_rays       float64

The library is built with -ffp-contract=off and `/`, sqrtf are the IEEE operations, so every comparison of A to E is bit for bit or
integer-exact; F keeps the bound of tests/test_gpu_data.py (one float32 ulp below 1).  Nothing in a case table comes from a kernel's
output.  tests/test_cpu_step_io_refs.py pins the references to torch's CPU Adam and to oracle/data_oracle.py and shows that every seeded
mutant fails on these tables; tests/test_gpu_step_io_kernels.py runs the entries."""
import fractions

import numpy as np

F = np.float32
SENT_F = F(-7777.0)
SENT_B = 0xA5                       # prefill of byte buffers and workspaces
SENT_I = np.int32(0x5A5A5A5A)
SENT_H = np.float16(-77.0)
IA_ERR_ARG = -1
IA_ERR_WORKSPACE = -3
ONE_BELOW = np.nextafter(F(1), F(0))                     # 0.99999994
FLT_MAX = np.finfo(F).max


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ======================================================================================================================
# A. ia_adam_step
# ======================================================================================================================
IA_ADAM_MAX_TENSORS = 8
ADAM_THREADS = 256
ADAM_PER_BLOCK = 4096               # 4 float4 per thread: quad k of thread t starts at element (k * 256 + t) * 4 of the workgroup
ADAM_BETAS = ((0.9, 0.99), (0.5, 0.99), (0.500001, 0.99), (0.3, 0.999), (0.0, 0.5))
ADAM_NUMELS = (1, 3, 4, 5, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 2)
ADAM_STEPS = 6
ADAM_MUTANTS = ("lerp_small_form_only", "check_without_tail", "check_without_fourth_quad", "check_first_tensor_only", "skip_advances_step",
                "flag_not_cleared")
FMA_TIES = [0, 0]                   # [sums that landed on a float32 tie, of which the exact value moved the result]: reported by the tests
_TIE_AT_MAX = float(FLT_MAX) + 2.0 ** 103


def fma32(a, b, c):
    """round_to_float32(a * b + c) with ONE rounding, for float32 arrays.  a * b is exact in float64 (48 bits); the float64 sum is rounded
    once, and rounding it again to float32 differs from the fused result only if it lies exactly half way between two float32 values
    (then the bits the first rounding dropped decide): those elements are recomputed in rational arithmetic."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F), np.asarray(c, F))
    shape = a.shape
    a, b, c = a.reshape(-1), b.reshape(-1), c.reshape(-1)
    with np.errstate(all="ignore"):
        s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
        r = s.astype(F)
        r64 = r.astype(np.float64)
        d = s - r64                                                          # exact; -/+ inf where r overflowed
        other = np.nextafter(r, np.where(d > 0, F(np.inf), F(-np.inf)))      # the float32 value on the far side of s
        tie = np.isfinite(s) & (d != 0) & ((np.abs(d) * 2 == np.abs(other.astype(np.float64) - r64)) | (np.abs(s) == _TIE_AT_MAX))
    if tie.any():
        r = r.copy()
        for i in zip(*np.nonzero(tie)):
            exact = fractions.Fraction(float(a[i])) * fractions.Fraction(float(b[i])) + fractions.Fraction(float(c[i]))
            FMA_TIES[0] += 1
            if exact != fractions.Fraction(float(s[i])):
                lo, hi = sorted((r[i], other[i]))
                new = hi if exact > fractions.Fraction(float(s[i])) else lo
                FMA_TIES[1] += int(new != r[i])
                r[i] = new
    return r.reshape(shape) if shape else r[0]


def non_finite(g):
    """GradScaler's check as the kernel makes it: exponent bits all ones"""
    return (bits(g) & 0x7f800000) == 0x7f800000


def _checked(g, mutant, tensor_index):
    """which elements of a gradient tensor a (mutated) non-finite check looks at"""
    n = g.size
    seen = np.ones(n, bool)
    if mutant == "check_without_tail":
        seen[n - n % 4:] = False                                             # the `else for (j = i; j < n; j++)` route
    elif mutant == "check_without_fourth_quad":
        seen[np.arange(n) % ADAM_PER_BLOCK >= 3 * ADAM_THREADS * 4] = False
        seen[n - n % 4:] = True
    elif mutant == "check_first_tensor_only" and tensor_index > 0:
        seen[:] = False
    return seen


def adam_ref(tensors, skip_in=None, zero_grad=False, carry=None, mutant=None):
    """One call of ia_adam_step.  tensors: list of dicts with float32 arrays p, g, m, v (flat, updated in place), `step` (float32 value),
    `lr` (a Python double, or a float32 value where the kernel reads lr_dev), beta1, beta2, eps (doubles) and `shadow` (float16 array,
    updated in place, or None).  skip_in: None (NULL) or a float32 value; non-zero or NaN skips.  Returns found_inf (bool).
    carry: a dict that lives as long as the workspace (only the `flag_not_cleared` mutant keeps anything in it)."""
    carry = {} if carry is None else carry
    bad = any(bool((non_finite(t["g"].reshape(-1)) & _checked(t["g"], mutant, i)).any()) for i, t in enumerate(tensors))
    bad = bad or bool(carry.get("any_bad", False))
    if mutant == "flag_not_cleared":
        carry["any_bad"] = bad
    skip = bad or (skip_in is not None and not (F(skip_in) == F(0)))
    for t in tensors:
        p, g, m, v = t["p"], t["g"], t["m"], t["v"]
        if skip and mutant == "skip_advances_step":
            t["step"] = F(F(t["step"]) + F(1))
        if not skip:
            t["step"] = F(F(t["step"]) + F(1))                                # step_t += 1 on a float32 tensor
            tt = float(t["step"])
            b1, b2 = float(t["beta1"]), float(t["beta2"])
            bc1, bc2 = 1 - b1 ** tt, 1 - b2 ** tt                             # Python floats
            neg_step, bc2_sqrt = F(-(float(t["lr"]) / bc1)), F(bc2 ** 0.5)
            with np.errstate(all="ignore"):
                w = F(1 - b1)
                diff = (g - m).astype(F)
                if abs(w) < F(0.5) or mutant == "lerp_small_form_only":      # ATen native/Lerp.h: is_lerp_weight_small
                    m[...] = fma32(w, diff, m)
                else:                                                         # cpu/LerpKernel.cpp: fmadd(weight - 1, end - start, end)
                    m[...] = fma32(F(w - F(1)), diff, g)
                v[...] = fma32((F(1 - b2) * g).astype(F), g, (F(b2) * v).astype(F))
                denom = ((np.sqrt(v) / bc2_sqrt).astype(F) + F(t["eps"])).astype(F)
                p[...] = (p + ((neg_step * m).astype(F) / denom).astype(F)).astype(F)
                if t.get("shadow") is not None:
                    t["shadow"][...] = p.astype(np.float16)                   # round to nearest even
        if zero_grad:
            g[...] = 0
    return bool(skip)


def adam_groupings():
    """the numels of ADAM_NUMELS as single tensors, in threes and in eights (IA_ADAM_MAX_TENSORS); in every group of several, a tensor
    that ends in a tail (numel % 4096 != 0, numel % 4 != 0) is followed directly by another tensor's first workgroup"""
    one = [(n,) for n in ADAM_NUMELS]
    three = [(4097, 4096, 5), (8191, 1, 4095), (3, 8193, 4), (3 * 4096 + 2, 4097, 1)]
    eight = [(1, 3, 4, 5, 4095, 4097, 4096, 8191), (8193, 3 * 4096 + 2, 5, 4097, 1, 4095, 3, 8191)]
    assert {n for g in three for n in g} == set(ADAM_NUMELS) and {n for g in eight for n in g} == set(ADAM_NUMELS)
    return one + three + eight


# (numels, tensor, element): where the one non-finite gradient element of a case sits
ADAM_BAD_POSITIONS = (
    [((4097,), 0, 0)]
    + [((4096, 5), 0, k * 1024 + k) for k in range(4)]                       # the four float4 slots of thread 0, a component each
    + [((8191,), 0, k * 1024 + 1020 + (3 - k)) for k in range(4)]            # ... of thread 255
    + [((8193,), 0, 4096 + 3 * 1024 + 1020 + 3)]                             # thread 255's last slot in a second workgroup
    + [((4097, 4096), 0, 4096)]                                              # the last element of a tail that is a workgroup of its own
    + [((4095,), 0, 4094), ((3,), 0, 2), ((3 * 4096 + 2, 4), 0, 3 * 4096 + 1)]   # tails behind full quads; no quad at all
    + [((5, 1, 4096), 1, 0)]                                                 # the only element of a one-element tensor
    + [((1, 3, 4, 5, 4095, 4097, 4096, 8191), 7, 8190)])                     # the last element of the eighth tensor
ADAM_BAD_VALUES = (np.uint32(0x7f800000), np.uint32(0xff800000), np.uint32(0x7fc12345), np.uint32(0xffa00001))   # inf, -inf, NaNs with payload


def adam_plan(numels, seed, bad=None, n_steps=ADAM_STEPS):
    """A seeded sequence of calls for one group of tensors: per tensor its hyper-parameters and initial state, per step the gradients, the
    learning rates, skip_in, zero_grad and whether found_inf is asked for.

      step 0  g[::5] = 0 on zero moments; skip_in NULL
      step 1  the arithmetic edges in the first elements: 1e-30 (g g underflows, the denominator is eps), 1e-40 (denormal), 3e19 (v becomes
              inf at beta2 = 0.5 and stays), FLT_MAX (finite: no skip); skip_in 0.0
      step 2  ONE non-finite element (`bad` = (tensor, element), default: the last element of the last tensor); skip_in -0.0
      step 3  clean again: proceeds, reports 0; lr_dev has changed
      step 4  clean gradients, skip_in 2.0 or NaN
      step 5  clean; found_inf = NULL

    beta pairs, lr routes (double / lr_dev), lr = 0, eps, the fp16 copy and a step counter preset to 1e6 rotate over the tensors with the seed."""
    rs = np.random.RandomState(1000 + seed)
    T = len(numels)
    tensors = []
    for i, n in enumerate(numels):
        b1, b2 = ADAM_BETAS[(i + seed) % len(ADAM_BETAS)]
        lr0 = (1e-2, 1e-3, 1e-5)[(i + seed) % 3]
        if T > 1 and i == (seed + 1) % T:
            lr0 = 0.0
        has_shadow = (i + seed) % 2 == 0 or (n % 4 != 0 and (i + seed) % 4 == 1)
        tensors.append(dict(numel=n, beta1=b1, beta2=b2, eps=(1e-15, 1e-8)[(i + seed) % 4 == 3], lr0=lr0, lr_dev=(i + seed) % 2 == 1,
                            has_shadow=has_shadow, step0=F(1e6) if T > 2 and i == (seed + 2) % T else F(0),
                            p0=(rs.randn(n) * 0.1).astype(F)))
    if bad is None:
        bad = (T - 1, numels[-1] - 1)
    steps = []
    for k in range(n_steps):
        g = [(rs.randn(n) * 10.0 ** rs.uniform(-7, 0)).astype(F) for n in numels]
        for a in g:
            if k == 0:
                a[::5] = 0
            if k == 1:
                edge = np.array([1e-30, 1e-40, 3e19, FLT_MAX, -1e-40], F)
                a[1:1 + len(edge)] = edge[:max(0, len(a) - 1)]
        if k == 2:
            g[bad[0]].view(np.uint32)[bad[1]] = ADAM_BAD_VALUES[(seed + bad[1]) % len(ADAM_BAD_VALUES)]
        skip_in = {0: None, 1: F(0.0), 2: F(-0.0), 3: F(-0.0), 4: (F(2.0), F(np.nan))[seed % 2], 5: None}.get(k)
        lr_scale = (1.0, 1.0, 0.5, 0.25, 0.25, 0.125)[k % 6]
        lrs = [F(t["lr0"] * lr_scale) if t["lr_dev"] else t["lr0"] * lr_scale for t in tensors]
        steps.append(dict(g=g, skip_in=skip_in, zero_grad=(k + seed) % 2 == 0, lrs=lrs, want_found=k != 5,
                          expect_skip=k in (2, 4)))
    return dict(numels=tuple(numels), tensors=tensors, steps=steps, bad=bad, seed=seed)


def adam_plans():
    """every plan the GPU test runs: the groupings, then the non-finite positions (steps 0 to 3 of the schedule are enough there)"""
    plans = [adam_plan(g, s) for s, g in enumerate(adam_groupings())]
    plans += [adam_plan(numels, 100 + s, bad=(t, e), n_steps=4) for s, (numels, t, e) in enumerate(ADAM_BAD_POSITIONS)]
    return plans


def adam_initial_state(plan):
    return [dict(p=t["p0"].copy(), m=np.zeros(t["numel"], F), v=np.zeros(t["numel"], F), step=F(t["step0"]), beta1=t["beta1"], beta2=t["beta2"],
                 eps=t["eps"], shadow=np.full(t["numel"], SENT_H, np.float16) if t["has_shadow"] else None) for t in plan["tensors"]]


def adam_run_ref(plan, mutant=None):
    """the plan through adam_ref: per step a snapshot {found, p, m, v, step, shadow, g} (lists over the tensors, copies)"""
    state, carry, out = adam_initial_state(plan), {}, []
    for st in plan["steps"]:
        for t, g, lr in zip(state, st["g"], st["lrs"]):
            t["g"], t["lr"] = g.copy(), lr
        found = adam_ref(state, st["skip_in"], st["zero_grad"], carry, mutant)
        out.append(dict(found=found, step=[float(t["step"]) for t in state], g=[t["g"].copy() for t in state],
                        shadow=[None if t["shadow"] is None else t["shadow"].copy() for t in state],
                        **{k: [t[k].copy() for t in state] for k in ("p", "m", "v")}))
    return out


def adam_snapshots_equal(a, b):
    for x, y in zip(a, b):
        if x["found"] != y["found"] or x["step"] != y["step"]:
            return False
        for k in ("p", "m", "v", "g"):
            if any(not np.array_equal(bits(u), bits(w)) for u, w in zip(x[k], y[k])):
                return False
        if any(u is not None and not np.array_equal(u.view(np.uint16), w.view(np.uint16)) for u, w in zip(x["shadow"], y["shadow"])):
            return False
    return True


# ======================================================================================================================
# B. ia_nonzero_select
# ======================================================================================================================
SELECT_WINDOWS = ((1, 1), (1, 63), (1, 64), (1, 65), (3, 128), (5, 130), (257, 3), (513, 2), (1000, 1))     # rows x cols
SELECT_NS = (0, 1, 3, 4, 5, 500)
SELECT_VALUES = np.array([1.0, 0.25, -1.0, 1e-40, np.nan], F)
SELECT_MUTANTS = ("gt_half", "gt_zero", "no_fixed_point")
MAX_DRAWS_WITHOUT_REPLACEMENT = 256


def select_frames(rows, cols):
    """(H, W, y0, y1, x0, x1): the window inside a larger mask at offsets that are no multiples of 64, and as the whole mask"""
    return ((rows + 12, cols + 48, 7, 7 + rows, 37, 37 + cols), (rows, cols, 0, rows, 0, cols))


def select_mask(frame, kind, seed, count=None):
    """a mask [H,W] whose surroundings of the window are dense garbage.  kind: "mixed" (about 20 % nonzero from SELECT_VALUES, zeros of
    both signs, empty rows at the start and at the end where there are 3 rows or more, and in the middle from 5 rows), "last_only", "all_zero",
    "count" (exactly `count` ones at seeded places)"""
    H, W, y0, y1, x0, x1 = frame
    rs = np.random.RandomState(seed)
    rows, cols = y1 - y0, x1 - x0
    m = np.where(rs.rand(H, W) < 0.5, F(1), F(0.5)).astype(F)
    win = np.where(rs.rand(rows, cols) < 0.5, F(0.0), F(-0.0)).astype(F)
    if kind == "mixed":
        on = rs.rand(rows, cols) < 0.2
        if rows * cols <= 2:
            on[...] = True
        win[on] = SELECT_VALUES[rs.randint(0, len(SELECT_VALUES), int(on.sum()))]
        if rows >= 3:
            for r in (0, rows - 1) + ((rows // 2,) if rows >= 5 else ()):
                win[r] = np.where(rs.rand(cols) < 0.5, F(0.0), F(-0.0))
    elif kind == "last_only":
        win[-1, -1] = F(0.25)
    elif kind == "count":
        win.reshape(-1)[rs.permutation(rows * cols)[:count]] = 1
    else:
        assert kind == "all_zero"
    m[y0:y1, x0:x1] = win
    return m


def _is_candidate(win, mutant):
    with np.errstate(invalid="ignore"):
        if mutant == "gt_half":
            return win > F(0.5)
        if mutant == "gt_zero":
            return win > 0
        return win != 0


def nonzero_select_ref(mask, window, u, without_replacement=False, mutant=None):
    """(rows [n], cols [n], count): np.nonzero(mask[y0:y1, x0:x1] != 0) in row-major order at rank min(floor(float32(u) * float32(count)),
    count - 1) -- relative to the window; without replacement the rank counts among the candidates not chosen before (popped from a
    list); -1 once nothing is left or the count is 0"""
    y0, y1, x0, x1 = window
    rr, cc = np.nonzero(_is_candidate(np.asarray(mask, F)[y0:y1, x0:x1], mutant))
    count = len(rr)
    remaining = list(range(count))
    rows, cols = [], []
    for ui in np.asarray(u, F).reshape(-1):
        left = len(remaining) if without_replacement else count
        if left == 0:
            rows.append(-1); cols.append(-1)
            continue
        r = min(int(np.floor(F(ui) * F(left))), left - 1)
        if without_replacement and mutant == "no_fixed_point":
            remaining.pop()                                                   # one fewer left, but r is taken as a rank among ALL candidates
        elif without_replacement:
            r = remaining.pop(r)
        rows.append(int(rr[r])); cols.append(int(cc[r]))
    return np.array(rows, np.int32), np.array(cols, np.int32), count


def select_draws(count, n, seed):
    """at least n draws: 0, 0.5, the float32 below 1, exactly 1 (outside [0,1): the one draw that reaches the rank's clamp to count - 1 --
    u < 1 never rounds u * count up to count), then for every rank r the float32 r / count and its two neighbours, the rest uniform"""
    rs = np.random.RandomState(seed)
    u = [F(0), F(0.5), ONE_BELOW, F(1)]
    for r in range(count):
        x = F(r / count)
        u += [np.nextafter(x, F(-1)), x, np.nextafter(x, F(2))]
    u = np.array(u, F)
    u = u[(u >= 0) & (u <= 1)]
    if len(u) < n:
        u = np.concatenate([u, rs.rand(n - len(u)).astype(F)])
    return u


def chunks(u, n):
    """the draws in calls of n; a short last call is filled up with 0.5"""
    out = []
    for i in range(0, max(len(u), 1), n):
        c = u[i:i + n]
        out.append(np.concatenate([c, np.full(n - len(c), 0.5, F)]))
    return out


def without_replacement_cases():
    """(name, frame, count, draws): the fixed-point loop among adjacent chosen elements, exhaustion, and the limit of 256 draws"""
    rs = np.random.RandomState(7)
    f20, f5, f300, f300b = select_frames(5, 130)[0], select_frames(1, 65)[0], select_frames(257, 3)[0], select_frames(3, 128)[1]
    return (("20 of 20, all draws 0", f20, 20, np.zeros(20, F)),
            ("20 of 20, all draws just below 1", f20, 20, np.full(20, ONE_BELOW, F)),
            ("20 of 20, random", f20, 20, rs.rand(20).astype(F)),
            ("8 of 5", f5, 5, rs.rand(8).astype(F)),
            ("8 of 5, all draws 0", f5, 5, np.zeros(8, F)),
            ("256 of 300", f300, 300, rs.rand(256).astype(F)),
            ("256 of 300, three rows, low draws", f300b, 300, (rs.rand(256) * 0.05).astype(F)))


# ======================================================================================================================
# C. ia_mask_edge / ia_mask_dilate
# ======================================================================================================================
MORPH_CASES = ((1, 1, 1), (1, 70, 5), (70, 1, 16), (9, 7, 16), (33, 65, 1), (33, 65, 2), (33, 65, 7), (33, 65, 8), (300, 1, 32))   # (H, W, k)
MORPH_MUTANTS = ("symmetric_window", "zero_border")


def _morph(mask, k, fn, mutant):
    m = np.asarray(mask, F)
    H, W = m.shape
    a = k // 2
    lo, hi = -a, (a if mutant == "symmetric_window" else k - 1 - a)
    out = np.empty((H, W), F)
    for y in range(H):
        for x in range(W):
            vals = [m[yy, xx] if (0 <= yy < H and 0 <= xx < W) else F(0)
                    for yy in range(y + lo, y + hi + 1) for xx in range(x + lo, x + hi + 1)
                    if mutant == "zero_border" or (0 <= yy < H and 0 <= xx < W)]
            out[y, x] = fn(vals)
    return out


def erode_ref(mask, k, mutant=None):
    """cv2.erode(mask, ones((k, k))): the minimum over rows / columns [-k//2, k-1-k//2] around the pixel, pixels outside the image skipped"""
    return _morph(mask, k, min, mutant)


def dilate_ref(mask, k, mutant=None):
    return _morph(mask, k, max, mutant)


def edge_band_ref(mask, k, mutant=None):
    return (dilate_ref(mask, k, mutant) - erode_ref(mask, k, mutant)).astype(F)


def morph_masks(H, W):
    """{name: mask}: blobs of {0.25, 0.5, 1} on 0 that touch every border, and uniform random floats"""
    rs = np.random.RandomState(H * 1000 + W)
    m = np.zeros((H, W), F)
    yy, xx = np.mgrid[0:H, 0:W]
    m[(yy - H * 0.5) ** 2 / max(H * 0.3, 1) ** 2 + (xx - W * 0.5) ** 2 / max(W * 0.3, 1) ** 2 < 1] = 1
    m[:max(1, H // 6), :max(1, W // 3)] = 0.25                               # top-left corner: top and left borders
    m[H - max(1, H // 8):, W - max(1, W // 4):] = 0.5                        # bottom-right corner: bottom and right borders
    if H * W > 1:
        m[(yy + xx) % 11 == 5] = 0                                           # holes one pixel wide
    return {"blobs": m, "random": rs.rand(H, W).astype(F)}


# ======================================================================================================================
# D. ia_sample_batch
# ======================================================================================================================
BATCH_H = BATCH_W = 16
BATCH_FLAT_NS = (1, 255, 256, 257)
BATCH_PATCHES = ((1, 1), (1, 4), (3, 1), (3, 4), (8, 1), (8, 4))            # (patch, n_patch)
BATCH_MUTANTS = ("fma",)


def batch_frame():
    """one 16 x 16 frame: uint8 image holding every byte value, the same as float32(u8 / 255), a mask of {0, 1, 0.25, 1/3, 0.999} and
    random float32 values, rays"""
    rs = np.random.RandomState(11)
    n = BATCH_H * BATCH_W
    u8 = np.stack([rs.permutation(256), rs.permutation(256), np.arange(256)], -1).astype(np.uint8)
    mask = rs.rand(n).astype(F)
    special = np.array([0, 1, 0.25, 1 / 3, 0.999], F)
    mask[:160] = special[rs.randint(0, 5, 160)]
    mask = mask[rs.permutation(n)]
    return dict(u8=u8, img_f=(u8 / 255.0).astype(F), mask=mask, rays_o=rs.randn(n, 3).astype(F), rays_d=rs.randn(n, 3).astype(F))


def sample_batch_ref(frame, W, flat_idx=None, corners=None, patch=0, bg=None, use_float_image=False, mutant=None):
    """(rgb [n,3], alpha [n], rays_o [n,3], rays_d [n,3], bg_out [n,3], idx_out [n]) of ia_sample_batch: v = float32(u8 / 255.0) (float64
    division, one rounding), rgb = fl(fl(v m) + fl(fl(1 - m) b)), b = 1 where bg is None"""
    if flat_idx is not None:
        pix = np.asarray(flat_idx, np.int64)
    else:
        rows, cols = corners
        pix = np.concatenate([((r + np.arange(patch))[:, None] * W + c + np.arange(patch)[None, :]).reshape(-1) for r, c in zip(rows, cols)])
    v = frame["img_f"][pix] if use_float_image else (frame["u8"][pix].astype(np.float64) / 255.0).astype(F)
    m = frame["mask"][pix][:, None].astype(F)
    b = np.ones((len(pix), 3), F) if bg is None else np.asarray(bg, F).reshape(len(pix), 3)
    if mutant == "fma":
        rgb = fma32(v, m, ((F(1) - m).astype(F) * b).astype(F))
    else:
        rgb = ((v * m).astype(F) + ((F(1) - m).astype(F) * b).astype(F)).astype(F)
    return rgb, m[:, 0].copy(), frame["rays_o"][pix], frame["rays_d"][pix], b.copy(), pix.astype(np.int32)


def batch_flat_indices(n):
    rs = np.random.RandomState(n)
    idx = rs.randint(0, BATCH_H * BATCH_W, n)
    idx[0] = BATCH_H * BATCH_W - 1
    if n > 3:
        idx[1], idx[2], idx[3] = 0, 0, BATCH_H * BATCH_W - 1               # repeated indices, the first and the last pixel
    return idx.astype(np.int32)


def batch_corners(patch, n_patch):
    """corners with (0, 0) and (H - P, W - P) among them"""
    rs = np.random.RandomState(patch * 10 + n_patch)
    rows, cols = rs.randint(0, BATCH_H - patch + 1, n_patch), rs.randint(0, BATCH_W - patch + 1, n_patch)
    rows[0], cols[0] = BATCH_H - patch, BATCH_W - patch
    if n_patch > 1:
        rows[1], cols[1] = 0, 0
    return rows.astype(np.int32), cols.astype(np.int32)


# ======================================================================================================================
# E. ia_patch_corners, ia_edge_indices, ia_near_far
# ======================================================================================================================
CORNER_MUTANTS = ("coin_le", "clamp_h_minus_p")
CORNER_NS = (1, 4, 65)


def _floor_mul(u, count, top):
    """min(floor(fl(u * float32(count))), top) in float32, as an integer"""
    return np.minimum(np.floor((np.asarray(u, F) * F(count)).astype(F)), F(top)).astype(np.int32)


def patch_corners_ref(row_mask, col_mask, draws, n, H, W, P, ratio_mask, mutant=None):
    """PatchSampler's corners: the mask picks where coin < ratio_mask and the pick is not -1, else floor(u (H - P)) clamped to H - P - 1
    (np.random.randint(0, H - P)); draws [1 + 2 n]: coin, row draws, column draws"""
    d = np.asarray(draws, F)
    use_mask = d[0] <= F(ratio_mask) if mutant == "coin_le" else d[0] < F(ratio_mask)
    off = 0 if mutant == "clamp_h_minus_p" else 1
    fr, fc = _floor_mul(d[1:1 + n], H - P, H - P - off), _floor_mul(d[1 + n:1 + 2 * n], W - P, W - P - off)
    rm, cm = np.asarray(row_mask, np.int32), np.asarray(col_mask, np.int32)
    from_mask = use_mask & (rm >= 0) & (cm >= 0)
    return np.where(from_mask, rm, fr).astype(np.int32), np.where(from_mask, cm, fc).astype(np.int32)


def corner_cases():
    """(name, H, W, P, ratio, n, draws, row_mask, col_mask)"""
    out = []
    below = np.nextafter(F(0.9), F(0))
    for n in CORNER_NS:
        rs = np.random.RandomState(n)
        for name, coin, ratio in (("coin == ratio", F(0.9), 0.9), ("coin just below ratio", below, 0.9), ("coin 0, ratio 1", F(0), 1.0),
                                  ("coin just below 1, ratio 1", ONE_BELOW, 1.0), ("coin 0, ratio 0", F(0), 0.0)):
            for H, W, P in ((40, 57, 16), (17, 18, 16), (9, 300, 8)):          # H - P = 1 in the second
                anchors = rs.rand(2 * n).astype(F)
                anchors[0], anchors[-1] = 0, ONE_BELOW
                if n > 1:
                    anchors[1], anchors[n] = ONE_BELOW, 0
                if n > 3:
                    anchors[2], anchors[n + 1] = 1, 1                         # exactly 1: the only draw that reaches the clamp to H - P - 1
                rm, cm = rs.randint(0, H - P, n).astype(np.int32), rs.randint(0, W - P, n).astype(np.int32)
                rm[::3] = -1
                cm[::3] = -1                                                  # -1 in some slots only
                out.append(("%s, n %d, %d x %d patch %d" % (name, n, H, W, P), H, W, P, ratio, n, np.concatenate([[coin], anchors]).astype(F), rm, cm))
    return out


def edge_indices_ref(r_m, c_m, r_e, c_e, draws, n_mask, n_edge, n_rand, H, W):
    """[mask picks | band picks | uniform picks] as flat indices; a pick of -1 falls back to the uniform pixel of its own draw,
    min(floor(fl(u * float32(H W))), H W - 1)"""
    n = n_mask + n_edge + n_rand
    uni = _floor_mul(np.asarray(draws, F)[:n], H * W, H * W - 1).astype(np.int64)
    out = uni.copy()
    for lo, cnt, r, c in ((0, n_mask, r_m, c_m), (n_mask, n_edge, r_e, c_e)):
        if cnt:
            p = np.asarray(r, np.int64)[:cnt] * W + np.asarray(c, np.int64)[:cnt]
            out[lo:lo + cnt] = np.where(p >= 0, p, uni[lo:lo + cnt])
    return out.astype(np.int32)


def edge_index_cases():
    """(name, H, W, n_mask, n_edge, n_rand, draws, r_m, c_m, r_e, c_e): each share empty in turn, -1 picks, a ragged launch"""
    out = []
    for name, (nm, ne, nr) in (("all three", (150, 77, 30)), ("no mask share", (0, 77, 30)), ("no band share", (150, 0, 30)),
                               ("no uniform share", (150, 77, 0)), ("one pick", (0, 0, 1))):
        rs = np.random.RandomState(nm + 3 * ne + 7 * nr)
        H, W = 37, 53
        draws = rs.rand(nm + ne + nr).astype(F)
        draws[0], draws[-1] = ONE_BELOW, 0 if nm + ne + nr > 1 else ONE_BELOW
        pick = lambda k: (rs.randint(0, H, k).astype(np.int32), rs.randint(0, W, k).astype(np.int32))
        (r_m, c_m), (r_e, c_e) = pick(nm), pick(ne)
        for r, c in ((r_m, c_m), (r_e, c_e)):
            r[::4] = -1
            c[::4] = -1
        out.append((name, H, W, nm, ne, nr, draws, r_m, c_m, r_e, c_e))
    return out


NEAR_FAR_NS = (1, 257)
NEAR_FAR_TRANSL = ((0.0, 0.0, 0.0), (0.1, -0.2, 5.0), (1e-40, 0.25, -3.0), (1e-20, 1e-20, 1e-20), (3.0, 4.0, 12.0), (0.013, 0.15, 4.93))


def near_far_ref(transl):
    """(near, far) = |t| -/+ 1 with |t| = sqrt(fl(fl(fl(x x) + fl(y y)) + fl(z z))) in float32 (numpy's order at peoplesnapshot.py:146)"""
    x, y, z = (F(v) for v in transl)
    with np.errstate(under="ignore"):
        d = np.sqrt(F(F(F(x * x) + F(y * y)) + F(z * z)))
    return F(d - F(1)), F(d + F(1))


# ======================================================================================================================
# F. ia_make_rays
# ======================================================================================================================
RAY_SHAPES = ((1, 1), (1, 300), (300, 1), (37, 53))
RAY_ULP = 6e-8                       # one float32 ulp below 1: both sides evaluate in float64 and round once


def ray_camera(H, W):
    """K with an off-centre principal point, a rotation about a skew axis, a translation"""
    K = np.array([[2000.0 * max(H, 8) / 1080, 0.3, W * 0.37 + 1.5], [0, 1900.0 * max(H, 8) / 1080, H * 0.61 - 0.25], [0, 0, 1]])
    axis = np.array([0.3, -0.8, 0.52])
    axis /= np.linalg.norm(axis)
    a = 0.7
    X = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(a) * X + (1 - np.cos(a)) * X @ X
    return K, R, np.array([0.1, -0.2, 0.3])


def make_rays_ref(K_inv, R, t, H, W):
    """rays_o [H W,3] = t; rays_d = normalise(R (K_inv [x, y, 1])) in float64, pixel by pixel, x fastest"""
    K_inv, R = np.asarray(K_inv, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3)
    d = np.empty((H * W, 3))
    for i in range(H * W):
        dc = K_inv @ np.array([float(i % W), float(i // W), 1.0])
        dw = R @ dc
        d[i] = dw / np.sqrt((dw * dw).sum())
    return np.tile(np.asarray(t, np.float64), (H * W, 1)), d
