"""float64 reference, error bounds, an fp32 emulation and mutants of `ia_scene_deep_composite`, written from the text of
include/instantavatar_hip_scene_deep.h ("scene composition", step 5).  numpy only: no GPU, no product import.

REFERENCE (`deep_ref`).  The procedure of the header in float64 on the fp32 inputs, with the same decisions as the kernel: the order
of the samples is decided by fp32 keys compared exactly, so it is never in doubt; a sample is skipped when alpha < thresh and a
list ends when its own T_k <= 1e-4.  A pixel where a float64 alpha comes within its error of thresh, or a T_k within its bound of
1e-4 at a step where that decides whether a head exists, is UNDECIDABLE and left out of the value comparison.

BOUNDS, |got - ref| <= sum K u M, the per-operation constants of tests/render_iter_refs.py (`U`, `K_TAU_X`, `K_TAU`, `K_SUB`, `K_MUL`,
`K_ADD`, `SECOND_ORDER`; derived there from the lowering of __expf, not tuned):
  tau   = __expf(x), x = fl(-sg dl): relative u (K_TAU_X |x| + K_TAU)
  alpha = 1 - tau: tau rel(tau) + K_SUB u |alpha|
  c f_k (only with a factor): one more product, K_MUL u |c f_k|
  w     = alpha T: T err(alpha) + |w| (rel(T) + K_MUL u), with rel(T) of the JOINT transmittance, which inherits rel(tau) + K_MUL u from
          every composited sample of every list (and K_SUB u + K_MUL u from the ground's factor 1 - a_g)
  C    += w c: |c| err(w) + |w| err(c) + u (K_MUL |w c| + K_ADD |C|);  D += w z alike
  T_k inherits rel(tau) + K_MUL u from its own samples only (it decides nothing but the list's end)
  ground: (c_g shade) a_g carries 2 K_MUL u, T times it rel(T) + K_MUL u, the sum K_ADD u |C|; a_g t_g one product
  end: T bg one product and one sum; 1 - T: T rel(T) + K_SUB u |1 - T|
second order: every relative error stays below 1e-3 (asserted), so the factor SECOND_ORDER covers the products of two.

EMULATION (`deep_emulated`): the kernel's loop in plain float32 with a correctly rounded exp, carrying one-line mutants (`MUTANTS`)."""
import numpy as np

from render_iter_refs import F, K_ADD, K_MUL, K_SUB, K_TAU, K_TAU_X, MAX_UNDECIDABLE, SECOND_ORDER, T_STOP, THRESH, U, _exp32

MAX_LAYERS, MAX_SLOTS = 8, 1024
MUTANTS = ("layer_order", "no_own_stop", "skip_attenuates", "tie_high", "ground_by_mean")


def _ground_ok(case, p):
    g = case.get("ground")
    if g is None:
        return False
    t_g, a_g, c_g, sh = g
    with np.errstate(all="ignore"):
        return bool(a_g[p] > 0 and np.isfinite(a_g[p]) and np.isfinite(t_g[p]) and np.isfinite(sh[p]) and np.isfinite(c_g[p]).all())


def _bg(case, n):
    bg = case.get("bg")
    if bg is None:
        return None
    bg = np.asarray(bg, F)
    return np.broadcast_to(bg.reshape(1, 3), (n, 3)) if bg.size == 3 else bg.reshape(n, 3)


def deep_ref(case):
    """case: dict(z, delta, sigma [K,S,n] fp32, rgb [K,S,n,3], factor None | [K,n], ground None | (t_g [n], a_g [n], c_g [n,3],
    shade [n]), bg None | [3] | [n,3], thresh).
    -> dict(rgb [n,3], alpha, depth [n], T [n], b_rgb, b_alpha, b_depth, undecidable [n] bool, interleaved_mask [n] bool,
    interleaved int, owners: per pixel the owners of the composited items in merged order (K = the ground), consecutive repeats
    removed, n_composited [n])"""
    z32, dl32 = np.asarray(case["z"], F), np.asarray(case["delta"], F)
    K, S, n = z32.shape
    assert 1 <= K <= MAX_LAYERS and 1 <= S <= MAX_SLOTS
    f64 = lambda x: np.asarray(x, F).astype(np.float64)
    z, dl, sg, col = f64(z32), f64(dl32), f64(case["sigma"]), f64(case["rgb"])
    assert sg.shape == (K, S, n) and col.shape == (K, S, n, 3)
    sg = np.where(np.isfinite(sg), sg, 0.0)
    col = np.where(np.isfinite(col), col, 0.0)
    fac = None if case.get("factor") is None else f64(case["factor"])
    thresh = float(F(case.get("thresh", THRESH)))
    bg = _bg(case, n)
    out = dict(rgb=np.zeros((n, 3)), alpha=np.zeros(n), depth=np.zeros(n), T=np.zeros(n), b_rgb=np.zeros((n, 3)), b_alpha=np.zeros(n),
               b_depth=np.zeros(n), undecidable=np.zeros(n, bool), interleaved_mask=np.zeros(n, bool), owners=[],
               n_composited=np.zeros(n, np.int64))
    for p in range(n):
        C, D, T, relT = np.zeros(3), 0.0, 1.0, 0.0
        bC, bD = np.zeros(3), 0.0
        Tk, relTk, cur = np.ones(K), np.zeros(K), np.zeros(K, np.int64)
        ground = _ground_ok(case, p)
        und, owners, seen, inter = False, [], set(), False
        with np.errstate(all="ignore"):
            for _ in range(K * S + 1):
                sel, zmin = -1, np.inf
                for k in range(K):
                    s = cur[k]
                    if s < S and dl32[k, s, p] > 0 and np.isfinite(z32[k, s, p]):
                        und |= bool(abs(Tk[k] - T_STOP) <= Tk[k] * relTk[k] * SECOND_ORDER)
                        if Tk[k] > T_STOP and z32[k, s, p] < zmin:
                            sel, zmin = k, z32[k, s, p]
                if ground and not zmin <= case["ground"][0][p]:
                    t_g, a_g, c_g, sh = (float(F(x[p])) if np.ndim(x[p]) == 0 else f64(x[p]) for x in case["ground"])
                    g = (c_g * sh) * a_g
                    term = T * g
                    Cn = C + term
                    bC = bC + np.abs(term) * (relT + 3 * K_MUL * U) + K_ADD * U * np.abs(Cn)
                    dterm = T * (a_g * t_g)
                    Dn = D + dterm
                    bD = bD + abs(dterm) * (relT + 2 * K_MUL * U) + K_ADD * U * abs(Dn)
                    C, D = Cn, Dn
                    T = T * (1.0 - a_g)
                    relT += (K_SUB + K_MUL) * U
                    ground = False
                    owners.append(K)
                    continue
                if sel < 0:
                    break
                k, s = sel, cur[sel]
                cur[k] += 1
                x = -sg[k, s, p] * dl[k, s, p]
                tau = np.exp(x)
                rel_tau = U * (K_TAU_X * abs(x) + K_TAU)
                alpha = 1.0 - tau
                e_alpha = tau * rel_tau + K_SUB * U * abs(alpha)
                if not np.isfinite(e_alpha):          # tau = inf: alpha = -inf, skipped under any thresh here
                    e_alpha = 0.0
                und |= bool(abs(alpha - thresh) <= e_alpha * SECOND_ORDER)
                if alpha < thresh:
                    continue
                c, e_c = col[k, s, p], np.zeros(3)
                if fac is not None:
                    c = c * fac[k, p]
                    e_c = K_MUL * U * np.abs(c)
                w = alpha * T
                e_w = T * e_alpha + abs(w) * (relT + K_MUL * U)
                Cn = C + w * c
                bC = bC + np.abs(c) * e_w + abs(w) * e_c + U * (K_MUL * np.abs(w * c) + K_ADD * np.abs(Cn))
                Dn = D + w * z[k, s, p]
                bD = bD + abs(z[k, s, p]) * e_w + U * (K_MUL * abs(w * z[k, s, p]) + K_ADD * abs(Dn))
                C, D = Cn, Dn
                T, Tk[k] = T * tau, Tk[k] * tau
                relT += rel_tau + K_MUL * U
                relTk[k] += rel_tau + K_MUL * U
                out["n_composited"][p] += 1
                if not owners or owners[-1] != k:
                    inter |= k in seen
                    seen.add(k)
                    owners.append(k)
        assert relT < 1e-3 and relTk.max() < 1e-3
        if bg is not None:
            b = f64(bg[p])
            rgb = C + T * b
            bC = bC + np.abs(T * b) * (relT + K_MUL * U) + K_ADD * U * np.abs(rgb)
            out["rgb"][p], out["alpha"][p] = rgb, 1.0
        else:
            out["rgb"][p], out["alpha"][p] = C, 1.0 - T
            out["b_alpha"][p] = (T * relT + K_SUB * U * abs(1.0 - T)) * SECOND_ORDER
        out["depth"][p], out["T"][p] = D, T
        out["b_rgb"][p], out["b_depth"][p] = bC * SECOND_ORDER, bD * SECOND_ORDER
        out["undecidable"][p], out["interleaved_mask"][p] = und, inter
        out["owners"].append(owners)
    out["interleaved"] = int(out["interleaved_mask"].sum())
    return out


def deep_emulated(case, mutant=None):
    """the kernel's loop in plain float32 (exp correctly rounded) -> dict(rgb [n,3], alpha, depth [n] fp32, interleaved int).
    mutant: one of MUTANTS
      layer_order      the lists are taken in layer order instead of depth order (a whole avatar in front of the next)
      no_own_stop      a list does not end where its own transmittance falls to 1e-4
      skip_attenuates  a skipped sample (alpha < thresh) still multiplies T and T_k
      tie_high         an exact tie in z goes to the higher layer
      ground_by_mean   the ground is placed by the avatars' mean depths: behind every list whose mean z lies in front of it"""
    assert mutant is None or mutant in MUTANTS
    z, dl = np.asarray(case["z"], F), np.asarray(case["delta"], F)
    K, S, n = z.shape
    sg, col = np.asarray(case["sigma"], F), np.asarray(case["rgb"], F)
    sg = np.where(np.isfinite(sg), sg, F(0))
    col = np.where(np.isfinite(col), col, F(0))
    fac = None if case.get("factor") is None else np.asarray(case["factor"], F)
    thresh = F(case.get("thresh", THRESH))
    bg = _bg(case, n)
    rgb, alpha, depth = np.zeros((n, 3), F), np.zeros(n, F), np.zeros(n, F)
    count = 0
    with np.errstate(all="ignore"):
        filled = (dl > 0) & np.isfinite(z)
        mean = np.where(filled, z, 0).astype(np.float64).sum(1) / np.maximum(filled.sum(1), 1)      # [K,n]
        for p in range(n):
            C, D, T = np.zeros(3, F), F(0), F(1)
            Tk, cur = np.ones(K, F), np.zeros(K, np.int64)
            ground = _ground_ok(case, p)
            last, seen, inter = -1, set(), False
            for _ in range(K * S + 1):
                sel, zmin, heads = -1, F(np.inf), []
                for k in range(K):
                    s = cur[k]
                    if s < S and dl[k, s, p] > 0 and np.isfinite(z[k, s, p]) and (mutant == "no_own_stop" or float(Tk[k]) > T_STOP):
                        heads.append(k)
                        better = z[k, s, p] <= zmin if mutant == "tie_high" else z[k, s, p] < zmin
                        if mutant == "layer_order":
                            better = sel < 0
                        if better:
                            sel, zmin = k, z[k, s, p]
                if ground:
                    t_g, a_g, c_g, sh = (x[p] for x in case["ground"])
                    first = not zmin <= t_g
                    if mutant == "ground_by_mean":
                        first = not any(mean[k, p] <= t_g for k in heads)
                    if first:
                        C = (C + (T * ((c_g * sh).astype(F) * a_g).astype(F)).astype(F)).astype(F)
                        D = F(D + F(T * F(a_g * t_g)))
                        T = F(T * F(F(1) - a_g))
                        ground, last = False, K
                        continue
                if sel < 0:
                    break
                k, s = sel, cur[sel]
                cur[k] += 1
                tau = F(_exp32(F(-sg[k, s, p] * dl[k, s, p])))
                a = F(F(1) - tau)
                if a < thresh:
                    if mutant == "skip_attenuates":
                        T, Tk[k] = F(T * tau), F(Tk[k] * tau)
                    continue
                c = col[k, s, p]
                if fac is not None:
                    c = (c * fac[k, p]).astype(F)
                w = F(a * T)
                C = (C + (w * c).astype(F)).astype(F)
                D = F(D + F(w * z[k, s, p]))
                T, Tk[k] = F(T * tau), F(Tk[k] * tau)
                if last != k:
                    inter |= k in seen
                    seen.add(k)
                    last = k
            if bg is not None:
                rgb[p], alpha[p] = (C + (T * bg[p]).astype(F)).astype(F), F(1)
            else:
                rgb[p], alpha[p] = C, F(F(1) - T)
            depth[p] = D
            count += int(inter)
    return dict(rgb=rgb, alpha=alpha, depth=depth, interleaved=count)


def deep_compare(got, ref, what, report=print):
    """The comparison of the GPU test.  got: rgb [n,3], alpha, depth [n], interleaved.  On the decidable pixels |got - ref| <= bound
    (one `RATIO <what> rgb .. alpha .. depth ..` line); exact where the bound is zero; the count of interleaved pixels is the
    reference's (an undecidable pixel may differ)."""
    und = ref["undecidable"]
    n = len(und)
    assert und.sum() <= MAX_UNDECIDABLE * n, (what, "undecidable pixels", int(und.sum()), n)
    ok = ~und
    worst = {}
    for key, b in (("rgb", "b_rgb"), ("alpha", "b_alpha"), ("depth", "b_depth")):
        g, r, bound = np.asarray(got[key], np.float64)[ok], ref[key][ok], ref[b][ok]
        fin = np.isfinite(r)
        assert np.isfinite(g[fin]).all(), (what, key, "non-finite output")
        g, r, bound = g[fin], r[fin], bound[fin]
        err = np.abs(g - r)
        zero = bound == 0
        assert (err[zero] == 0).all(), (what, key, "differs where the bound is zero", float(err[zero].max()) if zero.any() else 0)
        ratio = err[~zero] / bound[~zero]
        worst[key] = float(ratio.max()) if ratio.size else 0.0
    report("RATIO %-60s rgb %.3f alpha %.3f depth %.3f" % (what, worst["rgb"], worst["alpha"], worst["depth"]))
    assert max(worst.values()) <= 1.0, (what, "error / bound", worst)
    lo = int(ref["interleaved_mask"][ok].sum())
    assert lo <= int(got["interleaved"]) <= lo + int(und.sum()), (what, "interleaved", int(got["interleaved"]), ref["interleaved"])
    return worst


def differs(emu, ref):
    """whether an emulation's result lies beyond the reference's bound at some decidable pixel, or counts other interleaved pixels"""
    ok = ~ref["undecidable"]
    far = False
    for key, b in (("rgb", "b_rgb"), ("alpha", "b_alpha"), ("depth", "b_depth")):
        with np.errstate(invalid="ignore"):
            far |= bool((np.abs(np.asarray(emu[key], np.float64)[ok] - ref[key][ok]) > ref[b][ok]).any())
    return far
