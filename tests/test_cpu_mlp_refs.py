"""Pins tests/mlp_refs.py itself (no GPU): the lattice builders meet their two exactness conditions at every case size; a
plain host emulation of the kernels' arithmetic (numpy fp32 matmul over half operands, np.float16 at the rounding points,
weight gradients summed in two orders) attains every bound tests/test_gpu_mlp_kernels.py applies; six deliberate mutants of
that emulation do not; and with the rounding points switched off the backward reference is torch float64 autograd of the
plain MLP."""
import numpy as np
import pytest
import torch

import mlp_refs as mr


def _ratio(got, ref, bound, what, expect_fail=False):
    """worst |got - ref| / bound; where the bound is 0 the value must be exactly the reference's"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    z = bound == 0
    r = float((err[~z] / bound[~z]).max()) if (~z).any() else 0.0
    if (err[z] != 0).any():
        r = np.inf
    if not expect_fail:
        print("RATIO cpu-fp32 %-44s %.3f" % (what, r))
        assert r <= 1.0, (what, r)
    return r


# ---- the host emulation of k_field_bwd's arithmetic and its mutants --------------------------------------------------
MUTANTS = ("slots_not_shifted", "c1_mask_from_c2", "sigma_not_inserted", "last_sample_dropped", "c3_blocks_swapped", "no_inv_scale")
PREFILL = 7.0


def bwd_emul(inp, order="matmul", mutant=None):
    """-> dict(dfeat [V, 2L] with the prefill in the rows that are not written, g_w1 .. g_c3)"""
    f32 = lambda a: np.asarray(a).astype(np.float32)
    h = lambda a: a.astype(np.float16).astype(np.float32)
    V = len(inp["acts"])
    n = V if inp["n_live"] is None else min(V, inp["n_live"])
    if mutant == "last_sample_dropped":
        assert n % 32 != 0
        n -= 1
    rec = {k: v.astype(np.float32) for k, v in mr.split_record(inp["acts"][:n]).items()}
    W = {k: f32(inp[k]) for k in mr.WEIGHT_NAMES}
    S = np.float32(inp["S"])
    invS = np.float32(1) if mutant == "no_inv_scale" else np.float32(1) / S
    y, g = f32(inp["rgb"])[:n], f32(inp["d_rgb"])[:n]
    dY = np.zeros((n, 16), np.float32)
    dY[:, :3] = h(((g * y) * (np.float32(1) - y)) * S)
    dC2 = h(dY @ W["Wc3"]) * (rec["c2"] > 0)
    dC1 = h(dC2 @ W["Wc2"]) * ((rec["c2"] if mutant == "c1_mask_from_c2" else rec["c1"]) > 0)
    dCin = h(dC1 @ W["Wc1"])
    cin = mr.colour_input(rec["out"])
    dO = np.empty((n, 16), np.float32)
    if mutant == "slots_not_shifted":          # the constant in column 0: slot t reads column t
        dO[:, 1:] = dCin[:, 1:]
        cin = np.concatenate([cin[:, 15:], cin[:, :15]], 1)
    else:
        dO[:, 1:] = dCin[:, :15]
    dO[:, 0] = np.float32(0) if mutant == "sigma_not_inserted" else h(f32(inp["d_sigma"])[:n] * S)
    dH1 = h(dO @ W["W2"]) * (rec["h1"] > 0)
    out = dict(dfeat=np.full((V, W["W1"].shape[1]), PREFILL, np.float32))
    out["dfeat"][:n] = (dH1 @ W["W1"]) * invS
    for name, G, A in (("c3", dY, rec["c2"]), ("c2", dC2, rec["c1"]), ("c1", dC1, cin), ("w2", dO, rec["h1"]), ("w1", dH1, rec["feat"])):
        if order == "matmul":
            acc = G.T @ A
        else:                                   # tiles of 32 samples, last tile first, plain fp32 additions
            acc = np.zeros((G.shape[1], A.shape[1]), np.float32)
            for t in range((n + 31) // 32 - 1, -1, -1):
                acc = acc + G[32 * t:32 * t + 32].T @ A[32 * t:32 * t + 32]
        out["g_" + name] = acc * invS
    if mutant == "c3_blocks_swapped":
        out["g_c3"] = np.concatenate([out["g_c3"][:, 32:], out["g_c3"][:, :32]], 1)
    return out


def _compare(E, R, V, what, zero_bound, expect_fail=False):
    """worst ratio over dfeat and the five gradients (zero_bound: the lattice, everything exact)"""
    n = R["n"]
    full = np.full((V, R["dfeat"].shape[1]), PREFILL)
    full[:n] = R["dfeat"]
    b = np.zeros_like(full)
    if not zero_bound:
        b[:n] = R["b_dfeat"]
    worst = _ratio(E["dfeat"], full, b, what + " dfeat", expect_fail)
    for g in mr.GRADS:
        worst = max(worst, _ratio(E["g_" + g], R["g_" + g], np.zeros_like(R["b_" + g]) if zero_bound else R["b_" + g], what + " g_" + g, expect_fail))
    return worst


# ---- lattice ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_levels,V,n_live", mr.LATTICE_CASES)
def test_lattice_inputs_are_exact_and_the_emulation_equals_the_reference(n_levels, V, n_live):
    for S in mr.lattice_scales(V):
        inp, R = mr.lattice_inputs(n_levels, V, S, n_live)          # (asserts the two exactness conditions)
        assert R["n"] == (V if n_live is None else n_live)
        pre = mr.lattice_prefill(n_levels)
        for g in mr.GRADS:                                          # prefill + gradient is exact as well
            assert (np.abs(pre[g]).max() + R["M_" + g].max()) * S < 2 ** 24
            assert (R["g_" + g] == np.round(R["g_" + g] * S) / S).all()
        for order in ("matmul", "tiles"):
            assert _compare(bwd_emul(inp, order), R, V, "lattice L%d V%d S%g %s" % (n_levels, V, S, order), True) == 0.0
    assert mr.bwd_workspace_bytes(V, n_levels) == min(512, (V + 63) // 64) * (128 * n_levels + 7168) * 4


@pytest.mark.parametrize("mutant", MUTANTS)
def test_lattice_mutants_differ(mutant):
    for n_levels, V, n_live in ((8, 33, None), (16, 129, 100)):
        inp, R = mr.lattice_inputs(n_levels, V, 4.0, n_live)
        assert _compare(bwd_emul(inp, "tiles", mutant), R, V, mutant, True, expect_fail=True) > 1.0


# ---- real-valued -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[8, 16])
def real(request):
    inp = mr.host_real_inputs(request.param)
    R = mr.mlp_bwd_ref(**inp)
    mr.assert_real_case_is_hard(R)
    return request.param, inp, R


def test_plain_fp32_attains_the_backward_bounds(real):
    L, inp, R = real
    for order in ("matmul", "tiles"):
        _compare(bwd_emul(inp, order), R, mr.REAL_V, "real L%d %s" % (L, order), False)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_real_mutants_exceed_the_bounds(real, mutant):
    L, inp, R = real
    r = _compare(bwd_emul(inp, "matmul", mutant), R, mr.REAL_V, mutant, False, expect_fail=True)
    print("RATIO cpu-fp32 mutant L%d %-32s %.3g" % (L, mutant, r))
    assert r > 1.0, (mutant, r)


def test_plain_fp32_attains_the_forward_bounds():
    for L in (8, 16):
        W = mr.xavier_weights(L)
        rng = np.random.RandomState(1)
        acts, rgb, sigma = mr.mlp_fwd_emul(rng.uniform(-0.5, 0.5, (20011, 2 * L)), **W)
        rec = mr.split_record(acts)
        checks = mr.fwd_record_checks(acts, **W)
        for k in ("h1", "out", "c1", "c2"):
            ref, bound = checks[k]
            _ratio(rec[k], ref, bound, "forward L%d %s" % (L, k))
            assert (bound == 0).mean() > 0.75         # most elements are pinned bit for bit (`out`, with cancelling sums, the fewest)
        _ratio(rgb, *checks["rgb"], "forward L%d rgb" % L)
        assert (checks["rgb"][1] == 0).mean() > 0.9
        assert np.array_equal(sigma, rec["out"][:, 0].astype(np.float32))
        # teeth: the colour input without the shift, and a relu forgotten
        bad_c1 = np.maximum(np.concatenate([np.ones((len(acts), 1)), rec["out"][:, 1:]], 1) @ W["Wc1"].astype(np.float64).T, 0)
        assert _ratio(mr.rn16(bad_c1), *checks["c1"], "", expect_fail=True) > 1.0
        assert _ratio(mr.rn16(rec["c1"] @ W["Wc2"].astype(np.float64).T), *checks["c2"], "", expect_fail=True) > 1.0


# ---- the reference is the operation ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_levels", [8, 16])
def test_backward_reference_equals_autograd_without_the_rounding_points(n_levels):
    rng = np.random.RandomState(11 + n_levels)
    V, S = 257, 3.0
    W = {k: torch.tensor(v.astype(np.float64), requires_grad=True) for k, v in mr.xavier_weights(n_levels).items()}
    feat = torch.tensor(rng.uniform(-0.5, 0.5, (V, 2 * n_levels)), requires_grad=True)
    h1 = torch.relu(feat @ W["W1"].T)
    out = h1 @ W["W2"].T
    cin = torch.cat([out[:, 1:], torch.ones(V, 1, dtype=torch.float64)], 1)
    c1 = torch.relu(cin @ W["Wc1"].T)
    c2 = torch.relu(c1 @ W["Wc2"].T)
    rgb = torch.sigmoid((c2 @ W["Wc3"].T)[:, :3])
    d_rgb, d_sigma = rng.randn(V, 3), rng.randn(V)
    ((rgb * torch.tensor(d_rgb)).sum() + (out[:, 0] * torch.tensor(d_sigma)).sum()).backward()
    acts = np.concatenate([t.detach().numpy() for t in (feat, h1, out, c1, c2)], 1)
    R = mr.mlp_bwd_ref(acts, rgb.detach().numpy(), d_rgb, d_sigma, None, S, round16=False, **{k: v.detach().numpy() for k, v in W.items()})
    for got, want, what in ((R["dfeat"], feat.grad, "dfeat"), (R["g_w1"], W["W1"].grad, "W1"), (R["g_w2"], W["W2"].grad, "W2"),
                            (R["g_c1"], W["Wc1"].grad, "Wc1"), (R["g_c2"], W["Wc2"].grad, "Wc2")):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), what
    # Wc3: rows 0..2 produce rgb, the other 13 outputs are not read
    want = W["Wc3"].grad.numpy()
    assert np.abs(R["g_c3"] - want).max() <= 1e-12 * np.abs(want).max() and (R["g_c3"][3:] == 0).all()
    # a live count below V: the rows past it do not exist
    R2 = mr.mlp_bwd_ref(acts, rgb.detach().numpy(), d_rgb, d_sigma, 100, S, round16=False, **{k: v.detach().numpy() for k, v in W.items()})
    R3 = mr.mlp_bwd_ref(acts[:100], rgb.detach().numpy()[:100], d_rgb[:100], d_sigma[:100], None, S, round16=False,
                        **{k: v.detach().numpy() for k, v in W.items()})
    assert R2["n"] == 100 and all(np.array_equal(R2["g_" + g], R3["g_" + g]) for g in mr.GRADS)


# ---- grad scale ------------------------------------------------------------------------------------------------------
def test_grad_scale_reference():
    rgb, d_rgb, d_sigma = mr.grad_scale_inputs(300)
    assert mr.grad_scale_ref(rgb[:0], d_rgb[:0], d_sigma[:0], None) == mr.SCALE_EMPTY and np.isfinite(mr.SCALE_EMPTY)
    assert mr.grad_scale_ref(rgb, 0 * d_rgb, 0 * d_sigma, None) == mr.SCALE_EMPTY
    s = mr.grad_scale_ref(rgb, d_rgb, d_sigma, None)
    top = max(np.abs(d_rgb.astype(np.float64) * rgb * (1 - rgb)).max(), np.abs(d_sigma).max())
    assert abs(float(s) * top / 1024 - 1) < 1e-6
    big = d_sigma.copy()
    big[200] = 1e30
    assert mr.grad_scale_ref(rgb, d_rgb, big, 200) == mr.grad_scale_ref(rgb[:200], d_rgb[:200], d_sigma[:200], None)
    assert mr.grad_scale_ref(rgb, d_rgb, big, None) == np.float32(1024) / np.float32(1e30)
    for bad in (np.nan, np.inf, -np.inf):
        d = d_rgb.copy()
        d[17, 1] = bad
        assert np.isnan(mr.grad_scale_ref(rgb, d, d_sigma, None))
        assert mr.grad_scale_ref(rgb, d, d_sigma, 17) == mr.grad_scale_ref(rgb, d_rgb, d_sigma, 17)
