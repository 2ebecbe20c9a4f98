"""tests/step_io_refs.py on the CPU: `adam_ref` equals torch's CPU Adam at five beta pairs (moments bit for bit) and oracle.adam_step at the
shipped one, the data references equal oracle/data_oracle.py (itself pinned to the reference's Python by tests/golden) on the scene of
tests/test_gpu_data.py, the conditions that keep the GPU comparisons from passing vacuously hold on the references alone, and every seeded
mutant fails on the case tables that tests/test_gpu_step_io_kernels.py runs."""
import numpy as np
import pytest
import torch

import step_io_refs as sr

F = np.float32


# ---- A ---------------------------------------------------------------------------------------------------------------
def test_fma32_is_one_rounding_where_the_float64_sum_is_a_float32_tie():
    # x y = 2^-24 - 2^-70; c = 1 + 2^-23 (odd): the exact sum lies just below the tie and rounds DOWN; its float64 rounding is the tie itself
    # and would go to even, i.e. up
    x, y, c = F(2.0 ** -12 * (1 + 2.0 ** -23)), F(2.0 ** -12 * (1 - 2.0 ** -23)), F(1 + 2.0 ** -23)
    naive = F(np.float64(x) * np.float64(y) + np.float64(c))
    assert naive == F(1 + 2.0 ** -22) and sr.fma32(x, y, c) == c and sr.fma32(-x, y, -c) == -c
    assert sr.fma32(x, y, F(1)) == F(1)                                       # (an even neighbour: both agree)
    # just above a tie: x y = 2^-24 + 2^-46 + 2^-70 is kept by the float64 sum, no tie
    assert sr.fma32(x, x, F(1)) == F(1 + 2.0 ** -23)
    # the tie at the top of the range: exact sum below FLT_MAX + half an ulp stays finite
    big_x, big_y = F(2.0 ** 52 * (1 + 2.0 ** -23)), F(2.0 ** 51 * (1 - 2.0 ** -23))
    assert np.isinf(F(np.float64(big_x) * np.float64(big_y) + np.float64(sr.FLT_MAX))) and sr.fma32(big_x, big_y, sr.FLT_MAX) == sr.FLT_MAX
    assert np.isinf(sr.fma32(F(2.0 ** 52), F(2.0 ** 51), sr.FLT_MAX))          # the tie itself: to even, which is inf
    # arrays, and agreement with the plain double rounding off the ties
    rs = np.random.RandomState(0)
    a, b, c3 = (rs.randn(3, 20000) * 10.0 ** rs.uniform(-5, 5, (3, 20000))).astype(F)
    a[:3], b[:3], c3[:3] = [x, x, -x], [y, x, y], [c, 1, -c]
    got = sr.fma32(a, b, c3)
    plain = (a.astype(np.float64) * b.astype(np.float64) + c3.astype(np.float64)).astype(F)
    assert got[:3].tolist() == [c, F(1 + 2.0 ** -23), -c] and np.array_equal(got[3:], plain[3:])


def _torch_run(betas, numels, lrs, n_steps, seed=0):
    rs = np.random.RandomState(seed)
    P = [torch.nn.Parameter(torch.as_tensor(rs.randn(n).astype(F) * 0.1)) for n in numels]
    opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, lr in zip(P, lrs)], betas=betas, eps=1e-15)
    state = [dict(p=q.detach().numpy().copy(), p0=q.detach().numpy().copy(), m=np.zeros(n, F), v=np.zeros(n, F), step=F(0), beta1=betas[0], beta2=betas[1], eps=1e-15, lr=lr, shadow=None)
             for q, n, lr in zip(P, numels, lrs)]
    grads = []
    for k in range(n_steps):
        g = [(rs.randn(n) * 10.0 ** rs.uniform(-7, 0)).astype(F) for n in numels]     # scaled as in test_adam_oracle_matches_torch_adam_...
        for a in g:
            a[::5] = 0
        grads.append(g)
        for q, a, t in zip(P, g, state):
            q.grad = torch.as_tensor(a.copy())
            t["g"] = a.copy()
        opt.step()
        assert sr.adam_ref(state) is False
    return P, opt, state, grads


@pytest.mark.parametrize("betas", sr.ADAM_BETAS)
def test_adam_ref_equals_torch_cpu_adam(betas, oracle):
    n_steps, numels, lrs = 8, (5, 40003), (1e-2, 1e-5)
    P, opt, state, grads = _torch_run(betas, numels, lrs, n_steps)
    differ = []
    for q, t, lr in zip(P, state, lrs):
        assert float(opt.state[q]["step"]) == float(t["step"]) == n_steps
        assert np.array_equal(sr.bits(opt.state[q]["exp_avg"].numpy()), sr.bits(t["m"])), betas
        assert np.array_equal(sr.bits(opt.state[q]["exp_avg_sq"].numpy()), sr.bits(t["v"])), betas
        a = t["p"]
        d = np.abs(q.detach().numpy() - a)       # torch's Sleef sqrt is not correctly rounded: the allowance of test_adam_oracle_matches_torch_adam_...
        assert (d <= n_steps * lr * 2.4e-7 + 1.2e-7 * np.abs(a)).all(), float(d.max())
        differ.append(d > 0)
    assert np.concatenate(differ).mean() < 0.02, float(np.concatenate(differ).mean())      # (a fraction: over both tensors, one has 5 elements)
    # oracle.adam_step (numpy, plain double rounding in its FMA) is the same function: bit-equal at the shipped betas, and at the others too
    p = [t["p0"].copy() for t in state]
    st = [dict(step=0.0, exp_avg=np.zeros(n, F), exp_avg_sq=np.zeros(n, F)) for n in numels]
    for g in grads:
        assert oracle.adam_step(p, [a.copy() for a in g], st, list(lrs), betas=betas) is False
    for a, s, t in zip(p, st, state):
        assert np.array_equal(sr.bits(a), sr.bits(t["p"])) and np.array_equal(sr.bits(s["exp_avg"]), sr.bits(t["m"])) \
            and np.array_equal(sr.bits(s["exp_avg_sq"]), sr.bits(t["v"])), betas


def test_the_small_weight_lerp_form_leaves_torch_at_beta1_up_to_a_half():
    """what the kernel computed before: fma(g - m, 1 - beta1, m) whatever the weight"""
    for betas in sr.ADAM_BETAS:
        P, opt, state, grads = _torch_run(betas, (4099,), (1e-2,), 5)
        mut = [dict(p=state[0]["p"] * 0, m=np.zeros(4099, F), v=np.zeros(4099, F), step=F(0), beta1=betas[0], beta2=betas[1], eps=1e-15, lr=1e-2, shadow=None)]
        for g in grads:
            mut[0]["g"] = g[0].copy()
            sr.adam_ref(mut, mutant="lerp_small_form_only")
        n_diff = int((sr.bits(mut[0]["m"]) != sr.bits(opt.state[P[0]]["exp_avg"].numpy())).sum())
        print("beta1 %g: the small-weight form differs from torch in %d of 4099 exp_avg elements after 5 steps" % (betas[0], n_diff))
        assert (n_diff > 0) == (F(1 - betas[0]) >= F(0.5)), (betas, n_diff)


@pytest.fixture(scope="module")
def adam_table():
    plans = sr.adam_plans()
    return plans, [sr.adam_run_ref(p) for p in plans]


def test_adam_case_table_holds_what_the_gpu_test_relies_on(adam_table):
    plans, refs = adam_table
    assert [p["numels"] for p in plans[:len(sr.adam_groupings())]] == sr.adam_groupings()
    assert sum(len(p["numels"]) == 8 for p in plans) >= 3 and {n for p in plans for n in p["numels"]} >= set(sr.ADAM_NUMELS)
    seen = dict(v_inf=False, shadow_ragged=False, shadow_none=False, lr0=False, lr_dev=False, lr_double=False, step_1e6=False, betas=set(), flags=set(),
                zero_on_skip=False, kept_on_skip=False, bad_values=set(), denormal_m=False)
    for plan, ref in zip(plans, refs):
        assert [s["found"] for s in ref] == [st["expect_skip"] for st in plan["steps"]], plan["numels"]
        for k, (st, snap) in enumerate(zip(plan["steps"], ref)):
            for i, t in enumerate(plan["tensors"]):
                for key in ("p", "m", "v"):
                    assert not np.isnan(snap[key][i]).any(), (plan["numels"], k, key)      # no NaN: bits are comparable everywhere
                if snap["found"]:
                    prev = ref[k - 1]
                    assert all(np.array_equal(sr.bits(snap[key][i]), sr.bits(prev[key][i])) for key in ("p", "m", "v")) and snap["step"] == prev["step"]
                    assert (snap["g"][i] == 0).all() if st["zero_grad"] else np.array_equal(sr.bits(snap["g"][i]), sr.bits(st["g"][i]))
                    seen["zero_on_skip" if st["zero_grad"] else "kept_on_skip"] = True
                elif k > 0:
                    assert snap["step"][i] == ref[k - 1]["step"][i] + 1
                seen["v_inf"] |= bool(np.isinf(snap["v"][i]).any())
                seen["denormal_m"] |= bool(((snap["m"][i] != 0) & (np.abs(snap["m"][i]) < np.finfo(F).tiny)).any())
            seen["flags"].add("NULL" if st["skip_in"] is None else repr(float(st["skip_in"])))
        # FLT_MAX and denormal gradients are finite: step 1 is not skipped
        assert any(a.max() == sr.FLT_MAX for a in plan["steps"][1]["g"] if a.size >= 5) or max(plan["numels"]) < 5
        assert not ref[1]["found"] and ref[2]["found"] and not ref[3]["found"]
        t_bad, e_bad = plan["bad"]
        seen["bad_values"].add(int(sr.bits(plan["steps"][2]["g"][t_bad])[e_bad]))
        assert int(sum(sr.non_finite(a).sum() for a in plan["steps"][2]["g"])) == 1
        for t in plan["tensors"]:
            seen["shadow_ragged"] |= t["has_shadow"] and t["numel"] % 4 != 0
            seen["shadow_none"] |= not t["has_shadow"]
            seen["lr0"] |= t["lr0"] == 0
            seen["lr_dev"] |= t["lr_dev"]
            seen["lr_double"] |= not t["lr_dev"]
            seen["step_1e6"] |= t["step0"] == F(1e6)
            seen["betas"].add((t["beta1"], t["beta2"]))
        assert len({(t["beta1"], t["beta2"]) for t in plan["tensors"]}) == min(len(plan["tensors"]), len(sr.ADAM_BETAS))    # mixed within one call
    assert seen["betas"] == set(sr.ADAM_BETAS) and seen["flags"] == {"NULL", "0.0", "-0.0", "2.0", "nan"}, seen
    assert seen["bad_values"] == {int(v) for v in sr.ADAM_BAD_VALUES}, seen
    assert all(v for k, v in seen.items()), seen
    # a step counter of 1e6: both bias corrections are exactly 1
    assert 1 - 0.9 ** 1000001.0 == 1.0 and 1 - 0.999 ** 1000001.0 == 1.0
    print("adam case table: %d plans; float64 sums on a float32 tie %d, moved by the exact value %d" % (len(plans), sr.FMA_TIES[0], sr.FMA_TIES[1]))


def test_every_adam_mutant_fails_on_the_case_table(adam_table):
    plans, refs = adam_table
    where = {tuple(x[:3]): i for i, x in enumerate([(p["numels"],) + tuple(p["bad"]) for p in plans]) if i >= len(sr.adam_groupings())}
    killed = {m: [i for i, (p, r) in enumerate(zip(plans, refs)) if not sr.adam_snapshots_equal(sr.adam_run_ref(p, m), r)] for m in sr.ADAM_MUTANTS}
    print({m: len(v) for m, v in killed.items()})
    assert all(killed[m] for m in sr.ADAM_MUTANTS)
    n = len(plans)
    assert len(killed["skip_advances_step"]) == n and len(killed["flag_not_cleared"]) == n
    # the small-weight form: every plan with a tensor at beta1 <= 0.5 and more than a handful of elements
    big = [i for i, p in enumerate(plans) if any(F(1 - t["beta1"]) >= F(0.5) and t["numel"] > 1000 for t in p["tensors"])]
    assert len(big) > 8 and set(big) <= set(killed["lerp_small_form_only"])
    tails = [where[k] for k in (((4097, 4096), 0, 4096), ((4095,), 0, 4094), ((3,), 0, 2), ((3 * 4096 + 2, 4), 0, 3 * 4096 + 1))]
    assert set(tails) <= set(killed["check_without_tail"])
    fourth = [where[k] for k in (((4096, 5), 0, 3 * 1024 + 3), ((8191,), 0, 3 * 1024 + 1020), ((8193,), 0, 4096 + 3 * 1024 + 1023))]
    assert set(fourth) <= set(killed["check_without_fourth_quad"])
    later = [where[k] for k in (((5, 1, 4096), 1, 0), ((1, 3, 4, 5, 4095, 4097, 4096, 8191), 7, 8190))]
    assert set(later) <= set(killed["check_first_tensor_only"])
    # and nothing but the position decides there: the same plans pass with the element at index 0 of the first tensor
    first = where[((4097,), 0, 0)]
    assert all(first not in killed[m] for m in ("check_without_tail", "check_without_fourth_quad", "check_first_tensor_only"))


# ---- the data references against oracle/data_oracle.py ------------------------------------------------------------------
def _scene(H=135, W=120, N=3, seed=0):
    """the scene of tests/test_gpu_data.py"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.stack([(((yy - H * 0.55) / (H * 0.33)) ** 2 + ((xx - W * (0.45 + 0.03 * i)) / (W * 0.18)) ** 2 < 1).astype(F) for i in range(N)])
    masks[:, 10:14, 5:9] = 1.0
    imgs = rng.randint(0, 256, (N, H, W, 3)).astype(np.uint8)
    K = np.array([[2000.0 * H / 1080, 0, W / 2], [0, 2000.0 * H / 1080, H / 2], [0, 0, 1]])
    a = 0.3
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    c2w[:3, 3] = [0.1, -0.2, 0.3]
    smpl = dict(betas=rng.randn(1, 10).astype(F), body_pose=rng.randn(N, 69).astype(F) * 0.1,
                global_orient=rng.randn(N, 3).astype(F) * 0.1, transl=(rng.randn(N, 3) * 0.1 + [0, 0.15, 5]).astype(F))
    return imgs, masks, K, c2w, smpl


@pytest.fixture(scope="module")
def scene():
    return _scene()


@pytest.fixture(scope="module")
def scene_band(scene):
    col = scene[1][1].reshape(-1, 1)
    return sr.edge_band_ref(col, 16)


def test_morphology_refs_equal_the_data_oracle(scene, scene_band):
    from oracle import data_oracle as do
    masks = scene[1]
    col = masks[1].reshape(-1, 1)
    assert np.array_equal(sr.bits(scene_band), sr.bits(do.dilate(col, 16) - do.erode(col, 16))) and (scene_band != 0).sum() > 1000
    crop = masks[0][25:100, 15:85]                                            # the blob's outline and its inside
    rs = np.random.RandomState(5)
    for m in (crop, (crop * rs.rand(*crop.shape)).astype(F)):
        for k in (8, 5):
            assert np.array_equal(sr.bits(sr.dilate_ref(m, k)), sr.bits(do.dilate(m, k))), k
            assert np.array_equal(sr.bits(sr.erode_ref(m, k)), sr.bits(do.erode(m, k))), k


def test_edge_sampler_indices_from_the_refs_equal_the_data_oracle(scene, scene_band):
    from oracle import data_oracle as do
    mask = scene[1][1]
    N = mask.size
    draws = np.random.RandomState(2).rand(4096).astype(F)
    n_mask, n_edge = int(4096 * 0.6), int(4096 * 0.3)
    n_rand = 4096 - n_mask - n_edge
    r_m, c_m, _ = sr.nonzero_select_ref(mask.reshape(N, 1), (0, N, 0, 1), draws[:n_mask])
    r_e, c_e, _ = sr.nonzero_select_ref(scene_band.reshape(N, 1), (0, N, 0, 1), draws[n_mask:n_mask + n_edge])
    got = sr.edge_indices_ref(r_m, c_m, r_e, c_e, draws, n_mask, n_edge, n_rand, N, 1)
    assert np.array_equal(got, do.edge_sampler_indices(mask, draws, 4096, 0.6, 0.3, 16))
    # the 2-D geometry gives the same flat indices from (row, col) picks
    rows, cols, _ = sr.nonzero_select_ref(mask, (0, mask.shape[0], 0, mask.shape[1]), draws[:n_mask])
    assert np.array_equal(rows.astype(np.int64) * mask.shape[1] + cols, got[:n_mask])


def test_patch_corners_from_the_refs_equal_the_data_oracle(scene):
    from oracle import data_oracle as do
    mask = scene[1][0]
    H, W = mask.shape
    rng = np.random.RandomState(3)
    for coin, ratio in ((0.1, 1.0), (0.95, 0.9), (0.5, 0.9), (0.9, 0.9)):
        for P, n in ((32, 4), (16, 7)):
            draws = np.r_[coin, rng.rand(2 * n)].astype(F)
            o = P // 2
            rm, cm, _ = sr.nonzero_select_ref(mask, (o, H - o, o, W - o), draws[1:1 + n], without_replacement=True)
            rows, cols = sr.patch_corners_ref(rm, cm, draws, n, H, W, P, ratio)
            x, y = do.patch_sampler_corners(mask, draws, n, P, ratio)
            assert np.array_equal(rows, x) and np.array_equal(cols, y), (coin, ratio, P)


def test_sample_batch_near_far_and_rays_equal_the_data_oracle(scene):
    from oracle import data_oracle as do
    imgs, masks, K, c2w, smpl = scene
    H, W = masks.shape[1:]
    rng = np.random.RandomState(4)
    ro, rd = do.make_rays(K, c2w, H, W)
    o64, d64 = sr.make_rays_ref(np.linalg.inv(K), c2w[:3, :3], c2w[:3, 3], H, W)
    assert np.array_equal(o64.astype(F), ro.reshape(-1, 3)) and np.abs(d64.astype(F) - rd.reshape(-1, 3)).max() <= sr.RAY_ULP
    assert np.abs(d64 - rd.reshape(-1, 3)).max() <= 2.0 ** -24 * 1.0001          # the oracle's float32 is the rounding of the float64 value
    idx = 2
    draws = rng.rand(1024).astype(F)
    fn = lambda msk, *args: do.edge_sampler_sample(msk, args, draws, num_sample=1024, ratio_mask=0.6, ratio_edge=0.3, kernel_size=16)
    bg_full = rng.rand(H, W, 3).astype(F)
    ref = do.getitem_train(imgs[idx], masks[idx], ro, rd, smpl, idx, fn, bg_full)
    pix = do.edge_sampler_indices(masks[idx], draws, 1024, 0.6, 0.3, 16)
    # a fractional mask as a resized one would be: the same comparison must hold there (the oracle is numpy's own evaluation)
    for mask in (masks[idx], (masks[idx] * rng.rand(H, W)).astype(F)):
        if mask is not masks[idx]:
            ref = do.getitem_train(imgs[idx], mask, ro, rd, smpl, idx, lambda msk, *args: [np.asarray(a).reshape(H * W, -1)[pix] for a in (msk, *args)], bg_full)
            ref["alpha"] = ref["alpha"][:, 0]
        frame = dict(u8=imgs[idx].reshape(-1, 3), img_f=None, mask=mask.reshape(-1), rays_o=ro.reshape(-1, 3), rays_d=rd.reshape(-1, 3))
        rgb, alpha, o, d, bg, idx_out = sr.sample_batch_ref(frame, W, flat_idx=pix, bg=bg_full.reshape(-1, 3)[pix])
        assert np.array_equal(sr.bits(rgb), sr.bits(ref["rgb"])) and np.array_equal(alpha, ref["alpha"]) and np.array_equal(bg, ref["bg_color"])
        assert np.array_equal(o, ref["rays_o"]) and np.array_equal(d, ref["rays_d"]) and np.array_equal(idx_out, pix)
    near, far = sr.near_far_ref(smpl["transl"][idx])
    assert near == ref["near"][0] and far == ref["far"][0] and (ref["near"] == near).all()
    # white background (the evaluation split) and the patch route against plain slicing
    ev = do.getitem_eval(imgs[idx], masks[idx], ro, rd, smpl, idx)
    frame = dict(u8=imgs[idx].reshape(-1, 3), img_f=None, mask=masks[idx].reshape(-1), rays_o=ro.reshape(-1, 3), rays_d=rd.reshape(-1, 3))
    rgb = sr.sample_batch_ref(frame, W, flat_idx=np.arange(H * W))[0]
    assert np.array_equal(sr.bits(rgb), sr.bits(ev["rgb"]))
    rows, cols = np.array([0, H - 16, 40]), np.array([W - 16, 0, 33])
    got = sr.sample_batch_ref(frame, W, corners=(rows, cols), patch=16)
    want = np.stack([ev["rgb"].reshape(H, W, 3)[r:r + 16, c:c + 16] for r, c in zip(rows, cols)]).reshape(-1, 3)
    assert np.array_equal(sr.bits(got[0]), sr.bits(want))
    assert np.array_equal(got[5].reshape(3, 16, 16)[1, 2], (H - 16 + 2) * W + np.arange(16))


# ---- mutants of the data side ---------------------------------------------------------------------------------------------
def test_select_case_table_rejects_thresholds_instead_of_nonzero():
    killed = {m: 0 for m in ("gt_half", "gt_zero")}
    n_windows = 0
    for rows, cols in sr.SELECT_WINDOWS:
        for fi, frame in enumerate(sr.select_frames(rows, cols)):
            H, W, y0, y1, x0, x1 = frame
            assert (H, W) == (rows, cols) or (x0 % 64 and y0 % 64)
            mask = sr.select_mask(frame, "mixed", rows * 7 + cols + fi)
            win = mask[y0:y1, x0:x1]
            r, c, count = sr.nonzero_select_ref(mask, (y0, y1, x0, x1), sr.select_draws(0, 8, 0))
            assert count == int((win != 0).sum())
            if rows >= 3:
                assert not win[0].any() and not win[-1].any() and np.signbit(win[win == 0]).any() and count > 0
            if rows >= 5:
                assert not win[rows // 2].any() and win[:rows // 2].any() and win[rows // 2:].any()
            if count == 0:
                continue
            n_windows += 1
            u = sr.select_draws(count, 500, rows + cols)
            assert {0.0, 0.5, float(sr.ONE_BELOW), 1.0} <= set(u.tolist()) and len(u) >= 500
            ref = sr.nonzero_select_ref(mask, (y0, y1, x0, x1), u)
            rank = np.minimum(np.floor(u * F(count)).astype(np.int64), count - 1)
            assert set(rank.tolist()) == set(range(count))                                   # every rank is drawn
            rr, cc = np.nonzero(win != 0)
            assert np.array_equal(ref[0], rr[rank]) and np.array_equal(ref[1], cc[rank])
            for m in killed:
                got = sr.nonzero_select_ref(mask, (y0, y1, x0, x1), u, mutant=m)
                killed[m] += int(got[2] != count or not np.array_equal(got[0], ref[0]) or not np.array_equal(got[1], ref[1]))
    print("select windows with candidates: %d, thresholds rejected on %s" % (n_windows, killed))
    assert n_windows >= 14 and all(v >= n_windows - 4 for v in killed.values())     # (a window of one or two cells may hold only 1.0)
    # each special value on its own
    for val, kills in ((F(-1.0), {"gt_half", "gt_zero"}), (F(1e-40), {"gt_half"}), (F(0.25), {"gt_half"}), (F(np.nan), {"gt_half", "gt_zero"}), (F(-0.0), set())):
        one = np.zeros((1, 3), F)
        one[0, 1] = val
        count = sr.nonzero_select_ref(one, (0, 1, 0, 3), [0.5])[2]
        assert count == (0 if val == 0 else 1)
        assert {m for m in killed if sr.nonzero_select_ref(one, (0, 1, 0, 3), [0.5], mutant=m)[2] != count} == kills, val


def test_without_replacement_cases_need_the_fixed_point():
    for name, frame, count, u in sr.without_replacement_cases():
        H, W, y0, y1, x0, x1 = frame
        mask = sr.select_mask(frame, "count", 3, count=count)
        rows, cols, c = sr.nonzero_select_ref(mask, (y0, y1, x0, x1), u, without_replacement=True)
        assert c == count and len(u) <= sr.MAX_DRAWS_WITHOUT_REPLACEMENT
        n_valid = min(len(u), count)
        picks = list(zip(rows[:n_valid].tolist(), cols[:n_valid].tolist()))
        assert len(set(picks)) == n_valid and all(mask[y0 + r, x0 + c] != 0 for r, c in picks), name
        assert (rows[n_valid:] == -1).all() and (cols[n_valid:] == -1).all()
        if n_valid == count:
            assert len(set(picks)) == count                                                    # every candidate exactly once
        mut = sr.nonzero_select_ref(mask, (y0, y1, x0, x1), u, without_replacement=True, mutant="no_fixed_point")
        # (always taking the last of what is left needs no correction: nothing chosen lies below it)
        assert (np.array_equal(mut[0], rows) and np.array_equal(mut[1], cols)) == ("just below 1" in name), name
    assert any(len(u) == 256 for _, _, _, u in sr.without_replacement_cases())


def test_morph_case_table_rejects_the_symmetric_window_and_a_zero_border():
    killed = {m: set() for m in sr.MORPH_MUTANTS}
    for H, W, k in sr.MORPH_CASES:
        for name, m in sr.morph_masks(H, W).items():
            if name == "blobs":
                assert set(np.unique(m).tolist()) <= {0.0, 0.25, 0.5, 1.0}
                if H * W > 1:
                    assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()    # touches every border
            ref_d, ref_e = sr.dilate_ref(m, k), sr.erode_ref(m, k)
            assert np.array_equal(sr.bits(sr.edge_band_ref(m, k)), sr.bits(ref_d - ref_e)) and (ref_d >= m).all() and (ref_e <= m).all()
            if k == 1:
                assert np.array_equal(ref_d, m) and np.array_equal(ref_e, m)
            for mut in sr.MORPH_MUTANTS:
                if not (np.array_equal(sr.dilate_ref(m, k, mut), ref_d) and np.array_equal(sr.erode_ref(m, k, mut), ref_e)):
                    killed[mut].add((H, W, k, name))
    assert {c[:3] for c in killed["symmetric_window"]} == {c for c in sr.MORPH_CASES if c[2] % 2 == 0}      # every even k, no odd one
    assert {c[:3] for c in killed["zero_border"]} == {c for c in sr.MORPH_CASES if c[2] > 1}                 # erode at every border


def test_batch_case_table_rejects_a_contracted_blend():
    frame = sr.batch_frame()
    assert sorted(frame["u8"][:, 2].tolist()) == list(range(256)) and np.array_equal(frame["img_f"], (frame["u8"] / 255.0).astype(F))
    assert {0.0, 1.0, 0.25, float(F(1 / 3)), float(F(0.999))} <= set(frame["mask"].tolist()) and len(set(frame["mask"].tolist())) > 90
    rs = np.random.RandomState(0)
    n_diff = 0
    for n in sr.BATCH_FLAT_NS:
        idx = sr.batch_flat_indices(n)
        assert idx[0] == 255 and (n < 4 or (idx[1] == idx[2] == 0))
        bg = rs.rand(n, 3).astype(F)
        for b in (bg, None):
            ref = sr.sample_batch_ref(frame, sr.BATCH_W, flat_idx=idx, bg=b)
            assert np.array_equal(sr.bits(ref[0]), sr.bits(sr.sample_batch_ref(frame, sr.BATCH_W, flat_idx=idx, bg=b, use_float_image=True)[0]))
            mut = sr.sample_batch_ref(frame, sr.BATCH_W, flat_idx=idx, bg=b, mutant="fma")
            n_diff += int((sr.bits(mut[0]) != sr.bits(ref[0])).sum())
            binary = frame["mask"][idx][:, None] * np.ones(3, F) == np.round(frame["mask"][idx][:, None] * np.ones(3, F))
            assert np.array_equal(sr.bits(mut[0])[binary], sr.bits(ref[0])[binary])          # a 0/1 mask cannot tell them apart
    assert n_diff > 50, n_diff
    for patch, n_patch in sr.BATCH_PATCHES:
        rows, cols = sr.batch_corners(patch, n_patch)
        assert (rows[0], cols[0]) == (sr.BATCH_H - patch, sr.BATCH_W - patch) and (n_patch == 1 or (rows[1], cols[1]) == (0, 0))
        idx = sr.sample_batch_ref(frame, sr.BATCH_W, corners=(rows, cols), patch=patch)[5]
        assert len(idx) == n_patch * patch * patch and idx.max() == 255 and idx.min() >= 0


def test_corner_and_index_case_tables_reject_their_mutants():
    killed = {m: 0 for m in sr.CORNER_MUTANTS}
    cases = sr.corner_cases()
    for name, H, W, P, ratio, n, draws, rm, cm in cases:
        rows, cols = sr.patch_corners_ref(rm, cm, draws, n, H, W, P, ratio)
        assert (rows >= 0).all() and (rows < H - P).all() and (cols >= 0).all() and (cols < W - P).all(), name
        for m in killed:
            got = sr.patch_corners_ref(rm, cm, draws, n, H, W, P, ratio, mutant=m)
            k = not (np.array_equal(got[0], rows) and np.array_equal(got[1], cols))
            killed[m] += int(k)
            if m == "coin_le" and n > 1:
                assert k == name.startswith(("coin == ratio", "coin 0, ratio 0")), name
            if m == "clamp_h_minus_p" and n > 3 and not (draws[0] < F(ratio)):
                assert k, name                                                                 # the uniform branch with a draw of exactly 1
    assert all(v > 0 for v in killed.values()), killed
    assert any(H - P == 1 for _, H, W, P, *_ in cases) and {c[5] for c in cases} == set(sr.CORNER_NS)
    # u < 1 never rounds u * count up to count (why the clamp needs the draw 1.0 to be seen at all)
    for count in (1, 2, 3, 17, 24, 41, 292, 16200, 2 ** 24 - 1, 2 ** 24):
        assert np.floor(sr.ONE_BELOW * F(count)) == count - 1
    for name, H, W, nm, ne, nr, draws, r_m, c_m, r_e, c_e in sr.edge_index_cases():
        out = sr.edge_indices_ref(r_m, c_m, r_e, c_e, draws, nm, ne, nr, H, W)
        assert len(out) == nm + ne + nr and out.min() >= 0 and out.max() < H * W, name
        if nm > 4:
            assert out[0] == min(int(np.floor(draws[0] * F(H * W))), H * W - 1) and out[1] == r_m[1] * W + c_m[1]    # a -1 pick uses its own draw
    # 2^24 pixels: the last one is reached, never the one behind it
    top = sr.edge_indices_ref(None, None, None, None, np.array([sr.ONE_BELOW, 0, 0.5], F), 0, 0, 3, 4096, 4096)
    assert top.tolist() == [2 ** 24 - 1, 0, 2 ** 23]
    for t in sr.NEAR_FAR_TRANSL:
        near, far = sr.near_far_ref(t)
        assert abs(float(near) + 1 - np.sqrt(sum(float(F(v)) ** 2 for v in t))) < 1e-6 * max(1, float(far)) and abs(float(far) - float(near) - 2) < 1e-6
    assert sr.near_far_ref((0, 0, 0)) == (F(-1), F(1)) and sr.near_far_ref((3, 4, 12)) == (F(12), F(14))


def test_ray_cameras_are_general():
    for H, W in sr.RAY_SHAPES:
        K, R, t = sr.ray_camera(H, W)
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14 and np.abs(R - np.eye(3)).min() > 0.01
        assert abs(K[0, 2] - W / 2) > 0.1 and abs(K[1, 2] - H / 2) > 0.1
        o, d = sr.make_rays_ref(np.linalg.inv(K), R, t, H, W)
        assert o.shape == d.shape == (H * W, 3) and np.allclose((d * d).sum(1), 1, atol=1e-14) and (o == t).all()
