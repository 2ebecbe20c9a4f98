"""float64 restatements of the three fused-MLP entries (ia_field_bwd, ia_field_grad_scale, the activation record of
ia_field_fwd_train), their seeded input sets and the error bounds the GPU tests apply (numpy only: no GPU, no product import).
Same conventions as tests/backward_refs.py: every reference takes the arrays the C entry takes, sums come with a condition
magnitude M (the same expression with every term replaced by its absolute value), u = 2^-24 is the unit roundoff of fp32.

What is restated is the operation as include/instantavatar_hip.h documents it: five weight matrices fp16 [out][in]
(sig_w1 [64][2L], sig_w2 [16][64], col_w1 [64][16], col_w2 [64][64], col_w3 [16][64], no biases), the colour input
[out[1..15], 1] and the record [features 2L | h1 64 | out 16 | c1 64 | c2 64] per sample.  Nothing here knows how the
kernels lay the matrices out in registers.

Backward, rounding points (ia_field_bwd rounds every gradient it hands to the next layer to half, after multiplying the
incoming gradients by *scale = S; S is divided out of every fp32 result):
    dY   = rn16(fp32(((d_rgb y) (1 - y)) S))                     y = rgb, the fp32 operation order of the source
    dC2  = rn16(Wc3^T dY)  [c2 > 0]
    dC1  = rn16(Wc2^T dC2) [c1 > 0]
    dCin = rn16(Wc1^T dC1)
    dO   = [rn16(fp32(d_sigma S)), dCin[0..14]]                   (the gradient of the constant slot 15 is discarded)
    dH1  = rn16(W2^T dO)   [h1 > 0]
    dF   = (W1^T dH1) / S
    dW   = sum_n G A^T / S    (G, A) = (dY, c2), (dC2, c1), (dC1, [out[1..15], 1]), (dO, h1), (dH1, features)

Bound of the backward, by forward error propagation (`mlp_bwd_ref` returns it next to every value).  The masks are read
from the record, an input: no discontinuity.  dY and dO[0] are formed from fp32 inputs by the operations spelled above,
one rounding each (-ffp-contract=off): the reference forms them in numpy fp32 in the same order, so they carry no error.
A stage r = rn16(W^T g) then sees, per element,
    delta_pre = |W|^T delta_g  +  k u M          the incoming error; an fp32 sum of k exact products (half x half is exact
                                                 in fp32) in ANY order is within (k - 1) u M + O(u^2) of the true sum
    delta     = delta_pre + spacing16(|v| + delta_pre)   wherever delta_pre > 0, else 0
because |rn16(a) - rn16(b)| <= |a - b| + ulp16(a) / 2 + ulp16(b) / 2 <= |a - b| + ulp16(max(|a|, |b|)): a rounding may
flip to its neighbour, not farther.  spacing16 is 2^-24 below 2^-14 (the subnormal halves).  Where delta_pre = 0 (M = 0:
every product is zero) the stage is exact.  A closed mask makes value and error zero.
    dF:  |W1|^T delta_dH1 / S + (64 + 2) u M     64 terms, the rounding of 1 / S and of the product with it
    dW:  sum_n delta_G |A| / S + (n + 2) u M     n terms (n = live samples), 1 / S and the product with it; the caller's
                                                 g_* is zero in the real-valued case, so the final += is exact
On the lattice inputs every value is an integer that half and fp32 hold exactly (asserted by `lattice_inputs`), M = sum |.|
stays below 2^24 so every partial sum in any order is exact, and the bound is ZERO.

Forward, stage by stage from the kernel's own record (`fwd_stage`): r = rn16(relu(W a)) with a read back from the record.
The fp32 sum s of the kernel is within e = (k + 1) u M of the float64 value v.  Where v lies farther than e from every
rounding boundary of the half grid (the midpoints between neighbouring halves; for a relu stage also 0) s rounds to the same
half and the bound is ZERO; otherwise it is e + the spacing to the neighbour (one flip, as e is below the spacing except
next to the zero of a relu).  rgb = rn16(1 / (1 + expf(-s))): the HIP math API
documents expf at 1 ulp (2 u), the sum 1 + e and the correctly rounded division add u each, so the fp32 sigmoid is within
sigma (1 - sigma) e (1 + e) + 5 u sigma of the float64 one; the same boundary test is applied with that allowance.
"""
import numpy as np

U = 2.0 ** -24           # unit roundoff of fp32


def act_stride(n_levels):
    return 2 * n_levels + 208


def split_record(acts):
    """{feat, h1, out, c1, c2} (float64) of a record array fp16 [V, 2L + 208]"""
    a = np.asarray(acts)
    assert a.dtype in (np.float16, np.float64) and a.ndim == 2      # (float64: the unrounded operation, mlp_bwd_ref(round16=False))
    nf = a.shape[1] - 208
    assert nf in (16, 32)
    a = a.astype(np.float64)
    return dict(feat=a[:, :nf], h1=a[:, nf:nf + 64], out=a[:, nf + 64:nf + 80], c1=a[:, nf + 80:nf + 144], c2=a[:, nf + 144:nf + 208])


def join_record(feat, h1, out, c1, c2):
    return np.ascontiguousarray(np.concatenate([feat, h1, out, c1, c2], 1).astype(np.float16))


def colour_input(out):
    """[out[1..15], 1]"""
    return np.concatenate([out[:, 1:16], np.ones((len(out), 1), out.dtype)], 1)


def rn16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def spacing16(x):
    """spacing of the half grid at magnitude |x| (2^-24 in the subnormal range and at 0)"""
    x = np.ascontiguousarray(x, np.float64)
    e = ((x.view(np.int64) >> 52) & 0x7FF) - 1023              # |x| in [2^e, 2^(e+1)); halves below 2^-14 are 2^-24 apart
    return ((np.maximum(e, -14) - 10 + 1023) << 52).view(np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# ia_field_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _stage(G, dG, W, mask, round16):
    """r = rn16(W^T g) [mask] per sample (rows of G), W the forward matrix [k][m]; -> (r, delta, pre-rounding value, M)"""
    W = np.asarray(W, np.float64)
    v, M = G @ W, np.abs(G) @ np.abs(W)
    d = dG @ np.abs(W) + W.shape[0] * U * M
    if round16:
        r = rn16(v)
        d = np.where(d > 0, d + spacing16(np.abs(v) + d), 0.0)
    else:
        r = v
    if mask is not None:
        r, d, v = r * mask, d * mask, v * mask
    return r, d, v, M


def mlp_bwd_ref(acts, rgb, d_rgb, d_sigma, n_live, S, W1, W2, Wc1, Wc2, Wc3, round16=True):
    """The backward of both MLPs from the record (module docstring).  round16=False switches the half rounding points off
    (and forms dY in float64): the plain operation, for the comparison with autograd.  Returns the stages, their
    pre-rounding values ("pre"), dfeat [n, 2L] and the five gradients g_* with M_* and b_* (the bound), for the first
    n = min(V, n_live) samples."""
    V = len(acts)
    n = V if n_live is None else max(0, min(V, int(n_live)))
    rec = split_record(np.asarray(acts)[:n])
    S32 = np.float32(S)
    Sd = float(S32)
    if round16:
        y32, g32, s32 = np.asarray(rgb, np.float32)[:n], np.asarray(d_rgb, np.float32)[:n], np.asarray(d_sigma, np.float32)[:n]
        dy = rn16(((g32 * y32) * (np.float32(1) - y32)) * S32)
        go0 = rn16(s32 * S32)
    else:
        y = np.asarray(rgb, np.float64)[:n]
        dy = np.asarray(d_rgb, np.float64)[:n] * y * (1 - y) * Sd
        go0 = np.asarray(d_sigma, np.float64)[:n] * Sd
    dY = np.zeros((n, 16))
    dY[:, :3] = dy
    zero = np.zeros_like
    m2, m1, mh = (rec["c2"] > 0).astype(np.float64), (rec["c1"] > 0).astype(np.float64), (rec["h1"] > 0).astype(np.float64)
    dC2, e2, p2, _ = _stage(dY, zero(dY), Wc3, m2, round16)
    dC1, e1, p1, _ = _stage(dC2, e2, Wc2, m1, round16)
    dCin, ei, pi, _ = _stage(dC1, e1, Wc1, None, round16)
    dO = np.concatenate([go0[:, None], dCin[:, :15]], 1)
    eo = np.concatenate([np.zeros((n, 1)), ei[:, :15]], 1)
    dH1, eh, ph, _ = _stage(dO, eo, W2, mh, round16)
    W1d = np.asarray(W1, np.float64)
    out = dict(n=n, dY=dY, dC2=dC2, dC1=dC1, dCin=dCin, dO=dO, dH1=dH1, masks=dict(c2=m2, c1=m1, h1=mh),
               pre=dict(dY=dy, dC2=p2, dC1=p1, dCin=pi, dO0=go0, dH1=ph),
               dfeat=dH1 @ W1d / Sd, M_dfeat=np.abs(dH1) @ np.abs(W1d) / Sd)
    out["b_dfeat"] = eh @ np.abs(W1d) / Sd + (64 + 2) * U * out["M_dfeat"]
    for name, G, dG, A in (("c3", dY, zero(dY), rec["c2"]), ("c2", dC2, e2, rec["c1"]), ("c1", dC1, e1, colour_input(rec["out"])),
                           ("w2", dO, eo, rec["h1"]), ("w1", dH1, eh, rec["feat"])):
        out["g_" + name] = G.T @ A / Sd
        out["M_" + name] = np.abs(G).T @ np.abs(A) / Sd
        out["b_" + name] = dG.T @ np.abs(A) / Sd + (n + 2) * U * out["M_" + name]
    return out


GRADS = ("w1", "w2", "c1", "c2", "c3")          # the order of the g_* arguments of ia_field_bwd
GRAD_SHAPES = lambda n_levels: dict(w1=(64, 2 * n_levels), w2=(16, 64), c1=(64, 16), c2=(64, 64), c3=(16, 64))


def bwd_workspace_bytes(V, n_levels):
    """what the header's ia_field_bwd_workspace_bytes documents: one fp32 gradient set per workgroup of 2 x 32 samples, 512
    workgroups at most (restated for the CPU tests only; the GPU tests ask the library)"""
    nb = max(1, min(512, (max(V, 0) + 63) // 64))
    return nb * (64 * 2 * n_levels + 1024 + 1024 + 4096 + 1024) * 4


# ---- lattice inputs: bound zero ---------------------------------------------------------------------------------------
LATTICE_V = (1, 31, 32, 33, 63, 64, 65, 129)
BIG_V = 512 * 2 * 32 + 32 + 5          # 512 workgroups x 2 waves x 32 samples, one more full tile, 5 samples: a second grid-stride round
LATTICE_CASES = tuple((L, V, None) for L in (8, 16) for V in LATTICE_V) + ((8, 129, 100), (16, 129, 100), (16, BIG_V, None))
LATTICE_SCALES = (1.0, 4.0)
lattice_scales = lambda V: LATTICE_SCALES if V < 1000 else LATTICE_SCALES[1:]      # the large case once
HALF_EXACT = 2048                      # integers up to here are halves


def _sparse_pm1(rng, k, m, per_col):
    """[k][m] in {-1, 0, 1}, exactly per_col non-zeros in every column (the backward reduces a column: W^T g)"""
    W = np.zeros((k, m))
    for c in range(m):
        W[rng.choice(k, per_col, replace=False), c] = rng.choice([-1.0, 1.0], per_col)
    return W


def lattice_inputs(n_levels, V, S, n_live=None, seed=0):
    """Integer inputs on which the backward is exact.  Worst case per stage at S = 4: |dY| <= 16 * 1/4 * 4 = 16,
    |dC2| <= 3 * 16 = 48 (Wc3 dense), |dC1| <= 4 * 48 = 192, |dCin| <= 3 * 192 = 576, |dO[0]| <= 12, |dH1| <= 3 * 576 = 1728
    <= 2048 with 4 / 3 / 3 non-zeros per reduced column of Wc2 / Wc1 / W2.  Both exactness conditions are asserted on the
    reference before the inputs are returned: every pre-rounding stage value an integer of magnitude <= 2048, and
    M S < 2^24 for dfeat and every weight-gradient element (so any summation order is exact)."""
    rng = np.random.RandomState(7000 + 1000 * n_levels + V % 4099 + 17 * int(S) + seed)
    nf = 2 * n_levels
    W = dict(W1=rng.choice([-1.0, 0.0, 1.0], (64, nf)), W2=_sparse_pm1(rng, 16, 64, 3), Wc1=_sparse_pm1(rng, 64, 16, 3),
             Wc2=_sparse_pm1(rng, 64, 64, 4), Wc3=rng.choice([-1.0, 1.0], (16, 64)))
    W = {k: v.astype(np.float16) for k, v in W.items()}
    relu_ints = lambda cols: rng.randint(1, 3, (V, cols)) * (rng.rand(V, cols) < 0.45)         # >= 0 with exact zeros
    feat = rng.randint(-2, 3, (V, nf)) * (rng.rand(V, nf) < 0.7)
    out = rng.randint(-3, 4, (V, 16))
    acts = join_record(feat, relu_ints(64), out, relu_ints(64), relu_ints(64))
    rgb = rng.choice(np.array([0.25, 0.5, 0.75], np.float32), (V, 3))
    d_rgb = (16.0 * rng.randint(-1, 2, (V, 3))).astype(np.float32)
    d_sigma = rng.randint(-3, 4, V).astype(np.float32)
    inp = dict(acts=acts, rgb=rgb, d_rgb=d_rgb, d_sigma=d_sigma, n_live=n_live, S=np.float32(S), **W)
    R = mlp_bwd_ref(**inp)
    n = R["n"]
    for k, v in R["pre"].items():
        assert (v == np.round(v)).all() and np.abs(v).max() <= HALF_EXACT, ("stage not on the half lattice", k, float(np.abs(v).max()))
    rec = split_record(acts)
    assert (rec["out"] < 0).any() and all((rec[k] == 0).any() for k in ("feat", "h1", "c1", "c2"))
    for k, m in R["masks"].items():      # open on some samples, closed on others: per unit once there are enough samples
        assert m.any() and not m.all(), k
        assert n < 31 or (m.any(0).all() and not m.all(0).any()), k
    for g in GRADS:
        assert (R["M_" + g] * float(S)).max() < 2 ** 24 - 64, ("weight-gradient sum not exact in fp32", g, float(R["M_" + g].max()))
    assert (R["M_dfeat"] * float(S)).max() < 2 ** 24
    return inp, R


def lattice_prefill(n_levels, seed=0):
    """small integers the five g_* buffers hold before the call (the accumulate contract)"""
    rng = np.random.RandomState(7500 + seed)
    return {g: rng.randint(-5, 6, s).astype(np.float32) for g, s in GRAD_SHAPES(n_levels).items()}


# ---- real-valued inputs ---------------------------------------------------------------------------------------------
REAL_V = 4097
# a body-sized box as NeRFNGPNet.initialize(bbox) derives centre and scale from it: nothing dyadic
REAL_CENTER = np.array([0.0137, -0.2871, 0.0209], np.float32)
REAL_SCALE = np.array([2.0713, 2.3859, 1.1047], np.float32)
WEIGHT_NAMES = ("W1", "W2", "Wc1", "Wc2", "Wc3")


def xavier_weights(n_levels, seed=0):
    """fp16 matrices of the magnitude the synthetic field uses (uniform in +-sqrt(6 / (out + in)))"""
    rng = np.random.RandomState(8000 + n_levels + seed)
    shp = dict(W1=(64, 2 * n_levels), W2=(16, 64), Wc1=(64, 16), Wc2=(64, 64), Wc3=(16, 64))
    return {k: (rng.uniform(-1, 1, s) * np.sqrt(6.0 / sum(s))).astype(np.float16) for k, s in shp.items()}


def real_points(V, seed=0):
    """points inside and slightly outside the box"""
    rng = np.random.RandomState(8100 + seed + V % 977)
    u = rng.rand(V, 3) * 1.1 - 0.05
    return ((u - 0.5) * REAL_SCALE.astype(np.float64) + REAL_CENTER.astype(np.float64)).astype(np.float32)


def real_table(n_entries, seed=0):
    return np.random.RandomState(8200 + seed).uniform(-0.5, 0.5, (n_entries, 2)).astype(np.float16)


def real_gradients(V, seed=0, binades=24):
    """d_rgb [V, 3], d_sigma [V]: both signs, magnitudes 2^-U(0, binades); with the scale of ia_field_grad_scale the largest
    lands at 2^10 and the smallest below 2^-14, in the subnormal halves (y (1 - y) <= 1/4 takes two more binades off d_rgb)"""
    rng = np.random.RandomState(8300 + seed + V % 977)
    mag = lambda *s: (rng.choice([-1.0, 1.0], s) * 2.0 ** -rng.uniform(0, binades, s)).astype(np.float32)
    return mag(V, 3), mag(V)


def mlp_fwd_emul(feat, W1, W2, Wc1, Wc2, Wc3):
    """Plain fp32 emulation of the forward (fp32 matmul over half operands, np.float16 at the rounding points):
    -> (record fp16, rgb fp32 [V, 3], sigma fp32 [V]).  Builds the record of the CPU tests; the GPU tests take the kernel's."""
    f32 = lambda a: np.asarray(a).astype(np.float16).astype(np.float32)
    h16 = lambda a: a.astype(np.float16)
    relu = lambda a: np.maximum(a, np.float32(0))
    feat = h16(np.asarray(feat))
    h1 = h16(relu(f32(feat) @ f32(W1).T))
    out = h16(f32(h1) @ f32(W2).T)
    c1 = h16(relu(colour_input(f32(out)) @ f32(Wc1).T))
    c2 = h16(relu(f32(c1) @ f32(Wc2).T))
    a5 = f32(c2) @ f32(Wc3).T[:, :3]
    rgb = h16(np.float32(1) / (np.float32(1) + np.exp(-a5, dtype=np.float32))).astype(np.float32)
    return join_record(feat, h1, out, c1, c2), rgb, f32(out[:, 0])


def host_real_inputs(n_levels, V=REAL_V, seed=0):
    """the real-valued case with a host-made record (random half features through `mlp_fwd_emul`) and the reference's scale"""
    W = xavier_weights(n_levels, seed)
    rng = np.random.RandomState(8400 + seed + n_levels)
    acts, rgb, _ = mlp_fwd_emul(rng.uniform(-0.5, 0.5, (V, 2 * n_levels)), **W)
    d_rgb, d_sigma = real_gradients(V, seed)
    S = grad_scale_ref(rgb, d_rgb, d_sigma, None)
    return dict(acts=acts, rgb=rgb, d_rgb=d_rgb, d_sigma=d_sigma, n_live=None, S=S, **W)


def assert_real_case_is_hard(R):
    """what the real-valued case is there for: halves in the subnormal range, every mask both open and closed"""
    for k in ("dY", "dC2", "dC1", "dH1"):
        v = np.abs(R[k])
        assert ((v > 0) & (v < 2.0 ** -14)).any(), ("no subnormal half in", k)
    assert np.abs(R["dY"]).max() > 256      # and the top of the range is used
    for k, m in R["masks"].items():
        assert 0.1 < m.mean() < 0.9 and (m.any(0) & ~m.all(0)).sum() >= 32, k      # (a random layer has some dead units)


# ---------------------------------------------------------------------------------------------------------------------
# ia_field_grad_scale
# ---------------------------------------------------------------------------------------------------------------------
SCALE_EMPTY = np.float32(1024) / np.float32(1e-30)
SCALE_V = (1, 255, 256, 257, 65536 + 300)       # around one block of 256; 256 blocks x 256 threads and 300 more: a grid-stride round


def grad_scale_ref(rgb, d_rgb, d_sigma, n_live):
    """*scale = 1024 / max(|d_rgb y (1 - y)|, |d_sigma|, 1e-30) over the live samples in fp32, the operation order of the
    header's formula ((d_rgb y) (1 - y)); NaN when any term is NaN or the maximum infinite.  A maximum is the same in any
    order: the kernel must give these bits."""
    V = len(d_sigma)
    n = V if n_live is None else max(0, min(V, int(n_live)))
    y, g, s = np.asarray(rgb, np.float32)[:n], np.asarray(d_rgb, np.float32)[:n], np.asarray(d_sigma, np.float32)[:n]
    with np.errstate(all="ignore"):
        t = np.concatenate([np.abs((g * y) * (np.float32(1) - y)).ravel(), np.abs(s).ravel(), np.zeros(1, np.float32)])
        if np.isnan(t).any() or np.isinf(t).any():
            return np.float32(np.nan)
        return np.float32(np.float32(1024) / np.maximum(t.max(), np.float32(1e-30)))


def grad_scale_inputs(V, seed=0):
    rng = np.random.RandomState(8500 + seed + V % 977)
    rgb = rng.rand(V, 3).astype(np.float16).astype(np.float32)
    d_rgb = (rng.randn(V, 3) * 2.0 ** rng.randint(-12, 3, (V, 3))).astype(np.float32)
    d_sigma = (rng.randn(V) * 2.0 ** rng.randint(-12, 1, V) * 0.05).astype(np.float32)
    return rgb, d_rgb, d_sigma


# ---------------------------------------------------------------------------------------------------------------------
# ia_field_fwd_train: the record, stage by stage
# ---------------------------------------------------------------------------------------------------------------------
FIELD_ROUND = 256 * 12 * 64            # ia_launch_field: 256 workgroups at most x 12 waves x 64 samples per wave step
FWD_V = (1, 63, 64, 65, 769, FIELD_ROUND + 64 + 5)      # the last: one full round of the launch, a full tile and a ragged one
SHARD_V = 8192 + 65                    # at and above 8192 samples a call with an enc_ws takes the sharded encoding


def _near_boundary(v, e, relu):
    """(rn16(relu(v)), bound): zero where v is farther than e from every rounding boundary, else e + the spacing to the
    neighbour (|rn16(a) - rn16(b)| <= |a - b| + one spacing; results lie on the half grid, so with e below the spacing this
    admits exactly the neighbour -- e exceeds the spacing only next to the zero of a relu, among the subnormal halves)"""
    vr = np.maximum(v, 0.0) if relu else v
    r16 = vr.astype(np.float16)
    r = r16.astype(np.float64)
    bits = r16.view(np.uint16)
    e5 = ((bits >> 10) & 0x1F).astype(np.int32)
    sp = np.ldexp(1.0, np.maximum(e5, 1) - 25)                  # the gap from |r| to the next half away from zero
    d = np.abs(vr) - np.abs(r)
    # the boundaries are the midpoints of the gaps; towards zero the gap is half as wide when |r| is a power of two (not among
    # the subnormals, which are equally spaced)
    gap = np.where(((bits & 0x3FF) == 0) & (e5 > 1) & (d < 0), sp / 2, sp)
    dist = gap / 2 - np.abs(d)
    if relu:
        dist = np.where(v < 0, -v, np.minimum(dist, v))        # below zero the only boundary is zero itself
    return r, np.where(dist > e, 0.0, e + sp)


def fwd_stage(a, W, relu):
    """one layer from the record's own input a [V, k]: (reference half values as float64, bound per element)"""
    W = np.asarray(W, np.float64)
    v, M = a @ W.T, np.abs(a) @ np.abs(W).T
    return _near_boundary(v, (W.shape[1] + 1) * U * M, relu)


def fwd_rgb_stage(c2, Wc3):
    W = np.asarray(Wc3, np.float64)[:3]
    v, M = c2 @ W.T, np.abs(c2) @ np.abs(W).T
    e = (64 + 1) * U * M
    s = 1.0 / (1.0 + np.exp(-v))
    return _near_boundary(s, s * (1 - s) * e * (1 + e) + 5 * U * s, False)


def fwd_record_checks(acts, W1, W2, Wc1, Wc2, Wc3):
    """{stage: (reference, bound)} for h1, out, c1, c2, rgb, each from the previous stage AS THE RECORD HOLDS IT (acts: the record
    or its `split_record`)"""
    r = acts if isinstance(acts, dict) else split_record(acts)
    V, B = len(r["feat"]), 8192
    if V > B:          # in blocks of rows that stay in the cache: the large case is several times faster than in one piece
        parts = [fwd_record_checks({k: v[i:i + B] for k, v in r.items()}, W1, W2, Wc1, Wc2, Wc3) for i in range(0, V, B)]
        return {k: tuple(np.concatenate([p[k][j] for p in parts]) for j in range(2)) for k in parts[0]}
    return dict(h1=fwd_stage(r["feat"], W1, True), out=fwd_stage(r["h1"], W2, False), c1=fwd_stage(colour_input(r["out"]), Wc1, True),
                c2=fwd_stage(r["c1"], Wc2, True), rgb=fwd_rgb_stage(r["c2"], Wc3))
