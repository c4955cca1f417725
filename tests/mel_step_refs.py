"""Plain float64 statements of one reverse step of the mel samplers - the ancestral step and ProDiff's x0-prediction step, the DDIM family's
coefficients, the PLMS multistep update, the denoiser's input row - written from the definitions the kernel comments cite
(shallow_diffusion_tts.py:130-162, :165-197, :254-260, prodiff.py:141-153, net.py:114-116, Song et al. 2021 eq. 12 / 16) - not from the
kernels - with derived fp32 bounds and the controlled-output cases of tests/test_gpu_mel_sampler_steps.py. The mel counterpart of
tests/sampler_step_refs.py.

No GPU, no HIP library. tests/test_mel_step_refs_cpu.py checks the statements against the oracle (oracle/restatement.py) in float64, asserts
that the case table populates every regime, and shows each wrong variant of a statement leaving the bound on the table's own inputs.
"""
import math

import numpy as np

F64 = np.float64
U24 = 2.0 ** -24    # unit roundoff of fp32: one rounding moves a value v by at most U24 * |v|
M_MEL = 80          # mel bins
C_MEL = 256         # production residual_channels
K_MEL = 4           # timesteps = K_step of the small test nets
K_PLMS = 5          # the smallest K_step at which a PLMS call with four history entries moves x (at K_step = 4 that call is the no-op at t = 0)
KP_IN = 96          # the packed input projection's K: M rounded up to 32, zero filled beyond M
MEL_COEF_KEYS = ("recip", "recipm1", "c1", "c2", "sigma")


# ------------------------------------------------------------------------------------------------
# statements
# ------------------------------------------------------------------------------------------------
def mel_coef_ddpm(tables, t):
    """The float64 schedule entries of network time t for the ancestral step. `tables`: name -> 1-D table under the reference's buffer names (the
    fp32 tables the sampler reads, widened). sigma = exp(0.5 posterior_log_variance_clipped) for t > 0 and 0 at t = 0 (:159-162)."""
    g = lambda k: float(np.asarray(tables[k], F64)[t])
    return dict(recip=g("sqrt_recip_alphas_cumprod"), recipm1=g("sqrt_recipm1_alphas_cumprod"), c1=g("posterior_mean_coef1"),
                c2=g("posterior_mean_coef2"), sigma=math.exp(0.5 * g("posterior_log_variance_clipped")) if t > 0 else 0.0)


def _row_mask(shape, lens):
    B, T = shape[0], shape[1]
    return np.arange(T)[None, :] >= np.asarray(lens).reshape(B, 1)


def mel_step(x, net_out, coef, z, step, x0_pred=False, lens=None, dtype=F64):
    """One reverse step on x [B,T,M] (predict_start_from_noise, the clamp of p_mean_variance, q_posterior, p_sample's nonzero mask):
      x0 = clamp(recip x - recipm1 eps, -1, 1)   with eps = net_out, or x0 = net_out without a clamp when `x0_pred` (prodiff.py:144-148)
      x' = c1 x0 + c2 x + [step > 0] sigma z     (z is not touched at step 0, whatever it holds)
    and rows t >= lens[b] are 0. net_out broadcasts against x ([M] or [B,T,M]). dtype: float64 is the statement; float32 is "the same step in
    fp32 numpy on the CPU", every operation rounded, the yardstick of the 4 x rule."""
    x, z = np.asarray(x, dtype), np.asarray(z, dtype)
    net_out = np.broadcast_to(np.asarray(net_out, dtype), x.shape)
    k = {n: dtype(coef[n]) for n in MEL_COEF_KEYS if n in coef}
    x0 = net_out if x0_pred else np.clip(k["recip"] * x - k["recipm1"] * net_out, dtype(-1.0), dtype(1.0))
    out = k["c1"] * x0 + k["c2"] * x
    if step > 0:
        out = out + k["sigma"] * z
    if lens is not None:
        out = np.where(_row_mask(x.shape, lens)[..., None], dtype(0.0), out)
    assert out.dtype == dtype
    return out


def ddim_coef(ac_t, ac_prev, eta):
    """Song et al. 2021: sigma = eta sqrt((1 - ac_prev) / (1 - ac_t)) sqrt(1 - ac_t / ac_prev) (eq. 16) and
    x_prev = sqrt(ac_prev) x0 + sqrt(1 - ac_prev - sigma^2) eps' + sigma z with eps' = (x - sqrt(ac_t) x0) / sqrt(1 - ac_t) (eq. 12), collected as
    x_prev = c1 x0 + c2 x + sigma z. ac_prev = 1 on the last transition (to x_0): sigma = 0, c2 = 0, c1 = 1."""
    ac_t, ac_prev = float(ac_t), float(ac_prev)
    sigma = eta * math.sqrt((1.0 - ac_prev) / (1.0 - ac_t)) * math.sqrt(max(0.0, 1.0 - ac_t / ac_prev))
    dir_ = math.sqrt(max(0.0, 1.0 - ac_prev - sigma * sigma))
    c2 = dir_ / math.sqrt(1.0 - ac_t)
    c1 = math.sqrt(ac_prev) - c2 * math.sqrt(ac_t)
    return dict(c1=c1, c2=c2, sigma=sigma)


def mel_coef_ddim(tables, ac64, ts, i, eta, cast=np.float32):
    """Coefficients of transition i of the strided sampler over network times ts: the x0 prediction reads the fp32 tables at ts[i], the update
    ddim_coef(ac[ts[i]], ac[ts[i+1]] or 1, eta) on the float64 cumulative products, cast to fp32 (`cast`; None keeps float64)."""
    t = int(ts[i])
    k = ddim_coef(ac64[t], ac64[int(ts[i + 1])] if i + 1 < len(ts) else 1.0, eta)
    if cast is not None:
        k = {n: float(cast(v)) for n, v in k.items()}
    g = lambda n: float(np.asarray(tables[n], F64)[t])
    return dict(recip=g("sqrt_recip_alphas_cumprod"), recipm1=g("sqrt_recipm1_alphas_cumprod"), **k)


def plms_coef(a_t, a_prev):
    """get_x_pred (:170-178): x_pred = x + d (kx x - ke eps)"""
    a_t, a_prev = float(a_t), float(a_prev)
    st, sp = math.sqrt(a_t), math.sqrt(a_prev)
    return dict(d=a_prev - a_t, kx=1.0 / (st * (st + sp)), ke=1.0 / (st * (math.sqrt((1.0 - a_prev) * a_t) + math.sqrt((1.0 - a_t) * a_prev))))


def plms_prime(eps_history, eps_pred=None):
    """The five multistep combinations (:183-192). eps_history: newest first, [eps(x_t, t), the previous call's, ...], 1 to 4 entries. With one
    entry the call is the first of a run: eps' = eps itself for the predictor, (eps + eps_pred) / 2 once the second evaluation is there."""
    h = [np.asarray(e, F64) for e in eps_history]
    if len(h) == 1:
        return h[0] if eps_pred is None else (h[0] + np.asarray(eps_pred, F64)) / 2.0
    if len(h) == 2:
        return (3.0 * h[0] - h[1]) / 2.0
    if len(h) == 3:
        return (23.0 * h[0] - 16.0 * h[1] + 5.0 * h[2]) / 12.0
    return (55.0 * h[0] - 59.0 * h[1] + 37.0 * h[2] - 9.0 * h[3]) / 24.0


def plms_step(x, eps_history, a_t, a_prev, second_eval=None):
    """p_sample_plms (:165-197) on x [B,T,M]. eps_history as in plms_prime; on the first call of a run (one entry) `second_eval(x_pred)` gives
    the network's output at the predicted x and the previous time (the double evaluation, :184-186); without it the result is the predictor."""
    x = np.asarray(x, F64)
    k = plms_coef(a_t, a_prev)
    pred = lambda e: x + k["d"] * (k["kx"] * x - k["ke"] * e)
    if len(eps_history) == 1 and second_eval is not None:
        return pred(plms_prime(eps_history, second_eval(pred(plms_prime(eps_history)))))
    return pred(plms_prime(eps_history))


def plms_times(k_step, interval):
    """reversed(range(0, K_step, interval)) with each call's previous time max(t - interval, 0) (:254-260, :172)"""
    return [(t, max(t - interval, 0)) for t in reversed(range(0, k_step, interval))]


def mel_input_row(x, w_in, b_in, lens=None):
    """DiffNet's input (net.py:114-116): X = relu(input_projection(x)) = relu(W_in x + b_in), a M -> C conv of kernel 1; rows t >= lens[b] are
    zero. x [B,T,M]; w_in [C,M]; b_in [C] -> X [B,T,C]."""
    x, w_in, b_in = (np.asarray(a, F64) for a in (x, w_in, b_in))
    X = np.maximum(x @ w_in.T + b_in, 0.0)
    if lens is not None:
        X = np.where(_row_mask(x.shape, lens)[..., None], 0.0, X)
    return X


# ------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------
def dot_bound(a, w, bias):
    """The standard bound on a K-term fp32 dot product a . w[n] of these operands in any order, fused or not, K U24 sum |a w|, plus one rounding for
    the bias add. a [K], w [N,K], bias [N] -> (exact float64 value [N], bound [N])."""
    a, w, bias = (np.asarray(v, F64) for v in (a, w, bias))
    exact = w @ a + bias
    return exact, a.shape[-1] * U24 * (np.abs(w) @ np.abs(a)) + U24 * np.abs(exact)


def mel_step_bound(x, net_out, coef, z, step, e_net, x0_pred=False, lens=None, e_x=0.0, sigma_ulps=2, coef_casts=False):
    """Bound on |fp32 result - mel_step| for a sampler that evaluates the step in fp32 from the same fp32 x, z and coefficients and a network
    output that is off by at most e_net (dot_bound for the controlled net). One rounding (U24 relative) per fp32 operation, as ss_ddpm_update
    documents them - 9 for the ancestral step, none of the last four at step 0:
      x0:   recip*x, recipm1*eps, their difference         (3; the clamp is exact and 1-Lipschitz, and where the pre-clamp value is beyond a rail by
                                                            more than its own error the clamp's output carries none; x0_pred: none of the three)
      mean: c2*x, fma(c1, x0, c2*x)                        (2)
      x':   sigma = expf(0.5 logvar) to 2 ulp (`sigma_ulps`; 0 for a sigma the caller supplies in fp32), sigma*z (1), mean + sigma*z (1)
    `coef_casts`: c1, c2 and sigma are float64 values cast to fp32 - one more rounding on each of c1*x0, c2*x and sigma*z (3; pass sigma_ulps = 0).
    `e_x`: x itself is off by at most e_x (a chain of steps). Rows >= lens[b] are exactly 0: bound 0."""
    x, z = np.asarray(x, F64), np.asarray(z, F64)
    net_out = np.broadcast_to(np.asarray(net_out, F64), x.shape)
    e_net = np.broadcast_to(np.asarray(e_net, F64), x.shape)
    e_x = np.broadcast_to(np.asarray(e_x, F64), x.shape)
    if x0_pred:
        x0, e0 = net_out, e_net
    else:
        a, b = coef["recip"] * x, coef["recipm1"] * net_out
        raw = a - b
        e0 = abs(coef["recip"]) * e_x + abs(coef["recipm1"]) * e_net + U24 * (np.abs(a) + np.abs(b) + np.abs(raw))
        e0 = np.where((raw - e0 > 1.0) | (raw + e0 < -1.0), 0.0, e0)
        x0 = np.clip(raw, -1.0, 1.0)
    p, q = coef["c1"] * x0, coef["c2"] * x
    casts = 1.0 if coef_casts else 0.0
    e = abs(coef["c1"]) * e0 + abs(coef["c2"]) * e_x + U24 * (casts * np.abs(p) + (1.0 + casts) * np.abs(q) + np.abs(p + q))
    if step > 0:
        sz = coef["sigma"] * z
        e = e + U24 * ((1.0 + sigma_ulps + casts) * np.abs(sz) + np.abs(p + q + sz))
    if lens is not None:
        e = np.where(_row_mask(x.shape, lens)[..., None], 0.0, e)
    return e


def run_steps(x, net_out, e_net, steps, lens=None):
    """A chain of steps on a network whose output does not depend on x (the controlled net): the float64 statement and the bound of the whole
    chain, each step's bound fed the previous one's as e_x. steps: dicts(coef, z, step, and optionally x0_pred / sigma_ulps / coef_casts)."""
    ref, e = np.asarray(x, F64), 0.0
    for s in steps:
        kw = {k: s[k] for k in ("x0_pred", "sigma_ulps", "coef_casts") if k in s}
        e = mel_step_bound(ref, net_out, s["coef"], s["z"], s["step"], e_net, lens=lens, e_x=e, **kw)
        ref = mel_step(ref, net_out, s["coef"], s["z"], s["step"], x0_pred=s.get("x0_pred", False), lens=lens)
    return ref, e


def plms_step_bound(x, eps_history, a_t, a_prev, e_eps=0.0):
    """Bound on |fp32 result - plms_step| (no second evaluation: two or more entries, or the predictor) from the same fp32 inputs and an fp32
    alphas_cumprod table, history entries off by at most e_eps. Counted roundings: the combination eps' has at most 4 products, 3 sums and the
    division (8, each at most the sum S of the terms' magnitudes); d = a_prev - a_t (1), kx (5: two roots, a sum, a product, the quotient),
    ke (10), kx*x, ke*eps', their difference, d*(.), x + (.) - 16 on the term d (|kx x| + |ke eps'|) at the most, and one on the result."""
    x = np.asarray(x, F64)
    h = [np.abs(np.asarray(e, F64)) for e in eps_history]
    w = {1: (1.0,), 2: (1.5, 0.5), 3: (23 / 12, 16 / 12, 5 / 12), 4: (55 / 24, 59 / 24, 37 / 24, 9 / 24)}[len(h)]
    S = sum(wi * hi for wi, hi in zip(w, h))
    e_prime = 8.0 * U24 * S + sum(w) * e_eps
    k = plms_coef(a_t, a_prev)
    prime = plms_prime(eps_history)
    term = abs(k["d"]) * (np.abs(k["kx"] * x) + np.abs(k["ke"] * prime))
    out = x + k["d"] * (k["kx"] * x - k["ke"] * prime)
    return U24 * (16.0 * term + np.abs(out)) + abs(k["d"] * k["ke"]) * e_prime


def mel_input_row_bound(x, w_in, b_in):
    """|fp32 X - mel_input_row|: an M-term dot product in any order and the bias add (the ReLU is exact and 1-Lipschitz)"""
    x, w_in, b_in = (np.asarray(a, F64) for a in (x, w_in, b_in))
    return x.shape[-1] * U24 * (np.abs(x) @ np.abs(w_in).T) + U24 * np.abs(x @ w_in.T + b_in)


# ------------------------------------------------------------------------------------------------
# the controlled-output cases of the GPU test: inputs and their regimes, from a seed alone
# ------------------------------------------------------------------------------------------------
TARGET_DELTA = 4e-6    # the near-rail elements' pre-clamp x0 lies within this of a rail: some tens of fp32 ulp of 1, so that the roundings of the
#                        three operations before the clamp can carry an element across it, and far more than the rounding of the steered x itself
REGIMES = ("below", "above", "inside", "lo_out", "lo_in", "hi_in", "hi_out")

# Shapes: the smallest that still cover the launch forms. The GPU test asserts each precondition.
#   slices:  the split-K slices form of SkipSrc (the split-K pick returns > 1), lens = T and a ragged one
#   odd:     B*T odd, so the last mel_tail workgroup (MTR = 2 rows) holds one row; lens = T, 1 and T - 1
#   reduced: B*T odd and cdiv(T, 64) * B * 4 * 2 = 272 > 256 CUs: the pick returns 1 and the tail kernel reads the reduced G; B*T <= 2048
CASES = {
    "slices":  dict(B=2, T=97, lens=[97, 60], seed=61, ksplit_gt1=True),
    "odd":     dict(B=3, T=33, lens=[33, 1, 32], seed=62, ksplit_gt1=True),
    "reduced": dict(B=17, T=65, lens=[65, 1, 64, 33] * 4 + [65], seed=63, ksplit_gt1=False),
}
EXTREME = dict(B=2, T=33, lens=[33, 20], seed=64)     # the 1000-step schedule (steps 999 and 1)
for _c in (CASES["odd"], CASES["reduced"]):
    assert (_c["B"] * _c["T"]) % 2 == 1
assert -(-CASES["reduced"]["T"] // 64) * CASES["reduced"]["B"] * 4 * 2 > 256 and CASES["reduced"]["B"] * CASES["reduced"]["T"] <= 2048


def controlled_mel_weights(wset="dyadic", seed=7):
    """beta [C] (skip_projection.bias, mixed sign), w_final [M, C], b_final [M], fp32. With skip_projection.weight = 0 the stack's output is
    g = relu(beta) on every valid frame and eps[n] = w_final[n] . g + b_final[n], a 256-term dot product per mel bin.
      "dyadic": beta on a grid of 1/8 in [-2, 2], w_final of 1/256 in [-1/8, 1/8], b_final of 1/64: every product is a multiple of 2^-11 and every
                partial sum stays below 2^6, 17 bits - the dot product is exact in fp32 in ANY order, fused or not. The two launch forms sum it in
                different orders (mel_tail_kernel's comment) but reach the same eps bit for bit, so their outputs can be compared with torch.equal.
      "random": fp32 normals: the sum rounds, and differently per form."""
    r = np.random.default_rng(seed)
    if wset == "dyadic":
        beta = (r.integers(-16, 17, C_MEL) / 8.0).astype(np.float32)
        w = (r.integers(-32, 33, (M_MEL, C_MEL)) / 256.0).astype(np.float32)
        b = (r.integers(-32, 33, M_MEL) / 64.0).astype(np.float32)
    else:
        beta = (r.standard_normal(C_MEL) * 0.7).astype(np.float32)
        w = (r.standard_normal((M_MEL, C_MEL)) * 0.08).astype(np.float32)
        b = (r.standard_normal(M_MEL) * 0.3).astype(np.float32)
    return dict(beta=beta, w_final=w, b_final=b, wset=wset)


def net_output(weights):
    """(eps [M], e_eps [M]) of a valid frame of the controlled net: the float64 value and the bound on an fp32 evaluation of it - dot_bound's for
    weights that round; 0 for the dyadic set, whose every product, partial sum and bias add is exact in fp32 whatever the order (the CPU test
    asserts the grid, the magnitudes and two summation orders)"""
    eps, e = dot_bound(np.maximum(weights["beta"].astype(F64), 0.0), weights["w_final"], weights["b_final"])
    return eps, (np.zeros_like(e) if weights["wset"] == "dyadic" else e)


def _steer(r, shape, coef, eps, regime_of):
    """fp32 x whose pre-clamp x0 = recip x - recipm1 eps[n] falls into the regime of its element"""
    u = r.uniform(0.0, 1.0, shape)
    d = (0.25 + 0.75 * u) * TARGET_DELTA
    target = np.select([regime_of == k for k in range(len(REGIMES))],
                       [-1.25 - 2.0 * u, 1.25 + 2.0 * u, 1.9 * u - 0.95, -1.0 - d, -1.0 + d, 1.0 - d, 1.0 + d])
    return ((target + coef["recipm1"] * eps) / coef["recip"]).astype(np.float32)


def regime_masks(x, coef, eps):
    """which regime each element's float64 pre-clamp x0 lies in (from the fp32 x as the sampler reads it)"""
    raw = coef["recip"] * np.asarray(x, F64) - coef["recipm1"] * eps
    D = TARGET_DELTA
    return dict(below=raw < -1.0 - D, above=raw > 1.0 + D, inside=np.abs(raw) < 1.0 - D, lo_out=(raw < -1.0) & (raw >= -1.0 - D),
                lo_in=(raw > -1.0) & (raw <= -1.0 + D), hi_in=(raw < 1.0) & (raw >= 1.0 - D), hi_out=(raw > 1.0) & (raw <= 1.0 + D)), raw


def controlled_mel_case(name, tables, steps=None, wset="dyadic"):
    """Inputs of case `name` (or a spec like the entries of CASES with its "name") as numpy arrays, fp32 where the sampler reads fp32:
    x {step: [B,T,M]} steered for that step's coefficients, one regime per element by (t + n) % 8 (two of eight inside); z [K,B,T,M] with the
    t = 0 slab at 1e30 (it must contribute exactly 0); cond [B,T,256]; lens; valid [B,T]; weights, eps / e_eps [M]."""
    c = CASES[name] if isinstance(name, str) else name
    name = name if isinstance(name, str) else c["name"]
    B, T, M = c["B"], c["T"], M_MEL
    K = len(np.asarray(tables["posterior_mean_coef1"]))
    steps = tuple(steps) if steps is not None else (K - 1, 1, 0)
    r = np.random.default_rng(c["seed"])
    lens = np.asarray(c["lens"], np.int32)
    valid = np.arange(T)[None, :] < lens[:, None]
    weights = controlled_mel_weights(wset)
    eps, e_eps = net_output(weights)
    slot = (np.arange(T)[None, :, None] + np.arange(M)[None, None, :] + np.zeros((B, 1, 1), int)) % 8
    regime_of = np.minimum(slot, 2) + np.maximum(slot - 3, 0)      # slots 2 and 3: inside
    z = r.standard_normal((len(steps), B, T, M)).astype(np.float32)
    x = {s: _steer(r, (B, T, M), mel_coef_ddpm(tables, s), eps, regime_of) for s in steps}
    cond = (r.standard_normal((B, T, 256)) * 0.5).astype(np.float32)
    return dict(name=name, B=B, T=T, M=M, K=K, steps=steps, lens=lens, valid=valid, x=x, z_of={s: z[i] for i, s in enumerate(steps)}, cond=cond,
                weights=weights, eps=eps, e_eps=e_eps)


def noise_tape(case, fill=None):
    """[K,B,T,M] tape of a case: slab t holds the case's z of step t, slab 0 holds 1e30, every other slab 3.0 (a wrong slab index shows)"""
    tape = np.full((case["K"], case["B"], case["T"], case["M"]), 3.0 if fill is None else fill, np.float32)
    for s, z in case["z_of"].items():
        tape[s] = z
    tape[0] = 1e30
    return tape


def controlled_step(case, tables, step, x0_pred=False, coef=None, sigma_ulps=2):
    """(statement, bound) of step `step` alone on a case's inputs"""
    coef = coef or mel_coef_ddpm(tables, step)
    z = noise_tape(case)[step]
    ref = mel_step(case["x"][step], case["eps"], coef, z, step, x0_pred=x0_pred, lens=case["lens"])
    bound = mel_step_bound(case["x"][step], case["eps"], coef, z, step, case["e_eps"], x0_pred=x0_pred, lens=case["lens"], sigma_ulps=sigma_ulps)
    return ref, bound


def over_bound(out, ref, bound):
    """the largest |out - ref| / bound and the number of elements beyond it; a zero bound asks for equality. Non-finite values count as beyond."""
    out = np.asarray(out, F64)
    d = np.abs(out - ref)
    bad = ~np.isfinite(out) | (d > bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, d / bound, np.where(d > 0, np.inf, 0.0))
    return float(np.nanmax(np.where(np.isfinite(out), ratio, np.inf))), int(bad.sum())
