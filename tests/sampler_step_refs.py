"""Plain float64 statements of one reverse step of the joint f0 / uv sampler, of the f0 denoiser's input row and of the mel q-sample / denorm
pair, written from the definitions the kernel comments cite (gaussian_multinomial_diffusion.py:326-333, :374-413, :447-452, net.py:249-252,
shallow_diffusion_tts.py:199-204, :271-275) - not from the kernels - for tests/test_gpu_sampler_steps.py.

No GPU, no HIP library. tests/test_sampler_step_refs_cpu.py checks these statements against the oracle (oracle/restatement.py), and asserts the
input conditions of the GPU test (`controlled_case`, `decision_threshold`) from the reference alone.

`f0_joint_step` takes a `dtype`: torch.float64 is the statement; torch.float32 is "the same step in fp32 torch on the CPU", the yardstick
the decision threshold and the 4 x rule are measured with.
"""
import math

import numpy as np
import torch

F64 = np.float64
U24 = 2.0 ** -24    # unit roundoff of fp32: one rounding moves a value v by at most U24 * |v|

F0_COEF_KEYS = ("recip", "recipm1", "c1", "c2", "sigma", "log_alpha_t", "log_1m_alpha_t", "log_cp_tm1", "log_1m_cp_tm1")   # F0StepCoef


def f0_coef(tables, step):
    """The float64 schedule entries of network time `step` under the names of F0StepCoef. `tables`: name -> 1-D table under the reference's buffer
    names (the fp32 tables the sampler reads, widened). sigma = exp(0.5 posterior_log_variance_clipped) for step > 0, 0 at step 0 (:332-333);
    the multinomial prior is read at t - 1, at 0 for t = 0 (:378-381)."""
    g = lambda k, i: float(np.asarray(tables[k], F64)[i])
    tm1 = max(step - 1, 0)
    return dict(recip=g("sqrt_recip_alphas_cumprod", step), recipm1=g("sqrt_recipm1_alphas_cumprod", step),
                c1=g("posterior_mean_coef1", step), c2=g("posterior_mean_coef2", step),
                sigma=math.exp(0.5 * g("posterior_log_variance_clipped", step)) if step > 0 else 0.0,
                log_alpha_t=g("log_alpha", step), log_1m_alpha_t=g("log_1_min_alpha", step),
                log_cp_tm1=g("log_cumprod_alpha", tm1), log_1m_cp_tm1=g("log_1_min_cumprod_alpha", tm1))


def _log_add_exp(a, b):
    m = torch.maximum(a, b)
    return m + torch.log(torch.exp(a - m) + torch.exp(b - m))


def first_argmax2(s0, s1):
    """argmax over two classes, the first maximum on a tie (class 0)"""
    return (s1 > s0).to(torch.int64)


def f0_joint_step(f0, uv, eps, logits, lo, hi, z, u, coef, step, dtype=torch.float64):
    """One reverse step for every frame. f0, eps, lo, hi, z [B,T]; uv [B,T] integer class; logits [B,T,2]; u [B,2,T] uniforms in [0,1)
    (u[:, k] belongs to class k); coef: F0StepCoef names -> numbers. Returns numpy float64 / int64:
      f0_new [B,T], uv_new [B,T], margin [B,T] = (g1 + q1) - (g0 + q0), mag [B,T] = the largest intermediate magnitude of the uv part.
    Gaussian part: x0 = clamp(recip x - recipm1 eps, lo, hi); mean = c1 x0 + c2 x; x' = mean + [step > 0] sigma z.
    Multinomial part: log x_t = log(clamp(onehot, 1e-30)); log x0 = log_softmax(logits); ev = log_add_exp(log x0 + log cp_(t-1),
    log(1 - cp_(t-1)) - log 2), ev = log x0 at step 0; un = ev + log_add_exp(log x_t + log a_t, log(1 - a_t) - log 2); q = un - logsumexp(un);
    g = -log(-log(u + 1e-30) + 1e-30); uv' = argmax(g + q), the first maximum."""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)
    k = {n: torch.tensor(coef[n], dtype=dtype) for n in F0_COEF_KEYS}
    x, eps, lo, hi, z, logits, u = t(f0), t(eps), t(lo), t(hi), t(z), t(logits), t(u)
    cls = (torch.as_tensor(np.asarray(uv)) != 0).to(torch.int64)
    x0 = k["recip"] * x - k["recipm1"] * eps
    x0 = torch.minimum(torch.maximum(x0, lo), hi)
    mean = k["c1"] * x0 + k["c2"] * x
    f0_new = mean + k["sigma"] * z if step > 0 else mean
    log2 = math.log(2.0)
    log_xt = torch.log(torch.nn.functional.one_hot(cls, 2).to(dtype).clamp(min=1e-30))
    log_x0 = torch.log_softmax(logits, dim=-1)
    ev = log_x0 if step == 0 else _log_add_exp(log_x0 + k["log_cp_tm1"], k["log_1m_cp_tm1"] - log2)
    one = _log_add_exp(log_xt + k["log_alpha_t"], k["log_1m_alpha_t"] - log2)
    un = ev + one
    q = un - torch.logsumexp(un, dim=-1, keepdim=True)
    gum = -torch.log(-torch.log(u.transpose(1, 2) + 1e-30) + 1e-30)
    s = gum + q
    uv_new = first_argmax2(s[..., 0], s[..., 1])
    margin = s[..., 1] - s[..., 0]
    mag = torch.stack([v.abs().amax(-1) for v in (logits, log_xt + k["log_alpha_t"], log_x0, ev, one, un, q, gum, s)]).amax(0)
    n = lambda a: a.to(torch.float64).numpy()
    return n(f0_new), uv_new.numpy(), n(margin), n(mag)


def f0_step_bound(f0, eps, lo, hi, z, coef, step, e_eps):
    """Bound on |fp32 result - f0_joint_step's f0| for a sampler that evaluates the Gaussian part in fp32 from the same fp32 inputs and an eps that
    is off by at most e_eps: one rounding (U24 relative) per fp32 operation, 10 operations -
      x0:   recip*x, recipm1*eps, their difference  (3; the clamp is exact and 1-Lipschitz)
      mean: c1*x0, c2*x, their sum                  (3)
      x':   sigma = expf(0.5 logvar) to 2 ulp (2), sigma*z (1), mean + sigma*z (1) - none of the four at step 0.
    A fused multiply-add only leaves roundings out."""
    x, eps, lo, hi, z = (np.asarray(a, F64) for a in (f0, eps, lo, hi, z))
    e_eps = np.asarray(e_eps, F64)
    a, b = coef["recip"] * x, coef["recipm1"] * eps
    e = abs(coef["recipm1"]) * e_eps + U24 * (np.abs(a) + np.abs(b) + np.abs(a - b))
    x0 = np.clip(a - b, lo, hi)
    p, q = coef["c1"] * x0, coef["c2"] * x
    e = abs(coef["c1"]) * e + U24 * (np.abs(p) + np.abs(q) + np.abs(p + q))
    if step > 0:
        sz = coef["sigma"] * z
        e = e + U24 * (3.0 * np.abs(sz) + np.abs(p + q + sz))
    return e


def decision_threshold(margin64, margin32, mag):
    """Per-frame |margin| below which a frame's voicing decision is 'undecided': 4 x the largest fp32-CPU margin error of the case, never less than
    8 fp32 ulp at the frame's largest intermediate magnitude."""
    err = float(np.abs(np.asarray(margin32, F64) - margin64).max())
    floor = 8.0 * np.spacing(np.maximum(np.asarray(mag, F64), 2.0 ** -100).astype(np.float32)).astype(F64)
    return np.maximum(4.0 * err, floor), err


def f0_input_row(f0, uv, w_in, b_in, uv_embed, lens=None):
    """DDiffNet's input (net.py:249-252): X[..., :C/2] = input_projection(f0) = w_in f0 + b_in (a 1 -> C/2 conv of kernel 1),
    X[..., C/2:] = uv_embed[uv]; rows t >= lens[b] are zero. f0, uv [B,T]; w_in, b_in [C/2]; uv_embed [2, C/2] -> X [B,T,C]."""
    f0, w_in, b_in, uv_embed = (np.asarray(a, F64) for a in (f0, w_in, b_in, uv_embed))
    cls = (np.asarray(uv) != 0).astype(np.int64)
    X = np.concatenate([f0[..., None] * w_in.reshape(-1) + b_in, uv_embed[cls]], axis=-1)
    if lens is not None:
        X[np.arange(f0.shape[1])[None, :] >= np.asarray(lens)[:, None]] = 0.0
    return X


def mel_qsample(mel, smin, smax, sa, s1, z):
    """norm_spec then q_sample (shallow_diffusion_tts.py:271-272, :199-204): x = sa ((mel - min) / (max - min) * 2 - 1) + s1 z. mel, z [B,T,M].
    Also returns the largest magnitude each element passes through (for an ulp tolerance)."""
    mel, smin, smax, z = (np.asarray(a, F64) for a in (mel, smin, smax, z))
    d, den = mel - smin, smax - smin
    q = d / den
    xs = q * 2.0 - 1.0
    x = sa * xs + s1 * z
    mag = np.max(np.abs(np.stack([d, q * 2.0, xs, sa * xs, s1 * z, x])), axis=0)
    return x, np.maximum(mag, 1.0)


def mel_denorm(x, smin, smax, lens=None):
    """denorm_spec (shallow_diffusion_tts.py:274-275): mel = (x + 1) / 2 (max - min) + min; rows t >= lens[b] are zero. x [B,T,M].
    Also returns the largest magnitude each element passes through."""
    x, smin, smax = (np.asarray(a, F64) for a in (x, smin, smax))
    h = (x + 1.0) / 2.0
    p = h * (smax - smin)
    mel = p + smin
    mag = np.max(np.abs(np.stack([x + 1.0, p, mel])), axis=0)
    if lens is not None:
        mel[np.arange(x.shape[1])[None, :] >= np.asarray(lens)[:, None]] = 0.0
    return mel, mag


# ------------------------------------------------------------------------------------------------
# the controlled-output cases of the GPU test: inputs and their regimes, from a seed alone
# ------------------------------------------------------------------------------------------------
S_F0 = 4     # f0_timesteps of the test nets
C_F0 = 192   # production f0_residual_channels

# (l0 - l1) the final projection of net g gives on every valid frame; eps is O(1). "pm40": exp(-40) underflows the log-softmax's smaller term in
# fp32 and the decision rests on the prior alone; "near0": the logits carry no preference (net 0) / a mild one (net 1)
WEIGHT_SETS = {"pm40": (40.0, -40.0), "near0": (1e-3, 2.0)}

# B items in all; with `paired` the first half belongs to net 0 and the second to net 1, else every item to net `single`.
#   B*T mod 16: the tail kernel gives 16 lanes to a frame and 16 frames to a block. The paired net needs an even item count, so its B*T is even and
#   the remainders next to a full block are 2 and 14; 1 and 15 are reached through a one-net descriptor of the same weights (odd B).
#   lens: the full length, a single frame, ragged values. (lens > T is not accepted by the entry point: the stack's buffer descriptors are sized
#   len * row bytes per item, so a longer length would let an item's loads run into its neighbour - the product never passes one.)
CASES = {
    "pm40_b4":      dict(wset="pm40", paired=True, B=4, T=67, lens=[67, 1, 50, 33], seed=11),
    "near0_rem14":  dict(wset="near0", paired=True, B=2, T=135, lens=[135, 77], seed=12),
    "near0_rem2":   dict(wset="near0", paired=True, B=2, T=137, lens=[100, 137], seed=13),
    "single_rem1":  dict(wset="near0", paired=False, single=1, B=3, T=43, lens=[43, 20, 1], seed=14),
    "single_rem15": dict(wset="pm40", paired=False, single=0, B=1, T=143, lens=[130], seed=15),
}
for _c in CASES.values():
    assert (_c["B"] * _c["T"]) % 16 in (1, 2, 12, 14, 15)
U_EDGE = (0.0, U24, 1.0 - U24)
TARGET_DELTA = 5e-3   # |margin| the targeted frames are steered to: far above any threshold, below any error of substance in the log-space terms


def controlled_weights(wset):
    """Per net g in (0, 1): beta [C] (skip_projection.bias, mixed sign), w_final [3, C], b_final [3], all fp32, different per net. With
    skip_projection.weight = 0 the stack's output is g = relu(beta) on every valid frame and (eps, l0, l1) = w_final g + b_final."""
    out = []
    for g, shift in enumerate(WEIGHT_SETS[wset]):
        r = np.random.default_rng(1000 + 17 * g + sum(map(ord, wset)))
        beta = (r.standard_normal(C_F0) * 0.5).astype(np.float32)
        w = (r.standard_normal((3, C_F0)) * 0.2).astype(np.float32)
        act = np.maximum(beta.astype(F64), 0.0)
        d = w.astype(F64) @ act
        b = np.array([0.3 - 0.5 * g, 0.0, 0.0], F64)
        b[1] = shift / 2.0 - d[1]
        b[2] = -shift / 2.0 - d[2]
        out.append(dict(beta=beta, w_final=w, b_final=b.astype(np.float32)))
    return out


def net_output(weights, dtype=F64):
    """(eps, l0, l1) of a valid frame of one controlled net in `dtype` arithmetic, and in float64 the standard bound on a K-term fp32 dot product
    of these operands in any order, K * U24 * sum |g w|, plus one rounding for the bias add."""
    act = np.maximum(weights["beta"], 0.0).astype(dtype)
    w, b = weights["w_final"].astype(dtype), weights["b_final"].astype(dtype)
    out = (w @ act + b).astype(F64)
    a64, w64 = act.astype(F64), weights["w_final"].astype(F64)
    exact = w64 @ a64 + weights["b_final"].astype(F64)
    bound = C_F0 * U24 * (np.abs(w64) @ a64) + U24 * np.abs(exact)
    return out, bound


def reduced_spec(B, T):
    """the case of the reduced skip source: 16 items at the T the split-K pick gives (looked up by the tests)"""
    return dict(name=f"reduced_b{B}_t{T}", wset="near0", paired=True, B=B, T=T, lens=[T, 1, T - 5, T // 2] * (B // 4), seed=21)


def _gumbel_inv(g):
    """u with -log(-log(u)) = g"""
    return np.exp(-np.exp(-g))


def controlled_case(name, tables):
    """Inputs of case `name` as numpy arrays (fp32 values where the sampler reads fp32): f0, uv, lo, hi [B,T]; z [S,B,T]; u [S,B,2,T];
    cond [B,T,256]; lens; net_of_item [B]; per-frame regime masks (dict of [B,T] bool; for the u regimes [S,B,T])."""
    c = CASES[name] if isinstance(name, str) else name      # or a spec like the entries of CASES, with its "name"
    name = name if isinstance(name, str) else c["name"]
    B, T, S = c["B"], c["T"], S_F0
    r = np.random.default_rng(c["seed"])
    lens = np.asarray(c["lens"], np.int32)
    net_of_item = np.repeat(np.arange(2), B // 2) if c["paired"] else np.full(B, c["single"])
    tt = np.broadcast_to(np.arange(T)[None, :], (B, T))
    valid = tt < lens[:, None]
    f0 = r.standard_normal((B, T)).astype(np.float32)
    uv = r.integers(0, 2, (B, T)).astype(np.int32)
    # clamp regimes by frame index: lo == hi (always active), a narrow band (active on many frames), wide open (idle)
    pin, band = tt % 4 == 0, tt % 4 == 1
    mid = r.uniform(-1.0, 1.0, (B, T))
    lo = np.where(pin, mid, np.where(band, -0.3, -1e4)).astype(np.float32)
    hi = np.where(pin, mid, np.where(band, 0.4, 1e4)).astype(np.float32)
    z = r.standard_normal((S, B, T)).astype(np.float32)
    u = (r.integers(1, 1 << 24, (S, B, 2, T)).astype(F64) * U24).astype(np.float32)
    cond = (r.standard_normal((B, T, 256)) * 0.5).astype(np.float32)
    # edge uniforms: frame 6 j + 3 (+ 1) carries U_EDGE[j % 3] in slot 0 (slot 1), the other slot keeps its draw
    edge0, edge1 = np.zeros((S, B, T), bool), np.zeros((S, B, T), bool)
    for j, t in enumerate(range(3, T, 6)):
        u[:, :, 0, t] = U_EDGE[j % 3]
        edge0[:, :, t] = True
        if t + 1 < T:
            u[:, :, 1, t + 1] = U_EDGE[j % 3]
            edge1[:, :, t + 1] = True
    # targeted frames (t % 6 in (0, 2)): u of the step is chosen so that the margin of THAT single step from these inputs is +-TARGET_DELTA -
    # the voicing decision then checks q1 - q0 to that accuracy. Only where the needed Gumbel difference keeps both uniforms well inside (0, 1)
    ws = controlled_weights(c["wset"])
    outs = [net_output(w_)[0] for w_ in ws]
    eps = np.where(valid, np.stack([outs[g][0] for g in net_of_item])[:, None], 0.0)
    logits = np.where(valid[..., None], np.stack([outs[g][1:] for g in net_of_item])[:, None, :], 0.0)
    target = np.zeros((S, B, T), bool)
    for s in range(S):
        half = np.full((B, 2, T), 0.5)
        _, _, m, _ = f0_joint_step(f0, uv, eps, logits, lo, hi, z[s], half, f0_coef(tables, s), s)    # g1 = g0: the margin is q1 - q0
        want = np.where(tt % 12 < 6, TARGET_DELTA, -TARGET_DELTA) - m          # g1 - g0
        ok = ((tt % 6 == 0) | (tt % 6 == 2)) & (np.abs(want) <= 10.0)
        g_small = -1.5
        u0 = _gumbel_inv(np.where(want >= 0, g_small, g_small - want))
        u1 = _gumbel_inv(np.where(want >= 0, g_small + want, g_small))
        u[s, :, 0][ok] = u0[ok].astype(np.float32)
        u[s, :, 1][ok] = u1[ok].astype(np.float32)
        target[s] = ok
    assert u.min() >= 0.0 and u.max() < 1.0
    return dict(name=name, B=B, T=T, S=S, lens=lens, net_of_item=net_of_item, valid=valid, f0=f0, uv=uv, lo=lo, hi=hi, z=z, u=u, cond=cond,
                weights=ws, regimes=dict(pin=pin, band=band, idle=~(pin | band), edge0=edge0, edge1=edge1, target=target,
                                         uv0=uv == 0, uv1=uv != 0, padded=~valid))


def swapped_items(case):
    """The same case with the two nets' items exchanged: what net 0 saw goes to net 1 and the other way round (paired cases)."""
    h = case["B"] // 2
    roll = lambda a, ax: np.roll(a, h, axis=ax)
    out = dict(case, name=case["name"] + "_swapped", lens=roll(case["lens"], 0), valid=roll(case["valid"], 0))
    for k in ("f0", "uv", "lo", "hi", "cond"):
        out[k] = np.ascontiguousarray(roll(case[k], 0))
    for k in ("z", "u"):
        out[k] = np.ascontiguousarray(roll(case[k], 1))
    out["regimes"] = {k: roll(v, 0 if v.ndim == 2 else 1) for k, v in case["regimes"].items()}
    out["regimes"]["target"] = np.zeros_like(case["regimes"]["target"])    # the uniforms were steered for the other net's logits
    return out


def controlled_step(case, tables, step, dtype=torch.float64):
    """The statement of step `step` alone on a case's inputs: network outputs in `dtype` (fp32: the dot product in fp32 numpy), zero on padded
    frames, then f0_joint_step in `dtype`. Returns dict(f0, uv, margin, mag, eps, logits, e_eps [B,T])."""
    np_dt = F64 if dtype == torch.float64 else np.float32
    nets = case["net_of_item"]
    outs = [net_output(w_, np_dt) for w_ in case["weights"]]
    valid = case["valid"]
    eps = np.where(valid, np.stack([outs[g][0][0] for g in nets])[:, None], 0.0)
    logits = np.where(valid[..., None], np.stack([outs[g][0][1:] for g in nets])[:, None, :], 0.0)
    e_eps = np.where(valid, np.stack([outs[g][1][0] for g in nets])[:, None], 0.0)
    f0n, uvn, margin, mag = f0_joint_step(case["f0"], case["uv"], eps, logits, case["lo"], case["hi"], case["z"][step], case["u"][step],
                                          f0_coef(tables, step), step, dtype=dtype)
    return dict(f0=f0n, uv=uvn, margin=margin, mag=mag, eps=eps, logits=logits, e_eps=e_eps)


def check_controlled_step(case, tables, step, f0_out, uv_out):
    """What the GPU test asserts of one step's outputs f0_out / uv_out [B,T] (and the CPU test of an fp32 emulation): returns
      f0_ratio   max |f0_out - statement| / bound over all frames (padded ones: the statement with eps = logits = 0, bound with e_eps = 0)
      flips      decided frames whose class differs from the statement's
      undecided  [B,T] bool, thr [B,T], cpu_margin_err, and the fp32-CPU step's own f0 error over its bound (a check of the bound itself)."""
    ref = controlled_step(case, tables, step)
    cpu = controlled_step(case, tables, step, dtype=torch.float32)
    thr, cpu_err = decision_threshold(ref["margin"], cpu["margin"], ref["mag"])
    undecided = np.abs(ref["margin"]) < thr
    bound = f0_step_bound(case["f0"], ref["eps"], case["lo"], case["hi"], case["z"][step], f0_coef(tables, step), step, ref["e_eps"])
    f0_out = np.asarray(f0_out, F64)
    finite = np.isfinite(f0_out)
    ratio = np.where(finite, np.abs(f0_out - ref["f0"]) / bound, np.inf)
    flips = (np.asarray(uv_out) != ref["uv"]) & ~undecided
    return dict(f0_ratio=float(ratio.max()), f0_err=float(np.abs(f0_out - ref["f0"])[finite].max(initial=0.0)), f0_bound=float(bound.max()),
                flips=int(flips.sum()), flip_mask=flips, undecided=undecided, thr=thr, cpu_margin_err=cpu_err, ref=ref,
                cpu_f0_ratio=float((np.abs(cpu["f0"] - ref["f0"]) / bound).max()))
