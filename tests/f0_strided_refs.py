"""The strided joint f0 / uv sampler (ss_f0diff_sample_strided, ss_f0_strided_coef) stated in numpy float64, from its definition and the
reference lines that definition continues (gaussian_multinomial_diffusion.py:237-284 multinomial / Gaussian schedules, :326-333 gaussian_p_sample,
:374-413 q_posterior / p_sample; Song et al. 2021 eq. 12 / 16 for the Gaussian gap) - not from the kernel. No GPU, no HIP library.

A run is a strictly decreasing list of network times; the transition t -> s has s = the next entry, and s = -1 ("final": x_0, cumprod alpha = 1,
Lambda = 0) after the last. With beta the checkpoint's fp32 betas widened, a = 1 - beta, ac = cumprod(a), Lambda = cumsum(log a):
  recip = sqrt(1/ac_t), recipm1 = sqrt(1/ac_t - 1)
  sigma = eta sqrt((1 - ac_s)/(1 - ac_t)) sqrt(1 - ac_t/ac_s), c2 = sqrt(max(1 - ac_s - sigma^2, 0)/(1 - ac_t)), c1 = sqrt(ac_s) - c2 sqrt(ac_t)
  log_alpha_t = Lambda_t - Lambda_s, log_1m_alpha_t = log(1 - exp(log_alpha_t) + 1e-40)
  log_cp_tm1 = Lambda_s, log_1m_cp_tm1 = log(1 - exp(Lambda_s) + 1e-40); the final transition applies no prior term.
The per-frame arithmetic is the classic step's (sampler_step_refs.f0_joint_step) with these numbers rounded to fp32 under the names of F0StepCoef,
`step` = 0 for the final transition and 1 otherwise, and the tape rows of network time t.
"""
import numpy as np
import torch

import sampler_step_refs as SR

F64 = np.float64
FINAL = -1
# the transitions of a 4-step schedule the tests run: every gap, from the top and from the middle, and the final one from time 0
TRANSITIONS = ((3, 0), (3, 1), (1, 0), (3, 2), (2, 0), (2, 1), (0, FINAL))
ETAS = (0.0, 0.5, 1.0)


def schedule(betas):
    """betas (the fp32 buffer) -> (betas, ac = cumprod(1 - betas), Lambda = cumsum(log(1 - betas))) in float64"""
    b = np.asarray(betas, np.float32).astype(F64)
    a = 1.0 - b
    return b, np.cumprod(a), np.cumsum(np.log(a))


def strided_coef(betas, t, s, eta):
    """The nine float64 coefficients of the transition t -> s (s = FINAL: to x_0) under the names of F0StepCoef."""
    _, ac, lam = schedule(betas)
    assert 0 <= t < len(ac) and FINAL <= s < t and 0.0 <= eta <= 1.0
    ac_t, lam_t = ac[t], lam[t]
    ac_s, lam_s = (ac[s], lam[s]) if s >= 0 else (1.0, 0.0)
    sigma = eta * np.sqrt((1.0 - ac_s) / (1.0 - ac_t)) * np.sqrt(1.0 - ac_t / ac_s)
    c2 = np.sqrt(max(1.0 - ac_s - sigma * sigma, 0.0) / (1.0 - ac_t))
    c1 = np.sqrt(ac_s) - c2 * np.sqrt(ac_t)
    la = lam_t - lam_s
    return dict(recip=float(np.sqrt(1.0 / ac_t)), recipm1=float(np.sqrt(1.0 / ac_t - 1.0)), c1=float(c1), c2=float(c2), sigma=float(sigma),
                log_alpha_t=float(la), log_1m_alpha_t=float(np.log(1.0 - np.exp(la) + 1e-40)),
                log_cp_tm1=float(lam_s), log_1m_cp_tm1=float(np.log(1.0 - np.exp(lam_s) + 1e-40)))


def coef32(coef):
    """the coefficients as the kernel receives them: rounded to fp32 (and widened again)"""
    return {k: float(np.float32(coef[k])) for k in SR.F0_COEF_KEYS}


def step_flag(s):
    """f0_joint_step's `step` argument: 0 = no prior term and no noise term (the final transition), anything else = both"""
    return 0 if s == FINAL else 1


def successors(ts):
    """[(t, s)] of a list of network times"""
    ts = list(ts)
    assert all(a > b for a, b in zip(ts, ts[1:])) and ts[-1] >= 0
    return list(zip(ts, ts[1:] + [FINAL]))


def timesteps(S, n):
    """The rule of the product (plans.ddim_timesteps with S = f0_timesteps): n points of linspace(0, S-1) rounded, descending, n clipped to
    [1, S]; a single point is S-1 (the state is x_{S-1})."""
    n = max(1, min(int(n), S))
    if n == 1:
        return [S - 1]
    return sorted({int(round(v)) for v in np.linspace(0, S - 1, n)}, reverse=True)


def strided_step(f0, uv, eps, logits, lo, hi, z_tape, u_tape, betas, t, s, eta, dtype=torch.float64):
    """One transition for every frame: f0_joint_step with the fp32-rounded strided coefficients and the tape rows of time t.
    z_tape [S,B,T], u_tape [S,B,2,T]. Returns (f0_new, uv_new, margin, mag)."""
    return SR.f0_joint_step(f0, uv, eps, logits, lo, hi, z_tape[t], u_tape[t], coef32(strided_coef(betas, t, s, eta)), step_flag(s), dtype=dtype)


# ------------------------------------------------------------------------------------------------
# the multinomial gap by brute force (K classes, uniform transitions)
# ------------------------------------------------------------------------------------------------
def transition_matrix(a, K=2):
    """Q[i, j] = q(x_i = j | x_{i-1} = i): keep with probability a, else uniform over the K classes"""
    return a * np.eye(K) + (1.0 - a) / K * np.ones((K, K))


def posterior_brute(betas, t, s, K=2):
    """q(x_s = k | x_t = j, x0 = i) [i, j, k] from products of the per-step matrices: q(x_t | x_s) = Q_{s+1} ... Q_t, q(x_s | x0) = Q_0 ... Q_s
    (the identity for s = FINAL)."""
    b = schedule(betas)[0]
    prod = lambda lo_, hi_: np.linalg.multi_dot([np.eye(K), np.eye(K)] + [transition_matrix(1.0 - b[i], K) for i in range(lo_, hi_ + 1)])
    to_s, s_to_t = prod(0, s), prod(s + 1, t)
    un = to_s[:, None, :] * s_to_t.T[None, :, :]      # [i, j, k] = q(x_s = k | x0 = i) q(x_t = j | x_s = k)
    return un / un.sum(-1, keepdims=True)


def posterior_closed(coef, s, K=2):
    """The same table from the coefficients of the definition: (ac_s [k = i] + (1 - ac_s)/K) (a_{t|s} [k = j] + (1 - a_{t|s})/K), normalised;
    the final transition has no prior term: x0 itself."""
    eye = np.eye(K)
    like = np.exp(coef["log_alpha_t"]) * eye + np.exp(coef["log_1m_alpha_t"]) / K              # [j, k]
    prior = eye if s == FINAL else np.exp(coef["log_cp_tm1"]) * eye + np.exp(coef["log_1m_cp_tm1"]) / K    # [i, k]
    un = prior[:, None, :] * like[None, :, :]
    return un / un.sum(-1, keepdims=True)


# ------------------------------------------------------------------------------------------------
# the controlled cases of sampler_step_refs under a strided transition
# ------------------------------------------------------------------------------------------------
def _net_outputs(case, np_dt):
    nets, valid = case["net_of_item"], case["valid"]
    outs = [SR.net_output(w_, np_dt) for w_ in case["weights"]]
    eps = np.where(valid, np.stack([outs[g][0][0] for g in nets])[:, None], 0.0)
    logits = np.where(valid[..., None], np.stack([outs[g][0][1:] for g in nets])[:, None, :], 0.0)
    e_eps = np.where(valid, np.stack([outs[g][1][0] for g in nets])[:, None], 0.0)
    return eps, logits, e_eps


def steer(case, betas, t, s, eta):
    """The case with the uniforms of tape row t steered for the transition t -> s as controlled_case steers them for the classic step: on the
    targeted frames (t % 6 in (0, 2)) the margin of this one transition from the case's inputs is +-TARGET_DELTA. Returns a new case (the input is
    left unchanged); regimes['target'][t] holds the frames steered here."""
    B, T = case["B"], case["T"]
    tt = np.broadcast_to(np.arange(T)[None, :], (B, T))
    eps, logits, _ = _net_outputs(case, F64)
    half = np.full((case["S"], B, 2, T), 0.5)
    _, _, m, _ = strided_step(case["f0"], case["uv"], eps, logits, case["lo"], case["hi"], case["z"], half, betas, t, s, eta)
    want = np.where(tt % 12 < 6, SR.TARGET_DELTA, -SR.TARGET_DELTA) - m
    ok = ((tt % 6 == 0) | (tt % 6 == 2)) & (np.abs(want) <= 10.0) & case["regimes"]["target"].any()      # none for a swapped variant
    g_small = -1.5
    u0 = SR._gumbel_inv(np.where(want >= 0, g_small, g_small - want))
    u1 = SR._gumbel_inv(np.where(want >= 0, g_small + want, g_small))
    u = case["u"].copy()
    u[t, :, 0][ok] = u0[ok].astype(np.float32)
    u[t, :, 1][ok] = u1[ok].astype(np.float32)
    assert u.min() >= 0.0 and u.max() < 1.0
    target = case["regimes"]["target"].copy()
    target[t] = ok
    return dict(case, u=u, regimes=dict(case["regimes"], target=target))


def controlled_strided_step(case, betas, t, s, eta, dtype=torch.float64):
    """The statement of the transition t -> s alone on a case's inputs (sampler_step_refs.controlled_step with the strided coefficients)."""
    eps, logits, e_eps = _net_outputs(case, F64 if dtype == torch.float64 else np.float32)
    f0n, uvn, margin, mag = strided_step(case["f0"], case["uv"], eps, logits, case["lo"], case["hi"], case["z"], case["u"], betas, t, s, eta, dtype=dtype)
    return dict(f0=f0n, uv=uvn, margin=margin, mag=mag, eps=eps, logits=logits, e_eps=e_eps)


def check_strided_step(case, betas, t, s, eta, f0_out, uv_out):
    """sampler_step_refs.check_controlled_step for a strided transition: the same bound (f0_step_bound), the same decision threshold."""
    ref = controlled_strided_step(case, betas, t, s, eta)
    cpu = controlled_strided_step(case, betas, t, s, eta, dtype=torch.float32)
    thr, cpu_err = SR.decision_threshold(ref["margin"], cpu["margin"], ref["mag"])
    undecided = np.abs(ref["margin"]) < thr
    bound = SR.f0_step_bound(case["f0"], ref["eps"], case["lo"], case["hi"], case["z"][t], coef32(strided_coef(betas, t, s, eta)), step_flag(s), ref["e_eps"])
    f0_out = np.asarray(f0_out, F64)
    finite = np.isfinite(f0_out)
    ratio = np.where(finite, np.abs(f0_out - ref["f0"]) / bound, np.inf)
    flips = (np.asarray(uv_out) != ref["uv"]) & ~undecided
    return dict(f0_ratio=float(ratio.max()), f0_err=float(np.abs(f0_out - ref["f0"])[finite].max(initial=0.0)), f0_bound=float(bound.max()),
                flips=int(flips.sum()), flip_mask=flips, undecided=undecided, thr=thr, cpu_margin_err=cpu_err, ref=ref,
                cpu_f0_ratio=float((np.abs(cpu["f0"] - ref["f0"]) / bound).max()))
