"""DPM-Solver++ multistep sampling of the mel diffusion (ss_meldiff_sample_dpmpp) stated in numpy float64, from the paper (Lu et al. 2022,
"DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", Algorithm 2: data prediction, 2M) and the definitions of
the issue that asked for the sampler - not from the kernel - with a derived fp32 bound, the closed-form Gaussian case that shows the order of
the method, and the wrong variants of each statement. The multistep counterpart of tests/mel_step_refs.py, whose step bound it continues.

Symbols: ac = cumprod(1 - betas) in double, alpha = sqrt(ac), sigma = sqrt(1 - ac), lambda = 1/2 log(ac / (1 - ac)) = log(alpha / sigma).
Visited times ts[0] > ... > ts[n-1]; transition i leaves t = ts[i] for s = ts[i+1], the last one for x_0 (ac_s = 1, lambda_s = inf).
  x0_i = clamp(recip_t x - recipm1_t eps, -1, 1)                       (the DDIM sampler's own x0 prediction)
  (c1, c2) = ddim_coef(ac_t, ac_s, 0) = (-alpha_s (e^-h - 1), sigma_s / sigma_t),  h = lambda_s - lambda_t
  order 1:  x' = c1 x0_i + c2 x                                        first transition, every transition of order = 1, always the last one
  order 2:  x' = b0 x0_i + b1 x0_{i-1} + c2 x,  r = (lambda_t - lambda_{ts[i-1]}) / h,  b0 = c1 (1 + 1/(2r)),  b1 = -c1 / (2r)
Rows t >= lens[b] of x' and of the stored x0 are 0.

No GPU, no HIP library. tests/test_dpmpp_refs_cpu.py checks the statements; tests/test_gpu_dpmpp.py holds the kernel to them.
"""
import math

import numpy as np

import mel_step_refs as MR

F64 = np.float64
U24 = MR.U24
VARIANTS = ("r_inverted", "b1_sign", "second_order_last")
SLACK = 1.0 + 2.0 ** -10    # the bounds below are first order in U24; this covers the products of two roundings (each some 2^-24 of a term)


def half_logsnr(ac):
    ac = np.asarray(ac, F64)
    return 0.5 * np.log(ac / (1.0 - ac))


def schedule_tables(betas):
    """The two fp32 tables the x0 prediction reads, built as the reference builds them (float64 from the betas, stored as fp32) and widened
    again, plus the float64 cumulative products: (tables, ac64)."""
    ac = np.cumprod(1.0 - np.asarray(betas, F64))
    f = lambda v: v.astype(np.float32).astype(F64)
    return dict(sqrt_recip_alphas_cumprod=f(np.sqrt(1.0 / ac)), sqrt_recipm1_alphas_cumprod=f(np.sqrt(1.0 / ac - 1.0))), ac


def dpmpp_coef(ac64, ts, i, order, tables=None, variant=None):
    """Coefficients of transition i in float64: dict(recip, recipm1, b0, b1, c2, second, last). `tables` (name -> fp32 table, widened): the x0
    prediction reads them at ts[i] as the sampler does; None = the exact float64 values 1 / alpha_t and sigma_t / alpha_t. `variant`: one of
    VARIANTS, a deliberately wrong statement for the tests that show the bound catches it."""
    assert order in (1, 2) and variant in (None,) + VARIANTS
    ts = [int(t) for t in ts]
    t, last = ts[i], i + 1 == len(ts)
    ac_t, ac_s = float(ac64[t]), 1.0 if last else float(ac64[ts[i + 1]])
    k = MR.ddim_coef(ac_t, ac_s, 0.0)
    c1, c2 = k["c1"], k["c2"]
    b0, b1, second = c1, 0.0, False
    if order == 2 and i > 0 and (not last or variant == "second_order_last"):
        lam_t, lam_p = float(half_logsnr(ac_t)), float(half_logsnr(ac64[ts[i - 1]]))
        if last:   # the wrong variant: a finite stand-in for h = inf, the previous gap again (r = 1)
            r = 1.0
        else:
            r = (lam_t - lam_p) / (float(half_logsnr(ac_s)) - lam_t)
        if variant == "r_inverted":
            r = 1.0 / r
        b0, b1, second = c1 * (1.0 + 1.0 / (2.0 * r)), -c1 / (2.0 * r), True
        if variant == "b1_sign":
            b1 = -b1
    if tables is None:
        recip, recipm1 = math.sqrt(1.0 / ac_t), math.sqrt(1.0 / ac_t - 1.0)
    else:
        recip, recipm1 = (float(np.asarray(tables[n], F64)[t]) for n in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"))
    return dict(recip=recip, recipm1=recipm1, b0=b0, b1=b1, c2=c2, second=second, last=last)


def _row_mask(shape, lens):
    return np.arange(shape[1])[None, :] >= np.asarray(lens).reshape(shape[0], 1)


def dpmpp_step(x, eps, x0_prev, coef, lens=None, dtype=F64, clamp=True):
    """One transition on x [B,T,M]: (x', x0). float64 is the statement; float32 is the same step in fp32 numpy on the CPU, coefficients cast
    once and every operation rounded (numpy does not fuse: at most as good as the kernel's fmas), the yardstick of the real-weights test."""
    x, eps = np.asarray(x, dtype), np.broadcast_to(np.asarray(eps, dtype), np.shape(x))
    k = {n: dtype(coef[n]) for n in ("recip", "recipm1", "b0", "b1", "c2")}
    x0 = k["recip"] * x - k["recipm1"] * eps
    if clamp:
        x0 = np.clip(x0, dtype(-1.0), dtype(1.0))
    out = k["b0"] * x0 + k["c2"] * x
    if coef["second"]:
        out = out + k["b1"] * np.asarray(x0_prev, dtype)
    if lens is not None:
        m = _row_mask(x.shape, lens)[..., None]
        out, x0 = np.where(m, dtype(0.0), out), np.where(m, dtype(0.0), x0)
    assert out.dtype == dtype and x0.dtype == dtype
    return out, x0


def dpmpp_step_bound(x, eps, x0_prev, coef, e_eps, e_x=0.0, e_prev=0.0, lens=None):
    """Bound on |fp32 result - dpmpp_step| for a sampler that evaluates x' = fma(b1, x0_prev, fma(b0, x0, fl(c2 x))) (order 1: without the outer
    fma) with x0 = clamp(fl(recip x) - fl(recipm1 eps)) from an x off by at most e_x, an eps off by at most e_eps, a stored previous x0 off by at
    most e_prev, the fp32 tables for recip / recipm1 and b0, b1, c2 cast from double to fp32. One rounding (U24 relative) each:
      x0:  recip*x, recipm1*eps, their difference (3; the clamp is exact and 1-Lipschitz; an element whose pre-clamp value is beyond a rail by more
           than its own error comes out as the rail, with none) - MR.mel_step_bound's x0 term
      q = c2*x: the cast of c2 and the product (2) ; p = b0*x0: the cast of b0 (1), the inner fma's result (1 on p + q)
      s = b1*x0_prev: the cast of b1 (1), the outer fma's result (1 on p + q + s)
    times SLACK for the second-order terms. Returns (bound on x', bound on the stored x0); rows >= lens[b] are exactly 0: bound 0."""
    x = np.asarray(x, F64)
    eps, e_eps, e_x = (np.broadcast_to(np.asarray(v, F64), x.shape) for v in (eps, e_eps, e_x))
    a, b = coef["recip"] * x, coef["recipm1"] * eps
    raw = a - b
    e0 = abs(coef["recip"]) * e_x + abs(coef["recipm1"]) * e_eps + U24 * (np.abs(a) + np.abs(b) + np.abs(raw))
    e0 = np.where((raw - e0 > 1.0) | (raw + e0 < -1.0), 0.0, e0)
    x0 = np.clip(raw, -1.0, 1.0)
    p, q = coef["b0"] * x0, coef["c2"] * x
    e = abs(coef["b0"]) * e0 + abs(coef["c2"]) * e_x + U24 * (np.abs(p) + 2.0 * np.abs(q) + np.abs(p + q))
    if coef["second"]:
        s = coef["b1"] * np.asarray(x0_prev, F64)
        e = e + abs(coef["b1"]) * np.broadcast_to(np.asarray(e_prev, F64), x.shape) + U24 * (np.abs(s) + np.abs(p + q + s))
    e, e0 = e * SLACK, e0 * SLACK
    if lens is not None:
        m = _row_mask(x.shape, lens)[..., None]
        e, e0 = np.where(m, 0.0, e), np.where(m, 0.0, e0)
    return e, e0


def run_dpmpp(x, net, ac64, ts, order, tables=None, lens=None, e_net=0.0, variant=None, dtype=F64, clamp=True, i_lo=0, i_hi=None, x0_prev=None):
    """Positions [i_lo, i_hi) of the list from the state x (and, for i_lo > 0, the x0 of position i_lo - 1). `net(x, t)` returns eps at network
    time t (an array that ignores x is the controlled net). The last position of the LIST is first order to x_0 through the DDIM step
    (MR.mel_step: the fused epilogue of the sampler). Returns dict(x, x0 = the history as the sampler leaves it, e_x / e_x0 = the bounds of
    the float64 run (dtype = float64 only), clamped = whether the clamp acted anywhere)."""
    x = np.asarray(x, dtype)
    n = len(ts)
    i_hi = n if i_hi is None else i_hi
    e_x = e_prev = 0.0
    clamped = False
    x0h = None if x0_prev is None else np.asarray(x0_prev, dtype)
    for i in range(i_lo, i_hi):
        k = dpmpp_coef(ac64, ts, i, order, tables, variant)
        eps = net(x, int(ts[i])) if callable(net) else net
        raw = F64(k["recip"]) * np.asarray(x, F64) - F64(k["recipm1"]) * np.asarray(eps, F64)
        clamped |= bool((np.abs(raw) > 1.0).any()) and clamp
        if k["last"] and not k["second"]:
            coef = dict(recip=k["recip"], recipm1=k["recipm1"], c1=k["b0"], c2=k["c2"], sigma=0.0)
            if dtype == F64:
                e_x = MR.mel_step_bound(x, eps, coef, 0.0, 0, e_net, lens=lens, e_x=e_x, coef_casts=True) * SLACK
            assert clamp
            x = MR.mel_step(x, eps, coef, np.zeros_like(x), 0, lens=lens, dtype=dtype)
            continue
        if dtype == F64:
            e_x, e_prev = dpmpp_step_bound(x, eps, x0h, k, e_net, e_x=e_x, e_prev=e_prev, lens=lens)
        x, x0h = dpmpp_step(x, eps, x0h, k, lens=lens, dtype=dtype, clamp=clamp)
    return dict(x=x, x0=x0h, e_x=e_x, e_x0=e_prev, clamped=clamped)


# ------------------------------------------------------------------------------------------------
# the Gaussian case: data N(mu, s^2), for which the optimal eps model is closed-form
# ------------------------------------------------------------------------------------------------
GAUSS = dict(mu=0.2, s=0.3, zs=(-2.0, -1.0, -0.3, 0.5, 1.3, 2.0))
BETAS100 = np.linspace(1e-4, 0.06, 100)


def gaussian_error(ac64, ts, order, variant=None, mu=GAUSS["mu"], s=GAUSS["s"], zs=GAUSS["zs"]):
    """x_0 ~ N(mu, s^2): x_t ~ N(alpha_t mu, alpha_t^2 s^2 + sigma_t^2) and E[eps | x_t] = sigma_t (x_t - alpha_t mu) / (alpha_t^2 s^2 + sigma_t^2).
    The probability-flow ODE maps the z-quantile of x_T to the z-quantile mu + s z of x_0. Start at the z-quantile of x_{ts[0]} for every z of `zs`,
    run the sampler in float64 with the exact eps model, and return (the largest |x - (mu + s z)|, whether the clamp acted)."""
    ac = np.asarray(ac64, F64)
    al, sg = np.sqrt(ac), np.sqrt(1.0 - ac)
    t0 = int(ts[0])
    z = np.asarray(zs, F64).reshape(1, -1, 1)
    x = al[t0] * mu + z * math.sqrt(al[t0] ** 2 * s * s + sg[t0] ** 2)
    net = lambda xx, t: sg[t] * (xx - al[t] * mu) / (al[t] ** 2 * s * s + sg[t] ** 2)
    out = run_dpmpp(x, net, ac, ts, order, variant=variant)
    return float(np.abs(out["x"] - (mu + s * z)).max()), out["clamped"]
