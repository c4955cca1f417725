"""The float64 statements of tests/mel_step_refs.py checked on their own (no GPU) against the oracle (oracle/restatement.py) in float64, so that
a wrong reference cannot pass a wrong kernel; the input conditions tests/test_gpu_mel_sampler_steps.py relies on, asserted from the case table
alone (every clamp regime is populated at every step, the dyadic projection is exact in any order, the bound holds an fp32 emulation of the
step); and each wrong variant of a statement leaving the bound on the table's own inputs - the cases can see the error."""
import math

import numpy as np
import pytest
import torch

import mel_step_refs as MR
import sampler_step_refs as SR
from oracle import restatement as O
from stylesinger_amd import config, synth

F64, f32 = np.float64, np.float32
K = MR.K_MEL
P = "postdiff."
_CACHE = {}


def _hp(**over):
    return config.make_hparams(dict(dict(timesteps=K, K_step=K, f0_timesteps=4), **over))


def _sd64(**over):
    key = tuple(sorted(over.items()))
    if key not in _CACHE:
        sd = synth.synth_acoustic_state_dict(_hp(**over), 77)
        _CACHE[key] = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return _CACHE[key]


def _tables(sd=None, prefix=P):
    """the fp32 schedule buffers of a state dict, widened (the float64 state dict holds exactly these values)"""
    sd = sd or _sd64()
    return {k[len(prefix):]: v.numpy() for k, v in sd.items() if k.startswith(prefix) and "denoise_fn" not in k and v.dim() == 1}


class _f64:
    """torch's default dtype for the oracle's own constants"""

    def __enter__(self):
        torch.set_default_dtype(torch.float64)

    def __exit__(self, *a):
        torch.set_default_dtype(torch.float32)


class _Tape64(synth.NoiseTape):
    """the tape's fp32 draws, widened: a 0-dim float64 coefficient times an fp32 tensor is an fp32 product in torch, and the oracle would round there"""

    def randn(self, *shape):
        return super().randn(*shape).double()


def _close(a, b, what, rel=1e-12):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    err, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
    assert scale > 0.1 and err <= rel * scale, f"{what}: {err:.3e} against {rel * scale:.3e}"


def _inputs(B=1, T=6, seed=6):
    g = torch.Generator().manual_seed(seed)
    coarse = (torch.randn(B, T, MR.M_MEL, generator=g) * 0.8 - 3.0).double()
    cond = (torch.randn(B, T, 256, generator=g) * 0.5).double()
    return coarse, cond


def _btm(z):
    return z[:, 0].transpose(1, 2).double().numpy()


def _diffnet(sd, hp, x, t, cond, prefix="postdiff.denoise_fn"):
    with torch.no_grad():
        return O.diffnet(sd, hp, torch.from_numpy(np.ascontiguousarray(x)), torch.full((x.shape[0],), int(t), dtype=torch.long), cond, prefix=prefix).numpy()


def _qsample(sd, coarse, tape, k_step=K):
    t = lambda k: sd[P + k].numpy()
    smin, smax = t("spec_min")[0, 0], t("spec_max")[0, 0]
    B, T, M = coarse.shape
    x, _ = SR.mel_qsample(coarse.numpy(), smin, smax, t("sqrt_alphas_cumprod")[k_step - 1], t("sqrt_one_minus_alphas_cumprod")[k_step - 1],
                          _btm(tape.randn(B, 1, M, T)))
    return x, smin, smax


# ------------------------------------------------------------------------------------------------
# the statements against the oracle, in float64
# ------------------------------------------------------------------------------------------------
def test_tables_are_the_schedule():
    ref = synth.gaussian_schedule(K, _hp()["max_beta"])
    t = _tables()
    for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped"):
        assert np.array_equal(t[k], ref[k].double().numpy()), k
    c0 = MR.mel_coef_ddpm(t, 0)
    assert c0["sigma"] == 0.0 and math.exp(0.5 * t["posterior_log_variance_clipped"][0]) > 0     # the table's own entry at t = 0 is NOT zero


def test_mel_step_chain_is_mel_diffusion():
    hp, sd = _hp(), _sd64()
    coarse, cond = _inputs(B=2)
    trace = []
    with _f64(), torch.no_grad():
        mel = O.mel_diffusion(sd, hp, coarse, cond, _Tape64(8), trace=trace)
        tape = _Tape64(8)
        x, smin, smax = _qsample(sd, coarse, tape)
        for (i, x_or) in trace:
            eps = _diffnet(sd, hp, x, i, cond)
            x = MR.mel_step(x, eps, MR.mel_coef_ddpm(_tables(), i), _btm(tape.randn(*coarse.shape[:1], 1, MR.M_MEL, coarse.shape[1])), i)
            _close(x, x_or.numpy(), f"step {i}")
    assert [i for i, _ in trace] == list(reversed(range(K)))
    _close(SR.mel_denorm(x, smin, smax)[0], mel.numpy(), "denorm")


@pytest.mark.parametrize("ts,eta", [((3, 1), 0.0), ((2, 0), 0.0), ((3, 2, 1, 0), 1.0), ((3, 2, 0), 0.5)])
def test_ddim_coef_chain_is_mel_ddim(ts, eta):
    """the oracle applies its coefficients rounded to fp32, as the sampler does: so does the chain (mel_coef_ddim's cast)"""
    hp, sd = _hp(), _sd64()
    coarse, cond = _inputs()
    ac64 = np.cumprod(1.0 - sd[P + "betas"].numpy())
    with _f64(), torch.no_grad():
        mel = O.mel_ddim(sd, hp, coarse, cond, _Tape64(9), list(ts), eta=eta)
        tape = _Tape64(9)
        x, smin, smax = _qsample(sd, coarse, tape)
        for i, t in enumerate(ts):
            coef = MR.mel_coef_ddim(_tables(), ac64, ts, i, eta)
            z = _btm(tape.randn(1, 1, MR.M_MEL, coarse.shape[1])) if eta > 0 else np.zeros_like(x)
            x = MR.mel_step(x, _diffnet(sd, hp, x, t, cond), coef, z, 1 if eta > 0 else 0)
    _close(SR.mel_denorm(x, smin, smax)[0], mel.numpy(), f"ddim {ts} eta {eta}")
    last = MR.ddim_coef(ac64[ts[-1]], 1.0, eta)
    assert last == dict(c1=1.0, c2=0.0, sigma=0.0)       # the last transition lands on x0 itself
    # eta = 1 over every step is the ancestral posterior (:136-162): the schedule's own coefficients
    if eta == 1.0:
        full = synth.gaussian_schedule(K, hp["max_beta"])
        for i, t in enumerate(ts[:-1]):
            k = MR.ddim_coef(ac64[t], ac64[ts[i + 1]], 1.0)
            assert abs(k["c1"] - float(full["posterior_mean_coef1"][t])) < 1e-6 and abs(k["c2"] - float(full["posterior_mean_coef2"][t])) < 1e-6
            assert abs(k["sigma"] - math.exp(0.5 * float(full["posterior_log_variance_clipped"][t]))) < 1e-6


@pytest.mark.parametrize("k_step,interval", [(K, 1), (K, 2), (K, 3), (MR.K_PLMS, 1)])
def test_plms_step_chain_is_mel_plms(k_step, interval):
    """At K_step = 4 the call with four history entries is the one at t = 0, whose previous time is 0 too: a_prev = a_t and the update is the
    identity, whatever eps' is. K_step = 5 puts the fourth-order combination on t = 1."""
    over = dict(timesteps=k_step, K_step=k_step)
    hp, sd = _hp(**over), _sd64(**over)
    coarse, cond = _inputs()
    ac = sd[P + "alphas_cumprod"].numpy()
    moved = []
    with _f64(), torch.no_grad():
        mel = O.mel_plms(sd, hp, coarse, cond, _Tape64(10), interval)
        x, smin, smax = _qsample(sd, coarse, _Tape64(10), k_step)
        hist = []
        for t, tp in MR.plms_times(k_step, interval):
            hist = ([_diffnet(sd, hp, x, t, cond)] + hist)[:4]
            x_new = MR.plms_step(x, hist, ac[t], ac[tp], second_eval=lambda xp: _diffnet(sd, hp, xp, tp, cond))
            moved.append((len(hist), bool(np.abs(x_new - x).max() > 1e-3)))
            x = x_new
    assert MR.plms_times(K, 1) == [(3, 2), (2, 1), (1, 0), (0, 0)] and MR.plms_times(K, 2) == [(2, 0), (0, 0)]
    assert moved[-1][1] is False and all(m for _, m in moved[:-1])             # the call at t = 0 moves nothing; every other one does
    assert ((4, True) in moved) == (k_step == MR.K_PLMS)
    _close(SR.mel_denorm(x, smin, smax)[0], mel.numpy(), f"plms K {k_step} interval {interval}")


def test_x0_pred_chain_is_prodiff_sample():
    over = dict(decoder="prodiff", schedule_type="vpsde")
    hp, sd = _hp(**over), _sd64(**over)
    tables = _tables(sd, "diff_decoder.")
    _, cond = _inputs(B=2)
    trace = []
    with _f64(), torch.no_grad():
        out = O.prodiff_sample(sd, hp, cond, _Tape64(11), trace=trace)
        tape = _Tape64(11)
        shape = (2, 1, MR.M_MEL, cond.shape[1])
        x = _btm(tape.randn(*shape))
        seen = 0.0
        for (i, x_or) in trace:
            x0 = _diffnet(sd, hp, x, i, cond, prefix="diff_decoder.denoise_fn")
            seen = max(seen, float(np.abs(x0).max()))
            x = MR.mel_step(x, x0, MR.mel_coef_ddpm(tables, i), _btm(tape.randn(*shape)), i, x0_pred=True)
            _close(x, x_or.numpy(), f"prodiff step {i}")
    _close(x, out.numpy(), "prodiff")
    assert len(trace) == K


def test_mel_input_row_is_diffnets_input():
    sd = _sd64()
    p = "postdiff.denoise_fn.input_projection."
    r = np.random.default_rng(3)
    x = r.standard_normal((2, 9, MR.M_MEL))
    with _f64():
        ref = torch.relu(O.conv1d_cl(torch.from_numpy(x), sd[p + "weight"], sd[p + "bias"])).numpy()
    X = MR.mel_input_row(x, sd[p + "weight"][:, :, 0].numpy(), sd[p + "bias"].numpy(), lens=[9, 4])
    assert X.shape == (2, 9, MR.C_MEL) and np.all(X[1, 4:] == 0) and (X == 0).mean() > 0.2 and (X > 0).mean() > 0.2
    _close(X[0], ref[0], "input row")
    _close(X[1, :4], ref[1, :4], "input row, ragged")


# ------------------------------------------------------------------------------------------------
# input conditions of the GPU test
# ------------------------------------------------------------------------------------------------
def _case(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _CACHE:
        _CACHE[key] = MR.controlled_mel_case(name, _tables(), **kw)
    return _CACHE[key]


def test_the_dyadic_projection_is_exact_in_any_order_and_bears_load():
    w = MR.controlled_mel_weights("dyadic")
    assert (w["beta"] > 0).sum() > 80 and (w["beta"] < 0).sum() > 80         # the ReLU bears load
    eps, e_eps = MR.net_output(w)
    g = np.maximum(w["beta"], 0).astype(f32)
    fwd, rev = np.zeros(MR.M_MEL, f32), np.zeros(MR.M_MEL, f32)
    for k in range(MR.C_MEL):                                                   # two sequential fp32 orders, every partial sum rounded
        fwd = (fwd + w["w_final"][:, k] * g[k]).astype(f32)
        rev = (rev + w["w_final"][:, MR.C_MEL - 1 - k] * g[MR.C_MEL - 1 - k]).astype(f32)
    assert np.array_equal(fwd.astype(F64) + w["b_final"], eps) and np.array_equal(rev, fwd)
    assert np.array_equal((fwd + w["b_final"]).astype(F64), eps)               # ... and the bias add
    assert np.abs(w["w_final"].astype(F64)).dot(g.astype(F64)).max() < 64.0     # no partial sum of any order leaves 2^6
    assert (np.abs(eps) > 1.2).sum() >= 5 and (np.abs(eps) < 0.8).sum() >= 5    # x0-prediction: the output passes +-1 on some bins, not on others
    no_relu = w["w_final"].astype(F64) @ w["beta"].astype(F64) + w["b_final"]
    assert np.abs(no_relu - eps).min() > 1e-3                                   # a stack output without the ReLU shows on every bin
    for k, grid in (("beta", 8), ("w_final", 256), ("b_final", 64)):
        assert np.array_equal(w[k] * grid, np.round(w[k] * grid)) and np.abs(w[k]).max() <= 2.0
    assert np.all(e_eps == 0)                                                   # ... which is why the table's eps carries no error term
    r = MR.controlled_mel_weights("random")
    assert not np.array_equal(r["w_final"] * 256, np.round(r["w_final"] * 256)) and np.all(MR.net_output(r)[1] > 0)


@pytest.mark.parametrize("name", sorted(MR.CASES))
def test_controlled_cases_populate_every_regime(name):
    tables = _tables()
    case = _case(name)
    valid = np.broadcast_to(case["valid"][..., None], case["x"][0].shape)
    assert (~case["valid"]).any() and case["steps"] == (K - 1, 1, 0)
    for step in case["steps"]:
        coef = MR.mel_coef_ddpm(tables, step)
        masks, raw = MR.regime_masks(case["x"][step], coef, case["eps"])
        assert set(masks) == set(MR.REGIMES)
        total = sum(m.astype(int) for m in masks.values())
        assert np.all(total[valid] == 1), "an element sits exactly on a rail or in two regimes"
        for k, m in masks.items():
            assert int((m & valid).sum()) >= 20, (name, step, k, int((m & valid).sum()))
            for b in range(case["B"]):          # every item sees every regime, the one-frame item too
                assert (m & valid)[b].any(), (name, step, k, b)
        ref, bound = MR.controlled_step(case, tables, step)
        assert np.all(ref[~valid] == 0) and np.all(bound[~valid] == 0) and np.all(bound[valid] > 0)
        # the bound is far below what the regimes are apart by, and the near-rail elements are nearer to the rail than the bound on x0
        assert bound.max() < 1e-3
    tape = MR.noise_tape(case)
    assert np.all(tape[0] == 1e30) and np.array_equal(tape[K - 1], case["z_of"][K - 1]) and np.all(tape[2] == 3.0)


def _emulate(x, eps32, coef, z, step, x0_pred=False, lens=None):
    """ss_ddpm_update as common.h documents its roundings, in fp32 numpy: fl(recip x) - fl(recipm1 eps), the clamp, fma(c1, x0, fl(c2 x)),
    + fl(sigma z). The fused multiply-add goes through float64 (the product of two fp32 values is exact there)."""
    k = {n: f32(coef[n]) for n in MR.MEL_COEF_KEYS}
    x, eps32 = np.asarray(x, f32), np.broadcast_to(np.asarray(eps32, f32), np.shape(x))
    x0 = eps32 if x0_pred else np.clip(k["recip"] * x - k["recipm1"] * eps32, f32(-1), f32(1))
    mean = (F64(k["c1"]) * x0.astype(F64) + (k["c2"] * x).astype(F64)).astype(f32)
    out = mean + (k["sigma"] * np.asarray(z, f32) if step > 0 else f32(0))
    if lens is not None:
        out = np.where(MR._row_mask(x.shape, lens)[..., None], f32(0), out)
    return out.astype(f32)


@pytest.mark.parametrize("wset", ["dyadic", "random"])
def test_the_bound_holds_an_fp32_emulation_of_the_step(wset):
    """not a tolerance taken from an implementation: a check that the derived bound is not short of a rounding. The emulation's sigma is
    expf in fp32 (numpy's), its eps the fp32 matrix product."""
    tables = _tables()
    for name in sorted(MR.CASES):
        case = _case(name, wset=wset)
        w = case["weights"]
        eps32 = (w["w_final"] @ np.maximum(w["beta"], 0) + w["b_final"]).astype(f32)
        for step in case["steps"]:
            coef = MR.mel_coef_ddpm(tables, step)
            if step > 0:
                coef = dict(coef, sigma=float(np.exp(f32(0.5) * f32(tables["posterior_log_variance_clipped"][step]))))
            z = MR.noise_tape(case)[step]
            out = _emulate(case["x"][step], eps32, coef, z, step, lens=case["lens"])
            ref, bound = MR.controlled_step(case, tables, step)
            ratio, bad = MR.over_bound(out, ref, bound)
            assert bad == 0 and 0.0 < ratio <= 1.0, (name, step, ratio, bad)
            outp = _emulate(case["x"][step], eps32, coef, z, step, x0_pred=True, lens=case["lens"])
            refp, boundp = MR.controlled_step(case, tables, step, x0_pred=True)
            assert MR.over_bound(outp, refp, boundp)[1] == 0, (name, step, "x0_pred")


# ------------------------------------------------------------------------------------------------
# sensitivity: each wrong variant of a statement leaves the bound on the table's own inputs
# ------------------------------------------------------------------------------------------------
def _caught(out, ref, bound, where=None):
    bad = np.abs(np.asarray(out, F64) - ref) > bound
    return int((bad if where is None else bad & where).sum())


@pytest.mark.parametrize("name", sorted(MR.CASES))
def test_wrong_variants_of_the_step_are_caught(name):
    tables = _tables()
    case = _case(name)
    tape = MR.noise_tape(case)
    lens, eps = case["lens"], case["eps"]
    valid = np.broadcast_to(case["valid"][..., None], case["x"][0].shape)
    seen = {}
    for step in case["steps"]:
        x, coef = case["x"][step], MR.mel_coef_ddpm(tables, step)
        ref, bound = MR.controlled_step(case, tables, step)
        assert _caught(ref, ref, bound) == 0
        if step > 0:    # the noise slab of t - 1
            seen[("slab", step)] = _caught(MR.mel_step(x, eps, coef, tape[step - 1], step, lens=lens), ref, bound, valid)
        raw = coef["c1"] * (coef["recip"] * x.astype(F64) - coef["recipm1"] * eps) + coef["c2"] * x + (coef["sigma"] * tape[step].astype(F64) if step else 0.0)
        seen[("no_clamp", step)] = _caught(np.where(valid, raw, 0.0), ref, bound, valid)
        refp, boundp = MR.controlled_step(case, tables, step, x0_pred=True)
        clamped = MR.mel_step(x, np.clip(eps, -1.0, 1.0), coef, tape[step], step, x0_pred=True, lens=lens)
        seen[("clamp_under_x0_pred", step)] = _caught(clamped, refp, boundp, valid)
        if step == 0:   # sigma applied at t = 0: the table's own entry, exp(0.5 log 1e-20) = 1e-10, on the slab of 1e30
            sig0 = math.exp(0.5 * tables["posterior_log_variance_clipped"][0])
            seen[("sigma_at_0", 0)] = _caught(ref + np.where(valid, sig0 * tape[0].astype(F64), 0.0), ref, bound, valid)
        seen[("no_row_mask", step)] = _caught(MR.mel_step(x, eps, coef, tape[step], step), ref, bound, ~valid)
    for k, n in seen.items():
        assert n > 0, f"{name}: variant {k} stays inside the bound everywhere"


def test_wrong_variants_of_plms_are_caught():
    """On the controlled net every history entry is the same eps and every order collapses to it: the ring is only visible with a history
    that differs per slot - here random ones on a case's own x, in the GPU test the real weights."""
    case = _case("odd")
    x = case["x"][K - 1]
    ac = _sd64()[P + "alphas_cumprod"].numpy()
    r = np.random.default_rng(5)
    h = [r.standard_normal(x.shape).astype(f32) for _ in range(5)]
    a_t, a_p = ac[1], ac[0]
    for n in (2, 3, 4):
        ref, bound = MR.plms_step(x, h[:n], a_t, a_p), MR.plms_step_bound(x, h[:n], a_t, a_p)
        assert _caught(ref, ref, bound) == 0 and bound.max() < 1e-5
        assert _caught(MR.plms_step(x, [h[0]] + h[2:n + 1], a_t, a_p), ref, bound) > 0, f"history shifted by one slot, {n} entries"
        assert _caught(MR.plms_step(x, h[:n - 1], a_t, a_p), ref, bound) > 0, f"order one too low, {n} entries"
        if n < 4:
            assert _caught(MR.plms_step(x, h[:n + 1], a_t, a_p), ref, bound) > 0, f"order one too high, {n} entries"
    # the first call: the plain predictor for the average of the two evaluations
    ref = MR.plms_step(x, h[:1], a_t, a_p, second_eval=lambda xp: h[1])
    assert _caught(MR.plms_step(x, h[:1], a_t, a_p, second_eval=lambda xp: h[0]), ref, MR.plms_step_bound(x, [MR.plms_prime(h[:1], h[1])], a_t, a_p)) > 0
    # fp32 emulation of the update passes its bound
    k = {n_: f32(v) for n_, v in MR.plms_coef(a_t, a_p).items()}
    prime = ((f32(55) * h[0] - f32(59) * h[1] + f32(37) * h[2] - f32(9) * h[3]) / f32(24)).astype(f32)
    out = x + k["d"] * (k["kx"] * x - k["ke"] * prime)
    assert out.dtype == f32 and _caught(out, MR.plms_step(x, h[:4], a_t, a_p), MR.plms_step_bound(x, h[:4], a_t, a_p)) == 0


@pytest.mark.parametrize("ts,eta", [((3, 1), 0.0), ((2, 0), 0.0), ((3, 2, 0), 0.5)])
def test_wrong_variants_of_the_ddim_transitions_are_caught(ts, eta):
    tables = _tables()
    case = _case("odd", steps=(3, 2, 1, 0))
    ac64 = np.cumprod(1.0 - _sd64()[P + "betas"].numpy())
    tape = MR.noise_tape(case)
    valid = np.broadcast_to(case["valid"][..., None], case["x"][0].shape)

    def chain(coef_of, casts=True):
        steps = []
        for i, t in enumerate(ts):
            c = coef_of(i)
            steps.append(dict(coef=c, z=tape[t], step=1 if c["sigma"] != 0 else 0, sigma_ulps=0, coef_casts=casts))
        return MR.run_steps(case["x"][ts[0]], case["eps"], case["e_eps"], steps, lens=case["lens"])

    right = lambda i: MR.mel_coef_ddim(tables, ac64, ts, i, eta, cast=None)
    ref, bound = chain(right)
    assert _caught(chain(lambda i: MR.mel_coef_ddim(tables, ac64, ts, i, eta))[0], ref, bound) == 0       # the fp32 casts are inside the bound

    def prev_at_ts_i(i):    # ac_prev taken at ts[i]: the identity transition
        return dict(right(i), **MR.ddim_coef(ac64[ts[i]], ac64[ts[i]] if i + 1 < len(ts) else 1.0, eta))

    def last_not_to_one(i):   # the last transition stops at the next lower network time's ac (ac[0] from t = 0 itself)
        if i + 1 < len(ts):
            return right(i)
        return dict(right(i), **MR.ddim_coef(ac64[ts[i]], ac64[max(ts[i] - 1, 0)] if ts[i] > 0 else math.sqrt(ac64[0]), eta))

    assert _caught(chain(prev_at_ts_i)[0], ref, bound, valid) > 0
    assert _caught(chain(last_not_to_one)[0], ref, bound, valid) > 0
    if eta > 0:      # the slab of transition i instead of network time t
        steps = [dict(coef=right(i), z=tape[i], step=1 if right(i)["sigma"] != 0 else 0) for i, t in enumerate(ts)]
        assert _caught(MR.run_steps(case["x"][ts[0]], case["eps"], case["e_eps"], steps, lens=case["lens"])[0], ref, bound, valid) > 0


def test_nonzero_padding_columns_of_w_in_are_caught():
    """The packed input projection is [C][Kp_in = 96], zero beyond M = 80, and a reader that takes 96 values of a frame runs 16 into the next one:
    harmless only while the padding columns are zero."""
    case = _case("slices")
    x = case["x"][K - 1]
    sd = _sd64()
    w = sd["postdiff.denoise_fn.input_projection.weight"][:, :, 0].numpy().astype(f32)
    b = sd["postdiff.denoise_fn.input_projection.bias"].numpy().astype(f32)
    ref, bound = MR.mel_input_row(x, w, b, lens=case["lens"]), MR.mel_input_row_bound(x, w, b)
    flat = np.concatenate([x.reshape(-1), np.zeros(MR.KP_IN, f32)])
    rows = np.stack([flat[i * MR.M_MEL:i * MR.M_MEL + MR.KP_IN] for i in range(x.shape[0] * x.shape[1])]).reshape(x.shape[0], x.shape[1], MR.KP_IN)
    w96 = np.concatenate([w, np.zeros((MR.C_MEL, MR.KP_IN - MR.M_MEL), f32)], axis=1)
    assert _caught(MR.mel_input_row(rows, w96, b, lens=case["lens"]), ref, bound) == 0       # zero padding: the over-read is harmless
    w96[:, MR.M_MEL:] = 0.01
    assert _caught(MR.mel_input_row(rows, w96, b, lens=case["lens"]), ref, bound) > 0
    out32 = np.maximum(x @ w.T + b, 0).astype(f32)
    assert _caught(np.where(MR._row_mask(x.shape, case["lens"])[..., None], 0, out32), ref, bound) == 0


def test_extreme_schedule_case():
    """The 1000-step schedule of BASELINE config 4 (timesteps = K_step = 1000, max_beta = 0.06): at t = 999 sqrt(1 / ac - 1) is in the millions, one
    fp32 step of x moves the pre-clamp x0 by a good part of the rails' distance and the clamp decides nearly every element; at t = 1 the
    coefficients are benign and every regime is there. The bound follows the coefficients per element."""
    sched = {k: v.double().numpy() for k, v in synth.gaussian_schedule(1000, 0.06).items()}
    spec = dict(MR.EXTREME, name="extreme")
    case = MR.controlled_mel_case(spec, sched, steps=(999, 1))
    valid = np.broadcast_to(case["valid"][..., None], case["x"][999].shape)
    c999 = MR.mel_coef_ddpm(sched, 999)
    assert c999["recipm1"] > 1e6
    masks, raw = MR.regime_masks(case["x"][999], c999, case["eps"])
    assert (masks["below"] & valid).sum() > 100 and (masks["above"] & valid).sum() > 100 and (masks["inside"] & valid).sum() > 100
    masks1, _ = MR.regime_masks(case["x"][1], MR.mel_coef_ddpm(sched, 1), case["eps"])
    assert all((m & valid).sum() >= 20 for m in masks1.values())
    w = case["weights"]
    eps32 = (w["w_final"] @ np.maximum(w["beta"], 0) + w["b_final"]).astype(f32)
    for step in (999, 1):
        coef = MR.mel_coef_ddpm(sched, step)
        z = case["z_of"][step]
        ref = MR.mel_step(case["x"][step], case["eps"], coef, z, step, lens=case["lens"])
        bound = MR.mel_step_bound(case["x"][step], case["eps"], coef, z, step, case["e_eps"], lens=case["lens"])
        c32 = dict(coef, sigma=float(np.exp(f32(0.5) * f32(sched["posterior_log_variance_clipped"][step]))))
        assert MR.over_bound(_emulate(case["x"][step], eps32, c32, z, step, lens=case["lens"]), ref, bound)[1] == 0
        assert bound[valid].max() < 1e-5 * max(1.0, float(np.abs(ref).max()))
        no_clamp = coef["c1"] * (coef["recip"] * case["x"][step].astype(F64) - coef["recipm1"] * case["eps"]) + coef["c2"] * case["x"][step] + coef["sigma"] * z
        # at t = 999 posterior_mean_coef1 is 2e-8: the clamp decides x0 and x0 hardly reaches x'. At t = 1 a missing clamp shows
        assert step == 999 or _caught(np.where(valid, no_clamp, 0.0), ref, bound, valid) > 0
    assert MR.mel_coef_ddpm(sched, 999)["c1"] < 1e-7
