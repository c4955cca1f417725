"""The float64 statements of tests/dpmpp_refs.py (DPM-Solver++ multistep, data prediction) checked on the CPU: the coefficient identities, the
order of the method on the closed-form Gaussian case with log-SNR spacing, the spacing rule's known answers, the wrong variants leaving the derived
bound, the header / ABI, and the argument handling of the model, the C entry and the command line. No GPU."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import dpmpp_refs as DR
import mel_step_refs as MR
from stylesinger_amd import abi, config
from stylesinger_amd import lib as L
from stylesinger_amd import plans

F64 = np.float64
AC100 = np.cumprod(1.0 - DR.BETAS100)
AC1000 = np.cumprod(1.0 - np.linspace(1e-4, 0.06, 1000))


# ------------------------------------------------------------------------------------------------
# 1. coefficients
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [[99, 46, 11, 2, 0], [99, 70, 39, 18, 7, 3, 1, 0], [3, 2, 1, 0], [57]])
def test_order_one_is_ddim_and_the_history_weights_sum_to_c1(ts):
    """Order 1 (and the first and last transition of order 2) carries ddim_coef(ac_t, ac_s, 0), which is the paper's pair
    (-alpha_s (e^-h - 1), sigma_s / sigma_t); b0 + b1 = c1 to double rounding, so a constant x0 history reproduces DDIM."""
    ac = AC100
    al, sg, lam = np.sqrt(ac), np.sqrt(1.0 - ac), DR.half_logsnr(ac)
    for i, t in enumerate(ts):
        last = i + 1 == len(ts)
        d = MR.ddim_coef(ac[t], 1.0 if last else ac[ts[i + 1]], 0.0)
        assert d["sigma"] == 0.0
        k1, k2 = DR.dpmpp_coef(ac, ts, i, 1), DR.dpmpp_coef(ac, ts, i, 2)
        assert (k1["b0"], k1["b1"], k1["c2"], k1["second"]) == (d["c1"], 0.0, d["c2"], False)
        assert k2["c2"] == d["c2"] and k2["last"] == last
        assert k2["second"] == (0 < i < len(ts) - 1)
        if not k2["second"]:
            assert (k2["b0"], k2["b1"]) == (d["c1"], 0.0)
        else:
            assert k2["b1"] != 0.0 and abs(k2["b0"] + k2["b1"] - d["c1"]) <= 4 * np.spacing(abs(k2["b0"]) + abs(k2["b1"]))
            r = (lam[t] - lam[ts[i - 1]]) / (lam[ts[i + 1]] - lam[t])
            assert r > 0 and k2["b1"] == -d["c1"] / (2 * r) and k2["b1"] < 0 < k2["b0"]
        if not last:
            s = ts[i + 1]
            h = lam[s] - lam[t]
            assert h > 0
            assert abs(d["c2"] - sg[s] / sg[t]) <= 1e-14 * d["c2"] and abs(d["c1"] + al[s] * np.expm1(-h)) <= 1e-12
        else:
            assert (d["c1"], d["c2"]) == (1.0, 0.0)
        assert k1["recip"] == np.sqrt(1.0 / ac[t]) and k1["recipm1"] == np.sqrt(1.0 / ac[t] - 1.0)
    tables, ac2 = DR.schedule_tables(DR.BETAS100)
    assert np.array_equal(ac2, ac)
    kt = DR.dpmpp_coef(ac, ts, 0, 2, tables)
    assert kt["recip"] == float(np.float32(np.sqrt(1.0 / ac[ts[0]]))) and kt["recipm1"] == float(np.float32(np.sqrt(1.0 / ac[ts[0]] - 1.0)))


def test_a_constant_history_reproduces_ddim():
    r = np.random.default_rng(3)
    ts = [99, 46, 11, 2, 0]
    x = r.standard_normal((1, 4, 8))
    x0 = r.uniform(-0.9, 0.9, x.shape)
    for i in (1, 2, 3):
        k2, k1 = DR.dpmpp_coef(AC100, ts, i, 2), DR.dpmpp_coef(AC100, ts, i, 1)
        eps = (k2["recip"] * x - x0) / k2["recipm1"]      # the eps whose x0 prediction is x0
        a, h = DR.dpmpp_step(x, eps, x0, k2)
        b, _ = DR.dpmpp_step(x, eps, None, k1)
        assert np.abs(h - x0).max() < 1e-12 and np.abs(a - b).max() < 1e-12


# ------------------------------------------------------------------------------------------------
# 2. the Gaussian case
# ------------------------------------------------------------------------------------------------
def test_second_order_on_the_gaussian_case_with_logsnr_spacing():
    """Data N(0.2, 0.3^2) under the 100-step schedule, six start quantiles, error at x_0. With the times uniform in the log-SNR, 2M's error is at
    most a quarter of DDIM's for n in {5, 6, 8, 10} (measured 9.5 - 13.2 x), the clamp acts nowhere, and order = 1 gives DDIM's numbers."""
    for n, want in ((4, 3.4), (5, 12.0), (6, 9.5), (8, 11.2), (10, 13.2), (20, 7.4)):
        ts = plans.logsnr_timesteps(AC100, 100, n)
        d, dc = DR.gaussian_error(AC100, ts, 1)
        m, mc = DR.gaussian_error(AC100, ts, 2)
        print(f"n = {n}: {len(ts)} times, DDIM {d:.3e}, 2M {m:.3e}, ratio {d / m:.1f}")
        assert not dc and not mc, "the clamp acted"
        assert abs(d / m - want) < 0.06 * want, (n, d, m)      # the recorded table, to its printed digits
        if n in (5, 6, 8, 10):
            assert m <= 0.25 * d, (n, d, m)
        # order 1 IS the eta = 0 DDIM recursion x' = alpha_s x0 + sigma_s eps', written out here from Song et al. eq. 12
        al, sg = np.sqrt(AC100), np.sqrt(1.0 - AC100)
        worst = 0.0
        for z in DR.GAUSS["zs"]:
            mu, s = DR.GAUSS["mu"], DR.GAUSS["s"]
            x = al[ts[0]] * mu + z * np.sqrt(al[ts[0]] ** 2 * s * s + sg[ts[0]] ** 2)
            for i, t in enumerate(ts):
                eps = sg[t] * (x - al[t] * mu) / (al[t] ** 2 * s * s + sg[t] ** 2)
                x0 = (x - sg[t] * eps) / al[t]
                x = x0 if i + 1 == len(ts) else al[ts[i + 1]] * x0 + sg[ts[i + 1]] * eps
            worst = max(worst, abs(x - (mu + s * z)))
        assert abs(worst - d) <= 1e-9, (worst, d)


def test_uniform_spacing_gives_the_multistep_no_advantage():
    """The finding that makes the spacing rule part of the feature: on the uniform-in-t list the last transitions span most of the log-SNR range
    and 2M is no better than DDIM (0.186 against 0.139 at n = 10)."""
    ts = plans.strided_timesteps(100, 10)
    d, _ = DR.gaussian_error(AC100, ts, 1)
    m, _ = DR.gaussian_error(AC100, ts, 2)
    assert abs(d - 0.139) < 2e-3 and abs(m - 0.186) < 2e-3, (d, m)


# ------------------------------------------------------------------------------------------------
# 3. the spacing rule
# ------------------------------------------------------------------------------------------------
def test_logsnr_timesteps_known_answers_and_invariants():
    f = plans.logsnr_timesteps
    assert f(AC100, 100, 4) == [99, 31, 4, 0]
    assert f(AC100, 100, 5) == [99, 46, 11, 2, 0]
    assert f(AC100, 100, 8) == [99, 70, 39, 18, 7, 3, 1, 0]
    assert len(f(AC100, 100, 20)) == 17
    for ac, S in ((AC100, 100), (AC1000, 1000)):
        for K in (S, S // 2, 7, 2, 1):
            for n in (1, 2, 3, 4, 6, 10, 20, 50, S, S + 5):
                ts = f(ac, K, n)
                assert all(isinstance(t, int) for t in ts)
                assert all(a > b for a, b in zip(ts, ts[1:])), (K, n, ts)
                assert ts[0] == K - 1 and len(ts) <= max(n, 1) and all(0 <= t < K for t in ts), (K, n, ts)
                if n == 1 or K == 1:
                    assert ts == [K - 1]
                else:
                    assert ts[-1] == 0
                if n >= 2 and K >= 2:
                    assert len(ts) >= 2
    assert f(AC100, 100, 1000) == f(AC100, 100, 100) and len(f(AC100, 100, 100)) < 100     # the grid is capped at K points; even those share times
    assert f(AC100, 50, 5)[0] == 49 and f(AC100, 50, 5) != f(AC100, 100, 5)       # K_step < steps: the first K times alone


# ------------------------------------------------------------------------------------------------
# 4. the derived bound holds for fp32 arithmetic and no wrong variant stays inside it
# ------------------------------------------------------------------------------------------------
def _uneven_case(seed=5, betas=None, ts=None):
    """the 1000-step schedule on a list whose gaps in the log-SNR are uneven (a list uniform in it has r = 1 throughout) - r far from 1 on both
    sides, asserted by the first test - with a controlled net: an eps per mel bin that does not depend on x but differs per network time, so
    that the x0 prediction moves by some tenths from one position to the next (under ONE eps for all times it repeats itself wherever the clamp
    is idle, and b0 + b1 = c1 hides the history weights); fp32 values; x spread over and beyond the rails' preimage at ts[0]"""
    tables, ac = DR.schedule_tables(np.linspace(1e-4, 0.06, 1000) if betas is None else betas)
    ts = [999, 990, 600, 580, 40, 0] if ts is None else ts
    r = np.random.default_rng(seed)
    B, T, M = 2, 9, 80
    lens = [9, 5]
    eps_of = {t: (r.uniform(-0.4, 0.4, M) / DR.dpmpp_coef(ac, ts, i, 2, tables)["recipm1"]).astype(np.float32).astype(F64) for i, t in enumerate(ts)}
    k = DR.dpmpp_coef(ac, ts, 0, 2, tables)
    x = ((r.uniform(-1.3, 1.3, (B, T, M)) + k["recipm1"] * eps_of[ts[0]]) / k["recip"]).astype(np.float32)
    return tables, ac, ts, x, (lambda xx, t: eps_of[t]), lens


def test_fp32_restatement_stays_inside_the_bound():
    tables, ac, ts, x, eps, lens = _uneven_case()
    rs = [(DR.half_logsnr(ac[ts[i]]) - DR.half_logsnr(ac[ts[i - 1]])) / (DR.half_logsnr(ac[ts[i + 1]]) - DR.half_logsnr(ac[ts[i]])) for i in range(1, len(ts) - 1)]
    assert min(rs) < 0.5 and max(rs) > 2.0, rs        # uneven gaps: r far from 1 on both sides
    ref = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens)
    got = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens, dtype=np.float32)
    ratio, bad = MR.over_bound(got["x"], ref["x"], ref["e_x"])
    assert bad == 0 and ratio <= 1.0, (ratio, bad)
    valid = np.arange(9)[None, :] < np.asarray(lens)[:, None]
    assert np.all(ref["x"][~valid] == 0) and np.all(ref["x0"][~valid] == 0) and np.all(ref["e_x"][~valid] == 0)
    inside = valid[..., None] & (np.abs(ref["x"]) < 1.0)
    print(f"fp32 restatement {ratio:.3f} x bound; bound max {ref['e_x'].max():.3e}; {inside.mean():.2f} of the elements end inside the rails")
    assert 0 < ref["e_x"][valid].max() < 1e-3 and ref["clamped"] and inside.mean() > 0.3


@pytest.mark.parametrize("variant", DR.VARIANTS)
def test_wrong_variants_leave_the_bound(variant):
    tables, ac, ts, x, eps, lens = _uneven_case()
    ref = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens)
    wrong = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens, variant=variant)
    ratio, bad = MR.over_bound(wrong["x"], ref["x"], ref["e_x"])
    valid = int((np.arange(9)[None, :] < np.asarray(lens)[:, None]).sum()) * 80
    print(f"{variant}: {bad} of {valid} valid elements beyond the bound, the worst {ratio:.3g} x")
    assert bad > 0.3 * valid and ratio > 100.0, (variant, bad, ratio)
    # ... and on the short list of the GPU test's whole-loop case
    t4, ac4, ts4, x, eps, lens = _uneven_case(6, np.linspace(1e-4, 0.06, 4), [3, 2, 1, 0])
    ref = DR.run_dpmpp(x, eps, ac4, ts4, 2, t4, lens=lens)
    wrong = DR.run_dpmpp(x, eps, ac4, ts4, 2, t4, lens=lens, variant=variant)
    assert MR.over_bound(wrong["x"], ref["x"], ref["e_x"])[1] > 0


def test_a_coefficient_off_in_its_last_digits_leaves_the_bound():
    """on the short list of the GPU test's whole-loop case, where the bound is a few roundings of values of order 1: b1 of the last multistep
    transition off by 2e-6 relative - some 16 fp32 ulp - shows"""
    tables, ac, ts, x, eps, lens = _uneven_case(6, np.linspace(1e-4, 0.06, 4), [3, 2, 1, 0])
    ref = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens)
    assert ref["e_x"].max() < 1e-5
    real = DR.dpmpp_coef

    def off(ac64, ts_, i, order, tables=None, variant=None):
        k = real(ac64, ts_, i, order, tables, variant)
        if i == len(ts_) - 2:
            k["b1"] *= 1.0 + 2e-6       # some 16 fp32 ulp
        return k
    try:
        DR.dpmpp_coef = off
        wrong = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens)
    finally:
        DR.dpmpp_coef = real
    assert MR.over_bound(wrong["x"], ref["x"], ref["e_x"])[1] > 0


def test_loop_cut_of_the_statement():
    tables, ac, ts, x, eps, lens = _uneven_case()
    whole = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens)
    a = DR.run_dpmpp(x, eps, ac, ts, 2, tables, lens=lens, i_lo=0, i_hi=2)
    b = DR.run_dpmpp(a["x"], eps, ac, ts, 2, tables, lens=lens, i_lo=2, x0_prev=a["x0"])
    assert np.array_equal(b["x"], whole["x"])


# ------------------------------------------------------------------------------------------------
# 5. header and ABI
# ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry():
    lib = L.load()
    decl = abi.declarations()
    name = "ss_meldiff_sample_dpmpp"
    assert name in L.declared_symbols() and hasattr(lib, name)
    ret, args = decl[name]
    assert ret is ctypes.c_int and len(args) == 17
    assert args[6] is ctypes.c_void_p and [args[i] for i in (4, 5, 7, 8, 9, 11, 13)] == [ctypes.c_int] * 7 and args[15] is ctypes.c_int64
    assert lib.ss_abi_version() == 20 == abi.DEFINES["SS_ABI_VERSION"], "the export is additive"


# ------------------------------------------------------------------------------------------------
# 6. argument handling
# ------------------------------------------------------------------------------------------------
def _entry_call(**over):
    """ss_meldiff_sample_dpmpp with one argument wrong: every pointer is a host buffer that is never read before the refusal"""
    lib = L.load()
    net = L.WaveNet()
    dummy = np.zeros(64, np.float32)
    a = dict(net=ctypes.addressof(net), x=L.hptr(dummy), cond=L.hptr(dummy), B=1, T=8, ts=[3, 1, 0], i_lo=0, i_hi=None, ac=np.cumprod(1.0 - np.linspace(1e-4, 0.06, 4)),
             order=2, hist=L.hptr(dummy), ws=L.hptr(dummy), C=256, in_dim=80, L=20)
    a.update(over)
    net.C, net.L, net.steps, net.in_dim, net.out_dim, net.n_groups = a["C"], a["L"], 4, a["in_dim"], a["in_dim"], 1
    ts = None if a["ts"] is None else np.ascontiguousarray(np.asarray(a["ts"], np.int32))
    n_ts = a.get("n_ts", 0 if ts is None else len(ts))
    ac = None if a["ac"] is None else np.ascontiguousarray(a["ac"], dtype=F64)
    rc = lib.ss_meldiff_sample_dpmpp(a["net"], a["x"], a["cond"], None, a["B"], a["T"], None if ts is None else L.hptr(ts), n_ts, a["i_lo"],
                                     n_ts if a["i_hi"] is None else a["i_hi"], None if ac is None else L.hptr(ac), a["order"], a["hist"], 1, a["ws"], 0, None)
    return rc, lib.ss_last_error().decode()


@pytest.mark.parametrize("over,text", [
    (dict(net=None), "null pointer"), (dict(x=None), "null pointer"), (dict(cond=None), "null pointer"), (dict(ts=None, n_ts=3), "null pointer"),
    (dict(ac=None), "null pointer"), (dict(hist=None), "null pointer"), (dict(ws=None), "null pointer"),
    (dict(n_ts=0), "n_ts"), (dict(n_ts=-1), "n_ts"),
    (dict(ts=[3, 3, 0]), "strictly decreasing"), (dict(ts=[1, 3]), "strictly decreasing"), (dict(ts=[4, 0]), "strictly decreasing"), (dict(ts=[3, -1]), "strictly decreasing"),
    (dict(i_lo=-1), "position range"), (dict(i_lo=2, i_hi=1), "position range"), (dict(i_hi=4), "position range"),
    (dict(order=0), "order"), (dict(order=3), "order"), (dict(in_dim=78), "multiple of 4"),
])
def test_entry_refuses_bad_arguments_before_any_launch(over, text):
    rc, msg = _entry_call(**over)
    assert rc != 0 and msg.startswith("ss_meldiff_sample_dpmpp: ") and text in msg, (rc, msg)


def test_valid_arguments_pass_the_argument_checks():
    """the same call with nothing wrong in the listed arguments gets past every one of those checks: it is stopped by the next one, the net's
    shape (no layers), still before any launch"""
    rc, msg = _entry_call(L=0)
    assert rc != 0 and msg.startswith("ss_meldiff_sample_dpmpp: bad net C=256 L=0"), (rc, msg)


def _model(**hp):
    from stylesinger_amd.model import StyleSingerHIP
    m = StyleSingerHIP(None, hparams=config.make_hparams(dict(timesteps=8, K_step=8, f0_timesteps=2, **hp)))
    m.eval()
    return m


def test_hparams_defaults_and_precedence():
    hp = config.make_hparams()
    assert (hp["mel_sampler"], hp["mel_sample_steps"], hp["mel_sample_order"], hp["mel_sample_spacing"], hp["mel_sample_eta"]) == (None, None, 2, None, 0.0)
    assert config.make_hparams(dict(mel_sampler="dpmpp", mel_sample_steps=10))["mel_sample_steps"] == 10
    arg = lambda m, **kw: vars(m._mel_sampler_args(kw))
    # nothing set: the reference's loop; pndm_speedup: its PLMS sampler
    assert arg(_model()) == dict(name="ddpm", steps=None, order=2, spacing=None, eta=0.0, interval=None)
    assert arg(_model(pndm_speedup=2)) == dict(name="plms", steps=None, order=2, spacing=None, eta=0.0, interval=2)
    assert arg(_model(pndm_speedup=2), plms_interval=3)["interval"] == 3
    # hparams['mel_sampler'] over pndm_speedup's absence, with its own defaults
    m = _model(mel_sampler="dpmpp", mel_sample_steps=5)
    assert arg(m) == dict(name="dpmpp", steps=5, order=2, spacing="logsnr", eta=0.0, interval=None)
    assert arg(_model(mel_sampler="ddim", mel_sample_steps=5, mel_sample_eta=0.5)) == dict(name="ddim", steps=5, order=2, spacing="uniform", eta=0.5, interval=None)
    assert arg(_model(mel_sampler="dpmpp", mel_sample_steps=5, mel_sample_order=1, mel_sample_spacing="uniform"))["spacing"] == "uniform"
    assert arg(_model(mel_sampler="plms", pndm_speedup=4))["interval"] == 4
    # the explicit kwarg over the hparams
    assert arg(m, sampler="ddpm")["name"] == "ddpm"
    assert arg(m, sampler="ddim", ddim_steps=3) == dict(name="ddim", steps=3, order=2, spacing="uniform", eta=0.0, interval=None)
    assert arg(m, mel_steps=7, mel_order=1, mel_spacing="uniform") == dict(name="dpmpp", steps=7, order=1, spacing="uniform", eta=0.0, interval=None)
    assert arg(_model(pndm_speedup=2), sampler="dpmpp", mel_steps=4)["name"] == "dpmpp"
    assert arg(_model(), sampler="ddim", mel_steps=4, mel_spacing="logsnr", eta=1.0) == dict(name="ddim", steps=4, order=2, spacing="logsnr", eta=1.0, interval=None)
    assert arg(_model(), sampler="ddim", ddim_steps=6, mel_steps=4)["steps"] == 4
    # mel_stage reads its arguments alone
    assert vars(m._mel_sampler_args(dict(sampler="ddpm"), use_hparams=False))["name"] == "ddpm"
    assert _model().mel_timesteps(3) == [7, 4, 0] == _model().ddim_timesteps(3)


def test_value_errors_need_no_device():
    m = _model()
    txt = torch.ones(1, 3, dtype=torch.long)
    for kw, text in ((dict(sampler="euler"), "mel sampler 'euler'"), (dict(sampler="dpmpp", mel_steps=4, mel_spacing="cosine"), "mel_spacing"),
                     (dict(sampler="dpmpp", mel_steps=0), "mel_steps"), (dict(sampler="dpmpp", mel_steps=-3), "mel_steps"), (dict(sampler="ddim", mel_steps=0), "mel_steps"),
                     (dict(sampler="dpmpp"), "mel_steps"), (dict(sampler="dpmpp", mel_steps=4, mel_order=3), "mel_order"),
                     (dict(sampler="dpmpp", mel_steps=4, mel_order=0), "mel_order"), (dict(sampler="plms"), "plms_interval")):
        with pytest.raises(ValueError, match=text):
            m(txt, infer=True, **kw)
        if "plms" not in text:
            with pytest.raises(ValueError, match=text):
                m.mel_stage(torch.zeros(1, 4, 80), torch.zeros(1, 4, 256), **kw)
    for hp, text in ((dict(mel_sampler="dpmpp", mel_sample_steps=4, pndm_speedup=2), "pndm_speedup"), (dict(mel_sampler="ddim", mel_sample_steps=4, pndm_speedup=2), "pndm_speedup"),
                     (dict(mel_sampler="ddpm", pndm_speedup=2), "pndm_speedup"), (dict(mel_sampler="heun"), "mel sampler 'heun'"),
                     (dict(mel_sampler="dpmpp"), "mel_steps"), (dict(mel_sampler="dpmpp", mel_sample_steps=4, mel_sample_order=3), "mel_order"),
                     (dict(mel_sampler="dpmpp", mel_sample_steps=4, mel_sample_spacing="x"), "mel_spacing")):
        with pytest.raises(ValueError, match=text):
            _model(**hp)(txt, infer=True)


def test_cli_flags_land_on_the_hparams(monkeypatch):
    from stylesinger_amd import infer
    seen = {}
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(infer.StyleSingerInfer, "example_run", classmethod(lambda cls, hparams=None, *a, **k: seen.update(hp=hparams)))
    base = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"]
    infer.main(base + ["--mel-sampler", "dpmpp", "--mel-steps", "10"])
    assert seen["hp"] == dict(mel_sampler="dpmpp", mel_sample_steps=10)
    infer.main(base + ["--mel-sampler", "dpmpp", "--mel-steps", "12", "--mel-order", "1", "--mel-spacing", "uniform"])
    assert seen["hp"] == dict(mel_sampler="dpmpp", mel_sample_steps=12, mel_sample_order=1, mel_sample_spacing="uniform")
    infer.main(base + ["--mel-sampler", "ddim", "--mel-steps", "20", "--mel-spacing", "logsnr", "--mel-eta", "0.5"])
    assert seen["hp"] == dict(mel_sampler="ddim", mel_sample_steps=20, mel_sample_spacing="logsnr", mel_sample_eta=0.5)
    infer.main(base + ["--mel-sampler", "plms"])
    assert seen["hp"] == dict(mel_sampler="plms")
    infer.main(base)
    assert not seen["hp"]
    for bad in (["--mel-steps", "10"], ["--mel-order", "2"], ["--mel-spacing", "logsnr"], ["--mel-eta", "0.5"], ["--mel-sampler", "dpmpp"],
                ["--mel-sampler", "dpmpp", "--mel-steps", "0"], ["--mel-sampler", "ddpm", "--mel-steps", "4"], ["--mel-sampler", "euler", "--mel-steps", "4"],
                ["--mel-sampler", "dpmpp", "--mel-steps", "4", "--mel-order", "3"], ["--mel-sampler", "ddim", "--mel-steps", "4", "--mel-order", "2"],
                ["--mel-sampler", "dpmpp", "--mel-steps", "4", "--mel-eta", "0.5"], ["--mel-sampler", "ddim", "--mel-steps", "4", "--mel-eta", "1.5"]):
        with pytest.raises(SystemExit):
            infer.main(base + bad)


def test_sweep_takes_the_mel_sampler():
    from stylesinger_amd import sweep
    p = inspect.signature(sweep.style_transfer_sweep).parameters
    assert p["mel_sampler"].default == "ddim" and p["mel_spacing"].default is None and p["ddim_steps"].default == 50
    with pytest.raises(ValueError, match="mel_sampler"):
        sweep.style_transfer_sweep(None, [], [], mel_sampler="plms")
