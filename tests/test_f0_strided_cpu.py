"""The strided f0 / uv sampler without a GPU: `ss_f0_strided_coef` against the numpy definition (tests/f0_strided_refs.py), the exactness of the
multinomial and Gaussian gap forms in float64, the stride-1 identity against the reference's own fp32 tables (and the pack-time guard that rests
on it), the input conditions tests/test_gpu_f0_strided.py relies on, the timestep rule, and the header / argument errors of the new entries."""
import ctypes

import numpy as np
import pytest
import torch

import f0_strided_refs as FR
import sampler_step_refs as SR
from stylesinger_amd import abi, config, packing, plans, synth
from stylesinger_amd import lib as L

F64 = np.float64
KEYS = SR.F0_COEF_KEYS
MAX_BETA = config.make_hparams()["f0_max_beta"]


def _tables(S):
    t = {**synth.multinomial_schedule(S, MAX_BETA), **synth.gaussian_schedule(S, MAX_BETA)}
    return {k: v.numpy() for k, v in t.items() if v.dim() == 1}


def _lib_coef(betas, t, s, eta):
    b64 = np.ascontiguousarray(np.asarray(betas, np.float32).astype(F64))
    out = np.full(9, np.nan, np.float32)
    L.check(L.load().ss_f0_strided_coef(L.hptr(b64), len(b64), t, s, eta, L.hptr(out)), "ss_f0_strided_coef")
    return out


# ------------------------------------------------------------------------------------------------
# 1. the library's coefficients against the definition
# ------------------------------------------------------------------------------------------------
def _coef_pairs():
    pairs = [(4, t, s) for t in range(4) for s in range(-1, t)]
    r = np.random.default_rng(3)
    some = {(99, 0), (1, 0), (0, -1), (99, 98), (99, -1), (50, 25)}
    while len(some) < 40:
        t = int(r.integers(0, 100))
        some.add((t, int(r.integers(-1, t))))
    return pairs + [(100, t, s) for t, s in sorted(some)]


def test_library_coefficients_are_the_definition_rounded_to_fp32():
    """Every transition of S = 4 and a sample of S = 100 with (99, 0), (1, 0), (0, final), eta in {0, 0.5, 1}: the nine fp32 values equal the numpy
    float64 definition after rounding, or sit 1 fp32 ulp from it where the two libms' float64 log / exp round differently; which of the two
    applied is counted and printed."""
    equal = off_by_one = 0
    for S, t, s in _coef_pairs():
        betas = _tables(S)["betas"]
        for eta in FR.ETAS:
            got = _lib_coef(betas, t, s, eta)
            want = np.array([np.float32(FR.strided_coef(betas, t, s, eta)[k]) for k in KEYS])
            for k, a, b in zip(KEYS, got, want):
                if a == b:
                    equal += 1
                    continue
                assert abs(float(a) - float(b)) <= float(np.spacing(np.abs(b))), (S, t, s, eta, k, a, b)
                off_by_one += 1
    print(f"ss_f0_strided_coef: {equal} values equal to the definition after fp32 rounding, {off_by_one} one ulp away")
    assert equal > 0 and off_by_one <= 0.01 * equal


def test_final_transition_is_the_references_t0_row():
    for S in (4, 100):
        betas = _tables(S)["betas"]
        for t in (0, S - 1):
            for eta in FR.ETAS:
                c = FR.strided_coef(betas, t, FR.FINAL, eta)
                assert c["sigma"] == 0.0 and c["c2"] == 0.0 and c["c1"] == 1.0 and c["log_cp_tm1"] == 0.0
                got = dict(zip(KEYS, _lib_coef(betas, t, -1, eta)))
                assert got["sigma"] == 0.0 and got["c2"] == 0.0 and got["c1"] == 1.0 and got["log_cp_tm1"] == 0.0


# ------------------------------------------------------------------------------------------------
# 2. exactness of the two gap forms in float64
# ------------------------------------------------------------------------------------------------
def _exactness_pairs():
    pairs = [(4, t, s) for t in range(4) for s in range(-1, t)]
    r = np.random.default_rng(5)
    for _ in range(50):
        t = int(r.integers(0, 100))
        pairs.append((100, t, int(r.integers(-1, t))))
    return pairs


def test_multinomial_gap_posterior_is_exact():
    """K = 2: q(x_s | x_t, x0) from products of the per-step transition matrices against the closed form the coefficients define, for every pair
    of S = 4 and 50 random pairs of S = 100: <= 1e-12."""
    worst = 0.0
    for S, t, s in _exactness_pairs():
        betas = _tables(S)["betas"]
        brute = FR.posterior_brute(betas, t, s)
        closed = FR.posterior_closed(FR.strided_coef(betas, t, s, 1.0), s)
        assert np.allclose(brute.sum(-1), 1.0, atol=1e-14)
        worst = max(worst, float(np.abs(brute - closed).max()))
    print(f"multinomial gap posterior: closed form within {worst:.3e} of the matrix products")
    assert worst <= 1e-12


def test_gaussian_gap_identities():
    """c1 + c2 sqrt(ac_t) = sqrt(ac_s) (the mean of x_s given x0) and c2^2 (1 - ac_t) + sigma^2 = 1 - ac_s (its variance), both to 1e-12."""
    worst = 0.0
    for S, t, s in _exactness_pairs():
        betas = _tables(S)["betas"]
        _, ac, _ = FR.schedule(betas)
        ac_s = ac[s] if s >= 0 else 1.0
        for eta in FR.ETAS:
            c = FR.strided_coef(betas, t, s, eta)
            worst = max(worst, abs(c["c1"] + c["c2"] * np.sqrt(ac[t]) - np.sqrt(ac_s)), abs(c["c2"] ** 2 * (1.0 - ac[t]) + c["sigma"] ** 2 - (1.0 - ac_s)))
    assert worst <= 1e-12, worst


# ------------------------------------------------------------------------------------------------
# 3. stride 1, eta = 1 against the reference's fp32 tables; the pack-time guard
# ------------------------------------------------------------------------------------------------
def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0.0 else (0.0 if a == 0.0 else float("inf"))


@pytest.mark.parametrize("S", [4, 100])
def test_stride_one_eta_one_is_the_references_tables(S):
    """Every t: the nine coefficients of t -> t-1 (0 -> final) against what the classic step reads from the fp32 buffers
    (sampler_step_refs.f0_coef), relative deviation <= 1e-6. At t = 0 the two prior names are read by neither sampler (the final transition has
    no prior term; the classic table lookup is clamped to index 0 only to stay in range): there the definition's own values are asserted, and
    table entry 0 is compared as the prior of t = 1."""
    tables = _tables(S)
    worst, where = 0.0, None
    for t in range(S):
        mine, ref = FR.strided_coef(tables["betas"], t, t - 1, 1.0), SR.f0_coef(tables, t)
        for k in KEYS:
            if t == 0 and k in ("log_cp_tm1", "log_1m_cp_tm1"):
                assert mine["log_cp_tm1"] == 0.0 and mine["log_1m_cp_tm1"] == np.log(1e-40)
                continue
            d = _rel(mine[k], ref[k])
            if d > worst:
                worst, where = d, (k, t)
    print(f"S = {S}: stride-1 coefficients within {worst:.3e} (relative) of the reference's tables, worst {where}")
    assert worst <= 1e-6, (worst, where)
    # the product's guard measures the same thing with the library's coefficients
    betas, dev, _, err = packing.f0_strided_guard(tables)
    assert err is None and dev <= 1e-6 and betas.dtype == np.float64 and np.array_equal(betas, tables["betas"].astype(F64))


@pytest.mark.parametrize("name", ["log_cumprod_alpha", "log_1_min_alpha", "posterior_mean_coef2"])
def test_guard_refuses_tables_that_do_not_belong_to_the_betas(name):
    tables = dict(_tables(100))
    bad = tables[name].copy()
    bad[40] *= np.float32(1.0 + 1e-5)
    tables[name] = bad
    _, dev, where, err = packing.f0_strided_guard(tables)
    assert err is not None and "strided" in err and "refused" in err and dev > 1e-6 and where[1] in (40, 41)
    assert packing.F0_STRIDED_RTOL == 1e-6


# ------------------------------------------------------------------------------------------------
# 4. input conditions of the GPU test
# ------------------------------------------------------------------------------------------------
_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = SR.controlled_case(name, _tables(SR.S_F0))
    return _CASES[name]


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_controlled_cases_under_strided_transitions(name):
    """Every case of sampler_step_refs.CASES, the transitions of f0_strided_refs.TRANSITIONS, eta in {0, 0.5, 1}, the targeted frames steered with
    the strided coefficients: the fp32-CPU step passes the GPU test's check (0 flips, f0 <= 1.0 x f0_step_bound), undecided frames are <= 1 % of
    the valid ones, and every regime mask keeps >= 3 decided frames."""
    betas = _tables(SR.S_F0)["betas"]
    base = _case(name)
    valid = base["valid"]
    n_valid = int(valid.sum())
    worst_ratio = worst_thr = 0.0
    n_und = 0
    for t, s in FR.TRANSITIONS:
        for eta in FR.ETAS:
            case = FR.steer(base, betas, t, s, eta)
            cpu = FR.controlled_strided_step(case, betas, t, s, eta, dtype=torch.float32)
            chk = FR.check_strided_step(case, betas, t, s, eta, cpu["f0"], cpu["uv"])
            und, reg = chk["undecided"], case["regimes"]
            assert int(und.sum()) <= 0.01 * n_valid, (name, t, s, eta, int(und.sum()), n_valid)
            assert chk["flips"] == 0 and chk["f0_ratio"] <= 1.0, (name, t, s, eta, chk["flips"], chk["f0_ratio"])
            assert float(chk["thr"].max()) < 0.2 * SR.TARGET_DELTA
            worst_ratio, worst_thr, n_und = max(worst_ratio, chk["f0_ratio"]), max(worst_thr, float(chk["thr"].max())), n_und + int(und.sum())
            dec = ~und
            masks = dict(uv0=reg["uv0"], uv1=reg["uv1"], pin=reg["pin"], band=reg["band"], idle=reg["idle"], edge0=reg["edge0"][t], edge1=reg["edge1"][t],
                         target=reg["target"][t])
            if (~valid).any():
                masks["padded"] = reg["padded"]
            for k, m in masks.items():
                assert int((m & dec & valid).sum() if k not in ("padded", "target") else (m & dec).sum()) >= 3, (name, t, s, eta, k)
            m_t = chk["ref"]["margin"][reg["target"][t]]
            assert np.all(np.abs(m_t) > 0.5 * SR.TARGET_DELTA) and np.all(np.abs(m_t) < 2.0 * SR.TARGET_DELTA)
    print(f"{name}: fp32-CPU f0 at most {worst_ratio:.3f} x the bound, {n_und} undecided frames in all, largest threshold {worst_thr:.3e}")


def test_strided_step_with_stride_one_is_the_classic_step():
    """The restatement at t -> t-1, eta = 1 against sampler_step_refs.controlled_step on the same inputs: same classes on decided frames, f0 within
    the few-ulp coefficient differences (1e-6 relative on every coefficient -> far inside 1e-5 absolute at these magnitudes)."""
    tables = _tables(SR.S_F0)
    case = _case("near0_rem14")
    for t in range(SR.S_F0):
        a = FR.controlled_strided_step(case, tables["betas"], t, t - 1, 1.0)
        b = SR.controlled_step(case, tables, t)
        assert np.abs(a["f0"] - b["f0"]).max() < 1e-5
        assert np.array_equal(a["uv"], b["uv"]) or np.abs(b["margin"][a["uv"] != b["uv"]]).max() < 1e-4


# ------------------------------------------------------------------------------------------------
# 5. the timestep rule
# ------------------------------------------------------------------------------------------------
def test_timestep_rule():
    for S in (1, 4, 7, 100):
        holder = type("M", (plans.Plans,), {})()
        holder.hp = dict(f0_timesteps=S, K_step=S)
        for n in (-3, 0, 1, 2, 3, S - 1, S, S + 1, 10 * S):
            ts = holder.f0_strided_timesteps(n)
            assert ts == FR.timesteps(S, n), (S, n, ts)
            assert all(a > b for a, b in zip(ts, ts[1:])) and ts[0] == S - 1 and 0 <= ts[-1] < S
            k = max(1, min(n, S))
            assert len(ts) <= k
            if k >= 2:
                assert ts[-1] == 0 and ts == holder.ddim_timesteps(n)
            if n >= S:
                assert ts == list(range(S - 1, -1, -1))
    assert FR.timesteps(100, 10) == [99, 88, 77, 66, 55, 44, 33, 22, 11, 0] and len(FR.timesteps(100, 50)) == 50
    assert FR.successors([3, 1, 0]) == [(3, 1), (1, 0), (0, FR.FINAL)]


# ------------------------------------------------------------------------------------------------
# 6. header, exports, argument errors
# ------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entries():
    lib = L.load()
    decl = abi.declarations()
    for name, nargs in (("ss_f0diff_sample_strided", 23), ("ss_f0_strided_coef", 6)):
        assert name in L.declared_symbols() and hasattr(lib, name)
        assert decl[name][0] is ctypes.c_int and len(decl[name][1]) == nargs
    assert lib.ss_abi_version() == 20
    a = decl["ss_f0diff_sample_strided"][1]
    assert a[9] is ctypes.c_void_p and a[10] is ctypes.c_int and a[13] is ctypes.c_void_p and a[14] is ctypes.c_float and a[17] is ctypes.c_uint64


def _strided_call(**over):
    """ss_f0diff_sample_strided with one argument wrong: every pointer is a host buffer that is never read before the refusal"""
    lib = L.load()
    net = L.WaveNet()
    dummy = np.zeros(64, np.float32)
    a = dict(net=ctypes.addressof(net), f0=L.hptr(dummy), uv=L.hptr(dummy), cond=L.hptr(dummy), lo=L.hptr(dummy), hi=L.hptr(dummy), lens=None, B=1, T=8,
             ts=[3, 1, 0], i_lo=0, i_hi=None, betas=_tables(4)["betas"].astype(F64), eta=1.0, ws=L.hptr(dummy), C=192)
    a.update(over)
    net.C, net.L, net.steps, net.in_dim, net.out_dim, net.n_groups = a["C"], 10, 4, 1, 3, 1
    ts = None if a["ts"] is None else np.ascontiguousarray(np.asarray(a["ts"], np.int32))
    n_ts = a.get("n_ts", 0 if ts is None else len(ts))
    betas = None if a["betas"] is None else np.ascontiguousarray(a["betas"], dtype=F64)
    rc = lib.ss_f0diff_sample_strided(a["net"], a["f0"], a["uv"], a["cond"], a["lo"], a["hi"], a["lens"], a["B"], a["T"], None if ts is None else L.hptr(ts),
                                      n_ts, a["i_lo"], n_ts if a["i_hi"] is None else a["i_hi"], None if betas is None else L.hptr(betas), a["eta"],
                                      None, None, 17, None, 1, a["ws"], 0, None)
    return rc, lib.ss_last_error().decode()


BETAS4 = np.linspace(1e-4, 0.06, 4)


@pytest.mark.parametrize("over,text", [
    (dict(net=None), "null pointer"), (dict(f0=None), "null pointer"), (dict(ts=None, n_ts=3), "null pointer"), (dict(betas=None), "null pointer"),
    (dict(ws=None), "null pointer"),
    (dict(n_ts=0), "n_ts"), (dict(ts=[3, 3, 0]), "strictly decreasing"), (dict(ts=[1, 3]), "strictly decreasing"), (dict(ts=[4, 0]), "strictly decreasing"),
    (dict(ts=[3, -1]), "strictly decreasing"),
    (dict(i_lo=-1), "position range"), (dict(i_lo=2, i_hi=1), "position range"), (dict(i_hi=4), "position range"),
    (dict(eta=-0.1), "eta"), (dict(eta=1.5), "eta"), (dict(eta=float("nan")), "eta"),
    (dict(betas=np.where(np.arange(4) == 2, np.nan, BETAS4)), "betas[2]"), (dict(betas=np.where(np.arange(4) == 1, 1.0, BETAS4)), "betas[1]"),
    (dict(betas=np.where(np.arange(4) == 0, 0.0, BETAS4)), "betas[0]"), (dict(betas=np.where(np.arange(4) == 3, np.inf, BETAS4)), "betas[3]"),
])
def test_strided_entry_refuses_bad_arguments_before_any_launch(over, text):
    rc, msg = _strided_call(**over)
    assert rc != 0 and "ss_f0diff_sample_strided" in msg and text in msg, (rc, msg)


def test_valid_arguments_pass_the_argument_checks():
    """the same call with nothing wrong in the listed arguments gets past every one of those checks: it is stopped by the next one, the net's
    shape (C = 100 is not a multiple of 64), still before any launch"""
    rc, msg = _strided_call(C=100)
    assert rc != 0 and "bad net C=100" in msg, (rc, msg)


def test_coef_entry_refuses_bad_arguments():
    lib = L.load()
    b = np.ascontiguousarray(BETAS4)
    out = np.zeros(9, np.float32)
    for args, text in (((None, 4, 1, 0, 1.0, L.hptr(out)), "null"), ((L.hptr(b), 4, 1, 0, 1.0, None), "null"), ((L.hptr(b), 0, 0, -1, 1.0, L.hptr(out)), "steps"),
                       ((L.hptr(b), 4, 4, 0, 1.0, L.hptr(out)), "transition"), ((L.hptr(b), 4, 1, 1, 1.0, L.hptr(out)), "transition"),
                       ((L.hptr(b), 4, 1, -2, 1.0, L.hptr(out)), "transition"), ((L.hptr(b), 4, 1, 0, 2.0, L.hptr(out)), "eta")):
        assert lib.ss_f0_strided_coef(*args) != 0 and text in lib.ss_last_error().decode(), args
    bad = b.copy()
    bad[1] = -0.5
    assert lib.ss_f0_strided_coef(L.hptr(bad), 4, 1, 0, 1.0, L.hptr(out)) != 0 and "betas[1]" in lib.ss_last_error().decode()


def test_forward_and_cli_refusals_need_no_device(monkeypatch):
    from stylesinger_amd.model import StyleSingerHIP
    hp = config.make_hparams(dict(timesteps=2, K_step=2, f0_timesteps=2))
    assert hp["f0_sample_steps"] is None and hp["f0_sample_eta"] == 1.0
    assert config.make_hparams(dict(f0_sample_steps=10, f0_sample_eta=0.0))["f0_sample_steps"] == 10
    m = StyleSingerHIP(None, hparams=hp)
    m.eval()
    txt = torch.ones(1, 3, dtype=torch.long)
    f0, uv, hz = torch.full((1, 8), 8.0), torch.zeros(1, 8), torch.full((1, 8), 220.0)
    for kw in (dict(f0_steps=0), dict(f0_steps=-2)):
        with pytest.raises(ValueError, match="f0_steps"):
            m(txt, infer=True, **kw)
    for eta in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="f0_eta"):
            m(txt, infer=True, f0_steps=2, f0_eta=eta)
    with pytest.raises(ValueError, match="f0_steps.*given contour"):
        m(txt, infer=True, f0=f0, uv=uv, f0_steps=2)
    with pytest.raises(ValueError, match="f0_steps.*given contour"):
        m(txt, infer=True, pitch_hz=(hz, [8]), f0_steps=2)
    # the hparams defaults: checked like the kwargs, and simply unused with a given contour
    bad = StyleSingerHIP(None, hparams=dict(hp, f0_sample_steps=0))
    with pytest.raises(ValueError, match="f0_steps"):
        bad(txt, infer=True)
    assert bad._f0_sampler_args({}, True) == (None, 1.0)
    assert m._f0_sampler_args({}, False) == (None, 1.0)
    assert m._f0_sampler_args(dict(f0_steps=5, f0_eta=0), False) == ([1, 0], 0.0)
    # the command line
    from stylesinger_amd import infer
    seen = {}
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(infer.StyleSingerInfer, "example_run", classmethod(lambda cls, hparams=None, *a, **k: seen.update(hp=hparams)))
    base = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"]
    infer.main(base + ["--f0-steps", "10", "--f0-eta", "0.5"])
    assert seen["hp"]["f0_sample_steps"] == 10 and seen["hp"]["f0_sample_eta"] == 0.5
    infer.main(base)
    assert not seen["hp"] or "f0_sample_steps" not in seen["hp"]
    for bad_flags in (["--f0-steps", "0"], ["--f0-eta", "0.5"], ["--f0-steps", "4", "--f0-eta", "1.5"]):
        with pytest.raises(SystemExit):
            infer.main(base + bad_flags)


def test_sweep_takes_f0_steps_last():
    import inspect
    from stylesinger_amd import sweep
    params = list(inspect.signature(sweep.style_transfer_sweep).parameters)
    assert params[-1] == "f0_steps" and inspect.signature(sweep.style_transfer_sweep).parameters["f0_steps"].default is None
