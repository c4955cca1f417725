"""GPU parity of the strided joint f0 / uv sampler (ss_f0diff_sample_strided: f0_tail_kernel / f0_update_row of csrc/f0_sampler.hip with the
coefficients of a gap t -> s) against the float64 statements of tests/f0_strided_refs.py, whose input conditions tests/test_f0_strided_cpu.py
asserts without a GPU; its loop-cut and tape-addressing contracts; its stride-1 identity with ss_f0diff_sample; and forward(f0_steps=, f0_eta=).

The nets, cases, sentinels and tolerances are those of tests/test_gpu_sampler_steps.py (production C = 192, L = 10 pair, f0_timesteps = 4):
  * controlled net: f0 within sampler_step_refs.f0_step_bound (one rounding per fp32 operation + the dot product's bound), padded frames
    included; uv identical on every decided frame (margin >= max(4 x the fp32-CPU margin error, 8 ulp)); undecided frames <= 1 % of the valid ones.
  * real weights: f0 within 4 x the fp32 CPU oracle's own error against float64 (never less than 2 ulp), decided frames identical.
  * loop cuts, tape addressing, graph replay, feed-back: bit-identical (torch.equal).
  * whole model on golden acoustic_tiny_s4: the bounds of tests/test_gpu_parity.py.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f0_strided_refs as FR  # noqa: E402
import sampler_step_refs as SR  # noqa: E402
import test_gpu_parity as P  # noqa: E402
import test_gpu_sampler_steps as G  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import harness  # noqa: E402
from oracle import philox as PH  # noqa: E402
from oracle import restatement as R  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import synth  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

DEV = G.DEV
S = SR.S_F0
F64 = np.float64
LISTS = ([3, 0], [3, 1, 0], [3, 2, 0], [3, 2, 1, 0])


def _betas():
    return G._tables()["betas"]


class _Run:
    """Both f0 entry points on one set of inputs: device copies made once, one workspace kept across calls (a cut loop precomputes once)"""

    def __init__(self, net, *, B, T, cond, lo, hi, lens, z=None, u=None, seed=17, seed_dev=None):
        self.lib, self.net, self.B, self.T = L.load(), net, B, T
        self.cond, self.lo, self.hi = G._d(cond), G._d(lo), G._d(hi)
        self.lens = G._d(np.asarray(lens, np.int32))
        self.z = None if z is None else G._d(z)
        self.u = None if u is None else G._d(u)
        self.seed = seed
        self.seed_dev = None if seed_dev is None else torch.tensor([seed_dev], device=DEV, dtype=torch.int64)
        self.betas = np.ascontiguousarray(_betas().astype(F64))
        assert len(self.betas) == net.steps == S
        self.wsb = self.lib.ss_wavenet_workspace_bytes(ctypes.addressof(net), B, T)
        assert self.wsb > 0
        self.ws = torch.empty(self.wsb, device=DEV, dtype=torch.uint8)

    def strided(self, f, u, ts, i_lo, i_hi, eta, precompute):
        ts = np.ascontiguousarray(np.asarray(ts, np.int32))
        L.check(self.lib.ss_f0diff_sample_strided(ctypes.addressof(self.net), L.ptr(f), L.ptr(u), L.ptr(self.cond), L.ptr(self.lo), L.ptr(self.hi),
                                                  L.ptr(self.lens), self.B, self.T, L.hptr(ts), len(ts), i_lo, i_hi, L.hptr(self.betas), float(eta),
                                                  L.ptr(self.z), L.ptr(self.u), self.seed, L.ptr(self.seed_dev), precompute, L.ptr(self.ws), self.wsb,
                                                  L.stream_ptr()), "ss_f0diff_sample_strided")
        torch.cuda.synchronize()

    def classic(self, f, u, lo_step, hi_step, precompute):
        L.check(self.lib.ss_f0diff_sample(ctypes.addressof(self.net), L.ptr(f), L.ptr(u), L.ptr(self.cond), L.ptr(self.lo), L.ptr(self.hi), L.ptr(self.lens),
                                          self.B, self.T, L.ptr(self.z), L.ptr(self.u), self.seed, L.ptr(self.seed_dev), lo_step, hi_step, precompute,
                                          L.ptr(self.ws), self.wsb, L.stream_ptr()), "ss_f0diff_sample")
        torch.cuda.synchronize()


def _case_run(case, spec):
    model = G._controlled_model(spec["wset"])
    net = G._f0_net(model, None if spec["paired"] else spec["single"])
    return lambda c: _Run(net, B=c["B"], T=c["T"], cond=c["cond"], lo=c["lo"], hi=c["hi"], lens=c["lens"], z=c["z"], u=c["u"])


def _assert_step(tag, case, chk):
    n_valid, n_und = int(case["valid"].sum()), int(chk["undecided"].sum())
    print(f"[{tag}] f0 {chk['f0_err']:.3e} = {chk['f0_ratio']:.3f} x bound (fp32 CPU {chk['cpu_f0_ratio']:.3f} x); uv flips {chk['flips']}, "
          f"undecided {n_und} of {case['B'] * case['T']}")
    assert n_und <= 0.01 * n_valid, (tag, n_und, n_valid)
    assert chk["f0_ratio"] <= 1.0, f"{tag}: f0 is {chk['f0_ratio']:.3g} x its bound (padded frames included)"
    assert chk["flips"] == 0, f"{tag}: {chk['flips']} decided frames got the other class, first at {np.argwhere(chk['flip_mask'])[:4].tolist()}"


# ------------------------------------------------------------------------------------------------
# 1. controlled net, single transitions
# ------------------------------------------------------------------------------------------------
def _controlled_transitions(base, spec, what, lists=LISTS, etas=(0.0, 1.0), positions=None):
    betas = _betas()
    make = _case_run(base, spec)
    B, T = base["B"], base["T"]
    for ts in lists:
        for i, (t, s) in enumerate(FR.successors(ts)):
            if positions is not None and i not in positions:
                continue
            for eta in etas:
                case = FR.steer(base, betas, t, s, eta)    # the uniforms of tape row t steered for this very transition
                run = make(case)
                f, u = G._state(case["f0"], case["uv"])
                run.strided(f, u, ts, i, i + 1, eta, 1)
                f0_out, uv_out = G._split(f, u, B, T)       # asserts the sentinel tails
                assert set(np.unique(uv_out).tolist()) <= {0, 1}
                chk = FR.check_strided_step(case, betas, t, s, eta, f0_out, uv_out)
                record_measurement(f"f0_strided_{what}", case=case["name"], ts=list(ts), position=i, t=t, s=s, eta=eta, f0_err=chk["f0_err"],
                                   f0_bound=chk["f0_bound"], f0_ratio=chk["f0_ratio"], cpu_fp32_f0_ratio=chk["cpu_f0_ratio"], uv_flips=chk["flips"],
                                   undecided=int(chk["undecided"].sum()), frames=B * T, thr_max=float(chk["thr"].max()))
                _assert_step(f"{case['name']} {ts}[{i}] {t}->{s} eta {eta}", case, chk)


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_controlled_net_single_transitions(name):
    """Every position of the lists [3,0], [3,1,0], [3,2,0], [3,2,1,0] as a call [i, i+1) from the case's inputs, eta in {0, 1}: every regime of
    sampler_step_refs.controlled_case (clamp pinned / band / idle, edge uniforms, margins steered to +-5e-3 with the strided coefficients,
    l0 - l1 = +-40 / ~0, ragged lens with a single frame, B*T mod 16 in {1, 2, 14, 15}), padded frames checked like the rest, sentinels intact.
    These shapes take the split-K slices form of the skip source (asserted)."""
    spec = SR.CASES[name]
    base = SR.controlled_case(name, G._tables())
    assert G._ksplit(base["B"], base["T"]) > 1, "this shape no longer takes the slices form"
    _controlled_transitions(base, spec, "controlled")


def test_controlled_net_reduced_skip_source():
    """One strided transition (3 -> 1 of [3,1,0]) where the tail kernel reads the reduced tensor G: 16 items at the smallest T, not a multiple of
    16, at which the split-K pick returns 1 (the precondition is asserted)."""
    B = 16
    T = next(t for t in range(1, 4000) if t % 16 and G._ksplit(B, t) == 1)
    assert G._ksplit(B, T) == 1 and T % 16 != 0
    spec = SR.reduced_spec(B, T)
    _controlled_transitions(SR.controlled_case(spec, G._tables()), spec, "controlled_reduced", lists=([3, 1, 0],), etas=(1.0,), positions=(0,))


# ------------------------------------------------------------------------------------------------
# 2. real weights, list [3, 1, 0]
# ------------------------------------------------------------------------------------------------
def _oracle_transition(sd, hp, inp, f0, uv, t, s, eta, dtype):
    """G._oracle_step for a strided transition: oracle.ddiffnet at network time t per item on its valid frames, then the strided step statement"""
    B, T, h = inp["B"], inp["T"], inp["B"] // 2
    tt = torch.float64 if dtype == torch.float64 else torch.float32
    out = np.zeros((B, T, 3), F64)
    torch.set_default_dtype(tt)
    try:
        with torch.no_grad():
            for b in range(B):
                n = int(inp["lens"][b])
                o = R.ddiffnet(sd, hp, torch.from_numpy(f0[b:b + 1, :n]).to(tt), torch.from_numpy(uv[b:b + 1, :n]).long(), torch.full((1,), t, dtype=torch.long),
                               torch.from_numpy(inp["cond"][b:b + 1, :n]).to(tt), G.F0_NETS[b // h])
                out[b, :n] = o[0].double().numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    return FR.strided_step(f0, uv, out[..., 0], out[..., 1:], inp["lo"], inp["hi"], inp["z"], inp["u"], _betas(), t, s, eta, dtype=tt)


def _check_real_transition(name, inp, f0_in, uv_in, t, s, eta, f0_out, uv_out, sd32, sd64, hp):
    """the rules of G._check_real_step"""
    f64, uv64, m64, mag = _oracle_transition(sd64, hp, inp, f0_in, uv_in, t, s, eta, torch.float64)
    f32_, _, m32, _ = _oracle_transition(sd32, hp, inp, f0_in, uv_in, t, s, eta, torch.float32)
    thr, cpu_m_err = SR.decision_threshold(m64, m32, mag)
    und = np.abs(m64) < thr
    cpu_err = float(np.abs(f32_ - f64).max())
    floor = 2.0 * float(np.spacing(np.float32(np.abs(f64).max())))
    bound = max(4.0 * cpu_err, floor)
    err = float(np.abs(f0_out.astype(F64) - f64).max()) if np.isfinite(f0_out).all() else float("inf")
    flips = int(((uv_out != uv64) & ~und).sum())
    record_measurement("f0_strided_real_" + name, t=t, s=s, eta=eta, kernel_err=err, cpu_fp32_err=cpu_err, bound=bound, ratio=err / bound, uv_flips=flips,
                       undecided=int(und.sum()), frames=int(und.size), cpu_margin_err=cpu_m_err, thr_max=float(thr.max()))
    print(f"[real {name} {t}->{s}] f0 kernel {err:.3e} cpu-fp32 {cpu_err:.3e} bound {bound:.3e}; uv flips {flips}, undecided {int(und.sum())}")
    assert int(und.sum()) <= 0.01 * int((np.arange(inp["T"])[None] < inp["lens"][:, None]).sum())
    assert err <= bound, (name, t, s, err, cpu_err, bound)
    assert flips == 0, (name, t, s, flips)


@pytest.mark.parametrize("eta", [1.0, 0.0])
def test_real_weights_list_3_1_0_and_the_x_handover(eta):
    """Unmodified synthetic weights, ragged lens: the calls [0, 1), [0, 2) and [0, 3) of the list [3, 1, 0]. Transition i is judged on the call
    that ends with it, against the float64 oracle (oracle.ddiffnet at network time ts[i] + the strided step statement) started from the DEVICE's
    own state after the call one position shorter (the same launches, the same bits: test_loop_cut_is_bit_identical). In the longer calls the
    evaluation of position i reads the input row the previous transition's launch wrote: were that row not the input row of the new state
    (sampler_step_refs.f0_input_row, which is what oracle.ddiffnet builds from the state it is given), the network output and with it f0 and uv
    would leave the bound."""
    hp, sd32 = G._hp(), G._base_sd()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    model = G._model("real", sd32)
    inp = G._real_inputs()
    B, T = inp["B"], inp["T"]
    run = _Run(G._f0_net(model), B=B, T=T, cond=inp["cond"], lo=inp["lo"], hi=inp["hi"], lens=inp["lens"], z=inp["z"], u=inp["u"])
    ts = [3, 1, 0]
    f0_prev, uv_prev = inp["f0"], inp["uv"]
    for i, (t, s) in enumerate(FR.successors(ts)):
        f, u = G._state(inp["f0"], inp["uv"])
        run.strided(f, u, ts, 0, i + 1, eta, 1)
        f0_i, uv_i = G._split(f, u, B, T)
        _check_real_transition(f"position{i}_eta{eta:g}", inp, f0_prev, uv_prev, t, s, eta, f0_i, uv_i, sd32, sd64, hp)
        assert np.abs(f0_i - f0_prev).max() > 1e-3
        f0_prev, uv_prev = f0_i, uv_i


# ------------------------------------------------------------------------------------------------
# 3. stride 1, eta = 1 against ss_f0diff_sample
# ------------------------------------------------------------------------------------------------
ALL = list(range(S - 1, -1, -1))


def _coef_shift_bound(case, tables, t, eps):
    """How far the exact results of the two entries may lie apart at t -> t-1: every coefficient of the strided entry is within 1e-6 (relative) of
    the classic one (tests/test_f0_strided_cpu.py, the pack-time guard's bar). x0 = clamp(recip x - recipm1 eps) moves by at most
    1e-6 (|recip x| + |recipm1 eps|) (the clamp is 1-Lipschitz), c1 x0 by |c1| times that plus 1e-6 |c1 x0|, c2 x and sigma z by 1e-6 of themselves."""
    c = SR.f0_coef(tables, t)
    x, z = case["f0"].astype(F64), np.abs(case["z"][t].astype(F64))
    a, b = c["recip"] * x, c["recipm1"] * eps
    x0 = np.clip(a - b, case["lo"].astype(F64), case["hi"].astype(F64))
    return 1e-6 * (abs(c["c1"]) * (np.abs(a) + np.abs(b) + np.abs(x0)) + abs(c["c2"]) * np.abs(x) + c["sigma"] * z)


@pytest.mark.parametrize("name", ["pm40_b4", "near0_rem14"])
def test_stride_one_eta_one_is_the_default_entry(name):
    """ts = 3 ... 0, eta = 1 through the strided entry against ss_f0diff_sample, every transition alone from the case's inputs, on the case's
    tapes and on Philox with one seed. Tapes: BOTH entries meet the controlled-net check of the classic statement (f0 <= 1.0 x f0_step_bound,
    0 decided flips) - the strided one with its own few-ulp coefficients, which is the stride-1 identity. Philox: the uniforms are exact on the
    host (oracle.philox), so the classes are checked the same way; the Gaussian draw is the device's own Box-Muller, so f0 is compared between the
    two entries: within the sum of their two bounds plus the coefficient shift. Bit equality is not expected (and recorded, not asserted)."""
    spec, tables = SR.CASES[name], G._tables()
    base = SR.controlled_case(name, tables)
    B, T = base["B"], base["T"]
    model = G._controlled_model(spec["wset"])
    net = G._f0_net(model, None if spec["paired"] else spec["single"])
    seed_dev = 0x2468ACE
    for mode in ("tape", "philox"):
        case = base
        kw = dict(z=base["z"], u=base["u"])
        if mode == "philox":    # what the kernels draw for (seed = 17, device word): u exactly, z to the device's Box-Muller error
            zu = [PH.f0_step_draws(B, T, t, PH.make_key(17, 0, seed_dev)) for t in range(S)]
            case = dict(base, z=np.stack([a[0] for a in zu]).astype(np.float32), u=np.stack([a[1] for a in zu]).astype(np.float32),
                        regimes=dict(base["regimes"], target=np.zeros_like(base["regimes"]["target"])))
            assert np.array_equal(case["u"].astype(F64), np.stack([a[1] for a in zu])), "24-bit uniforms are exact in fp32"
            kw = dict(seed=17, seed_dev=seed_dev)
        run = _Run(net, B=B, T=T, cond=base["cond"], lo=base["lo"], hi=base["hi"], lens=base["lens"], **kw)
        for i, t in enumerate(ALL):
            outs = {}
            for entry in ("classic", "strided"):
                f, u = G._state(base["f0"], base["uv"])
                if entry == "classic":
                    run.classic(f, u, t, t + 1, 1)
                else:
                    run.strided(f, u, ALL, i, i + 1, 1.0, 1)
                outs[entry] = G._split(f, u, B, T)
            chks = {e: SR.check_controlled_step(case, tables, t, *outs[e]) for e in outs}
            ndiff = int((outs["classic"][0] != outs["strided"][0]).sum())
            d = np.abs(outs["classic"][0].astype(F64) - outs["strided"][0])
            record_measurement("f0_strided_stride1", case=name, mode=mode, t=t, f0_elements_differing=ndiff, f0_max_diff=float(d.max()),
                               uv_elements_differing=int((outs["classic"][1] != outs["strided"][1]).sum()),
                               classic_ratio=chks["classic"]["f0_ratio"], strided_ratio=chks["strided"]["f0_ratio"])
            print(f"[{name} {mode} t {t}] entries differ in {ndiff} f0 elements (max {d.max():.3e}); classic {chks['classic']['f0_ratio']:.3f} x, "
                  f"strided {chks['strided']['f0_ratio']:.3f} x bound")
            for e, chk in chks.items():
                assert chk["flips"] == 0 and int(chk["undecided"].sum()) <= 0.01 * int(base["valid"].sum()), (name, mode, t, e, chk["flips"])
                if mode == "tape":
                    assert chk["f0_ratio"] <= 1.0, (name, mode, t, e, chk["f0_ratio"])
            if mode == "philox":
                ref = chks["classic"]["ref"]
                bound = SR.f0_step_bound(case["f0"], ref["eps"], case["lo"], case["hi"], case["z"][t], SR.f0_coef(tables, t), t, ref["e_eps"])
                lim = 2.0 * bound + _coef_shift_bound(case, tables, t, ref["eps"])
                assert np.all(d <= lim), (name, t, float((d / lim).max()))


def _zero_final_model():
    """the synthetic weights with the final projection of both f0 denoisers zeroed: eps = l0 = l1 = 0, so a step depends on the draws alone"""
    sd = dict(G._base_sd())
    for net in G.F0_NETS:
        for k in ("output_projection.weight", "output_projection.bias"):
            sd[f"{net}.{k}"] = sd[f"{G.ALIASES[net]}.{k}"] = torch.zeros_like(sd[f"{net}.{k}"])
    return G._model("zero_final", sd)


def test_stride_one_consumes_the_default_entrys_draws():
    """Final projection = 0: x' = c1 clamp(recip x) + c2 x + sigma z and the class follows u and the previous class alone. The whole loops of the
    two entries then agree to the coefficient differences - 4 steps of products of magnitude <= ~10 moving by 1e-6 each: 1e-4 - on tapes and on
    Philox, where a draw taken from another row or counter would show at the size of sigma z (~0.1). With a swapped tape row they do differ."""
    inp = G._real_inputs()
    B, T = inp["B"], inp["T"]
    net = G._f0_net(_zero_final_model())
    wide = dict(lo=np.full_like(inp["lo"], -1e4), hi=np.full_like(inp["hi"], 1e4))     # the clamp idle: z of every step reaches the output
    for mode in ("tape", "philox"):
        kw = dict(z=inp["z"], u=inp["u"]) if mode == "tape" else dict(seed=17, seed_dev=0x1234567)
        run = _Run(net, B=B, T=T, cond=inp["cond"], lens=inp["lens"], **wide, **kw)
        f_c, u_c = G._state(inp["f0"], inp["uv"])
        run.classic(f_c, u_c, 0, S, 1)
        f_s, u_s = G._state(inp["f0"], inp["uv"])
        run.strided(f_s, u_s, ALL, 0, S, 1.0, 1)
        d = float((f_c - f_s).abs().max())
        nu = int((u_c != u_s).sum())
        record_measurement("f0_strided_draws", mode=mode, f0_max_diff=d, uv_elements_differing=nu)
        print(f"[draws {mode}] f0 max diff {d:.3e}, {nu} classes differ")
        assert bool(torch.isfinite(f_s).all()) and d <= 1e-4 and nu == 0, (mode, d, nu)
        assert float((f_s[:B * T] - G._d(inp["f0"]).reshape(-1)).abs().max()) > 1e-2
    z_sw = inp["z"].copy()
    z_sw[[1, 2]] = z_sw[[2, 1]]
    run = _Run(net, B=B, T=T, cond=inp["cond"], lens=inp["lens"], z=z_sw, u=inp["u"], **wide)
    f_x, u_x = G._state(inp["f0"], inp["uv"])
    run.strided(f_x, u_x, ALL, 0, S, 1.0, 1)
    assert float((f_x - f_c).abs().max()) > 1e-2, "exchanging two tape rows changed nothing: the check above bears no load"


# ------------------------------------------------------------------------------------------------
# 4. loop cuts   5. tape addressing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [1.0, 0.5])
def test_loop_cut_is_bit_identical(eta):
    """The list [3, 1, 0] in one call == one call per position == a 2 + rest cut, only the first call precomputing, bit for bit in f0 and uv, with
    tapes and with Philox. Every call but the first of a cut takes its first input row from f0_input_kernel where the one-call loop takes the tail
    kernel's."""
    inp = G._real_inputs()
    B, T = inp["B"], inp["T"]
    net = G._f0_net(G._model("real", G._base_sd()))
    ts = [3, 1, 0]
    for mode in ("tape", "philox"):
        kw = dict(z=inp["z"], u=inp["u"]) if mode == "tape" else dict(seed=17, seed_dev=0x1234567)
        run = _Run(net, B=B, T=T, cond=inp["cond"], lo=inp["lo"], hi=inp["hi"], lens=inp["lens"], **kw)
        f, u = G._state(inp["f0"], inp["uv"])
        run.strided(f, u, ts, 0, 3, eta, 1)
        whole = (f.clone(), u.clone())
        G._split(f, u, B, T)
        assert bool(torch.isfinite(whole[0]).all()) and float((whole[0][:B * T] - G._d(inp["f0"]).reshape(-1)).abs().max()) > 1e-3
        for cname, cuts in (("single", [(0, 1), (1, 2), (2, 3)]), ("2+rest", [(0, 2), (2, 3)])):
            f, u = G._state(inp["f0"], inp["uv"])
            for j, (a, b) in enumerate(cuts):
                run.strided(f, u, ts, a, b, eta, 1 if j == 0 else 0)
            nf, nu = int((f != whole[0]).sum()), int((u != whole[1]).sum())
            record_measurement("f0_strided_cut", mode=mode, cut=cname, eta=eta, f0_elements_differing=nf, uv_elements_differing=nu)
            assert torch.equal(f, whole[0]) and torch.equal(u, whole[1]), f"{mode} cut {cname}: {nf} f0 and {nu} uv elements differ from the one-call loop"


def test_tapes_are_addressed_by_network_time():
    """[3, 1, 0]: tapes whose rows of time 2 (not in the list) are NaN give the bits of clean tapes; with eta = 0 an all-NaN Gaussian tape gives
    finite output, identical to a clean tape's and to no Gaussian tape at all."""
    inp = G._real_inputs()
    B, T = inp["B"], inp["T"]
    net = G._f0_net(G._model("real", G._base_sd()))
    ts = [3, 1, 0]

    def go(z, u, eta):
        run = _Run(net, B=B, T=T, cond=inp["cond"], lo=inp["lo"], hi=inp["hi"], lens=inp["lens"], z=z, u=u)
        f, uu = G._state(inp["f0"], inp["uv"])
        run.strided(f, uu, ts, 0, 3, eta, 1)
        G._split(f, uu, B, T)
        return f, uu
    z_nan, u_nan = inp["z"].copy(), inp["u"].copy()
    z_nan[2], u_nan[2] = np.nan, np.nan
    for eta in (1.0, 0.5):
        clean, holed = go(inp["z"], inp["u"], eta), go(z_nan, u_nan, eta)
        assert bool(torch.isfinite(clean[0]).all())
        assert torch.equal(clean[0], holed[0]) and torch.equal(clean[1], holed[1]), f"eta {eta}: a row of a time outside the list was read"
    z_moved = inp["z"].copy()
    z_moved[1] += 1.0
    assert not torch.equal(go(z_moved, inp["u"], 1.0)[0], go(inp["z"], inp["u"], 1.0)[0]), "row 1 (in the list) is not read"
    det = go(inp["z"], inp["u"], 0.0)
    for z in (np.full_like(inp["z"], np.nan), None):
        other = go(z, inp["u"], 0.0)
        assert bool(torch.isfinite(other[0]).all()) and torch.equal(other[0], det[0]) and torch.equal(other[1], det[1])
    assert not torch.equal(det[0], go(inp["z"], inp["u"], 1.0)[0])


# ------------------------------------------------------------------------------------------------
# 6. the whole model
# ------------------------------------------------------------------------------------------------
SEED = 77
_gold = {}


def _golden_case():
    """golden acoustic_tiny_s4 built as tests/test_gpu_parity._run_hip builds it: two models of the same weights, one of which never runs strided"""
    if not _gold:
        case = harness.load_case("acoustic_tiny_s4")
        meta = case["meta"]
        hp, sd, batch = harness.case_setup(meta)
        models = []
        for _ in range(2):
            m = StyleSingerHIP(None, hparams=hp)
            m.load_state_dict(sd, strict=True)
            m.eval().to(DEV)
            models.append(m)
        b = {k: v.to(DEV) for k, v in batch.items()}
        kw = dict(mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"], ref_f0=b["ref_f0"],
                  global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"])
        _gold.update(meta=meta, gold=case["out"], models=models, txt=b["txt_tokens"], kw=kw)
    return _gold


def _fwd(model, c, **kw):
    ret = model(c["txt"], **{**c["kw"], **kw})
    torch.cuda.synchronize()
    return ret


def test_forward_all_steps_eta_one_meets_the_goldens_bounds():
    """forward(f0_steps = f0_timesteps, f0_eta = 1) on the golden's noise tape goes through the strided entry and meets what
    test_acoustic_hip_matches_reference_golden asks of the default path on this golden."""
    c = _golden_case()
    meta, gold = c["meta"], c["gold"]
    assert meta["steps_f0"] == 4
    model = c["models"][0]
    model.use_graphs = "off"
    noise = synth.draw_acoustic_noise(synth.NoiseTape(meta["tape_seed"]), meta["B"], meta["T"], meta["steps_f0"], meta["steps_mel"])
    calls = []
    orig = model._run_f0_pair
    model._run_f0_pair = lambda pl, tape=None, ts=None, eta=1.0: (calls.append((ts, eta)), orig(pl, tape, ts=ts, eta=eta))[1]
    try:
        ret = _fwd(model, c, noise=noise, f0_steps=meta["steps_f0"], f0_eta=1.0)
    finally:
        del model._run_f0_pair
    assert calls == [([3, 2, 1, 0], 1.0)], "the strided entry did not run"
    err = (ret["pitch_pred"].cpu() - gold["pitch_pred"]).abs().max().item()
    assert err <= P.STAGE_TOL, f"pitch_pred max abs err {err:.3e}"
    uv_flip = ((ret["pitch_pred"][..., 1].cpu() > 0) != (gold["pitch_pred"][..., 1] > 0)).float().mean().item()
    assert uv_flip == 0.0, f"voicing flips {uv_flip}"
    assert torch.allclose(ret["f0_denorm"].cpu(), gold["f0_denorm"], rtol=2e-4, atol=1e-2)
    l1 = (ret["mel_out"].cpu() - gold["mel_out"]).abs().mean().item()
    record_measurement("f0_strided_golden", case="acoustic_tiny_s4", pitch_pred_err=err, mel_l1=l1)
    print(f"acoustic_tiny_s4 through the strided entry: pitch_pred max abs err {err:.3e}, mel L1 {l1:.3e}")
    assert l1 <= P.MEL_L1_TOL, f"mel L1 {l1:.3e}"


def test_forward_two_steps_eager_graph_default_slot_and_feedback():
    """forward(f0_steps = 2): eager == captured-and-replayed == replayed again, bit for bit, under graph slot ("f0", 2, 1.0); the default call
    afterwards replays slot "f0" and equals, bit for bit, the same call on a model that never ran strided; and the strided forward's pitch_pred
    fed back as f0 = / uv = reproduces its mel_out bits."""
    c = _golden_case()
    model, fresh = c["models"]
    same = ("f0_a", "uv_a", "f0_b", "uv_b", "pitch_pred", "f0_denorm", "mel_out")
    model.use_graphs = "off"
    eager = _fwd(model, c, seed=SEED, f0_steps=2)
    model.use_graphs = "on"
    first = _fwd(model, c, seed=SEED, f0_steps=2)
    again = _fwd(model, c, seed=SEED, f0_steps=2)
    pl = next(iter(model._plans.values()))
    assert ("f0", 2, 1.0) in pl.graphs
    for k in same:
        assert torch.equal(eager[k], first[k]) and torch.equal(eager[k], again[k]), k
    assert bool(torch.isfinite(eager["mel_out"]).all())
    # another sampler, not a relabelled default loop
    default = _fwd(model, c, seed=SEED)
    assert pl.g_f0 is not None and pl.g_f0 is pl.graphs["f0"] and pl.graphs["f0"] is not pl.graphs[("f0", 2, 1.0)]
    assert not torch.equal(default["f0_a"], eager["f0_a"])
    det = _fwd(model, c, seed=SEED, f0_steps=2, f0_eta=0.0)
    assert ("f0", 2, 0.0) in pl.graphs and not torch.equal(det["f0_a"], eager["f0_a"])
    fresh.use_graphs = "on"
    untouched = _fwd(fresh, c, seed=SEED)
    assert set(next(iter(fresh._plans.values())).graphs) == {"f0", "mel"}
    for k in same:
        assert torch.equal(default[k], untouched[k]), k
    replay = _fwd(model, c, seed=SEED)
    for k in same:
        assert torch.equal(default[k], replay[k]), k
    # feed-back: the mel loop draws what it drew, whichever f0 sampler ran
    model.use_graphs = "off"
    given = _fwd(model, c, seed=SEED, f0=eager["pitch_pred"][..., 0], uv=eager["pitch_pred"][..., 1])
    for k in ("f0_denorm", "pitch_coarse", "pitch_pred", "decoder_inp", "mel_out"):
        assert torch.equal(given[k], eager[k]), k
    with pytest.raises(ValueError, match="f0_steps"):
        _fwd(model, c, seed=SEED, f0=eager["pitch_pred"][..., 0], uv=eager["pitch_pred"][..., 1], f0_steps=2)


def test_a_checkpoint_whose_tables_do_not_fit_its_betas_is_refused_for_strided_sampling_only():
    sd = dict(G._base_sd())
    for gen in ("f0_gen", "f0_gen_inpainte"):
        bad = sd[gen + ".log_cumprod_alpha"].clone()
        bad[2] *= 1.001
        sd[gen + ".log_cumprod_alpha"] = bad
    model = G._model("bad_tables", sd)
    sched = model._pk["f0_pair"]["sched"]
    assert sched["strided_error"] is not None and sched["strided_dev"] > 1e-6
    assert G._model("real", G._base_sd())._pk["f0_pair"]["sched"]["strided_error"] is None
    pl = model._plan(1, 64, torch.device(DEV))
    with pytest.raises(L.StyleSingerHipError, match="strided f0 sampling .* refused"):
        model._run_f0_pair(pl, ts=[3, 1, 0], eta=1.0)
