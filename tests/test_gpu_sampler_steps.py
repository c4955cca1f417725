"""GPU unit parity of the joint f0 / uv sampler step (f0_input_kernel, f0_tail_kernel, f0_update_row of csrc/f0_sampler.hip) and of the samplers'
loop-cut contract, through the C-ABI (ss_f0diff_sample, ss_meldiff_sample, ss_mel_qsample, ss_mel_denorm) against the float64 statements of
tests/sampler_step_refs.py (themselves checked by tests/test_sampler_step_refs_cpu.py, which also asserts the input conditions used here).

The paired net comes the product's way: StyleSingerHIP(None, hparams=...) with f0_timesteps = 4, a synthetic state dict, .to(device), pack,
`_pk["f0_pair"]["net"]` - production C = 192, L = 10, n_groups = 2. State buffers carry a sentinel tail (7.0 / -7).

Tolerances (none taken from a kernel's output):
  * controlled net (skip_projection.weight = 0, so the stack's output is relu(beta) exactly and (eps, l0, l1) a 192-term fp32 dot product of
    known operands): eps within K 2^-24 sum |g w| + one rounding for the bias; f0 within that pushed through the step plus one rounding for each of
    its 10 fp32 operations (sampler_step_refs.f0_step_bound lists them). uv identical on every frame whose float64 margin is at least
    thr = max(4 x the fp32-CPU margin error of the case, 8 fp32 ulp at the frame's largest intermediate); the share of frames below thr is
    asserted <= 1 % of the valid frames.
  * real weights: f0 within 4 x the fp32 CPU oracle's own error against float64 (never less than 2 ulp), thr as above with the network's fp32
    error inside the measured margin error.
  * loop cuts: bit-identical (torch.equal), except the mel sampler with the `mel_tail` knob on, where cut and whole differ by the summation order
    of the input projection: the project's bound for exactly that (tests/test_gpu_round4.py, max <= 1e-5 and mean <= 1e-6).
  * ss_mel_qsample: 8 fp32 roundings (mel - min, max - min, the quotient, * 2, - 1, sa *, s1 *, the sum), ss_mel_denorm: 4 (x + 1, max - min,
    the product, + min; / 2 is exact): one ulp each at the largest magnitude the element passes through.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sampler_step_refs as SR  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import restatement as R  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

DEV = "cuda:0"
SENT, SENT_I = 7.0, -7
TAIL = 37            # sentinel elements behind every state buffer
S = SR.S_F0
F64 = np.float64
F0_NETS = ("gm_diffnet", "gm_diffnet_inpainte")
ALIASES = {"gm_diffnet": "f0_gen._denoise_fn", "gm_diffnet_inpainte": "f0_gen_inpainte._denoise_fn"}   # the same modules, registered twice

_cache = {}


def _hp(**over):
    return config.make_hparams(dict(timesteps=4, K_step=4, f0_timesteps=S, **over))


def _base_sd():
    if "sd" not in _cache:
        _cache["sd"] = synth.synth_acoustic_state_dict(_hp(), 77)
    return _cache["sd"]


def _tables():
    sd = _base_sd()
    return {k[len("f0_gen."):]: v.numpy() for k, v in sd.items() if k.startswith("f0_gen.") and "_denoise_fn" not in k and v.dim() == 1}


def _model(key, sd, **hp_over):
    if key not in _cache:
        m = StyleSingerHIP(None, hparams=_hp(**hp_over))
        m.load_state_dict(sd)
        m.eval().to(DEV)
        m._ensure_packed()
        _cache[key] = m
    return _cache[key]


def _controlled_model(wset):
    """the synthetic weights with, in both f0 denoisers, skip_projection.weight = 0, skip_projection.bias = beta and the final projection of the
    weight set (different per net)"""
    key = "controlled_" + wset
    if key in _cache:
        return _cache[key]
    sd = dict(_base_sd())
    for net, w in zip(F0_NETS, SR.controlled_weights(wset)):
        new = {"skip_projection.weight": torch.zeros_like(sd[net + ".skip_projection.weight"]),
               "skip_projection.bias": torch.from_numpy(w["beta"].copy()),
               "output_projection.weight": torch.from_numpy(w["w_final"].copy())[:, :, None],
               "output_projection.bias": torch.from_numpy(w["b_final"].copy())}
        for k, v in new.items():
            assert sd[f"{net}.{k}"].shape == v.shape
            sd[f"{net}.{k}"] = sd[f"{ALIASES[net]}.{k}"] = v
    return _model(key, sd)


def _f0_net(model, single=None):
    """the product's paired descriptor, or a one-net descriptor of the same packed weights (odd item counts)"""
    if single is None:
        return model._pk["f0_pair"]["net"]
    key = ("single", id(model), single)
    if key not in _cache:
        hp = model.hp
        _cache[key] = model._pack_wavenet([F0_NETS[single]], "f0_gen", hp["f0_residual_channels"], hp["f0_residual_layers"],
                                          hp["f0_dilation_cycle_length"], hp["f0_timesteps"], 1, 3, True)
    return _cache[key]["net"]


def _d(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _state(f0, uv):
    """f0 / uv device buffers with a sentinel tail"""
    n = f0.size
    f = torch.full((n + TAIL,), SENT, device=DEV)
    u = torch.full((n + TAIL,), SENT_I, device=DEV, dtype=torch.int32)
    f[:n] = _d(f0.reshape(-1).astype(np.float32))
    u[:n] = _d(uv.reshape(-1).astype(np.int32))
    return f, u


class _F0Run:
    """ss_f0diff_sample on one set of inputs: device copies made once, one workspace kept across calls (a cut loop precomputes once)"""

    def __init__(self, net, *, B, T, cond, lo, hi, lens, z=None, u=None, seed=17, seed_dev=None):
        self.lib, self.net, self.B, self.T = L.load(), net, B, T
        self.cond, self.lo, self.hi = _d(cond), _d(lo), _d(hi)
        self.lens = _d(np.asarray(lens, np.int32))
        self.z = None if z is None else _d(z)
        self.u = None if u is None else _d(u)
        self.seed = seed
        self.seed_dev = None if seed_dev is None else torch.tensor([seed_dev], device=DEV, dtype=torch.int64)
        self.wsb = self.lib.ss_wavenet_workspace_bytes(ctypes.addressof(net), B, T)
        assert self.wsb > 0
        self.ws = torch.empty(self.wsb, device=DEV, dtype=torch.uint8)

    def __call__(self, f, u, lo_step, hi_step, precompute):
        L.check(self.lib.ss_f0diff_sample(ctypes.addressof(self.net), L.ptr(f), L.ptr(u), L.ptr(self.cond), L.ptr(self.lo), L.ptr(self.hi), L.ptr(self.lens),
                                          self.B, self.T, L.ptr(self.z), L.ptr(self.u), self.seed, L.ptr(self.seed_dev), lo_step, hi_step, precompute,
                                          L.ptr(self.ws), self.wsb, L.stream_ptr()), "ss_f0diff_sample")
        torch.cuda.synchronize()


def _split(f, u, B, T):
    n = B * T
    assert bool((f[n:] == SENT).all()) and bool((u[n:] == SENT_I).all()), "rows beyond B*T were written"
    return f[:n].cpu().numpy().reshape(B, T), u[:n].cpu().numpy().reshape(B, T)


def _ksplit(B, T):
    return L.load().ss_gemm16_ksplit_pick(B, T, SR.C_F0, 10 * SR.C_F0)


# ------------------------------------------------------------------------------------------------
# a / b. controlled-output net: arithmetic, edges, strides, both SkipSrc forms
# ------------------------------------------------------------------------------------------------
def _controlled_core(case, spec, what):
    """steps S-1, 1 and 0 each alone from the case's inputs, judged by sampler_step_refs.check_controlled_step"""
    tables = _tables()
    model = _controlled_model(spec["wset"])
    net = _f0_net(model, None if spec["paired"] else spec["single"])
    B, T = case["B"], case["T"]
    run = _F0Run(net, B=B, T=T, cond=case["cond"], lo=case["lo"], hi=case["hi"], lens=case["lens"], z=case["z"], u=case["u"])
    n_valid = int(case["valid"].sum())
    outs = {}
    for step in (S - 1, 1, 0):
        f, u = _state(case["f0"], case["uv"])
        run(f, u, step, step + 1, 1)
        f0_out, uv_out = _split(f, u, B, T)
        chk = SR.check_controlled_step(case, tables, step, f0_out, uv_out)
        n_und = int(chk["undecided"].sum())
        record_measurement(f"sampler_step_{what}", case=case["name"], step=step, f0_err=chk["f0_err"], f0_bound=chk["f0_bound"], f0_ratio=chk["f0_ratio"],
                           cpu_fp32_f0_ratio=chk["cpu_f0_ratio"], uv_flips=chk["flips"], undecided=n_und, frames=B * T,
                           thr_max=float(chk["thr"].max()), cpu_margin_err=chk["cpu_margin_err"])
        print(f"[{case['name']} step {step}] f0 {chk['f0_err']:.3e} = {chk['f0_ratio']:.3f} x bound (fp32 CPU {chk['cpu_f0_ratio']:.3f} x); "
              f"uv flips {chk['flips']}, undecided {n_und} of {B * T}")
        assert n_und <= 0.01 * n_valid, (n_und, n_valid)
        assert set(np.unique(uv_out).tolist()) <= {0, 1}
        assert chk["f0_ratio"] <= 1.0, f"{case['name']} step {step}: f0 is {chk['f0_ratio']:.3g} x its bound (padded frames included)"
        assert chk["flips"] == 0, f"{case['name']} step {step}: {chk['flips']} decided frames got the other class, first at {np.argwhere(chk['flip_mask'])[:4].tolist()}"
        outs[step] = (f0_out, uv_out)
    return outs


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_controlled_net_single_steps(name):
    """Every regime of sampler_step_refs.controlled_case on known frames - initial uv 0 / 1, lo == hi / a band / idle clamps, u in {0, 2^-24,
    1 - 2^-24} in either slot, margins steered to +-5e-3, l0 - l1 = +-40 / ~0, ragged lens with lens = T and lens = 1, B*T mod 16 in {1, 2, 14, 15}
    - at steps S-1, 1 and 0, each run alone. Padded frames are updated by the kernel (eps = logits = 0, not b_final) and are checked like the rest;
    rows beyond B*T keep their sentinel. All of these shapes take the split-K slices form of the skip source (asserted).
    Paired cases run a second time with the two nets' items exchanged: the results follow the weights, not the slots."""
    spec = SR.CASES[name]
    case = SR.controlled_case(name, _tables())
    assert _ksplit(case["B"], case["T"]) > 1, "this shape no longer takes the slices form"
    outs = _controlled_core(case, spec, "controlled")
    if spec["paired"]:
        sw = SR.swapped_items(case)
        outs_sw = _controlled_core(sw, spec, "controlled_swapped")
        h = case["B"] // 2
        both = case["valid"] & np.roll(case["valid"], h, axis=0)
        for step in outs:
            back = np.roll(outs_sw[step][0], -h, axis=0)     # the swapped run's outputs in the original item order
            assert np.abs(back - outs[step][0])[both].max() > 1e-3, "exchanging the nets' items changed nothing: the per-net weights bear no load"


def test_controlled_net_reduced_skip_source():
    """The other SkipSrc form: the smallest T, not a multiple of 16, at which the split-K pick returns 1 for 16 items - the tail kernel then reads
    the reduced tensor G the skip GEMM wrote (bias, ReLU and row mask applied there). The precondition is asserted, so that a tuning change cannot
    silently drop the path."""
    B = 16
    T = next(t for t in range(1, 4000) if t % 16 and _ksplit(B, t) == 1)
    assert _ksplit(B, T) == 1 and T % 16 != 0
    spec = SR.reduced_spec(B, T)
    print(f"reduced form at B = {B}, T = {T}")
    _controlled_core(SR.controlled_case(spec, _tables()), spec, "controlled_reduced")


# ------------------------------------------------------------------------------------------------
# c. real weights: row indexing and the X hand-over
# ------------------------------------------------------------------------------------------------
REAL = dict(B=4, T=83, lens=[83, 41, 1, 70], seed=31)


def _real_inputs():
    r = np.random.default_rng(REAL["seed"])
    B, T = REAL["B"], REAL["T"]
    mid = r.uniform(-1, 1, (B, T))
    return dict(B=B, T=T, lens=np.asarray(REAL["lens"], np.int32), f0=r.standard_normal((B, T)).astype(np.float32),
                uv=r.integers(0, 2, (B, T)).astype(np.int32), lo=(mid - 0.25).astype(np.float32), hi=(mid + 0.25).astype(np.float32),
                z=r.standard_normal((S, B, T)).astype(np.float32), u=(r.integers(1, 1 << 24, (S, B, 2, T)) * SR.U24).astype(np.float32),
                cond=(r.standard_normal((B, T, 256)) * 0.5).astype(np.float32))


def _oracle_step(sd, hp, inp, f0, uv, step, dtype):
    """One step of both nets on the items of `inp` (first half net 0, second half net 1) in `dtype`: oracle.ddiffnet per item on its valid
    frames (the kernels mask rows >= lens, which is the network on the shorter sequence), then the step statement; padded frames with
    eps = logits = 0."""
    B, T, h = inp["B"], inp["T"], inp["B"] // 2
    tt = torch.float64 if dtype == torch.float64 else torch.float32
    out = np.zeros((B, T, 3), F64)
    torch.set_default_dtype(tt)
    try:
        with torch.no_grad():
            for b in range(B):
                n = int(inp["lens"][b])
                o = R.ddiffnet(sd, hp, torch.from_numpy(f0[b:b + 1, :n]).to(tt), torch.from_numpy(uv[b:b + 1, :n]).long(), torch.full((1,), step, dtype=torch.long),
                               torch.from_numpy(inp["cond"][b:b + 1, :n]).to(tt), F0_NETS[b // h])
                out[b, :n] = o[0].double().numpy()
    finally:
        torch.set_default_dtype(torch.float32)
    coef = SR.f0_coef(_tables(), step)
    return SR.f0_joint_step(f0, uv, out[..., 0], out[..., 1:], inp["lo"], inp["hi"], inp["z"][step], inp["u"][step], coef, step, dtype=tt)


def _check_real_step(name, inp, f0_in, uv_in, step, f0_out, uv_out, sd32, sd64, hp):
    f64, uv64, m64, mag = _oracle_step(sd64, hp, inp, f0_in, uv_in, step, torch.float64)
    f32_, _, m32, _ = _oracle_step(sd32, hp, inp, f0_in, uv_in, step, torch.float32)
    thr, cpu_m_err = SR.decision_threshold(m64, m32, mag)
    und = np.abs(m64) < thr
    cpu_err = float(np.abs(f32_ - f64).max())
    floor = 2.0 * float(np.spacing(np.float32(np.abs(f64).max())))
    bound = max(4.0 * cpu_err, floor)
    err = float(np.abs(f0_out.astype(F64) - f64).max()) if np.isfinite(f0_out).all() else float("inf")
    flips = int(((uv_out != uv64) & ~und).sum())
    record_measurement("sampler_step_real_" + name, step=step, kernel_err=err, cpu_fp32_err=cpu_err, bound=bound, ratio=err / bound, uv_flips=flips,
                       undecided=int(und.sum()), frames=int(und.size), cpu_margin_err=cpu_m_err, thr_max=float(thr.max()))
    print(f"[real {name} step {step}] f0 kernel {err:.3e} cpu-fp32 {cpu_err:.3e} bound {bound:.3e}; uv flips {flips}, undecided {int(und.sum())}, "
          f"cpu margin err {cpu_m_err:.3e}")
    assert int(und.sum()) <= 0.01 * int((np.arange(inp["T"])[None] < inp["lens"][:, None]).sum())
    assert err <= bound, (name, step, err, cpu_err, bound)
    assert flips == 0, (name, step, flips)


def test_real_weights_two_steps_and_the_x_handover():
    """Unmodified synthetic weights, steps S-1 and S-2, ragged lens, per-frame variety: against the step statement fed the float64 network output
    (oracle.ddiffnet on a float64 state dict). Step S-1 is a call of its own (its X row comes from f0_input_kernel). Step S-2 is judged on the
    ONE call [S-2, S), whose second evaluation reads the X row the tail kernel wrote; its reference starts from the device's own state after
    step S-1 (the same launches, the same bits: test_f0_loop_cut_is_bit_identical), so that a frame too close to call at S-1 cannot leak into S-2.
    Measured on an MI355X: kernel 1.5e-7 / 9.5e-8 against the CPU's 1.4e-7 / 9.2e-8, a quarter of the bound - the F(4,3) gate form needs no allowance."""
    hp, sd32 = _hp(), _base_sd()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    model = _model("real", sd32)
    inp = _real_inputs()
    B, T = inp["B"], inp["T"]
    run = _F0Run(_f0_net(model), B=B, T=T, cond=inp["cond"], lo=inp["lo"], hi=inp["hi"], lens=inp["lens"], z=inp["z"], u=inp["u"])
    f, u = _state(inp["f0"], inp["uv"])
    run(f, u, S - 1, S, 1)
    f0_1, uv_1 = _split(f, u, B, T)
    _check_real_step("first", inp, inp["f0"], inp["uv"], S - 1, f0_1, uv_1, sd32, sd64, hp)
    f, u = _state(inp["f0"], inp["uv"])
    run(f, u, S - 2, S, 1)
    f0_2, uv_2 = _split(f, u, B, T)
    _check_real_step("handover", inp, f0_1, uv_1, S - 2, f0_2, uv_2, sd32, sd64, hp)
    assert np.abs(f0_2 - f0_1).max() > 1e-3


# ------------------------------------------------------------------------------------------------
# d. loop-cut contract
# ------------------------------------------------------------------------------------------------
CUTS = {"single": [(t, t + 1) for t in reversed(range(S))], "2+2": [(2, 4), (0, 2)]}


def _f0_cut_identity(model, what):
    inp = _real_inputs()
    B, T = inp["B"], inp["T"]
    net = _f0_net(model)
    for mode in ("tape", "philox"):
        kw = dict(z=inp["z"], u=inp["u"]) if mode == "tape" else dict(seed=17, seed_dev=0x1234567)
        run = _F0Run(net, B=B, T=T, cond=inp["cond"], lo=inp["lo"], hi=inp["hi"], lens=inp["lens"], **kw)
        f, u = _state(inp["f0"], inp["uv"])
        run(f, u, 0, S, 1)
        whole = (f.clone(), u.clone())
        _split(f, u, B, T)
        assert bool(torch.isfinite(whole[0]).all()) and float((whole[0][:B * T] - _d(inp["f0"]).reshape(-1)).abs().max()) > 1e-3
        for cname, cuts in CUTS.items():
            f, u = _state(inp["f0"], inp["uv"])
            for i, (lo_s, hi_s) in enumerate(cuts):
                run(f, u, lo_s, hi_s, 1 if i == 0 else 0)
            nf, nu = int((f != whole[0]).sum()), int((u != whole[1]).sum())
            record_measurement("sampler_cut_" + what, mode=mode, cut=cname, f0_elements_differing=nf, uv_elements_differing=nu,
                               f0_max_diff=float((f - whole[0]).abs().max()))
            assert torch.equal(f, whole[0]) and torch.equal(u, whole[1]), \
                f"{what} {mode} cut {cname}: {nf} f0 and {nu} uv elements differ from the one-call loop (max {float((f - whole[0]).abs().max()):.3e})"


def test_f0_loop_cut_is_bit_identical():
    """ss_f0diff_sample(0, S, precompute = 1) in one call == S calls [t, t+1) == a 2 + 2 cut, only the first call precomputing, bit for bit in f0 and
    uv, with tapes and with Philox (noise = gumbel_u = NULL, the same seed / device seed word). Every call but the last of a cut takes its first X
    row from f0_input_kernel where the one-call loop takes the tail kernel's: the header's "exactly f0_input_kernel's values"."""
    _f0_cut_identity(_model("real", _base_sd()), "f0")


class _MelRun:
    def __init__(self, net, *, B, T, cond, lens, z=None, seed=29, seed_dev=None):
        self.lib, self.net, self.B, self.T = L.load(), net, B, T
        self.cond, self.lens = _d(cond), _d(np.asarray(lens, np.int32))
        self.z = None if z is None else _d(z)
        self.seed = seed
        self.seed_dev = None if seed_dev is None else torch.tensor([seed_dev], device=DEV, dtype=torch.int64)
        self.wsb = self.lib.ss_wavenet_workspace_bytes(ctypes.addressof(net), B, T)
        assert self.wsb > 0
        self.ws = torch.empty(self.wsb, device=DEV, dtype=torch.uint8)

    def __call__(self, x, lo_step, hi_step, precompute):
        L.check(self.lib.ss_meldiff_sample(ctypes.addressof(self.net), L.ptr(x), L.ptr(self.cond), L.ptr(self.lens), self.B, self.T, L.ptr(self.z), self.seed,
                                           L.ptr(self.seed_dev), lo_step, hi_step, precompute, L.ptr(self.ws), self.wsb, L.stream_ptr()), "ss_meldiff_sample")
        torch.cuda.synchronize()


def _mel_inputs():
    r = np.random.default_rng(41)
    B, T, M = 2, 97, 80
    lens = np.asarray([97, 60], np.int32)
    x = r.standard_normal((B, T, M)).astype(np.float32)
    x[np.arange(T)[None, :] >= lens[:, None]] = 0.0
    return dict(B=B, T=T, M=M, lens=lens, x=x, cond=(r.standard_normal((B, T, 256)) * 0.5).astype(np.float32),
                z=r.standard_normal((4, B, T, M)).astype(np.float32))


def _mel_cuts(model, what, exact):
    """whole loop vs the cuts of CUTS through the model's mel net; returns the largest (max, mean) difference seen"""
    inp = _mel_inputs()
    B, T, M = inp["B"], inp["T"], inp["M"]
    net = model._pk["mel"]["net"]
    assert net.steps == 4
    n = B * T * M
    worst = (0.0, 0.0)
    for mode in ("tape", "philox"):
        kw = dict(z=inp["z"]) if mode == "tape" else dict(seed=29, seed_dev=0x7654321)
        run = _MelRun(net, B=B, T=T, cond=inp["cond"], lens=inp["lens"], **kw)

        def fresh():
            x = torch.full((n + TAIL,), SENT, device=DEV)
            x[:n] = _d(inp["x"]).reshape(-1)
            return x
        x = fresh()
        run(x, 0, 4, 1)
        whole = x.clone()
        assert bool((whole[n:] == SENT).all()) and bool(torch.isfinite(whole).all())
        assert float((whole[:n] - _d(inp["x"]).reshape(-1)).abs().max()) > 1e-2
        for cname, cuts in CUTS.items():
            x = fresh()
            for i, (lo_s, hi_s) in enumerate(cuts):
                run(x, lo_s, hi_s, 1 if i == 0 else 0)
            d = (x - whole).abs()
            dmax, dmean, ndiff = float(d.max()), float(d[:n].mean()), int((x != whole).sum())
            record_measurement("sampler_cut_" + what, mode=mode, cut=cname, elements_differing=ndiff, max_diff=dmax, mean_diff=dmean)
            print(f"[{what} {mode} cut {cname}] {ndiff} elements differ, max {dmax:.3e} mean {dmean:.3e}")
            if exact:
                assert torch.equal(x, whole), f"{what} {mode} cut {cname}: {ndiff} elements differ from the one-call loop (max {dmax:.3e})"
            worst = (max(worst[0], dmax), max(worst[1], dmean))
    return worst


def test_mel_loop_cut():
    """ss_meldiff_sample through the product's mel net (K_step = 4), whole loop against single-step and 2 + 2 cuts, tapes and Philox. With the
    `mel_tail` knob at 0 every evaluation is the same launches however the loop is cut: bit-identical. With the knob at its default a call's
    first evaluation takes its input projection from the matrix-core launch and later ones from mel_tail_kernel: the same fp32 products in
    another summation order, held to the project's bound for exactly that difference (test_small_launch_tail_kernels_agree...: max <= 1e-5,
    mean <= 1e-6)."""
    lib = L.load()
    model = _model("real", _base_sd())
    before = lib.ss_get_tuning(b"mel_tail")
    assert before == 1
    try:
        dmax, dmean = _mel_cuts(model, "mel_tail_on", exact=False)
        L.check(lib.ss_set_tuning(b"mel_tail", 0), "mel_tail")
        _mel_cuts(model, "mel_tail_off", exact=True)
    finally:
        L.check(lib.ss_set_tuning(b"mel_tail", before), "mel_tail")
    assert dmax <= 1e-5 and dmean <= 1e-6, (dmax, dmean)


def test_fp16sd_loop_cut_is_bit_identical():
    """mfma_precision = "fp16sd" at a small shape, 3 weight sets and 3 addend sets over 4 evaluations (the set index wraps inside the loop): evaluation j
    reads set j % n whichever call it falls into, so cut and whole are bit-identical - for the mel sampler and for the f0 pair (which keeps the
    three-product bf16 form in this mode)."""
    model = _model("fp16sd", _base_sd(), mfma_precision="fp16sd", fp16sd_sets=3, fp16sd_e_sets=3)
    assert model._pk["mel"]["net"].n_wsets == 3
    _mel_cuts(model, "mel_fp16sd", exact=True)
    _f0_cut_identity(model, "f0_fp16sd")


# ------------------------------------------------------------------------------------------------
# e. ss_mel_qsample / ss_mel_denorm values and mask
# ------------------------------------------------------------------------------------------------
def _ulps(out, ref, mag, n):
    tol = n * np.spacing(np.abs(mag).astype(np.float32)).astype(F64)
    d = np.abs(out.astype(F64) - ref)
    assert np.isfinite(out).all()
    return float((d / tol).max()), int((d > tol).sum())


def test_mel_qsample_and_denorm_values_beyond_one_grid_pass():
    """A recorded noise, the model's spec_min / spec_max, ragged lens and rows*M = 2 160 240 > 8192 blocks x 256 threads (the grid cap: the
    grid-stride loops take a second pass), sentinel behind the output. q-sample has no row mask; denorm zeroes rows >= lens."""
    lib = L.load()
    hp = _hp()
    B, T, M = 3, 9001, 80
    assert B * T * M > 8192 * 256
    lens_h = [9001, 4500, 1]
    r = np.random.default_rng(51)
    smin = np.asarray(hp["spec_min"], np.float32)[:M]
    smax = np.asarray(hp["spec_max"], np.float32)[:M]
    mel = (smin + (smax - smin) * r.uniform(-0.05, 1.05, (B, T, M))).astype(np.float32)
    z = r.standard_normal((B, T, M)).astype(np.float32)
    sa, s1 = np.float32(0.8671875), np.float32(0.498046875)
    n = B * T * M
    x = torch.full((n + TAIL,), SENT, device=DEV)
    mel_d, smin_d, smax_d, z_d = _d(mel), _d(smin), _d(smax), _d(z)      # named: they must outlive the launches
    L.check(lib.ss_mel_qsample(L.ptr(mel_d), L.ptr(smin_d), L.ptr(smax_d), float(sa), float(s1), L.ptr(z_d), 0, None, L.ptr(x), B, T, M,
                               L.stream_ptr()), "qsample")
    torch.cuda.synchronize()
    assert bool((x[n:] == SENT).all()), "ss_mel_qsample wrote behind B*T*M"
    ref, mag = SR.mel_qsample(mel, smin, smax, float(sa), float(s1), z)
    x_h = x[:n].cpu().numpy().reshape(B, T, M)
    q_ratio, q_bad = _ulps(x_h, ref, mag, 8)
    # denorm of the device's own q-sample (fp32 values, widened)
    lens = _d(np.asarray(lens_h, np.int32))
    out = torch.full((n + TAIL,), SENT, device=DEV)
    L.check(lib.ss_mel_denorm(L.ptr(x), L.ptr(smin_d), L.ptr(smax_d), L.ptr(out), B, T, M, L.ptr(lens), None, L.stream_ptr()), "denorm")
    torch.cuda.synchronize()
    assert bool((out[n:] == SENT).all()), "ss_mel_denorm wrote behind B*T*M"
    dref, dmag = SR.mel_denorm(x_h, smin, smax, lens=lens_h)
    o_h = out[:n].cpu().numpy().reshape(B, T, M)
    valid = np.arange(T)[None, :] < np.asarray(lens_h)[:, None]
    assert np.all(o_h[~valid] == 0.0), "rows >= lens are not zero"
    d_ratio, d_bad = _ulps(o_h[valid], dref[valid], dmag[valid], 4)
    record_measurement("sampler_mel_qsample_denorm", qsample_err_over_8ulp=q_ratio, denorm_err_over_4ulp=d_ratio, elements=n)
    print(f"q-sample {q_ratio:.3f} x 8 ulp, denorm {d_ratio:.3f} x 4 ulp over {n} elements")
    assert q_bad == 0 and d_bad == 0, (q_ratio, q_bad, d_ratio, d_bad)
