"""GPU unit parity of the mel sampler step in every sampler and launch form - mel_tail_kernel, the SS_EPI_DDPM epilogue of ss_conv_gemm (both
round through ss_ddpm_update, csrc/common.h), ss_prodiff_sample, ss_meldiff_sample_ddim (ddim_coef), ss_meldiff_sample_plms and ss_mel_denorm's
`nonfinite` flag - through the C-ABI against the float64 statements of tests/mel_step_refs.py (themselves checked against the oracle, with the
case table's regimes and the wrong variants it catches, by tests/test_mel_step_refs_cpu.py).

The nets come the product's way (StyleSingerHIP(None, hparams=...), a synthetic state dict, pack, `_pk["mel"]["net"]`: production C = 256,
L = 20, M = 80) with the helpers of tests/test_gpu_sampler_steps.py. State buffers carry a sentinel tail; tuning knobs are restored in `finally`.

Tolerances (none taken from a kernel's output):
  * controlled net (skip_projection.weight = 0, so the stack's output is relu(beta) exactly and eps[n] a 256-term fp32 dot product of known
    operands): per element, mel_step_refs.mel_step_bound - eps within K 2^-24 sum |g w| + one rounding for the bias, pushed through the step, plus
    one rounding for each of its 9 fp32 operations; padded rows exactly 0. Chains of steps (ProDiff, DDIM) feed each step's bound to the next.
    The table's weights are dyadic: the dot product is exact in fp32 in any order, so its eps term is 0 (the bound is the step's own roundings
    alone, some 1e-7: a coefficient off in its last digits shows) and the two launch forms - which sum it in different orders - reach the same
    eps and, by ss_ddpm_update's promise, the same bits: torch.equal. With a projection that rounds (wset "random") the eps term bears load
    and the forms' eps may differ in the last bits, which the code does not promise away (mel_tail_kernel: "only the summation order over K
    differs"); both are held to the bound there and the number of differing elements is recorded.
  * real weights: 4 x the fp32-CPU oracle's own error against the float64 oracle on the same inputs, never less than 2 ulp of the largest value.
"""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mel_step_refs as MR  # noqa: E402
import sampler_step_refs as SR  # noqa: E402
import test_gpu_sampler_steps as GS  # noqa: E402  (its helpers: _hp, _base_sd, _model, _MelRun, _d, the sentinels)
from conftest import record_measurement  # noqa: E402
from oracle import restatement as R  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

DEV, SENT, TAIL = GS.DEV, GS.SENT, GS.TAIL
F64, f32 = np.float64, np.float32
K, M, C = MR.K_MEL, MR.M_MEL, MR.C_MEL
LAYERS = 20
NET = "postdiff.denoise_fn."
_d = GS._d
_cache = {}


def _tables(sd=None):
    sd = sd or GS._base_sd()
    return {k[len("postdiff."):]: v.double().numpy() for k, v in sd.items() if k.startswith("postdiff.") and "denoise_fn" not in k and v.dim() == 1}


def _controlled_sd(sd, wset):
    sd, w = dict(sd), MR.controlled_mel_weights(wset)
    new = {"skip_projection.weight": torch.zeros_like(sd[NET + "skip_projection.weight"]), "skip_projection.bias": torch.from_numpy(w["beta"].copy()),
           "output_projection.weight": torch.from_numpy(w["w_final"].copy())[:, :, None], "output_projection.bias": torch.from_numpy(w["b_final"].copy())}
    for k, v in new.items():
        assert sd[NET + k].shape == v.shape, k
        sd[NET + k] = v
    return sd


def _controlled_model(wset="dyadic"):
    return GS._model("mel_controlled_" + wset, _controlled_sd(GS._base_sd(), wset))


def _extreme():
    """the controlled net under the 1000-step schedule of BASELINE config 4 (timesteps = K_step = 1000, max_beta = 0.06)"""
    if "extreme" not in _cache:
        hp = config.make_hparams(dict(timesteps=1000, K_step=1000, f0_timesteps=GS.S))
        sd = _controlled_sd(synth.synth_acoustic_state_dict(hp, 77), "dyadic")
        m = StyleSingerHIP(None, hparams=hp)
        m.load_state_dict(sd)
        m.eval().to(DEV)
        m._ensure_packed()
        _cache["extreme"] = (m, _tables(sd))
    return _cache["extreme"]


def _fresh(x):
    buf = torch.full((x.size + TAIL,), SENT, device=DEV)
    buf[:x.size] = _d(np.asarray(x, f32)).reshape(-1)
    return buf


def _take(buf, shape):
    n = int(np.prod(shape))
    assert bool((buf[n:] == SENT).all()), "elements beyond B*T*M were written"
    return buf[:n].cpu().numpy().reshape(shape)


@contextlib.contextmanager
def _knob(name, value):
    lib = L.load()
    before = lib.ss_get_tuning(name)
    try:
        L.check(lib.ss_set_tuning(name, value), name.decode())
        yield
    finally:
        L.check(lib.ss_set_tuning(name, before), name.decode())


def _ksplit(B, T):
    return L.load().ss_gemm16_ksplit_pick(B, T, C, LAYERS * C)


def _assert_form(net, B, T, tail, ksplit_gt1=None):
    """the preconditions of the launch form a test relies on (resolve_form's rules), so that a tuning change cannot silently drop it"""
    assert net.C == C and net.L == LAYERS and net.in_dim == M and net.mfma_bf16 == 0
    assert L.load().ss_get_tuning(b"mel_tail") == (1 if tail else 0)
    if tail:
        assert B * T <= 8 * torch.cuda.get_device_properties(0).multi_processor_count, "this shape no longer takes mel_tail_kernel"
    if ksplit_gt1 is not None:
        k = _ksplit(B, T)
        assert (k > 1) if ksplit_gt1 else (k == 1), f"split-K pick {k} at B = {B}, T = {T}"


def _judge(what, out, ref, bound, valid, **tags):
    ratio, bad = MR.over_bound(out, ref, bound)
    err = float(np.abs(out.astype(F64) - ref)[np.isfinite(out)].max(initial=0.0))
    record_measurement("mel_step_" + what, err=err, bound_max=float(bound.max()), err_over_bound=ratio, elements_beyond=bad, **tags)
    print(f"[{what} {tags}] err {err:.3e}, {ratio:.3f} x bound, {bad} elements beyond")
    assert np.all(out[~valid] == 0.0), f"{what} {tags}: rows >= lens are not exactly 0"
    assert bad == 0, f"{what} {tags}: {bad} elements beyond their bound, the worst {ratio:.3g} x"
    return ratio


# ------------------------------------------------------------------------------------------------
# a. controlled net, single steps, both launch forms
# ------------------------------------------------------------------------------------------------
def _single_steps(model, case, tables, what, ksplit_gt1):
    net = model._pk["mel"]["net"]
    B, T = case["B"], case["T"]
    tape = MR.noise_tape(case)
    assert np.all(tape[0] == 1e30)
    bufs = {}
    assert L.load().ss_get_tuning(b"mel_tail") == 1, "the knob's default"
    for tail in (1, 0):
        with _knob(b"mel_tail", tail):
            _assert_form(net, B, T, tail, ksplit_gt1)
            run = GS._MelRun(net, B=B, T=T, cond=case["cond"], lens=case["lens"], z=tape)
            for step in case["steps"]:
                buf = _fresh(case["x"][step])
                run(buf, step, step + 1, 1)
                out = _take(buf, (B, T, M))
                coef = MR.mel_coef_ddpm(tables, step)
                z = tape[step]
                ref = MR.mel_step(case["x"][step], case["eps"], coef, z, step, lens=case["lens"])
                bound = MR.mel_step_bound(case["x"][step], case["eps"], coef, z, step, case["e_eps"], lens=case["lens"])
                _judge(what, out, ref, bound, case["valid"], case=case["name"], step=step, mel_tail=tail)
                bufs[(tail, step)] = buf
    assert L.load().ss_get_tuning(b"mel_tail") == 1
    return bufs


@pytest.mark.parametrize("name", sorted(MR.CASES))
def test_controlled_net_single_steps_in_both_launch_forms(name):
    """Every case of mel_step_refs.CASES at steps K-1, 1 and 0, each run alone with a recorded tape whose t = 0 slab holds 1e30 (it must
    contribute exactly 0), with mel_tail_kernel (the knob's default; every one of these shapes takes it: asserted) and through the SS_EPI_DDPM
    launch (knob at 0). Every element inside its bound - each clamp regime sits on known elements, among them pre-clamp values within 4e-6 of a
    rail on either side -, padded rows exactly 0, the sentinel behind the buffer intact, and the two forms bit-identical (dyadic weights: the same
    eps in any summation order, then ss_ddpm_update's promise). "slices" and "odd" take the split-K slices form of the skip source, "reduced"
    the reduced tensor (both asserted); in "odd" and "reduced" B*T is odd: the last mel_tail workgroup holds one row."""
    spec = MR.CASES[name]
    tables = _tables()
    case = MR.controlled_mel_case(name, tables)
    if name == "reduced":
        assert _ksplit(case["B"], case["T"]) == 1 and case["B"] * case["T"] <= 2048
    bufs = _single_steps(_controlled_model(), case, tables, "controlled", spec["ksplit_gt1"])
    for step in case["steps"]:
        a, b = bufs[(1, step)], bufs[(0, step)]
        ndiff = int((a != b).sum())
        record_measurement("mel_step_forms", case=name, step=step, elements_differing=ndiff)
        assert torch.equal(a, b), f"{name} step {step}: mel_tail_kernel and the SS_EPI_DDPM launch differ in {ndiff} elements"


def test_controlled_net_with_a_projection_that_rounds():
    """The "odd" shape with fp32-normal weights: eps is a sum that rounds, differently per launch form. Both forms inside the bound (whose eps term
    K 2^-24 sum |g w| now bears load); how many elements differ between them is recorded, not asserted (see the module docstring)."""
    tables = _tables()
    case = MR.controlled_mel_case("odd", tables, wset="random")
    bufs = _single_steps(_controlled_model("random"), case, tables, "controlled_random", True)
    for step in case["steps"]:
        a, b = bufs[(1, step)], bufs[(0, step)]
        record_measurement("mel_step_forms_random", step=step, elements_differing=int((a != b).sum()), max_diff=float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------
# b. the SS_EPI_DDPM epilogue directly, in every tile it is built for
# ------------------------------------------------------------------------------------------------
TILES = {1: (128, "128x128"), 2: (64, "64x128"), 3: (64, "64x64"), 4: (128, "128x64"), 5: (128, "128x32")}    # SS_TILE_* -> (BM, name)


@pytest.mark.parametrize("tile", sorted(TILES))
def test_ddpm_epilogue_update_in_every_tile(tile):
    """ss_conv_gemm(epi = SS_EPI_DDPM) on A = relu(beta) in every row and the packed controlled projection - the same eps as in part a - with the
    tile given explicitly (SS_TILE_AUTO would pick one by block count): T = 2 BM + 13, N = 80, lens on a tile joint, one past one, 1 and T;
    ddpm_x0_pred 0 / 1 and mask_rows on / off, at step K-1's coefficients with a recorded noise. The bound of part a; with the mask off rows >=
    lens are updated too, from the eps their zero A rows give: the bias. C has two spare rows per item and 8 spare columns: rows >= T and columns >= N keep the sentinel."""
    lib = L.load()
    BM, tname = TILES[tile]
    tables = _tables()
    T, N, ldc = 2 * BM + 13, M, M + 8
    lens_h = [2 * BM, BM + 1, 1, T]
    B = len(lens_h)
    case = MR.controlled_mel_case(dict(name="tile_" + tname, B=B, T=T, lens=lens_h, seed=70 + tile), tables, steps=(K - 1,))
    w = case["weights"]
    step = K - 1
    coef = MR.mel_coef_ddpm(tables, step)
    sigma32 = float(np.exp(f32(0.5) * f32(tables["posterior_log_variance_clipped"][step])))    # within an ulp of the sampler's expf: inside sigma_ulps = 2
    A = _d(np.ascontiguousarray(np.broadcast_to(np.maximum(w["beta"], 0), (B, T, C))))
    W = L.pack_conv_weight(_d(w["w_final"]))
    bias = L.pack_bias(_d(w["b_final"]))
    assert tuple(W.shape) == (96, C) and bias.numel() == 96
    lens = _d(np.asarray(lens_h, np.int32))
    z = case["z_of"][step]
    z_d = _d(z)
    rows_alloc = T + 2
    # rows >= lens[b] of A read as 0 whatever mask_rows says (the header's rule): their eps is the bias alone, exactly
    row_ok = case["valid"][..., None]
    net_out = np.where(row_ok, case["eps"], w["b_final"].astype(F64))
    e_net = np.where(row_ok, case["e_eps"], 0.0)
    for x0_pred in (0, 1):
        for mask in (True, False):
            Cbuf = torch.full((B, rows_alloc, ldc), SENT, device=DEV)
            Cbuf[:, :T, :N] = _d(case["x"][step])
            a = L._fill_args(A, W, Cbuf, B=B, T=T, Cin=C, N=N, Np=96, Kp=C, lens=lens, bias=bias, epi=L.EPI_DDPM, mask_rows=mask, ldc=ldc,
                             c_bs=rows_alloc * ldc, tile=tile)
            a.ddpm_recip, a.ddpm_recipm1, a.ddpm_c1, a.ddpm_c2, a.ddpm_sigma = coef["recip"], coef["recipm1"], coef["c1"], coef["c2"], sigma32
            a.ddpm_x0_pred = x0_pred
            L.set_members(a, noise=z_d)
            a.seed, a.step = 5, step
            assert a.tile == tile and a.epi == L.EPI_DDPM      # the tile launched is the one asked for: only SS_TILE_AUTO picks
            L.check(lib.ss_conv_gemm(ctypes.byref(a), L.stream_ptr()), f"ss_conv_gemm DDPM tile {tname}")
            torch.cuda.synchronize()
            assert bool((Cbuf[:, T:] == SENT).all()), f"tile {tname}: rows >= T were written"
            assert bool((Cbuf[:, :, N:] == SENT).all()), f"tile {tname}: columns >= N were written"
            out = Cbuf[:, :T, :N].cpu().numpy()
            lens_ref = lens_h if mask else None
            ref = MR.mel_step(case["x"][step], net_out, coef, z, step, x0_pred=bool(x0_pred), lens=lens_ref)
            bound = MR.mel_step_bound(case["x"][step], net_out, coef, z, step, e_net, x0_pred=bool(x0_pred), lens=lens_ref)
            valid = case["valid"] if mask else np.ones_like(case["valid"])
            _judge("epilogue", out, ref, bound, valid, tile=tname, x0_pred=x0_pred, mask_rows=int(mask))
            if not mask:
                assert np.any(out[~case["valid"]] != 0.0), "mask_rows = 0 still zeroed the rows >= lens"


# ------------------------------------------------------------------------------------------------
# c. ProDiff: x0-prediction with the caller's coefficients
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", [1, K])
def test_prodiff_sample_on_the_controlled_net(n_steps):
    """ss_prodiff_sample with caller-supplied c1 / c2 / sigma on the controlled net: the network output IS x0 and passes through without a clamp
    (|x0| > 1.2 on some bins, < 0.8 on others: asserted by the CPU test). sigma[0] = 0.7 must be ignored, and so must the t = 0 slab of 1e30.
    n_steps = 1 is step 0 alone, n_steps = K the chain K-1 .. 0, each step's bound fed to the next."""
    tables = _tables()
    case = MR.controlled_mel_case("odd", tables)
    assert (np.abs(case["eps"]) > 1.2).any() and (np.abs(case["eps"]) < 0.8).any()
    net = _controlled_model()._pk["mel"]["net"]
    B, T = case["B"], case["T"]
    # the caller's own coefficients, none of them degenerate (the schedule's c1[0] = 1, c2[0] = 0 would make step 0 the identity on x0)
    c1 = np.asarray([0.625, 0.5, 0.40625, 0.3], f32)
    c2 = np.asarray([0.3, 0.4375, 0.55, 0.65625], f32)
    sigma = np.asarray([0.7, 0.2, 0.15, 0.11], f32)
    assert len(c1) == K and sigma[0] != 0
    tape = MR.noise_tape(case)
    x_in = case["x"][K - 1]
    wsb = L.load().ss_wavenet_workspace_bytes(ctypes.addressof(net), B, T)
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    buf = _fresh(x_in)
    cond, lens, tape_d = _d(case["cond"]), _d(case["lens"]), _d(tape)
    L.ops.ss_prodiff_sample(net, buf, cond, lens, B, T, tape_d, 37, None, n_steps, c1, c2, sigma, 1, ws, wsb)
    torch.cuda.synchronize()
    out = _take(buf, (B, T, M))
    steps = [dict(coef=dict(recip=0.0, recipm1=0.0, c1=float(c1[t]), c2=float(c2[t]), sigma=float(sigma[t]) if t > 0 else 0.0), z=tape[t], step=t,
                  x0_pred=True, sigma_ulps=0) for t in reversed(range(n_steps))]
    ref, bound = MR.run_steps(x_in, case["eps"], case["e_eps"], steps, lens=case["lens"])
    _judge("prodiff", out, ref, bound, case["valid"], n_steps=n_steps)
    assert np.abs(ref).max() > 1.2     # values beyond the clamp's rails came through


# ------------------------------------------------------------------------------------------------
# d. DDIM family: coefficients, the last transition, the noise slab
# ------------------------------------------------------------------------------------------------
def _ddim_run(model, case, tables, ac64, ts, eta, tape):
    net = model._pk["mel"]["net"]
    B, T = case["B"], case["T"]
    wsb = L.load().ss_wavenet_workspace_bytes(ctypes.addressof(net), B, T)
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    buf = _fresh(case["x"][ts[0]])
    cond, lens, tape_d = _d(case["cond"]), _d(case["lens"]), _d(tape)
    ts_h = np.ascontiguousarray(np.asarray(ts, np.int32))
    L.ops.ss_meldiff_sample_ddim(net, buf, cond, lens, B, T, ts_h, len(ts), ac64, float(eta), tape_d, 31, None, 1, ws, wsb)
    torch.cuda.synchronize()
    out = _take(buf, (B, T, M))
    steps = []
    for i, t in enumerate(ts):    # the float64 coefficients; their casts to fp32 are one more rounding each (coef_casts)
        c = MR.mel_coef_ddim(tables, ac64, ts, i, eta, cast=None)
        steps.append(dict(coef=c, z=tape[t], step=1 if c["sigma"] != 0.0 else 0, sigma_ulps=0, coef_casts=True))
    ref, bound = MR.run_steps(case["x"][ts[0]], case["eps"], case["e_eps"], steps, lens=case["lens"])
    _judge("ddim", out, ref, bound, case["valid"], ts=list(ts), eta=eta)
    return buf


def test_ddim_transitions_on_the_controlled_net():
    """ss_meldiff_sample_ddim on the controlled net, the coefficients from the float64 statement (Song et al. eq. 12 / 16):
      eta = 0, ts = (2, 0) and (3, 1) - strided, ending at 0 and above it (the last transition goes to ac = 1 either way); the tape is ignored:
               filled with 1e30
      eta = 0.5, ts = (3, 2, 0) - a tape whose slabs differ per network time, and transition i never equals its network time t where a draw is
               used: the slab index is t, not i
      eta = 1, ts = (3, 2, 1, 0) - the ancestral loop's steps with coefficients built another way (float64 from the cumulative products, against the
               fp32 tables and expf there): algebraically ss_meldiff_sample, not bit for bit, and the code does not promise it - held to the bound;
               the elements that differ from ss_meldiff_sample are recorded."""
    tables = _tables()
    model = _controlled_model()
    case = MR.controlled_mel_case("odd", tables, steps=(3, 2, 1, 0))
    ac64 = np.ascontiguousarray(model._pk["mel"]["sched"]["alphas_cumprod_f64"])
    assert np.array_equal(ac64, np.cumprod(1.0 - tables["betas"]))
    hot = np.full((K, case["B"], case["T"], M), 1e30, f32)
    for ts in ((2, 0), (3, 1)):
        _ddim_run(model, case, tables, ac64, ts, 0.0, hot)
    tape = MR.noise_tape(case)
    assert not np.array_equal(tape[3], tape[2]) and not np.array_equal(tape[2], tape[1])
    _ddim_run(model, case, tables, ac64, (3, 2, 0), 0.5, tape)
    full = _ddim_run(model, case, tables, ac64, (3, 2, 1, 0), 1.0, tape)
    with _knob(b"mel_tail", 0):
        run = GS._MelRun(model._pk["mel"]["net"], B=case["B"], T=case["T"], cond=case["cond"], lens=case["lens"], z=tape)
        buf = _fresh(case["x"][3])
        run(buf, 0, K, 1)
    record_measurement("mel_step_ddim_eta1_vs_ddpm", elements_differing=int((buf != full).sum()), max_diff=float((buf - full).abs().max()))


# ------------------------------------------------------------------------------------------------
# e. schedule extremes
# ------------------------------------------------------------------------------------------------
def test_extreme_schedule_single_steps():
    """The 1000-step schedule: steps t = 999 (sqrt(1 / ac - 1) ~ 3e6: one fp32 step of x moves the pre-clamp x0 by a good part of the rails'
    distance, the clamp decides nearly every element) and t = 1, each alone at B = 2, T = 33, in both launch forms. The bound scales with the
    coefficients and is asserted per element."""
    model, tables = _extreme()
    assert model._pk["mel"]["net"].steps == 1000 and MR.mel_coef_ddpm(tables, 999)["recipm1"] > 1e6
    case = MR.controlled_mel_case(dict(MR.EXTREME, name="extreme"), tables, steps=(999, 1))
    bufs = _single_steps(model, case, tables, "extreme", None)
    for step in case["steps"]:
        assert torch.equal(bufs[(1, step)], bufs[(0, step)]), f"extreme step {step}: the two launch forms differ"


# ------------------------------------------------------------------------------------------------
# f. real weights against the float64 oracle
# ------------------------------------------------------------------------------------------------
def _real_inputs():
    """ragged lens (T, T // 2, 1, T - 13) and one more item (T - 1) so that B*T is odd (four items give an even count whatever T is)"""
    r = np.random.default_rng(83)
    B, T = 5, 45
    lens = np.asarray([T, T // 2, 1, T - 13, T - 1], np.int32)
    assert (B * T) % 2 == 1
    valid = np.arange(T)[None, :] < lens[:, None]
    x = r.standard_normal((B, T, M)).astype(f32)
    x[~valid] = 0.0
    smin, smax = np.asarray(GS._hp()["spec_min"], f32)[:M], np.asarray(GS._hp()["spec_max"], f32)[:M]
    coarse = (smin + (smax - smin) * r.uniform(0.05, 0.95, (B, T, M))).astype(f32)
    return dict(B=B, T=T, lens=lens, valid=valid, x=x, coarse=coarse, smin=smin, smax=smax, cond=(r.standard_normal((B, T, 256)) * 0.5).astype(f32),
                z=r.standard_normal((K, B, T, M)).astype(f32), zq=r.standard_normal((B, T, M)).astype(f32))


def _sd_pair():
    sd32 = GS._base_sd()
    if "sd64" not in _cache:
        _cache["sd64"] = {k: (v.double() if v.is_floating_point() else v) for k, v in sd32.items()}
    return sd32, _cache["sd64"]


@contextlib.contextmanager
def _default_dtype(tt):
    torch.set_default_dtype(tt)
    try:
        with torch.no_grad():
            yield
    finally:
        torch.set_default_dtype(torch.float32)


def _oracle_step(sd, inp, x_in, step, tt):
    """oracle.diffnet per item on its valid frames (the kernels mask rows >= lens, which is the network on the shorter sequence), then the step
    statement in the same precision"""
    B, T = inp["B"], inp["T"]
    np_dt = F64 if tt == torch.float64 else f32
    eps = np.zeros((B, T, M), np_dt)
    with _default_dtype(tt):
        for b in range(B):
            n = int(inp["lens"][b])
            o = R.diffnet(sd, GS._hp(), torch.from_numpy(x_in[b:b + 1, :n]).to(tt), torch.full((1,), step, dtype=torch.long),
                          torch.from_numpy(inp["cond"][b:b + 1, :n]).to(tt))
            eps[b, :n] = o[0].numpy()
    return MR.mel_step(x_in, eps, MR.mel_coef_ddpm(_tables(), step), inp["z"][step], step, lens=inp["lens"], dtype=np_dt).astype(F64)


def _four_x(what, out, ref64, ref32, valid, **tags):
    """4 x the fp32-CPU oracle's own error against float64, never less than 2 ulp of the largest value (the rule of _check_real_step)"""
    cpu_err = float(np.abs(ref32 - ref64).max())
    bound = max(4.0 * cpu_err, 2.0 * float(np.spacing(f32(np.abs(ref64).max()))))
    err = float(np.abs(out.astype(F64) - ref64).max()) if np.isfinite(out).all() else float("inf")
    ratio = err / cpu_err if cpu_err > 0 else float("inf")
    record_measurement("mel_step_real_" + what, kernel_err=err, cpu_fp32_err=cpu_err, bound=bound, gpu_over_cpu_fp32=ratio, **tags)
    print(f"[real {what} {tags}] kernel {err:.3e}, cpu-fp32 {cpu_err:.3e} ({ratio:.2f} x), bound {bound:.3e}")
    assert np.all(out[~valid] == 0.0), f"{what}: rows >= lens are not exactly 0"
    assert err <= bound, (what, tags, err, cpu_err, bound)


def test_real_weights_two_steps_and_the_x_handover():
    """Unmodified synthetic weights, ragged lens, B*T odd, mel_tail_kernel (asserted). Step K-1 is a call of its own. Step K-2 is judged on the ONE
    call [K-2, K), whose second evaluation reads the X row mel_tail_kernel wrote - the only check of its input-projection half against a
    reference; its reference starts from the device's own state after step K-1 (the first evaluation of either call is the same launches).
    Measured on an MI355X: kernel 2.25e-7 / 1.50e-7 against the CPU's 2.25e-7 / 1.78e-7 (1.00 x / 0.84 x), a quarter of the bound."""
    sd32, sd64 = _sd_pair()
    model = GS._model("real", sd32)
    net = model._pk["mel"]["net"]
    inp = _real_inputs()
    B, T = inp["B"], inp["T"]
    _assert_form(net, B, T, True)
    run = GS._MelRun(net, B=B, T=T, cond=inp["cond"], lens=inp["lens"], z=inp["z"])
    buf = _fresh(inp["x"])
    run(buf, K - 1, K, 1)
    x1 = _take(buf, (B, T, M))
    _four_x("first", x1, _oracle_step(sd64, inp, inp["x"], K - 1, torch.float64), _oracle_step(sd32, inp, inp["x"], K - 1, torch.float32), inp["valid"], step=K - 1)
    buf = _fresh(inp["x"])
    run(buf, K - 2, K, 1)
    x2 = _take(buf, (B, T, M))
    _four_x("handover", x2, _oracle_step(sd64, inp, x1, K - 2, torch.float64), _oracle_step(sd32, inp, x1, K - 2, torch.float32), inp["valid"], step=K - 2)
    assert np.abs(x2 - x1)[inp["valid"]].max() > 1e-2


class _OneDraw:
    """a tape that hands the oracle one recorded q-sample noise [1, T, M] in the reference's layout"""

    def __init__(self, z, tt):
        self.z = torch.from_numpy(np.ascontiguousarray(z)).to(tt).transpose(1, 2)[:, None]

    def randn(self, *shape):
        assert tuple(shape) == tuple(self.z.shape), (shape, self.z.shape)
        return self.z


def _oracle_plms(sd, hp, inp, interval, tt):
    B, T = inp["B"], inp["T"]
    out = np.zeros((B, T, M), F64)
    with _default_dtype(tt):
        for b in range(B):
            n = int(inp["lens"][b])
            o = R.mel_plms(sd, hp, torch.from_numpy(inp["coarse"][b:b + 1, :n]).to(tt), torch.from_numpy(inp["cond"][b:b + 1, :n]).to(tt),
                           _OneDraw(inp["zq"][b:b + 1, :n], tt), interval)
            out[b, :n] = o[0].double().numpy()
    return out


def _real_model(k_step):
    """(model, hp, fp32 state dict, float64 state dict) of the unmodified synthetic weights at timesteps = K_step = k_step"""
    if k_step == K:
        return (GS._model("real", GS._base_sd()), GS._hp()) + _sd_pair()
    key = ("real", k_step)
    if key not in _cache:
        hp = config.make_hparams(dict(timesteps=k_step, K_step=k_step, f0_timesteps=GS.S))
        sd = synth.synth_acoustic_state_dict(hp, 77)
        m = StyleSingerHIP(None, hparams=hp)
        m.load_state_dict(sd)
        m.eval().to(DEV)
        m._ensure_packed()
        _cache[key] = (m, hp, sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
    return _cache[key]


@pytest.mark.parametrize("k_step,interval", [(K, 1), (K, 2), (MR.K_PLMS, 1)])
def test_real_weights_plms_against_the_oracle(k_step, interval):
    """ss_mel_qsample -> ss_meldiff_sample_plms(step_hi = K_step) -> ss_mel_denorm against oracle.mel_plms in float64, per item on its valid
    frames. At K_step = 4, interval = 1 walks the double evaluation, then two and three history entries, interval = 2 the double evaluation
    alone: the last call of either run is the one at t = 0, whose previous time is 0 too (a_prev = a_t: the identity, whatever eps' is). The
    call with four history entries first moves x at K_step = 5 (t = 1): the third run.
    On the controlled net every history entry is the same eps and every multistep order collapses to it, so the history ring - which slot holds
    which evaluation - is only visible with real weights: this is its test.
    Measured on an MI355X: kernel 1.27e-6 / 1.03e-6 / 1.27e-6 against the CPU's 1.44e-6 / 1.09e-6 / 1.30e-6 (0.88 x / 0.95 x / 0.97 x)."""
    model, hp, sd32, sd64 = _real_model(k_step)
    net = model._pk["mel"]["net"]
    assert net.steps == k_step
    inp = _real_inputs()
    B, T = inp["B"], inp["T"]
    tables = _tables(sd32)
    n = B * T * M
    smin, smax, lens = _d(inp["smin"]), _d(inp["smax"]), _d(inp["lens"])
    coarse, zq, cond = _d(inp["coarse"]), _d(inp["zq"]), _d(inp["cond"])
    x = torch.full((n + TAIL,), SENT, device=DEV)
    L.ops.ss_mel_qsample(coarse, smin, smax, float(tables["sqrt_alphas_cumprod"][k_step - 1]), float(tables["sqrt_one_minus_alphas_cumprod"][k_step - 1]),
                         zq, 0, None, x, B, T, M)
    hist = torch.full((6 * n + TAIL,), SENT, device=DEV)
    wsb = L.load().ss_wavenet_workspace_bytes(ctypes.addressof(net), B, T)
    ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
    ac = np.ascontiguousarray(model._pk["mel"]["sched"]["alphas_cumprod_np"])
    assert ac.dtype == f32 and np.array_equal(ac.astype(F64), tables["alphas_cumprod"])
    L.ops.ss_meldiff_sample_plms(net, x, cond, lens, B, T, k_step, interval, ac, 1, hist, ws, wsb)
    mel = torch.full((n + TAIL,), SENT, device=DEV)
    L.ops.ss_mel_denorm(x, smin, smax, mel, B, T, M, lens, None)
    torch.cuda.synchronize()
    assert bool((x[n:] == SENT).all()) and bool((hist[6 * n:] == SENT).all())
    out = _take(mel, (B, T, M))
    _four_x("plms", out, _oracle_plms(sd64, hp, inp, interval, torch.float64), _oracle_plms(sd32, hp, inp, interval, torch.float32), inp["valid"],
            k_step=k_step, interval=interval)


# ------------------------------------------------------------------------------------------------
# g. ss_mel_denorm's nonfinite flag
# ------------------------------------------------------------------------------------------------
def test_mel_denorm_nonfinite_flag():
    """The flag is OR-ed with 1 when a valid frame holds inf or NaN, is not touched when only rows >= lens[b] do - those still come out as 0 -
    and is not touched when everything is finite (a word of 4 stays 4)."""
    hp = GS._hp()
    B, T = 3, 37
    lens_h = [37, 20, 1]
    r = np.random.default_rng(91)
    smin, smax = _d(np.asarray(hp["spec_min"], f32)[:M]), _d(np.asarray(hp["spec_max"], f32)[:M])
    lens = _d(np.asarray(lens_h, np.int32))
    valid = np.arange(T)[None, :] < np.asarray(lens_h)[:, None]
    base = r.uniform(-1, 1, (B, T, M)).astype(f32)
    ref, _ = SR.mel_denorm(base, np.asarray(hp["spec_min"], f32)[:M], np.asarray(hp["spec_max"], f32)[:M], lens=lens_h)

    def run(x_h):
        flag = torch.full((1 + 3,), 4, device=DEV, dtype=torch.int32)
        out = torch.full((x_h.size + TAIL,), SENT, device=DEV)
        x_d = _d(x_h)
        L.ops.ss_mel_denorm(x_d, smin, smax, out, B, T, M, lens, flag)
        torch.cuda.synchronize()
        assert bool((flag[1:] == 4).all())
        return int(flag[0].item()), _take(out, (B, T, M))

    flag, out = run(base)
    assert flag == 4, "all finite: the flag was touched"
    assert np.all(out[~valid] == 0) and np.abs(out[valid] - ref[valid]).max() < 1e-5
    for bad in (np.inf, -np.inf, np.nan):
        x = base.copy()
        x[1, 19, 7] = bad         # the last valid frame of item 1
        flag, out = run(x)
        assert flag == 5, f"{bad} on a valid frame: flag {flag}"
        assert np.all(out[~valid] == 0)
        x = base.copy()
        x[1, 20, 7] = bad         # the first padded frame of item 1
        x[2, 1:, :] = bad         # every padded frame of item 2
        flag, out = run(x)
        assert flag == 4, f"{bad} on padded frames only: flag {flag}"
        assert np.all(out[~valid] == 0), "padded rows holding non-finite values do not come out as 0"
        assert np.array_equal(out[valid], run(base)[1][valid])
