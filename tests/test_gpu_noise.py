"""The production noise path: every kernel that draws from SsPhilox (csrc/common.h) against the host restatement oracle/philox.py, which
tests/test_noise_cpu.py pins to the Random123 known answers. Every real run draws on the device; every other parity test injects a tape.

Tolerances. Integer-derived values (masks, sentinels, padding / tile / launch-form invariance) are compared with torch.equal. A device normal is
sqrtf(-2 logf(u1)) {cos, sin}f(fl(2 pi) u2) in fp32 and the host value is float64 from the same exact uniforms: per element
|z_dev - z_host| <= (r + 1) 2^-21 with r = the draw's Box-Muller radius (philox.normal_bound: angle error r * 4.2e-7, plus a few ulp of logf /
sincosf / the product). Recurrences propagate that bound through the float64 recurrence. The whole path keeps the project's bars.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_measurement  # noqa: E402
from oracle import philox as P  # noqa: E402
from oracle import restatement as R  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402
from stylesinger_amd.vocoder import HifiGAN  # noqa: E402

MEL_L1_TOL = 1e-5   # the project's bars (tests/test_gpu_parity.py)
WAV_TOL = 1e-5
DEV = "cuda:0"
SENT = 7.25         # sentinel: not a value any draw produces exactly by accident in these buffers


def _ratio(dev, host, r, what):
    """assert the per-element bound and return the largest observed |dev - host| / bound"""
    d = np.abs(dev.detach().cpu().double().numpy() - host)
    ratio = d / P.normal_bound(r)
    worst = float(ratio.max())
    assert worst <= 1.0, f"{what}: |z_dev - z_host| is {worst:.2f} x its bound at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    return worst


def _seed_word(v):
    return torch.tensor([v], device=DEV, dtype=torch.int64)


def test_fill_normal_matches_the_restatement():
    """n not a multiple of 4, a counter offset that carries from the low into the high word inside the buffer, a seed with a high word, and the
    device seed word absent / present (its addition carries into the key's high word)."""
    lib = L.load()
    n = 4099
    offset = (3 << 32) + 0xFFFFFF00          # block 256 of the 1025 crosses 2^32
    worst = 0.0
    for seed, seed_dev in ((0x9ABCDEF112345678, None), (0x9ABCDEF1FFFFFFF0, 0x25), (5, 0)):
        x = torch.full((n + 9,), SENT, device=DEV)
        sd = None if seed_dev is None else _seed_word(seed_dev)
        L.check(lib.ss_fill_normal(L.ptr(x), n, seed, L.ptr(sd), offset, L.stream_ptr()), "ss_fill_normal")
        z, r = P.fill_normal(n, P.make_key(0, seed, seed_dev or 0), offset, want_radius=True)
        worst = max(worst, _ratio(x[:n], z, r, f"ss_fill_normal seed={seed:#x}"))
        assert bool((x[n:] == SENT).all()), "ss_fill_normal wrote behind n"
    record_measurement("noise_fill_normal", max_err_over_bound=worst, n=n)


def test_fill_normal_rows_matches_and_does_not_depend_on_T():
    lib = L.load()
    B, seed, seed_dev = 3, (7 << 32) | 11, 1234
    sd = _seed_word(seed_dev)
    key = P.make_key(0, seed, seed_dev)
    outs, worst = {}, 0.0
    for T in (1, 5, 750, 1501):
        ld = T + 3
        x = torch.full((B, ld), SENT, device=DEV)
        L.check(lib.ss_fill_normal_rows(L.ptr(x), B, T, ld, seed, L.ptr(sd), L.stream_ptr()), "ss_fill_normal_rows")
        z, r = P.fill_normal_rows(B, T, key, want_radius=True)
        worst = max(worst, _ratio(x[:, :T], z, r, f"ss_fill_normal_rows T={T}"))
        assert bool((x[:, T:] == SENT).all()), f"T={T}: columns behind T were written"
        outs[T] = x[:, :T].clone()
    for Ts, Tl in ((1, 5), (5, 750), (750, 1501), (1, 1501)):
        assert torch.equal(outs[Ts], outs[Tl][:, :Ts]), f"the first {Ts} columns depend on T ({Tl})"
    x = torch.empty(B, 8, device=DEV)      # no device word: the host seed alone
    L.check(lib.ss_fill_normal_rows(L.ptr(x), B, 8, 8, seed, None, L.stream_ptr()), "ss_fill_normal_rows")
    z, r = P.fill_normal_rows(B, 8, seed, want_radius=True)
    worst = max(worst, _ratio(x, z, r, "ss_fill_normal_rows, no device word"))
    record_measurement("noise_fill_normal_rows", max_err_over_bound=worst)


def test_mel_qsample_draw_matches_the_restatement():
    """sqrt_ac = 0, sqrt_1mac = 1: x = 0 * xs + 1 * z = z."""
    lib = L.load()
    B, T, M, seed, seed_dev = 3, 37, 80, 23 + (1 << 40), 99
    mel = torch.rand(B, T, M, device=DEV) * -5.0
    smin, smax = torch.full((M,), -6.0, device=DEV), torch.zeros(M, device=DEV)
    x = torch.full((B * T * M + 5,), SENT, device=DEV)
    L.check(lib.ss_mel_qsample(L.ptr(mel), L.ptr(smin), L.ptr(smax), 0.0, 1.0, None, seed, L.ptr(_seed_word(seed_dev)), L.ptr(x), B, T, M, L.stream_ptr()), "qsample")
    z, r = P.mel_qsample_noise(B, T, M, P.make_key(0, seed, seed_dev), want_radius=True)
    worst = _ratio(x[:B * T * M].view(B, T, M), z, r, "ss_mel_qsample")
    assert bool((x[B * T * M:] == SENT).all())
    record_measurement("noise_mel_qsample", max_err_over_bound=worst)


TILES = {"auto": 0, "128x128": 1, "64x128": 2, "64x64": 3, "128x64": 4, "128x32": 5}    # SS_TILE_* of include/stylesinger_hip.h


def _ddpm_draw(B, T, lens, step, seed, sd, tile, sigma=1.0, rows_alloc=None):
    """SS_EPI_DDPM with zero weights and coefficients: eps = 0, x0 = 0, mean = 0, C = sigma * z (0 on masked rows). C has `rows_alloc` rows per
    item (>= T): the rows behind T keep the sentinel."""
    N, Cin = 80, 32
    rows_alloc = rows_alloc or T + 2
    A = torch.zeros(B, T, Cin, device=DEV)
    W = torch.zeros(96, 32, device=DEV)
    bias = torch.zeros(96, device=DEV)
    C = torch.full((B, rows_alloc, N), SENT, device=DEV)
    C[:, :T] = 0.5
    a = L._fill_args(A, W, C, B=B, T=T, Cin=Cin, N=N, Np=96, Kp=32, lens=lens, bias=bias, epi=L.EPI_DDPM, mask_rows=True, ldc=N, c_bs=rows_alloc * N, tile=tile)
    a.ddpm_recip = a.ddpm_recipm1 = a.ddpm_c1 = a.ddpm_c2 = 0.0
    a.ddpm_sigma = sigma
    a.noise = None
    a.seed = seed
    a.seed_dev = L.ptr(sd)
    a.step = step
    L.check(L.load().ss_conv_gemm(ctypes.byref(a), L.stream_ptr()), f"ss_conv_gemm DDPM tile {tile}")
    return C


@pytest.mark.parametrize("T", [5, 97, 333, 1500])
def test_ddpm_epilogue_draw_in_every_tile(T):
    """The four-frames-per-block draw of the SS_EPI_DDPM epilogue (ss_mel_draw4) in EVERY tile shape the epilogue is built for - SS_TILE_AUTO gives
    the same N = 80 projection 64x64, 64x128, 128x128 or 128x32 by block count, so the big launches never see the small ones' tiles - at several
    steps, with ragged lengths and the device seed word: C == z against the restatement, the same bits in every tile, and the same bits when
    the frame axis is padded."""
    B, seed, seed_dev = 3, 29 + (5 << 32), 1234
    sd = _seed_word(seed_dev)
    key = P.make_key(0, seed, seed_dev)
    lens_h = [T, max(1, T - 3), max(1, (T * 2) // 5)]
    lens = torch.tensor(lens_h, device=DEV, dtype=torch.int32)
    valid = (torch.arange(T, device=DEV)[None, :] < lens[:, None])[..., None]
    worst = 0.0
    for step in (0, 7, 99, 999):
        z, r = P.mel_step_noise(B, T, 80, step, key, want_radius=True)
        outs = {}
        for name, tile in TILES.items():
            C = _ddpm_draw(B, T, lens, step, seed, sd, tile)
            assert bool((C[:, T:] == SENT).all()), f"tile {name}: rows behind T were written"
            assert bool((C[:, :T][~valid.expand(-1, -1, 80)] == 0).all()), f"tile {name}: masked rows are not zero"
            outs[name] = C[:, :T].clone()
            if step in (7, 999) or name == "auto":
                m = valid.expand(-1, -1, 80).cpu().numpy()
                worst = max(worst, _ratio(C[:, :T][valid.expand(-1, -1, 80)], z[m], r[m], f"DDPM epilogue T={T} step={step} tile {name}"))
        for name in TILES:
            assert torch.equal(outs[name], outs["auto"]), f"T={T} step={step}: tile {name} draws other bits than the auto tile"
        padded = _ddpm_draw(B, T + 27, lens, step, seed, sd, 0)
        assert torch.equal(padded[:, :T], outs["auto"]), f"T={T} step={step}: the draw depends on the padded frame count"
    no_sd = _ddpm_draw(B, T, lens, 7, seed, None, 0)
    z, r = P.mel_step_noise(B, T, 80, 7, seed, want_radius=True)
    m = valid.expand(-1, -1, 80).cpu().numpy()
    worst = max(worst, _ratio(no_sd[:, :T][valid.expand(-1, -1, 80)], z[m], r[m], "DDPM epilogue without the device word"))
    mean_only = _ddpm_draw(B, T, lens, 7, seed, sd, 0, sigma=0.0)
    assert bool((mean_only[:, :T] == 0).all()), "sigma = 0 must leave C at the mean"
    record_measurement("noise_mel_step_epilogue", T=T, max_err_over_bound=worst, tiles=len(TILES))


# ------------------------------------------------------------------------------------------------
# the samplers' bookkeeping: zero-eps recurrences through StyleSingerHIP.mel_stage
# ------------------------------------------------------------------------------------------------
def _model(hp, sd, **attrs):
    m = StyleSingerHIP(None, hparams=hp)
    m.load_state_dict(sd)
    m.eval().to(DEV)
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


K_MEL = 16


def _zero_eps_model(**attrs):
    """real-shaped synthetic weights with the mel denoiser's final projection zeroed: eps = 0 exactly, whatever the stack computes"""
    hp = config.make_hparams(dict(timesteps=K_MEL, K_step=K_MEL, f0_timesteps=2))
    sd = synth.synth_acoustic_state_dict(hp, 81)
    for k in ("postdiff.denoise_fn.output_projection.weight", "postdiff.denoise_fn.output_projection.bias"):
        sd[k] = torch.zeros_like(sd[k])
    return hp, sd, _model(hp, sd, **attrs)


def _f64(sd, name):
    return sd[f"postdiff.{name}"].double().numpy()      # the fp32 tables the kernels read, widened


def _recurrence(x, steps):
    """x <- c1 clamp(recip x, -1, 1) + c2 x + sigma z in float64 over `steps` = [(recip, c1, c2, sigma, z, r)], and the bound on the fp32 device
    result: the error e of x passes through the update's derivative (c2, plus c1 recip where the clamp is - or within e may be - inactive),
    every draw adds sigma * normal_bound(r) (+ 2 ulp of sigma = expf(.) on |sigma z|), every fp32 update at most one rounding per product
    and sum: 2^-23 (|c1 x0| + |c2 x| + |sigma z| + |x_new|)."""
    e = 2.0 ** -22 * (np.abs(x) + 1.0)         # the q-sample: the normalisation and two products in fp32
    for recip, c1, c2, sigma, z, r in steps:
        y = recip * x
        x0 = np.clip(y, -1.0, 1.0)
        free = np.abs(y) <= 1.0 + recip * e
        xn = c1 * x0 + c2 * x + (sigma * z if sigma != 0.0 else 0.0)
        e = (abs(c2) + np.where(free, abs(c1) * recip, 0.0)) * e + 2.0 ** -23 * (np.abs(c1 * x0) + np.abs(c2 * x) + np.abs(xn))
        if sigma != 0.0:
            e = e + sigma * P.normal_bound(r) + 2.0 ** -21 * np.abs(sigma * z)
        x = xn
    return x, e


def _mel_stage_reference(sd, coarse, lens_h, seed, bounds, sampler, ts=None):
    B, T, M = coarse.shape
    smin, smax = _f64(sd, "spec_min")[0, 0], _f64(sd, "spec_max")[0, 0]
    K = K_MEL
    c = coarse.double().numpy()
    xs = (c - smin) / (smax - smin) * 2.0 - 1.0
    x = _f64(sd, "sqrt_alphas_cumprod")[K - 1] * xs + _f64(sd, "sqrt_one_minus_alphas_cumprod")[K - 1] * P.mel_qsample_noise(B, T, M, P.make_key(P.KEY_MEL_Q, seed))
    recip = _f64(sd, "sqrt_recip_alphas_cumprod")
    out_x, out_e = np.zeros_like(x), np.zeros_like(x)
    if sampler == "ddpm":
        c1, c2, lv = _f64(sd, "posterior_mean_coef1"), _f64(sd, "posterior_mean_coef2"), _f64(sd, "posterior_log_variance_clipped")
        for i in range(len(bounds) - 1):
            b0, nb = bounds[i], bounds[i + 1] - bounds[i]
            steps = []
            for t in reversed(range(K)):
                z, r = P.mel_step_noise(nb, T, M, t, P.make_key(P.key_mel_steps(b0), seed), want_radius=True)
                steps.append((recip[t], c1[t], c2[t], float(np.exp(0.5 * lv[t])) if t > 0 else 0.0, z, r))
            out_x[b0:b0 + nb], out_e[b0:b0 + nb] = _recurrence(x[b0:b0 + nb], steps)
    else:   # ddim, eta = 1: the coefficients as ss_meldiff_sample_ddim computes them (double, then cast to float), the draw of network time t
        ac = np.cumprod(1.0 - _f64(sd, "betas"))       # as the model rebuilds the table in float64 from the fp32 betas buffer
        steps = []
        for i, t in enumerate(ts):
            ac_t, ac_p = ac[t], (ac[ts[i + 1]] if i + 1 < len(ts) else 1.0)
            sig = np.sqrt((1.0 - ac_p) / (1.0 - ac_t)) * np.sqrt(max(0.0, 1.0 - ac_t / ac_p))
            c2 = np.sqrt(max(0.0, 1.0 - ac_p - sig * sig) / (1.0 - ac_t))
            c1 = np.sqrt(ac_p) - c2 * np.sqrt(ac_t)
            z, r = P.mel_step_noise(B, T, M, t, P.make_key(P.KEY_MEL_ALT, seed), want_radius=True)
            steps.append((recip[t], float(np.float32(c1)), float(np.float32(c2)), float(np.float32(sig)), z, r))
        out_x, out_e = _recurrence(x, steps)
    for b, n in enumerate(lens_h):
        out_x[b, n:] = 0.0
    return out_x, out_e


def _run_mel_stage(model, coarse, cond, lens_h, seed, **kw):
    B, T, _ = coarse.shape
    lens = torch.tensor(lens_h, device=DEV, dtype=torch.int32)
    model.mel_stage(coarse.to(DEV), cond.to(DEV), lens, seed=seed, **kw)
    pl = model._plan(B, T, torch.device(DEV))
    torch.cuda.synchronize()
    return pl.xm.clone(), list(pl.bounds)


def _check_recurrence(x_dev, ref, err, lens_h, what):
    d = np.abs(x_dev.cpu().double().numpy() - ref)
    worst = 0.0
    for b, n in enumerate(lens_h):
        assert float(d[b, n:].max(initial=0.0)) == 0.0, f"{what}: masked frames of item {b} are not zero"
        worst = max(worst, float((d[b, :n] / err[b, :n]).max()))
    assert worst <= 1.0, f"{what}: |x_dev - x_host| is {worst:.2f} x the propagated bound"
    return worst


def _stage_inputs(B, T, gen_seed):
    g = torch.Generator(device="cpu").manual_seed(gen_seed)
    coarse = (torch.randn(B, T, 80, generator=g) * 0.8 - 3.0).clamp(-6.0, 0.0)
    cond = torch.randn(B, T, 256, generator=g) * 0.5
    return coarse, cond


def test_mel_tail_kernel_and_epilogue_draw_the_same_noise_at_the_latency_shape():
    """B = 1, T = 333 takes mel_tail_kernel (knob mel_tail = 1) or the matrix-core epilogue (0). With the final projection zeroed both forms see
    eps = 0 exactly and run x <- c1 clamp(recip x) + c2 x + sigma_t z_t on the same draws: bit-equal to each other, and inside the propagated bound
    of the float64 recurrence driven by the host draws (step = network time t, key 29, q-sample key 23).

    Before both forms shared `ss_ddpm_update` (csrc/common.h) this failed: inside the bound (0.224 x / 0.228 x after 16 steps) but 17 259 of
    26 640 elements differed, by up to 4.77e-7 - the compiler had fused the multiply-adds of c1 x0 + c2 x + sigma z differently in the two
    translation units. The shared update spells out the roundings the epilogue has always had."""
    hp, sd, model = _zero_eps_model()
    lib = L.load()
    B, T, seed = 1, 333, 4242
    coarse, cond = _stage_inputs(B, T, 1)
    before = lib.ss_get_tuning(b"mel_tail")
    assert before == 1
    try:
        x_tail, bounds = _run_mel_stage(model, coarse, cond, [T], seed)
        L.check(lib.ss_set_tuning(b"mel_tail", 0), "mel_tail")
        x_epi, _ = _run_mel_stage(model, coarse, cond, [T], seed)
    finally:
        L.check(lib.ss_set_tuning(b"mel_tail", before), "mel_tail")
    ref, err = _mel_stage_reference(sd, coarse, [T], seed, bounds, "ddpm")
    w_tail = _check_recurrence(x_tail, ref, err, [T], "mel_tail_kernel")
    w_epi = _check_recurrence(x_epi, ref, err, [T], "SS_EPI_DDPM at B = 1")
    ndiff, dmax = int((x_tail != x_epi).sum()), float((x_tail - x_epi).abs().max())
    print(f"zero-eps ddpm, B=1 T=333: tail kernel {w_tail:.3f} x bound, epilogue {w_epi:.3f} x bound; {ndiff} elements differ between the forms, max {dmax:.3e}")
    record_measurement("noise_mel_stage_b1_t333", tail_over_bound=w_tail, epilogue_over_bound=w_epi, elements_differing=ndiff, max_diff=dmax, steps=K_MEL)
    other = _run_mel_stage(model, coarse, cond, [T], seed + 1)[0]
    assert float((other - x_tail).abs().max()) > 0.1
    assert torch.equal(x_tail, x_epi), f"{ndiff} elements differ between mel_tail_kernel and the epilogue it replaces (max {dmax:.3e})"


@pytest.mark.parametrize("B,T,streams", [(4, 1500, 2), (3, 97, 2)])
def test_ddpm_sampler_draws_per_step_item_and_batch_half(B, T, streams):
    """The matrix-core epilogue inside the sampler loop, the batch split over two streams (keys 29 + 7919 b0, the item index restarting at 0 in
    every half; B = 3 splits unevenly), ragged lengths."""
    hp, sd, model = _zero_eps_model(n_streams=streams)
    seed = 777
    coarse, cond = _stage_inputs(B, T, 2)
    lens_h = [T - 17 * b for b in range(B)]
    x, bounds = _run_mel_stage(model, coarse, cond, lens_h, seed)
    assert len(bounds) == 3 and 0 < bounds[1] < B, bounds
    ref, err = _mel_stage_reference(sd, coarse, lens_h, seed, bounds, "ddpm")
    worst = _check_recurrence(x, ref, err, lens_h, f"ddpm B={B} T={T}")
    record_measurement(f"noise_mel_stage_ddpm_b{B}_t{T}", over_bound=worst, halves=bounds, steps=K_MEL)
    # teeth: the same run against a restatement that puts both halves on the first half's key must be far outside
    wrong, _ = _mel_stage_reference(sd, coarse, lens_h, seed, [0, B], "ddpm")
    assert np.abs(wrong[bounds[1]:] - x[bounds[1]:].cpu().numpy()).max() > 0.1


@pytest.mark.parametrize("n_steps", [K_MEL, 6])
def test_ddim_eta1_draws_at_the_network_time(n_steps):
    """ddim with eta = 1 at stride 1 and at a stride > 1 (key 31): every update draws with step = its NETWORK time ts[i], not the loop index."""
    hp, sd, model = _zero_eps_model()
    B, T, seed = 2, 97, 31337
    coarse, cond = _stage_inputs(B, T, 3)
    lens_h = [T, T - 30]
    ts = model.ddim_timesteps(n_steps)
    assert len(ts) == n_steps and ts[0] == K_MEL - 1 and ts[-1] == 0
    x, bounds = _run_mel_stage(model, coarse, cond, lens_h, seed, sampler="ddim", ddim_steps=n_steps, eta=1.0)
    ref, err = _mel_stage_reference(sd, coarse, lens_h, seed, bounds, "ddim", ts=ts)
    worst = _check_recurrence(x, ref, err, lens_h, f"ddim eta=1, {n_steps} of {K_MEL} steps")
    record_measurement(f"noise_mel_stage_ddim_{n_steps}of{K_MEL}", over_bound=worst)


# ------------------------------------------------------------------------------------------------
# vocoder source
# ------------------------------------------------------------------------------------------------
def _vocoder():
    cfg = config.make_vocoder_config()
    vsd = synth.synth_vocoder_state_dict(cfg, 91)
    return HifiGAN(cfg, vsd, device=DEV), vsd


def test_hifigan_source_philox_equals_its_restatement_as_a_tape():
    """rand_ini = sine_noise = NULL (device Philox, key = seed) against the same call fed the restated draws as tapes: the initial phases are exact
    fp32 numbers (the sine part is the same arithmetic in both runs), the additive noise differs by amp * (z_dev - z_host), amp <= 0.1 / 3."""
    voc, vsd = _vocoder()
    B, T, seed = 2, 40, 2024
    Ls = T * 256
    f0 = torch.full((B, T), 220.0)
    f0[1] = 140.0 + 3.0 * torch.arange(T)
    f0[1, 9:23] = 0.0                          # partly unvoiced
    mel = (torch.randn(B, T, 80, generator=torch.Generator().manual_seed(4)) * 0.8 - 3.0).clamp(-6.0, 1.5)
    wav_p, har_p = voc.model(mel.to(DEV), f0.to(DEV), seed=seed, return_source=True)
    noise = P.vocoder_noise(seed, B, Ls)
    wav_t, har_t = voc.model(mel.to(DEV), f0.to(DEV), noise=noise, return_source=True)
    r = P.sine_noise(B, Ls, seed, want_radius=True)[1]
    lw = vsd["m_source.l_linear.weight"].reshape(-1).double().abs().numpy()
    amp = np.where(np.repeat(f0.numpy(), 256, axis=1) > 0, 0.003, 0.1 / 3.0)[..., None]
    bound = (amp * P.normal_bound(r) * lw).sum(-1) + 2.0 ** -21        # tanh is 1-Lipschitz; a few ulp of the O(1) sum
    ratio = float(((har_p - har_t).abs().cpu().double().numpy() / bound).max())
    e_w = float((wav_p - wav_t).abs().max())
    print(f"harmonic source, Philox vs restated tape: {ratio:.3f} x bound, wav max {e_w:.3e}")
    record_measurement("noise_hifigan_source", har_over_bound=ratio, wav_max=e_w)
    assert ratio <= 1.0 and e_w <= WAV_TOL
    wrong = dict(noise, sine_noise=noise["sine_noise"].roll(1, dims=1))
    assert float((voc.model(mel.to(DEV), f0.to(DEV), noise=wrong, return_source=True)[1] - har_p).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------
# whole path
# ------------------------------------------------------------------------------------------------
WP_SEED, WP_LENS, WP_STEPS = 20260, (198, 150, 97), 20


def whole_path_setup():
    hp = config.make_hparams(dict(timesteps=WP_STEPS, K_step=WP_STEPS, f0_timesteps=WP_STEPS))
    sd = synth.synth_acoustic_state_dict(hp, 85)
    T, Tp, Tr = max(WP_LENS), 9, 60
    items = [synth.synth_utterance(i, n, Tp - i, Tr - 7 * i, hp, 85) for i, n in enumerate(WP_LENS)]
    size = dict(txt_tokens=Tp, note=Tp, note_type=Tp, note_dur=Tp, mel2ph=T, ref_mels=Tr, ref_f0=Tr)

    def pad(t, n):
        out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype)
        out[:t.shape[0]] = t
        return out
    batch = {k: torch.stack([pad(it[k], size.get(k, it[k].shape[0])) for it in items]) for k in items[0]}
    return hp, sd, items, batch


def item_noise(noise, i, Ti):
    return {k: {kk: (vv[:, i:i + 1, ..., :Ti] if kk.startswith(("z_steps", "u_steps")) else vv[i:i + 1, ..., :Ti]) for kk, vv in v.items()} for k, v in noise.items()}


def _fwd(model, b, **kw):
    return model(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"], ref_f0=b["ref_f0"],
                 global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"], **kw)


def _dist(a, b):
    """mel L1 / max over the valid frames, voicing flips, pitch_coarse mismatches between two forward results"""
    l1 = n = 0.0
    mx, flips, coarse = 0.0, 0, 0
    for i, Ti in enumerate(WP_LENS):
        d = (a["mel_out"][i, :Ti] - b["mel_out"][i, :Ti]).abs()
        l1, n, mx = l1 + float(d.sum()), n + d.numel(), max(mx, float(d.max()))
        flips += int((a["uv_a"][i, :Ti] != b["uv_a"][i, :Ti]).sum()) + int((a["uv_b"][i, :Ti] != b["uv_b"][i, :Ti]).sum())
        coarse += int((a["pitch_coarse"][i, :Ti] != b["pitch_coarse"][i, :Ti]).sum())
    return dict(mel_l1=l1 / n, mel_max=mx, flips=flips, coarse=coarse)


def test_whole_path_device_philox_equals_the_restated_tape_and_the_oracle():
    """One synthetic model, B = 3 ragged (198 / 150 / 97 frames, bucketed to 256), 20 f0 and 20 mel steps: forward(seed = s) - every draw on the
    device - against forward(noise = model_noise(s)) - the same draws restated on the host and fed as a tape - eager and as replayed hipGraphs, the
    vocoder the same way, and the CPU oracle (R.acoustic_forward, item by item as the reference runs) on those draws: the first comparison of
    the production noise with the oracle. Bars: the project's (mel L1 <= 1e-5, wav <= 1e-5, no voicing flip, pitch_coarse equal).

    Seed 20260 was checked on the CPU before the GPU run: the oracle run twice, once on the host draws rounded to fp32 and once with every
    Gaussian draw moved by +- its bound (r + 1) 2^-21 (random signs), gives the same uv in every step's result of both f0 samplers for all three
    items - no voicing decision of this input sits within draw rounding of its threshold.

    Teeth: the tape run repeated with a wrong restatement (step index shifted by one; items 0 and 1 swapped) is at least 100 x the bar away."""
    hp, sd, items, batch = whole_path_setup()
    B, T, S = len(WP_LENS), max(WP_LENS), WP_STEPS
    model = _model(hp, sd, use_graphs="off")
    b = {k: v.to(DEV) for k, v in batch.items()}
    dev_run = _fwd(model, b, seed=WP_SEED)
    bounds = list(model._plan(B, model.bucket_frames(T), torch.device(DEV)).bounds)
    noise = P.model_noise(WP_SEED, B, T, S, S, bounds)
    tape_run = _fwd(model, b, noise=noise)
    eager = _dist(dev_run, tape_run)
    model.use_graphs = "on"
    g1 = _fwd(model, b, seed=WP_SEED)     # captures
    g1 = {k: v.clone() for k, v in g1.items() if torch.is_tensor(v)}
    g2 = _fwd(model, b, seed=WP_SEED)     # replays
    for k in ("mel_out", "uv_a", "uv_b", "f0_a", "f0_b", "pitch_coarse"):
        assert torch.equal(g1[k], dev_run[k]) and torch.equal(g2[k], dev_run[k]), f"hipGraph replay differs from the eager launches in {k}"
    graph = _dist(g2, tape_run)
    # vocoder on the tape run's output
    voc, _ = _vocoder()
    mel_v = tape_run["mel_out"].clamp(-6.0, 1.5)
    lens_t = torch.tensor(WP_LENS, device=DEV, dtype=torch.int32)
    wav_p = voc.model(mel_v, tape_run["f0_denorm"], lens=lens_t, seed=WP_SEED)
    wav_t = voc.model(mel_v, tape_run["f0_denorm"], lens=lens_t, noise=P.vocoder_noise(WP_SEED, B, T * 256))
    wav_max = float((wav_p - wav_t).abs().max())
    # the CPU oracle on the same draws, item by item
    o_l1 = o_n = 0.0
    o_flips = 0
    for i, (Ti, it) in enumerate(zip(WP_LENS, items)):
        with torch.no_grad():
            ref = R.acoustic_forward(sd, hp, {k: v[None] for k, v in it.items()}, P.ReplayTape(item_noise(noise, i, Ti)), mel2ph=it["mel2ph"][None])
        d = (dev_run["mel_out"][i, :Ti].cpu() - ref["mel_out"][0]).abs()
        o_l1, o_n = o_l1 + float(d.sum()), o_n + d.numel()
        o_flips += int((dev_run["uv_a"][i, :Ti].cpu().long() != ref["uv_a"][0]).sum()) + int((dev_run["uv_b"][i, :Ti].cpu().long() != ref["uv_b"][0]).sum())
        assert torch.equal(dev_run["pitch_coarse"][i, :Ti].cpu(), ref["pitch_coarse"][0]), f"item {i}: pitch_coarse differs from the oracle"
    o_l1 /= o_n
    print(f"whole path, device Philox vs restated tape: eager {eager}, graph {graph}, wav max {wav_max:.3e}; vs the CPU oracle: mel L1 {o_l1:.3e}, flips {o_flips}")
    record_measurement("noise_whole_path", eager=eager, graph=graph, wav_max=wav_max, oracle_mel_l1=o_l1, oracle_flips=o_flips, seed=WP_SEED)
    for name, d in (("eager", eager), ("graph", graph)):
        assert d["flips"] == 0 and d["coarse"] == 0 and d["mel_l1"] <= MEL_L1_TOL, (name, d)
    assert wav_max <= WAV_TOL
    assert o_flips == 0 and o_l1 <= MEL_L1_TOL
    # teeth
    def shifted(nz):
        out = {k: dict(v) for k, v in nz.items()}
        for k in out:
            out[k]["z_steps"] = nz[k]["z_steps"].roll(1, dims=0)
        return out

    def swapped(nz):
        perm = [1, 0, 2]
        return {k: {kk: (vv[:, perm] if kk.startswith(("z_steps", "u_steps")) else vv[perm]) for kk, vv in v.items()} for k, v in nz.items()}
    for name, wrong in (("step index shifted by one", shifted(noise)), ("items 0 and 1 swapped", swapped(noise))):
        d = _dist(dev_run, _fwd(model, b, noise=wrong))
        print(f"teeth, {name}: {d}")
        assert d["mel_l1"] >= 100.0 * MEL_L1_TOL, (name, d)
