"""The vocoder with a generator whose ONLY stage the grouped Winograd kernel takes has 32 channels (upsample_initial_channel = 64, rates 8 x 8:
stages of 32 and 16 channels), so that what SS_VOC_WINO switches is exactly the 32-column tile of ss_wino43_conv.

Batches, inputs, reference and bound are built the way tests/vocoder_shape_cases.py builds them for its own generator cases (its helpers,
unchanged): wav against the float64 generator on the fp32 harmonic source, within 4 x the larger error of the fp32 CPU restatement in direct
and in emulated grouped-F(4,3) form (WinoConvs emulates every square 3 / 7 / 11-tap conv, the 16-channel stage included, so the bound is
no tighter than the device's arithmetic warrants), at least 2 fp32 ulp at 1.0."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_vocoder_shapes as S  # noqa: E402  (device-side helpers: buffers with sentinel tails, ss_hifigan_forward)
import vocoder_shape_cases as V  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import restatement as R  # noqa: E402
from oracle.wino_vocoder_numerics import WinoConvs  # noqa: E402
from stylesinger_amd import config, lib as L, synth  # noqa: E402
from stylesinger_amd.vocoder import HifiGanGeneratorHIP  # noqa: E402

CASE = dict(upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=64, audio_sample_rate=16000)
SEED = 3264


@functools.lru_cache(maxsize=None)
def _generator():
    cfg = config.make_vocoder_config(CASE)
    return cfg, synth.synth_vocoder_state_dict(cfg, SEED)


@functools.lru_cache(maxsize=None)
def _inputs(batch):
    cfg, _ = _generator()
    B, T, _ = V.BATCHES[batch]
    hp = config.make_hparams()
    seed = SEED + 10 + sorted(V.BATCHES).index(batch)
    g = torch.Generator().manual_seed(seed)
    mel = (torch.randn(B, T, 80, generator=g) * 0.8 - 3.0).clamp(hp["mel_vmin"], hp["mel_vmax"])
    f0 = torch.stack([synth.synth_f0_hz(i, T, seed, dtype=torch.float32) for i in range(B)])
    noise = synth.draw_vocoder_noise(synth.NoiseTape(seed + 1), B, T * V.hop_of(cfg))
    return mel, f0, noise


@functools.lru_cache(maxsize=None)
def _reference(batch):
    """As vocoder_shape_cases.generator_reference: per item har (fp32), wav64, the two CPU fp32 errors and the bound."""
    cfg, vsd = _generator()
    mel, f0, noise = _inputs(batch)
    hop = V.hop_of(cfg)
    vsd64 = {k: v.double() for k, v in vsd.items()}
    out = []
    with torch.no_grad():
        for b, n in enumerate(V.BATCHES[batch][2]):
            m, f = mel[b:b + 1, :n], f0[b:b + 1, :n]
            wav32, har = R.hifigan_forward(vsd, cfg, m, f, V.ItemTape(noise, b, n * hop))
            with WinoConvs():
                wav_w, _ = R.hifigan_forward(vsd, cfg, m, f, None, har=har)
            wav64, _ = R.hifigan_forward(vsd64, cfg, m.double(), None, None, har=har.double())
            e_direct = (wav32.double() - wav64).abs().max().item()
            e_wino = (wav_w.double() - wav64).abs().max().item()
            out.append(dict(n=n, har=har[0], wav64=wav64[0], e_direct=e_direct, e_wino=e_wino,
                            bound=max(4.0 * max(e_direct, e_wino), V.WAV_FLOOR)))
    return out


def _packed(monkeypatch, wino):
    if wino:
        monkeypatch.delenv("SS_VOC_WINO", raising=False)
    else:
        monkeypatch.setenv("SS_VOC_WINO", "0")
    monkeypatch.delenv("SS_PRECISION", raising=False)
    cfg, vsd = _generator()
    gen = HifiGanGeneratorHIP(cfg)
    gen.load_state_dict(vsd, strict=True)
    gen.eval().to(S.DEV)
    gen.pack()
    assert gen._pk["hg"].wino == (1 if wino else 0)
    return gen


def test_only_the_32_channel_stage_qualifies():
    cfg, _ = _generator()
    lib = L.load()
    widths = [cfg["upsample_initial_channel"] >> (i + 1) for i in range(len(cfg["upsample_rates"]))]
    assert widths == [32, 16]
    for k, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
        for d in list(ds) + [1]:
            assert lib.ss_wino43_conv_ok(32, k, d) == 1 and lib.ss_wino43_conv_ok(16, k, d) == 0


@pytest.mark.parametrize("batch", list(V.BATCHES))
def test_c32_generator_matches_float64_in_both_conv_forms(batch, monkeypatch):
    cfg, _ = _generator()
    hop = V.hop_of(cfg)
    B, T, lens = V.BATCHES[batch]
    mel, f0, noise = _inputs(batch)
    ref = _reference(batch)
    wavs = {}
    for form, wino in (("wino", True), ("direct", False)):
        wav, har = S._forward(_packed(monkeypatch, wino), mel, f0, lens, noise)
        wavs[form] = wav
        worst = 0.0
        for b, r in enumerate(ref):
            n = r["n"] * hop
            eh = (har[b, :n] - r["har"]).abs().max().item()
            ew = (wav[b, :n].double() - r["wav64"]).abs().max().item()
            print(f"c32 {batch} {form} item {b} (T={r['n']}): har err {eh:.3e}; wav err {ew:.3e} (CPU fp32: direct {r['e_direct']:.3e}, "
                  f"F(4,3) {r['e_wino']:.3e}), bound {r['bound']:.3e}")
            worst = max(worst, ew / r["bound"])
        record_measurement(f"voc_c32_{form}_{batch}", worst_err_over_bound=worst)
        for b, r in enumerate(ref):
            n = r["n"] * hop
            assert bool((wav[b, n:] == 0).all()), f"{form}: wav of item {b} is not exactly 0 behind its {r['n']} frames"
            assert (har[b, :n] - r["har"]).abs().max().item() <= V.HAR_TOL
            assert (wav[b, :n].double() - r["wav64"]).abs().max().item() <= r["bound"], (batch, form, b)
    assert not torch.equal(wavs["wino"], wavs["direct"]), "SS_VOC_WINO=0 must have switched the C = 32 stage to the direct kernel"
