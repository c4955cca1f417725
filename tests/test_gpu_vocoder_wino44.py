"""The vocoder with a generator of two stages, 64 and 32 channels (upsample_initial_channel = 128, rates 8 x 8): its k = 7 / 11 ResBlock convs
are the ones ss_wino44_conv_ok covers, on the 64-column and on the 32-column tile; the k = 3 convs stay on ss_wino43_conv.

That the k = 7 / 11 convs really take the F(4,4) kernel is shown from the pack: which path ss_hifigan_forward runs is decided in native
code by the same ss_wino44_conv_ok the pack asks, with no switch to turn, so the waveform of "the same generator through ss_wino43_conv"
cannot be produced through the entry point. Instead: (a) the pack transforms exactly the twelve k = 7 / 11 weights of each stage with
wino44_group_weight (14 and 21 components per input channel; ss_wino43_conv would read 18 and 24 from those rows and compute something
else), (b) the waveform from that pack is within the case's bound of the float64 generator, which only the F(4,4) kernel can get from it,
and (c) it differs from the waveform of the direct form (SS_VOC_WINO=0), which is within the same bound.

Inputs, reference and bound as tests/test_gpu_vocoder_c32.py builds them (the helpers of tests/vocoder_shape_cases.py, unchanged)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_vocoder_shapes as S  # noqa: E402
import vocoder_shape_cases as V  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import restatement as R  # noqa: E402
from oracle.wino_vocoder_numerics import WinoConvs  # noqa: E402
from stylesinger_amd import config, lib as L, synth  # noqa: E402
from stylesinger_amd.vocoder import HifiGanGeneratorHIP  # noqa: E402

CASE = dict(upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=128, audio_sample_rate=16000)
SEED = 6444
BATCH = "b3_t13_ragged"


@functools.lru_cache(maxsize=None)
def _generator():
    cfg = config.make_vocoder_config(CASE)
    return cfg, synth.synth_vocoder_state_dict(cfg, SEED)


@functools.lru_cache(maxsize=None)
def _inputs():
    cfg, _ = _generator()
    B, T, _ = V.BATCHES[BATCH]
    hp = config.make_hparams()
    g = torch.Generator().manual_seed(SEED + 10)
    mel = (torch.randn(B, T, 80, generator=g) * 0.8 - 3.0).clamp(hp["mel_vmin"], hp["mel_vmax"])
    f0 = torch.stack([synth.synth_f0_hz(i, T, SEED + 10, dtype=torch.float32) for i in range(B)])
    noise = synth.draw_vocoder_noise(synth.NoiseTape(SEED + 11), B, T * V.hop_of(cfg))
    return mel, f0, noise


@functools.lru_cache(maxsize=None)
def _reference():
    """As vocoder_shape_cases.generator_reference: per item har (fp32), wav64, the two CPU fp32 errors and the bound."""
    cfg, vsd = _generator()
    mel, f0, noise = _inputs()
    hop = V.hop_of(cfg)
    vsd64 = {k: v.double() for k, v in vsd.items()}
    out = []
    with torch.no_grad():
        for b, n in enumerate(V.BATCHES[BATCH][2]):
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


def test_k7_k11_convs_run_as_f44_groups(monkeypatch):
    cfg, _ = _generator()
    assert [cfg["upsample_initial_channel"] >> (i + 1) for i in range(2)] == [64, 32] and list(cfg["resblock_kernel_sizes"]) == [3, 7, 11]
    hop = V.hop_of(cfg)
    B, T, lens = V.BATCHES[BATCH]
    mel, f0, noise = _inputs()
    ref = _reference()

    seen = []
    real = L.wino44_group_weight

    def recording(w):
        out = real(w)
        seen.append((tuple(w.shape), tuple(out.shape)))
        return out
    monkeypatch.setattr(L, "wino44_group_weight", recording)
    wavs = {}
    for form, wino in (("wino", True), ("direct", False)):
        wavs[form], har = S._forward(_packed(monkeypatch, wino), mel, f0, lens, noise)
        for b, r in enumerate(ref):
            n = r["n"] * hop
            ew = (wavs[form][b, :n].double() - r["wav64"]).abs().max().item()
            print(f"c64 {form} item {b} (T={r['n']}): wav err {ew:.3e} (CPU fp32: direct {r['e_direct']:.3e}, F(4,3) {r['e_wino']:.3e}), bound {r['bound']:.3e}")
            record_measurement(f"voc_wino44_{form}_item{b}", wav_err=ew, bound=r["bound"])
            assert bool((wavs[form][b, n:] == 0).all())
            assert (har[b, :n] - r["har"]).abs().max().item() <= V.HAR_TOL
            assert ew <= r["bound"], (form, b, ew, r["bound"])
    # (a) the wino pack: convs1 (d = 1, 3, 5) and convs2 (d = 1) of the k = 7 and k = 11 ResBlocks of both stages, nothing else
    assert sorted(seen) == sorted([((c, c, 7), (c, c, 14)) for c in (64, 32)] * 6 + [((c, c, 11), (c, c, 21)) for c in (64, 32)] * 6), seen
    # (c)
    assert not torch.equal(wavs["wino"], wavs["direct"])
