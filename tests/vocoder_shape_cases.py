"""Shared cases of the vocoder shape tests (CPU-importable; test_gpu_vocoder_shapes.py runs them on the device, test_vocoder_shapes_cpu.py checks
their input conditions from the reference side alone).

A generator case is a `config.make_vocoder_config` override, chosen as the smallest way into one code path of hifigan.hip; a source case is
an f0 contour for `ss_hifigan_source`. The references are computed once per case (lru_cache) and never modified by a test."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import restatement as R  # noqa: E402
from oracle.wino_vocoder_numerics import WinoConvs  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402

WAV_TOL = 1e-5            # the project's waveform bar (test_gpu_parity.py, test_gpu_round4.py)
HAR_TOL = 2e-6            # harmonic source up to the golden's 51 200 samples (test_gpu_parity.py)
HAR_TOL_LONG = 2e-5       # phase integrated over more samples than that (test_fp32_waveform_matches_oracle_at_full_length)
HAR_TOL_SAMPLES = 51200
WAV_FLOOR = 2.0 * 2.0 ** -23   # 2 fp32 ulp at 1.0: |wav| <= 1

GENERATOR_CASES = {
    # 5 stages, last stage C = 16 (< 32: padded Np / Kp, 16 position groups in the noise conv, conv_post with C = 16), hop 512
    "hop512_5ups": dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], audio_sample_rate=44100),
    # hop 64 (the minimum): L = T * 64 is no multiple of 256 (partial conv_post tile); two ResBlock kernels (1/n scale, the j > 0 accumulate);
    # k = 5 and dilations 2, 4 never take the Winograd kernel
    "hop64_2ups": dict(upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=128, audio_sample_rate=16000,
                       resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 2, 4], [1, 3, 5]]),
    # hop 1024 (1024-thread source blocks, 16 waves in the block scan), u = 4 polyphase upsamplers (pad = 2, two phases per group)
    "hop1024": dict(upsample_rates=[8, 8, 4, 4], upsample_kernel_sizes=[16, 16, 8, 8], upsample_initial_channel=256),
    # C = 512 in stage 0 (more channels than the noise conv has threads), K = 1024 in conv_pre / ups[0]
    "wide1024": dict(upsample_initial_channel=1024),
    # the yardstick row: the same tests at the shape every other test uses
    "default": dict(),
}
# (B, T, lens): one short item whose every conv tile is partial (stage 0: 72 rows = one 64-position noise-conv tile + 8), and a ragged batch
BATCHES = {"b1_t9": (1, 9, (9,)), "b3_t13_ragged": (3, 13, (13, 1, 9))}


def hop_of(cfg):
    return int(np.prod(cfg["upsample_rates"]))


@functools.lru_cache(maxsize=None)
def generator(name):
    """(cfg, state dict) of a generator case; the seed depends on the case so that no two cases share weights by accident."""
    cfg = config.make_vocoder_config(GENERATOR_CASES[name])
    return cfg, synth.synth_vocoder_state_dict(cfg, 300 + sorted(GENERATOR_CASES).index(name))


class ItemTape:
    """Replays item `i` of a pre-drawn vocoder noise dict in the order hifigan_forward draws (rand_ini, sine noise, unused source noise)."""
    def __init__(self, noise, i, n):
        self.q = [noise["rand_ini"][i:i + 1], noise["sine_noise"][i:i + 1, :n], torch.zeros(1, n, 1)]

    def rand(self, *shape):
        return self.q.pop(0).clone()

    def randn(self, *shape):
        return self.q.pop(0).clone()


class BatchTape:
    """The same for a whole batch (every item at full length)."""
    def __init__(self, noise):
        B, n = noise["sine_noise"].shape[:2]
        self.q = [noise["rand_ini"], noise["sine_noise"], torch.zeros(B, n, 1)]

    def rand(self, *shape):
        return self.q.pop(0).clone()

    def randn(self, *shape):
        return self.q.pop(0).clone()


@functools.lru_cache(maxsize=None)
def generator_inputs(name, batch):
    """mel [B,T,80] inside [mel_vmin, mel_vmax], f0 [B,T] Hz, the noise dict of length T * hop - built like test_gpu_round4.py::_voc_inputs."""
    cfg, _ = generator(name)
    B, T, _ = BATCHES[batch]
    hp = config.make_hparams()
    seed = 7000 + 10 * sorted(GENERATOR_CASES).index(name) + sorted(BATCHES).index(batch)
    g = torch.Generator().manual_seed(seed)
    mel = (torch.randn(B, T, 80, generator=g) * 0.8 - 3.0).clamp(hp["mel_vmin"], hp["mel_vmax"])
    f0 = torch.stack([synth.synth_f0_hz(i, T, seed, dtype=torch.float32) for i in range(B)])
    noise = synth.draw_vocoder_noise(synth.NoiseTape(seed + 1), B, T * hop_of(cfg))
    return mel, f0, noise


@functools.lru_cache(maxsize=None)
def generator_reference(name, batch):
    """Per item of the batch, on the inputs truncated to the item's length and with the item's own tape:
         har   - fp32 harmonic source of the fp32 restatement (its fp32 roundings are part of the source's definition)
         wav64 - the generator in float64 applied to that source: what `wav` is judged against
         e_direct / e_wino - max error against wav64 of the fp32 restatement, and of the fp32 restatement under the CPU emulation of the
                 grouped F(4,3) arithmetic (oracle.wino_vocoder_numerics.WinoConvs)
         bound - 4 x the larger of the two (the project's rule for fp32 arithmetic in the small-kernel tests), at least 2 fp32 ulp at 1.0"""
    cfg, vsd = generator(name)
    mel, f0, noise = generator_inputs(name, batch)
    hop = hop_of(cfg)
    vsd64 = {k: v.double() for k, v in vsd.items()}
    out = []
    with torch.no_grad():
        for b, n in enumerate(BATCHES[batch][2]):
            m, f = mel[b:b + 1, :n], f0[b:b + 1, :n]
            wav32, har = R.hifigan_forward(vsd, cfg, m, f, ItemTape(noise, b, n * hop))
            with WinoConvs():
                wav_w, _ = R.hifigan_forward(vsd, cfg, m, f, None, har=har)
            wav64, _ = R.hifigan_forward(vsd64, cfg, m.double(), None, None, har=har.double())
            e_direct = (wav32.double() - wav64).abs().max().item()
            e_wino = (wav_w.double() - wav64).abs().max().item()
            out.append(dict(n=n, har=har[0], wav64=wav64[0], e_direct=e_direct, e_wino=e_wino, yardstick=max(e_direct, e_wino),
                            bound=max(4.0 * max(e_direct, e_wino), WAV_FLOOR)))
    return out


# ------------------------------------------------------------------------------------------------
# NSF source contours (B = 2, different per item). `gen`: the generator case whose hop / sample rate / l_linear the source runs with.
# ------------------------------------------------------------------------------------------------
def _contour(kind, T, cfg):
    sr, hop = cfg["audio_sample_rate"], hop_of(cfg)
    t = torch.arange(T, dtype=torch.float32)
    if kind == "first_unvoiced":
        f0 = torch.stack([210.0 + 2.0 * t, 330.0 - 1.5 * t])
        f0[:, 0] = 0.0
    elif kind == "all_unvoiced":
        f0 = torch.zeros(2, T)
    elif kind == "constant":
        f0 = torch.stack([torch.full((T,), 220.0), torch.full((T,), 331.7)])
    elif kind == "alternating":
        f0 = torch.stack([torch.full((T,), 180.0), 260.0 + t])
        f0[0, 0::2] = 0.0
        f0[1, 1::2] = 0.0
    elif kind == "integer_advance":   # f0 = k sr / hop: the phase advances by an integer per frame, wraps fall on frame boundaries
        f0 = torch.stack([torch.full((T,), float(sr) / hop), torch.full((T,), 2.0 * sr / hop)])
    elif kind == "high":              # f0 (h + 1) / sr >= 1 for the upper harmonics: the % 1 of the per-sample increment matters
        f0 = torch.stack([torch.linspace(1000.0, 4000.0, T), torch.full((T,), 4000.0)])
        f0[1, T // 2:] = 3999.5
    elif kind == "tracker":           # the long chunk-carry runs: tracker-like contours with unvoiced runs
        f0 = torch.stack([synth.synth_f0_hz(i, T, 4242, dtype=torch.float32) for i in range(2)])
    else:
        raise KeyError(kind)
    return f0.contiguous()


SCAN_CHUNK = 2048   # hifigan.hip: frames per pass of src_base_kernel / src_scan_kernel
SOURCE_CASES = {
    # name: (generator case, contour, T)
    "carry_2chunks": ("hop64_2ups", "tracker", SCAN_CHUNK + 1),
    "carry_3chunks": ("hop64_2ups", "tracker", 2 * SCAN_CHUNK + 1),
    "first_unvoiced": ("hop64_2ups", "first_unvoiced", 40),
    "all_unvoiced": ("hop64_2ups", "all_unvoiced", 40),
    "constant": ("hop64_2ups", "constant", 40),
    "alternating": ("hop64_2ups", "alternating", 40),
    "integer_advance": ("hop64_2ups", "integer_advance", 40),
    "high_4000hz_sr16000": ("hop64_2ups", "high", 40),
    "first_unvoiced_hop1024": ("hop1024", "first_unvoiced", 40),
    "first_unvoiced_hop512": ("hop512_5ups", "first_unvoiced", 40),
    "first_unvoiced_default": ("default", "first_unvoiced", 40),
}
PHILOX_CASES = {"philox_hop64": ("hop64_2ups", 40, 2031), "philox_hop1024": ("hop1024", 12, 2032)}   # name: (generator case, T, seed)


def source_bound(samples):
    return HAR_TOL if samples <= HAR_TOL_SAMPLES else HAR_TOL_LONG


@functools.lru_cache(maxsize=None)
def source_inputs(name):
    gen, kind, T = SOURCE_CASES[name]
    cfg, _ = generator(gen)
    f0 = _contour(kind, T, cfg)
    noise = synth.draw_vocoder_noise(synth.NoiseTape(8100 + sorted(SOURCE_CASES).index(name)), 2, T * hop_of(cfg))
    return f0, noise


@functools.lru_cache(maxsize=None)
def source_reference(name):
    cfg, vsd = generator(SOURCE_CASES[name][0])
    f0, noise = source_inputs(name)
    with torch.no_grad():
        return R.nsf_source(vsd, cfg, f0, BatchTape(noise))


def nsf_source_closed_form(vsd, cfg, f0, noise):
    """A second statement of SineGen.forward + SourceModuleHnNSF.forward (source.py:348-441, 518-531), written from their definition and
    independent of oracle.restatement.nsf_source: numpy float64, one closed form per frame instead of two running sums over samples, rounded
    to fp32 wherever the reference holds an fp32 tensor. Inside a frame the per-sample increment `rad` is constant, so
        cumsum(rad)[f, k]         = base_f + (k + 1) rad_f,                  base_f = sum_{f' < f} hop rad_f' (+ the initial phase)
        cumsum(rad + shift)[f, k] = q_f + (k + 1 - w) rad_f + w fl(rad_f - 1),   w = wraps of the frame up to sample k (an integer count)
    with torch's double accumulator and fp32 result for both. Returns har [B, L] float64."""
    f32, f64 = np.float32, np.float64
    hop, sr = hop_of(cfg), f32(cfg["audio_sample_rate"])
    f0 = f0.numpy().astype(f32)
    B, T = f0.shape
    nh = cfg["harmonic_num"] + 1
    fh = (f0[:, :, None] * np.arange(1, nh + 1, dtype=f32)).astype(f32)           # f0_buf: fundamental and overtones
    r = (fh / sr).astype(f32)
    rad = (r - np.floor(r)).astype(f32)                                           # % 1                       [B, T, nh]
    ini = noise["rand_ini"].numpy().astype(f32).copy()
    ini[:, 0] = 0
    r0 = (rad[:, 0] + ini).astype(f32)                                            # sample 0 carries the initial phase
    d0 = r0.astype(f64) - rad[:, 0].astype(f64)
    rad64 = rad.astype(f64)
    base = np.cumsum(hop * rad64, axis=1) - hop * rad64 + d0[:, None]             # before frame f            [B, T, nh]
    k1 = np.arange(1, hop + 1, dtype=f64)[None, None, :, None]
    c1 = (base[:, :, None] + k1 * rad64[:, :, None]).astype(f32)                  # first cumsum, fp32 result [B, T, hop, nh]
    tmp = (c1 - np.floor(c1)).astype(f32).reshape(B, T * hop, nh)
    over = np.zeros((B, T * hop, nh), dtype=bool)
    over[:, 1:] = (tmp[:, 1:] - tmp[:, :-1]) < 0
    w = np.cumsum(over.reshape(B, T, hop, nh), axis=2).astype(f64)                # wraps of the frame up to and including sample k
    radm1 = (rad - f32(1.0)).astype(f32).astype(f64)                              # fl(rad + shift) at a wrap
    s = (hop - w[:, :, -1]) * rad64 + w[:, :, -1] * radm1                         # the frame's sum of the second cumsum's addends
    s[:, 0] += d0
    q = np.cumsum(s, axis=1) - s
    q[:, 0] += d0                                                                 # frame 0: every sample of it already includes sample 0's r0
    c2 = (q[:, :, None] + (k1 - w) * rad64[:, :, None] + w * radm1[:, :, None]).astype(f32)
    arg = ((c2 * f32(2.0)).astype(f32) * f32(np.pi)).astype(f32)
    sines = (np.sin(arg.astype(f64)).astype(f32) * f32(0.1)).astype(f32).reshape(B, T * hop, nh)
    uv = np.repeat((f0 > 0).astype(f32), hop, axis=1)[:, :, None]
    namp = (uv * f32(0.003) + ((f32(1.0) - uv) * f32(0.1) / f32(3.0)).astype(f32)).astype(f32)
    sw = ((sines * uv).astype(f32) + (namp * noise["sine_noise"].numpy().astype(f32)).astype(f32)).astype(f32)
    lw = vsd["m_source.l_linear.weight"].reshape(-1).numpy().astype(f64)
    return np.tanh(sw.astype(f64) @ lw + float(vsd["m_source.l_linear.bias"][0]))
