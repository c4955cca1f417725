"""The on-device resampler (`ss_resample_poly`, csrc/resample.hip) and the reference-audio intake built on it: the kernel against the float64
table-loop restatement (tests/resample_ref.py) within the fp32 forward bound, determinism and batch independence, `preprocess_input` /
`preprocess_batch` / `infer_once` from audio of other rates and sample formats, graph capture. Parity with `librosa.load` is UNPINNED
(librosa / resampy are un-vendored); the definition is stylesinger_amd/resample.py's."""
import functools
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_measurement  # noqa: E402
from resample_ref import resample_f64  # noqa: E402
from stylesinger_amd import audiofile, config, synth  # noqa: E402
from stylesinger_amd import resample as RS  # noqa: E402

PAIRS = [(44100, 48000), (16000, 48000), (96000, 48000), (22050, 48000), (48000, 16000)]
N_IN = (20000, 4001, 300, 1)   # several output tiles; shorter than a filter wing (48 -> 16 kHz: 191 taps); a single sample
PAD = 37                       # row stride = Lx + PAD


@functools.lru_cache(maxsize=None)
def _case(sr_in, sr_out):
    """inputs [4, Lx] (float32 values), and per item the float64 result and sum |w| |x| - computed once per rate pair"""
    rng = np.random.default_rng(sr_in + 3 * sr_out)
    x = np.zeros((len(N_IN), max(N_IN)), dtype=np.float32)
    ref = []
    for b, n in enumerate(N_IN):
        x[b, :n] = (0.3 * rng.standard_normal(n)).astype(np.float32)
        ref.append(resample_f64(x[b, :n].astype(np.float64), sr_in, sr_out, with_bound=True))
    return x, ref


def _device_input(x):
    """rows strided (ldx > Lx), everything past an item's own samples NaN: padding must not leak into a sum"""
    buf = torch.full((x.shape[0], x.shape[1] + PAD), float("nan"))
    for b, n in enumerate(N_IN):
        buf[b, :n] = torch.from_numpy(x[b, :n])
    return buf.cuda()[:, :x.shape[1]]


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_kernel_matches_the_float64_restatement_within_the_fp32_forward_bound(sr_in, sr_out):
    """|y_dev - y_f64| <= (taps + 2) 2^-24 sum_j |w_j| |x_j| per output: weights rounded once to fp32 (one unit roundoff per product) plus an
    fp32 FMA chain of `taps` terms. Outputs past an item's length, and the `fix_length` sample, are exactly zero."""
    x, ref = _case(sr_in, sr_out)
    xd = _device_input(x)
    assert xd.stride(0) == x.shape[1] + PAD
    y, lens = RS.resample_batch(xd, list(N_IN), sr_in, sr_out)
    y = y.cpu().numpy().astype(np.float64)
    _, up, down, taps, _ = RS.polyphase_bank(sr_in, sr_out)
    assert lens == [RS.out_len(n, sr_in, sr_out) for n in N_IN] and y.shape == (len(N_IN), max(lens))
    worst = 0.0
    for b, n in enumerate(N_IN):
        want, s = ref[b]
        assert len(want) == lens[b]
        nc = n * up // down
        err, bound = np.abs(y[b, :nc] - want[:nc]), (taps + 2) * 2.0 ** -24 * s[:nc]
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        worst = max(worst, ratio)
        print(f"{sr_in} -> {sr_out} item {b} (n_in {n}, {nc} outputs): max |err| {err.max() if nc else 0.0:.3e}, worst err / bound {ratio:.4f}")
        assert np.isfinite(y[b]).all(), "NaN padding leaked"
        assert (err <= bound).all(), (b, float(err.max()))
        assert (y[b, nc:] == 0.0).all(), "columns past the computed outputs (the fix_length sample included) are exactly zero"
    record_measurement(f"resample_device_vs_float64_restatement_{sr_in}_{sr_out}", pinned=False, worst_err_over_fp32_forward_bound=worst, taps=taps)


def test_resampler_is_deterministic_and_independent_of_the_batch():
    x, _ = _case(44100, 48000)
    xd = _device_input(x)
    a, lens = RS.resample_batch(xd, list(N_IN), 44100, 48000)
    b, _ = RS.resample_batch(xd, list(N_IN), 44100, 48000)
    assert torch.equal(a, b)
    alone, n1 = RS.resample_batch(torch.from_numpy(x[1:2, :N_IN[1] + 5].copy()).cuda(), [N_IN[1]], 44100, 48000)   # another Lx, Ly, B
    assert n1 == [lens[1]] and torch.equal(alone[0, :n1[0]], a[1, :n1[0]]) and (a[1, n1[0]:] == 0).all()


def test_resample_batch_is_graph_capturable():
    x, _ = _case(44100, 48000)
    xd = torch.from_numpy(x).cuda()
    eager, _ = RS.resample_batch(xd, list(N_IN), 44100, 48000)     # (also uploads the bank and the length vectors once)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, _ = RS.resample_batch(xd, list(N_IN), 44100, 48000)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------
def _harmonic(n, sr, f0=220.0):
    """~band-limited sung-note-like signal: 8 harmonics with vibrato, rendered at any rate"""
    t = np.arange(n) / sr
    ph = 2 * np.pi * f0 * t + 0.3 * np.sin(2 * np.pi * 5.0 * t)
    return sum(0.2 / h * np.sin(h * ph + 0.3 * h) for h in range(1, 9)).astype(np.float32)


def _write_wav(path, tag, bits, channels, rate, payload):
    align = channels * bits // 8
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    return str(path)


@pytest.fixture(scope="module")
def tiny():
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    inf = StyleSingerInfer(hp, device=torch.device("cuda:0"), model_state=synth.synth_acoustic_state_dict(hp, 5),
                           vocoder_state=synth.synth_vocoder_state_dict(None, 5), emotion_state=synth.synth_emotion_state_dict(5),
                           speaker_state=synth.synth_emotion_state_dict(6))
    return inf, hp


FEATURES = ("mel", "f0", "spk_embed", "emo_embed")


@pytest.mark.filterwarnings("ignore:StyleSingerInfer. trim_long_silences skipped")
def test_preprocess_input_takes_files_of_other_rates_and_formats(tiny, tmp_path):
    inf, hp = tiny
    n = 30870                                   # 0.7 s at 44.1 kHz
    w = _harmonic(n, 44100)
    pcm = np.round(w * 32767).astype("<i2")
    stereo = np.stack([pcm, pcm[::-1]], axis=1)  # two different channels
    f_i16 = _write_wav(tmp_path / "stereo16.wav", 1, 16, 2, 44100, stereo.tobytes())
    f_f32 = _write_wav(tmp_path / "mono32.wav", 3, 32, 1, 44100, w.astype("<f4").tobytes())
    it = synth.synth_batch(1, 40, 5, 8, hp, 5)
    base = dict(name="t", ph_token=it["txt_tokens"][0].numpy(), note=it["note"][0].numpy(), note_dur=it["note_dur"][0].numpy(),
                note_type=it["note_type"][0].numpy(), mel2ph=it["mel2ph"][0].numpy())
    n48 = RS.out_len(n, 44100, 48000)
    for path in (f_i16, f_f32):
        a = inf.preprocess_input(dict(base, ref_audio=path), vad_flags=False)
        assert a["mel"].shape == (n48 // 256 + 1, 80) and a["f0"].shape == (n48 // 256 + 1,) and np.isfinite(a["mel"]).all()
        arr, sr = audiofile.load_audio(path)
        assert sr == 44100 and len(arr) == n
        by_hand, (nh,) = RS.resample_batch(torch.from_numpy(arr)[None].cuda(), [n], 44100, 48000)
        assert nh == n48
        routes = (dict(ref_audio=(arr, 44100)), dict(ref_audio=arr, ref_sr=44100), dict(ref_audio=by_hand[0, :nh].cpu().numpy()))
        for r in routes:
            o = inf.preprocess_input(dict(base, **r), vad_flags=False)
            for k in FEATURES:
                assert np.array_equal(a[k], o[k]), (path, sorted(r), k)
    assert (a["f0"] > 0).sum() > 30, "the tracker finds the note in the resampled audio"
    # a 48 kHz 16-bit file: the same results as the array route without a rate (no resampling on that path)
    w48 = _harmonic(33600, 48000)
    pcm48 = np.round(w48 * 32767).astype("<i2")
    f48 = _write_wav(tmp_path / "mono48.wav", 1, 16, 1, 48000, pcm48.tobytes())
    p = inf.preprocess_input(dict(base, ref_audio=f48), vad_flags=False)
    q = inf.preprocess_input(dict(base, ref_audio=pcm48.astype(np.float32) / 32768.0), vad_flags=False)
    for k in FEATURES:
        assert np.array_equal(p[k], q[k]), k
    out = inf.infer_once(dict(base, ref_audio=f_i16), vad_flags=False)
    assert out.ndim == 1 and len(out) > 0 and np.isfinite(out).all()


def test_preprocess_batch_with_mixed_rates_equals_the_items_one_by_one(tiny):
    inf, hp = tiny
    srs = [44100, 48000, 16000]
    lens = [30870, 33600 - 77, 11200 + 5]
    wav = torch.zeros(3, max(lens))
    for b, (n, sr) in enumerate(zip(lens, srs)):
        wav[b, :n] = torch.from_numpy(_harmonic(n, sr, f0=(196.0, 262.0, 330.0)[b]))
    it = synth.synth_batch(3, 48, 6, 8, hp, 5)
    keys = ("txt_tokens", "note", "note_dur", "note_type", "mel2ph")
    batch = inf.preprocess_batch(wav, lens, None, None, *[it[k] for k in keys[:4]], mel2ph=it["mel2ph"], ref_srs=srs)
    for b in range(3):
        one = inf.preprocess_batch(wav[b:b + 1, :lens[b]], [lens[b]], None, None, *[it[k][b:b + 1] for k in keys[:4]], mel2ph=it["mel2ph"][b:b + 1],
                                   ref_srs=[srs[b]])
        n_mel = RS.out_len(lens[b], srs[b], 48000) // 256 + 1
        assert one["ref_mels"].shape[1] >= n_mel
        for k in ("ref_mels", "ref_f0", "ref_f0_hz"):
            assert torch.equal(batch[k][b, :n_mel], one[k][0, :n_mel]), (b, k)
        for k in ("spk_embed", "emo_embed"):
            assert torch.equal(batch[k][b], one[k][0]), (b, k)
