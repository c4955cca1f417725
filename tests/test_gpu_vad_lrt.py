"""The "lrt" voice-activity decision on the device (`ss_vad_lrt`, csrc/vad_lrt.hip; `vad_flags="lrt"`): the kernel against its definition
(stylesinger_amd/vadtrim.py::lrt_statistic) on every synthetic case of tests/vad_lrt_cases.py - the flags exactly (tests/test_vad_lrt_cpu.py
has shown that no window of any case sits near the threshold), the statistic within TOL (1 + |stat|), TOL = 16 x the float64 spread of the
definition itself -, batch and padding independence and determinism bit for bit, device flags through `trim_long_silences_device`, and the
entry point end to end. Parity with webrtcvad is neither claimed nor wanted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vad_lrt_cases as K  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import vadtrim as V  # noqa: E402

DEV = torch.device("cuda:0")


def _device(buf, lens, lens_on_device=False):
    x = torch.from_numpy(np.array(buf, dtype=np.float32)).to(DEV)      # (a copy: the shared cases are read-only)
    n = torch.tensor(lens, dtype=torch.int32).to(DEV) if lens_on_device else lens
    flags, stat = V.lrt_flags_device(x, n)
    assert flags.dtype == torch.uint8 and stat.dtype == torch.float64 and flags.shape == stat.shape and flags.is_cuda and stat.is_cuda
    return flags.cpu().numpy(), stat.cpu().numpy()


@pytest.mark.parametrize("name", K.CASES)
def test_kernel_equals_the_definition(name):
    """One item alone, its length read from a device array (then max_windows = the buffer's windows, two more than the item's): flags equal
    everywhere with no exclusions, |stat_dev - stat_host| <= TOL (1 + |stat_host|), columns at and beyond nW zero."""
    x, n, _, _ = K.case(name)
    stat_h, flags_h = K.host(name)
    nw = n // K.SPW
    buf = np.zeros((1, (nw + 2) * K.SPW + 5), dtype=np.float32)
    buf[0, :n] = x
    flags, stat = _device(buf, [n], lens_on_device=True)
    assert flags.shape == (1, nw + 2)
    err = float(np.max(np.abs(stat[0, :nw] - stat_h) / (1.0 + np.abs(stat_h)))) if nw else 0.0
    print(f"{name}: nW = {nw}, flagged {int(flags[0].sum())}, stat error {err:.2e} (TOL {K.tol():.2e})")
    assert np.array_equal(flags[0, :nw], flags_h), (name, np.nonzero(flags[0, :nw] != flags_h)[0][:8])
    assert err <= K.tol(), (name, err)
    assert not flags[0, nw:].any() and (stat[0, nw:] == 0).all()


def test_rows_do_not_depend_on_the_batch_the_stride_or_the_padding_and_repeat_bit_for_bit():
    buf0, lens = K.batch_buffer(K.BATCH3, 0.0)
    buf1, _ = K.batch_buffer(K.BATCH3, 1000.0)
    assert all(abs(buf1[i, n]) == 1000.0 and abs(buf1[i, -1]) == 1000.0 for i, n in enumerate(lens))
    f0, s0 = _device(buf0, lens)
    f0b, s0b = _device(buf0, lens)
    f1, s1 = _device(buf1, lens)
    assert np.array_equal(f0, f0b) and np.array_equal(s0.view(np.int64), s0b.view(np.int64)), "two runs"
    assert np.array_equal(f0, f1) and np.array_equal(s0.view(np.int64), s1.view(np.int64)), "zeros or +-1000 beyond the lengths"
    assert f0.shape == (3, max(lens) // K.SPW)
    for i, name in enumerate(K.BATCH3):
        x, n, _, _ = K.case(name)
        nw = n // K.SPW
        fa, sa = _device(x[None, :], [n])                                   # alone, another row stride, nothing behind the item
        assert fa.shape == (1, nw)
        assert np.array_equal(fa[0], f0[i, :nw]) and np.array_equal(sa[0].view(np.int64), s0[i, :nw].view(np.int64)), name
        assert np.array_equal(fa[0], K.host(name)[1]), name
        assert not f0[i, nw:].any() and (s0[i, nw:] == 0).all(), name


def test_device_flags_go_through_the_trim_without_a_host_copy():
    buf, lens = K.batch_buffer(K.BATCH3, 0.0)
    x = torch.from_numpy(buf).to(DEV)
    flags, _ = V.lrt_flags_device(x, lens)
    out_d, lens_d = V.trim_long_silences_device(x, lens, flags)
    out_h, lens_h = V.trim_long_silences_device(x, lens, flags.cpu().numpy())
    assert torch.equal(out_d, out_h) and torch.equal(lens_d, lens_h)
    kept = [int(v) for v in lens_d.cpu()]
    want = [int(V.window_mask(K.host(k)[1]).sum()) * K.SPW for k in K.BATCH3]
    assert kept == want and kept[0] < lens[0] - 28 * K.SPW, (kept, want)      # the 1.32 s pause is gone
    with pytest.raises(ValueError, match="flags must be"):
        V.trim_long_silences_device(x, lens, flags[:, :5])


def test_entry_point_with_the_lrt_decision():
    """`preprocess_input(vad_flags="lrt")` on an item with a long pause: the emotion embedding equals, bit for bit, the one from the flags
    `lrt_statistic` gives for the device-normalised audio, and differs from the untrimmed one; mel, f0 and the speaker embedding are the same in
    all three. `infer_once(vad_flags="lrt")` and an instance made with vad="lrt" run and agree."""
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    states = dict(model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 5),
                  emotion_state=synth.synth_emotion_state_dict(5), speaker_state=synth.synth_emotion_state_dict(6))
    inf = StyleSingerInfer(hp, device=DEV, **states)
    n = 256 * 140
    wav = K.harmonic_item(n, [(1000, 12000), (26000, 35000)], -60.0, 21)      # 74 windows, a pause of 29
    it = synth.synth_batch(1, 40, 5, 8, hp, 5)
    base = dict(name="t", ph_token=it["txt_tokens"][0].numpy(), note=it["note"][0].numpy(), note_dur=it["note_dur"][0].numpy(),
                note_type=it["note_type"][0].numpy(), mel2ph=it["mel2ph"][0].numpy())
    norm = inf._emo_front().normalize_volume(torch.from_numpy(wav)[None].to(DEV), torch.tensor([n]))[0].cpu().numpy()
    stat, flags = V.lrt_statistic(norm, n)
    assert np.min(np.abs(stat - V.LRT_ETA)) > K.tol() * (1.0 + V.LRT_ETA)
    assert flags[3:24].all() and not flags[27:52].any() and flags[56:72].all()
    a = inf.preprocess_input(dict(base, ref_audio=wav), vad_flags="lrt")
    b = inf.preprocess_input(dict(base, ref_audio=wav), vad_flags=flags)
    with pytest.warns(UserWarning, match="trim_long_silences skipped"):
        type(inf)._warned_untrimmed = False
        c = inf.preprocess_input(dict(base, ref_audio=wav), vad_flags=False)
    assert np.array_equal(a["emo_embed"], b["emo_embed"]) and not np.array_equal(a["emo_embed"], c["emo_embed"])
    for k in ("mel", "f0", "spk_embed"):
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    with pytest.raises(ValueError, match="emo_vad_flags"):
        inf.preprocess_batch(torch.from_numpy(wav)[None], [n], None, None, torch.from_numpy(base["ph_token"])[None], torch.from_numpy(base["note"])[None],
                             torch.from_numpy(base["note_dur"])[None], torch.from_numpy(base["note_type"])[None], emo_vad_flags="energy")
    out = inf.infer_once(dict(base, ref_audio=wav), vad_flags="lrt")
    inf2 = StyleSingerInfer(hp, device=DEV, vad="lrt", **states)
    out2 = inf2.infer_once(dict(base, ref_audio=wav))
    assert out.ndim == 1 and len(out) > 0 and np.isfinite(out).all()
    assert out.shape == out2.shape and np.abs(out - out2).max() <= 1e-5, np.abs(out - out2).max()      # the project's fp32 waveform bar
