"""The resampler's host side (no GPU): the polyphase bank against the independent table-loop restatement (tests/resample_ref.py), the restatement
against analytically resampled tones, the length rule, the WAV intake and the argument checks of `ss_resample_poly`. Parity with `librosa.load`
itself is UNPINNED (librosa / resampy are un-vendored); what is held here is the definition in stylesinger_amd/resample.py."""
import struct

import numpy as np
import pytest

from resample_ref import resample_f64
from stylesinger_amd import audiofile, lib
from stylesinger_amd import resample as RS

PAIRS = [(44100, 48000), (16000, 48000), (96000, 48000), (22050, 48000), (48000, 16000)]
# up, down, taps, left: upsampling walks the table in steps of 512 = one zero crossing: 64 left taps (input n itself included; only offsets 0 and 1
# leave room for the 64th) and 63 right ones, 64 where a phase comes within 1 / 512 of the next input (up = 320: 512 / 320 -> offset 1);
# downsampling by 2 / 3 walks it in steps of 256 / int(170.67) = 170: 128 / 192 left taps and 127 / 191 right ones.
PARAMS = {(44100, 48000): (160, 147, 127, 63), (16000, 48000): (3, 1, 127, 63), (96000, 48000): (1, 2, 255, 127),
          (22050, 48000): (320, 147, 128, 63), (48000, 16000): (1, 3, 383, 191)}


def _apply_bank(bank, up, down, taps, left, x, n_out):
    xz = np.concatenate([np.zeros(left), x, np.zeros(taps)])
    y = np.zeros(n_out)
    for t in range(len(x) * up // down):
        q = t * down
        y[t] = bank[q % up] @ xz[q // up:q // up + taps]
    return y


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_bank_applied_to_random_input_equals_the_table_loop_restatement(sr_in, sr_out):
    rng = np.random.default_rng(sr_in)
    x = rng.standard_normal(701)
    ref = resample_f64(x, sr_in, sr_out)
    bank, up, down, taps, left = RS.polyphase_bank_f64(sr_in, sr_out)
    got = _apply_bank(bank, up, down, taps, left, x, len(ref))
    err = float(np.abs(got - ref).max())
    print(f"{sr_in} -> {sr_out}: float64 bank vs restatement {err:.3e}")
    assert err <= 1e-12
    b32, *rest = RS.polyphase_bank(sr_in, sr_out)
    assert b32.dtype == np.float32 and tuple(rest) == (up, down, taps, left) and np.array_equal(b32, bank.astype(np.float32))
    assert RS.polyphase_bank(sr_in, sr_out)[0] is b32, "cached per rate pair"


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_bank_parameters_and_gain(sr_in, sr_out):
    bank, up, down, taps, left = RS.polyphase_bank_f64(sr_in, sr_out)
    assert (up, down, taps, left) == PARAMS[(sr_in, sr_out)] and bank.shape == (up, taps)
    scale = min(1.0, sr_out / sr_in)
    step = int(scale * 512)
    gain = bank.sum(axis=1)
    print(f"{sr_in} -> {sr_out}: row sums - 1 in [{gain.min() - 1:.3e}, {gain.max() - 1:.3e}]")
    if step == scale * 512:
        assert np.abs(gain - 1).max() <= 2e-6        # DC is in band: the in-band figure below
    else:                                            # the truncated step samples the filter scale * 512 / step times too densely: that much gain at most
        assert (gain > 1).all() and gain.max() - 1 <= scale * 512 / step - 1 <= 4e-3


def _tones(rng, sr_in, sr_out, k=12):
    f = rng.uniform(50.0, 0.85 * min(sr_in, sr_out) / 2, k)
    return f, rng.uniform(0.02, 0.08, k), rng.uniform(0, 2 * np.pi, k)


def _render(f, a, ph, n, sr):
    t = np.arange(n) / sr
    return sum(ai * np.sin(2 * np.pi * fi * t + pi) for fi, ai, pi in zip(f, a, ph))


# 48000 -> 16000 is left out on purpose: its truncated table step (170 for 170.67, as the package truncates) gives the 0.27 % gain pinned above
@pytest.mark.parametrize("sr_in", [44100, 16000, 22050, 32000, 96000])
def test_restatement_is_near_ideal_in_band(sr_in):
    """12 tones below 0.85 x the lower Nyquist, 6000 input samples: away from the ends (140 input samples: the wings are 64 / 128 long) the
    resampled signal is the analytically re-sampled one to 2e-6 (3 x the worst figure measured with a numpy statement of the definition)."""
    sr_out, n_in = 48000, 6000
    rng = np.random.default_rng(7 + sr_in)
    f, a, ph = _tones(rng, sr_in, sr_out)
    y = resample_f64(_render(f, a, ph, n_in, sr_in), sr_in, sr_out)
    want = _render(f, a, ph, len(y), sr_out)
    m = -(-140 * sr_out // sr_in)
    err = float(np.abs(y - want)[m:len(y) - m].max())
    print(f"{sr_in} -> {sr_out}: interior error vs analytic tones {err:.3e}")
    assert len(y) - 2 * m > 1000 and err <= 2e-6
    if sr_in == 96000:   # stop band: a tone above the new Nyquist is removed
        t = np.arange(n_in) / sr_in
        z = resample_f64(0.5 * np.sin(2 * np.pi * 1.15 * 24000 * t), sr_in, sr_out)
        leak = float(np.abs(z)[m:len(z) - m].max())
        print(f"96000 -> 48000: 0.5-amplitude tone at 1.15 x Nyquist comes out at {leak:.3e}")
        assert leak <= 1e-7


def test_out_len_and_the_padded_last_sample():
    for n_in, want in ((1, 2), (146, 159), (147, 160), (148, 162), (4001, 4355)):
        assert RS.out_len(n_in, 44100, 48000) == want == -(-n_in * 160 // 147)
        assert RS.computed_len(n_in, 44100, 48000) == n_in * 160 // 147
    rng = np.random.default_rng(1)
    x = rng.standard_normal(148) + 3.0
    y = resample_f64(x, 44100, 48000)
    assert len(y) == 162 and y[161] == 0.0 and y[160] != 0.0          # 148 * 160 / 147 = 161.09: 161 computed, one appended zero
    y = resample_f64(x[:147], 44100, 48000)
    assert len(y) == 160 and y[159] != 0.0                            # an integer product: nothing appended
    assert RS.out_len(5, 48000, 48000) == 5 and RS.out_len(7, 48000, 16000) == 3 and RS.computed_len(7, 48000, 16000) == 2
    same, lens = RS.resample_batch(x, [148], 48000, 48000)            # equal rates: the arguments come back untouched (no device needed)
    assert same is x and lens == [148]
    with pytest.raises(ValueError, match="47999.*48000|48000.*47999"):
        RS.polyphase_bank(47999, 48000)


def _wav_bytes(tag, bits, channels, rate, payload, extensible=False, extra_chunks=b""):
    align = channels * bits // 8
    if extensible:
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, channels, rate, rate * align, align, bits, 22, bits, 0) + struct.pack("<H", tag) + \
            bytes.fromhex("000000001000800000aa00389b71")
    else:
        fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + extra_chunks + b"data" + struct.pack("<I", len(payload)) + payload
    body += b"\0" * (len(payload) & 1)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def test_load_audio_decodes_the_sample_formats_exactly(tmp_path):
    rng = np.random.default_rng(3)
    n = 301

    def check(name, blob, want, rate):
        p = tmp_path / name
        p.write_bytes(blob)
        got, sr = audiofile.load_audio(str(p))
        assert sr == rate and got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got, want), name
        return p
    f32 = np.float32
    for ch in (1, 2):
        mono = (lambda v: v[:, 0] if ch == 1 else (v[:, 0] + v[:, 1]) / f32(2))
        u8 = rng.integers(0, 256, (n, ch), dtype=np.uint8)
        check(f"u8_{ch}.wav", _wav_bytes(1, 8, ch, 22050, u8.tobytes()), mono((u8.astype(f32) - 128) / 128), 22050)
        i16 = rng.integers(-32768, 32768, (n, ch)).astype("<i2")
        i16[0, 0], i16[1, 0] = -32768, 32767
        p16 = check(f"i16_{ch}.wav", _wav_bytes(1, 16, ch, 48000, i16.tobytes()), mono(i16.astype(f32) / 32768), 48000)
        assert np.array_equal(audiofile.load_audio(p16)[0], audiofile.load_pcm16(str(p16), 48000)), "bit-equal to the strict loader"
        i24 = rng.integers(-2 ** 23, 2 ** 23, (n, ch))
        i24[0, 0], i24[1, 0] = -2 ** 23, 2 ** 23 - 1
        raw24 = b"".join(int(v).to_bytes(3, "little", signed=True) for v in i24.reshape(-1))
        check(f"i24_{ch}.wav", _wav_bytes(1, 24, ch, 44100, raw24), mono(i24.astype(f32) / f32(2 ** 23)), 44100)
        i32 = rng.integers(-2 ** 31, 2 ** 31, (n, ch)).astype("<i4")
        check(f"i32_{ch}.wav", _wav_bytes(1, 32, ch, 96000, i32.tobytes()), mono((i32.astype(np.float64) / 2 ** 31).astype(f32)), 96000)
        x32 = rng.uniform(-1, 1, (n, ch)).astype("<f4")
        check(f"f32_{ch}.wav", _wav_bytes(3, 32, ch, 44100, x32.tobytes()), mono(x32), 44100)
        x64 = rng.uniform(-1, 1, (n, ch)).astype("<f8")
        check(f"f64_{ch}.wav", _wav_bytes(3, 64, ch, 16000, x64.tobytes()), mono(x64.astype(f32)), 16000)
    # extensible headers (either sub-format), an odd-sized LIST chunk (+ its pad byte) before the data, an odd-sized data chunk
    check("ext_pcm.wav", _wav_bytes(1, 24, 2, 44100, raw24, extensible=True), (lambda v: (v[:, 0] + v[:, 1]) / f32(2))(i24.astype(f32) / f32(2 ** 23)), 44100)
    check("ext_f32.wav", _wav_bytes(3, 32, 1, 32000, x32[:, 0].tobytes(), extensible=True), x32[:, 0], 32000)
    lst = b"LIST" + struct.pack("<I", 7) + b"INFOabc" + b"\0"
    check("list.wav", _wav_bytes(1, 16, 1, 44100, i16[:, 0].tobytes(), extra_chunks=lst), i16[:, 0].astype(f32) / 32768, 44100)
    check("odd.wav", _wav_bytes(1, 8, 1, 8000, u8[:, 0].tobytes()), (u8[:, 0].astype(f32) - 128) / 128, 8000)
    # refused, saying why
    (tmp_path / "a.flac").write_bytes(b"fLaC" + bytes(64))
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):
        audiofile.load_audio(tmp_path / "a.flac")
    (tmp_path / "adpcm.wav").write_bytes(_wav_bytes(2, 4, 1, 8000, bytes(64)))
    with pytest.raises(ValueError, match="format tag 0x2"):
        audiofile.load_audio(str(tmp_path / "adpcm.wav"))
    (tmp_path / "i12.wav").write_bytes(_wav_bytes(1, 40, 1, 8000, bytes(40)))
    with pytest.raises(ValueError, match="unsupported sample format"):
        audiofile.load_audio(str(tmp_path / "i12.wav"))


def test_resample_argument_errors_are_reported_before_a_device_is_touched():
    l = lib.load()
    assert "ss_resample_poly" in lib.declared_symbols()
    assert l.ss_resample_poly(None, 0, 0, None, None, 0, 0, None, None, 1, None, 1, 1, 1, 0, None) != 0 and b"ss_resample_poly" in l.ss_last_error()
    p = 0x1000   # placeholder non-null pointers: every refusal below comes before anything is dereferenced or launched
    assert l.ss_resample_poly(p, 8, 8, p, 2 * p, 8, 8, p, None, 1, p, 4097, 1, 127, 63, None) != 0 and b"bad filter" in l.ss_last_error()
    assert l.ss_resample_poly(p, 4, 8, p, 2 * p, 8, 8, p, None, 1, p, 3, 1, 127, 63, None) != 0 and b"bad dims" in l.ss_last_error()
    assert l.ss_resample_poly(p, 8, 8, p, 2 * p, 8, 8, p, None, 1, p, 1, 15000, 2000, 63, None) != 0 and b"down + taps" in l.ss_last_error()
    assert l.ss_resample_poly(p, 8, 8, p, p, 8, 8, p, None, 1, p, 3, 1, 127, 63, None) != 0 and b"alias" in l.ss_last_error()
    assert l.ss_abi_version() == 20, "the export is additive"
