"""The vocoder output denoise's host side (no GPU): the float64 restatement (tests/denoise_ref.py) against torch's float64 stft / istft, the
argument checks of `ss_wav_denoise`, the workspace query, the opt-in resolver, and the plugin / hparams plumbing. Parity with librosa itself is
UNPINNED (the package is un-vendored); what is held here is the definition in stylesinger_amd/denoise.py."""
import numpy as np
import pytest
import torch

from denoise_ref import denoise_ref, envelope, hann, sine_noise, zero_envelope
from stylesinger_amd import config, lib
from stylesinger_amd import denoise as DN

GEOMETRIES = [(1024, 256), (512, 128), (2048, 512), (1024, 512), (256, 256)]


def _torch_route(x, N, H, v):
    """torch.stft(center=True, pad_mode='constant') -> polar(clamp(|S| - v, 0), angle) -> torch.istft, float64"""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float64))
    w = torch.from_numpy(hann(N))
    S = torch.stft(xt, N, hop_length=H, win_length=N, window=w, center=True, pad_mode="constant", return_complex=True)
    Y = torch.polar(torch.clamp(S.abs() - v, min=0.0), torch.angle(S))
    return S.shape[-1], torch.istft(Y, N, hop_length=H, win_length=N, window=w, center=True).numpy()


TORCH_REFUSALS = ("window overlap add min", "Expected reduction dim")   # istft: an envelope that touches zero (H = N); an empty result (one frame)


@pytest.mark.parametrize("v", [0.0, 0.1])
@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("N,H", GEOMETRIES)
def test_restatement_matches_torch_float64(N, H, T, v):
    """max-abs <= 1e-12 (both are float64 orderings of the same sums; measured 2e-16 ... 4e-16). n = (T - 1) H + 5: T frames, five samples that
    reach the frames but not the output. torch is asked in every case; where its istft REFUSES with one of the two errors above (H = N: the
    envelope touches zero; T = 1: the result is empty) the case has no torch answer: an empty result is held to its length, H = N at v = 0 to the
    identity out == in at every sample whose envelope is not zero (`test_restatement_is_the_identity_where_torch_refuses`), and H = N at v = 0.1
    has no comparison here beyond the recorded refusal - the device test holds the kernel to the restatement there."""
    n = (T - 1) * H + 5
    x = sine_noise(n, 100 + T)
    got = denoise_ref(x, N, H, v)
    assert got.shape == (H * (n // H),) and got.dtype == np.float64
    try:
        frames, ref = _torch_route(x, N, H, v)
    except RuntimeError as e:
        assert any(r in str(e) for r in TORCH_REFUSALS), e
        assert H == N or T == 1, "torch refuses only the zero envelope and the empty result"
        print(f"N {N} H {H} T {T} v {v}: torch.istft refuses ({[r for r in TORCH_REFUSALS if r in str(e)][0]}): no comparison")
        return
    assert frames == T == 1 + n // H
    err = np.abs(got - ref).max()
    print(f"N {N} H {H} T {T} v {v}: restatement vs torch float64 {err:.2e}")
    assert ref.shape == got.shape and err <= 1e-12


@pytest.mark.parametrize("T", [2, 9])
def test_restatement_is_the_identity_where_torch_refuses(T):
    """(256, 256), v = 0: out == in except at the samples whose envelope is 0 (w[0] = 0: exact zeros). A sample is w irfft(rfft(w x)) / w^2: the
    transform pair's rounding error (a few 2^-53 per butterfly level on a frame of |x| <= 1: within 4 log2(N) 2^-52) is divided by w[k], 1.5e-4
    next to a frame edge - the bound is that quotient per sample (measured: 1.0e-12 there, 2e-16 away from the edges), not a flat 1e-12."""
    N = H = 256
    n = (T - 1) * H + 5
    x = sine_noise(n, 100 + T)
    ident = denoise_ref(x, N, H, 0.0)
    live = ~zero_envelope(n, N, H)
    assert len(ident) == (T - 1) * H and live.sum() == len(ident) - len(ident) // N
    w_at = hann(N)[(np.arange(len(ident)) + N // 2) % H]
    err = np.abs(ident - x[:len(ident)])
    print(f"N {N} H {H} T {T}: identity {err[live].max():.2e}")
    assert (err[live] <= 4 * np.log2(N) * 2.0 ** -52 / w_at[live]).all()
    assert (ident[~live] == 0.0).all(), "w[0] = 0: an undivided sample is an exact zero"


def test_fp32_transform_cannot_hold_the_bar_where_the_hop_is_the_frame():
    """Why hop_size == fft_size runs in float64 on the device. The same steps in fp32 (`denoise_f32_emulation`: torch's fp32 FFT, fp32 arrays) lie
    within 1e-6 of the restatement where frames overlap (measured 1.2e-7 ... 2.4e-7), and beyond the 1e-5 bar at (256, 256) (measured 1.0e-4 ...
    6.4e-4 at 1 ... 40 hops): there a sample is divided by w^2 alone, the transform's rounding error by w, 1.5e-4 next to a frame edge. The
    restatement rounded once to fp32 - what a float64 kernel stores - stays inside the bar at the same inputs."""
    from denoise_ref import denoise_f32_emulation
    for N, H, hops in ((1024, 256, 12), (1024, 512, 12), (256, 64, 40)):
        x = sine_noise(hops * H, 3)
        err = np.abs(denoise_f32_emulation(x, N, H, 0.1) - denoise_ref(x, N, H, 0.1)).max()
        print(f"fp32 emulation N {N} H {H}: {err:.2e}")
        assert err <= 1e-6
    for hops in (1, 12, 40):
        x = sine_noise(hops * 256, 3)
        ref = denoise_ref(x, 256, 256, 0.1)
        err = np.abs(denoise_f32_emulation(x, 256, 256, 0.1) - ref).max()
        stored = np.abs(ref.astype(np.float32).astype(np.float64) - ref).max()
        print(f"fp32 emulation N 256 H 256, {hops} hops: {err:.2e}; the restatement rounded to fp32: {stored:.2e} (max |y| {np.abs(ref).max():.1f})")
        assert err > 1e-5 and stored <= 2e-6


def test_restatement_layout():
    """frame count, envelope length and the cut: the numbers of the definition"""
    assert len(envelope(5 * 256 + 3, 1024, 256)) == 1024 + 256 * 5
    assert np.allclose(envelope(40 * 256, 1024, 256)[1024:-1024], 1.5, rtol=0, atol=1e-12), "Hann^2 at 75 % overlap sums to 1.5"
    assert zero_envelope(1024, 256, 256).tolist() == [k % 256 == 128 for k in range(1024)]
    assert not zero_envelope(1024, 256, 64).any()
    assert len(denoise_ref(np.zeros(63), 256, 64, 0.1)) == 0
    big = denoise_ref(sine_noise(2048, 5), 1024, 256, 1e6)
    assert (big == 0.0).all()
    assert (denoise_ref(np.zeros(2048), 1024, 256, 0.0) == 0.0).all(), "m = 0 gives 0, not NaN"


def test_table_holds_the_twiddles_and_the_window():
    t = DN.table_f64(256)
    assert t.shape == (768,) and t.dtype == np.float64
    tw = t[0:512:2] + 1j * t[1:512:2]
    assert tw[0] == 0 and tw[1] == 1
    for s in (1, 2, 4, 8, 16, 32, 64, 128):
        assert np.abs(tw[s:2 * s] - np.exp(-2j * np.pi * np.arange(s) / (2 * s))).max() <= 2e-16, s
    assert tw[2] == 1 and tw[3].real == np.cos(np.pi / 2) and tw[3].imag == -1.0
    assert np.array_equal(t[512:], hann(256)) and t[512] == 0.0 and t[512 + 128] == 1.0


def test_symbols_and_argument_errors_are_reported_before_a_device_is_touched():
    l = lib.load()
    for name in ("ss_wav_denoise", "ss_wav_denoise_workspace_bytes"):
        assert name in lib.declared_symbols()
    p = 1 << 32   # placeholder non-null pointers: every refusal below comes before anything is dereferenced or launched

    far = p + (1 << 30)   # an output range that does not touch the input's

    def run(x=p, ldx=4096, Lx=4096, n=p, y=far, ldy=4096, Ly=4096, n_out=p, B=2, n_fft=1024, hop=256, v=0.1, table=p, ws=None, wsb=0):
        return l.ss_wav_denoise(x, ldx, Lx, n, y, ldy, Ly, n_out, B, n_fft, hop, v, table, ws, wsb, None)
    for null in ("x", "n", "y", "n_out", "table"):
        assert run(**{null: None}) != 0 and b"ss_wav_denoise: null argument" in l.ss_last_error(), null
    for n_fft in (1000, 128, 4096, 0):
        assert run(n_fft=n_fft) != 0 and b"bad fft_size" in l.ss_last_error(), n_fft
    for hop in (0, 32, 96, 2048, 384):
        assert run(hop=hop) != 0 and b"bad hop_size" in l.ss_last_error(), hop
    assert run(ldx=4095) != 0 and b"bad dims" in l.ss_last_error()
    assert run(ldy=4000) != 0 and b"bad dims" in l.ss_last_error()
    assert run(B=0) != 0 and b"bad dims" in l.ss_last_error()
    assert run(B=65536) != 0 and b"bad dims" in l.ss_last_error()
    assert run(Lx=4100, ldx=4100, Ly=4095, ldy=4095) != 0 and b"shorter than the longest possible output (4096 samples)" in l.ss_last_error()
    assert run(Lx=4100, ldx=4100, Ly=4095, ldy=4095, n_fft=2048, hop=2048) != 0 and b"(4096 samples)" in l.ss_last_error()
    for v in (-0.1, float("nan"), float("inf")):
        assert run(v=v) != 0 and b"bad v" in l.ss_last_error(), v
    assert run(wsb=-1) != 0 and b"workspace of -1 bytes, need 0" in l.ss_last_error()
    for y in (p, p + 4, p + 4 * (4096 + 4095), p - 4 * (4096 + 4095)):      # equal, shifted, the last / first float of the two ranges shared
        assert run(y=y) != 0 and b"alias" in l.ss_last_error(), hex(y)
    assert run(y=p + 4 * 2 * 4096, v=-1.0) != 0 and b"bad v" in l.ss_last_error(), "adjacent ranges are not aliases (the call fails later, on v)"
    assert l.ss_abi_version() == 20, "the export is additive"


def test_workspace_query():
    """0 for every supported geometry (the header's formula: the overlap-add lives in LDS), negative for an unsupported one"""
    l = lib.load()
    for N, H in GEOMETRIES + [(256, 64), (2048, 64), (2048, 2048)]:
        assert l.ss_wav_denoise_workspace_bytes(8, 384000, N, H) == 0, (N, H)
    for N, H in ((1000, 250), (1024, 0), (1024, 384), (1024, 32), (128, 64), (4096, 1024), (1024, 2048)):
        assert l.ss_wav_denoise_workspace_bytes(8, 384000, N, H) < 0, (N, H)
    assert l.ss_wav_denoise_workspace_bytes(0, 384000, 1024, 256) < 0 and l.ss_wav_denoise_workspace_bytes(8, 0, 1024, 256) < 0


def test_the_opt_in_resolver():
    assert DN.resolve_denoise(None) is None and DN.resolve_denoise({}) is None
    for off in (0, 0.0, -0.1, None):
        assert DN.resolve_denoise(dict(vocoder_denoise_c=off)) is None
    assert DN.resolve_denoise(dict(vocoder_denoise_c=0, fft_size=1000)) is None, "off: the geometry is nobody's business"
    assert DN.resolve_denoise(dict(vocoder_denoise_c=0.1)) == 0.1
    assert DN.resolve_denoise(dict(vocoder_denoise_c=0.1, fft_size=512, win_size=512, hop_size=128)) == 0.1
    assert DN.geometry(dict(fft_size=512, win_size=512, hop_size=128)) == (512, 128) and DN.geometry({}) == (1024, 256)
    for bad, key in ((dict(fft_size=1000, win_size=1000), "fft_size"), (dict(fft_size=4096, win_size=4096), "fft_size"), (dict(fft_size=128, win_size=128), "fft_size"),
                     (dict(fft_size=1024.0), "fft_size"), (dict(win_size=512), "win_size"), (dict(fft_size=2048), "win_size"), (dict(hop_size=96), "hop_size"),
                     (dict(hop_size=32), "hop_size"), (dict(hop_size=2048), "hop_size"), (dict(hop_size=0), "hop_size")):
        with pytest.raises(lib.StyleSingerHipError, match=key + "=") as ei:
            DN.resolve_denoise(dict(vocoder_denoise_c=0.1, **bad))
        assert "vocoder_denoise_c" in str(ei.value)
    with pytest.raises(lib.StyleSingerHipError, match="finite"):
        DN.resolve_denoise(dict(vocoder_denoise_c=float("inf")))


def test_device_entry_point_refuses_host_tensors_and_bad_arguments():
    with pytest.raises(lib.StyleSingerHipError, match="device tensors"):
        DN.denoise_batch(torch.zeros(1, 4096), [4096], 1024, 256, 1024, 0.1)
    with pytest.raises(lib.StyleSingerHipError, match="win_size="):
        DN.denoise_batch(torch.zeros(1, 4096), [4096], 1024, 256, 512, 0.1)
    with pytest.raises(ValueError, match="v must be"):
        DN.denoise_batch(torch.zeros(1, 4096), [4096], 1024, 256, 1024, -1.0)


def test_plugin_and_hparams_plumbing_without_a_device():
    from stylesinger_amd.infer import StyleSingerInfer
    from stylesinger_amd.vocoder import HifiGAN
    hp = config.make_hparams()
    assert hp["vocoder_denoise_c"] == 0.0 and "fft_size" not in hp and "win_size" not in hp, "the reference's default; nothing else is new"
    hp = config.make_hparams(dict(vocoder_denoise_c=0.1, fft_size=512, win_size=512, hop_size=128))
    assert (hp["vocoder_denoise_c"], hp["fft_size"], hp["win_size"], hp["hop_size"]) == (0.1, 512, 512, 128)
    assert HifiGAN(device="cpu")._denoise_v is None and HifiGAN(hparams=dict(vocoder_denoise_c=0.0), device="cpu")._denoise_v is None
    voc = HifiGAN(hparams=dict(vocoder_denoise_c=0.1), device="cpu")
    assert voc._denoise_v == 0.1 and voc.hparams["vocoder_denoise_c"] == 0.1
    with pytest.raises(lib.StyleSingerHipError, match="fft_size=1000"):
        HifiGAN(hparams=dict(vocoder_denoise_c=0.1, fft_size=1000, win_size=1000), device="cpu")
    with pytest.raises(lib.StyleSingerHipError, match="win_size=512"):
        StyleSingerInfer(dict(vocoder_denoise_c=0.1, win_size=512), device="cuda")   # refused before anything touches a device
    # the batched path needs hop_size == the generator's hop (then n_out == n): refused by spec2wav_batch, before the denoise launch
    voc = HifiGAN(hparams=dict(vocoder_denoise_c=0.1, hop_size=128), device="cpu")
    voc.model = type("G", (), dict(hop=256, __call__=lambda self, *a, **k: torch.zeros(1, 512)))()
    with pytest.raises(lib.StyleSingerHipError, match="hop_size=128"):
        voc.spec2wav_batch(None, None)


@pytest.mark.parametrize("flag,want", [(["--vocoder-denoise-c", "0.1"], 0.1), (["--vocoder-denoise-c", "0"], 0.0), ([], None)])
def test_cli_flag_sets_the_hparam(monkeypatch, flag, want):
    """`python -m stylesinger_amd.infer ... --vocoder-denoise-c V`: main() hands hparams['vocoder_denoise_c'] = V to the run (the checkpoint
    loads and the run itself are stubbed: no file, no device); without the flag the key is not set at all."""
    from stylesinger_amd import infer
    seen = {}
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(infer.StyleSingerInfer, "example_run", classmethod(lambda cls, hparams=None, *a, **k: seen.update(hp=hparams)))
    infer.main(["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"] + flag)
    assert "hp" in seen
    if want is None:
        assert not seen["hp"] or "vocoder_denoise_c" not in seen["hp"]
    else:
        assert seen["hp"]["vocoder_denoise_c"] == want
        from stylesinger_amd import denoise as DN
        assert DN.resolve_denoise(config.make_hparams(seen["hp"])) == (want or None)
