"""The "lrt" voice-activity decision without a GPU: the properties of its definition (stylesinger_amd/vadtrim.py::lrt_statistic) on the
synthetic cases of tests/vad_lrt_cases.py, the float64 spread of the definition itself, the threshold margin of every case (so that the device
comparison, tests/test_gpu_vad_lrt.py, can demand exact flags), the host wiring (`_resolve_vad`, `StyleSingerInfer(vad=)`, `--vad`) and the
argument checks of `ss_vad_lrt`. Parity with webrtcvad is neither claimed nor wanted; the constants are unassessed on recordings.

Measured spread of the definition (numpy's FFT against a direct float64 DFT, largest |delta| / (1 + |stat|) over all cases): 1.37e-14, at the
one-window item (the other cases: 3e-16 .. 1.4e-14). TOL = 16 x spread = 2.2e-13: the factor covers a third summation order, the kernel's radix-2
transform (restated in numpy it sits at 4.0e-14 from the definition)."""
import ctypes

import numpy as np
import pytest

import vad_lrt_cases as K
from stylesinger_amd import lib, vadtrim as V


def test_constants_and_empty_item():
    assert (V.LRT_PEAK_DB, V.LRT_N_MIN, V.LRT_ETA) == (30.0, 1.0, 1.0)
    assert (V.LRT_N_FFT, V.LRT_K_LO, V.LRT_K_HI, V.LRT_Q_DIV) == (512, 3, 127, 10)
    x, n, _, _ = K.case("nw0")
    stat, flags = V.lrt_statistic(x, n)
    assert stat.shape == (0,) and stat.dtype == np.float64 and flags.shape == (0,) and flags.dtype == np.uint8


@pytest.mark.parametrize("name", K.CASES)
def test_definition_properties(name):
    """Clean items: every window wholly inside a voiced stretch is flagged, no window that touches none is. The item without pauses and the one
    at 20 dB SNR: every window is flagged (the peak rule: towards "everything is voice"). Silence: nothing is flagged, the statistic is 0."""
    x, n, voiced, kind = K.case(name)
    stat, flags = K.host(name)
    assert stat.shape == flags.shape == (n // K.SPW,) and stat.dtype == np.float64 and flags.dtype == np.uint8
    assert np.isfinite(stat).all() and (stat >= 0).all() and np.array_equal(flags, (stat > V.LRT_ETA).astype(np.uint8))
    on, off = K.expected_windows(n, voiced)
    if kind == "clean":
        assert len(on) and len(off) and flags[on].all() and not flags[off].any(), (name, stat[on].min(), stat[off].max())
    elif kind == "all":
        assert flags.all(), (name, stat.min())
    elif kind == "none":
        assert not flags.any() and (stat == 0).all(), name
    else:
        assert flags[on].all(), name      # too few noise windows for a stable noise spectrum: voiced windows are still voiced


def test_quantile_steps_from_one_to_two_windows_between_10_and_11():
    """q = max(1, ceil(nW / 10)): with ONE window a tenth as loud as the rest the noise spectrum is that window at nW = 10 (the statistic of
    the others is large), the mean of it and a loud one at nW = 11 (the peak rule then caps it 30 dB under the loudest window)."""
    rng = np.random.default_rng(3)
    for nw, q in ((10, 1), (11, 2)):
        P = rng.uniform(1e6, 2e6, size=(nw, 125))
        P[4] *= 0.01
        stat, flags = V.lrt_from_power(P)
        E = P.sum(1)
        quiet = np.sort(np.argsort(E, kind="stable")[:q])
        N = P[quiet].sum(0) / q
        thr = E.max() * 1e-3
        N = np.maximum(N * min(1.0, thr / N.sum()), V.LRT_N_MIN)
        g = P / N
        want = np.where(g > 1, g - np.log(np.maximum(g, 1.0)) - 1, 0).sum(1) / 125
        assert np.allclose(stat, want, rtol=1e-12, atol=0) and flags.sum() >= nw - 1


def test_ties_go_to_the_smaller_index():
    P = np.full((20, 125), 50.0)
    P[7:] = 1.0e6           # windows 0 .. 6 tie at the bottom (60 dB down: the peak rule stays out of it): q = 2 takes 0 and 1, N = 50
    stat, _ = V.lrt_from_power(P)
    assert (stat[:7] == 0).all() and (stat[7:] > 0).all()
    P2 = P.copy()
    P2[0, 0] = 75.0         # window 0 now louder than its peers: 1 and 2 are taken, and window 0's first bin exceeds the noise
    stat2, _ = V.lrt_from_power(P2)
    assert stat2[0] == ((1.5 - np.log(1.5)) - 1.0) / 125 and (stat2[1:7] == 0).all()
    P3 = P.copy()
    P3[1, 0] = 25.0         # a quieter window 1 and the tie 0, 2, ...: 1 and 0 are taken, bin 0 of the noise is their mean 37.5
    stat3, _ = V.lrt_from_power(P3)
    g = 50.0 / 37.5
    assert stat3[1] == 0 and stat3[0] == stat3[2] == ((g - np.log(g)) - 1.0) / 125


def test_spread_of_the_definition_and_threshold_margin():
    """The definition evaluated twice in float64 (numpy's FFT, a direct DFT); TOL = 16 x the largest difference. No window of any case may lie
    within TOL (1 + LRT_ETA) of LRT_ETA: a condition on the INPUTS (a violation = another seed, never another tolerance), asserted on the host
    definition alone so that the device comparison can demand exact flags."""
    spread, per = K.definition_spread()
    print("spread of the definition per case:", {k: "%.2e" % v for k, v in per.items()})
    assert 0 < spread < 1e-12, per      # float64 round-off, nothing structural
    tol = K.tol()
    assert tol == 16.0 * spread
    for name in K.CASES:
        stat, _ = K.host(name)
        if len(stat):
            margin = float(np.min(np.abs(stat - V.LRT_ETA)))
            print(name, "closest window to the threshold: %.3e" % margin)
            assert margin > tol * (1.0 + V.LRT_ETA), (name, margin)
            x, n, _, _ = K.case(name)
            _, flags_dft = V.lrt_from_power(K.dft_power(x, n))
            assert np.array_equal(flags_dft, K.host(name)[1]), name


def test_window_mask_of_lrt_flags_keeps_the_voiced_stretches_and_drops_the_long_pause():
    x, n, voiced, _ = K.case("pauses")
    _, flags = K.host("pauses")
    mask = V.window_mask(flags)
    on, _ = K.expected_windows(n, voiced)
    assert mask[on].all()
    (a0, b0), (a1, b1) = [(a // K.SPW, b // K.SPW) for a, b in voiced]
    assert a1 - b0 == 44      # the pause: 1.32 s
    assert not mask[b0 + 8:a1 - 8].any() and not mask[:a0 - 8].any()      # smoothing (8) and dilation (6) reach a few windows into it, no further
    kept = int(mask.sum()) * K.SPW
    assert kept < n - 28 * K.SPW


def test_item_does_not_depend_on_what_follows_it():
    x, n, _, _ = K.case("nw33")
    buf = np.concatenate([x, np.full(1000, 1000.0, np.float32)])
    a, fa = V.lrt_statistic(buf, n)
    assert np.array_equal(a, K.host("nw33")[0]) and np.array_equal(fa, K.host("nw33")[1])


def test_resolve_vad_and_constructor_default():
    from stylesinger_amd.infer import StyleSingerInfer
    inf = StyleSingerInfer.__new__(StyleSingerInfer)
    assert inf._resolve_vad("lrt") == "lrt" and inf._resolve_vad("webrtc") == "webrtc"
    with pytest.raises(ValueError, match="vad_flags"):
        inf._resolve_vad("energy")
    if not V.have_webrtcvad():      # vad=None: today's behaviour, and the message names the new way out
        with pytest.raises(ImportError, match='vad_flags="lrt"'):
            inf._resolve_vad(None)
    inf.vad = "lrt"
    assert inf._resolve_vad(None) == "lrt" and inf._resolve_vad("webrtc") == "webrtc"
    assert inf._resolve_vad([1, 0]).shape == (1, 2)
    with pytest.raises(ValueError, match="vad="):
        StyleSingerInfer(None, device="cuda", vad="energy")      # refused before anything touches a device


def test_cli_vad_flag(monkeypatch, capsys):
    from stylesinger_amd import infer
    base = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"]
    with pytest.raises(SystemExit) as e:
        infer.main(base + ["--vad", "lrt", "--no-vad-trim"])
    assert e.value.code == 2 and "exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        infer.main(base + ["--vad", "energy"])
    assert e.value.code == 2 and "invalid choice" in capsys.readouterr().err
    seen = {}
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(infer.StyleSingerInfer, "example_run", classmethod(lambda cls, *a, vad_flags=None, **k: seen.update(vad=vad_flags)))
    for flag, want in ((["--vad", "lrt"], "lrt"), (["--vad", "webrtc"], "webrtc"), ([], None), (["--no-vad-trim"], False)):
        infer.main(base + flag)
        got = seen.pop("vad")
        assert got == want and type(got) is type(want), (flag, got)


def test_entry_points_are_declared_and_refuse_bad_arguments():
    names = lib.declared_symbols()
    assert "ss_vad_lrt" in names and "ss_vad_lrt_workspace_bytes" in names
    l = lib.load()
    assert l.ss_abi_version() == 20
    restype, argtypes = lib.declarations()["ss_vad_lrt"]
    assert restype is ctypes.c_int and len(argtypes) == 21 and argtypes[10:13] == [ctypes.c_double] * 3
    q = l.ss_vad_lrt_workspace_bytes
    assert q(0, 1) == 0 and q(1, 0) == 0
    assert 0 < q(1, 1) < q(1, 2) < q(2, 2) and q(8, 266) == 8 * 266 * q(1, 1) and q(32, 1000) == 32 * 1000 * 129 * 8
    assert l.ss_vad_lrt(None, 0, None, 1, 1, 480, 512, 3, 127, 10, 30.0, 1.0, 1.0, None, None, 1, None, 1, None, 0, None) != 0
    assert b"ss_vad_lrt" in l.ss_last_error() and b"null" in l.ss_last_error()
    # every other refusal comes before a launch too: host buffers stand in for device memory, nothing reads them
    wav, n, tab = (ctypes.c_float * 1024)(), (ctypes.c_int32 * 1)(), (ctypes.c_double * 2048)()
    fl, ws = (ctypes.c_uint8 * 8)(), (ctypes.c_double * (129 * 2))()
    good = dict(spw=480, n_fft=512, k_lo=3, k_hi=127, q_div=10, max_w=2, ws_bytes=129 * 2 * 8, fstride=2)

    def run(**kw):
        a = dict(good, **kw)
        return l.ss_vad_lrt(ctypes.addressof(wav), 1024, ctypes.addressof(n), 1, a["max_w"], a["spw"], a["n_fft"], a["k_lo"], a["k_hi"], a["q_div"],
                            30.0, 1.0, 1.0, ctypes.addressof(tab), ctypes.addressof(fl), a["fstride"], None, 0, ctypes.addressof(ws), a["ws_bytes"], None)
    for kw, word in ((dict(n_fft=500), b"n_fft"), (dict(n_fft=256), b"samples_per_window"), (dict(k_hi=257), b"bin range"), (dict(k_lo=4, k_hi=3), b"bin range"),
                     (dict(n_fft=1024, k_lo=0, k_hi=400), b"bins"), (dict(ws_bytes=129 * 2 * 8 - 1), b"workspace"), (dict(q_div=0), b"q_div"),
                     (dict(max_w=5000, ws_bytes=1 << 40), b"max_windows"), (dict(fstride=1), b"strides")):
        assert run(**kw) != 0, kw
        err = l.ss_last_error()
        assert b"ss_vad_lrt" in err and word in err, (kw, err)
