"""Contour alignment by dynamic time warping without a GPU: the definition (stylesinger_amd/pitch.py::contour_align, align_path) against the
reference's own algorithm (utils/dtw.py: time_warp, align_from_distances) and against a brute-force minimum over all monotone paths, the band rule,
the not-aligned fallback, the musical case the mode exists for, and the host plumbing (forward's refusals are in tests/test_gpu_contour_align.py:
forward needs packed weights)."""
import itertools
import sys
import types
import warnings

import numpy as np
import pytest

import contour_align_cases as K
from stylesinger_amd import abi
from stylesinger_amd import lib
from stylesinger_amd import pitch as P


def _ref_dtw():
    """The reference's utils/dtw.py, or None where the reference is not mounted. numba is not installed: `@jit` becomes the identity."""
    from oracle import refimport
    if not refimport.available():
        return None
    if "numba" not in sys.modules:
        sys.modules["numba"] = types.SimpleNamespace(jit=lambda f: f)
    refimport.load()
    import importlib
    return importlib.import_module("utils.dtw")


# ---- 1. the definition against the reference's algorithm ------------------------------------------------------------------------------------
def test_path_equals_the_reference_algorithm_on_padded_matrices():
    """The reference treats row 0 / column 0 of its matrix as a boundary (dtw[0, 1:] = dtw[1:, 0] = inf, the walk stops at i == 0 or j == 0), so the
    definition on C equals align_from_distances on C padded with one leading row and column: [r - 1 for r in ref(pad(C))[1:]]."""
    dtw = _ref_dtw()
    if dtw is None:
        pytest.skip("the reference is not mounted")
    rng = np.random.default_rng(5)
    for _ in range(300):
        n_t, n_c = (int(v) for v in rng.integers(1, 14, 2))
        C = rng.integers(0, 5, (n_t, n_c))                  # five distinct costs: ties on most cells
        padded = np.zeros((n_t + 1, n_c + 1), dtype=np.float64)
        padded[1:, 1:] = C
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = [r - 1 for r in dtw.align_from_distances(padded)[1:]]
        idx, cost = P.align_path(C)
        assert list(idx) == want, (n_t, n_c)
        assert cost == int(dtw.time_warp(padded)[n_t, n_c])


# ---- 2. the definition's own properties -------------------------------------------------------------------------------------------------------
def _brute_min(C):
    """Minimum cost over ALL monotone paths (steps down, right, diagonal) from (0, 0) to the far corner."""
    n_t, n_c = C.shape
    best = None
    stack = [(0, 0, int(C[0, 0]))]
    while stack:
        i, j, s = stack.pop()
        if i == n_t - 1 and j == n_c - 1:
            best = s if best is None else min(best, s)
            continue
        for a, b in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
            if a < n_t and b < n_c:
                stack.append((a, b, s + int(C[a, b])))
    return best


def test_full_matrix_cost_is_the_minimum_over_all_monotone_paths():
    rng = np.random.default_rng(11)
    for n_t, n_c in itertools.product(range(1, 6), repeat=2):
        for _ in range(4):
            C = rng.integers(0, 7, (n_t, n_c))
            idx, cost = P.align_path(C)
            assert cost == _brute_min(C), (n_t, n_c)
            assert idx[0] == 0 and (np.diff(idx) >= 0).all() and idx[-1] <= n_c - 1          # a monotone path from the first cell


def test_cost_does_not_rise_with_the_band_and_a_wide_band_is_the_full_matrix():
    rng = np.random.default_rng(12)
    for _ in range(40):
        n_t, n_c = (int(v) for v in rng.integers(2, 20, 2))
        C = rng.integers(0, 9, (n_t, n_c))
        full_idx, full_cost = P.align_path(C)
        w0 = -(-n_c // n_t)                                 # ceil(n_c / n_t): the narrowest band that is connected
        last = None
        for W in range(w0, max(n_t, n_c) + 3):
            idx, cost = P.align_path(C, W)
            assert idx is not None and cost >= full_cost
            assert last is None or cost <= last, (n_t, n_c, W)
            last = cost
            if W >= max(n_t, n_c):
                assert cost == full_cost and np.array_equal(idx, full_idx)


def test_every_band_with_nc_le_W_nt_reaches_the_end_cell():
    for n_t, n_c in itertools.product(range(1, 25), repeat=2):
        C = np.zeros((n_t, n_c), dtype=np.int64)
        for W in (0, 1, 2, 3, 5, 8, 30):
            W = max(W, -(-n_c // n_t))
            assert n_c <= W * n_t
            idx, cost = P.align_path(C, W)
            assert idx is not None and cost == 0, (n_t, n_c, W)
            ci = P.align_band_centres(n_t, n_c)
            assert (np.abs(idx - ci) <= W).all()            # the path stays inside the band


def test_an_item_the_band_cannot_connect_gets_the_linear_fit_and_status_1():
    rng = np.random.default_rng(13)
    g = K.random_cents(rng, 50)
    m = K.random_midi(rng, 3)
    for shift in (0.0, -2.5):
        out, idx, cost, status = P.contour_align(g, m, band=4, shift=shift)        # 50 > 4 * 3
        assert status == 1 and cost == 0 and (idx == -1).all()
        assert np.array_equal(out, P.contour_fit(g, 3, shift))
    out, idx, cost, status = P.contour_align(g, m, band=17)                          # 50 <= 17 * 3: aligned
    assert status == 0 and (idx >= 0).all()
    for gg, mm, n in ((g[:0], m, 3), (g, m[:0], 0)):                                  # empty items
        out, idx, cost, status = P.contour_align(gg, mm)
        assert status == 1 and cost == 0 and out.shape == (n,) and not out.any() and (idx == -1).all()


def test_cents_and_costs():
    hz = K.cents_to_hz([6900, 5700, 6001, 3000, 12345])
    assert K.cents_margin(hz) < 1e-3
    assert list(P.align_cents(hz)) == [6900, 5700, 6001, 3000, 12345]
    assert list(P.align_cents(hz, shift=-12)) == [5700, 4500, 4801, 1800, 11145]
    assert list(P.align_cents(np.float32([0.0, -3.0, np.nan, np.inf, 1e-30]))) == [P.ALIGN_UNVOICED] * 3 + [P.ALIGN_CENTS_HI, P.ALIGN_CENTS_LO]
    U = P.ALIGN_UNVOICED
    C = P.align_cost_matrix([6000, U, 9000], [6000, U, 6050])
    assert C.tolist() == [[0, P.ALIGN_UV_COST, P.ALIGN_CAP], [P.ALIGN_UV_COST, 0, P.ALIGN_UV_COST], [50, P.ALIGN_UV_COST, P.ALIGN_CAP]]
    # the clip of the guide's cents lies further than the cap outside the notes' range on both sides: it cannot change a cost
    assert P.ALIGN_CENTS_LO <= 100 - P.ALIGN_CAP and P.ALIGN_CENTS_HI >= 12700 + P.ALIGN_CAP
    assert (P.ALIGN_CAP, P.ALIGN_UV_COST) == (1200, 300)


# ---- 3. the musical case ------------------------------------------------------------------------------------------------------------------------
def test_a_guide_with_its_own_timing_is_warped_onto_the_score_where_the_linear_fit_fails():
    mc = K.musical_case()
    midi, guide, want = mc["midi"], mc["guide"], mc["want"]
    assert K.cents_margin(guide) < 1e-3
    # a condition on the INPUT: linear scaling puts the wrong note on at least one voiced frame in five
    linear = P.contour_fit(guide, len(midi))
    assert K.wrong_note_share(linear, want) >= 0.2
    for band in (None, K.BAND):
        out, idx, cost, status = P.contour_align(guide, midi, band=band)
        assert status == 0 and cost == 0
        assert out.dtype == np.float32 and np.array_equal(out, want)              # the note's frequency on EVERY frame, 0 on the rest
        assert K.wrong_note_share(out, want) == 0.0
        assert np.array_equal(guide[idx], want)
    # the guide an octave low, transposed into the score's key: the same result (x0.5 and x2 are exact in fp32)
    low = (guide * np.float32(0.5)).astype(np.float32)
    assert K.cents_margin(low, 12) < 1e-3
    out, idx, cost, status = P.contour_align(low, midi, band=K.BAND, shift=12)
    assert status == 0 and cost == 0 and np.array_equal(out, want)
    # without the transposition no voiced pair matches: every voiced score frame costs something (there is no automatic key detection)
    _, _, cost_low, _ = P.contour_align(low, midi, band=K.BAND)
    assert cost_low >= int((want > 0).sum())


# ---- 4. plumbing --------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_abi_version_stays():
    names = lib.declared_symbols()
    assert "ss_contour_align" in names and "ss_contour_align_workspace_bytes" in names
    assert abi.DEFINES["SS_ABI_VERSION"] == 20
    assert (lib.ALIGN_MAX_T, lib.ALIGN_MAX_LC) == (abi.DEFINES["SS_ALIGN_MAX_T"], abi.DEFINES["SS_ALIGN_MAX_LC"]) == (P.ALIGN_MAX_T, P.ALIGN_MAX_LC)
    assert P.ALIGN_MAX_T >= 5625 and P.ALIGN_MAX_LC >= 5625                       # the longest item of the benchmark configurations
    assert 16 * P.ALIGN_MAX_T + 2 * P.ALIGN_MAX_LC <= 160 * 1024                  # the kernel's LDS layout at the caps
    assert (P.ALIGN_MAX_T + P.ALIGN_MAX_LC) * P.ALIGN_CAP < P.ALIGN_INF < 2 ** 31 - P.ALIGN_CAP   # int32 D cannot overflow
    restype, argtypes = lib.declarations()["ss_contour_align"]
    assert len(argtypes) == 21


def test_entry_refuses_bad_arguments_before_any_launch():
    l = lib.load()
    p = 4096     # any non-null address: every call below is refused before it is used
    ok = dict(f0=p, ldc=8, Lc=8, lc=p, midi=p, ldm=8, lt=p, band=0, uv=300, cap=1200, shift=0.0, out=2 * p, ldo=8, idx=p, cost=p, st=p, T=8, B=1, ws=p,
              wsb=64)

    def call(**kw):
        a = dict(ok, **kw)
        return l.ss_contour_align(a["f0"], a["ldc"], a["Lc"], a["lc"], a["midi"], a["ldm"], a["lt"], a["band"], a["uv"], a["cap"], a["shift"], a["out"],
                                  a["ldo"], a["idx"], a["cost"], a["st"], a["T"], a["B"], a["ws"], a["wsb"], None)
    for kw, word in ((dict(f0=None), b"null pointer"), (dict(midi=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(st=None), b"null pointer"),
                     (dict(B=0), b"bad dims"), (dict(ldc=4), b"bad dims"), (dict(ldm=4), b"bad dims"), (dict(ldo=4), b"bad dims"),
                     (dict(out=p), b"alias"), (dict(wsb=63), b"workspace"), (dict(band=2, wsb=39), b"workspace"),
                     (dict(shift=48.5), b"semitones"), (dict(shift=float("nan")), b"semitones"),
                     (dict(T=P.ALIGN_MAX_T + 1, ldm=P.ALIGN_MAX_T + 1, ldo=P.ALIGN_MAX_T + 1), b"caps"),
                     (dict(Lc=P.ALIGN_MAX_LC + 1, ldc=P.ALIGN_MAX_LC + 1), b"caps"), (dict(cap=1201), b"cap="), (dict(uv=-1), b"uv_cost=")):
        assert call(**kw) != 0, kw
        err = l.ss_last_error()
        assert b"ss_contour_align" in err and word in err, (kw, err)
    q = l.ss_contour_align_workspace_bytes
    assert q(3, 100, 50, 0) == 3 * 100 * 50 and q(3, 100, 50, 4) == 3 * 100 * 9 and q(3, 100, 50, 40) == 3 * 100 * 50
    assert q(1, P.ALIGN_MAX_T, P.ALIGN_MAX_LC, 0) == P.ALIGN_MAX_T * P.ALIGN_MAX_LC
    assert q(0, 8, 8, 0) == 0 and q(1, P.ALIGN_MAX_T + 1, 8, 0) == 0 and q(1, 8, P.ALIGN_MAX_LC + 1, 0) == 0 and q(1, 0, 8, 0) == 0


def test_device_wrapper_refuses_host_tensors():
    import torch
    with pytest.raises(lib.StyleSingerHipError, match="device tensors"):
        P.contour_align_device(torch.zeros(1, 8), [8], torch.zeros(1, 8, dtype=torch.long), torch.tensor([8], dtype=torch.int32), 8)


def test_align_inputs_and_pitch_inputs():
    import torch
    from stylesinger_amd import producers
    f = producers.align_inputs
    assert f({}, False, 48000, 256) == {} and f({"pitch_hz": [1.0]}, True, 48000, 256) == {}
    assert f({"pitch_align": "dtw"}, True, 48000, 256) == dict(pitch_align="dtw", pitch_align_band=375)       # 2.0 s by default
    assert f({"pitch_align": "dtw", "pitch_align_band_s": 0.5}, True, 24000, 128) == dict(pitch_align="dtw", pitch_align_band=94)
    assert f({"pitch_align": "dtw", "pitch_align_band_s": 0}, True, 48000, 256)["pitch_align_band"] == 0      # full
    for inp, has, word in (({"pitch_align": "dtw"}, False, "needs one of them"), ({"pitch_align": "linear"}, True, "'dtw'"),
                           ({"pitch_align_band_s": 1.0}, True, "needs pitch_align"), ({"pitch_align": "dtw", "pitch_align_band_s": -1}, True, ">= 0")):
        with pytest.raises(ValueError, match=word):
            f(inp, has, 48000, 256)
    me = types.SimpleNamespace(hparams=dict(audio_sample_rate=48000, hop_size=256), device=torch.device("cpu"))
    out = producers.ReferenceProducers._pitch_inputs(me, {"pitch_hz": np.full(9, 220.0), "pitch_shift": 2, "pitch_align": "dtw", "pitch_align_band_s": 1.0})
    assert out["pitch_align"] == "dtw" and out["pitch_align_band"] == 188 and out["pitch_shift"] == 2.0 and out["pitch_hz"][1] == [9]
    assert "pitch_align" not in producers.ReferenceProducers._pitch_inputs(me, {"pitch_hz": np.full(9, 220.0)})
    with pytest.raises(ValueError, match="needs one of them"):
        producers.ReferenceProducers._pitch_inputs(me, {"pitch_align": "dtw"})


def test_plan_song_copies_the_alignment_keys_into_every_segment_batch():
    from stylesinger_amd import controls, song
    assert "pitch_align" in controls.CONTOUR_KEYS and "pitch_align_band_s" in controls.CONTOUR_KEYS
    P_ = 8
    inp = dict(ph_token=list(range(1, P_ + 1)), note=[60, 62, 0, 64, 65, 0, 67, 69], note_dur=[0.3] * P_, note_type=[2, 2, 1, 2, 2, 1, 2, 2],
               ph_dur=[0.3] * P_, pitch_hz=np.full(100, 220.0), pitch_shift=1.0, pitch_align="dtw", pitch_align_band_s=0.5)
    plan = song.plan_song(inp, sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    assert len(plan.batches) >= 2
    for b in plan.batches:
        assert b["pitch_align"] == "dtw" and b["pitch_align_band"] == 94 and b["pitch_shift"] == 1.0 and "pitch_hz" in b
    plain = song.plan_song({k: v for k, v in inp.items() if not k.startswith("pitch_align")}, sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    assert all("pitch_align" not in b and "pitch_align_band" not in b for b in plain.batches)
    for k in range(len(plan.batches)):                       # the planner's cut of the contour is the linear one, with or without the mode
        assert np.array_equal(plan.batches[k]["pitch_hz"][0].numpy(), plain.batches[k]["pitch_hz"][0].numpy())
    with pytest.raises(ValueError, match="ph_dur"):
        song.plan_song({k: v for k, v in inp.items() if k != "ph_dur"})
    with pytest.raises(ValueError, match="needs one of them"):
        song.plan_song({k: v for k, v in inp.items() if k not in ("pitch_hz", "pitch_shift")})
    with pytest.raises(ValueError, match="needs pitch_align"):
        song.plan_song({k: v for k, v in inp.items() if k != "pitch_align"})


def test_cli_refuses_alignment_flags_without_a_contour(capsys, monkeypatch, tmp_path):
    from stylesinger_amd import infer
    base = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"]
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: pytest.fail("a checkpoint was loaded before the flags were checked"))
    for extra, word in ((["--pitch-align", "dtw"], "--pitch-align needs"), (["--pitch-align-band-s", "1", "--pitch-npy", "c.npy"], "needs --pitch-align"),
                        (["--pitch-align", "linear", "--pitch-npy", "c.npy"], "invalid choice"),
                        (["--pitch-align", "dtw", "--pitch-align-band-s", "-1", "--pitch-audio", "g.wav"], ">= 0")):
        with pytest.raises(SystemExit) as e:
            infer.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
    # with a contour the flags reach the run as inp['pitch_align'] / inp['pitch_align_band_s']
    seen = {}
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(infer.StyleSingerInfer, "example_run", classmethod(lambda cls, hparams=None, *a, pitch=None, **k: seen.update(pitch=pitch)))
    np.save(tmp_path / "c.npy", np.full(10, 220.0))
    infer.main(base + ["--pitch-npy", str(tmp_path / "c.npy"), "--pitch-align", "dtw", "--pitch-align-band-s", "0"])
    assert seen["pitch"]["pitch_align"] == "dtw" and seen["pitch"]["pitch_align_band_s"] == 0.0 and len(seen["pitch"]["pitch_hz"]) == 10
