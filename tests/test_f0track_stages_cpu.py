"""What tests/f0track_stage_refs.py claims about its own inputs, constants and decoder, the host-side geometry of the device tracker
(stylesinger_amd/f0track.py) against oracle/praat_pitch.py at every geometry the GPU file runs, and the argument refusals of `ss_f0track`
(they precede any launch, so they run without a device)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f0track_stage_refs as S  # noqa: E402
from oracle import praat_pitch as P  # noqa: E402
from stylesinger_amd import f0track as FT  # noqa: E402
from stylesinger_amd import lib  # noqa: E402


@pytest.mark.parametrize("name", list(S.INPUTS))
def test_every_gpu_input_is_stable_under_the_r_bound_and_its_spread_constants_hold(name):
    """The input condition of the exact assertions (candidate count, lags, selected candidate unchanged when the restatement's own r moves
    by the R bound, 8 seeded trials) and the committed SPREAD constants: not below the spread measured here, and not a loose guess either
    (they are the measurement rounded up to two digits)."""
    tr = S.perturbation_trials(name)
    assert tr["stable"], name
    if tr["frames"] == 0:
        assert name not in S.SPREAD and name in ("constant", "zeros", "frames0")
        return
    df, ds = S.SPREAD[name]
    print(f"{name}: spread over {S.TRIALS} trials {tr['df']:.3e} Hz, {tr['ds']:.3e}; committed {df:.1e}, {ds:.1e}")
    assert tr["df"] <= df and tr["ds"] <= ds, (name, tr)
    assert df == pytest.approx(S.round_up_2(tr["df"]), rel=1e-9) and ds == pytest.approx(S.round_up_2(tr["ds"]), rel=1e-9), (name, tr)


@pytest.mark.parametrize("name", list(S.INPUTS))
def test_inputs_are_fp16_valued_with_exact_sums_and_the_stats_reference_equals_the_restatement(name):
    """gpeak may be asserted EQUAL on the device only where the mean's sum is exact: all inputs are on the fp16 grid and short enough that every
    partial sum, in any order, is a float64. And the stats reference (direct float64, longdouble sums) agrees with the restatement's numpy."""
    x = S.signal(name)
    assert x.dtype == np.float32 and (x == x.astype(np.float16).astype(np.float32)).all()
    assert S.sums_are_exact(x) and len(x) % 2 == 0
    gpeak, intens, frames = S.stats_reference(name)
    x64 = x.astype(np.float64)
    assert float(np.sum(x64.astype(np.longdouble))) / len(x64) == S._mean(x64)
    ref = S.restatement(name)
    if ref is None:
        assert len(intens) == 0
        return
    assert len(intens) == ref["g"]["n_frames"]
    assert np.abs(np.where(intens < 0, 0.0, intens) - ref["intens"]).max() <= 4 * np.finfo(np.float64).eps
    if name == "constant":
        assert gpeak == 0.0 and x.any() and (intens == 0.0).all()
    if name == "zeros":
        assert gpeak == 0.0 and not x.any()


def test_the_inputs_reach_the_branches_they_were_built_for():
    # all 15 places full on every frame, at least one REPLACEMENT and one rejection per frame, candidates at or above the ceiling, path below it
    for name in ("tone1500", "tone1500_noise"):
        ref = S.restatement(name)
        assert len(ref["frames"]) == 33
        for (fs, _), r, lags in zip(ref["frames"], ref["r"], ref["lags"]):
            counts = {}
            P.frame_candidates(r, ref["g"], S.VOICING_THRESHOLD, counts=counts)
            assert len(fs) == S.MAXC and counts.get("replaced", 0) >= 1 and counts.get("rejected", 0) >= 1
            assert max(fs) >= ref["g"]["ceiling"] and lags[1:] != sorted(lags[1:])
        assert (ref["f0"] > 0).all() and (ref["f0"] < ref["g"]["ceiling"]).all()
    # silent frames (local peak exactly 0) inside a live item, next to voiced and to unvoiced live frames
    gpeak, intens, _ = S.stats_reference("silent_stretch")
    ref = S.restatement("silent_stretch")
    assert gpeak > 0 and 3 <= (intens == -1.0).sum() < len(intens) and len(intens) == 50
    assert (ref["f0"][intens == -1.0] == 0).all() and (ref["f0"] > 0).sum() >= 20 and ((ref["f0"] == 0) & (intens > 0)).any()
    # the silence-threshold term of the unvoiced strength is positive on some frames, and the item has voiced frames too
    ref = S.restatement("quiet_on_dc")
    knee = 2.0 * P.SILENCE_THRESHOLD / (1.0 + S.VOICING_THRESHOLD)
    assert (ref["intens"] < knee).sum() >= 5 and (ref["f0"] > 0).sum() >= 5
    # the ragged batch: 0, 1, 2, 33, 33 and 50 frames
    g = S.tables("default")[0]
    assert [FT.frame_grid(g, len(S.signal(n)))[0] for n in S.RAGGED] == [0, 1, 2, 33, 33, 50]
    assert [len(S.signal(n)) for n in S.RAGGED[:3]] == [1536, 256 * 8, 256 * 9]
    # 40 to 60 mel frames for every other signal
    for name, geom in S.INPUTS.items():
        if not name.startswith("frames"):
            assert 40 <= len(S.signal(name)) // S.GEOMETRIES[geom][1] <= 60, name
    # the other geometries are the ones the lag ownership of f0t_autocorr_kernel needs
    assert {k: S.tables(k)[0]["nlag"] for k in S.GEOMETRIES} == S.GEOMETRY_NLAG
    for name, geom in S.INPUTS.items():
        if name.startswith("geom_"):
            assert (S.restatement(name)["f0"] > 0).all()


def test_autocorr_reference_and_the_fft_route_agree_far_inside_the_derived_bound():
    """The restatement's FFT route against direct longdouble sums: a small fraction of the derived bound (the issue measured 9e-4), which is
    what makes "near the bound" on the device worth a look."""
    worst = 0.0
    for name in ("silent_stretch", "geom_sr16000", "geom_floor71"):
        _, intens, frames = S.stats_reference(name)
        _, _, wr = S.tables(S.INPUTS[name])
        ref, bound = S.restatement(name), S.r_bound(S.INPUTS[name])
        for i in [i for i in range(len(intens)) if intens[i] > 0][::9]:
            r = S.autocorr_reference(frames[i], wr)
            assert r[0] == 1.0 and len(r) == len(bound)
            worst = max(worst, float(np.max(np.abs(ref["r"][i] - r).astype(np.float64) / bound)))
    print(f"FFT route vs longdouble direct sums: {worst:.2e} of the bound")
    assert worst <= 0.05


@pytest.mark.parametrize("B,max_frames,nlag", [(1, 1, 4), (1, 33, 899), (6, 50, 899), (3, 7, 299), (2, 36, 449), (5, 34, 1013), (32, 1493, 899)])
def test_workspace_decoder_fits_the_size_the_library_asks_for(B, max_frames, nlag):
    layout, total = S.workspace_layout(B, max_frames, nlag)
    assert [r[0] for r in layout] == ["gpeak", "R", "intensity", "cand_f", "cand_s", "cand_i", "n_cand", "psi"]
    off = 0
    for name, o, dt, shape in layout:      # contiguous, in order, every region aligned for its type
        assert o == off and o % np.dtype(dt).itemsize == 0
        off += int(np.prod(shape)) * np.dtype(dt).itemsize
    need = lib.load().ss_f0track_workspace_bytes(B, max_frames, nlag)
    assert off == total and total <= need
    if B * max_frames * (nlag + 1) < 1 << 20:
        raw = np.arange(need, dtype=np.uint32).astype(np.uint8)
        ws = S.decode_workspace(raw, B, max_frames, nlag)
        assert ws["gpeak"].shape == (B,) and ws["R"].shape == (B, max_frames, nlag + 1) and ws["psi"].shape == (B, max_frames, S.MAXC)
        assert ws["psi"][-1, -1, -1] == raw[total - 1] and ws["cand_i"].dtype == np.int32


COUNTS = {"default": (40 * 256, 256 * 50 + 18, 9000), "hop128": (50 * 128, 128 * 40 + 54, 3000), "sr44100": (40 * 256, 256 * 45 + 130, 8270),
          "sr24000": (44 * 128, 128 * 41 + 6, 1500), "sr16000": (40 * 128, 128 * 43 + 100, 1000), "floor71": (41 * 256, 256 * 50 + 254, 9100)}


@pytest.mark.parametrize("geom", list(S.GEOMETRIES))
def test_host_geometry_and_frame_grid_follow_the_restatement_at_every_geometry(geom):
    sr, hop, floor = S.GEOMETRIES[geom]
    ts = S.time_step(geom)
    d = FT.geometry(sr, ts, floor, S.CEILING)
    for n in COUNTS[geom]:
        assert n % 2 == 0
        g = P.geometry(n, sr, ts, floor, S.CEILING)
        for k in ("dx", "nsamp_period", "halfnsamp_period", "nsamp_window", "halfnsamp_window", "maximum_lag", "time_step", "pitch_floor"):
            assert d[k] == g[k], (k, d[k], g[k])
        assert d["pitch_ceiling"] == g["ceiling"] and d["nlag"] == g["brent_ixmax"] and d["hop"] == hop and d["sr"] == sr
        assert d["window_duration"] == 3.0 / floor and d["nlag"] < 1024
        nf, left = FT.frame_grid(d, n)
        assert nf == g["n_frames"] and nf >= 1
        for i in (0, nf - 1):
            ws, ms, me = P.frame_start(g, i)
            right = left + i * hop + 1
            assert ws == right - d["halfnsamp_window"] and ms == right - d["nsamp_period"] and me == right + d["nsamp_period"]
            assert ws >= 0 and ws + d["nsamp_window"] <= n and ms >= 0 and me <= n
    assert any(n % hop for n in COUNTS[geom])


@pytest.mark.parametrize("geom", list(S.GEOMETRIES))
def test_frame_grid_has_no_frames_exactly_when_the_restatement_refuses_the_sound(geom):
    sr, hop, floor = S.GEOMETRIES[geom]
    ts = S.time_step(geom)
    d = FT.geometry(sr, ts, floor, S.CEILING)
    edge = int(np.ceil(3.0 / floor * sr))
    for n in (2, hop, edge - 3, edge - 2, edge - 1, edge, edge + 1, edge + 2, edge + hop):
        try:
            g = P.geometry(n, sr, ts, floor, S.CEILING)
        except ValueError as e:
            assert "shorter than the analysis window" in str(e)
            assert FT.frame_grid(d, n) == (0, 0), n
        else:
            assert FT.frame_grid(d, n)[0] == g["n_frames"] >= 1, n


def test_ss_f0track_refuses_bad_geometry_workspace_and_alignment_before_any_launch():
    """Real host buffers and a real parameter struct: the checks come before any launch and before any dereference but the struct's."""
    l = lib.load()
    n = 40 * 256
    wav = np.zeros(n, dtype=np.float32)
    out = np.full(40, 7.0, dtype=np.float32)

    def call(floor=80.0, ws_short=0, ws_shift=0, mutate=None):
        g, grid, max_frames, prm, lpad = FT.launch_setup([n], n, pitch_floor=floor)
        if mutate:
            mutate(prm)
        meta = np.array([[n], [grid[0][0]], [grid[0][1]]], dtype=np.int32)
        win, win_r = (t.numpy() for t in FT._window_tables(g, "cpu"))
        need = l.ss_f0track_workspace_bytes(1, max_frames, g["nlag"])
        ws = np.zeros(need // 8 + 4, dtype=np.float64)       # 8-byte aligned, with room to shift
        assert ws.ctypes.data % 8 == 0
        return l.ss_f0track(wav.ctypes.data, n, meta[0].ctypes.data, meta[1].ctypes.data, meta[2].ctypes.data, 1, max_frames, ctypes.byref(prm),
                            win.ctypes.data, win_r.ctypes.data, out.ctypes.data, 40, lpad, ws.ctypes.data + ws_shift, need - ws_short, None)

    assert FT.geometry(48000, 256 / 48000, 70.0, 800.0)["nlag"] == 1027
    assert call(floor=70.0) != 0 and b"bad geometry (window 2054, nlag 1027" in l.ss_last_error()
    assert call(ws_short=1) != 0 and b"workspace too small" in l.ss_last_error()
    assert call(ws_shift=4) != 0 and b"8-byte aligned" in l.ss_last_error()

    def odd_window(prm):
        prm.nsamp_window += 1
    assert call(mutate=odd_window) != 0 and b"bad geometry (window 1799, nlag 899" in l.ss_last_error()
    assert (out == 7.0).all()


def test_launch_setup_is_what_track_f0_device_launches_with():
    g, grid, max_frames, prm, lpad = FT.launch_setup([40 * 256, 1536, 57 * 256], 57 * 256)
    assert grid == [(33, 1023), (0, 0), (50, 1023)] and max_frames == 50 and lpad == 4
    assert (prm.nsamp_window, prm.halfnsamp_window, prm.nsamp_period, prm.halfnsamp_period, prm.maximum_lag, prm.nlag, prm.hop) == (1798, 899, 600, 301, 601, 899, 256)
    assert (prm.sample_rate, prm.pitch_floor, prm.pitch_ceiling, prm.voicing_threshold, prm.silence_threshold) == (48000.0, 80.0, 800.0, 0.6, 0.03)
    assert (prm.octave_cost, prm.octave_jump_cost, prm.voiced_unvoiced_cost) == (0.01, 0.35, 0.14) and prm.time_step == 256 / 48000 * 1000 / 1000
    assert FT.launch_setup([50 * 128], 50 * 128, hop_size=128)[4] == 8
    assert FT.launch_setup([100], 100)[2] == 1                                     # no frames: max_frames stays a valid launch dimension
    with pytest.raises(ValueError):
        FT.launch_setup([40 * 256], 40 * 256 - 1)                                  # the item is longer than the buffer
    with pytest.raises(KeyError):
        FT.launch_setup([40 * 256], 40 * 256, hop_size=200)
