"""The f0 tracker (csrc/f0track.hip) stage by stage: `ss_f0track` is called directly with a workspace the test owns, every region of which is
read back and held to a plain high-precision statement of the same operation. References, bars, inputs and the reasons for each are in
tests/f0track_stage_refs.py; tests/test_f0track_stages_cpu.py asserts the input condition the exact assertions here rest on (the
restatement's own candidate count, lags and path do not move when its autocorrelation moves by the derived R bound).

Every launch here starts from a workspace filled with 0xFF bytes (NaN doubles, -1 counts): a read of a region the kernels leave unwritten
on purpose - R of silent frames and items, rows beyond an item's frames, candidate slots >= n_cand, psi of frame 0 - cannot hide behind the
zeros a fresh allocation tends to hold. The contour lies inside a larger guarded buffer: nothing may be written outside [B, n_out].

No test here builds a frame on which the path chooses between "unvoiced" and a candidate at or above the ceiling: such a frame cannot exist
(f0track_stage_refs docstring); those candidates are exercised as lattice nodes by the 1500 Hz inputs.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import f0track_stage_refs as S  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import praat_pitch as P  # noqa: E402
from stylesinger_amd import f0track as FT  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

GUARD, SENTINEL = 64, -12345.0
_runs = {}


def _bits(a):
    return np.ascontiguousarray(a).view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def run(names, n_out=None, fill=0xFF):
    """One `ss_f0track` launch over the named inputs (one geometry) -> dict(out [B, n_out] float32, ws: the decoded workspace, n_frames, lpad,
    n_out, g). Cached: the stage tests of an input share one launch. n_out defaults to lpad + max_frames + 3."""
    key = (tuple(names), n_out, fill)
    if key in _runs:
        return _runs[key]
    geom = S.INPUTS[names[0]]
    assert all(S.INPUTS[n] == geom for n in names)
    sr, hop, floor = S.GEOMETRIES[geom]
    dev = torch.device("cuda:0")
    sigs = [S.signal(n) for n in names]
    ns, B = [len(s) for s in sigs], len(sigs)
    wav = np.zeros((B, max(ns)), dtype=np.float32)
    for b, s in enumerate(sigs):
        wav[b, :len(s)] = s
    g, grid, max_frames, prm, lpad = FT.launch_setup(ns, wav.shape[1], sr, hop, floor, S.CEILING, S.VOICING_THRESHOLD)
    assert g["nlag"] == S.GEOMETRY_NLAG[geom]
    n_out = lpad + max_frames + 3 if n_out is None else n_out
    lib = L.load()
    win, win_r = FT._window_tables(g, dev)
    wav_d = torch.from_numpy(wav).to(dev)
    meta = torch.tensor([ns, [nf for nf, _ in grid], [lf for _, lf in grid]], dtype=torch.int32).to(dev)
    ws = torch.full((lib.ss_f0track_workspace_bytes(B, max_frames, g["nlag"]),), fill, device=dev, dtype=torch.uint8)
    guarded = torch.full((GUARD + B * n_out + GUARD,), SENTINEL, device=dev, dtype=torch.float32)
    out = guarded[GUARD:GUARD + B * n_out]
    L.check(lib.ss_f0track(L.ptr(wav_d), wav.shape[1], L.ptr(meta[0]), L.ptr(meta[1]), L.ptr(meta[2]), B, max_frames, ctypes.byref(prm), L.ptr(win),
                           L.ptr(win_r), L.ptr(out), n_out, lpad, L.ptr(ws), ws.numel(), L.stream_ptr()), "ss_f0track")
    torch.cuda.synchronize()
    host = guarded.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[-GUARD:] == SENTINEL).all(), "ss_f0track wrote outside [B, n_out]"
    res = dict(out=host[GUARD:-GUARD].reshape(B, n_out).copy(), ws=S.decode_workspace(ws.cpu().numpy(), B, max_frames, g["nlag"]),
               n_frames=[nf for nf, _ in grid], lpad=lpad, n_out=n_out, g=g)
    _runs[key] = res
    return res


ALL = list(S.INPUTS)
LIVE = [n for n in ALL if n in S.SPREAD]


@pytest.mark.parametrize("name", ALL)
def test_stats_stage_global_peak_intensity_and_silence_markers(name):
    r = run((name,))
    gpeak, intens, _ = S.stats_reference(name)
    nf = r["n_frames"][0]
    assert nf == len(intens)
    got_gp, got_it = float(r["ws"]["gpeak"][0]), r["ws"]["intensity"][0, :nf]
    assert got_gp == gpeak, (got_gp, gpeak)             # the mean's sum is exact for these inputs (asserted on the CPU): no rounding to differ in
    marker = intens <= 0.0
    assert np.array_equal(_bits(got_it[marker]), _bits(intens[marker]))   # 0.0: silent item, -1.0: silent frame
    err = np.abs(got_it[~marker] - intens[~marker]) / np.spacing(intens[~marker]) if (~marker).any() else np.zeros(1)
    record_measurement(f"f0track_stage_stats_{name}", gpeak_equal=True, intensity_worst_ulp=float(err.max()), frames=nf, silent_frames=int(marker.sum()))
    assert err.max() <= 4.0, err.max()


@pytest.mark.parametrize("name", LIVE)
def test_autocorrelation_stage_against_longdouble_direct_sums_within_the_derived_bound(name):
    """|dR[k]| <= 2 * nsamp_window * 2^-53 / window_r[k] at every lag 0 .. nlag of every live frame; R[0] == 1.0 exactly. The restatement's
    FFT route sits at ~1e-3 of this bound: a device figure near 1 deserves a look even though it passes."""
    r = run((name,))
    _, intens, frames = S.stats_reference(name)
    _, _, wr = S.tables(S.INPUTS[name])
    bound = S.r_bound(S.INPUTS[name])
    worst, worst_at = 0.0, None
    for i in np.flatnonzero(intens > 0):
        got = r["ws"]["R"][0, i]
        assert got[0] == 1.0
        ratio = np.abs(got.astype(np.longdouble) - S.autocorr_reference(frames[i], wr)).astype(np.float64) / bound
        assert np.isfinite(ratio).all()
        if ratio.max() > worst:
            worst, worst_at = float(ratio.max()), (int(i), int(ratio.argmax()))
    print(f"{name}: R worst |dR| / bound {worst:.3e} at (frame, lag) {worst_at}")
    record_measurement(f"f0track_stage_autocorr_{name}", worst_over_bound=worst, frame_lag=worst_at, nlag=len(bound) - 1, frames=int((intens > 0).sum()))
    assert worst <= 1.0, (worst, worst_at)


@pytest.mark.parametrize("name", ALL)
def test_candidate_stage_counts_and_lags_exact_frequencies_and_strengths_within_ten_spreads(name):
    """n_cand and the integer lags slot by slot EQUAL to the restatement's (they are, on every input); frequency and strength of the refined
    candidates within 10 x the restatement's own spread under the R bound.

    Measured on an MI355X: worst |df| 7.1e-13 .. 8.0e-8 Hz against bars of 1.4e-8 .. 4.9e-7 Hz (at most 0.21 of the bar: geom_sr24000), worst
    |ds| 2.9e-15 .. 5.6e-15 against bars of 2.8e-12 and up. This test found two defects the final contour had hidden: `f0t_sinc` advanced its
    angles by running sums over 70 terms (tone1500: 5.7e-6 Hz off), and the compiler's fused multiply-adds in the interpolation and in Brent's
    parabola step moved one candidate in ten by a whole termination step of the minimiser (1e-5 Hz at 220 Hz, 5.7e-2 Hz on the breathy input's
    lag-2 candidates). The file is now built without contraction."""
    r = run((name,))
    ref = S.restatement(name)
    nf = r["n_frames"][0]
    if ref is None:
        assert nf == 0
        return
    ws = r["ws"]
    df = ds = 0.0
    for i in range(nf):
        fs, ss = ref["frames"][i]
        nc = int(ws["n_cand"][0, i])
        assert nc == len(fs), (i, nc, len(fs))
        assert ws["cand_i"][0, i, :nc].tolist() == ref["lags"][i], (i, ws["cand_i"][0, i, :nc].tolist(), ref["lags"][i])
        assert ws["cand_f"][0, i, 0] == 0.0 and ws["cand_s"][0, i, 0] == 0.0
        if nc > 1:
            df = max(df, float(np.abs(ws["cand_f"][0, i, 1:nc] - np.asarray(fs[1:])).max()))
            ds = max(ds, float(np.abs(ws["cand_s"][0, i, 1:nc] - np.asarray(ss[1:])).max()))
    if name not in S.SPREAD:
        assert df == 0.0 and ds == 0.0       # no live frame: only the unvoiced candidate everywhere
        return
    bar_f, bar_s = S.candidate_bars(name)
    print(f"{name}: candidates worst |df| {df:.3e} Hz (bar {bar_f:.1e}), |ds| {ds:.3e} (bar {bar_s:.1e})")
    record_measurement(f"f0track_stage_candidates_{name}", worst_df_hz=df, bar_df_hz=bar_f, worst_ds=ds, bar_ds=bar_s, count_or_lag_mismatches=0)
    assert df <= bar_f and ds <= bar_s, (df, bar_f, ds, bar_s)


@pytest.mark.parametrize("name", ALL)
def test_viterbi_stage_alone_on_the_devices_own_candidates_is_bit_exact(name):
    """The device's cand_f / cand_s / n_cand / intensity through `praat_pitch.path_finder` on the host: with identical inputs only log2 ulps
    differ, so the device contour is float32 of the host's selection on every frame - the candidates at or above the ceiling included (the
    1500 Hz inputs have one or two per frame)."""
    r = run((name,))
    nf, lpad, ws = r["n_frames"][0], r["lpad"], r["ws"]
    want = np.zeros(r["n_out"], dtype=np.float32)
    if nf:
        frames = [(ws["cand_f"][0, i, :ws["n_cand"][0, i]].tolist(), ws["cand_s"][0, i, :ws["n_cand"][0, i]].tolist()) for i in range(nf)]
        intens = np.maximum(ws["intensity"][0, :nf], 0.0)
        gref = dict(ceiling=min(S.CEILING, 0.5 * r["g"]["sr"]), time_step=r["g"]["time_step"])
        sel = P.path_finder(frames, intens, gref, S.VOICING_THRESHOLD)
        want[lpad:lpad + nf] = sel.astype(np.float32)
        if name.startswith("tone1500"):
            assert all(max(f) >= gref["ceiling"] for f, _ in frames) and (sel < gref["ceiling"]).all() and (sel > 0).all()
    assert np.array_equal(_bits(r["out"][0]), _bits(want)), np.flatnonzero(r["out"][0] != want)


@pytest.mark.parametrize("name", ALL)
def test_end_to_end_contour_against_the_restatement(name):
    """`to_pitch_ac` of the restatement at column lpad: no voicing flip, frequency within the candidate bar + half an fp32 ulp. The other
    geometries also go through `track_f0_device(sr=, hop_size=, pitch_floor=)`, which must launch exactly this.

    Measured on an MI355X: no voicing flip on any input; worst |df| 0.13 .. 0.995 of the frame's bar, i.e. the fp32 rounding of the output
    (half an ulp is 7.6e-6 Hz at 220 Hz, 3.05e-5 Hz at 750 Hz)."""
    r = run((name,))
    ref = S.restatement(name)
    nf, lpad = r["n_frames"][0], r["lpad"]
    want = np.zeros(r["n_out"])
    if ref is not None:
        assert nf == len(ref["f0"])
        want[lpad:lpad + nf] = ref["f0"]
    got = r["out"][0].astype(np.float64)
    flips = int(((got > 0) != (want > 0)).sum())
    both = (got > 0) & (want > 0)
    over = max([0.0] + [abs(got[i] - want[i]) / S.contour_bar(name, want[i]) for i in np.flatnonzero(both)])
    worst = max([0.0] + [abs(got[i] - want[i]) for i in np.flatnonzero(both)])
    print(f"{name}: {int(both.sum())} voiced frames, flips {flips}, worst |df| {worst:.3e} Hz = {over:.3f} of its bar")
    record_measurement(f"f0track_stage_end_to_end_{name}", voiced_frames=int(both.sum()), voicing_flips=flips, worst_df_hz=worst, worst_over_bar=over)
    assert flips == 0 and over <= 1.0, (flips, worst, over)
    assert (got[:lpad] == 0).all() and (got[lpad + nf:] == 0).all()
    if name.startswith("geom_"):
        sr, hop, floor = S.GEOMETRIES[S.INPUTS[name]]
        x = torch.from_numpy(S.signal(name).copy())[None].cuda()
        same = FT.track_f0_device(x, [x.shape[1]], r["n_out"], sr=sr, hop_size=hop, pitch_floor=floor).cpu().numpy()
        assert np.array_equal(_bits(same), _bits(r["out"]))


def _assert_written_regions_equal(a, b, rows_a, rows_b, n_frames, what):
    """the regions the kernels are specified to write, bit for bit, between item rows_a of run a and rows_b of run b"""
    ma, mb = S.written_mask(a["ws"], a["n_frames"]), S.written_mask(b["ws"], b["n_frames"])
    for ia, ib, nf in zip(rows_a, rows_b, n_frames):
        for region in ("gpeak", "intensity", "n_cand", "R", "cand_f", "cand_s", "cand_i", "psi"):
            xa, xb = a["ws"][region][ia], b["ws"][region][ib]
            if region != "gpeak":
                ka, kb = ma[region][ia][:nf], mb[region][ib][:nf]
                assert np.array_equal(ka, kb), (what, region, ia)
                xa, xb = xa[:nf][ka], xb[:nf][kb]
            assert np.array_equal(_bits(np.atleast_1d(xa)), _bits(np.atleast_1d(xb))), (what, region, ia)


def test_ragged_batch_items_equal_their_own_launches_stage_by_stage():
    """B = 6 in one launch - 0, 1, 2, 33 frames, a constant item (gpeak == 0 with non-zero samples), 50 frames: each item's contour and every
    stage region equal its single-item launch bit for bit; the item without a frame comes back as an all-zero row."""
    batch = run(S.RAGGED)
    assert batch["n_frames"] == [0, 1, 2, 33, 33, 50] and batch["n_out"] == batch["lpad"] + 53
    assert not batch["out"][0].any() and not batch["out"][4].any()
    assert batch["ws"]["gpeak"][4] == 0.0 and (batch["ws"]["intensity"][4, :33] == 0.0).all() and (batch["ws"]["n_cand"][4, :33] == 1).all()
    for b, name in enumerate(S.RAGGED):
        one = run((name,), n_out=batch["n_out"])
        assert np.array_equal(_bits(batch["out"][b]), _bits(one["out"][0])), name
        _assert_written_regions_equal(batch, one, [b], [0], [batch["n_frames"][b]], name)
    assert (batch["out"][3] == 0).all() and (batch["out"][5] > 0).sum() >= 20      # the breathy item stays unvoiced, the long one is mostly voiced


def test_ragged_batch_with_a_short_output_row_is_the_head_of_the_full_one():
    """n_out = lpad + 20 < lpad + n_frames: the `lpad + i < ld_out` clamp. Equal to the first n_out columns of the full result; `run` checks
    that nothing lands outside [B, n_out] (the rows are packed, so a write past a row's end would also land in the next row)."""
    full = run(S.RAGGED)
    n_out = full["lpad"] + 20
    short = run(S.RAGGED, n_out=n_out)
    assert short["out"].shape == (6, n_out)
    assert np.array_equal(_bits(short["out"]), _bits(full["out"][:, :n_out]))
    assert (short["out"][5, full["lpad"]:] > 0).sum() >= 10


@pytest.mark.parametrize("names", [S.RAGGED, ("silent_stretch",)], ids=["ragged", "silent_stretch"])
def test_results_do_not_depend_on_what_the_workspace_held(names):
    """0xFF bytes against zeros in the workspace before the launch: the same contour, and the same bits in every region the kernels are
    specified to write. What they leave unwritten must still hold the fill - nothing else writes there, and nothing may read it."""
    a, b = run(names, fill=0xFF), run(names, fill=0x00)
    assert np.array_equal(_bits(a["out"]), _bits(b["out"]))
    B = len(names)
    _assert_written_regions_equal(a, b, range(B), range(B), a["n_frames"], "poison")
    mask = S.written_mask(a["ws"], a["n_frames"])
    for region, m in mask.items():
        assert (_bits(a["ws"][region])[~m] == np.iinfo(_bits(a["ws"][region]).dtype).max).all(), region
        assert (_bits(b["ws"][region])[~m] == 0).all(), region
