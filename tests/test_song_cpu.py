"""Singing a whole score, host side (no GPU): the planner of stylesinger_amd/song.py (phrase split at rests, greedy merge, the global frame grid
with ph_dur, contour slices, batches), the numpy restatement of the two kernels (tests/song_ref.py), the two exports and their argument checks,
and the command line's usage errors."""
import json
import os
import warnings

import numpy as np
import pytest

import song_ref as R
from stylesinger_amd import lib, song

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR, HOP = 48000, 256


def _example():
    with open(os.path.join(ROOT, "stylesinger_amd", "example_input.json")) as fh:
        inp = {k: v for k, v in json.load(fh).items() if k != "source"}
    inp["ph_token"] = [3 + (7 * i) % 50 for i in range(len(inp["ph"]))]
    return inp


def _score(note, note_type=None, note_dur=None, **kw):
    P = len(note)
    note_type = [1 if n == 0 else 2 for n in note] if note_type is None else note_type
    return dict(ph_token=list(range(3, 3 + P)), note=list(note), note_dur=[0.5] * P if note_dur is None else list(note_dur), note_type=list(note_type), **kw)


def _ranges(plan):
    return [(g["first"], g["last"]) for g in plan.segments]


def _estimate(inp, first, last):
    """the definition, restated: a phone counts when it starts the range or its (note, note_dur, note_type) differs from the phone before it"""
    key = list(zip(inp["note"], inp["note_dur"], inp["note_type"]))
    return sum(inp["note_dur"][i] for i in range(first, last) if i == first or key[i] != key[i - 1])


def _plan_quiet(*a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        return song.plan_song(*a, **kw)


# ---- planner: the shipped example score -----------------------------------------------------------------------------------------------------
def test_example_score_minimal_phrases_and_their_estimated_seconds():
    inp = _example()
    assert song.minimal_phrases(inp["note"], inp["note_type"]) == [(0, 13), (13, 24), (24, 31)]
    secs = [song.range_seconds(a, b, inp["note"], inp["note_dur"], inp["note_type"]) for a, b in ((0, 13), (13, 24), (24, 31))]
    want = [_estimate(inp, a, b) for a, b in ((0, 13), (13, 24), (24, 31))]
    assert np.allclose(secs, want, rtol=1e-12, atol=0)
    assert np.allclose(secs, [4.02, 3.18, 2.39], atol=0.01)
    # consecutive phones that share a note count once: the first phrase is far shorter than the sum of its note_dur entries
    assert sum(inp["note_dur"][:13]) > 6.5 > secs[0]


@pytest.mark.parametrize("max_seconds,want", [(12.0, [(0, 31)]), (6.0, [(0, 13), (13, 31)]), (5.0, [(0, 13), (13, 24), (24, 31)])])
def test_example_score_merges_greedily(max_seconds, want):
    plan = _plan_quiet(_example(), SR, HOP, max_seconds=max_seconds)
    assert _ranges(plan) == want
    assert all(g["n_frames"] is None and g["start_frame"] is None for g in plan.segments) and plan.n_frames is None
    assert "mel2ph" not in plan.batches[0]           # left to the duration predictor
    for g in plan.segments:
        assert g["seconds"] == pytest.approx(_estimate(_example(), g["first"], g["last"]), rel=1e-12)
        assert g["seconds"] <= max_seconds


def test_a_phrase_longer_than_the_limit_stays_whole_with_one_warning_each():
    with pytest.warns(UserWarning) as rec:
        plan = song.plan_song(_example(), SR, HOP, max_seconds=1.0)
    assert _ranges(plan) == [(0, 13), (13, 24), (24, 31)]
    msgs = [str(w.message) for w in rec]
    assert len(msgs) == 3
    for m, (a, b) in zip(msgs, _ranges(plan)):
        assert f"[{a}, {b})" in m


# ---- planner: other scores ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,note,note_type,want", [
    ("leading rests open the first phrase", [0, 0, 60, 62, 0, 64], None, [(0, 5), (5, 6)]),
    ("a run of rests closes one phrase", [60, 0, 0, 0, 62, 0, 0, 64, 65], None, [(0, 4), (4, 7), (7, 9)]),
    ("no rest at all", [60, 62, 64, 65], None, [(0, 4)]),
    ("all rests", [0, 0, 0], None, [(0, 3)]),
    ("a rest by note_type alone", [60, 61, 62, 63], [2, 1, 2, 2], [(0, 2), (2, 4)]),
    ("a rest by note alone", [60, 0, 62], [2, 2, 2], [(0, 2), (2, 3)]),
])
def test_minimal_phrases_of_other_scores_tile_the_phones(name, note, note_type, want):
    sc = _score(note, note_type)
    assert song.minimal_phrases(sc["note"], sc["note_type"]) == want, name
    for max_seconds in (0.1, 1.0, 2.0, 100.0):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plan = song.plan_song(sc, SR, HOP, max_seconds=max_seconds, segment_batch=2)
        r = _ranges(plan)
        assert r[0][0] == 0 and r[-1][1] == len(note) and all(r[i][1] == r[i + 1][0] for i in range(len(r) - 1)) and all(a < b for a, b in r)
        assert set(r) <= {(a, b) for a in [w[0] for w in want] for b in [w[1] for w in want]}, "a cut inside a minimal phrase"
        # every segment is a row of exactly one batch, and the rows carry the segment's phones
        seen = sorted(s for rows in plan.rows for s in rows)
        assert seen == list(range(len(r))) and all(len(rows) <= 2 for rows in plan.rows)
        for g in plan.segments:
            b = plan.batches[g["batch"]]
            n = g["last"] - g["first"]
            assert plan.rows[g["batch"]][g["row"]] == g["index"]
            assert b["txt_tokens"][g["row"], :n].tolist() == sc["ph_token"][g["first"]:g["last"]] and (b["txt_tokens"][g["row"], n:] == 0).all()
            assert b["note"][g["row"], :n].tolist() == sc["note"][g["first"]:g["last"]]


def test_batches_are_ordered_by_size_descending_with_ties_in_song_order():
    # phrases of 2, 4, 2, 3, 4 phones, each closed by a rest
    note = [60, 0, 60, 61, 62, 0, 60, 0, 60, 61, 0, 60, 61, 62, 0]
    plan = _plan_quiet(_score(note), SR, HOP, max_seconds=0.6 * 4, segment_batch=2)
    assert [g["last"] - g["first"] for g in plan.segments] == [2, 4, 2, 3, 4]
    assert plan.rows == [[1, 4], [3, 0], [2]]
    ph_dur = [0.1] * len(note)
    ph_dur[11] = 0.12                                      # with ph_dur the order is by frames: the last phrase is now the longest
    plan = _plan_quiet(_score(note, ph_dur=ph_dur), SR, HOP, max_seconds=0.45, segment_batch=2)
    assert plan.rows == [[4, 1], [3, 0], [2]]


# ---- planner: with ph_dur -------------------------------------------------------------------------------------------------------------------
def _timed_score(pitch=False):
    rng = np.random.default_rng(3)
    note = [60, 62, 0, 64, 65, 66, 0, 0, 67, 0, 69, 70, 0]
    ph_dur = rng.uniform(0.03, 0.3, len(note))
    ph_dur[4] = 0.0                                        # a phone without a frame
    ph_dur[10] = 0.0011                                    # shorter than half a hop: no frame either, or one, as the rounding falls
    sc = _score(note, ph_dur=ph_dur.tolist())
    if pitch:
        n = 517
        hz = 220.0 + 60.0 * np.sin(np.arange(n) / 9.0)
        hz[40:55] = 0
        sc["pitch_hz"] = hz
    return sc


def test_ph_dur_grid_is_global():
    sc = _timed_score()
    total = int(np.floor(np.sum(np.asarray(sc["ph_dur"], dtype=np.float64)) * SR / HOP + 0.5))
    bounds = song.frame_bounds(sc["ph_dur"], SR, HOP)
    assert bounds[0] == 0 and bounds[-1] == total and (np.diff(bounds) >= 0).all() and bounds[5] == bounds[4], "the zero-length phone owns no frame"
    grid = np.repeat(np.arange(1, len(sc["note"]) + 1), np.diff(bounds))      # global mel2ph, 1-based
    for max_seconds in (0.3, 0.7, 100.0):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            plan = song.plan_song(sc, SR, HOP, max_seconds=max_seconds, segment_batch=2)
        assert plan.n_frames == total and sum(g["n_frames"] for g in plan.segments) == total
        parts = []
        for g in plan.segments:
            m = plan.batches[g["batch"]]["mel2ph"][g["row"]].numpy()
            assert (m[g["n_frames"]:] == 0).all() and (m[:g["n_frames"]] > 0).all()
            parts.append(m[:g["n_frames"]] + g["first"])
            assert g["start_frame"] == bounds[g["first"]], "every segment starts on its score time"
            assert g["seconds"] == pytest.approx(float(np.sum(sc["ph_dur"][g["first"]:g["last"]])), rel=1e-12)
        assert np.array_equal(np.concatenate(parts), grid)
    seg = next(g for g in plan.segments if g["first"] <= 4 < g["last"])
    m = plan.batches[seg["batch"]]["mel2ph"][seg["row"]].numpy()
    assert (4 - seg["first"] + 1) not in m and (5 - seg["first"] + 1) in m, "the zero-frame phone survives: it keeps its index, its neighbours theirs"


def test_contour_is_fitted_once_and_its_slices_tile_it():
    from stylesinger_amd.pitch import contour_fit
    sc = _timed_score(pitch=True)
    sc["pitch_shift"] = -2.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plan = song.plan_song(sc, SR, HOP, max_seconds=0.7, segment_batch=2)
    assert len(plan.segments) >= 3
    fitted = contour_fit(sc["pitch_hz"], plan.n_frames).astype(np.float32)
    assert np.array_equal(plan.pitch_hz, fitted) and (fitted == 0).any() and (fitted > 0).any()
    parts = []
    for g in plan.segments:
        b = plan.batches[g["batch"]]
        hz, lens = b["pitch_hz"]
        assert lens[g["row"]] == g["n_frames"] and b["pitch_shift"] == -2.0 and hz.shape == b["mel2ph"].shape
        assert (hz[g["row"], g["n_frames"]:] == 0).all()
        parts.append(hz[g["row"], :g["n_frames"]].numpy())
    assert np.array_equal(np.concatenate(parts), fitted)


@pytest.mark.parametrize("key,value", [("pitch_hz", np.full(50, 220.0)), ("pitch_audio", "guide.wav"), ("pitch_shift", 2.0)])
def test_pitch_keys_without_ph_dur_are_refused_with_the_reason(key, value):
    sc = _example()
    sc[key] = value
    with pytest.raises(ValueError, match=r"(?s)ph_dur.*frame counts are not known before rendering"):
        song.plan_song(sc, SR, HOP)


def test_planner_refusals():
    with pytest.raises(ValueError, match="ph_token"):
        song.plan_song({k: v for k, v in _example().items() if k != "ph_token"}, SR, HOP)
    with pytest.raises(ValueError, match="ph_dur entries"):
        song.plan_song(dict(_example(), ph_dur=[0.1] * 5), SR, HOP)
    with pytest.raises(ValueError, match="non-negative"):
        song.plan_song(_score([60, 0], ph_dur=[0.1, -0.1]), SR, HOP)
    with pytest.raises(ValueError, match="pitch_shift"):
        song.plan_song(_score([60, 0], ph_dur=[0.1, 0.1], pitch_shift=2.0), SR, HOP)
    with pytest.raises(ValueError, match="no frame"):
        song.plan_song(_score([60, 0, 61, 0], ph_dur=[0.2, 0.1, 0.0, 0.0]), SR, HOP, max_seconds=0.3)

    class Enc:
        def encode(self, s):
            return [5 + len(p) for p in s.split(" ")]
    plan = _plan_quiet({k: v for k, v in _example().items() if k != "ph_token"}, SR, HOP, ph_encoder=Enc())
    assert plan.batches[0]["txt_tokens"][0].tolist() == [5 + len(p) for p in _example()["ph"]]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def test_restatement_without_fade_is_concatenate():
    rng = np.random.default_rng(0)
    lens = np.array([3, 0, 1, 7, 2])
    for unit in (1, 80, 64):
        rows = [rng.standard_normal((n, unit)).astype(np.float32) for n in lens]
        T = 9
        src = np.full((5, T * unit), np.nan, np.float32)
        order = [3, 0, 4, 1, 2]
        for r, s in enumerate(order):
            src[r, :lens[s] * unit] = rows[s].ravel()
        off = R.offsets_ref(lens)
        assert off.tolist() == [0, 3, 3, 4, 11, 13]
        out = np.full(13 * unit + 5, np.nan, np.float32)
        assert R.place_ref(src, np.array(order), lens, off, unit, out) == 0
        assert np.array_equal(out[:13 * unit], np.concatenate([r.ravel() for r in rows])) and np.isnan(out[13 * unit:]).all()
    assert R.offsets_ref([2, -5, 3]).tolist() == [0, 2, 2, 5]


def test_restatement_fades_both_sides_of_every_joint_and_not_the_songs_ends():
    lens, unit, fade = np.array([3, 1, 2]), 64, 48
    win = R.fade_window(fade)
    assert np.array_equal(win, song.fade_window(fade)) and win.dtype == np.float32
    assert np.allclose(win.astype(np.float64) + win[::-1], 1.0, atol=1e-7) and (np.diff(win) > 0).all() and 0 < win[0] < win[-1] < 1
    src = np.ones((3, 3 * unit), np.float32)
    out = np.full(6 * unit, np.nan, np.float32)
    assert R.place_ref(src, np.array([0, 1, 2]), lens, R.offsets_ref(lens), unit, out, win) == 0
    a, b, c = out[:192], out[192:256], out[256:]
    assert (a[:144] == 1).all() and np.array_equal(a[144:], win[::-1])                  # the first segment: no fade in, a full fade out
    f = 32                                                                              # the 1-frame segment: f = min(48, 64 // 2)
    g = np.array([win[((2 * k + 1) * fade) // (2 * f)] for k in range(f)], np.float32)
    assert np.array_equal(b[:f], g) and np.array_equal(b[f:], g[::-1])
    assert np.array_equal(c[:48], win) and (c[48:] == 1).all()                          # the last segment: a full fade in, no fade out


def test_gain_index_is_k_at_full_length_and_stays_inside_the_table():
    for fade in (1, 2, 5, 48, 240):
        assert [R.gain_index(k, fade, fade) for k in range(fade)] == list(range(fade))
        for f in range(1, fade + 1):
            idx = [R.gain_index(k, f, fade) for k in range(f)]
            assert 0 <= min(idx) and max(idx) < fade and idx == sorted(idx)


def test_restatement_clamps_and_flags():
    lens, unit = np.array([2, 3]), 4
    src = np.arange(2 * 8, dtype=np.float32).reshape(2, 8)                              # lds = 8 floats: the 3-frame segment does not fit
    out = np.full(20, np.nan, np.float32)
    assert R.place_ref(src, np.array([0, 1]), lens, R.offsets_ref(lens), unit, out) == R.FLAG_READ
    assert np.array_equal(out[:16], src.ravel()) and np.isnan(out[16:]).all()
    out = np.full(20, np.nan, np.float32)
    assert R.place_ref(src, np.array([0, 1]), lens, R.offsets_ref(lens), unit, out, cap=14) == R.FLAG_READ | R.FLAG_WRITE
    assert np.array_equal(out[:14], src.ravel()[:14]) and np.isnan(out[14:]).all()
    assert R.place_ref(src, np.array([0, 2]), lens, R.offsets_ref(lens), unit, out) == R.FLAG_INDEX
    assert (R.FLAG_READ, R.FLAG_WRITE, R.FLAG_INDEX) == (song.FLAG_READ, song.FLAG_WRITE, song.FLAG_INDEX)


# ---- library and command line ---------------------------------------------------------------------------------------------------------------
def test_exports_are_declared_and_refuse_bad_arguments_before_a_device_is_touched():
    l = lib.load()
    names = lib.declared_symbols()
    assert "ss_song_offsets" in names and "ss_song_place" in names and hasattr(l, "ss_song_offsets") and hasattr(l, "ss_song_place")
    p = 0x1000   # placeholder non-null pointers: every refusal below comes before anything is dereferenced or launched
    assert l.ss_song_offsets(p, -1, p, None) != 0 and b"ss_song_offsets: S=-1" in l.ss_last_error()
    assert l.ss_song_offsets(p, 4, None, None) != 0 and b"ss_song_offsets: null pointer" in l.ss_last_error()
    assert l.ss_song_offsets(None, 4, p, None) != 0 and b"null pointer" in l.ss_last_error()
    ok = dict(src=p, lds=64, seg=p, B=2, lens=p, offsets=p, S=3, unit=4, win=None, fade=0, out=2 * p, cap=256, flags=None, stream=None)
    call = lambda **kw: l.ss_song_place(*{**ok, **kw}.values())
    assert call(S=-1) != 0 and b"bad dims" in l.ss_last_error()
    assert call(B=0) != 0 and b"bad dims" in l.ss_last_error()
    assert call(unit=0) != 0 and b"unit=0" in l.ss_last_error()
    assert call(unit=-3) != 0 and b"unit=-3" in l.ss_last_error()
    assert call(fade=8) != 0 and b"without a window table" in l.ss_last_error()
    assert call(fade=-1) != 0 and b"fade=-1" in l.ss_last_error()
    assert call(out=None) != 0 and b"ss_song_place: null pointer" in l.ss_last_error()
    assert call(src=None) != 0 and b"null pointer" in l.ss_last_error()
    assert call(lds=0) != 0 and b"bad sizes" in l.ss_last_error()
    assert call(cap=-1) != 0 and b"bad sizes" in l.ss_last_error()
    assert call(out=p) != 0 and b"alias" in l.ss_last_error()
    assert l.ss_abi_version() == 20, "the exports are additive"


def test_score_with_a_pitch_flag_and_no_ph_dur_is_a_usage_error(tmp_path, capsys):
    from stylesinger_amd import infer
    path = tmp_path / "song.json"
    path.write_text(json.dumps({k: v for k, v in _example().items() if k != "ph_token"}))
    base = ["--exp-dir", "x", "--vocoder-dir", "x", "--emotion-ckpt", "x", "--speaker-ckpt", "x", "--phone-set", "x", "--score", str(path)]
    for extra in (["--pitch-npy", "c.npy", "--pitch-shift", "2"], ["--pitch-audio", "guide.wav"]):
        if extra[0] == "--pitch-npy":
            np.save(tmp_path / "c.npy", np.full(10, 220.0))
            extra[1] = str(tmp_path / "c.npy")
        with pytest.raises(SystemExit) as e:
            infer.main(base + extra)
        assert e.value.code == 2 and "ph_dur" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        infer.main(base[:-2] + ["--segments-out", "t.json"])
    assert e.value.code == 2 and "--score" in capsys.readouterr().err
