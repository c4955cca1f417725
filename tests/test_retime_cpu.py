"""Retiming the score to a sung guide, host side (no GPU): the integer definition `stylesinger_amd/pitch.py::retime_to_guide` on the case table of
tests/retime_cases.py (its properties, the identity and the integer stretch, the cases that are not retimed), the header's declaration, the
refusals of the entry, of `forward`, of the producers, the planner and the command line - all before a device is touched."""
import types

import numpy as np
import pytest

import contour_align_cases as K
import retime_cases as R
from stylesinger_amd import abi, config, lib
from stylesinger_amd import pitch as P


# ---- 1. the definition ----------------------------------------------------------------------------------------------------------------------------
def _spans(midi):
    """anchors a_0 .. a_m of a score, restated with a loop"""
    Mc = [100 * min(int(v), 127) if v > 0 else None for v in midi]
    return [0] + [i for i in range(1, len(Mc)) if Mc[i] != Mc[i - 1]] + [len(Mc)]


def _properties(mel2ph, midi, n_c, out, src, status, n_spans):
    n_t = len(mel2ph)
    a = _spans(midi)
    assert n_spans == (len(a) - 1 if n_t else 0)
    assert out.dtype == np.int64 and src.dtype == np.int32 and len(out) == len(src) >= n_c
    assert not out[n_c:].any() and (src[n_c:] == -1).all()
    if n_t == 0 or n_c == 0:
        assert status == 1 and not out.any() and (src == -1).all()
        return
    s = src[:n_c].astype(np.int64)
    assert (s >= 0).all() and (s < n_t).all() and (np.diff(s) >= 0).all(), "src is non-decreasing and inside the item"
    assert np.array_equal(out[:n_c], np.asarray(mel2ph)[s]) and (np.diff(out[:n_c]) >= 0).all() and (out[:n_c] >= 1).all()
    if status == 0:
        for k in range(len(a) - 1):                             # every span that had a score frame has a guide frame
            assert ((s >= a[k]) & (s < a[k + 1])).any(), k
    else:
        assert np.array_equal(s, P.align_band_centres(n_c, n_t)), "not retimed: the linear stretch"


@pytest.mark.parametrize("name", R.NAMES)
def test_the_case_table_has_the_properties(name):
    c, e = R.cases()[name], R.expected(name)
    assert e["status"] == R.WANT_STATUS.get(name, 0) and e["n_spans"] == R.WANT_SPANS.get(name, e["n_spans"])
    _properties(c["mel2ph"], c["midi"], len(c["guide"]), e["out"], e["src"], e["status"], e["n_spans"])
    # a wider output buffer: the same values, 0 / -1 beyond the guide
    out, src, status, m = P.retime_to_guide(c["mel2ph"], c["midi"], e["idx"], e["status_align"], len(c["guide"]), Lc=len(c["guide"]) + 3)
    assert np.array_equal(out[:-3], e["out"]) and np.array_equal(src[:-3], e["src"]) and not out[-3:].any() and (src[-3:] == -1).all()
    assert (status, m) == (e["status"], e["n_spans"])


def test_random_monotone_paths_keep_the_properties():
    """idx need not come from a DTW: any non-decreasing path into [0, n_c) - also one that crowds either end - gives a valid layout."""
    rng = np.random.default_rng(11)
    for trial in range(300):
        n_t, n_c = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        n_ph = int(rng.integers(1, 8))
        midi_ph = rng.choice([0, 60, 60, 62, 64], size=n_ph)
        mel2ph = np.sort(rng.integers(1, n_ph + 1, size=n_t))
        midi = midi_ph[mel2ph - 1]
        mode = trial % 3
        idx = np.sort(rng.integers(0, n_c, size=n_t)) if mode == 0 else np.full(n_t, n_c - 1) if mode == 1 else np.zeros(n_t, dtype=np.int64)
        out, src, status, m = P.retime_to_guide(mel2ph, midi, idx, 0, n_c)
        assert status == (1 if n_c < m else 0)
        _properties(mel2ph, midi, n_c, out, src, status, m)


def test_a_guide_that_is_the_scores_own_step_contour_changes_nothing():
    c, e = R.cases()["identity"], R.expected("identity")
    assert e["status"] == 0 and np.array_equal(e["src"], np.arange(len(c["midi"]))) and np.array_equal(e["out"], c["mel2ph"])


@pytest.mark.parametrize("f", [2, 3])
def test_every_frame_repeated_f_times_is_the_integer_stretch(f):
    mel2ph, midi = R.score(R.MELODY)
    g = np.repeat(K.note_hz(midi), f)
    _, idx, cost, st = P.contour_align(g, midi)
    out, src, status, m = P.retime_to_guide(mel2ph, midi, idx, st, len(g))
    assert cost == 0 and status == 0 and m == 5
    assert np.array_equal(src, np.arange(len(g)) // f) and np.array_equal(out, np.repeat(mel2ph, f))


def test_per_note_stretches_with_detuning_put_the_anchors_on_the_true_note_starts():
    """Stretches of 1x to 3x per note and +-20 cents of noise: every guide frame gets a phone of the note the guide sings there."""
    rng = np.random.default_rng(2)
    mel2ph, midi = R.score(R.MELODY)
    notes = [60, 0, 62, 64, 65]
    score_frames = [7, 3, 9, 6, 4]
    for _ in range(20):
        sung = [int(round(f * rng.uniform(1.0, 3.0))) for f in score_frames]
        cents = np.repeat(np.asarray(notes) * 100, sung) + rng.integers(-20, 21, size=sum(sung))
        g = np.where(np.repeat(notes, sung) > 0, K.cents_to_hz(cents), np.float32(0)).astype(np.float32)
        _, idx, _, st = P.contour_align(g, midi)
        out, src, status, m = P.retime_to_guide(mel2ph, midi, idx, st, len(g))
        assert status == 0 and np.array_equal(midi[src], np.repeat(notes, sung))
        starts = np.concatenate([[0], np.cumsum(sung)[:-1]])
        assert np.array_equal(src[starts], np.concatenate([[0], np.cumsum(score_frames)[:-1]])), "a note's first guide frame takes its first score frame"


def test_a_note_the_guide_leaves_out_keeps_a_frame_and_crowded_ends_stay_inside():
    for name in ("guide_skips_a_note", "guide_skips_the_last_notes", "guide_skips_the_first_notes", "n_c_equals_m"):
        c, e = R.cases()[name], R.expected(name)
        assert e["status"] == 0 and set(c["midi"][e["src"]]) == {60, 62, 64, 65}, name
    e = R.expected("n_c_equals_m")
    assert np.array_equal(e["src"], [1, 4, 7, 10])              # one guide frame per note: the centre of its three score frames
    # phones inside a note keep their proportions: the note 62 of MELODY has phones of 5 and 4 frames, sung over 20 guide frames
    e, c = R.expected("melody"), R.cases()["melody"]
    n4, n5 = int((e["out"] == 4).sum()), int((e["out"] == 5).sum())
    assert n4 + n5 == 20 and abs(n4 - 20 * 5 / 9) <= 1


def test_not_retimed_is_the_linear_stretch_and_the_alignment_function_is_untouched():
    c, e = R.cases()["alignment_refused"], R.expected("alignment_refused")
    assert e["status_align"] == 1 and (e["idx"] == -1).all() and e["status"] == 1
    assert np.array_equal(e["src"], ((2 * np.arange(50) + 1) * 3) // (2 * 50))
    e = R.expected("n_c_equals_m_minus_1")
    assert e["status_align"] == 0 and e["status"] == 1 and np.array_equal(e["src"], [2, 6, 10])


# ---- 2. plumbing ----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_abi_version_stays():
    assert "ss_retime_mel2ph" in lib.declared_symbols()
    assert abi.DEFINES["SS_ABI_VERSION"] == 20
    proto = abi.PROTOTYPES["ss_retime_mel2ph"]
    assert proto.launch and len(proto.params) == 17
    assert [p.pointee for p in proto.params[:2]] == ["int64_t", None] and proto.params[8].pointee == "int64_t" and proto.params[10].pointee == "int32_t"
    assert (2 * P.ALIGN_MAX_LC + 1) * P.ALIGN_MAX_T < 2 ** 31 and max(P.ALIGN_MAX_T, P.ALIGN_MAX_LC) < 2 ** 16   # int32 map, uint16 LDS entries


def test_entry_refuses_bad_arguments_before_any_launch():
    l = lib.load()
    assert l.ss_abi_version() == 20, "the export is additive"
    p = 4096     # any non-null address: every call below is refused before it is used
    ok = dict(mel2ph=p, ldm=8, midi=p, ldn=8, idx=p, sa=p, lt=p, lc=p, out=2 * p, ldo=8, src=p, st=p, ns=p, T=8, Lc=8, B=1)

    def call(**kw):
        a = dict(ok, **kw)
        return l.ss_retime_mel2ph(a["mel2ph"], a["ldm"], a["midi"], a["ldn"], a["idx"], a["sa"], a["lt"], a["lc"], a["out"], a["ldo"], a["src"], a["st"],
                                  a["ns"], a["T"], a["Lc"], a["B"], None)
    for kw, word in ((dict(mel2ph=None), b"null pointer"), (dict(idx=None), b"null pointer"), (dict(sa=None), b"null pointer"), (dict(lc=None), b"null pointer"),
                     (dict(ns=None), b"null pointer"), (dict(B=0), b"bad dims"), (dict(B=65536), b"bad dims"), (dict(T=0), b"bad dims"),
                     (dict(ldm=4), b"bad dims"), (dict(ldn=4), b"bad dims"), (dict(ldo=4), b"bad dims"), (dict(out=p), b"alias"),
                     (dict(T=P.ALIGN_MAX_T + 1, ldm=P.ALIGN_MAX_T + 1, ldn=P.ALIGN_MAX_T + 1), b"caps"),
                     (dict(Lc=P.ALIGN_MAX_LC + 1, ldo=P.ALIGN_MAX_LC + 1), b"caps")):
        assert call(**kw) != 0, kw
        err = l.ss_last_error()
        assert b"ss_retime_mel2ph" in err and word in err, (kw, err)


def test_device_wrapper_refuses_host_tensors():
    import torch
    z = torch.zeros(1, 8, dtype=torch.long)
    with pytest.raises(lib.StyleSingerHipError, match="device tensors"):
        P.retime_device(z, torch.tensor([8], dtype=torch.int32), z, z.int(), torch.zeros(1, dtype=torch.int32), [8], 8)


def test_forward_argument_checks_fire_before_any_device_work():
    """A model built on the CPU (no device, no packed weights): the refusals come from the argument checks at the top of forward."""
    import torch
    from stylesinger_amd.model import StyleSingerHIP
    m = StyleSingerHIP(None, hparams=config.make_hparams(dict(timesteps=2, K_step=2, f0_timesteps=2)))
    m.eval()
    txt = torch.ones(1, 3, dtype=torch.long)
    f0, uv, hz = torch.full((1, 8), 8.0), torch.zeros(1, 8), torch.full((1, 8), 220.0)
    for kw, word in ((dict(pitch_timing="score", pitch_hz=(hz, [8])), "'guide'"), (dict(pitch_timing=True, pitch_hz=(hz, [8])), "'guide'"),
                     (dict(pitch_timing="guide"), "needs pitch_hz"), (dict(pitch_timing="guide", f0=f0, uv=uv), "needs pitch_hz.*f0 / uv"),
                     (dict(pitch_timing="guide", pitch_hz=(hz, [8]), f0=f0, uv=uv), "not both"),
                     (dict(pitch_timing="guide", pitch_hz=(hz, [8]), f0_steps=2), "f0_steps"),
                     (dict(pitch_timing="guide", pitch_hz=(hz, [8]), pitch_align="linear"), "'dtw'"),
                     (dict(pitch_timing="guide", pitch_hz=(hz, [8]), pitch_align_band=-1), ">= 0"),
                     (dict(pitch_hz=(hz, [8]), pitch_align_band=4), "needs pitch_align")):          # without pitch_timing: as before
        with pytest.raises(ValueError, match=word):
            m(txt, infer=True, **kw)


def test_align_inputs_and_pitch_inputs_carry_pitch_timing():
    import torch
    from stylesinger_amd import producers
    f = producers.align_inputs
    assert f({"pitch_timing": "guide"}, True, 48000, 256) == dict(pitch_timing="guide", pitch_align_band=375)      # the 2.0 s default band
    assert f({"pitch_timing": "guide", "pitch_align_band_s": 0.5}, True, 24000, 128) == dict(pitch_timing="guide", pitch_align_band=94)
    assert f({"pitch_timing": "guide", "pitch_align": "dtw", "pitch_align_band_s": 0}, True, 48000, 256) == dict(pitch_timing="guide", pitch_align="dtw",
                                                                                                              pitch_align_band=0)
    assert f({"pitch_align": "dtw"}, True, 48000, 256) == dict(pitch_align="dtw", pitch_align_band=375)            # without the key: as before
    for inp, has, word in (({"pitch_timing": "guide"}, False, "needs one of them"), ({"pitch_timing": "score"}, True, "'guide'"),
                           ({"pitch_timing": "guide", "pitch_align": "linear"}, True, "'dtw'"),
                           ({"pitch_timing": "guide", "pitch_align_band_s": -1}, True, ">= 0")):
        with pytest.raises(ValueError, match=word):
            f(inp, has, 48000, 256)
    me = types.SimpleNamespace(hparams=dict(audio_sample_rate=48000, hop_size=256), device=torch.device("cpu"))
    out = producers.ReferenceProducers._pitch_inputs(me, {"pitch_hz": np.full(9, 220.0), "pitch_timing": "guide", "pitch_shift": -1})
    assert out["pitch_timing"] == "guide" and out["pitch_align_band"] == 375 and "pitch_align" not in out and out["pitch_shift"] == -1.0
    assert "pitch_timing" not in producers.ReferenceProducers._pitch_inputs(me, {"pitch_hz": np.full(9, 220.0), "pitch_align": "dtw"})


def test_plan_song_copies_pitch_timing_into_every_segment_batch_and_needs_ph_dur():
    from stylesinger_amd import controls, song
    assert "pitch_timing" in controls.CONTOUR_KEYS
    n = 8
    inp = dict(ph_token=list(range(1, n + 1)), note=[60, 62, 0, 64, 65, 0, 67, 69], note_dur=[0.3] * n, note_type=[2, 2, 1, 2, 2, 1, 2, 2],
               ph_dur=[0.3] * n, pitch_hz=np.full(100, 220.0), pitch_timing="guide")
    plan = song.plan_song(inp, sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    plain = song.plan_song({k: v for k, v in inp.items() if k != "pitch_timing"}, sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    assert len(plan.batches) >= 2
    for b, q in zip(plan.batches, plain.batches):
        assert b["pitch_timing"] == "guide" and b["pitch_align_band"] == 375 and "pitch_align" not in b and "pitch_timing" not in q
        assert b["pitch_hz"][1] == q["pitch_hz"][1] and b["pitch_hz"][0].shape == b["mel2ph"].shape       # a slice per segment, of its own frame count
    assert [(g["start_frame"], g["n_frames"]) for g in plan.segments] == [(g["start_frame"], g["n_frames"]) for g in plain.segments]
    with pytest.raises(ValueError, match="ph_dur"):
        song.plan_song({k: v for k, v in inp.items() if k != "ph_dur"})
    with pytest.raises(ValueError, match="needs one of them"):
        song.plan_song({k: v for k, v in inp.items() if k != "pitch_hz"})


def test_cli_carries_pitch_timing_and_refuses_it_without_a_contour(capsys, monkeypatch, tmp_path):
    from stylesinger_amd import infer
    base = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"]
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: pytest.fail("a checkpoint was loaded before the flags were checked"))
    for extra, word in ((["--pitch-timing", "guide"], "--pitch-timing needs"), (["--pitch-timing", "score", "--pitch-npy", "c.npy"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            infer.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err
    seen = {}
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(infer.StyleSingerInfer, "example_run", classmethod(lambda cls, hparams=None, *a, pitch=None, **k: seen.update(pitch=pitch)))
    np.save(tmp_path / "c.npy", np.full(10, 220.0))
    infer.main(base + ["--pitch-npy", str(tmp_path / "c.npy"), "--pitch-timing", "guide", "--pitch-align-band-s", "1.5"])
    assert seen["pitch"]["pitch_timing"] == "guide" and seen["pitch"]["pitch_align_band_s"] == 1.5 and "pitch_align" not in seen["pitch"]
