"""Singing a whole score on the GPU: the two kernels of csrc/song.hip bit-equal to their host restatement (tests/song_ref.py), and
`StyleSingerInfer.sing_score` bit-equal to that restatement applied to `infer_batch` of the plan's own batches - with a song-level pitch contour,
with three batches in flight, for a single-segment score against the plain `infer_batch` of that item, and with a loudness target on the whole song.
The model is the tiny synthetic one (3 sampler steps); the reference's features travel inside `inp`, so no emotion or speaker encoder is needed."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import song_ref as R  # noqa: E402
from stylesinger_amd import config, song, synth  # noqa: E402

DEV = torch.device("cuda:0")
SEED = 31
NAN = float("nan")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------------------
def test_offsets_scan_beyond_one_workgroup():
    rng = np.random.default_rng(0)
    lens = rng.integers(0, 4, 300).astype(np.int32)          # 300 entries: a second chunk of the 256-thread workgroup, carried total
    got = song.song_offsets(torch.from_numpy(lens).to(DEV)).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, R.offsets_ref(lens)) and got[-1] == lens.sum() and (lens == 0).any() and (lens == 3).any()
    assert song.song_offsets(torch.zeros(0, dtype=torch.int32, device=DEV)).cpu().tolist() == [0]
    assert song.song_offsets(torch.tensor([2, -5, 3], dtype=torch.int32, device=DEV)).cpu().tolist() == [0, 2, 2, 5]      # a negative length counts as 0


LENS = [3, 0, 1, 7, 2]


@pytest.mark.parametrize("lens,unit,fade,misalign", [
    (LENS, 64, 48, False),                  # the 1-frame segment takes f = 32; 16-byte accesses
    (LENS, 80, 0, False),                   # the mel
    (LENS, 1, 0, False),                    # the f0: one float per access
    (LENS, 256, 240, False),                # the 7-frame segment (1792 floats) spans two workgroups of the 16-byte form
    (LENS, 64, 48, True),                   # a source that is not 16-byte aligned: the one-float form with a fade
    ([500, 0, 1, 700, 2], 3, 48, False),    # unit % 4 != 0: the one-float form over three workgroups; the 1-frame segment takes f = 1
])
def test_place_is_bit_equal_to_the_restatement(lens, unit, fade, misalign):
    rng = np.random.default_rng(unit + fade)
    lens = np.asarray(lens, dtype=np.int32)
    S, T = len(lens), int(max(lens)) + 2                    # lds wider than any row
    total = int(lens.sum())
    segs = [np.array([3, -1, 0], np.int32), np.array([4, 2, 1], np.int32)]      # two sources, out of song order, one skipped row
    srcs = []
    for seg in segs:
        a = np.full((len(seg), T * unit), NAN, np.float32)
        for r, s in enumerate(seg):
            n = (lens[s] if s >= 0 else 2) * unit
            a[r, :n] = rng.standard_normal(n).astype(np.float32)
        srcs.append(a)
    cap = (total + 2) * unit
    want = np.full(cap, NAN, np.float32)
    off = R.offsets_ref(lens)
    win = R.fade_window(fade) if fade else None
    for a, seg in zip(srcs, segs):
        assert R.place_ref(a, seg, lens, off, unit, want, win) == 0
    lens_d = torch.from_numpy(lens).to(DEV)
    off_d = song.song_offsets(lens_d)
    out = torch.full((cap,), NAN, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    win_d = None if win is None else torch.from_numpy(win).to(DEV)
    for a, seg in zip(srcs, segs):
        if misalign:
            buf = torch.empty(a.size + 1, device=DEV)
            src = buf[1:].view(a.shape)
            src.copy_(torch.from_numpy(a))
            assert src.data_ptr() % 16 == 4
        else:
            src = torch.from_numpy(a).to(DEV)
        song.song_place(src, torch.from_numpy(seg).to(DEV), lens_d, off_d, unit, out, win=win_d, flags=flags)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isfinite(got[:total * unit]).all() and np.isnan(got[total * unit:]).all()
    assert flags.item() == 0


def test_place_clamps_reads_and_writes_and_says_so():
    lens, unit, T = np.array([3, 5, 2], np.int32), 64, 4      # the 5-frame segment is longer than a source row (lds = 4 frames)
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, T * unit)).astype(np.float32)
    seg = np.array([1, 2, 0], np.int32)
    off = R.offsets_ref(lens)
    cap = (int(lens.sum()) - 1) * unit                       # one frame short: the last segment loses its second frame
    win = R.fade_window(48)
    want = np.full(cap + 3 * unit, NAN, np.float32)
    assert R.place_ref(a, seg, lens, off, unit, want, win, cap=cap) == R.FLAG_READ | R.FLAG_WRITE
    lens_d = torch.from_numpy(lens).to(DEV)
    out = torch.full((cap + 3 * unit,), NAN, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    song.song_place(torch.from_numpy(a).to(DEV), torch.from_numpy(seg).to(DEV), lens_d, song.song_offsets(lens_d), unit, out,
                    win=torch.from_numpy(win).to(DEV), flags=flags, cap=cap)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert flags.item() == song.FLAG_READ | song.FLAG_WRITE == 3
    assert np.isnan(got[cap:]).all(), "nothing is written past cap"
    assert np.array_equal(_bits(got), _bits(want))
    assert np.isnan(got[(3 + 4) * unit:(3 + 5) * unit]).all() and np.isfinite(got[:(3 + 4) * unit]).all()   # the frame that could not be read
    # a song index past S is refused, flagged, and the other rows are placed
    out.fill_(NAN)
    flags.zero_()
    song.song_place(torch.from_numpy(a).to(DEV), torch.tensor([0, 3, -1], dtype=torch.int32, device=DEV), lens_d, song.song_offsets(lens_d), unit, out,
                    flags=flags)
    torch.cuda.synchronize()
    assert flags.item() == song.FLAG_INDEX and torch.equal(out[:3 * unit].cpu(), torch.from_numpy(a[0, :3 * unit])) and torch.isnan(out[3 * unit:]).all()


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------------------
PHRASES = (5, 3, 6, 2, 4)                 # phones per minimal phrase, the closing rest included
FRAMES = (40, 22, 51, 9, 30)              # about this many frames each


@pytest.fixture(scope="module")
def singer():
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    inf = StyleSingerInfer(hp, device=DEV, model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 11))
    inf.model.use_graphs = "off"
    ref = synth.synth_utterance(0, 8, 4, 50, hp, 5)
    feats = dict(mel=ref["ref_mels"].numpy(), f0=np.exp2(ref["ref_f0"].numpy().astype(np.float64)), spk_embed=ref["spk_embed"].numpy(),
                 emo_embed=ref["emo_embed"].numpy())
    return inf, feats


def _score(feats):
    """five minimal phrases of 5, 3, 6, 2, 4 phones, each closed by one rest; ph_dur so that they take about 40, 22, 51, 9, 30 frames"""
    rng = np.random.default_rng(1)
    tok, note, typ, ndur, pdur = [], [], [], [], []
    for n, fr in zip(PHRASES, FRAMES):
        w = rng.uniform(0.5, 1.5, n)
        pdur += (w / w.sum() * fr * 256 / 48000).tolist()
        tok += rng.integers(3, 60, n).tolist()
        note += rng.integers(50, 75, n - 1).tolist() + [0]
        typ += [2] * (n - 1) + [1]
        ndur += rng.uniform(0.1, 0.4, n).tolist()
    return dict(ph_token=tok, note=note, note_type=typ, note_dur=ndur, ph_dur=pdur, **feats)


MAX_SECONDS = 65 * 256 / 48000            # 40 + 22 and 51 + 9 merge, the next phrase does not fit either time: three segments


def _restate(inf, plan, fade):
    results = []
    for i, b in enumerate(plan.batches):
        res = inf.infer_batch(b, seed=SEED + i)
        results.append({k: res[k].cpu().numpy() for k in ("wav", "mel", "f0", "lens")})
    return R.stitch_ref(results, plan.rows, len(plan.segments), 256, fade)


def _assert_song(out, want):
    wav, mel, f0, off = want
    assert np.array_equal(_bits(out["wav"].cpu().numpy()), _bits(wav)), "wav"
    assert np.array_equal(_bits(out["mel"].cpu().numpy()), _bits(mel)), "mel"
    assert np.array_equal(_bits(out["f0"].cpu().numpy()), _bits(f0)), "f0"
    assert [g["start_frame"] for g in out["segments"]] == off[:-1].tolist() and [g["n_frames"] for g in out["segments"]] == np.diff(off).tolist()
    assert out["wav"].numel() == int(off[-1]) * 256 and tuple(out["mel"].shape) == (int(off[-1]), 80) and out["f0"].numel() == int(off[-1])
    assert np.isfinite(wav).all() and np.isfinite(mel).all() and np.abs(wav).max() > 0


def test_sing_score_equals_the_restatement_of_its_own_batches(singer):
    inf, feats = singer
    sc = _score(feats)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = inf.sing_score(sc, max_seconds=MAX_SECONDS, segment_batch=2, in_flight=1, seed=SEED)
    plan = out["plan"]
    assert [(g["first"], g["last"]) for g in plan.segments] == [(0, 8), (8, 16), (16, 20)] and plan.rows == [[0, 1], [2]]
    total = int(np.floor(np.sum(np.asarray(sc["ph_dur"])) * 48000 / 256 + 0.5))
    assert plan.n_frames == total == sum(g["n_frames"] for g in out["segments"])
    assert "style_cache" in plan.batches[0] and plan.batches[0]["mel2ph"].shape[0] == 2 and plan.batches[1]["mel2ph"].shape[0] == 1
    assert len({g["n_frames"] for g in out["segments"][:2]}) == 2, "the first batch is ragged"
    want = _restate(inf, plan, 240)
    _assert_song(out, want)
    assert "lufs" not in out
    # the joints are faded, the song's ends are not: the restatement without a fade differs only within 240 samples of the two joints
    plain = _restate(inf, plan, 0)[0]
    diff = np.nonzero(_bits(plain) != _bits(want[0]))[0]
    joints = [g["start_frame"] * 256 for g in out["segments"][1:]]
    assert len(diff) > 0 and all(min(abs(d - j) for j in joints) <= 240 for d in diff)
    # three batches in flight: the same song
    out3 = inf.sing_score(sc, max_seconds=MAX_SECONDS, segment_batch=2, in_flight=3, seed=SEED)
    for k in ("wav", "mel", "f0"):
        assert torch.equal(out3[k], out[k]), k
    assert out3["segments"] == out["segments"]
    # another seed is another song
    assert not torch.equal(inf.sing_score(sc, max_seconds=MAX_SECONDS, segment_batch=2, seed=SEED + 1)["mel"], out["mel"])


def test_sing_score_with_a_contour_over_the_whole_song(singer):
    inf, feats = singer
    sc = _score(feats)
    n = 200                                                 # the contour's own grid: not the song's frame count
    hz = 220.0 + 70.0 * np.sin(np.arange(n) / 7.0)
    hz[30:44] = 0
    hz[120:123] = 0
    sc.update(pitch_hz=hz, pitch_shift=1.5)
    out = inf.sing_score(sc, max_seconds=MAX_SECONDS, segment_batch=2, in_flight=1, seed=SEED)
    plan = out["plan"]
    assert "pitch_hz" in plan.batches[0] and plan.batches[1]["pitch_shift"] == 1.5
    _assert_song(out, _restate(inf, plan, 240))
    f0 = out["f0"].cpu().numpy().astype(np.float64)
    fitted = plan.pitch_hz.astype(np.float64)
    assert len(fitted) == len(f0) and np.array_equal(f0 > 0, fitted > 0), "the slices sit where the song's frames are"
    v = fitted > 0
    assert v.any() and (~v).any() and np.allclose(f0[v], fitted[v] * 2 ** (1.5 / 12), rtol=1e-5, atol=0)
    assert "f0_a" not in next(iter(inf.infer_batches(plan.batches[:1], in_flight=1, seed=SEED)))["model_out"]
    with pytest.raises(ValueError, match="frame counts are not known before rendering"):
        inf.sing_score({k: v for k, v in sc.items() if k != "ph_dur"})


def test_sing_score_without_ph_dur_places_by_the_lengths_on_the_device(singer):
    """Predicted durations: the host knows no frame count before the final sync, and the batch order (by phone count) is not the order of the frame counts."""
    inf, feats = singer
    sc = {k: v for k, v in _score(feats).items() if k != "ph_dur"}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = inf.sing_score(sc, max_seconds=2.0, segment_batch=2, in_flight=1, seed=SEED)      # note_dur estimate: 1.31, 0.76, 2.00 (two phrases), 1.00 s
    plan = out["plan"]
    assert [(g["first"], g["last"]) for g in plan.segments] == [(0, 5), (5, 8), (8, 16), (16, 20)] and plan.rows == [[2, 0], [3, 1]]
    assert plan.n_frames is None and "mel2ph" not in plan.batches[0]
    _assert_song(out, _restate(inf, plan, 240))
    assert all(g["n_frames"] > 0 for g in out["segments"])
    out3 = inf.sing_score(sc, max_seconds=2.0, segment_batch=2, in_flight=3, seed=SEED)
    assert torch.equal(out3["wav"], out["wav"]) and out3["segments"] == out["segments"]


def test_single_segment_score_equals_infer_batch_of_that_item(singer):
    inf, feats = singer
    sc = _score(feats)
    out = inf.sing_score(sc, max_seconds=12.0, seed=SEED)     # 152 frames: one segment
    plan = out["plan"]
    assert len(plan.segments) == 1 and plan.rows == [[0]]
    item = dict(sc, mel2ph=plan.batches[0]["mel2ph"][0].cpu().numpy())
    del item["ph_dur"]
    batch = inf.input_to_batch(item)                          # the single-utterance surface: no style cache, no plan
    assert "style_cache" not in batch
    res = inf.infer_batch(batch, seed=SEED)
    F = plan.n_frames
    assert int(res["lens"][0]) == F == out["mel"].shape[0]
    assert torch.equal(out["wav"], res["wav"][0, :F * 256]) and torch.equal(out["mel"], res["mel"][0, :F]) and torch.equal(out["f0"], res["f0"][0, :F])


def test_loudness_applies_to_the_whole_song(singer):
    inf, feats = singer
    sc = _score(feats)
    kw = dict(max_seconds=MAX_SECONDS, segment_batch=2, seed=SEED)
    plain = inf.sing_score(sc, **kw)
    loud = inf.sing_score(sc, out_lufs=-20.0, **kw)
    assert isinstance(loud["lufs"], float) and np.isfinite(loud["lufs"])
    y, lufs = inf._to_lufs(plain["wav"][None], [plain["wav"].numel()], -20.0)
    assert torch.equal(loud["wav"], y[0]) and loud["lufs"] == float(lufs[0])
    assert not torch.equal(loud["wav"], plain["wav"]) and torch.equal(loud["mel"], plain["mel"])
    inf.hparams["out_loudness_lufs"] = -20.0                  # the hparams form of the same target
    try:
        assert torch.equal(inf.sing_score(sc, **kw)["wav"], loud["wav"])
    finally:
        inf.hparams["out_loudness_lufs"] = None


def test_score_run_writes_the_song_and_its_timeline(singer, tmp_path):
    """what `--score song.json --segments-out timeline.json` does once the checkpoints are loaded"""
    import json
    import wave
    from stylesinger_amd import infer
    _inf, feats = singer
    hp = dict(timesteps=3, K_step=3, f0_timesteps=3)
    full = config.make_hparams(hp)
    out_path, tl_path = tmp_path / "out" / "song.wav", tmp_path / "timeline.json"
    res = infer._score_run(_score(feats), hp, str(out_path), segments_out=str(tl_path), max_seconds=MAX_SECONDS, segment_batch=2, device=DEV,
                           model_state=synth.synth_acoustic_state_dict(full, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 11))
    with wave.open(str(out_path), "rb") as wf:
        assert (wf.getframerate(), wf.getsampwidth(), wf.getnchannels(), wf.getnframes()) == (48000, 2, 1, res["wav"].numel())
    tl = json.loads(tl_path.read_text())
    assert tl["n_samples"] == res["wav"].numel() and tl["hop"] == 256 and tl["sample_rate"] == 48000
    assert [(g["first_phone"], g["last_phone"]) for g in tl["segments"]] == [(0, 8), (8, 16), (16, 20)]
    assert [g["start_sample"] for g in tl["segments"]] == [g["start_frame"] * 256 for g in res["segments"]]
    assert tl["segments"][0]["start_sample"] == 0 and sum(g["n_samples"] for g in tl["segments"]) == tl["n_samples"]
