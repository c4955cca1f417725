"""Retiming the score to a sung guide on the GPU: `ss_retime_mel2ph` (behind `ss_contour_align`) against the definition chain
`pitch.contour_align` -> `pitch.retime_to_guide` on the case table of tests/retime_cases.py - mel2ph', src, status and n_spans exactly equal - and
`StyleSingerHIP.forward(pitch_hz=..., pitch_timing="guide")` / `sing_score` on the synthetic weights.

Integer cents are injected through Hz (contour_align_cases.cents_to_hz); every case asserts the rounding margin of the device's cents."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import contour_align_cases as K  # noqa: E402
import retime_cases as R  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import pitch as P  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

DEV = torch.device("cuda:0")


def _launch(items, T, Lc, band, shift=0.0, extra=0):
    """items = [case dict] -> (out, src, status, n_spans, idx, status_align) as numpy from ONE launch of each kernel, the frame axes padded to T / Lc
    and every row stride `extra` wider than its width; what lies past an item's lengths is filled with values that would show in a result (phone 77,
    note 99, 999 Hz), what lies past the output's Lc columns must come back untouched (-5)."""
    B = len(items)
    hz = np.full((B, Lc + extra), 999.0, dtype=np.float32)
    mel2ph = np.full((B, T + extra), 77, dtype=np.int64)
    midi = np.full((B, T + extra), 99, dtype=np.int64)
    for b, c in enumerate(items):
        assert K.cents_margin(c["guide"], shift) < 0.25, "test input: a guide frame too close to a rounding boundary of the cents"
        hz[b, :len(c["guide"])] = c["guide"]
        mel2ph[b, :len(c["midi"])] = c["mel2ph"]
        midi[b, :len(c["midi"])] = c["midi"]
    hz_d, mp_d, md_d = torch.from_numpy(hz).to(DEV)[:, :Lc], torch.from_numpy(mel2ph).to(DEV)[:, :T], torch.from_numpy(midi).to(DEV)[:, :T]
    lens_c = torch.tensor([len(c["guide"]) for c in items], dtype=torch.int32, device=DEV)
    lens_t = torch.tensor([len(c["midi"]) for c in items], dtype=torch.int32, device=DEV)
    _, idx, _, st_a = P.contour_align_device(hz_d, lens_c, md_d, lens_t, T, band=band, shift=shift)
    out = torch.full((B, Lc + extra), -5, dtype=torch.int64, device=DEV)
    src = torch.full((B, Lc), -5, dtype=torch.int32, device=DEV)
    status = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    n_spans = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    L.ops.ss_retime_mel2ph(mp_d, mp_d.stride(0), md_d, md_d.stride(0), idx, st_a, lens_t, lens_c, out, out.stride(0), src, status, n_spans, T, Lc, B)
    if extra == 0:                                              # the wrapper is the same launch
        w = P.retime_device(mp_d, lens_t, md_d, idx, st_a, lens_c, Lc)
        assert torch.equal(w[0], out) and torch.equal(w[1], src) and torch.equal(w[2], status) and torch.equal(w[3], n_spans)
    torch.cuda.synchronize()
    assert (out[:, Lc:] == -5).all(), "columns beyond Lc were written"
    return tuple(t.cpu().numpy() for t in (out[:, :Lc], src, status, n_spans, idx, st_a))


def _equal_to(got, b, want, n_c):
    """row b of a launch against the definition's result for the item (its own width n_c): 0 / -1 in the padding"""
    out, src, status, n_spans = got[:4]
    assert status[b] == want["status"] and n_spans[b] == want["n_spans"], (status[b], want["status"], n_spans[b], want["n_spans"])
    assert np.array_equal(out[b, :n_c], want["out"][:n_c]) and np.array_equal(src[b, :n_c], want["src"][:n_c])
    assert not out[b, n_c:].any() and (src[b, n_c:] == -1).all()


# ---- 1. the kernel against the definition ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.NAMES)
def test_kernel_equals_the_definition(name):
    c, e = R.cases()[name], R.expected(name)
    n_t, n_c = len(c["midi"]), len(c["guide"])
    got = _launch([c], max(n_t, 1), max(n_c, 1), c["band"], c["shift"])
    assert got[5][0] == e["status_align"] and np.array_equal(got[4][0, :n_t], e["idx"])
    _equal_to(got, 0, e, n_c)
    assert e["status"] == R.WANT_STATUS.get(name, 0)


def test_a_ragged_batch_in_wider_buffers_equals_every_items_own_launch():
    names = ["melody", "n_c_equals_m_minus_1", "phones_without_frames"]
    items = [R.cases()[n] for n in names]
    assert all(c["band"] is None and c["shift"] == 0.0 for c in items)
    T, Lc = 40, 56
    got = _launch(items, T, Lc, None, extra=7)
    again = _launch(items, T, Lc, None, extra=7)
    for a, b in zip(got, again):                                # two launches on the same input: bit-identical
        assert np.array_equal(a, b)
    for b, (name, c) in enumerate(zip(names, items)):
        n_c = len(c["guide"])
        _equal_to(got, b, R.expected(name), n_c)
        alone = _launch([c], len(c["midi"]), n_c, None)
        assert np.array_equal(alone[0][0], got[0][b, :n_c]) and np.array_equal(alone[1][0], got[1][b, :n_c])
        assert alone[2][0] == got[2][b] and alone[3][0] == got[3][b]
    assert got[2].tolist() == [0, 1, 0]


def test_two_items_at_the_caps():
    """T = Lc = 8192: 4850 and 8192 anchors (ten and sixteen chunks of the block scans, the LDS arrays full). The path is ss_contour_align's own
    (band 4): the host definition of the alignment would build the whole cost matrix."""
    items = R.long_items()
    assert P.ALIGN_MAX_T == P.ALIGN_MAX_LC == 8192 and all(len(c["midi"]) == len(c["guide"]) == 8192 for c in items)
    got = _launch(items, 8192, 8192, 4)
    assert got[5].tolist() == [0, 0]
    for b, c in enumerate(items):
        out, src, status, m = P.retime_to_guide(c["mel2ph"], c["midi"], got[4][b], got[5][b], 8192)
        assert status == 0 and m == 1 + int((np.diff(c["midi"]) != 0).sum())
        _equal_to(got, b, dict(out=out, src=src, status=status, n_spans=m), 8192)
        assert np.array_equal(K.note_hz(c["midi"][src]), c["guide"]), "every guide frame took a score frame of the note it sings"
    assert got[3].tolist() == [int((np.diff(items[0]["midi"]) != 0).sum()) + 1, 8192]
    assert np.array_equal(got[1][1], np.arange(8192))           # item 1: n_c == m, the identity


def test_wrapper_refuses_sizes_beyond_the_caps():
    z = torch.zeros(1, 8, dtype=torch.int64, device=DEV)
    one = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="caps"):
        P.retime_device(z, one, z, z.int(), one, None, P.ALIGN_MAX_LC + 1)
    with pytest.raises(ValueError, match="mel2ph"):
        P.retime_device(z[:, :4], one, z, z.int(), one, None, 8)


# ---- 2. forward(pitch_timing="guide") --------------------------------------------------------------------------------------------------------------
NOTES1, FRAMES1, SUNG1 = [62, 65, 60, 0, 67], [6, 7, 5, 4, 8], [9, 6, 8, 4, 9]              # item 1: 30 score frames, 36 guide frames
SUNG0 = [6, 7, 3, 5, 12, 6, 5]                                                                 # item 0 (the musical case's score, 42): 44 guide frames


@pytest.fixture(scope="module")
def sung():
    """The tiny synthetic model of the pitch tests (3 sampler steps) on a batch of two scores with their mel2ph given (T = 42) and a guide per item
    that sings the same notes in another timing and another length (Lc = 44)."""
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 5))
    model.eval().to(DEV)
    model.use_graphs = "off"
    mc = K.musical_case()
    items = [synth.synth_utterance(0, 42, 7, 50, hp, 5), synth.synth_utterance(1, 30, 5, 38, hp, 5)]
    for it, notes, mel2ph in ((items[0], K.NOTES, mc["mel2ph"]), (items[1], NOTES1, np.repeat(np.arange(1, 6), FRAMES1))):
        it["note"] = torch.tensor(notes, dtype=torch.long)
        it["note_type"] = torch.tensor([1 if n == 0 else 2 for n in notes], dtype=torch.long)
        it["mel2ph"] = torch.from_numpy(np.asarray(mel2ph, dtype=np.int64))
    width = dict(txt_tokens=7, note=7, note_type=7, note_dur=7, mel2ph=42, ref_mels=50, ref_f0=50)

    def pad(t, n):
        out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype)
        out[:t.shape[0]] = t
        return out
    batch = {k: torch.stack([pad(it[k], width.get(k, it[k].shape[0])) for it in items]).to(DEV) for k in items[0]}

    def run(mel2ph="score", **kw):
        b = batch
        ret = model(b["txt_tokens"], mel2ph=b["mel2ph"] if isinstance(mel2ph, str) else mel2ph, spk_embed=b["spk_embed"], emo_embed=b["emo_embed"],
                    ref_mels=b["ref_mels"], ref_f0=b["ref_f0"], global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"],
                    note_type=b["note_type"], **kw)
        torch.cuda.synchronize()
        return ret
    guides = [np.repeat(K.note_hz(K.NOTES), SUNG0), np.repeat(K.note_hz(NOTES1), SUNG1)]
    lens_c, Lc = [len(g) for g in guides], max(len(g) for g in guides)
    hz = np.zeros((2, Lc), dtype=np.float32)
    for b, g in enumerate(guides):
        hz[b, :len(g)] = g
    return dict(model=model, hp=hp, batch=batch, run=run, guides=guides, lens_c=lens_c, Lc=Lc, hz=torch.from_numpy(hz).to(DEV),
                notes=[np.asarray(K.NOTES), np.asarray(NOTES1)])


def _host_retimed(sung, mel2ph_score, band=None, shift=0.0):
    """the definition chain on the host for every item of the batch -> (mel2ph' [2, Lc], src, status, idx per item)"""
    out = np.zeros((2, sung["Lc"]), dtype=np.int64)
    src = np.full((2, sung["Lc"]), -1, dtype=np.int32)
    status, idxs = [], []
    for b, g in enumerate(sung["guides"]):
        mp = mel2ph_score[b][mel2ph_score[b] > 0]
        midi = sung["notes"][b][mp - 1]
        _, idx, _, st_a = P.contour_align(g, midi, band=band, shift=shift)
        out[b], src[b], st, _ = P.retime_to_guide(mp, midi, idx, st_a, len(g), Lc=sung["Lc"])
        status.append(st)
        idxs.append(idx)
    return out, src, status, idxs


def test_forward_in_the_guides_timing_equals_forward_on_the_host_retimed_mel2ph(sung):
    score = sung["batch"]["mel2ph"].cpu().numpy()
    want_m2p, want_src, want_st, want_idx = _host_retimed(sung, score)
    assert want_st == [0, 0] and not np.array_equal(want_m2p[:, :42], score)          # the guide does move the notes
    pitch = (sung["hz"], sung["lens_c"])
    a = sung["run"](pitch_hz=pitch, pitch_timing="guide", seed=3)
    b = sung["run"](mel2ph=torch.from_numpy(want_m2p).to(DEV), pitch_hz=pitch, seed=3)
    assert a["mel_out"].shape == (2, sung["Lc"], 80) and a["lens"].cpu().tolist() == sung["lens_c"]
    for k in ("mel_out", "f0_denorm", "mel2ph"):
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["mel2ph"].cpu().numpy(), want_m2p) and np.array_equal(a["pitch_retime_src"].cpu().numpy(), want_src)
    assert a["pitch_retime_status"].cpu().tolist() == [0, 0] and torch.equal(a["mel2ph_score"], sung["batch"]["mel2ph"])
    idx = a["pitch_align_idx"].cpu().numpy()
    assert idx.shape == (2, 42) and a["pitch_align_status"].cpu().tolist() == [0, 0] and a["pitch_align_cost"].cpu().tolist() == [0, 0]
    for i in range(2):                                          # the alignment's outputs stay on the SCORE's frame axis
        assert np.array_equal(idx[i, :len(want_idx[i])], want_idx[i]) and (idx[i, len(want_idx[i]):] == -1).all()
    assert "pitch_retime_src" not in b and "mel2ph_score" not in b and "f0_a" not in a
    # the contour is used one to one: voiced exactly where the guide is
    assert np.array_equal(a["f0_denorm"].cpu().numpy() > 0, sung["hz"].cpu().numpy() > 0)
    # band and shift reach the alignment; pitch_align="dtw" next to pitch_timing changes nothing
    low = (sung["hz"] * 0.5, sung["lens_c"])
    c = sung["run"](pitch_hz=low, pitch_timing="guide", pitch_align="dtw", pitch_align_band=16, pitch_shift=12.0, seed=3, skip_decoder=True)
    assert torch.equal(c["mel2ph"], a["mel2ph"]) and c["pitch_align_cost"].cpu().tolist() == [0, 0]
    assert torch.equal(c["f0_denorm"], a["f0_denorm"])         # x0.5 and x2 are exact


def test_forward_retimes_predicted_durations_too(sung):
    pitch = (sung["hz"], sung["lens_c"])
    a = sung["run"](mel2ph=None, pitch_hz=pitch, pitch_timing="guide", seed=3, skip_decoder=True)
    plain = sung["run"](mel2ph=None, pitch_hz=pitch, seed=3, skip_decoder=True)
    assert torch.equal(a["mel2ph_score"], plain["mel2ph"]) and torch.equal(a["dur_choice"], plain["dur_choice"])
    want_m2p, want_src, want_st, _ = _host_retimed(sung, plain["mel2ph"].cpu().numpy())
    assert a["mel2ph"].shape == (2, sung["Lc"]) and np.array_equal(a["mel2ph"].cpu().numpy(), want_m2p)
    assert np.array_equal(a["pitch_retime_src"].cpu().numpy(), want_src) and a["pitch_retime_status"].cpu().tolist() == want_st


# ---- 3. entry points -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inf(sung):
    from stylesinger_amd.infer import StyleSingerInfer
    hp = sung["hp"]
    ins = StyleSingerInfer(hp, device=DEV, model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 11))
    ins.model.use_graphs = "off"
    return ins


def test_infer_batch_carries_the_key(sung, inf):
    pitch = (sung["hz"], sung["lens_c"])
    want = sung["run"](pitch_hz=pitch, pitch_timing="guide", pitch_align_band=16, seed=3)
    res = inf.infer_batch(dict(sung["batch"], pitch_hz=pitch, pitch_timing="guide", pitch_align_band=16), vocode=False, seed=3)
    assert torch.equal(res["mel"], want["mel_out"]) and torch.equal(res["model_out"]["mel2ph"], want["mel2ph"])
    assert res["model_out"]["pitch_retime_status"].cpu().tolist() == [0, 0]


def test_sing_score_keeps_segment_starts_and_the_songs_length(inf):
    """Two segments of four phones; the guide lives on the song's frame grid and sings segment 0's first two notes with their lengths swapped. Every
    segment is sung in the timing of its slice: the notes move inside segment 0, the segments and the song stay where the plan put them."""
    import warnings
    notes = [60, 64, 62, 0, 67, 65, 69, 0]
    d = [6, 14, 5, 4, 5, 6, 12, 4]                           # score frames per phone
    e = [14, 6, 5, 4, 5, 6, 12, 4]                           # guide frames per phone: the same total inside each segment
    ref = synth.synth_utterance(0, 8, 4, 50, inf.hparams, 5)
    sc = dict(ph_token=[5, 9, 13, 4, 7, 21, 30, 4], note=notes, note_type=[1 if n == 0 else 2 for n in notes], note_dur=[0.1] * 8,
              ph_dur=[f * 256 / 48000 for f in d], mel=ref["ref_mels"].numpy(), f0=np.exp2(ref["ref_f0"].numpy().astype(np.float64)),
              spk_embed=ref["spk_embed"].numpy(), emo_embed=ref["emo_embed"].numpy(), pitch_hz=np.repeat(K.note_hz(notes), e))
    kw = dict(max_seconds=30 * 256 / 48000, segment_batch=2, in_flight=1, seed=3)
    lin = inf.sing_score(sc, **kw)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # every segment is retimed: no warning
        out = inf.sing_score(dict(sc, pitch_timing="guide", pitch_align_band_s=10.2 * 256 / 48000), **kw)
    assert out["plan"].batches[0]["pitch_timing"] == "guide" and out["plan"].batches[0]["pitch_align_band"] == 10
    assert [(g["start_frame"], g["n_frames"]) for g in out["segments"]] == [(g["start_frame"], g["n_frames"]) for g in lin["segments"]] == [(0, 29), (29, 27)]
    assert out["f0"].shape == lin["f0"].shape == (56,) and out["wav"].shape == lin["wav"].shape
    assert [g["pitch_retime_status"] for g in out["segments"]] == [0, 0] and "pitch_retime_status" not in lin["segments"][0]
    guide = np.repeat(K.note_hz(notes), e)
    assert K.wrong_note_share(out["f0"].cpu().numpy(), guide) == 0.0 and np.array_equal(out["f0"].cpu().numpy() > 0, guide > 0)
    assert K.wrong_note_share(lin["f0"].cpu().numpy(), np.repeat(K.note_hz(notes), d)) >= 8 / 48     # the score's clock drifts against the take
