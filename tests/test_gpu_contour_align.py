"""Contour alignment on the GPU: `ss_contour_align` against its definition (stylesinger_amd/pitch.py::contour_align) - idx, cost and status
exact, out bit-equal to fl32(g[idx]) * fl32(2^(shift / 12)) - and `StyleSingerHIP.forward(pitch_hz=..., pitch_align="dtw")` on the musical case of
tests/contour_align_cases.py.

Integer cents are injected through Hz (cases.cents_to_hz): the device's fp32 evaluation of 1200 log2(g / 440) + 100 shift is a few ulp of a value
below 16384 (< 5e-3 cent) away from an integer, so its rounding to cents cannot flip; every test asserts that margin in float64 on the host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import contour_align_cases as K  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import pitch as P  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

DEV = torch.device("cuda:0")
THREADS = 512                 # contour_align.hip: CA_THREADS
EPS = 2.0 ** -23              # fp32: ulp(x) <= EPS * |x|
EXP2F_ULP = 1.0               # documented maximum error of the device's exp2f, in ulp
ULP_LOG = 2.0 ** -20          # fp32 spacing in [8, 16): log2 of every frequency from 256 Hz up lies there


def _launch(items, T, Lc, band, shift=0.0, ldc_extra=5):
    """items = [(guide fp32 [n_c], midi int64 [n_t])] -> the device results as numpy, from ONE launch with the frame axes padded to T / Lc (padding
    filled with values a kernel that read it would show: 999 Hz, note 99) and a guide row stride of Lc + ldc_extra."""
    B = len(items)
    hz = np.full((B, Lc + ldc_extra), 999.0, dtype=np.float32)
    midi = np.full((B, T), 99, dtype=np.int64)
    for b, (g, m) in enumerate(items):
        hz[b, :len(g)] = g
        midi[b, :len(m)] = m
    hz_d = torch.from_numpy(hz).to(DEV)[:, :Lc]            # a view: row stride Lc + ldc_extra
    lens_c = [len(g) for g, _ in items]
    lens_t = torch.tensor([len(m) for _, m in items], dtype=torch.int32, device=DEV)
    out, idx, cost, status = P.contour_align_device(hz_d, lens_c, torch.from_numpy(midi).to(DEV), lens_t, T, band=band, shift=shift)
    fit = P.contour_fit_device(hz_d, lens_c, lens_t, T, shift)
    torch.cuda.synchronize()
    return out.cpu().numpy(), idx.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy(), fit.cpu().numpy()


def _check(items, T, Lc, band, shift=0.0, want_status=None):
    out, idx, cost, status, fit = _launch(items, T, Lc, band, shift)
    scale = np.float32(2.0 ** (shift / 12.0))
    for b, (g, m) in enumerate(items):
        assert K.cents_margin(g, shift) < 0.25, "test input: a guide frame too close to a rounding boundary of the cents"
        w_out, w_idx, w_cost, w_status = P.contour_align(g, m, band=band, shift=shift)
        n_t = len(m)
        assert status[b] == w_status and cost[b] == w_cost, (b, status[b], w_status, cost[b], w_cost)
        assert np.array_equal(idx[b, :n_t], w_idx), b
        assert (idx[b, n_t:] == -1).all() and not out[b, n_t:].any()
        if w_status == 0:
            src = g[w_idx]
            assert np.array_equal(out[b, :n_t], np.where(src > 0, src * scale, np.float32(0)).astype(np.float32)), b
            assert np.array_equal(out[b, :n_t], w_out)
        else:                                                   # not aligned: the arithmetic of ss_contour_fit, bit for bit
            assert np.array_equal(out[b], fit[b]), b
        if want_status is not None:
            assert w_status == want_status[b]
    return out, idx, cost, status


def _items(rng, n_t, n_c, content):
    if content == "ties":
        return K.tie_rich(rng, n_c), K.tie_rich_midi(rng, n_t)
    return K.random_cents(rng, n_c), K.random_midi(rng, n_t)


# ---- 1. the kernel against the definition ------------------------------------------------------------------------------------------------------
# (n_t, n_c, band): the smallest shapes that reach a distinct path of the kernel
SHAPES = [(1, 1, None), (1, 7, None), (7, 1, None),            # one row / one column: every diagonal holds one cell
          (37, 53, None), (53, 37, 4),                         # full matrix; a narrow band (37 <= 4 * 53)
          (66, 62, 16), (62, 66, None), (66, 62, None), (62, 66, 16),                              # around one wavefront of 64 rows / columns
          (THREADS + 3, THREADS - 3, 16), (THREADS - 3, THREADS + 3, None),                        # around the workgroup's 512 threads: a full
          (THREADS + 3, THREADS - 3, None), (THREADS - 3, THREADS + 3, 16)]                        # diagonal takes a second pass of the lanes


@pytest.mark.parametrize("content", ["ties", "random"])
@pytest.mark.parametrize("n_t,n_c,band", SHAPES)
def test_kernel_equals_the_definition(n_t, n_c, band, content):
    rng = np.random.default_rng(1000 * n_t + n_c + (7 if content == "ties" else 0))
    shift = 0.0 if content == "ties" else -3.0
    _check([_items(rng, n_t, n_c, content)], n_t, n_c, band, shift, want_status=[0])


def test_more_guide_frames_per_score_frame_than_the_band_allows_is_the_linear_fit():
    rng = np.random.default_rng(3)
    _check([_items(rng, 3, 50, "random")], 3, 50, 4, want_status=[1])          # 50 > 4 * 3
    _check([_items(rng, 3, 50, "random")], 8, 64, 4, shift=5.0, want_status=[1])


def test_a_batch_of_ragged_items_in_padded_buffers():
    rng = np.random.default_rng(4)
    items = [_items(rng, 20, 33, "ties"), (np.zeros(0, np.float32), K.tie_rich_midi(rng, 9)), _items(rng, 41, 29, "random")]
    for band in (None, 6):
        out, idx, cost, status = _check(items, 48, 40, band, want_status=[0, 1, 0])
        again = _launch(items, 48, 40, band)
        for a, b in zip((out, idx, cost, status), again):       # two launches on the same input: bit-identical
            assert np.array_equal(a, b)
        for b in (0, 2):                                        # row b of the batch = the item alone in buffers of its own size
            g, m = items[b]
            o1, i1, c1, s1, _ = _launch([items[b]], len(m), len(g), band, ldc_extra=0)
            assert np.array_equal(o1[0], out[b, :len(m)]) and np.array_equal(i1[0], idx[b, :len(m)]) and c1[0] == cost[b] and s1[0] == status[b]
    items[1] = (K.tie_rich(rng, 9), np.zeros(0, np.int64))      # the other empty: no score frames
    _check(items, 48, 40, None, want_status=[0, 1, 0])


def test_a_long_item_in_a_band():
    rng = np.random.default_rng(5)
    _check([_items(rng, 1500, 1400, "ties")], 1500, 1400, 64, want_status=[0])


def test_the_musical_case_on_the_kernel():
    mc = K.musical_case()
    for band, shift, g in ((None, 0.0, mc["guide"]), (K.BAND, 0.0, mc["guide"]), (K.BAND, 12.0, mc["guide"] * np.float32(0.5))):
        out, idx, cost, status = _check([(g, mc["midi"])], len(mc["midi"]), len(g), band, shift, want_status=[0])
        assert cost[0] == 0 and np.array_equal(out[0], mc["want"])


def test_entry_refuses_bad_arguments_and_launches_nothing():
    l = L.load()
    T = Lc = 16
    hz = torch.full((1, Lc), 220.0, device=DEV)
    midi = torch.full((1, T), 57, dtype=torch.int64, device=DEV)
    lens = torch.tensor([16], dtype=torch.int32, device=DEV)
    out = torch.full((1, T), -7.0, device=DEV)
    idx = torch.full((1, T), -7, dtype=torch.int32, device=DEV)
    cost = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(T * Lc, dtype=torch.uint8, device=DEV)
    ok = dict(f0=L.ptr(hz), ldc=Lc, Lc=Lc, lc=L.ptr(lens), midi=L.ptr(midi), ldm=T, lt=L.ptr(lens), band=0, uv=P.ALIGN_UV_COST, cap=P.ALIGN_CAP, shift=0.0,
              out=L.ptr(out), ldo=T, idx=L.ptr(idx), cost=L.ptr(cost), st=L.ptr(st), T=T, B=1, ws=L.ptr(ws), wsb=ws.numel())

    def call(**kw):
        a = dict(ok, **kw)
        return l.ss_contour_align(a["f0"], a["ldc"], a["Lc"], a["lc"], a["midi"], a["ldm"], a["lt"], a["band"], a["uv"], a["cap"], a["shift"], a["out"],
                                  a["ldo"], a["idx"], a["cost"], a["st"], a["T"], a["B"], a["ws"], a["wsb"], L.stream_ptr())
    for kw, word in ((dict(lc=None), b"null pointer"), (dict(idx=None), b"null pointer"), (dict(out=L.ptr(hz)), b"alias"), (dict(wsb=T * Lc - 1), b"workspace"),
                     (dict(shift=48.5), b"semitones"), (dict(shift=-49.0), b"semitones"),
                     (dict(T=P.ALIGN_MAX_T + 1, ldm=P.ALIGN_MAX_T + 1, ldo=P.ALIGN_MAX_T + 1), b"caps"),
                     (dict(Lc=P.ALIGN_MAX_LC + 1, ldc=P.ALIGN_MAX_LC + 1), b"caps")):
        assert call(**kw) != 0, kw
        err = l.ss_last_error()
        assert b"ss_contour_align" in err and word in err, (kw, err)
    torch.cuda.synchronize()
    assert (out == -7).all() and (idx == -7).all() and cost.item() == -7 and st.item() == -7, "a refused call wrote to its outputs"
    assert call() == 0                                          # ... and the same arguments unmodified are accepted
    torch.cuda.synchronize()
    assert st.item() == 0 and cost.item() == 0 and torch.equal(out, hz)
    with pytest.raises(ValueError, match="caps"):
        P.contour_align_device(torch.zeros(1, P.ALIGN_MAX_LC + 1, device=DEV), None, torch.zeros(1, 8, dtype=torch.int64, device=DEV), lens, 8)
    with pytest.raises(ValueError, match="ALIGN_MAX_WORKSPACE_BYTES"):     # 80 full items at the caps: 5 GiB of directions
        P.contour_align_device(torch.zeros(80, P.ALIGN_MAX_LC, device=DEV), None, torch.zeros(80, P.ALIGN_MAX_T, dtype=torch.int64, device=DEV),
                               torch.zeros(80, dtype=torch.int32, device=DEV), P.ALIGN_MAX_T)


# ---- 2. forward(pitch_align="dtw") ---------------------------------------------------------------------------------------------------------------
def _given_rel_bound():
    """|f0_denorm - note frequency| / frequency for a fitted contour that IS the guide's fp32 sample (the warp copies, shift = 0): the derivation of
    tests/test_gpu_pitch_given.py::_fwd_rel_bound without its fit term - norm_interp_f0_device rounds the float64 log2(f0 + 1e-8) to fp32
    (ULP_LOG / 2 in the exponent; 1e-8 / 80 relative from the offset), ss_pitch_given takes exp2f of it (EXP2F_ULP ulp) - plus the fp32 rounding of
    the note's frequency in the guide itself (EPS / 2)."""
    return (2.0 ** (ULP_LOG / 2) - 1) + 1e-8 / 80 + EXP2F_ULP * EPS + EPS / 2


@pytest.fixture(scope="module")
def sung():
    """The tiny synthetic model of the pitch tests (3 sampler steps) on a batch of two scores: item 0 = the musical case (42 frames, 7 phones), item 1
    = 30 frames of five notes; mel2ph given, T_out = 42 (bucket 128)."""
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 5))
    model.eval().to(DEV)
    model.use_graphs = "off"
    mc = K.musical_case()
    notes1, frames1 = [62, 65, 60, 0, 67], [6, 7, 5, 4, 8]
    midi1 = np.repeat(np.asarray(notes1, dtype=np.int64), frames1)
    items = [synth.synth_utterance(0, 42, 7, 50, hp, 5), synth.synth_utterance(1, 30, 5, 38, hp, 5)]
    for it, notes, mel2ph in ((items[0], K.NOTES, mc["mel2ph"]), (items[1], notes1, np.repeat(np.arange(1, 6), frames1))):
        it["note"] = torch.tensor(notes, dtype=torch.long)
        it["note_type"] = torch.tensor([1 if n == 0 else 2 for n in notes], dtype=torch.long)
        it["mel2ph"] = torch.from_numpy(np.asarray(mel2ph, dtype=np.int64))
    width = dict(txt_tokens=7, note=7, note_type=7, note_dur=7, mel2ph=42, ref_mels=50, ref_f0=50)

    def pad(t, n):
        out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype)
        out[:t.shape[0]] = t
        return out
    batch = {k: torch.stack([pad(it[k], width.get(k, it[k].shape[0])) for it in items]).to(DEV) for k in items[0]}

    def run(**kw):
        b = batch
        ret = model(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"],
                    ref_f0=b["ref_f0"], global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"],
                    skip_decoder=True, **kw)
        torch.cuda.synchronize()
        return ret
    want = np.zeros((2, 42), dtype=np.float32)                  # the score's note frequency per frame: fp32 (what a guide holds) and exact
    want[0], want[1, :30] = mc["want"], K.note_hz(midi1)
    want64 = np.zeros((2, 42))
    want64[0], want64[1, :30] = K.note_hz_f64(mc["midi"]), K.note_hz_f64(midi1)
    warped = np.zeros((2, 42), dtype=np.float32)                # item 0: the guide with its own timing; item 1: the score's timing
    warped[0], warped[1, :30] = mc["guide"], want[1, :30]
    return dict(model=model, hp=hp, batch=batch, run=run, want=want, want64=want64, warped=torch.from_numpy(warped).to(DEV), lens=[42, 30])


def test_forward_warps_the_guide_onto_the_score(sung):
    want, lens = sung["want"], sung["lens"]
    assert (want[want > 0] >= 256.0).all()                      # ULP_LOG is the spacing of log2 from 256 Hz up
    for kw in (dict(), dict(pitch_align_band=K.BAND)):
        ret = sung["run"](pitch_hz=(sung["warped"], lens), pitch_align="dtw", **kw)
        got = ret["f0_denorm"].cpu().double().numpy()
        assert got.shape == (2, 42) and ret["pitch_align_idx"].shape == (2, 42) and "f0_a" not in ret
        assert ret["pitch_align_cost"].cpu().tolist() == [0, 0] and ret["pitch_align_status"].cpu().tolist() == [0, 0]
        v = want > 0
        rel = np.abs(got - sung["want64"])[v] / sung["want64"][v]
        print(f"forward(pitch_align='dtw'{', band' if kw else ''}): f0_denorm vs the note frequency, max rel err {rel.max():.3e} (bound {_given_rel_bound():.3e})")
        assert np.array_equal(got > 0, v)                       # voiced exactly where the score has a note (the rests are unvoiced in the guide)
        assert (rel <= _given_rel_bound()).all()
        idx, guide = ret["pitch_align_idx"].cpu().numpy(), sung["warped"].cpu().numpy()
        assert (idx[1, 30:] == -1).all()
        for b in range(2):                                      # every score frame took a guide frame that holds its own note
            assert np.array_equal(guide[b][idx[b, :lens[b]]], want[b, :lens[b]])
    # the linear fit on the same input puts the wrong note on at least the share of frames the CPU test established
    lin = sung["run"](pitch_hz=(sung["warped"], lens))
    assert "pitch_align_idx" not in lin and "pitch_align_status" not in lin
    assert K.wrong_note_share(lin["f0_denorm"][0].cpu().numpy(), want[0]) >= 0.2
    assert K.wrong_note_share(ret["f0_denorm"][0].cpu().numpy(), want[0]) == 0.0


def test_forward_leaves_a_guide_with_the_scores_timing_alone(sung):
    guide = torch.from_numpy(sung["want"]).to(DEV)              # piecewise constant, unwarped
    a = sung["run"](pitch_hz=(guide, sung["lens"]), pitch_align="dtw")
    b = sung["run"](pitch_hz=(guide, sung["lens"]))
    for k in ("f0_denorm", "pitch_pred", "pitch_coarse", "decoder_inp"):
        assert torch.equal(a[k], b[k]), k
    assert a["pitch_align_cost"].cpu().tolist() == [0, 0]


def test_forward_without_the_mode_is_the_parents_sequence_bit_for_bit(sung):
    """pitch_align=None: contour_fit_device + norm_interp_f0_device + ss_pitch_given, called by hand on the bucket-padded frame axis."""
    model, b, lens_c = sung["model"], sung["batch"], [42, 30]
    ret = sung["run"](pitch_hz=(sung["warped"], lens_c), pitch_shift=1.5, pitch_align=None)
    T = model.bucket_frames(42)
    mel2ph = torch.zeros(2, T, dtype=torch.int64, device=DEV)
    mel2ph[:, :42] = b["mel2ph"]
    lens_t = (mel2ph != 0).sum(1).to(torch.int32)
    hz = P.contour_fit_device(sung["warped"], lens_c, lens_t, T, 1.5)
    f0_g, uv_g = P.norm_interp_f0_device(hz, lens_t, sung["hp"])
    pp = torch.empty(2, T, 2, device=DEV)
    den = torch.empty(2, T, device=DEV)
    co = torch.empty(2, T, dtype=torch.int64, device=DEV)
    L.check(L.load().ss_pitch_given(L.ptr(f0_g), L.ptr(uv_g), L.ptr(mel2ph), L.ptr(pp), L.ptr(den), L.ptr(co), 2 * T, L.stream_ptr()), "ss_pitch_given")
    torch.cuda.synchronize()
    assert torch.equal(ret["f0_denorm"], den[:, :42]) and torch.equal(ret["pitch_pred"], pp[:, :42]) and torch.equal(ret["pitch_coarse"], co[:, :42])
    assert not any(k.startswith("pitch_align") for k in ret)


def test_forward_refusals(sung):
    hz, lens = sung["warped"], sung["lens"]
    f0 = torch.zeros(2, 42, device=DEV)
    for kw, word in ((dict(pitch_align="dtw"), "needs pitch_hz"), (dict(pitch_align="dtw", f0=f0, uv=f0), "needs pitch_hz"),
                     (dict(pitch_hz=(hz, lens), pitch_align="linear"), "'dtw'"), (dict(pitch_hz=(hz, lens), pitch_align=True), "'dtw'"),
                     (dict(pitch_hz=(hz, lens), pitch_align_band=8), "needs pitch_align"),
                     (dict(pitch_hz=(hz, lens), pitch_align="dtw", pitch_align_band=-1), ">= 0")):
        with pytest.raises(ValueError, match=word):
            sung["run"](**kw)


# ---- 3. entry points -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inf(sung):
    from stylesinger_amd.infer import StyleSingerInfer
    hp = sung["hp"]
    ins = StyleSingerInfer(hp, device=DEV, model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 11))
    ins.model.use_graphs = "off"
    return ins


def test_entry_points_carry_the_alignment_keys(sung, inf):
    lens = sung["lens"]
    want = sung["run"](pitch_hz=(sung["warped"], lens), pitch_align="dtw", pitch_align_band=K.BAND)
    res = inf.infer_batch(dict(sung["batch"], pitch_hz=(sung["warped"], lens), pitch_align="dtw", pitch_align_band=K.BAND), vocode=False, seed=3)
    assert torch.equal(res["f0"], want["f0_denorm"]) and torch.equal(res["model_out"]["pitch_align_idx"], want["pitch_align_idx"])
    assert res["model_out"]["pitch_align_status"].cpu().tolist() == [0, 0]
    # the single-utterance surface: the musical case with the band in seconds
    it = {k: v[0].cpu() for k, v in sung["batch"].items()}
    band_s = (K.BAND + 0.2) * inf.hparams["hop_size"] / inf.hparams["audio_sample_rate"]      # -> K.BAND frames
    inp = dict(ph_token=it["txt_tokens"].numpy(), mel=it["ref_mels"].numpy(), spk_embed=it["spk_embed"].numpy(), emo_embed=it["emo_embed"].numpy(),
               note=it["note"].numpy(), note_dur=it["note_dur"].numpy(), note_type=it["note_type"].numpy(), f0=np.exp2(it["ref_f0"].numpy()),
               mel2ph=it["mel2ph"].numpy(), pitch_hz=K.musical_case()["guide"], pitch_align="dtw", pitch_align_band_s=band_s)
    one = inf.input_to_batch(inp)
    assert one["pitch_align"] == "dtw" and one["pitch_align_band"] == K.BAND
    r1 = inf.infer_batch(one, vocode=False, seed=3)
    assert r1["model_out"]["pitch_align_cost"].item() == 0 and K.wrong_note_share(r1["f0"][0].cpu().numpy(), sung["want"][0]) == 0.0
    wav = inf.infer_once(inp)
    assert wav.shape == (42 * 256,) and np.isfinite(wav).all() and np.abs(wav).max() > 0
    # a guide with more frames per score frame than the band allows: the linear fit, named in a warning where the host waits anyway
    long_guide = np.repeat(K.musical_case()["guide"], 40)
    with pytest.warns(UserWarning, match=r"pitch_align: items \[0\] not aligned"):
        inf.infer_once(dict(inp, pitch_hz=long_guide, pitch_align_band_s=band_s))
    with pytest.raises(ValueError, match="needs one of them"):
        inf.infer_once({k: v for k, v in inp.items() if k != "pitch_hz"})


def test_sing_score_warps_every_segments_slice_onto_its_own_notes(inf):
    """Two segments of four phones; the guide lives on the song's frame grid and sings segment 0's first two notes with their lengths swapped. The
    planner cuts the contour linearly (the slices are the segments' own frames); inside segment 0 only the warp puts the notes right."""
    import warnings
    notes = [60, 64, 62, 0, 67, 65, 69, 0]
    d = [6, 14, 5, 4, 5, 6, 12, 4]                           # score frames per phone
    e = [14, 6, 5, 4, 5, 6, 12, 4]                           # guide frames per phone: the same total inside each segment
    ref = synth.synth_utterance(0, 8, 4, 50, inf.hparams, 5)
    sc = dict(ph_token=[5, 9, 13, 4, 7, 21, 30, 4], note=notes, note_type=[1 if n == 0 else 2 for n in notes], note_dur=[0.1] * 8,
              ph_dur=[f * 256 / 48000 for f in d], mel=ref["ref_mels"].numpy(), f0=np.exp2(ref["ref_f0"].numpy().astype(np.float64)),
              spk_embed=ref["spk_embed"].numpy(), emo_embed=ref["emo_embed"].numpy(), pitch_hz=np.repeat(K.note_hz(notes), e))
    want = np.repeat(K.note_hz(notes), d)
    kw = dict(max_seconds=30 * 256 / 48000, segment_batch=2, in_flight=1, seed=3)
    lin = inf.sing_score(sc, **kw)
    assert [g["n_frames"] for g in lin["segments"]] == [29, 27]
    assert K.wrong_note_share(lin["f0"].cpu().numpy(), want) >= 8 / 48          # the 8 frames of the second note that the guide still sings the first on
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # every segment is aligned: no warning
        out = inf.sing_score(dict(sc, pitch_align="dtw", pitch_align_band_s=10.2 * 256 / 48000), **kw)
    assert out["plan"].batches[0]["pitch_align"] == "dtw" and out["plan"].batches[0]["pitch_align_band"] == 10
    assert K.wrong_note_share(out["f0"].cpu().numpy(), want) == 0.0 and np.array_equal(out["f0"].cpu().numpy() > 0, want > 0)
    # a band of one frame cannot hold either segment's warp, but both stay aligned (n_c == n_t): a higher cost, not a refusal
    narrow = inf.sing_score(dict(sc, pitch_align="dtw", pitch_align_band_s=1.2 * 256 / 48000), **kw)
    assert K.wrong_note_share(narrow["f0"].cpu().numpy(), want) > 0.0
