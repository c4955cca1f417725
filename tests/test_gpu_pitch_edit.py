"""The pitch expression controls on the GPU: `ss_pitch_edit_runs` / `ss_pitch_edit` against the float64 definition `pitch.pitch_edit` on the case
table of tests/pitch_edit_cases.py (every item x W in {1, 3, 31} x three parameter sets), and `StyleSingerHIP.forward(pitch_correct=, vibrato_scale=,
vibrato_add=)` / `infer_batch` / `sing_score` on the synthetic weights of the pitch tests.

Bounds. The device adds the definition's sums in the definition's order in float64 (relative error ~1e-13 at worst, from sin and the order of a
wave's reduction), so it rounds to the definition's fp32 value or, next to a rounding boundary, to its neighbour: every edited frame within 1 fp32
ulp, and at most 1 % of the sung frames different at all (tests/test_pitch_edit_cpu.py shows that even the reversed summation order stays inside
that cap on these inputs). Statistics: sums of n float64 terms in another order, within n 2^-52 of the sum of the absolute values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import contour_align_cases as K  # noqa: E402
import pitch_edit_cases as C  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import pitch as P  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

DEV = torch.device("cuda:0")
EPS64 = 2.0 ** -52
NEUTRAL = dict(alpha=0.0, kappa=1.0, vibrato=None)


def _launch(data, W, prm, extra=0, rows=None, T=None):
    """One launch of each kernel on items `rows` (default all) of `data`, every row stride `extra` wider than T; outputs are pre-filled with values
    that would show (-5 / NaN). -> dict of numpy arrays; the columns beyond T of f_out must come back untouched."""
    rows = list(range(C.B)) if rows is None else rows
    T = C.T if T is None else T
    B = len(rows)
    wide = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.pad(a[rows][:, :T], ((0, 0), (0, extra)), constant_values=7).astype(dt))).to(DEV)
    f, u, midi = wide(data["f"], np.float32), wide(data["u"], np.float32), wide(data["midi"], np.int64)
    lens = torch.tensor([min(data["lens"][b], T) for b in rows], dtype=torch.int32, device=DEV)
    out = torch.full((B, T + extra), -5.0, device=DEV)
    lo = torch.full((B, T), -5, dtype=torch.int32, device=DEV)
    hi = torch.full((B, T), -5, dtype=torch.int32, device=DEV)
    n_tiles = (T + C.TILE - 1) // C.TILE
    partial = torch.full((B, n_tiles, 6), float("nan"), dtype=torch.float64, device=DEV)
    stats = torch.full((B, 6), float("nan"), dtype=torch.float64, device=DEV)
    vib = prm["vibrato"] or (1.0, 0.0, 0, 1)
    w = torch.from_numpy(P.edit_weights(W)).to(DEV)
    L.ops.ss_pitch_edit_runs(midi, midi.stride(0), lens, lo, hi, T, B)
    L.ops.ss_pitch_edit(f, f.stride(0), midi, midi.stride(0), u, lens, lo, hi, w, W, P.EDIT_K0, prm["alpha"], prm["kappa"], float(vib[1]),
                        P.vibrato_omega(vib[0], C.FPS), int(vib[2]), int(vib[3]), out, partial, stats, T, B)
    torch.cuda.synchronize()
    assert (out[:, T:] == -5).all(), "columns beyond T were written"
    return dict(f=out[:, :T].cpu().numpy(), stats=stats.cpu().numpy(), run_lo=lo.cpu().numpy(), run_hi=hi.cpu().numpy())


_got = {}


def _device(W, name):
    if (W, name) not in _got:
        _got[W, name] = _launch(C.batch(), W, C.PARAMS[name])
    return _got[W, name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


CASES = [(W, name) for W in C.WS for name in C.PARAMS]


@pytest.mark.parametrize("W,name", CASES)
def test_kernels_match_the_definition(W, name):
    got, want, d, sung = _device(W, name), C.reference(W, name), C.batch(), C.sung_mask()
    # held-run bounds: exact
    assert np.array_equal(got["run_lo"], want["run_lo"]) and np.array_equal(got["run_hi"], want["run_hi"])
    # unsung frames and frames past lens: the input's bits
    assert np.array_equal(_bits(got["f"])[~sung], _bits(d["f"])[~sung])
    # edited frames: within one fp32 ulp, at most 1 % different at all
    g, r = got["f"][sung], want["f"][sung]
    differ = int((g != r).sum())
    print(f"W={W} {name}: {differ} of {sung.sum()} sung frames differ from the definition; max |diff| / ulp = "
          f"{np.max(np.abs(g.astype(np.float64) - r) / np.spacing(np.abs(r))):.2f}")
    assert np.all(np.abs(g.astype(np.float64) - r) <= np.spacing(np.abs(r)))
    assert differ <= 0.01 * sung.sum()
    assert not np.array_equal(g, d["f"][sung])                       # the edit does something
    # statistics
    prm = C.PARAMS[name]
    for b, n in enumerate(C.LENS):
        gs, ws = got["stats"][b], want["stats"][b]
        assert gs[0] == ws[0] and gs[5] == ws[5], (b, gs, ws)      # the two counts: exact
        if n == 0 or not sung[b].any():
            assert not gs.any()
            continue
        p = P.pitch_edit_parts(d["f"][b, :n], d["midi"][b, :n], W, prm["alpha"], prm["kappa"], prm["vibrato"], fps=C.FPS)
        v = p["sung"] & ~(d["u"][b, :n] > 0)
        cnt, ns = int(v.sum()), int(p["sung"].sum())
        dd, q = (p["x"] - p["m"])[v], (p["m"] - p["nbar"])[v]
        tol = (cnt + 4) * EPS64
        assert abs(gs[1] ** 2 * cnt - np.sum(dd * dd)) <= tol * np.sum(dd * dd), (b, gs[1], ws[1])
        assert abs(gs[2] - ws[2]) * cnt <= tol * np.sum(np.abs(q)) and abs(gs[3] - ws[3]) * cnt <= tol * np.sum(np.abs(q)), (b, gs, ws)
        # x' - x: the difference of two values of this size, each a few float64 roundings from the definition's
        assert abs(gs[4] - ws[4]) <= ns * EPS64 * max(np.max(np.abs(p["x"])), np.max(np.abs(p["xe"]))), (b, gs[4], ws[4])
    if prm["vibrato"] is not None:
        assert got["stats"][0, 5] > 0 and got["stats"][1, 5] > 0


@pytest.mark.parametrize("W", C.WS)
def test_neutral_parameters_through_the_kernel_are_bit_identical(W):
    got, d = _launch(C.batch(), W, NEUTRAL), C.batch()
    assert np.array_equal(_bits(got["f"]), _bits(d["f"]))
    assert got["stats"][:, 4].max() < 1e-9 and not got["stats"][:, 5].any()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f = dev(d["f"])
    same = P.pitch_edit_device(f, dev(d["u"]), dev(d["midi"]), torch.tensor(C.LENS, dtype=torch.int32, device=DEV), W, 0.0, 1.0)
    assert same[0] is f and same[1:] == (None, None, None)         # the wrapper launches and allocates nothing


@pytest.mark.parametrize("W,name", CASES)
def test_padding_strides_and_batching_do_not_reach_a_result(W, name):
    base = _device(W, name)
    for variant in (_launch(C.poisoned(1.0), W, C.PARAMS[name]), _launch(C.poisoned(-1.0), W, C.PARAMS[name], extra=5)):
        inside = np.arange(C.T)[None, :] < np.asarray(C.LENS)[:, None]
        assert np.array_equal(_bits(variant["f"])[inside], _bits(base["f"])[inside])
        assert np.array_equal(variant["run_lo"], base["run_lo"]) and np.array_equal(variant["run_hi"], base["run_hi"])
        assert np.array_equal(_bits(variant["stats"]), _bits(base["stats"]))
        pois = C.poisoned(1.0)["f"]
        assert np.array_equal(np.abs(variant["f"][~inside]), np.abs(pois[~inside]))       # past lens: f_out = f_in, whatever it holds
    strided = _launch(C.batch(), W, C.PARAMS[name], extra=3)
    for k in ("f", "stats"):
        assert np.array_equal(_bits(strided[k]), _bits(base[k])), k
    assert np.array_equal(strided["run_lo"], base["run_lo"]) and np.array_equal(strided["run_hi"], base["run_hi"])
    for b, n in enumerate(C.LENS):                                  # every item alone, in a buffer of its own length
        if n == 0:
            continue
        alone = _launch(C.batch(), W, C.PARAMS[name], rows=[b], T=n)
        assert np.array_equal(_bits(alone["f"][0]), _bits(base["f"][b, :n])) and np.array_equal(_bits(alone["stats"][0]), _bits(base["stats"][b]))
        assert np.array_equal(alone["run_lo"][0], base["run_lo"][b, :n]) and np.array_equal(alone["run_hi"][0], base["run_hi"][b, :n])


def test_the_wrapper_is_the_same_launch_and_the_window_cap_is_refused():
    d = C.batch()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    f, u, midi, lens = dev(d["f"]), dev(d["u"]), dev(d["midi"]), torch.tensor(C.LENS, dtype=torch.int32, device=DEV)
    prm = C.PARAMS["all"]
    out, stats, lo, hi = P.pitch_edit_device(f, u, midi, lens, 31, prm["alpha"], prm["kappa"], prm["vibrato"], fps=C.FPS)
    base = _device(31, "all")
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(base["f"])) and np.array_equal(_bits(stats.cpu().numpy()), _bits(base["stats"]))
    assert np.array_equal(lo.cpu().numpy(), base["run_lo"]) and np.array_equal(hi.cpu().numpy(), base["run_hi"])
    with pytest.raises(ValueError, match="refused"):
        P.pitch_edit_device(f, u, midi, lens, 256, 0.5, 1.0)
    # the C entry: an error code, and nothing written
    W = P.EDIT_MAX_W + 1
    o = torch.full_like(f, -5.0)
    partial = torch.full((C.B, 4, 6), -5.0, dtype=torch.float64, device=DEV)
    st = torch.full((C.B, 6), -5.0, dtype=torch.float64, device=DEV)
    w = torch.from_numpy(P.edit_weights(W)).to(DEV)
    with pytest.raises(L.StyleSingerHipError, match="refused"):
        L.ops.ss_pitch_edit(f, C.T, midi, C.T, u, lens, lo, hi, w, W, P.EDIT_K0, 0.5, 1.0, 0.0, 0.0, 0, 1, o, partial, st, C.T, C.B)
    torch.cuda.synchronize()
    assert (o == -5).all() and (partial == -5).all() and (st == -5).all()


# ---- forward ------------------------------------------------------------------------------------------------------------------------------------------
NOTES1, FRAMES1, SUNG1 = [62, 65, 60, 0, 67], [6, 7, 5, 4, 8], [9, 6, 8, 4, 9]
SUNG0 = [6, 7, 3, 5, 12, 6, 5]
EDIT = dict(pitch_correct=0.7, vibrato_scale=0.5)


@pytest.fixture(scope="module")
def sung():
    """The tiny synthetic model of the pitch tests (3 sampler steps) on a batch of two scores with their mel2ph given (T = 42) and a guide per item
    that sings the same notes in another timing (Lc = 44): the recipe of tests/test_gpu_retime.py."""
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

    def run(**kw):
        b = batch
        ret = model(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"], ref_f0=b["ref_f0"],
                    global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"], seed=3, **kw)
        torch.cuda.synchronize()
        return ret
    guides = [np.repeat(K.note_hz(K.NOTES), SUNG0), np.repeat(K.note_hz(NOTES1), SUNG1)]
    lens_c, Lc = [len(g) for g in guides], max(len(g) for g in guides)
    hz = np.zeros((2, Lc), dtype=np.float32)
    for b, g in enumerate(guides):
        hz[b, :len(g)] = g
    return dict(model=model, hp=hp, batch=batch, run=run, pitch=(torch.from_numpy(hz).to(DEV), lens_c))


def _check_edited(sung, base, ed, W=31, alpha=0.7, kappa=0.5, vibrato=None):
    """ed = the forward with the edit, base = the same forward without: ed's pitch is pitch_edit_device + ss_pitch_given of base's."""
    b = sung["batch"]
    mel2ph = ed["mel2ph"]
    assert torch.equal(mel2ph, base["mel2ph"])
    B, T = mel2ph.shape
    midi = torch.empty(B, T, device=DEV, dtype=torch.int64)
    L.ops.ss_gather_expand_i64(b["note"].contiguous(), mel2ph.contiguous(), midi, B, b["note"].shape[1], T)
    lens = (mel2ph > 0).sum(1).to(torch.int32)
    pp = base["pitch_pred"]
    f, u = pp[..., 0].contiguous(), pp[..., 1].contiguous()
    want_f, want_stats, _, _ = P.pitch_edit_device(f, u, midi, lens, W, alpha, kappa, vibrato, fps=187.5)
    assert torch.equal(ed["pitch_pred"][..., 0], want_f) and torch.equal(ed["pitch_pred"][..., 1], u)
    assert not torch.equal(want_f, f)
    want = (torch.empty(B, T, 2, device=DEV), torch.empty(B, T, device=DEV), torch.empty(B, T, device=DEV, dtype=torch.int64))
    L.ops.ss_pitch_given(want_f, u, mel2ph.contiguous(), *want, B * T)
    assert torch.equal(ed["pitch_pred"], want[0]) and torch.equal(ed["f0_denorm"], want[1]) and torch.equal(ed["pitch_coarse"], want[2])
    assert torch.equal(ed["f0_denorm_pred"], ed["f0_denorm"])
    assert torch.equal(ed["pitch_pred_raw"], pp) and torch.equal(ed["f0_denorm_raw"], base["f0_denorm"])
    assert torch.equal(ed["pitch_edit"], want_stats) and ed["pitch_edit"].shape == (B, 6) and ed["pitch_edit"].dtype == torch.float64
    assert not torch.equal(ed["mel_out"], base["mel_out"]) and not torch.equal(ed["decoder_inp"], base["decoder_inp"])
    # and the definition, per item: within an ulp of what the device wrote
    for i in range(B):
        n = int(lens[i])
        ref, st, _, _ = P.pitch_edit(f[i, :n].cpu().numpy(), midi[i, :n].cpu().numpy(), W, alpha, kappa, vibrato, u=u[i, :n].cpu().numpy(), fps=187.5)
        got = want_f[i, :n].cpu().numpy()
        assert np.all(np.abs(got.astype(np.float64) - ref) <= np.spacing(np.abs(ref))) and want_stats[i, 0].item() == st[0]
    return want_stats


def test_forward_edits_the_predicted_pitch(sung):
    base, ed = sung["run"](), sung["run"](**EDIT)
    stats = _check_edited(sung, base, ed)
    assert stats[:, 4].min().item() > 0                              # every item has sung frames, and they moved
    assert torch.equal(ed["f0_a"], base["f0_a"]) and torch.equal(ed["style"], base["style"])       # nothing upstream changes
    # the window and a synthetic vibrato reach the kernel: delay 20 ms = 4 frames, fade 5 ms = 1 frame
    ed2 = sung["run"](pitch_correct=0.2, vibrato_scale=1.0, vibrato_add=(6.0, 35.0, 20.0, 5.0), pitch_smooth_ms=40.0, skip_decoder=True)
    base2 = sung["run"](skip_decoder=True)
    f, u = base2["pitch_pred"][..., 0].contiguous(), base2["pitch_pred"][..., 1].contiguous()
    midi = torch.empty(2, 42, device=DEV, dtype=torch.int64)
    L.ops.ss_gather_expand_i64(sung["batch"]["note"], sung["batch"]["mel2ph"], midi, 2, 7, 42)
    lens = (sung["batch"]["mel2ph"] > 0).sum(1).to(torch.int32)
    want_f, want_stats, _, _ = P.pitch_edit_device(f, u, midi, lens, 4, 0.2, 1.0, (6.0, 35.0, 4, 1), fps=187.5)
    assert torch.equal(ed2["pitch_pred"][..., 0], want_f) and torch.equal(ed2["pitch_edit"], want_stats)
    no_vib, _, _, _ = P.pitch_edit_device(f, u, midi, lens, 4, 0.2, 1.0)
    assert not torch.equal(no_vib, want_f)                          # held notes of 6 frames and more carry the vibrato
    # hparams are the default, an explicit value wins
    sung["model"].hp.update(EDIT)
    try:
        via_hp, off = sung["run"](skip_decoder=True), sung["run"](skip_decoder=True, pitch_correct=0.0, vibrato_scale=1.0)
    finally:
        sung["model"].hp.update(pitch_correct=None, vibrato_scale=None)
    assert torch.equal(via_hp["pitch_pred"], ed["pitch_pred"]) and "pitch_edit" not in off and torch.equal(off["pitch_pred"], base["pitch_pred"])


@pytest.mark.parametrize("branch", [dict(pitch_align="dtw"), dict(pitch_timing="guide"), dict(), "f0"])
def test_forward_edits_a_given_contour_in_every_branch(sung, branch):
    if branch == "f0":
        pred = sung["run"](skip_decoder=True)
        branch = dict(f0=pred["pitch_pred"][..., 0].contiguous(), uv=pred["pitch_pred"][..., 1].contiguous())
    else:
        branch = dict(branch, pitch_hz=sung["pitch"])
    base, ed = sung["run"](**branch), sung["run"](**branch, **EDIT)
    _check_edited(sung, base, ed)
    for k in ("pitch_align_idx", "pitch_retime_src", "mel2ph_score"):
        assert (k in ed) == (k in base) and (k not in ed or torch.equal(ed[k], base[k])), k


@pytest.mark.parametrize("branch", [dict(), dict(pitch_align="dtw"), dict(pitch_timing="guide")])
def test_a_neutral_edit_is_no_edit(sung, branch):
    kw = dict(branch, pitch_hz=sung["pitch"]) if branch else {}
    absent = sung["run"](**kw)
    neutral = sung["run"](**kw, pitch_correct=0.0, vibrato_scale=1.0, vibrato_add=(5.5, 0.0), pitch_smooth_ms=200.0)
    assert set(absent) == set(neutral) and not {"pitch_edit", "pitch_pred_raw", "f0_denorm_raw"} & set(neutral)
    for k, v in absent.items():
        if torch.is_tensor(v):
            assert torch.equal(v, neutral[k]), k


# ---- entry points ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inf(sung):
    from stylesinger_amd.infer import StyleSingerInfer
    hp = sung["hp"]
    ins = StyleSingerInfer(hp, device=DEV, model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 11))
    ins.model.use_graphs = "off"
    return ins


def test_infer_batch_carries_the_keys(sung, inf):
    kw = dict(EDIT, vibrato_add=(6.0, 35.0, 20.0, 5.0), pitch_smooth_ms=40.0)
    want = sung["run"](**kw)
    res = inf.infer_batch(dict(sung["batch"], **kw), vocode=False, seed=3)
    assert torch.equal(res["mel"], want["mel_out"]) and torch.equal(res["f0"], want["f0_denorm"]) and torch.equal(res["pitch_edit"], want["pitch_edit"])
    assert "pitch_edit" not in inf.infer_batch(sung["batch"], vocode=False, seed=3)


def test_sing_score_applies_the_edit_per_segment(inf):
    notes = [60, 64, 62, 0, 67, 65, 69, 0]
    ref = synth.synth_utterance(0, 8, 4, 50, inf.hparams, 5)
    sc = dict(ph_token=[5, 9, 13, 4, 7, 21, 30, 4], note=notes, note_type=[1 if n == 0 else 2 for n in notes], note_dur=[0.1] * 8,
              ph_dur=[f * 256 / 48000 for f in [6, 14, 5, 4, 5, 6, 12, 4]], mel=ref["ref_mels"].numpy(),
              f0=np.exp2(ref["ref_f0"].numpy().astype(np.float64)), spk_embed=ref["spk_embed"].numpy(), emo_embed=ref["emo_embed"].numpy(),
              pitch_hz=np.repeat(K.note_hz(notes), [6, 14, 5, 4, 5, 6, 12, 4]) * 2.0 ** (30.0 / 1200.0))      # a guide 30 cents sharp: voiced on every note
    kw = dict(max_seconds=30 * 256 / 48000, segment_batch=2, in_flight=1, seed=3)
    plain = inf.sing_score(sc, **kw)
    out = inf.sing_score(dict(sc, pitch_correct=1.0, vibrato_scale=0.0, pitch_smooth_ms=40.0), **kw)
    assert len(out["segments"]) == 2 and "pitch_edit" not in plain
    assert all(b["pitch_correct"] == 1.0 and b["vibrato_scale"] == 0.0 and b["pitch_smooth_ms"] == 40.0 for b in out["plan"].batches)
    st = out["pitch_edit"].cpu().numpy()
    assert st.shape == (2, 6) and (st[:, 0] > 0).all() and (st[:, 4] > 0).all()
    assert out["f0"].shape == plain["f0"].shape and not torch.equal(out["f0"], plain["f0"])
    # hard-tuned by construction: inside a held note (further than the window from its ends) the f0 IS the note's
    f0 = out["f0"].cpu().numpy()
    hz = K.note_hz(notes)
    assert abs(1200 * np.log2(f0[13] / hz[1])) < 0.01 and abs(1200 * np.log2(f0[46] / hz[6])) < 0.01     # frames 6..19 sing note 64, 40..51 note 69
    # without ph_dur the keys are accepted too (the durations are the model's own)
    free = inf.sing_score(dict({k: v for k, v in sc.items() if k not in ("ph_dur", "pitch_hz")}, pitch_correct=1.0, vibrato_scale=0.0), **kw)
    assert free["pitch_edit"].shape[1] == 6
