"""Pitch control on the GPU: `ss_pitch_given` against a float64 restatement, the given-f0 forms of StyleSingerHIP.forward (f0= / uv=, the
reference's use_gt_f0 test step; pitch_hz=, a contour in Hz fitted to the score by `ss_contour_fit`) against the predicted-f0 forward they must
reproduce when fed its own contour, against the REAL reference's golden outputs, and the entry points that carry them.

Documented accuracy of the device math these bounds rest on (HIP math API, single precision): exp2f and log2f are within 1 ulp."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_parity as P  # noqa: E402  (its fixtures' recipe and its mel bound; nothing of it is collected here)
from oracle import harness  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402
from stylesinger_amd.pitch import contour_fit, contour_fit_device, norm_interp_f0_device  # noqa: E402

DEV = torch.device("cuda:0")
EPS = 2.0 ** -23              # fp32: ulp(x) <= EPS * |x|
EXP2F_ULP = LOG2F_ULP = 1.0   # documented maximum error of the device functions, in ulp
ULP_LOG = 2.0 ** -20          # fp32 spacing in [8, 16): log2 of every frequency from 256 Hz up lies there, lower ones are spaced finer
SEED = 77


# ---- 1. the kernel against float64 -----------------------------------------------------------------------------------------------------
F0_MEL_MIN = 1127 * math.log(1 + 50.0 / 700)
F0_MEL_MAX = 1127 * math.log(1 + 1100.0 / 700)


def _coarse_f64(hz):
    """utils/pitch_utils.py f0_to_coarse in float64 -> (bin, distance of mel + 0.5 to the nearest integer = to a rounding boundary, in bins)"""
    mel = 1127 * np.log(1 + hz / 700)
    mel = np.where(mel > 0, (mel - F0_MEL_MIN) * 254 / (F0_MEL_MAX - F0_MEL_MIN) + 1, mel)
    inside = (mel > 1) & (mel < 255)          # clamped values sit on 1 / 255 exactly: no rounding decision left
    mel = np.clip(mel, 1, 255)
    y = mel + 0.5
    dist = np.where(inside, np.abs(y - np.round(y)), 0.5)
    return np.floor(y).astype(np.int64), dist


def _hz_f64(f0, uv, mel2ph):
    hz = np.exp2(f0.astype(np.float64))
    hz[(uv > 0) | (mel2ph == 0)] = 0.0
    return hz


@pytest.mark.parametrize("B,T", [(2, 37), (3, 100)])   # 74 frames: part of one block; 300: a tail block past the first 256 threads
def test_pitch_given_kernel_matches_float64(B, T):
    rng = np.random.default_rng(100 * B + T)
    n = B * T
    f0 = rng.uniform(6.0, 10.0, n).astype(np.float32)
    f0[:6] = [5.0, 5.5, 5.64, 10.11, 10.3, 10.9]          # below 50 Hz and above 1100 Hz: beyond the coarse range on both sides
    uv = (rng.random(n) < 0.3).astype(np.float32)
    uv[:6] = 0
    uv[6:9] = [0.5, 2.0, 1.0]                             # "uv > 0" is the rule, not "uv == 1"
    mel2ph = rng.integers(1, 9, n).astype(np.int64)
    mel2ph[rng.random(n) < 0.1] = 0
    mel2ph[:9] = 1
    # keep every frame at least 1e-3 bins from a rounding boundary of the float64 restatement: nudge the few that are closer
    for _ in range(50):
        _, dist = _coarse_f64(_hz_f64(f0, uv, mel2ph))
        close = dist < 1e-3
        if not close.any():
            break
        f0[close] += np.float32(0.004)
    hz = _hz_f64(f0, uv, mel2ph)
    want_coarse, dist = _coarse_f64(hz)
    assert (dist >= 1e-3).all(), "test inputs: a frame sits on a rounding boundary"
    assert (want_coarse[:3] == 1).all() and (want_coarse[3:6] == 255).all() and ((uv > 0).mean() > 0.2) and (mel2ph == 0).any()
    d = lambda a: torch.from_numpy(a).to(DEV)
    f0_d, uv_d, m_d = d(f0), d(uv), d(mel2ph)
    pp = torch.full((n, 2), float("nan"), device=DEV)
    den = torch.full((n,), float("nan"), device=DEV)
    co = torch.full((n,), -1, device=DEV, dtype=torch.int64)
    L.check(L.load().ss_pitch_given(L.ptr(f0_d), L.ptr(uv_d), L.ptr(m_d), L.ptr(pp), L.ptr(den), L.ptr(co), n, L.stream_ptr()), "ss_pitch_given")
    torch.cuda.synchronize()
    assert torch.equal(pp[:, 0].cpu(), torch.from_numpy(f0)) and torch.equal(pp[:, 1].cpu(), torch.from_numpy(uv))   # x/2 + x/2 is exact
    got = den.cpu().double().numpy()
    assert (got[hz == 0] == 0).all() and (got[hz > 0] > 0).all()
    bound = EXP2F_ULP * EPS * hz                           # the input is exact, exp2f is the only rounding
    err = np.abs(got - hz)
    print(f"ss_pitch_given n={n}: f0_denorm max rel err {np.max(err[hz > 0] / hz[hz > 0]):.3e} (bound {EXP2F_ULP * EPS:.3e}); "
          f"min distance to a bin boundary {dist.min():.2e}")
    assert (err <= bound).all()
    assert np.array_equal(co.cpu().numpy(), want_coarse)


# ---- the golden cases of the parity tests, built as test_gpu_parity._run_hip builds them ---------------------------------------------------
class _Case:
    def __init__(self, name):
        self.name = name
        self.gold = harness.load_case(name)
        meta = self.meta = self.gold["meta"]
        assert meta["give_mel2ph"]
        hp, sd, batch = harness.case_setup(meta)
        self.hp, self.sd = hp, sd
        self.model = StyleSingerHIP(None, hparams=hp)
        self.model.load_state_dict(sd, strict=True)
        self.model.eval().to(DEV)
        self.model.use_graphs = "off"
        self.noise = synth.draw_acoustic_noise(synth.NoiseTape(meta["tape_seed"]), meta["B"], meta["T"], meta["steps_f0"], meta["steps_mel"])
        self.batch = b = {k: v.to(DEV) for k, v in batch.items()}
        self.kw = dict(mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"], ref_f0=b["ref_f0"],
                       global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"])
        self.pred = self.run(noise=self.noise)          # the predicted-f0 forward on the golden's noise tape: computed once, read only

    def run(self, **kw):
        ret = self.model(self.batch["txt_tokens"], **{**self.kw, **kw})
        torch.cuda.synchronize()
        return ret


_cases = {}


@pytest.fixture(params=["acoustic_tiny_s4", "acoustic_b2_s3"])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = _Case(request.param)
    c = _cases[request.param]
    c.model.use_graphs = "off"
    return c


SAME = ("f0_denorm", "f0_denorm_pred", "pitch_coarse", "pitch_pred", "decoder_inp", "mel_out")


# ---- 2. feed-back identity ----------------------------------------------------------------------------------------------------------------
def test_forward_fed_its_own_contour_reproduces_the_predicted_forward(case):
    pred = case.pred
    mel_only = {"mel": case.noise["mel"]}                 # a recorded tape without f0_a / f0_b is accepted
    for nz in (case.noise, mel_only):
        again = case.run(noise=nz, f0=pred["pitch_pred"][..., 0], uv=pred["pitch_pred"][..., 1])
        for k in SAME:
            assert torch.equal(again[k], pred[k]), k
        assert not any(k in again for k in ("f0_a", "uv_a", "f0_b", "uv_b", "gdiff1", "mdiff1"))
        assert torch.equal(again["f0_denorm_pred"], again["f0_denorm"])
    # on-device Philox noise: the mel loop must draw the same numbers whether the f0 loops ran or not
    p2 = case.run(seed=SEED)
    g2 = case.run(seed=SEED, f0=p2["pitch_pred"][..., 0], uv=p2["pitch_pred"][..., 1])
    for k in SAME:
        assert torch.equal(g2[k], p2[k]), k
    assert "f0_a" in p2 and "f0_a" not in g2
    assert not torch.equal(p2["mel_out"], pred["mel_out"])


# ---- 3. against the REAL reference's own output -----------------------------------------------------------------------------------------------
def test_given_reference_contour_meets_the_parity_bound_of_the_golden(case):
    gold = case.gold["out"]
    pp = gold["pitch_pred"].to(DEV)
    ret = case.run(noise={"mel": case.noise["mel"]}, f0=pp[..., 0], uv=pp[..., 1])
    assert torch.equal(ret["pitch_pred"].cpu(), gold["pitch_pred"])
    assert torch.allclose(ret["f0_denorm"].cpu(), gold["f0_denorm"], rtol=2e-4, atol=1e-2)      # test_gpu_parity.py:71
    l1 = (ret["mel_out"].cpu() - gold["mel_out"]).abs().mean().item()
    print(f"{case.name} given the reference's pitch_pred: mel L1 {l1:.3e} (bound {P.MEL_L1_TOL:g})")
    assert l1 <= P.MEL_L1_TOL                                                                   # test_gpu_parity.py:16,76


# ---- 4. the contour form --------------------------------------------------------------------------------------------------------------------
def _fit_rel_bound(shift):
    """|kernel - float64 definition| / value for ss_contour_fit on contours within 80..800 Hz: la, lc = log2f (LOG2F_ULP ulp of a value < 16 each;
    their errors enter the exponent with weights 1 - fr and fr), d = lc - la, fr and fr * d each rounded once (|d| <= log2(10), EPS / 2 each),
    the sum rounded once (ULP_LOG / 2); exp2f (EXP2F_ULP ulp) of that exponent; scale rounded to fp32 and one product when shift != 0."""
    e = LOG2F_ULP * ULP_LOG + 3 * math.log2(10.0) * EPS / 2 + ULP_LOG / 2
    return (2.0 ** e - 1) + EXP2F_ULP * EPS + (EPS if shift else 0.0)


def _fwd_rel_bound(shift):
    """... and through forward: norm_interp_f0_device rounds the float64 log2(f0 + 1e-8) to fp32 (ULP_LOG / 2 in the exponent; 1e-8 / 80 relative from
    the offset), ss_pitch_given takes exp2f of it."""
    return _fit_rel_bound(shift) + (2.0 ** (ULP_LOG / 2) - 1) + 1e-8 / 80 + EXP2F_ULP * EPS


def _contour(rng, B, n):
    t = np.arange(n)
    hz = np.stack([250.0 + 120.0 * np.sin(t * 2 * np.pi / (n / 2.3) + b) + 50.0 * np.sin(t * 2 * np.pi / 11.0) for b in range(B)])
    hz = np.clip(hz, 80.0, 800.0)
    for b in range(B):                                     # unvoiced runs, one of them at the start
        hz[b, :3 + b] = 0
        for s in rng.integers(5, n - 5, 3):
            hz[b, s:s + int(rng.integers(1, 7))] = 0
    return hz.astype(np.float32)


@pytest.fixture(scope="module")
def ragged():
    """B = 2, items of 70 and 45 frames (T_out = 70, bucket 128), 3 sampler steps: the batch of test_ragged_batch_equals_per_item_runs"""
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 5))
    model.eval().to(DEV)
    model.use_graphs = "off"
    items = [synth.synth_utterance(0, 70, 7, 50, hp, 5), synth.synth_utterance(1, 45, 5, 38, hp, 5)]
    width = dict(txt_tokens=7, note=7, note_type=7, note_dur=7, mel2ph=70, ref_mels=50, ref_f0=50)

    def pad(t, n):
        out = torch.zeros((n,) + tuple(t.shape[1:]), dtype=t.dtype)
        out[:t.shape[0]] = t
        return out
    batch = {k: torch.stack([pad(it[k], width.get(k, it[k].shape[0])) for it in items]).to(DEV) for k in items[0]}

    def run(b=batch, **kw):
        ret = model(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"],
                    ref_f0=b["ref_f0"], global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"], **kw)
        torch.cuda.synchronize()
        return ret
    return dict(model=model, batch=batch, run=run, lens=[70, 45])


def test_contour_at_the_score_length_equals_the_reference_form(ragged):
    lens = ragged["lens"]
    hz = torch.from_numpy(_contour(np.random.default_rng(1), 2, 70)).to(DEV)
    a = ragged["run"](seed=SEED, pitch_hz=(hz, lens))
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    assert torch.equal(contour_fit_device(hz, lens, lens_d, 70), hz * (torch.arange(70, device=DEV)[None] < lens_d[:, None])), "a bit-exact copy"
    f0, uv = norm_interp_f0_device(hz, lens_d)
    b = ragged["run"](seed=SEED, f0=f0, uv=uv)
    for k in SAME:
        assert torch.equal(a[k], b[k]), k
    v = (hz > 0) & (torch.arange(70, device=DEV)[None] < lens_d[:, None])
    assert torch.equal(a["f0_denorm"] > 0, v) and torch.isfinite(a["mel_out"]).all()
    assert "f0_a" not in a and a["mel_out"].shape == (2, 70, 80) and a["mel_out"][1, 45:].abs().max().item() == 0.0


@pytest.mark.parametrize("Lc", [140, 67])   # 2 * T_out and T_out - 3
def test_fitted_contour_matches_the_float64_definition(ragged, Lc):
    lens_t = ragged["lens"]
    lens_c = [Lc, Lc - 9]
    hz = _contour(np.random.default_rng(Lc), 2, Lc)
    hz_d = torch.from_numpy(hz).to(DEV)
    lens_d = torch.tensor(lens_t, dtype=torch.int32, device=DEV)
    want = np.zeros((2, 70))
    for b in range(2):
        want[b, :lens_t[b]] = contour_fit(hz[b, :lens_c[b]], lens_t[b])
    fit = contour_fit_device(hz_d, lens_c, lens_d, 70).cpu().double().numpy()
    ret0 = ragged["run"](skip_decoder=True, pitch_hz=(hz_d, lens_c))
    ret12 = ragged["run"](skip_decoder=True, pitch_hz=(hz_d, lens_c), pitch_shift=12)
    fwd0, fwd12 = ret0["f0_denorm"].cpu().double().numpy(), ret12["f0_denorm"].cpu().double().numpy()
    voiced = want > 0
    assert voiced.any() and (~voiced[0, :70]).any()
    rel = lambda got, ref: float(np.max(np.abs(got - ref)[voiced] / ref[voiced]))
    print(f"Lc={Lc}: kernel vs definition {rel(fit, want):.3e} (bound {_fit_rel_bound(0):.3e}); forward {rel(fwd0, want):.3e}, "
          f"shift 12 {rel(fwd12, 2 * want):.3e} (bounds {_fwd_rel_bound(0):.3e}, {_fwd_rel_bound(12):.3e})")
    for got, ref, bound in ((fit, want, _fit_rel_bound(0)), (fwd0, want, _fwd_rel_bound(0)), (fwd12, 2 * want, _fwd_rel_bound(12))):
        assert np.array_equal(got > 0, voiced)             # voicing: exactly the nearest source frame's, 0 past each item's length
        assert (np.abs(got - ref)[voiced] <= bound * ref[voiced]).all()
    assert ret0["f0_denorm"].shape == (2, 70) and "f0_a" not in ret0


def test_contour_form_does_not_depend_on_the_batch_order_and_sings_an_unvoiced_item_unvoiced(ragged):
    lens_t, lens_c = ragged["lens"], [90, 61]
    hz = torch.from_numpy(_contour(np.random.default_rng(9), 2, 90)).to(DEV)
    a = ragged["run"](skip_decoder=True, pitch_hz=(hz, lens_c), pitch_shift=-2.5)
    flip = {k: v.flip(0).contiguous() for k, v in ragged["batch"].items()}
    b = ragged["run"](flip, skip_decoder=True, pitch_hz=(hz.flip(0).contiguous(), lens_c[::-1]), pitch_shift=-2.5)
    for k in ("f0_denorm", "pitch_pred", "pitch_coarse"):
        assert torch.equal(a[k], b[k].flip(0)), k
    lens_d = torch.tensor(lens_t, dtype=torch.int32, device=DEV)
    one = contour_fit_device(hz[1:], lens_c[1:], lens_d[1:], 70, -2.5)      # item 1 alone = item 1 of the batch
    assert torch.equal(one[0], contour_fit_device(hz, lens_c, lens_d, 70, -2.5)[1])
    # an item without a voiced frame: norm_interp_f0's all-unvoiced rule (f0 = 0, uv = 1) - every frame unvoiced, bin 1, a finite mel
    hz0 = hz.clone()
    hz0[1] = 0
    r = ragged["run"](seed=SEED, pitch_hz=(hz0, lens_c))
    assert r["f0_denorm"][1].abs().max().item() == 0.0 and (r["pitch_coarse"][1] == 1).all() and (r["pitch_pred"][1, :45, 1] == 1).all()
    assert (r["f0_denorm"][0] > 0).any() and torch.isfinite(r["mel_out"]).all()


# ---- 5. graphs ------------------------------------------------------------------------------------------------------------------------------
def test_given_f0_forward_under_hipgraphs_is_bit_equal_and_captures_no_f0_graph():
    hp = config.make_hparams(dict(timesteps=5, K_step=5, f0_timesteps=5))
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 3))
    model.eval().to(DEV)
    batch = {k: v.to(DEV) for k, v in synth.synth_batch(2, 90, 6, 70, hp, 3).items()}   # the shape of test_hipgraph_replay_matches_eager_and_reseeds
    f0 = torch.log2(torch.from_numpy(np.clip(_contour(np.random.default_rng(2), 2, 90), 80.0, None))).to(DEV)
    uv = (torch.from_numpy(_contour(np.random.default_rng(2), 2, 90)) == 0).float().to(DEV)

    def run(seed):
        return model(batch["txt_tokens"], mel2ph=batch["mel2ph"], spk_embed=batch["spk_embed"], emo_embed=batch["emo_embed"],
                     ref_mels=batch["ref_mels"], ref_f0=batch["ref_f0"], f0=f0, uv=uv, global_steps=320000, infer=True, note=batch["note"],
                     note_dur=batch["note_dur"], note_type=batch["note_type"], seed=seed)["mel_out"].clone()
    model.use_graphs = "off"
    eager = run(SEED)
    model.use_graphs = "on"
    before = model.n_captures
    g1 = run(SEED)   # captures
    g2 = run(SEED)   # replays
    g3 = run(SEED + 1)
    assert torch.equal(eager, g1) and torch.equal(g1, g2)
    assert (g3 - g2).abs().max().item() > 1e-3 and torch.isfinite(g3).all()
    plans = list(model._plans.values())
    assert len(plans) == 1 and plans[0].g_f0 is None and plans[0].g_mel is not None and model.n_captures == before + 1


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ragged):
    run = ragged["run"]
    f0, uv = torch.full((2, 70), 8.0, device=DEV), torch.zeros(2, 70, device=DEV)
    with pytest.raises(ValueError, match=r"(?s)69.*70"):
        run(f0=f0[:, :69], uv=uv[:, :69])
    with pytest.raises(ValueError, match=r"(?s)128.*70"):
        run(f0=torch.zeros(2, 128, device=DEV), uv=torch.ones(2, 128, device=DEV))      # the bucket is not the caller's frame count
    # predicted durations (the golden case whose durations are predicted): the count that the message names is the predicted one
    meta = harness.load_case("acoustic_dur_s2")["meta"]
    hp, sd, db = harness.case_setup(meta)
    dm = StyleSingerHIP(None, hparams=hp)
    dm.load_state_dict(sd, strict=True)
    dm.eval().to(DEV)
    dm.use_graphs = "off"
    db = {k: v.to(DEV) for k, v in db.items()}
    dkw = dict(spk_embed=db["spk_embed"], emo_embed=db["emo_embed"], ref_mels=db["ref_mels"], ref_f0=db["ref_f0"], global_steps=320000, infer=True,
               note=db["note"], note_dur=db["note_dur"], note_type=db["note_type"], skip_decoder=True)
    T_pred = dm(db["txt_tokens"], **dkw)["mel2ph"].shape[1]
    Bd = meta["B"]
    with pytest.raises(ValueError, match=rf"(?s){T_pred + 1}.*{T_pred}.*predicted"):
        dm(db["txt_tokens"], f0=torch.zeros(Bd, T_pred + 1, device=DEV), uv=torch.ones(Bd, T_pred + 1, device=DEV), **dkw)
    # ... and a contour is fitted to whatever frame count comes out
    r = dm(db["txt_tokens"], pitch_hz=(torch.full((Bd, 33), 220.0, device=DEV), [33] * Bd), **dkw)
    assert r["f0_denorm"].shape == (Bd, T_pred) and torch.equal(r["f0_denorm"] > 0, r["mel2ph"] > 0) and (r["mel2ph"] > 0).any()
    with pytest.raises(ValueError, match="f0 without uv"):
        run(f0=f0)
    with pytest.raises(ValueError, match="pitch_hz"):
        run(f0=f0, uv=uv, pitch_hz=(torch.full((2, 70), 220.0, device=DEV), [70, 45]))
    with pytest.raises(ValueError, match="batch of 2"):
        run(pitch_hz=(torch.full((1, 70), 220.0, device=DEV), [70]))
    with pytest.raises(NotImplementedError):
        ragged["model"](ragged["batch"]["txt_tokens"], f0=f0, uv=uv, infer=False)


# ---- 7. entry points ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_carry_the_contour(case):
    from stylesinger_amd.infer import StyleSingerInfer
    vsd = synth.synth_vocoder_state_dict(None, 11)
    inf = StyleSingerInfer(case.hp, device=DEV, model_state=case.sd, vocoder_state=vsd)
    inf.model.use_graphs = "off"
    pred = case.pred
    want = case.run(noise=case.noise, f0=pred["pitch_pred"][..., 0], uv=pred["pitch_pred"][..., 1])
    batch = dict(case.batch, f0=pred["pitch_pred"][..., 0], uv=pred["pitch_pred"][..., 1])
    res = inf.infer_batch(batch, noise=case.noise, vocode=False)
    assert torch.equal(res["mel"], want["mel_out"]) and torch.equal(res["f0"], want["f0_denorm"]) and "f0_a" not in res["model_out"]
    assert torch.equal(res["mel"], pred["mel_out"])
    # the reference's test step: the batch's f0 / uv count only with hparams['use_gt_f0']
    class Sink:
        def submit_batch(self, names, pcm, lens, hop):
            self.n = len(names)
    names = [f"item{i}" for i in range(case.meta["B"])]
    off = inf.infer_batch_to_files(dict(batch, f0=batch["f0"] + 0.5), names, Sink(), seed=SEED)
    assert "f0_a" in off["model_out"]
    inf.hparams["use_gt_f0"] = True
    on = inf.infer_batch_to_files(dict(batch, f0=batch["f0"] + 0.5), names, Sink(), seed=SEED)
    assert "f0_a" not in on["model_out"] and torch.equal(on["model_out"]["pitch_pred"][..., 0], batch["f0"] + 0.5)
    inf.hparams["use_gt_f0"] = False
    if case.meta["B"] == 1:
        # the single-utterance surface: a contour in Hz of another length than the score, transposed
        it = {k: v[0].cpu() for k, v in case.batch.items()}
        T = it["mel2ph"].shape[0]
        inp = dict(ph_token=it["txt_tokens"].numpy(), mel=it["ref_mels"].numpy(), spk_embed=it["spk_embed"].numpy(), emo_embed=it["emo_embed"].numpy(),
                   note=it["note"].numpy(), note_dur=it["note_dur"].numpy(), note_type=it["note_type"].numpy(), f0=np.exp2(it["ref_f0"].numpy()),
                   mel2ph=it["mel2ph"].numpy(), pitch_hz=_contour(np.random.default_rng(4), 1, T + 15)[0], pitch_shift=3.0)
        wav = inf.infer_once(inp)
        assert wav.shape == (T * 256,) and np.isfinite(wav).all() and np.abs(wav).max() > 0
        with pytest.raises(ValueError, match="pitch_shift"):
            inf.infer_once({k: v for k, v in inp.items() if k != "pitch_hz"})
