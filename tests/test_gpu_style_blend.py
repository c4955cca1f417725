"""The reference blend end to end on the GPU: forward(ref_mels [B, R, Tr, 80], ref_f0 [B, R, Tr], ref_weights=), `encode_style_blend`, `infer_batch`
with a pool from `_device_batch`, and `sing_score` with inp['ref_audios'] - on the weights of the small golden case acoustic_tiny_s4 (synthetic:
what is checked is the mechanism - the identities a weighted pool must satisfy - not how a trained checkpoint renders a blend, which is unassessed).

References: A = the case's own (Tr = 40), B = a second synthetic one with Tr = 23 (clipped-normal log-mel, bin 0 never 0, a log2 f0
contour), zero-padded to 40 rows where the two are stacked. The pooled path pads every reference to Ts = 64 rows (a multiple of the 32-key tile),
so "the plain call" it is held to bit for bit is the single-reference forward on the reference zero-padded to 64 rows: the same launches on the
same shapes."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import style_blend_refs as S  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import harness  # noqa: E402
from oracle import restatement as R  # noqa: E402
from stylesinger_amd import config, f0track, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP, resolve_ref_weights  # noqa: E402

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def tiny():
    """(model, hp, sd, device batch, a function that runs forward on given references, the single-reference run on A): built once, shared."""
    case = harness.load_case("acoustic_tiny_s4")
    meta = case["meta"]
    hp, sd, batch = harness.case_setup(meta)
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(sd, strict=True)
    model.eval().to(DEV)
    b = {k: v.to(DEV) for k, v in batch.items()}
    other = synth.synth_utterance(1, meta["T"], meta["Tp"], 23, hp, meta["seed"])
    pad = lambda x, n: torch.nn.functional.pad(x, [0, 0] * (x.dim() - 1) + [0, n - x.shape[0]])
    refs = dict(A=(b["ref_mels"][0], b["ref_f0"][0]), B=(pad(other["ref_mels"], 40).to(DEV), pad(other["ref_f0"], 40).to(DEV)))

    def run(ref_mels, ref_f0, **kw):
        noise = synth.draw_acoustic_noise(synth.NoiseTape(meta["tape_seed"]), meta["B"], meta["T"], meta["steps_f0"], meta["steps_mel"])
        ret = model(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=ref_mels, ref_f0=ref_f0,
                    global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"], noise=noise, **kw)
        torch.cuda.synchronize()
        return ret

    def pool(*names):
        return torch.stack([refs[n][0] for n in names])[None], torch.stack([refs[n][1] for n in names])[None]
    pad64 = lambda x: torch.nn.functional.pad(x, [0, 0] * (x.dim() - 1) + [0, 64 - x.shape[0]])
    single = {n: run(pad64(refs[n][0])[None], pad64(refs[n][1])[None]) for n in ("A", "B")}
    return dict(model=model, hp=hp, sd=sd, batch=batch, run=run, pool=pool, refs=refs, single=single)


def test_one_reference_as_a_pool_is_the_plain_forward_bit_for_bit(tiny):
    """R = 1: style and the mel of the 4-step run equal the plain call on the same reference padded to Ts, bit for bit."""
    mel, f0 = tiny["refs"]["A"]
    got = tiny["run"](mel[None, None], f0[None, None], ref_weights=[1])
    plain = tiny["single"]["A"]
    assert torch.equal(got["style"], plain["style"]) and torch.equal(got["mel_out"], plain["mel_out"])
    assert tuple(got["style_rq"].shape) == (1, 64, 256) and tuple(got["ref_f0"].shape) == (1, 64) and tuple(got["rq_codes"].shape)[:2] == (1, 64)
    assert torch.equal(got["style_rq"], plain["style_rq"]) and torch.equal(got["rq_codes"], plain["rq_codes"])
    assert torch.isfinite(got["mel_out"]).all() and torch.isfinite(got["style"]).all()


def test_weights_one_zero_are_the_first_reference_alone_bit_for_bit(tiny):
    mels, f0s = tiny["pool"]("A", "B")
    got = tiny["run"](mels, f0s, ref_weights=[1, 0])
    assert torch.equal(got["style"], tiny["single"]["A"]["style"]) and torch.equal(got["mel_out"], tiny["single"]["A"]["mel_out"])
    other = tiny["run"](mels, f0s, ref_weights=[[0.0, 2.5]])
    assert torch.equal(other["style"], tiny["single"]["B"]["style"])


def test_the_same_reference_twice_is_that_reference(tiny):
    """(A, A) with (0.3, 0.7) is mathematically A alone. Bound: 4 x the error fp32 arithmetic has on the two aligner layers - the float32 run of
    their restatement (tests/style_blend_refs.py::align_layers) against its float64 run, on this content and this style sequence - and never less
    than 2 ulp of the output's magnitude: the 4 x rule of test_gpu_small_kernels.py. Nothing in it comes from the kernel's output."""
    model, sd, hp, batch = tiny["model"], tiny["sd"], tiny["hp"], tiny["batch"]
    mels, f0s = tiny["pool"]("A", "A")
    got = tiny["run"](mels, f0s, ref_weights=[0.3, 0.7])
    d = float((got["style"] - tiny["single"]["A"]["style"]).abs().max().item())
    cache = model.encode_style_blend(mels, f0s, [0.3, 0.7])
    with torch.no_grad():
        enc = R.encoder(sd, hp, batch["txt_tokens"]) + R.note_encoder(sd, hp, batch["note"], batch["note_dur"], batch["note_type"])
        content = R.expand_states(enc, batch["mel2ph"])
        kw = dict(R=2, Ts=64, seg_lens=cache["seg_lens"].cpu(), seg_logw=cache["seg_logw"].cpu())
        ref64 = S.align_layers(sd, content, cache["sty"].cpu(), dtype=torch.float64, **kw)
        cpu32 = S.align_layers(sd, content, cache["sty"].cpu(), dtype=torch.float32, **kw)
    cpu_err = float((cpu32.double() - ref64).abs().max().item())
    bound = max(4.0 * cpu_err, 2.0 * float(np.spacing(np.float32(ref64.abs().max().item()))))
    err64 = float((got["style"].cpu().double() - ref64).abs().max().item())
    record_measurement("style_blend_same_reference_twice", vs_single_reference=d, cpu_fp32_err=cpu_err, bound=bound, ratio=d / bound, vs_float64=err64)
    print(f"[style blend (A, A)] vs A alone {d:.3e}, cpu-fp32 {cpu_err:.3e}, bound {bound:.3e}, vs float64 {err64:.3e}")
    assert cache["seg_lens"].tolist() == [[40, 40]]
    assert d <= bound, (d, cpu_err, bound)


def test_an_even_blend_of_two_references_is_neither(tiny):
    mels, f0s = tiny["pool"]("A", "B")
    got = tiny["run"](mels, f0s, ref_weights=[0.5, 0.5])
    assert torch.isfinite(got["style"]).all() and torch.isfinite(got["mel_out"]).all()
    for n in ("A", "B"):
        assert (got["style"] - tiny["single"][n]["style"]).abs().max().item() > 1e-3, n
    assert torch.equal(got["style"], tiny["run"](mels, f0s)["style"]), "no weights = equal weights"
    cache = tiny["model"].encode_style_blend(mels, f0s)
    assert cache["seg_lens"].tolist() == [[40, 23]] and cache["seg_lens"].dtype == torch.int32 and tuple(cache["sty"].shape) == (1, 128, 256)
    assert np.array_equal(cache["seg_logw"].cpu().numpy(), resolve_ref_weights(None, 1, 2)[0]) and all(v.shape[0] == 1 for v in cache.values())
    assert torch.equal(tiny["run"](mels, f0s, style_cache=cache)["style"], got["style"])


# ---- the entry points ------------------------------------------------------------------------------------------------------------------------
def _sung_wave(n, f_lo, f_hi, seed):
    """a sung-note-like signal: a harmonic complex with vibrato and a glide"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 48000.0
    ph = 2 * np.pi * np.cumsum(np.linspace(f_lo, f_hi, n) * (1 + 0.02 * np.sin(2 * np.pi * 5.0 * t))) / 48000.0
    return (sum(0.25 / h * np.sin(h * ph + 0.3 * h) for h in range(1, 9)) + 0.002 * rng.standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def singer():
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    inf = StyleSingerInfer(hp, device=DEV, model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 11),
                           emotion_state=synth.synth_emotion_state_dict(5), speaker_state=synth.synth_emotion_state_dict(6))
    inf.model.use_graphs = "off"
    return inf, [_sung_wave(256 * 60, 200.0, 260.0, 3), _sung_wave(256 * 45, 300.0, 240.0, 4)]


def test_infer_batch_with_a_blended_batch(singer):
    inf, clips = singer
    it = synth.synth_batch(1, 40, 5, 8, inf.hparams, 5)
    base = dict(ph_token=it["txt_tokens"][0].numpy(), note=it["note"][0].numpy(), note_dur=it["note_dur"][0].numpy(),
                note_type=it["note_type"][0].numpy(), mel2ph=it["mel2ph"][0].numpy())
    n0 = f0track.N_TRACK_CALLS
    batch = inf._device_batch(dict(base, ref_audios=[clips[0], (clips[1], 48000)], ref_weights=[0.7, 0.3]), vad_flags=False)
    assert f0track.N_TRACK_CALLS == n0 + 1, "the R clips go through the producers as ONE batch"
    assert tuple(batch["ref_mels"].shape) == (1, 2, 61, 80) and tuple(batch["ref_f0"].shape) == (1, 2, 61) and batch["n_mel"] == [61, 46]
    assert np.allclose(batch["ref_weights"], [[0.7, 0.3]]) and (batch["ref_mels"][0, 1, 46:] == 0).all()
    for k in ("spk_embed", "emo_embed"):
        assert tuple(batch[k].shape) == (1, 256) and abs(batch[k].norm().item() - 1.0) < 1e-5, k
    res = inf.infer_batch({k: v for k, v in batch.items() if k not in ("n_mel", "wav_fn", "ref_f0_hz")})
    assert tuple(res["wav"].shape) == (1, 40 * 256) and res["lens"].tolist() == [40] and torch.isfinite(res["wav"]).all()
    assert res["model_out"]["style_rq"].shape[1] == 2 * 64
    alone = inf._device_batch(dict(base, ref_audio=clips[0]), vad_flags=False)
    first = inf._device_batch(dict(base, ref_audios=clips, ref_weights=[1, 0]), vad_flags=False)
    # weights (1, 0): the first clip's features (the producers run it inside a batch of two: equal to fp32 rounding, not necessarily bit for bit)
    assert (first["ref_mels"][0, 0] - alone["ref_mels"][0]).abs().max().item() <= 1e-4
    for k in ("spk_embed", "emo_embed"):
        assert (first[k] - alone[k]).abs().max().item() <= 1e-5, k
    out = inf.infer_once(dict(base, ref_audios=clips), vad_flags=False)
    assert out.ndim == 1 and len(out) > 0 and np.isfinite(out).all()


def test_sing_score_encodes_a_pool_of_references_once(singer, monkeypatch):
    inf, clips = singer
    rng = np.random.default_rng(1)
    tok, note, typ, ndur, pdur = [], [], [], [], []
    for n, fr in zip((5, 3, 6), (40, 22, 51)):     # three phrases, each closed by a rest: three segments in two batches
        w = rng.uniform(0.5, 1.5, n)
        pdur += (w / w.sum() * fr * 256 / 48000).tolist()
        tok += rng.integers(3, 60, n).tolist()
        note += rng.integers(50, 75, n - 1).tolist() + [0]
        typ += [2] * (n - 1) + [1]
        ndur += rng.uniform(0.1, 0.4, n).tolist()
    sc = dict(ph_token=tok, note=note, note_type=typ, note_dur=ndur, ph_dur=pdur, ref_audios=clips, ref_weights=[2, 1])
    L.load()
    calls = []
    real = L.ops.ss_ref_lens
    monkeypatch.setattr(L.ops, "ss_ref_lens", lambda *a: (calls.append(a[1]), real(*a))[1])
    encodes = []
    real_encode = inf.model.encode_style
    monkeypatch.setattr(inf.model, "encode_style", lambda *a: (encodes.append(tuple(a[0].shape)), real_encode(*a))[1])
    out = inf.sing_score(sc, max_seconds=55 * 256 / 48000, segment_batch=2, in_flight=1, seed=7, vad_flags=False)
    assert len(out["plan"].batches) == 2 and len(out["segments"]) == 3
    assert calls == [2] and encodes == [(2, 64, 80)], "ONE encode of the flat batch of R = 2 references for the whole song"
    assert out["plan"].batches[0]["style_cache"]["seg_lens"].tolist() == [[61, 46]] * 2
    total = int(np.floor(np.sum(np.asarray(pdur)) * 48000 / 256 + 0.5))
    assert out["wav"].numel() == total * 256 and torch.isfinite(out["wav"]).all() and out["wav"].abs().max().item() > 0
    with pytest.raises(ValueError, match="not both"):
        inf.sing_score(dict(sc, ref_audio=clips[0]), vad_flags=False)
