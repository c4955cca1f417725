"""The on-device BS.1770 meter (`ss_loudness_measure` / `ss_loudness_apply`, csrc/loudness.hip), the reference-audio intake with
hparams['loud_norm'] and the output LUFS target: the kernel against the independent float64 restatement (tests/loudness_ref.py) within half an
fp32 ulp of the gain, the peak rule, determinism and batch independence, graph capture, `preprocess_batch` / `infer_once` / `infer_batch`.
Parity with pyloudnorm is UNPINNED (the package is un-vendored); the definition is stylesinger_amd/loudness.py's."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_measurement  # noqa: E402
from loudness_ref import gated_signal, loudness_ref, normalize_ref  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import loudness as LD  # noqa: E402

RATES = (48000, 22050)
PAD = 37                                        # row stride = widest item + PAD
L_TOL = 20.0 * math.log10(1.0 + 2.0 ** -24)     # 5.18e-7 LU: half an fp32 ulp of the gain, the only place the loudness is consumed


def _lengths(rate):
    """one block exactly; one sample more; a last block past the end; rounded down to one block; 26 blocks, hundreds of chunks, a partial last one"""
    return [int(0.4 * rate), int(0.4 * rate) + 1, int(0.46 * rate), int(0.44 * rate), int(2.93 * rate) + 17]


@functools.lru_cache(maxsize=None)
def _case(rate):
    """the five gated signals of a rate and their restated loudness - computed once, never modified"""
    lens = _lengths(rate)
    xs = [gated_signal(n, rate) for n in lens]
    return lens, xs, [loudness_ref(x, rate) for x in xs]


def _device_input(xs, lens):
    """rows strided (ldx > L), everything past an item's own samples NaN: padding must not leak into a sum"""
    buf = torch.full((len(xs), max(lens) + PAD), float("nan"))
    for b, x in enumerate(xs):
        buf[b, :lens[b]] = torch.from_numpy(x)
    return buf.cuda()[:, :max(lens)]


def _gates(z):
    l = [-0.691 + 10.0 * math.log10(v) if v > 0 else -math.inf for v in z]
    J1 = [j for j in range(len(z)) if l[j] >= -70.0]
    if not J1:
        return J1, []
    rel = -0.691 + 10.0 * math.log10(sum(z[j] for j in J1) / len(J1)) - 10.0
    return J1, [j for j in range(len(z)) if l[j] > rel and l[j] > -70.0]


def _apply_f32(x, g):
    """the fp32 statement of the gain and the peak rule for a given g32"""
    g = np.float32(g)
    y = (g * x).astype(np.float32)
    P = np.float32(g * np.float32(np.abs(x).max()))
    return (y / P).astype(np.float32) if P > 1 else y


def _ulps(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


@pytest.mark.parametrize("chunk", [None, 256, 64])
@pytest.mark.parametrize("rate", RATES)
def test_kernel_matches_the_float64_restatement(rate, chunk):
    """|L_dev - L_ref| <= 20 log10(1 + 2^-24) = 5.18e-7 LU per item, equal gating sets, g32 within 1 ulp, the output bit-equal to fl32(g32 x).
    An fp32 filter state could never reach this; two float64 orderings of the cascade differ by ~1e-12 LU.
    Measured on an MI355X (recorded): worst |dL| 1.9e-12 LU / worst relative z_j error 6.3e-13 at the default chunk (48 kHz),
    1.5e-11 LU / 7.2e-12 at chunk 64."""
    lens, xs, refs = _case(rate)
    for n, r in zip(lens, refs):   # on the reference alone: no block sits within 0.1 LU of a threshold, so a flipped gate cannot be rounding
        assert all(abs(v + 70.0) >= 0.1 and abs(v - r["rel"]) >= 0.1 for v in r["l"]), n
    assert (len(refs[-1]["z"]), len(refs[-1]["J1"]), len(refs[-1]["J2"])) == (26, 24, 14 if rate == 48000 else 13)
    xd = _device_input(xs, lens)
    assert xd.stride(0) == max(lens) + PAD
    y, m = LD.normalize_batch(xd, lens, rate, chunk=chunk)
    z = LD.measure_batch(xd, lens, rate, chunk=chunk)["z"].cpu().numpy()
    lufs, gain, peak, y = m["lufs"].cpu().numpy(), m["gain"].cpu().numpy(), m["peak"].cpu().numpy(), y.cpu().numpy()
    assert np.isfinite(y).all(), "NaN padding leaked"
    worst_dl, worst_z = 0.0, 0.0
    for b, (n, x, r) in enumerate(zip(lens, xs, refs)):
        nb = len(r["z"])
        assert m["n_blocks"][b] == nb and (z[b, nb:] == 0).all()
        J1, J2 = _gates(list(z[b, :nb]))
        zerr = max(abs(z[b, j] - r["z"][j]) / r["z"][j] for j in range(nb))
        dl = abs(lufs[b] - r["L"])
        g_ref = np.float32(10.0 ** ((-22.0 - r["L"]) / 20.0))
        print(f"{rate} Hz chunk {chunk} item {b} (n {n}, {nb} blocks): L {lufs[b]:.9f} |dL| {dl:.3e} LU, worst rel z err {zerr:.3e}, "
              f"g32 {gain[b]!r} vs {g_ref!r}")
        worst_dl, worst_z = max(worst_dl, dl), max(worst_z, zerr)
        assert J1 == r["J1"] and J2 == r["J2"], (b, J1, J2)
        assert dl <= L_TOL, (b, dl)
        assert _ulps(gain[b], g_ref) <= 1, (b, gain[b], g_ref)
        assert peak[b] == np.abs(x).max()
        assert np.array_equal(y[b, :n], _apply_f32(x, gain[b])), b
        assert (y[b, n:] == 0.0).all(), "exact zeros past the item's length"
    record_measurement(f"loudness_device_vs_float64_restatement_{rate}_chunk_{chunk or LD.DEFAULT_CHUNK}", pinned=False, worst_abs_dL_LU=worst_dl,
                       worst_rel_z_err=worst_z, bound_LU=L_TOL)


@functools.lru_cache(maxsize=None)
def _clicks():
    rate, n = 48000, int(1.3 * 48000)
    x = 0.003 * np.random.default_rng(7).standard_normal(n)
    x[::rate // 4] += 0.9
    return rate, x.astype(np.float32)


def test_peak_rule_divides_by_the_peak_in_fp32():
    rate, x = _clicks()
    yr, Lr, gr = normalize_ref(x, rate)
    assert np.float32(gr * np.abs(x).max()) > 1, "the case must fire the rule"
    y, m = LD.normalize_batch(torch.from_numpy(x)[None].cuda(), [len(x)], rate)
    y, g = y[0].cpu().numpy(), m["gain"].cpu().numpy()[0]
    print(f"click train: L {float(m['lufs'][0]):.6f} (ref {Lr:.6f}), g32 {g!r}, g32 * peak {np.float32(g * np.abs(x).max())!r}")
    assert abs(float(m["lufs"][0]) - Lr) <= L_TOL and _ulps(g, gr) <= 1
    assert np.abs(y).max() == np.float32(1.0)
    assert np.array_equal(y, _apply_f32(x, g))


def test_meter_is_deterministic_and_independent_of_the_batch():
    lens, xs, _ = _case(22050)
    xd = _device_input(xs, lens)
    ya, ma = LD.normalize_batch(xd, lens, 22050)
    yb, mb = LD.normalize_batch(xd, lens, 22050)
    assert torch.equal(ya, yb) and all(torch.equal(ma[k], mb[k]) for k in ("lufs", "gain", "peak"))
    n = lens[-1]
    alone = torch.zeros(3, n + 5)                      # another B, another width, another row
    alone[1, :n] = torch.from_numpy(xs[-1])
    alone[0, :lens[0]] = torch.from_numpy(xs[0])
    alone[2, :lens[2]] = torch.from_numpy(xs[2])
    y1, m1 = LD.normalize_batch(alone.cuda(), [lens[0], n, lens[2]], 22050)
    assert torch.equal(y1[1, :n], ya[-1, :n])
    for k in ("lufs", "gain", "peak"):
        assert torch.equal(m1[k][1], ma[k][-1]), k
    z1 = LD.measure_batch(alone.cuda(), [lens[0], n, lens[2]], 22050)["z"]
    za = LD.measure_batch(xd, lens, 22050)["z"]
    assert torch.equal(z1[1], za[-1])


def test_short_items_and_silence_on_the_device():
    rate = 22050
    n = int(0.4 * rate)
    x = torch.zeros(3, 2 * n)
    x[0, :n - 1] = torch.from_numpy(gated_signal(n, rate)[:n - 1])
    x[2, :n] = torch.from_numpy(gated_signal(n, rate))
    xd = x.cuda()
    with pytest.raises(ValueError, match="fewer than one"):
        LD.normalize_batch(xd, [n - 1, 2 * n, n], rate)
    y, m = LD.normalize_batch(xd, [n - 1, 2 * n, n], rate, short="skip")
    lufs = m["lufs"].cpu().numpy()
    assert math.isnan(lufs[0]) and lufs[1] == -math.inf and math.isfinite(lufs[2])
    assert m["gain"].cpu().tolist()[:2] == [1.0, 1.0] and m["n_blocks"] == [0, 5, 1]
    assert torch.equal(y[:2], xd[:2]), "untouched"


def test_normalize_batch_is_graph_capturable():
    lens, xs, _ = _case(22050)
    xd = _device_input(xs, lens)
    eager, me = LD.normalize_batch(xd, lens, 22050)     # (also uploads the tables and the block bounds once)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, mo = LD.normalize_batch(xd, lens, 22050)
    out.fill_(float("nan"))
    mo["lufs"].fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(mo["lufs"], me["lufs"])


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------
def _harmonic(n, sr, f0=220.0):
    t = np.arange(n) / sr
    ph = 2 * np.pi * f0 * t + 0.3 * np.sin(2 * np.pi * 5.0 * t)
    return sum(0.2 / h * np.sin(h * ph + 0.3 * h) for h in range(1, 9)).astype(np.float32)


RAW_HP = dict(timesteps=3, K_step=3, f0_timesteps=3, loud_norm=True)


def _instance(hparams, **kw):
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(hparams)
    return StyleSingerInfer(hparams, device=torch.device("cuda:0"), model_state=synth.synth_acoustic_state_dict(hp, 5),
                            vocoder_state=synth.synth_vocoder_state_dict(None, 5), emotion_state=synth.synth_emotion_state_dict(5),
                            speaker_state=synth.synth_emotion_state_dict(6), **kw), hp


@pytest.fixture(scope="module")
def tiny():
    return _instance(RAW_HP, loudness="bs1770")


KEYS = ("txt_tokens", "note", "note_dur", "note_type")


def test_loud_norm_without_the_keyword_stays_refused():
    with pytest.raises(NotImplementedError, match="loud_norm"):
        _instance(RAW_HP)


@pytest.mark.filterwarnings("ignore:StyleSingerInfer. trim_long_silences skipped")
def test_intake_normalises_what_process_audio_returns_and_leaves_the_emotion_branch(tiny):
    inf, hp = tiny
    n = 33600
    wav = torch.from_numpy(0.2 * _harmonic(n, 48000))[None]
    it = synth.synth_batch(1, 40, 5, 8, hp, 5)
    args = [it[k] for k in KEYS]
    a = inf.preprocess_batch(wav, [n], None, None, *args, mel2ph=it["mel2ph"])
    y, m = LD.normalize_batch(wav.cuda(), [n], 48000)
    assert abs(float(m["lufs"][0]) + 22.0) > 1.0, "the reference is not already at the target"
    by_hand = inf.preprocess_batch(y, [n], None, None, *args, mel2ph=it["mel2ph"], loud_norm=False)
    plain = inf.preprocess_batch(wav, [n], None, None, *args, mel2ph=it["mel2ph"], loud_norm=False)
    for k in ("ref_mels", "ref_f0", "ref_f0_hz", "spk_embed"):
        assert torch.equal(a[k], by_hand[k]), k
    assert not torch.equal(a["ref_mels"], plain["ref_mels"])
    assert torch.equal(a["emo_embed"], plain["emo_embed"]), "preprocess_wav reloads the file: the emotion branch sees the un-normalised audio"
    base = dict(name="t", ph_token=it["txt_tokens"][0].numpy(), note=it["note"][0].numpy(), note_dur=it["note_dur"][0].numpy(),
                note_type=it["note_type"][0].numpy(), mel2ph=it["mel2ph"][0].numpy())
    p = inf.preprocess_input(dict(base, ref_audio=wav[0].numpy()), vad_flags=False)
    assert np.array_equal(p["mel"], a["ref_mels"][0, :n // 256 + 1].cpu().numpy())
    out = inf.infer_once(dict(base, ref_audio=(wav[0].numpy(), 48000)), vad_flags=False)
    assert out.ndim == 1 and len(out) > 0 and np.isfinite(out).all()


def test_intake_with_mixed_rates_equals_the_items_one_by_one(tiny):
    from stylesinger_amd import resample as RS
    inf, hp = tiny
    srs = [44100, 48000, 16000]
    lens = [30870, 33600 - 77, 11200 + 5]
    wav = torch.zeros(3, max(lens))
    for b, (n, sr) in enumerate(zip(lens, srs)):
        wav[b, :n] = torch.from_numpy((0.1, 0.4, 0.25)[b] * _harmonic(n, sr, f0=(196.0, 262.0, 330.0)[b]))
    it = synth.synth_batch(3, 48, 6, 8, hp, 5)
    batch = inf.preprocess_batch(wav, lens, None, None, *[it[k] for k in KEYS], mel2ph=it["mel2ph"], ref_srs=srs)
    for b in range(3):
        one = inf.preprocess_batch(wav[b:b + 1, :lens[b]], [lens[b]], None, None, *[it[k][b:b + 1] for k in KEYS], mel2ph=it["mel2ph"][b:b + 1],
                                   ref_srs=[srs[b]])
        n_mel = RS.out_len(lens[b], srs[b], 48000) // 256 + 1
        for k in ("ref_mels", "ref_f0", "ref_f0_hz"):
            assert torch.equal(batch[k][b, :n_mel], one[k][0, :n_mel]), (b, k)
        for k in ("spk_embed", "emo_embed"):
            assert torch.equal(batch[k][b], one[k][0]), (b, k)


def test_output_target_brings_every_item_to_the_requested_loudness(tiny):
    """Restated loudness of the result over lens * hop samples = the target within 1e-5 LU: one fp32 rounding of the gain (<= 5.2e-7 LU) plus the
    fp32 roundings of the products, which are zero-mean (each <= 2^-24 relative; over >= 19200 samples their effect on a block mean is far below
    1e-6). Where the peak rule fired the loudness is below the target by exactly the clamp 20 log10 P."""
    inf, hp = tiny
    hop = inf.vocoder.model.hop
    batch = {k: v.cuda() for k, v in synth.synth_batch(2, 80, 8, 12, hp, 5).items()}
    plain = inf.infer_batch(batch, seed=3)
    res = inf.infer_batch(batch, seed=3, out_lufs=-16.0)
    assert torch.equal(plain["lens"], res["lens"]) and res["lufs"].shape == (2,) and res["lufs"].dtype == torch.float64
    for b, frames in enumerate(res["lens"].cpu().tolist()):
        n = frames * hop
        assert n >= 0.4 * 48000
        x, y = plain["wav"][b, :n].cpu().numpy(), res["wav"][b, :n].cpu().numpy()
        L_in = loudness_ref(x, 48000)["L"]
        g = np.float32(10.0 ** ((-16.0 - L_in) / 20.0))
        P = np.float32(g * np.float32(np.abs(x).max()))
        want = -16.0 - (20.0 * math.log10(float(P)) if P > 1 else 0.0)
        got = loudness_ref(y, 48000)["L"]
        print(f"item {b}: in {L_in:.6f} LUFS, g32 * peak {P!r}, out {got:.7f} LUFS, wanted {want:.7f}")
        assert abs(float(res["lufs"][b]) - L_in) <= L_TOL
        assert abs(got - want) <= 1e-5
        assert (res["wav"][b, n:] == 0).all()
    short = {k: v.cuda() for k, v in synth.synth_batch(1, 40, 5, 8, hp, 5).items()}   # 40 frames = 10240 samples < one 0.4 s block
    plain = inf.infer_batch(short, seed=3)
    with pytest.warns(UserWarning, match="shorter than one 0.4 s gating block"):
        res = inf.infer_batch(short, seed=3, out_lufs=-16.0)
    n = int(res["lens"][0]) * hop
    assert n < 0.4 * 48000 and math.isnan(float(res["lufs"][0])) and torch.equal(res["wav"][0, :n], plain["wav"][0, :n])
