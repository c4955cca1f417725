"""The on-device true-peak limiter (`ss_limit_true_peak`, csrc/limiter.hip) and the output paths built on it: the kernel against the independent
float64 restatement (tests/limiter_ref.py) within the fp32 forward bound that file derives, the hard conditions exactly (the ceiling, min_gain,
n_limited), padding, gain forms, determinism and batch independence, graph capture, `infer_batch` / `sing_score`. The inputs are
tests/limiter_cases.py's (tests/test_limiter_cpu.py checks on the reference alone that every count is decided). Conformance with a standard
true-peak meter is NOT claimed."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_measurement  # noqa: E402
from limiter_cases import C as CEIL, CEILING_DB, SR, TILE, WINDOWS, cases, gain_case  # noqa: E402
from limiter_ref import limiter_ref  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import limiter as LM  # noqa: E402
from stylesinger_amd import loudness as LD  # noqa: E402

PAD = 37                                   # row stride = widest item + PAD
HARD = float(CEIL) * (1.0 + 2.0 ** -22)    # max |y|: the two fp32 roundings of fl(c / e) and fl(g x')


@functools.lru_cache(maxsize=None)
def _ref(i, W):
    return limiter_ref(cases()[i][1], SR, CEIL, W, with_bound=True)


def _device_input(xs, fill, width=None, pad=PAD):
    """rows strided (ldx > Lx); everything past an item's own samples is `fill` (0, or +-1000 alternating: padding must not leak into a result)"""
    Lx = max(1, max(len(x) for x in xs)) if width is None else width
    buf = torch.zeros(len(xs), Lx + pad)
    if fill:
        buf[:] = fill * (1.0 - 2.0 * (torch.arange(Lx + pad) % 2))
    for b, x in enumerate(xs):
        buf[b, :len(x)] = torch.from_numpy(np.array(x))
    return buf.cuda()[:, :Lx]


def _run(xs, W, fill=0.0, gain=None, **kw):
    xd = _device_input(xs, fill, **kw)
    y, rep = LM.limit_batch(xd, [len(x) for x in xs], SR, CEILING_DB, W=W, gain=gain, with_gain_curve=True)
    return y, rep


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _check_item(name, ref, y, g, min_gain, n_limited):
    """one item against its restatement -> the worst err / bound of g and of y"""
    n = len(ref["g"])
    yd, gd = y[:n].astype(np.float64), g[:n].astype(np.float64)
    assert np.isfinite(y).all() and (y[n:] == 0.0).all(), (name, "exact zeros past the item's length")
    eg, ey = np.abs(gd - ref["g"]), np.abs(yd - ref["y"])
    assert (eg <= ref["dg"]).all(), (name, float(eg.max()))
    assert (ey <= ref["dy"]).all(), (name, float(ey.max()))
    assert np.abs(yd).max(initial=0.0) <= HARD, (name, float(np.abs(yd).max()))
    assert np.array_equal(_bits(y[:n]), _bits(g[:n] * ref["xp"])), (name, "y = fl32(g x')")
    assert _bits(min_gain) == _bits(g[:n].min() if n else 1.0), (name, "min_gain is the minimum of the device's own g, bit for bit")
    assert ref["decided"], name
    assert int(n_limited) == ref["n_limited"] == int((g[:n] < 1.0).sum()), (name, int(n_limited), ref["n_limited"])
    fr = lambda e, b: float((e[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0
    return fr(eg, ref["dg"]), fr(ey, ref["dy"])


@pytest.mark.parametrize("W", WINDOWS)
def test_kernel_matches_the_float64_restatement_within_the_fp32_forward_bound(W):
    """|g_dev - g_ref| <= dg and |y_dev - y_ref| <= dy per sample (the bound of tests/limiter_ref.py: the fp32 forward error of the 127-term
    banked sums carried through c / e, the window minimum and the W-term mean), and exactly: max |y| <= c (1 + 2^-22), y = fl32(g x'),
    min_gain = min g bit for bit, n_limited = the reference's count, zeros past n. All lengths and peak placements in one ragged batch with
    ldx > Lx; run twice, with zeros and with +-1000 past every item's end: bit-identical.
    Measured on an MI355X (recorded, profiles/limiter_parity.json): worst err / bound of g and y 0.07 / 0.07 at W = 1,
    0.06 / 0.07 at W = 2, 0.19 / 0.19 at W = 96, 0.23 / 0.20 at W = 512."""
    xs = [x for _, x in cases()]
    y0, rep0 = _run(xs, W, fill=0.0)
    y1, rep1 = _run(xs, W, fill=1000.0)
    assert y0.stride(0) == y0.shape[1] and y0.shape[1] == max(len(x) for x in xs)
    for k in ("min_gain", "n_limited", "g"):
        assert torch.equal(rep0[k], rep1[k]), (k, "what the buffer holds past n[b] is never read into a result")
    assert torch.equal(y0, y1)
    y, g, mg, nl = y0.cpu().numpy(), rep0["g"].cpu().numpy(), rep0["min_gain"].cpu().numpy(), rep0["n_limited"].cpu().numpy()
    worst_g = worst_y = 0.0
    for i, (name, x) in enumerate(cases()):
        fg, fy = _check_item(name, _ref(i, W), y[i], g[i], mg[i], nl[i])
        print(f"W {W:3d} {name:18s} n {len(x):5d}: n_limited {nl[i]:5d} min_gain {mg[i]:.6f}  worst err / bound: g {fg:.4f}  y {fy:.4f}")
        worst_g, worst_y = max(worst_g, fg), max(worst_y, fy)
        assert (g[i, len(x):] == 1.0).all()
    names = [n for n, _ in cases()]
    q = names.index("quiet")
    assert nl[q] == 0 and mg[q] == 1.0 and np.array_equal(_bits(y[q, :len(xs[q])]), _bits(xs[q])), "a signal that fits passes untouched, bit for bit"
    assert nl[names.index("loud")] == len(xs[names.index("loud")]) and (W < 2 or nl[names.index("sine_fs4")] == 3000), "limited (almost) everywhere"
    assert nl[names.index("len_0")] == 0 and mg[names.index("len_0")] == 1.0
    record_measurement(f"limiter_device_vs_float64_restatement_W_{W}", pinned=False, worst_g_err_over_bound=worst_g, worst_y_err_over_bound=worst_y,
                       items=len(xs), ceiling_db=CEILING_DB, rate=SR)


def test_gain_forms_null_ones_and_a_measured_loudness_gain():
    xs = [x for _, x in cases()]
    W = 96
    a, ra = _run(xs, W)
    b, rb = _run(xs, W, gain=torch.ones(len(xs), device="cuda"))
    assert torch.equal(a, b) and all(torch.equal(ra[k], rb[k]) for k in ("g", "min_gain", "n_limited")), "gain = NULL is gain = 1"
    # a per-item gain from a real ss_loudness_measure call: the limiter takes what the meter wrote, no peak rule in between
    x2, target, g_host = gain_case()
    xd = _device_input(x2, 1000.0)
    lens = [len(x) for x in x2]
    m = LD.measure_batch(xd, lens, SR, target=target)
    gains = m["gain"].cpu().numpy()
    y, rep = LM.limit_batch(xd, lens, SR, CEILING_DB, W=W, gain=m["gain"], with_gain_curve=True)
    y, g, mg, nl = y.cpu().numpy(), rep["g"].cpu().numpy(), rep["min_gain"].cpu().numpy(), rep["n_limited"].cpu().numpy()
    for b_, x in enumerate(x2):
        assert abs(int(_bits(gains[b_])) - int(_bits(g_host[b_]))) <= 1, "the meter's gain within 1 ulp of the host's"
        assert gains[b_] * np.abs(x).max() > 1.0, "the peak rule would have fired"
        ref = limiter_ref(x, SR, CEIL, W, gain=gains[b_], with_bound=True)
        fg, fy = _check_item(f"gain_{b_}", ref, y[b_], g[b_], mg[b_], nl[b_])
        print(f"measured gain {gains[b_]!r} (host {g_host[b_]!r}): n_limited {nl[b_]} min_gain {mg[b_]:.6f}  worst err / bound: g {fg:.4f}  y {fy:.4f}")
        assert 0 < nl[b_] < len(x)


def test_limiter_is_deterministic_and_independent_of_the_batch():
    xs = [x for _, x in cases()]
    names = [n for n, _ in cases()]
    for W in (96, LM.LIMIT_MAX_W):
        a, ra = _run(xs, W)
        b, rb = _run(xs, W)
        assert torch.equal(a, b) and all(torch.equal(ra[k], rb[k]) for k in ("g", "min_gain", "n_limited")), "a second time"
        for name in (f"len_{2 * TILE + 517}", "peak_both_sides", f"len_{TILE + 1}"):
            i = names.index(name)
            n = len(xs[i])
            one, r1 = _run([xs[i]], W, fill=1000.0, width=n + 5, pad=3)     # alone: another B, Lx, ldx and ldy (an odd one: the scalar stores)
            assert torch.equal(one[0, :n], a[i, :n]) and torch.equal(r1["g"][0, :n], ra["g"][i, :n]), (W, name)
            assert torch.equal(r1["min_gain"][0], ra["min_gain"][i]) and torch.equal(r1["n_limited"][0], ra["n_limited"][i])


def test_limit_batch_is_graph_capturable():
    xs = [x for _, x in cases()]
    xd = _device_input(xs, 0.0)
    lens = [len(x) for x in xs]
    eager, re_ = LM.limit_batch(xd, lens, SR, CEILING_DB)     # (also uploads the bank and the length vector once)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        out, ro = LM.limit_batch(xd, lens, SR, CEILING_DB)
    out.fill_(float("nan"))
    ro["n_limited"].fill_(-1)
    gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(ro["n_limited"], re_["n_limited"]) and torch.equal(ro["min_gain"], re_["min_gain"])


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def singer():
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    inf = StyleSingerInfer(hp, device=torch.device("cuda:0"), model_state=synth.synth_acoustic_state_dict(hp, 5),
                           vocoder_state=synth.synth_vocoder_state_dict(None, 11))
    inf.model.use_graphs = "off"
    return inf, hp


def test_infer_batch_applies_the_loudness_gain_in_full_and_meets_the_ceiling(singer):
    inf, hp = singer
    hop = inf.vocoder.model.hop
    batch = {k: v.cuda() for k, v in synth.synth_batch(2, 80, 8, 12, hp, 5).items()}
    plain = inf.infer_batch(batch, seed=3)
    lens = [int(v) * hop for v in plain["lens"].cpu()]
    assert min(lens) >= 0.4 * SR
    for target in (-14.0, None):
        m = LD.measure_batch(plain["wav"], lens, SR, target=-14.0 if target is None else target)
        if target is None:   # a target that surely asks for more than the ceiling allows: gain * peak = 2 for item 0
            lufs0, peak0 = float(m["lufs"][0]), float(m["peak"][0])
            target = lufs0 + 20.0 * np.log10(2.0 / peak0)
            m = LD.measure_batch(plain["wav"], lens, SR, target=target)
            assert float(m["gain"][0] * m["peak"][0]) > 1.9
        res = inf.infer_batch(batch, seed=3, out_lufs=target, out_true_peak_db=-1.0)
        assert torch.equal(res["loudness_gain"], m["gain"]) and torch.equal(res["lufs"], m["lufs"]), "the gain the meter reports, not divided by a peak"
        want, rep = LM.limit_batch(plain["wav"], lens, SR, -1.0, gain=m["gain"])
        assert torch.equal(res["wav"], want) and torch.equal(res["limiter"]["n_limited"], rep["n_limited"])
        assert res["limiter"]["min_gain"].shape == (2,) and res["limiter"]["n_limited"].dtype == torch.int32
        peak = res["wav"].abs().amax(dim=1).cpu().numpy().astype(np.float64)
        fired = (m["gain"] * m["peak"] > 1).cpu().tolist()
        print(f"target {target:.3f} LUFS: gain {m['gain'].cpu().tolist()}, gain * peak > 1: {fired}, output sample peak {peak}, "
              f"n_limited {res['limiter']['n_limited'].cpu().tolist()}, min_gain {res['limiter']['min_gain'].cpu().tolist()}")
        assert (peak <= float(LM.ceiling_f32(-1.0)) * (1.0 + 2.0 ** -22)).all()
        for b in range(2):
            n = lens[b]
            if not fired[b] and int(res["limiter"]["n_limited"][b]) == 0:   # nothing to limit: the gain alone, bit for bit
                assert torch.equal(res["wav"][b, :n], (m["gain"][b] * plain["wav"][b, :n]))
            assert (res["wav"][b, n:] == 0).all()
    assert int(res["limiter"]["n_limited"][0]) > 0 and float(res["limiter"]["min_gain"][0]) < 1.0
    # without a loudness target the limiter runs on the waveform as synthesised
    res = inf.infer_batch(batch, seed=3, out_true_peak_db=-30.0)
    want, rep = LM.limit_batch(plain["wav"], lens, SR, -30.0)
    assert torch.equal(res["wav"], want) and "lufs" not in res and "loudness_gain" not in res
    assert float(res["wav"].abs().max()) <= float(LM.ceiling_f32(-30.0)) * (1.0 + 2.0 ** -22)


def test_default_path_is_bit_identical_without_the_limiter(singer):
    inf, hp = singer
    batch = {k: v.cuda() for k, v in synth.synth_batch(2, 80, 8, 12, hp, 5).items()}
    res = inf.infer_batch(batch, seed=3, out_lufs=None, out_true_peak_db=None)
    assert "limiter" not in res and "lufs" not in res and "loudness_gain" not in res
    bare = inf.infer_batch(batch, seed=3, vocode=False)
    wav = inf.vocode(bare["mel"], bare["f0"], bare["lens"], seed=3 + 101)   # the vocoder's output, nothing after it
    assert torch.equal(res["wav"], wav)
    hop = inf.vocoder.model.hop
    lens = [int(v) * hop for v in res["lens"].cpu()]
    loud = inf.infer_batch(batch, seed=3, out_lufs=-16.0)     # the loudness target alone keeps its peak rule
    y, lufs = inf._to_lufs(wav, lens, -16.0)
    assert torch.equal(loud["wav"], y) and torch.equal(loud["lufs"], lufs) and "limiter" not in loud


def test_sing_score_limits_the_whole_song_once(singer):
    inf, hp = singer
    ref = synth.synth_utterance(0, 8, 4, 50, hp, 5)
    feats = dict(mel=ref["ref_mels"].numpy(), f0=np.exp2(ref["ref_f0"].numpy().astype(np.float64)), spk_embed=ref["spk_embed"].numpy(),
                 emo_embed=ref["emo_embed"].numpy())
    rng = np.random.default_rng(1)
    tok, note, typ, ndur, pdur = [], [], [], [], []
    for n, fr in zip((5, 3, 6), (40, 22, 51)):     # three phrases, each closed by a rest
        w = rng.uniform(0.5, 1.5, n)
        pdur += (w / w.sum() * fr * 256 / 48000).tolist()
        tok += rng.integers(3, 60, n).tolist()
        note += rng.integers(50, 75, n - 1).tolist() + [0]
        typ += [2] * (n - 1) + [1]
        ndur += rng.uniform(0.1, 0.4, n).tolist()
    sc = dict(ph_token=tok, note=note, note_type=typ, note_dur=ndur, ph_dur=pdur, **feats)
    kw = dict(max_seconds=65 * 256 / 48000, segment_batch=2, seed=7)
    plain = inf.sing_score(sc, **kw)
    assert len(plain["segments"]) >= 2 and "limiter" not in plain
    N = plain["wav"].numel()
    ceiling = min(-1.0, 20.0 * np.log10(0.5 * float(plain["wav"].abs().max())))     # at most half the song's own peak: something to limit
    out = inf.sing_score(sc, out_true_peak_db=ceiling, **kw)
    want, rep = LM.limit_batch(plain["wav"][None], [N], SR, ceiling)
    assert torch.equal(out["wav"], want[0]), "the whole song after the stitch, never per segment"
    assert out["limiter"]["n_limited"].shape == (1,) and torch.equal(out["limiter"]["n_limited"], rep["n_limited"])
    assert 0 < int(out["limiter"]["n_limited"][0]) and float(out["wav"].abs().max()) <= float(LM.ceiling_f32(ceiling)) * (1.0 + 2.0 ** -22)
    assert torch.equal(out["mel"], plain["mel"]) and out["segments"] == plain["segments"]
    inf.hparams["out_true_peak_db"] = ceiling                  # the hparams form of the same ceiling
    try:
        assert torch.equal(inf.sing_score(sc, **kw)["wav"], out["wav"])
    finally:
        inf.hparams["out_true_peak_db"] = None


def test_example_run_writes_a_file_under_the_ceiling_with_the_loudness_gain_in_full(tmp_path):
    """what `python -m stylesinger_amd.infer ... --out-lufs -14 --out-true-peak -1` does once the checkpoints are loaded (synthetic weights here): the
    file's sample peak is at or under -1 dBFS and the waveform is the plain run's times the meter's gain, limited - not divided by its peak"""
    import json
    import os
    import wave
    from stylesinger_amd.infer import StyleSingerInfer
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "token_encoder.json")))
    ps = tmp_path / "phone_set.json"
    ps.write_text(json.dumps(gold["phone_set"]))
    t = np.arange(256 * 300) / SR
    ph = 2 * np.pi * 220.0 * t + 0.3 * np.sin(2 * np.pi * 5.0 * t)
    ref = tmp_path / "ref.wav"
    with wave.open(str(ref), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(SR)
        wf.writeframes(np.round(sum(0.2 / h * np.sin(h * ph + 0.3 * h) for h in range(1, 9)) * 32767).astype("<i2").tobytes())
    base = dict(timesteps=3, K_step=3, f0_timesteps=3)

    def run(name, **extra):
        hp = config.make_hparams(dict(base, **extra))
        return StyleSingerInfer.example_run(hp, str(ref), str(tmp_path / name), vad_flags=False, device=torch.device("cuda:0"),
                                            model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 5),
                                            emotion_state=synth.synth_emotion_state_dict(5), speaker_state=synth.synth_emotion_state_dict(6),
                                            phone_set=str(ps))
    plain = run("plain.wav")
    out = run("limited.wav", out_loudness_lufs=-14.0, out_true_peak_db=-1.0)
    n = len(plain)
    assert len(out) == n and n >= 0.4 * SR
    xd = torch.from_numpy(np.ascontiguousarray(plain, dtype=np.float32))[None].cuda()
    m = LD.measure_batch(xd, [n], SR, target=-14.0)
    want, rep = LM.limit_batch(xd, [n], SR, -1.0, gain=m["gain"])
    assert np.array_equal(_bits(out), _bits(want[0].cpu().numpy())), "the meter's gain in full, then the limiter"
    c = float(LM.ceiling_f32(-1.0))
    with wave.open(str(tmp_path / "limited.wav"), "rb") as wf:
        pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")
    print(f"example run: gain {float(m['gain'][0]):.4f}, gain * peak {float(m['gain'][0] * m['peak'][0]):.4f}, n_limited {int(rep['n_limited'][0])} of {n}, "
          f"file peak {np.abs(pcm.astype(np.int32)).max() / 32767:.6f} (ceiling {c:.6f})")
    assert len(pcm) == n and np.abs(pcm.astype(np.int32)).max() <= c * (1.0 + 2.0 ** -22) * 32767
    # a target this item's crest factor does not fit under (gain * peak = 2): the peak rule would halve it, the limiter keeps the gain
    hot = -14.0 + 20.0 * np.log10(2.0 / float(m["gain"][0] * m["peak"][0]))
    out = run("hot.wav", out_loudness_lufs=hot, out_true_peak_db=-1.0)
    m = LD.measure_batch(xd, [n], SR, target=hot)
    want, rep = LM.limit_batch(xd, [n], SR, -1.0, gain=m["gain"])
    assert float(m["gain"][0] * m["peak"][0]) > 1.9 and 0 < int(rep["n_limited"][0])
    assert np.array_equal(_bits(out), _bits(want[0].cpu().numpy()))
    untouched = LM.limit_batch(xd, [n], SR, -1.0, gain=m["gain"], with_gain_curve=True)[1]["g"][0, :n] == 1.0
    assert torch.equal(want[0, :n][untouched], (m["gain"][0] * xd[0, :n])[untouched]), "where the limiter does nothing, the full loudness gain"
    with wave.open(str(tmp_path / "hot.wav"), "rb") as wf:
        pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")
    print(f"hot target {hot:.3f} LUFS: n_limited {int(rep['n_limited'][0])} of {n}, file peak {np.abs(pcm.astype(np.int32)).max() / 32767:.6f}")
    assert np.abs(pcm.astype(np.int32)).max() <= c * (1.0 + 2.0 ** -22) * 32767 and np.abs(pcm.astype(np.int32)).max() >= 0.99 * c * 32767
