"""The pitch expression controls without a GPU: the float64 definition `pitch.pitch_edit` against its own stated properties, the argument rules
(`resolve_pitch_edit`, forward, the C entry points), the header, and the key handling of the planner, the producers and the command line.
The window's frequency response is computed from the weights here; no response figure is written down in this file."""
import types

import numpy as np
import pytest

import pitch_edit_cases as C
from stylesinger_amd import abi, config, controls
from stylesinger_amd import lib
from stylesinger_amd import pitch as P

HP = dict(audio_sample_rate=48000, hop_size=256)


def _response(W, hz, fps):
    """|H| of the full window at a modulation frequency, from the weights themselves"""
    w, k = P.edit_weights(W), np.arange(-W, W + 1)
    return abs(np.sum(w * np.exp(-2j * np.pi * hz * k / fps)) / np.sum(w))


def _random_item(rng, n, p_rest=0.1):
    midi = np.repeat(rng.integers(55, 75, n // 9 + 1), 9)[:n].astype(np.int64)
    midi[np.repeat(rng.random(n // 9 + 1) < p_rest, 9)[:n]] = 0
    f = (rng.uniform(6.5, 9.5, n)).astype(np.float32)
    return f, midi


def test_the_neutral_edit_returns_the_input_bits():
    rng = np.random.default_rng(1)
    for W in C.WS:
        f, midi = _random_item(rng, 4000)
        out, stats, _, _ = P.pitch_edit(f, midi, W, 0.0, 1.0)
        assert out.dtype == np.float32 and np.array_equal(out.view(np.int32), f.view(np.int32))
        assert stats[4] < 1e-9 and stats[5] == 0
        out, _, _, _ = P.pitch_edit(f, midi, W, 0.0, 1.0, vibrato=(5.0, 0.0, 3, 2), fps=C.FPS)     # depth 0 is no vibrato
        assert np.array_equal(out.view(np.int32), f.view(np.int32))
    d = C.batch()
    for b, n in enumerate(C.LENS):
        out, _, _, _ = P.pitch_edit(d["f"][b, :n], d["midi"][b, :n], 31)
        assert np.array_equal(out.view(np.int32), d["f"][b, :n].view(np.int32))


def test_full_correction_without_vibrato_is_the_glided_note_target():
    d = C.batch()
    for W in C.WS:
        for b, n in enumerate(C.LENS):
            f, midi = d["f"][b, :n], d["midi"][b, :n]
            out, _, _, _ = P.pitch_edit(f, midi, W, 1.0, 0.0)
            p = P.pitch_edit_parts(f, midi, W, 1.0, 0.0)
            s = p["sung"]
            # m + 1 (nbar - m) + 0 (x - m) is nbar up to one rounding of the sum
            assert np.array_equal(out[~s].view(np.int32), f[~s].view(np.int32))
            assert np.array_equal(out[s], (p["nbar"][s] / 1200.0).astype(np.float32)), (W, b)
            assert np.all(np.abs(p["xe"][s] - p["nbar"][s]) <= 2 * np.spacing(p["nbar"][s]))
    # inside a long held note the target IS the note
    midi = np.full(200, 64, dtype=np.int64)
    p = P.pitch_edit_parts(np.full(200, 8.3, dtype=np.float32), midi, 31, 1.0, 0.0)
    assert np.allclose(p["nbar"], P.EDIT_K0 + 100.0 * (64 - 69), rtol=0, atol=1e-9)
    out, _, _, _ = P.pitch_edit(np.full(200, 8.3, dtype=np.float32), midi, 31, 1.0, 0.0)
    assert np.array_equal(out, np.full(200, np.float32(np.log2(440.0) + (64 - 69) / 12.0)))


def test_flattening_leaves_the_windows_response_at_the_vibrato_rate():
    """On a long constant note with a pure 6 Hz vibrato, kappa = 0 leaves |H(6 Hz)| * depth of it on interior frames: the window is symmetric, so
    a tone comes out scaled by its real response H, computed here from the weights. The tone is given in float64 cents (an fp32 log2 contour
    cannot hold a pure tone: its grid is 6e-4 cents wide there)."""
    W, n, depth, rate = 31, 1200, 50.0, 6.0
    t = np.arange(n)
    base = P.EDIT_K0 + 100.0 * (62 - 69)
    tone = depth * np.sin(2 * np.pi * rate * t / C.FPS)
    p = P.pitch_edit_parts(np.zeros(n, dtype=np.float32), np.full(n, 62, dtype=np.int64), W, 0.0, 0.0, cents=base + tone)
    w, k = P.edit_weights(W), np.arange(-W, W + 1)
    H = np.sum(w * np.cos(2 * np.pi * rate * k / C.FPS)) / np.sum(w)
    assert abs(abs(H) - _response(W, rate, C.FPS)) < 1e-15
    inner = slice(W, n - W)
    assert np.max(np.abs((p["xe"][inner] - base) - H * tone[inner])) < 1e-9          # cents
    assert abs(np.max(np.abs(p["xe"][inner] - base)) - abs(H) * depth) < 1e-3 * abs(H) * depth   # (the samples come that close to the tone's crest)
    assert np.array_equal(p["xe"], p["m"] + 0.0 * (p["nbar"] - p["m"]) + 0.0 * (p["x"] - p["m"]) + 0.0)
    # the trend drops the vibrato band and keeps the melody
    assert all(_response(W, hz, C.FPS) < 0.1 for hz in (5.0, 6.0, 7.0)) and _response(W, 1.0, C.FPS) > 0.9


def test_scale_two_doubles_the_vibrato_exactly():
    d = C.batch()
    f, midi = d["f"][0], d["midi"][0]
    one, two = P.pitch_edit_parts(f, midi, 3, 0.0, 1.0), P.pitch_edit_parts(f, midi, 3, 0.0, 2.0)
    s = one["sung"]
    assert np.array_equal(two["m"], one["m"])
    assert np.array_equal(two["xe"][s], (two["m"] + 2.0 * (two["x"] - two["m"]))[s])          # 2 (x - m) is exact in float64
    assert np.array_equal(2.0 * (one["x"] - one["m"])[s], ((one["x"] - one["m"]) + (one["x"] - one["m"]))[s])


def test_windows_never_cross_a_rest_or_an_item_end():
    d = C.batch()
    for W in C.WS:
        for name, prm in C.PARAMS.items():
            for b, n in enumerate(C.LENS):
                f, midi, u = d["f"][b, :n], d["midi"][b, :n], d["u"][b, :n]
                whole, _, lo, hi = P.pitch_edit(f, midi, W, prm["alpha"], prm["kappa"], prm["vibrato"], u=u, fps=C.FPS)
                sung = midi > 0
                edges = np.flatnonzero(np.diff(np.concatenate([[0], sung.astype(np.int8), [0]])))
                for a, e in zip(edges[::2], edges[1::2]):      # every region on its own
                    part, _, plo, phi = P.pitch_edit(f[a:e], midi[a:e], W, prm["alpha"], prm["kappa"], prm["vibrato"], fps=C.FPS)
                    assert np.array_equal(part.view(np.int32), whole[a:e].view(np.int32)), (W, name, b, a, e)
                    assert np.array_equal(plo + a, lo[a:e]) and np.array_equal(phi + a, hi[a:e])
                assert np.array_equal(whole[~sung].view(np.int32), f[~sung].view(np.int32))


def test_synthetic_vibrato_envelope():
    rate, depth, delay, fade = C.VIB
    omega = P.vibrato_omega(rate, C.FPS)
    assert omega == 2 * np.pi * rate / C.FPS
    need = delay + 2 * fade
    for n, on in ((need - 1, False), (need, True), (need + 37, True)):
        midi = np.concatenate([np.full(n, 60), [0, 0], np.full(5, 62)]).astype(np.int64)
        p = P.pitch_edit_parts(np.full(len(midi), 8.0, dtype=np.float32), midi, 3, 0.0, 1.0, C.VIB, fps=C.FPS)
        s = p["s"]
        assert not s[n:].any()                                    # the rest and the short run
        if not on:
            assert not s.any()
            continue
        o = delay
        assert not s[:o].any() and s[o] == 0.0                    # phase 0 at the onset
        t = np.arange(o, n)
        up, down = np.minimum(1.0, (t - o + 1) / fade), np.minimum(1.0, (n - t) / fade)
        env = up * down
        assert np.array_equal(s[o:n], depth * up * down * np.sin((t - o) * omega))
        assert env[0] == 1.0 / fade and env[-1] == 1.0 / fade and (np.diff(env[:fade]) > 0).all() and (np.diff(env[-fade:]) < 0).all()
        if n >= need + 1:
            assert env.max() == 1.0
        assert np.max(np.abs(s)) <= depth
    # item 0 of the case table: the 27-frame run carries none, the 28-frame run does
    r = C.reference(3, "all")
    p = P.pitch_edit_parts(C.batch()["f"][0], C.batch()["midi"][0], 3, vibrato=C.VIB, fps=C.FPS)
    assert not p["s"][:27].any() and p["s"][27 + delay + 1:55].all() and r["stats"][0, 5] > 0


def test_run_bounds_match_a_scalar_loop():
    d = C.batch()
    rng = np.random.default_rng(3)
    rows = [d["midi"][b, :n] for b, n in enumerate(C.LENS)] + [_random_item(rng, 300, 0.3)[1], np.asarray([128, 127, 200, 0, -3, 5], dtype=np.int64)]
    for midi in rows:
        lo, hi = P.held_runs(midi)
        n = len(midi)
        key = [min(int(m), 127) if m > 0 else 0 for m in midi]
        for t in range(n):
            if key[t] == 0:
                assert lo[t] == -1 and hi[t] == -1
                continue
            a = t
            while a > 0 and key[a - 1] == key[t]:
                a -= 1
            e = t + 1
            while e < n and key[e] == key[t]:
                e += 1
            assert (lo[t], hi[t]) == (a, e)
    lo, hi = P.held_runs(np.asarray([128, 127, 200, 0, -3, 5]))
    assert lo.tolist() == [0, 0, 0, -1, -1, 5] and hi.tolist() == [3, 3, 3, -1, -1, 6]       # 128 and 200 are sung as 127


def test_summation_order_moves_few_frames():
    """What the GPU test's cap on differing frames rests on: the same definition with the window sums in DESCENDING k differs from the ascending one
    in at most 1 % of the sung frames of the case table, and never by more than one fp32 ulp."""
    d, sung = C.batch(), C.sung_mask()
    for W in C.WS:
        for name, prm in C.PARAMS.items():
            differ = total = 0
            for b, n in enumerate(C.LENS):
                if n == 0:
                    continue
                p = P.pitch_edit_parts(d["f"][b, :n], d["midi"][b, :n], W, prm["alpha"], prm["kappa"], prm["vibrato"], fps=C.FPS, descending=True)
                got = (p["xe"] / 1200.0).astype(np.float32)[sung[b, :n]]
                want = C.reference(W, name)["f"][b, :n][sung[b, :n]]
                differ += int((got != want).sum())
                total += len(want)
                assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want)))
            assert differ <= 0.01 * total, (W, name, differ, total)


def test_edit_window_frames():
    assert P.edit_window_frames(333, HP) == 31 and P.edit_window_frames(P.EDIT_SMOOTH_MS, HP) == 31
    assert P.edit_window_frames(0, HP) == 1 and P.edit_window_frames(5, HP) == 1
    assert P.edit_window_frames(333, dict(audio_sample_rate=24000, hop_size=128)) == 31 and P.edit_window_frames(333, dict(audio_sample_rate=24000, hop_size=256)) == 16
    for ms in (100.0, 250.0, 1000.0):
        assert P.edit_window_frames(ms, HP) == max(1, round(ms * 1e-3 * 187.5 / 2))
    with pytest.raises(ValueError):
        P.edit_window_frames(-1, HP)
    w = P.edit_weights(4)
    assert len(w) == 9 and w[4] == 1.0 and np.array_equal(w, w[::-1]) and (w > 0).all() and w.dtype == np.float64
    assert P.EDIT_K0 == 1200.0 * np.log2(440.0)


def test_resolve_pitch_edit_precedence_and_refusals():
    r = P.resolve_pitch_edit
    assert r({}, HP) is None and r(dict(pitch_correct=0.0, vibrato_scale=1.0), HP) is None
    assert r(dict(vibrato_add=(5.0, 0.0)), HP) is None and r(dict(pitch_smooth_ms=100), HP) is None          # depth 0, the window alone: neutral
    got = r(dict(pitch_correct=0.7), HP)
    assert got == dict(W=31, alpha=0.7, kappa=1.0, vibrato=None, fps=187.5)
    got = r(dict(vibrato_add=(5.5, 30.0)), HP)
    assert got["vibrato"] == (5.5, 30.0, round(0.25 * 187.5), round(0.15 * 187.5)) and got["alpha"] == 0.0 and got["kappa"] == 1.0
    assert r(dict(vibrato_add=(5.5, 30.0, 100.0, 0.0)), HP)["vibrato"] == (5.5, 30.0, 19, 1)                # fade_frames >= 1
    hp = dict(HP, pitch_correct=0.5, vibrato_scale=0.0, pitch_smooth_ms=100.0, vibrato_add=None)
    assert r({}, hp) == dict(W=9, alpha=0.5, kappa=0.0, vibrato=None, fps=187.5)                            # hparams win over neutral
    assert r(dict(pitch_correct=0.0, vibrato_scale=1.0), hp) is None                                        # an explicit value wins over hparams
    assert r(dict(vibrato_scale=2.0, pitch_correct=None), hp) == dict(W=9, alpha=0.5, kappa=2.0, vibrato=None, fps=187.5)
    for kw, word in ((dict(pitch_correct=-0.1), "pitch_correct"), (dict(pitch_correct=1.5), "pitch_correct"), (dict(vibrato_scale=-1), "vibrato_scale"),
                     (dict(vibrato_add=(0.0, 30.0)), "rate"), (dict(vibrato_add=(47.0, 30.0)), "rate"), (dict(vibrato_add=(5.0, -1.0)), "depth"),
                     (dict(vibrato_add=(5.0, 1201.0)), "depth"), (dict(vibrato_add=(5.0, 30.0, -1.0)), "times"), (dict(vibrato_add=(5.0, 30.0, 1.0, -2.0)), "times"),
                     (dict(vibrato_add=5.0), "rate_hz, depth_cents"), (dict(pitch_correct=0.5, pitch_smooth_ms=3000.0), "cap"),
                     (dict(pitch_smooth_ms=-5.0), "pitch_smooth_ms")):
        with pytest.raises(ValueError, match=word):
            r(kw, HP)
    assert r(dict(vibrato_add=(187.5 / 4, 30.0)), HP) is not None                                           # the rate bound is inclusive


def test_forward_refuses_bad_edits_before_any_device_work():
    import torch
    from stylesinger_amd.model import StyleSingerHIP
    m = StyleSingerHIP(None, hparams=config.make_hparams(dict(timesteps=2, K_step=2, f0_timesteps=2)))
    m.eval()
    txt = torch.ones(1, 3, dtype=torch.long)
    for kw, word in ((dict(pitch_correct=2.0), "pitch_correct"), (dict(vibrato_scale=-0.5), "vibrato_scale"), (dict(vibrato_add=(0.0, 10.0)), "rate"),
                     (dict(vibrato_add=(5.0, 5000.0)), "depth"), (dict(vibrato_add=(5.0, 50.0, -1.0)), "times"),
                     (dict(pitch_correct=0.5, pitch_smooth_ms=1e5), "cap")):
        with pytest.raises(ValueError, match=word):
            m(txt, infer=True, **kw)
    for k in controls.EDIT_KEYS:
        assert k in config.DEFAULT_HPARAMS and config.DEFAULT_HPARAMS[k] is None


def test_device_wrapper_refuses_host_tensors():
    import torch
    z = torch.zeros(1, 8)
    with pytest.raises(lib.StyleSingerHipError, match="device tensors"):
        P.pitch_edit_device(z, z, z.long(), None, 3, 0.5, 1.0)


def test_header_declares_the_entries_and_the_abi_is_20():
    assert abi.DEFINES["SS_ABI_VERSION"] == 20 and lib.ABI_VERSION == 20
    assert abi.DEFINES["SS_PITCH_EDIT_TILE"] == P.EDIT_TILE == C.TILE and abi.DEFINES["SS_PITCH_EDIT_MAX_W"] == P.EDIT_MAX_W == 255
    runs, edit = abi.PROTOTYPES["ss_pitch_edit_runs"], abi.PROTOTYPES["ss_pitch_edit"]
    assert runs.launch and edit.launch
    assert [p.name for p in runs.params] == ["midi", "ldm", "lens", "run_lo", "run_hi", "T", "B", "stream"]
    names = [p.name for p in edit.params]
    assert names == ["f_in", "ld", "midi", "ldm", "u", "lens", "run_lo", "run_hi", "w", "W", "K0", "alpha", "kappa", "vib_depth", "vib_omega", "vib_delay",
                     "vib_fade", "f_out", "stats_partial", "stats", "T", "B", "stream"]
    by = {p.name: p for p in edit.params}
    assert by["w"].pointee == "double" and by["stats"].pointee == "double" and by["K0"].pointee is None and by["f_out"].pointee == "float"
    assert C.T <= 3 * P.EDIT_TILE + 40 and C.B <= 6


def test_library_exports_and_refuses_without_launching():
    """The C entry points check their arguments before any launch: callable without a device."""
    l = lib.load()
    assert l.ss_abi_version() == 20
    p = 4096   # never dereferenced: every call below is refused by the argument checks

    def edit(W=3, T=64, B=1, ld=64, ldm=64, f_in=p, f_out=2 * p, alpha=0.5, kappa=1.0, depth=0.0, delay=0, fade=1, lo=p, hi=p):
        return l.ss_pitch_edit(f_in, ld, p, ldm, p, p, lo, hi, p, W, P.EDIT_K0, alpha, kappa, depth, 0.1, delay, fade, f_out, p, p, T, B, None)
    for kw, word in ((dict(W=256), b"refused"), (dict(W=0), b"refused"), (dict(f_in=None), b"null pointer"), (dict(T=0), b"bad dims"), (dict(B=0), b"bad dims"),
                     (dict(B=65536), b"bad dims"), (dict(ld=63), b"bad dims"), (dict(ldm=63), b"bad dims"), (dict(f_out=p), b"alias"),
                     (dict(alpha=1.5), b"alpha"), (dict(kappa=-1.0), b"alpha"), (dict(depth=10.0, fade=0), b"vibrato"), (dict(depth=10.0, lo=None), b"vibrato"),
                     (dict(depth=-1.0), b"vibrato")):
        assert edit(**kw) != 0, kw
        err = l.ss_last_error()
        assert b"ss_pitch_edit" in err and word in err, (kw, err)
    for args, word in (((None, 64, p, p, p, 64, 1, None), b"null pointer"), ((p, 63, p, p, p, 64, 1, None), b"bad dims"), ((p, 64, p, p, p, 0, 1, None), b"bad dims")):
        assert l.ss_pitch_edit_runs(*args) != 0
        assert b"ss_pitch_edit_runs" in l.ss_last_error() and word in l.ss_last_error()


def test_planner_producers_and_cli_carry_the_keys_without_ph_dur(capsys, monkeypatch, tmp_path):
    import json
    import torch
    from stylesinger_amd import infer, producers, song
    assert not set(controls.EDIT_KEYS) & set(controls.CONTOUR_KEYS)
    n = 8
    inp = dict(ph_token=list(range(1, n + 1)), note=[60, 62, 0, 64, 65, 0, 67, 69], note_dur=[0.3] * n, note_type=[2, 2, 1, 2, 2, 1, 2, 2],
               pitch_correct=0.8, vibrato_scale=0.5, vibrato_add=[5.5, 30.0], pitch_smooth_ms=250)
    assert song.check_pitch_keys(inp) == []                                           # no ph_dur needed
    plan = song.plan_song(inp, sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    plain = song.plan_song({k: v for k, v in inp.items() if k not in controls.EDIT_KEYS}, sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    assert len(plan.batches) >= 2
    for b, q in zip(plan.batches, plain.batches):
        assert b["pitch_correct"] == 0.8 and b["vibrato_scale"] == 0.5 and b["vibrato_add"] == (5.5, 30.0) and b["pitch_smooth_ms"] == 250.0
        assert not set(controls.EDIT_KEYS) & set(q) and "mel2ph" not in b
    with_dur = song.plan_song(dict(inp, ph_dur=[0.3] * n), sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    assert all(b["pitch_correct"] == 0.8 and "mel2ph" in b for b in with_dur.batches)
    with pytest.raises(ValueError, match="pitch_correct"):
        song.plan_song(dict(inp, pitch_correct=3.0))
    me = types.SimpleNamespace(hparams=HP, device=torch.device("cpu"))
    out = producers.ReferenceProducers._pitch_inputs(me, {"pitch_correct": 1, "vibrato_add": [6, 20, 100]})
    assert out == dict(pitch_correct=1.0, vibrato_add=(6, 20, 100))
    assert producers.ReferenceProducers._pitch_inputs(me, {}) == {}
    with pytest.raises(ValueError, match="vibrato_scale"):
        producers.ReferenceProducers._pitch_inputs(me, {"vibrato_scale": -2})
    # the command line
    base = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"]
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: pytest.fail("a checkpoint was loaded before the flags were checked"))
    for extra, word in ((["--pitch-correct", "1.5"], "pitch_correct"), (["--vibrato-scale", "-1"], "vibrato_scale"), (["--vibrato-add", "0", "30"], "rate"),
                        (["--vibrato-add", "5", "2000"], "depth"), (["--vibrato-delay-ms", "100"], "belongs to --vibrato-add"),
                        (["--vibrato-fade-ms", "100"], "belongs to --vibrato-add"), (["--vibrato-add", "5", "30", "--vibrato-fade-ms", "-1"], "times"),
                        (["--pitch-correct", "0.5", "--pitch-smooth-ms", "9000"], "cap")):
        with pytest.raises(SystemExit) as e:
            infer.main(base + extra)
        assert e.value.code == 2 and word in capsys.readouterr().err, extra
    seen = {}
    monkeypatch.setattr(infer.torch, "load", lambda *a, **k: {})
    monkeypatch.setattr(infer.StyleSingerInfer, "example_run", classmethod(lambda cls, hparams=None, *a, pitch=None, **k: seen.update(pitch=pitch)))
    infer.main(base + ["--pitch-correct", "0.9", "--vibrato-scale", "0", "--vibrato-add", "5.5", "25", "--vibrato-delay-ms", "300", "--pitch-smooth-ms", "200"])
    assert seen["pitch"] == dict(pitch_correct=0.9, vibrato_scale=0.0, vibrato_add=(5.5, 25.0, 300.0, None), pitch_smooth_ms=200.0)
    infer.main(base)
    assert seen["pitch"] == {}
    # --score without ph_dur accepts these flags (and still refuses a contour flag)
    score = dict(ph_token=[1, 2], note=[60, 62], note_dur=[0.3, 0.3], note_type=[2, 2])
    (tmp_path / "s.json").write_text(json.dumps(score))
    monkeypatch.setattr(infer, "_score_run", lambda sc, *a, **k: seen.update(score=sc))
    infer.main(base + ["--score", str(tmp_path / "s.json"), "--pitch-correct", "1", "--vibrato-scale", "0"])
    assert seen["score"]["pitch_correct"] == 1.0 and seen["score"]["vibrato_scale"] == 0.0 and "ph_dur" not in seen["score"]
    np.save(tmp_path / "c.npy", np.full(10, 220.0))
    with pytest.raises(SystemExit):
        infer.main(base + ["--score", str(tmp_path / "s.json"), "--pitch-correct", "1", "--pitch-npy", str(tmp_path / "c.npy")])
    assert "ph_dur" in capsys.readouterr().err
