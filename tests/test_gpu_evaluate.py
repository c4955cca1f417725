"""The objective metrics on the GPU: every kernel of csrc/evaluate.hip against its definition (stylesinger_amd/evaluate.py) - q, path, plen, cost,
status and the four counts exact, the two float64 sums within derived bounds, the cosine within 2 fp32 ulp - and `score_wavs` /
`StyleSingerInfer.evaluate` end to end on synthetic audio.

Every kernel case runs twice: in buffers of the items' own size and in larger ones whose padding holds values a kernel that read it would show
(+-1000 in q, NaN in mel and f0); the two results must be bit-identical and equal to the definition."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import evaluate_cases as K  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import evaluate as E  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -52                # float64: ulp(x) <= U * |x|
LOG2_ULP = 1.0                # documented maximum error of the device's float64 log2, in ulp (HIP math API: log2, double precision)
SQRT_ULP = 1.0                # ... and of its float64 sqrt


# ---- launch helpers -------------------------------------------------------------------------------------------------------------------------------------
def _q_buffer(items, T, fill):
    Kp = items[0].shape[1]
    buf = np.full((len(items), T, Kp), fill, dtype=np.int16)
    for b, q in enumerate(items):
        buf[b, :len(q)] = q
    return torch.from_numpy(buf).to(DEV)


def _f0_buffer(items, T, extra):
    buf = np.full((len(items), T + extra), np.nan, dtype=np.float32)
    for b, f in enumerate(items):
        buf[b, :len(f)] = f
    return torch.from_numpy(buf).to(DEV)[:, :T]               # a view: row stride T + extra


def _align(qas, qbs, band, pad):
    """One launch pair over the batch, frame axes padded by `pad` = (extra rows of a, extra rows of b, fill) -> numpy results + the device dict"""
    ea, eb, fill = pad
    Ta, Tb = max(1, max(len(q) for q in qas)) + ea, max(1, max(len(q) for q in qbs)) + eb
    qa, qb = _q_buffer(qas, Ta, fill), _q_buffer(qbs, Tb, -fill)
    al = E.align_device(qa, [len(q) for q in qas], qb, [len(q) for q in qbs], band)
    torch.cuda.synchronize()
    plen = al["plen"].cpu().numpy()
    paths = [al["path"][b, :plen[b]].cpu().numpy() for b in range(len(qas))]
    return dict(paths=paths, plen=plen, cost=al["cost"].cpu().numpy(), status=al["status"].cpu().numpy(), dev=al, qa=qa, qb=qb)


def _reduce(run, f0as, f0bs, use_path):
    qa, qb, al = run["qa"], run["qb"], run["dev"]
    fa, fb = _f0_buffer(f0as, qa.shape[1], 3), _f0_buffer(f0bs, qb.shape[1], 5)
    counts, sums = E.reduce_device(qa, fa, al["lens_a"], qb, fb, al["lens_b"], al["path"] if use_path else None, al["plen"] if use_path else None)
    torch.cuda.synchronize()
    return counts.cpu().numpy(), sums.cpu().numpy()


PADS = ((0, 0, 1000), (5, 9, -1000))
WORST = dict(dist=0.0, cents=0.0)     # the largest measured share of each sum's bound (printed by the tests that feed it)


def _check_sums(got_counts, got_sums, want):
    assert [int(v) for v in got_counts] == [want["P"], want["n_both"], want["n_vde"], want["n_gpe"]]
    P = want["P"]
    # dist_sum: non-negative terms, every sqrt within SQRT_ULP ulp, at most P - 1 roundings of partial sums that never exceed the total
    bar_d = P * max(SQRT_ULP, 1.0) * U * want["dist_sum"]
    # cents_sq_sum: per term the log2 (LOG2_ULP ulp on the device, <= 1 on the host), the product with 1200 and the square (one rounding each; the
    # division is the same correctly rounded operation on both sides): (1 + 2 (LOG2_ULP + 1) + ...) < 8 ulp, + the roundings of the summation
    bar_c = (8 * max(LOG2_ULP, 1.0) + 2 * P) * U * want["cents_sq_sum"]
    ed, ec = abs(got_sums[0] - want["dist_sum"]), abs(got_sums[1] - want["cents_sq_sum"])
    if bar_d > 0:
        WORST["dist"] = max(WORST["dist"], ed / bar_d)
    if bar_c > 0:
        WORST["cents"] = max(WORST["cents"], ec / bar_c)
    assert ed <= bar_d and ec <= bar_c, (ed, bar_d, ec, bar_c)


def _check_items(qas, qbs, band, want_status=None, f0_seed=0):
    """align + reduce of the batch in both paddings against the definition, item by item; -> the first run"""
    rng = np.random.default_rng(f0_seed)
    f0as, f0bs = [K.random_f0(rng, len(q)) for q in qas], [K.random_f0(rng, len(q)) for q in qbs]
    want = [E.dtw_path(a, b, band) for a, b in zip(qas, qbs)]
    runs = [_align(qas, qbs, band, pad) for pad in PADS]
    reds = [(_reduce(r, f0as, f0bs, True), _reduce(r, f0as, f0bs, False)) for r in runs]
    for b, (w_path, w_P, w_cost, w_status) in enumerate(want):
        for r in runs:
            assert r["status"][b] == w_status and r["plen"][b] == w_P and r["cost"][b] == w_cost, (b, r["status"][b], w_status, r["plen"][b], w_P, r["cost"][b], w_cost)
            assert np.array_equal(r["paths"][b], w_path), b
        if want_status is not None:
            assert w_status == want_status[b]
        on_path = E.path_metrics(qas[b], qbs[b], f0as[b], f0bs[b], w_path)
        on_ident = E.path_metrics(qas[b], qbs[b], f0as[b], f0bs[b], E.identity_path(len(qas[b]), len(qbs[b])))
        for (cp, sp), (ci, si) in reds:
            _check_sums(cp[b], sp[b], on_path)
            _check_sums(ci[b], si[b], on_ident)
    for (cp, sp), (ci, si) in reds[1:]:                        # the two paddings: bit-identical
        assert np.array_equal(cp, reds[0][0][0]) and np.array_equal(sp, reds[0][0][1]) and np.array_equal(ci, reds[0][1][0]) and np.array_equal(si, reds[0][1][1])
    return runs[0]


# ---- 1. ss_eval_mcep ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Kc", [1, 13, 24])
@pytest.mark.parametrize("n_mels", [80, 7])
@pytest.mark.parametrize("T", [1, 5, 70])
def test_mcep_equals_the_float32_restatement(T, n_mels, Kc):
    rng = np.random.default_rng(100 * T + n_mels + Kc)
    lens = {1: [1, 0, 1], 5: [5, 3, 0], 70: [70, 33, 64]}[T]
    mels = [K.wide_mel(rng, n, n_mels) if b else K.corner_mel(rng, n, n_mels) for b, n in enumerate(lens)]
    hp = dict(mel_vmin=K.VMIN, mel_vmax=K.VMAX)
    got = []
    for et, ec, fill in ((0, 0, np.nan), (3, 5, 1000.0)):
        buf = np.full((3, T + et, n_mels + ec), fill, dtype=np.float32)
        for b, m in enumerate(mels):
            buf[b, :len(m), :n_mels] = m
        q = E.mcep_q_device(torch.from_numpy(buf).to(DEV)[:, :, :n_mels], lens, hp, K=Kc)       # a view: frame stride n_mels + ec
        torch.cuda.synchronize()
        q = q.cpu().numpy()
        Kp = (Kc + 1) // 2 * 2
        assert q.shape == (3, T + et, Kp) and q.dtype == np.int16
        for b, m in enumerate(mels):
            want = E.mcep_q(m, len(m), K=Kc, vmin=K.VMIN, vmax=K.VMAX)
            assert np.array_equal(q[b, :len(m)], want), (b, np.abs(q[b, :len(m)].astype(int) - want).max())
            assert not q[b, len(m):].any()                  # rows past lens ...
        if Kp > Kc:
            assert not q[:, :, Kc:].any()                   # ... and the pad column are 0
        got.append(q[:, :T])
    assert np.array_equal(got[0], got[1])


# ---- 2. ss_eval_cost_band + ss_eval_dtw + ss_eval_reduce ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["ties", "random"])
@pytest.mark.parametrize("n_a,n_b,band", K.SHAPES)
def test_path_and_sums_equal_the_definition(n_a, n_b, band, content):
    rng = np.random.default_rng(1000 * n_a + n_b + (7 if content == "ties" else 0))
    make = K.tie_q if content == "ties" else K.random_q
    _check_items([make(rng, n_a)], [make(rng, n_b)], band, want_status=[0], f0_seed=n_a)
    print(f"{n_a} x {n_b} band {band} {content}: worst share of the bounds so far: dist_sum {WORST['dist']:.3f}, cents_sq_sum {WORST['cents']:.3f}")


def test_the_largest_legal_distances_through_the_cepstrum_kernel():
    """q of corner-valued mels (every bin at an end of the clip range) through ss_eval_mcep: the largest S and cost the definition allows."""
    rng = np.random.default_rng(21)
    hp = dict(mel_vmin=K.VMIN, mel_vmax=K.VMAX)
    ma, mb = K.corner_mel(rng, 70), K.corner_mel(rng, 75)
    qa = E.mcep_q_device(torch.from_numpy(ma).to(DEV)[None], None, hp)[0].cpu().numpy()
    qb = E.mcep_q_device(torch.from_numpy(mb).to(DEV)[None], None, hp)[0].cpu().numpy()
    assert np.array_equal(qa, E.mcep_q(ma)) and np.array_equal(qb, E.mcep_q(mb))
    assert E.sq_dist_matrix(qa, qb).max() > 3e7
    # K = 2 coefficients in a two-column q: the shortest row the packed dot product takes, and an odd dword count per row is not needed
    for band in (None, 8):
        run = _check_items([qa], [qb], band, want_status=[0])
        assert run["cost"][0] > 70 * 3000
    _check_items([qa[:, :2].copy()], [qb[:, :2].copy()], None, want_status=[0])
    _check_items([qa[:, :14].copy()], [qb[:, :14].copy()], 8, want_status=[0])


def test_a_batch_of_ragged_items_one_of_them_not_aligned():
    rng = np.random.default_rng(4)
    qas = [K.tie_q(rng, 20), K.random_q(rng, 3), K.random_q(rng, 41)]
    qbs = [K.tie_q(rng, 33), K.random_q(rng, 50), K.random_q(rng, 29)]
    _check_items(qas, qbs, None, want_status=[0, 0, 0])
    run = _check_items(qas, qbs, 6, want_status=[0, 1, 0])     # 50 > 6 * 3
    for b in (0, 2):                                           # row b of the batch = the item alone
        one = _align([qas[b]], [qbs[b]], 6, PADS[0])
        assert np.array_equal(one["paths"][0], run["paths"][b]) and one["cost"][0] == run["cost"][b] and one["status"][0] == run["status"][b]
    qas[1] = qas[1][:0]                                        # an empty item: status 1, no path, no frames
    run = _check_items(qas, qbs, None, want_status=[0, 1, 0])
    assert run["plen"][1] == 0


def test_a_long_item_in_a_band():
    rng = np.random.default_rng(5)
    _check_items([K.tie_q(rng, 1500)], [K.tie_q(rng, 1400)], 64, want_status=[0])


def test_entries_refuse_on_the_device_and_write_nothing():
    l = L.load()
    q = torch.zeros(1, 8, 24, dtype=torch.int16, device=DEV)
    lens = torch.tensor([8], dtype=torch.int32, device=DEV)
    ws = torch.zeros(192, dtype=torch.uint8, device=DEV)
    path = torch.full((1, 16, 2), -7, dtype=torch.int32, device=DEV)
    plen, cost, st = (torch.full((1,), -7, dtype=torch.int32, device=DEV) for _ in range(3))
    assert l.ss_eval_dtw(L.ptr(lens), L.ptr(lens), 0, L.ptr(path), L.ptr(plen), L.ptr(cost), L.ptr(st), 8, 8, 1, L.ptr(ws), 191, L.stream_ptr()) != 0
    assert b"ss_eval_dtw" in l.ss_last_error() and b"workspace" in l.ss_last_error()
    assert l.ss_eval_cost_band(L.ptr(q), L.ptr(lens), L.ptr(q), L.ptr(lens), 24, 0, 8, 8, 1, L.ptr(ws), 191, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert (path == -7).all() and plen.item() == -7 and cost.item() == -7 and st.item() == -7 and not ws.any()
    with pytest.raises(ValueError, match="cap"):
        E.align_device(torch.zeros(1, E.EVAL_MAX_T + 1, 2, dtype=torch.int16, device=DEV), None, torch.zeros(1, 8, 2, dtype=torch.int16, device=DEV), None)
    with pytest.raises(ValueError, match="EVAL_MAX_WORKSPACE_BYTES"):     # 32 full items at the cap: 6 GiB
        E.align_device(torch.zeros(32, E.EVAL_MAX_T, 2, dtype=torch.int16, device=DEV), None, torch.zeros(32, E.EVAL_MAX_T, 2, dtype=torch.int16, device=DEV), None)


# ---- 3. ss_cosine_rows ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 256])
def test_cosine_rows(C):
    rng = np.random.default_rng(C)
    a = rng.standard_normal((6, C)).astype(np.float32)
    b = rng.standard_normal((6, C)).astype(np.float32)
    b[0] = a[0]                                                # equal
    b[1] = -a[1]                                               # opposite
    if C > 1:                                                  # orthogonal: disjoint supports
        a[2, C // 2:] = 0
        b[2, :C // 2] = 0
    b[3] = 0                                                   # a zero row has no direction: 0
    got = E.cosine_rows_device(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
    want = np.asarray([E.singer_cos(x, y) for x, y in zip(a, b)])
    ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), 2.0 ** -126).astype(np.float32))
    print(f"C = {C}: cosine worst {ulp.max():.3f} fp32 ulp of the float64 value")
    assert (ulp <= 2).all() and got[3] == 0
    assert got[0] == 1.0 and got[1] == -1.0
    if C > 1:
        assert got[2] == 0


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------------------------------
SR, HOP = 48000, 256


def _sung(f0, n, seed=0):
    """an eight-harmonic complex (tests/f0track_stage_refs.py::_complex) under a slow amplitude envelope, with a little noise"""
    t = np.arange(n) / float(SR)
    w = sum(0.25 / h * np.sin(2 * np.pi * f0 * h * t + 0.3 * h) for h in range(1, 9)) * (0.7 + 0.3 * np.sin(2 * np.pi * 2.0 * t))
    return (w + 0.001 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def front():
    from stylesinger_amd.frontend import MelFrontendHIP
    return MelFrontendHIP(None, device=DEV)


def _wavs(items, extra=0, fill=np.nan):
    L_ = max(len(w) for w in items) + extra
    buf = np.full((len(items), L_), fill, dtype=np.float32)
    for b, w in enumerate(items):
        buf[b, :len(w)] = w
    return torch.from_numpy(buf).to(DEV), [len(w) for w in items]


def test_an_item_against_itself_scores_zero(front):
    a = [_sung(220.0, 60 * HOP), _sung(330.0, 47 * HOP + 100, 1)]
    res = None
    for extra, fill in ((0, 0.0), (700, np.nan)):              # what follows an item's samples in the buffer does not matter
        wa, la = _wavs(a, extra, fill)
        r = E.score_wavs(front, wa, la, wa.clone(), la)
        assert r["status"].cpu().tolist() == [0, 0] and r["cost"].cpu().tolist() == [0, 0] and r["plen"].cpu().tolist() == [61, 48]
        for k in E.DERIVED:
            assert (r[k] == 0).all(), k
        assert r["counts"][:, 1].min().item() >= 20            # most frames are voiced on both sides: the zeros above mean something
        assert "singer_cos" not in r and r["frames_a"] == [61, 48]
        if res is not None:
            assert torch.equal(r["counts"], res["counts"]) and torch.equal(r["sums"], res["sums"])
        res = r


def test_a_transposed_item_is_a_gross_error_beyond_20_percent_and_a_cents_offset_inside(front):
    n = 60 * HOP
    wa, la = _wavs([_sung(220.0, n), _sung(220.0, n)])
    up4, up2 = 2.0 ** (4 / 12), 2.0 ** (2 / 12)                # + 26 %: beyond the rule; + 12.2 %: inside it, 200 cents
    wb, lb = _wavs([_sung(220.0 / up4, n), _sung(220.0 / up2, n)])
    for align in ("dtw", "frames"):
        r = E.score_wavs(front, wa, la, wb, lb, align=align)
        n_both = r["counts"][:, 1].cpu().numpy()
        assert (n_both >= 20).all() and r["status"].cpu().tolist() == [0, 0]
        print(f"{align}: gpe {r['gpe']}, f0_rmse_cents {r['f0_rmse_cents']}, mcd_db {r['mcd_db']}, n_both {n_both}")
        assert r["gpe"][0] == 1.0 and r["gpe"][1] == 0.0
        assert abs(r["f0_rmse_cents"][0] - 400.0) <= 5.0 and abs(r["f0_rmse_cents"][1] - 200.0) <= 5.0      # the tracker's accuracy on these signals
        assert (r["mcd_db"] > 0).all() and np.isfinite(r["mcd_db"]).all()
        assert r["mean"]["gpe"] == 0.5


def test_frames_alignment_scores_the_common_frames(front):
    wa, la = _wavs([_sung(220.0, 50 * HOP), _sung(262.0, 31 * HOP)])
    wb, lb = _wavs([_sung(220.0, 41 * HOP + 17), _sung(262.0, 58 * HOP)])
    r = E.score_wavs(front, wa, la, wb, lb, align="frames")
    assert r["plen"].cpu().tolist() == [42, 32] and r["counts"][:, 0].cpu().tolist() == [42, 32] and "path" not in r
    assert r["status"].cpu().tolist() == [0, 0] and np.isfinite(r["mcd_db"]).all()
    d = E.score_wavs(front, wa, la, wb, lb, align="dtw", band_s=0)
    assert (d["plen"].cpu().numpy() >= [51, 59]).all() and d["band"] == 0
    with pytest.warns(UserWarning, match=r"items \[1\] not aligned"):      # 59 target frames > 1 * 32 rendered ones in a band of one frame
        w = E.score_wavs(front, wa, la, wb, lb, align="dtw", band_s=1.2 * HOP / SR)
    assert w["status"].cpu().tolist() == [0, 1] and w["plen"].cpu().tolist()[1] == 32


@pytest.fixture(scope="module")
def inf():
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(dict(timesteps=3, K_step=3, f0_timesteps=3))
    ins = StyleSingerInfer(hp, device=DEV, model_state=synth.synth_acoustic_state_dict(hp, 5), vocoder_state=synth.synth_vocoder_state_dict(None, 11),
                           speaker_state=None)
    ins.model.use_graphs = "off"
    return ins


def test_infer_evaluate_on_a_tiny_model_and_the_render_is_untouched(inf):
    batch = {k: v.to(DEV) for k, v in synth.synth_batch(2, 24, 5, 30, inf.hparams, 5).items()}
    before = inf.infer_batch(batch, seed=3)
    torch.cuda.synchronize()
    tw, tl = _wavs([_sung(220.0, 30 * HOP), _sung(247.0, 20 * HOP)])
    for kw in (dict(), dict(align="frames"), dict(target_srs=[SR, SR], band_s=0.5)):
        r = inf.evaluate(before, tw, tl, **kw)
        assert tuple(r["counts"].shape) == (2, 4) and tuple(r["sums"].shape) == (2, 2) and r["counts"].dtype == torch.int64 and r["sums"].dtype == torch.float64
        assert r["frames_a"] == [25, 25] and r["frames_b"] == [31, 21]
        for k in E.DERIVED:
            assert r[k].shape == (2,) and np.isfinite(r[k]).all() and math.isfinite(r["mean"][k]), k
        assert (r["mcd_db"] > 0).all() and ((0 <= r["ffe"]) & (r["ffe"] <= 1)).all()
    r24 = inf.evaluate(before, torch.stack([tw[0, ::2], tw[1, ::2]]).contiguous(), [tl[0] // 2, tl[1] // 2], target_srs=[SR // 2, SR // 2])
    assert r24["frames_b"] == [31, 21] and np.isfinite(r24["mcd_db"]).all()          # a target at another rate is resampled first
    after = inf.infer_batch(batch, seed=3)                      # scoring in between changes nothing the renderer computes
    for k in ("mel", "f0", "wav", "lens"):
        assert torch.equal(before[k], after[k]), k
    with pytest.raises(ValueError, match="no 'wav'"):
        inf.evaluate(inf.infer_batch(batch, seed=3, vocode=False), tw, tl)


def test_command_line_scores_two_wav_files(tmp_path, capsys):
    import json
    from stylesinger_amd.writer import save_wav
    w = _sung(220.0, 40 * HOP)
    save_wav(w, str(tmp_path / "a.wav"), SR)
    save_wav(_sung(196.0, 20 * HOP + 64), str(tmp_path / "b24.wav"), SR // 2)      # a target file at another rate: resampled to the model's first
    rep = E.main(["--pred", str(tmp_path / "a.wav"), "--target", str(tmp_path / "a.wav"), "--json", str(tmp_path / "out.json")])
    assert json.loads(capsys.readouterr().out) == rep == json.loads((tmp_path / "out.json").read_text())
    assert rep["status"] == 0 and rep["frames_pred"] == rep["frames_target"] == rep["path_len"] == 41 and rep["align"] == "dtw" and rep["band_frames"] == 375
    assert all(rep[k] == 0 for k in E.DERIVED) and "singer_cos" not in rep and "not SPTK" in rep["note"]
    rep = E.main(["--pred", str(tmp_path / "a.wav"), "--target", str(tmp_path / "b24.wav"), "--align", "frames"])
    assert rep["frames_target"] == (2 * (20 * HOP + 64)) // HOP + 1 == rep["path_len"] and rep["align"] == "frames"
