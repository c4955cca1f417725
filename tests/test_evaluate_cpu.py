"""The objective metrics without a GPU: the definitions of stylesinger_amd/evaluate.py (quantised mel cepstrum, the warp with its diagonal-first tie
order, the counts and sums along the path) on cases that can be checked by hand, the entries' refusals before a device is touched, the workspace
query and the command line's argument errors. The kernels against these definitions: tests/test_gpu_evaluate.py."""
import itertools
import math

import numpy as np
import pytest

import evaluate_cases as K
from stylesinger_amd import abi
from stylesinger_amd import evaluate as E
from stylesinger_amd import lib

ENTRIES = {"ss_eval_mcep": 14, "ss_eval_dtw_workspace_bytes": 4, "ss_eval_cost_band": 12, "ss_eval_dtw": 13, "ss_eval_reduce": 17, "ss_cosine_rows": 6}


# ---- 1. plumbing -----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_abi_version_stays():
    decl = lib.declarations()
    for name, nargs in ENTRIES.items():
        assert name in lib.declared_symbols() and len(decl[name][1]) == nargs, name
    l = lib.load()                                            # resolves EVERY declared symbol, or raises
    for name in lib.declared_symbols():
        assert hasattr(l, name), name
    assert l.ss_abi_version() == 20 == abi.DEFINES["SS_ABI_VERSION"]
    assert E.EVAL_MAX_T == abi.DEFINES["SS_EVAL_MAX_T"] == 8192 and E.EVAL_MAX_K == abi.DEFINES["SS_EVAL_MAX_K"] >= K.KP
    assert E.EVAL_MAX_T >= 5625                               # the longest item of the benchmark configurations
    assert 14 * E.EVAL_MAX_T <= 160 * 1024                    # the sweep's LDS layout at the cap
    assert 2 * E.EVAL_MAX_T * 46341 < E.EVAL_INF < 2 ** 31 - 46341   # int32 D cannot overflow: a path has < 2 T cells of cost <= isqrt(2^31)


def _calls():
    l = lib.load()
    p = 4096     # any non-null, aligned address: every call below is refused before it is used
    ok = dict(mel=p, ldm=80, bs=800, lens=p, tab=p, q=p, B=1, T=10, N=80, K=24, s=256.0, vmin=-6.0, vmax=1.5, qa=p, qb=p, la=p, lb=p, Kp=24, band=0, Ta=8, Tb=8,
              ws=p, wsb=192, path=p, plen=p, cost=p, st=p, fa=p, fb=p, ldfa=8, ldfb=8, counts=p, sums=p)

    def mcep(**kw):
        a = dict(ok, **kw)
        return l.ss_eval_mcep(a["mel"], a["ldm"], a["bs"], a["lens"], a["tab"], a["q"], a["B"], a["T"], a["N"], a["K"], a["s"], a["vmin"], a["vmax"], None)

    def cost(**kw):
        a = dict(ok, **kw)
        return l.ss_eval_cost_band(a["qa"], a["la"], a["qb"], a["lb"], a["Kp"], a["band"], a["Ta"], a["Tb"], a["B"], a["ws"], a["wsb"], None)

    def dtw(**kw):
        a = dict(ok, **kw)
        return l.ss_eval_dtw(a["la"], a["lb"], a["band"], a["path"], a["plen"], a["cost"], a["st"], a["Ta"], a["Tb"], a["B"], a["ws"], a["wsb"], None)

    def red(**kw):
        a = dict(ok, **kw)
        return l.ss_eval_reduce(a["qa"], a["fa"], a["ldfa"], a["la"], a["qb"], a["fb"], a["ldfb"], a["lb"], a["Kp"], a["path"], a["plen"], a["Ta"], a["Tb"],
                                a["B"], a["counts"], a["sums"], None)

    def cos(**kw):
        a = dict(dict(a=p, b=p, out=p, rows=2, C=8), **kw)
        return l.ss_cosine_rows(a["a"], a["b"], a["out"], a["rows"], a["C"], None)
    return l, dict(ss_eval_mcep=mcep, ss_eval_cost_band=cost, ss_eval_dtw=dtw, ss_eval_reduce=red, ss_cosine_rows=cos)


def test_entries_refuse_bad_arguments_before_any_launch():
    l, f = _calls()
    big = E.EVAL_MAX_T + 1
    cases = [("ss_eval_mcep", dict(mel=None), b"null pointer"), ("ss_eval_mcep", dict(q=None), b"null pointer"), ("ss_eval_mcep", dict(tab=None), b"null pointer"),
             ("ss_eval_mcep", dict(ldm=79), b"bad dims"), ("ss_eval_mcep", dict(K=E.EVAL_MAX_K + 1), b"bad dims"), ("ss_eval_mcep", dict(K=0), b"bad dims"),
             ("ss_eval_mcep", dict(vmin=-60.0, vmax=15.0), b"beyond int16"),       # 256 sqrt(80) 75 = 171 731
             ("ss_eval_mcep", dict(s=489.0), b"beyond int16"),                     # 489 sqrt(80) 7.5 + 1 = 32 804 (488: 32 737, accepted by the bound)
             ("ss_eval_mcep", dict(vmin=100.0, vmax=101.0), b"beyond int16"),      # a narrow range far from 0: q itself leaves int16
             ("ss_eval_mcep", dict(N=7, ldm=7, K=24, s=1000.0), b"beyond int16"),  # K >= N: 24 * 28063^2 >= 2^31
             ("ss_eval_mcep", dict(vmin=2.0, vmax=1.0), b"range"), ("ss_eval_mcep", dict(s=float("nan")), b"scale"),
             ("ss_eval_cost_band", dict(qa=None), b"null pointer"), ("ss_eval_cost_band", dict(ws=None), b"null pointer"),
             ("ss_eval_cost_band", dict(lb=None), b"null pointer"), ("ss_eval_cost_band", dict(Kp=23), b"bad dims"), ("ss_eval_cost_band", dict(B=0), b"bad dims"),
             ("ss_eval_cost_band", dict(Ta=big, wsb=1 << 40), b"cap"), ("ss_eval_cost_band", dict(Tb=big, wsb=1 << 40), b"cap"),
             ("ss_eval_cost_band", dict(wsb=191), b"workspace"), ("ss_eval_cost_band", dict(band=2, wsb=119), b"workspace"),
             ("ss_eval_cost_band", dict(qa=4098), b"alignment"),
             ("ss_eval_dtw", dict(path=None), b"null pointer"), ("ss_eval_dtw", dict(st=None), b"null pointer"), ("ss_eval_dtw", dict(ws=None), b"null pointer"),
             ("ss_eval_dtw", dict(Ta=big, wsb=1 << 40), b"cap"), ("ss_eval_dtw", dict(Tb=big, wsb=1 << 40), b"cap"), ("ss_eval_dtw", dict(wsb=191), b"workspace"),
             ("ss_eval_dtw", dict(band=2, wsb=119), b"workspace"), ("ss_eval_dtw", dict(B=0), b"bad dims"), ("ss_eval_dtw", dict(path=4100), b"alignment"),
             ("ss_eval_reduce", dict(fa=None), b"null pointer"), ("ss_eval_reduce", dict(sums=None), b"null pointer"),
             ("ss_eval_reduce", dict(path=None), b"go together"), ("ss_eval_reduce", dict(plen=None), b"go together"),
             ("ss_eval_reduce", dict(ldfa=7), b"bad dims"), ("ss_eval_reduce", dict(Ta=big, ldfa=big), b"cap"), ("ss_eval_reduce", dict(Kp=0), b"bad dims"),
             ("ss_cosine_rows", dict(a=None), b"null pointer"), ("ss_cosine_rows", dict(out=None), b"null pointer"), ("ss_cosine_rows", dict(C=0), b"bad dims"),
             ("ss_cosine_rows", dict(rows=0), b"bad dims")]
    for name, kw, word in cases:
        assert f[name](**kw) != 0, (name, kw)
        err = l.ss_last_error()
        assert name.encode() in err and word in err, (name, kw, err)
    # the Python forms refuse the same ranges, before any tensor is looked at
    for kw in (dict(vmin=-60.0, vmax=15.0), dict(s=489.0), dict(vmin=100.0, vmax=101.0)):
        with pytest.raises(ValueError, match="beyond int16"):
            E.mcep_bound(**dict(dict(n_mels=80, K=24, s=256.0, vmin=-6.0, vmax=1.5), **kw))
    assert E.mcep_bound(80, 24, 256.0, -6.0, 1.5) == pytest.approx(256 * math.sqrt(80) * 7.5 + 1)
    assert E.mcep_bound(80, 24, 488.0, -6.0, 1.5) <= 32767
    assert E.mcep_bound(7, 24, 256.0, -6.0, 1.5) == pytest.approx(256 * math.sqrt(14) * 7.5 + 1)


def test_workspace_query():
    q = lib.load().ss_eval_dtw_workspace_bytes
    for B, Ta, Tb, band in ((3, 100, 50, 0), (3, 100, 50, 4), (3, 100, 50, 40), (1, 7, 300, 16), (2, 1, 1, 0), (1, E.EVAL_MAX_T, E.EVAL_MAX_T, 375)):
        assert q(B, Ta, Tb, band) == 3 * B * Ta * (min(Tb, 2 * band + 1) if band > 0 else Tb), (B, Ta, Tb, band)
    assert q(1, E.EVAL_MAX_T, E.EVAL_MAX_T, 0) == 3 * E.EVAL_MAX_T ** 2
    assert q(0, 8, 8, 0) == 0 and q(1, E.EVAL_MAX_T + 1, 8, 0) == 0 and q(1, 8, E.EVAL_MAX_T + 1, 0) == 0 and q(1, 0, 8, 0) == 0 and q(1, 8, 0, 0) == 0


def test_device_wrappers_refuse_host_tensors():
    import torch
    q = torch.zeros(1, 8, 24, dtype=torch.int16)
    f = torch.zeros(1, 8)
    for call in (lambda: E.mcep_q_device(torch.zeros(1, 8, 80)), lambda: E.align_device(q, [8], q, [8]), lambda: E.reduce_device(q, f, [8], q, f, [8]),
                 lambda: E.cosine_rows_device(f, f), lambda: E.score_pairs(torch.zeros(1, 8, 80), f, [8], torch.zeros(1, 8, 80), f, [8])):
        with pytest.raises(lib.StyleSingerHipError, match="device tensors"):
            call()
    with pytest.raises(ValueError, match="'dtw' or 'frames'"):
        E.score_pairs(None, None, None, None, None, None, align="linear")
    with pytest.raises(ValueError, match="seconds >= 0"):
        E.score_pairs(None, None, None, None, None, None, band_s=-1.0)
    assert E.band_frames(2.0, 48000, 256) == 375 and E.band_frames(0, 48000, 256) == 0 and E.band_frames(0.5, 24000, 128) == 94


# ---- 2. the quantised cepstrum ------------------------------------------------------------------------------------------------------------------------
def test_table_is_the_orthonormal_dct_without_c0():
    for N in (80, 7):
        tab = E.mcep_table(N, N - 1).astype(np.float64)
        assert np.abs(tab @ tab.T - np.eye(N - 1)).max() < 1e-6
        assert np.abs(tab.sum(axis=1)).max() < 1e-5           # orthogonal to c0, the frame's level
    assert E.mcep_table(80, 24).dtype == np.float32 and E.mcep_table(80, 24).shape == (24, 80)


def test_mcep_q_is_the_fp32_chain_and_masks_what_it_must():
    rng = np.random.default_rng(1)
    mel = K.wide_mel(rng, 9)
    q = E.mcep_q(mel, 6, K=13)
    assert q.shape == (9, 14) and q.dtype == np.int16 and not q[6:].any() and not q[:, 13].any() and q[:6, :13].any()
    # the chain written out for one coefficient of one frame, scalar float32
    tab = E.mcep_table(80, 13)
    m = np.clip(mel[2], np.float32(K.VMIN), np.float32(K.VMAX))
    c = np.float32(0)
    for n in range(80):
        c = np.float32(c + np.float32(m[n] * tab[4, n]))
    assert q[2, 4] == int(np.rint(np.float32(c * np.float32(256))))
    # clipping: values beyond the range give what the range's ends give
    assert np.array_equal(E.mcep_q(np.clip(mel, K.VMIN, K.VMAX), 6, K=13), q)
    # close to the float64 DCT: the quantisation step is 1 / 256
    ref = np.clip(mel[:6], K.VMIN, K.VMAX).astype(np.float64) @ tab.astype(np.float64).T * 256
    assert np.abs(q[:6, :13] - ref).max() <= 0.5 + 5e-2           # (80 fp32 roundings of sums below 64: < 80 * 2^-19 * 256 = 0.04 counts)


def test_parseval_bound_on_corner_valued_mels():
    rng = np.random.default_rng(2)
    qa, qb = E.mcep_q(K.corner_mel(rng, 40)), E.mcep_q(K.corner_mel(rng, 40))
    bound = E.mcep_bound(80, 24, 256.0, K.VMIN, K.VMAX)
    assert max(np.abs(qa).max(), np.abs(qb).max()) <= bound
    S = E.sq_dist_matrix(qa, qb)
    assert S.max() <= (bound + math.sqrt(24)) ** 2 < 2.96e8 < 2 ** 31 and S.max() > 1e7       # (+ sqrt(K) / 2 per side: the rounding of rint)
    assert E.isqrt(S).max() <= 17178 + 5
    # the opposite corners: every bin at vmin against every bin at vmax has NO cepstral distance (a level shift lives in c0, which is left out)
    lo, hi = np.full((1, 80), K.VMIN, np.float32), np.full((1, 80), K.VMAX, np.float32)
    assert E.sq_dist_matrix(E.mcep_q(lo), E.mcep_q(hi)).max() <= 24
    for v in (0, 1, 2, 3, 15, 16, 17, 2 ** 31 - 1, 46340 ** 2, 46340 ** 2 - 1, 46341 ** 2 - 1):
        assert int(E.isqrt(np.asarray([v]))[0]) == math.isqrt(v)


# ---- 3. the warp ---------------------------------------------------------------------------------------------------------------------------------------
def _brute_min(C):
    n_a, n_b = C.shape
    best, stack = None, [(0, 0, int(C[0, 0]))]
    while stack:
        i, j, s = stack.pop()
        if i == n_a - 1 and j == n_b - 1:
            best = s if best is None else min(best, s)
            continue
        for a, b in ((i + 1, j), (i, j + 1), (i + 1, j + 1)):
            if a < n_a and b < n_b:
                stack.append((a, b, s + int(C[a, b])))
    return best


def _is_path(path, n_a, n_b):
    steps = np.diff(path, axis=0)
    return (tuple(path[0]) == (0, 0) and tuple(path[-1]) == (n_a - 1, n_b - 1)
            and all(tuple(s) in ((1, 1), (1, 0), (0, 1)) for s in steps))


def test_warp_cost_is_the_minimum_over_all_monotone_paths():
    rng = np.random.default_rng(11)
    for n_a, n_b in itertools.product(range(1, 6), repeat=2):
        for _ in range(4):
            C = rng.integers(0, 7, (n_a, n_b))
            path, cost = E.warp_path(C)
            assert cost == _brute_min(C) and _is_path(path, n_a, n_b)
            assert cost == sum(int(C[i, j]) for i, j in path)


def test_an_item_against_itself_and_against_its_doubled_copy():
    rng = np.random.default_rng(12)
    q = K.random_q(rng, 23)
    f0 = K.random_f0(rng, 23)
    for band in (None, 2, 5):
        path, P, cost, status = E.dtw_path(q, q, band)
        assert status == 0 and cost == 0 and P == 23 and np.array_equal(path, E.identity_path(23, 23))
        m = E.path_metrics(q, q, f0, f0, path)
        d = E.derive(**m)
        assert m["dist_sum"] == 0 and d == dict(mcd_db=0.0, ffe=0.0, vde=0.0, gpe=0.0, f0_rmse_cents=0.0)
    q2, f2 = K.doubled(q), np.repeat(f0, 2)
    want = np.stack([np.repeat(np.arange(23), 2), np.arange(46)], axis=1)
    for band in (None, 2):                                    # a band of 2 frames holds the staircase: c_i = 2 i + 1
        path, P, cost, status = E.dtw_path(q, q2, band)
        assert status == 0 and cost == 0 and P == 2 * 23 and np.array_equal(path, want)
        assert E.derive(**E.path_metrics(q, q2, f0, f2, path))["ffe"] == 0.0
    path, P, cost, status = E.dtw_path(q, q2, 1)              # 46 <= 1 * 23 fails: not aligned
    assert status == 1 and cost == 0 and P == 23 and np.array_equal(path, E.identity_path(23, 46))


def test_ties_take_the_diagonal_first():
    z = np.zeros((9, K.KP), np.int16), np.zeros((13, K.KP), np.int16)
    path, P, cost, status = E.dtw_path(*z)
    want = [(0, j) for j in range(4)] + [(i, i + 4) for i in range(9)]       # the diagonal from (8, 12) back to (0, 4), then left
    assert status == 0 and cost == 0 and P == 13 and [tuple(p) for p in path] == want
    # up-first (contour_align's order) would walk the matrix edge: 9 + 13 - 1 = 21 cells for the same cost
    path, P, _, _ = E.dtw_path(z[1], z[0])
    assert P == 13 and [tuple(p) for p in path] == [(i, 0) for i in range(4)] + [(i + 4, i) for i in range(9)]


def test_an_item_the_band_cannot_connect_is_scored_frame_by_frame():
    rng = np.random.default_rng(13)
    qa, qb = K.random_q(rng, 3), K.random_q(rng, 50)
    path, P, cost, status = E.dtw_path(qa, qb, 4)             # 50 > 4 * 3
    assert status == 1 and cost == 0 and P == 3 and np.array_equal(path, E.identity_path(3, 50))
    assert E.dtw_path(qa, qb, 17)[3] == 0                     # 50 <= 17 * 3
    assert E.dtw_path(qb, qa, 4)[3] == 0                      # fewer target frames than rendered ones always connects
    for a, b in ((qa[:0], qb), (qa, qb[:0])):
        path, P, cost, status = E.dtw_path(a, b)
        assert status == 1 and P == 0 and path.shape == (0, 2)
        assert all(math.isnan(v) for v in E.derive(**E.path_metrics(a, b, np.zeros(len(a)), np.zeros(len(b)), path)).values())


def test_every_band_with_nb_le_W_na_reaches_the_end_cell():
    for n_a, n_b in itertools.product(range(1, 16), repeat=2):
        C = np.zeros((n_a, n_b), dtype=np.int64)
        for W in (1, 2, 3, 5, 8, 30):
            W = max(W, -(-n_b // n_a))
            path, cost = E.warp_path(C, W)
            assert path is not None and cost == 0 and _is_path(path, n_a, n_b)
            assert (np.abs(path[:, 1] - E.band_centres(n_a, n_b)[path[:, 0]]) <= W).all()


# ---- 4. counts and sums -----------------------------------------------------------------------------------------------------------------------------------
def test_counts_on_the_20_percent_boundary():
    fa, fb, want = K.boundary_contours()
    q = np.zeros((9, K.KP), np.int16)
    m = E.path_metrics(q, q, fa, fb, E.identity_path(9, 9))
    assert {k: m[k] for k in want} == want
    d = E.derive(**m)
    assert d["ffe"] == (2 + 3) / 9 and d["vde"] == 2 / 9 and d["gpe"] == 3 / 6 and d["mcd_db"] == 0.0
    cents = [1200 * math.log2(float(a) / float(b)) for a, b in zip(fa, fb) if a > 0 and b > 0]
    assert d["f0_rmse_cents"] == pytest.approx(math.sqrt(sum(c * c for c in cents) / 6), rel=1e-12)
    # the same frames through a warp path that repeats one: every count follows the PATH, not the frames
    path = np.asarray([(0, 0), (1, 1), (1, 2), (2, 2)], dtype=np.int32)
    m = E.path_metrics(q, q, fa, fb, path)
    assert (m["P"], m["n_both"], m["n_vde"], m["n_gpe"]) == (4, 4, 0, 2)     # frame 1 of a is counted twice: against frames 1 and 2 of b


def test_mcd_of_a_known_distance():
    qa, qb = np.zeros((4, K.KP), np.int16), np.zeros((4, K.KP), np.int16)
    qb[:, 0], qb[:, 1] = 3 * 256, 4 * 256                     # ||c_a - c_b|| = 5 log10 units on every frame
    m = E.path_metrics(qa, qb, np.zeros(4), np.zeros(4), E.identity_path(4, 4))
    assert m["dist_sum"] == 4 * 5 * 256 and E.derive(**m)["mcd_db"] == pytest.approx(50 * math.sqrt(2))
    assert E.singer_cos([1, 0, 0], [1, 0, 0]) == 1.0 and E.singer_cos([1, 2], [-1, -2]) == pytest.approx(-1.0) and E.singer_cos([1, 0], [0, 3]) == 0.0
    assert E.singer_cos([0, 0], [1, 1]) == 0.0


# ---- 5. the command line -----------------------------------------------------------------------------------------------------------------------------------
def test_cli_argument_errors(capsys, monkeypatch):
    from stylesinger_amd import audiofile
    monkeypatch.setattr(audiofile, "load_audio", lambda *a, **k: pytest.fail("a file was read before the flags were checked"))
    base = ["--pred", "a.wav", "--target", "b.wav"]
    for argv, word in ((base + ["--band-s", "1.0"], "--band-s needs --align dtw"), (base + ["--align", "frames", "--band-s", "1.0"], "--band-s needs --align dtw"),
                       (base + ["--align", "dtw", "--band-s", "-1"], ">= 0"), (base + ["--align", "linear"], "invalid choice"),
                       (["--pred", "a.wav"], "--target"), (["--target", "b.wav"], "--pred")):
        with pytest.raises(SystemExit) as e:
            E.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv
