"""The true-peak limiter without a GPU: stylesinger_amd/limiter.py's host definition against the independent restatement
(tests/limiter_ref.py), the invariants of the definition, the inter-sample case against its analytic value, that every input of the GPU test has
an `n_limited` the reference alone decides, the argument refusals, the `out_wav_norm` exclusion and the header. Conformance with a standard
true-peak meter is NOT claimed (the estimate is the project's own 4x interpolator)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from limiter_cases import C as CEIL, CEILING_DB, SR, WINDOWS, cases, gain_case, inter_sample_sine
from limiter_ref import limiter_ref
from stylesinger_amd import abi, config
from stylesinger_amd import limiter as LM


@functools.lru_cache(maxsize=None)
def _ref(i, W):
    return limiter_ref(cases()[i][1], SR, CEIL, W, with_bound=True)


@pytest.mark.parametrize("W", WINDOWS)
def test_host_definition_equals_the_independent_restatement(W):
    """two float64 statements of the same definition: they differ by the order of a 127-term and a W-term sum, <= 1e-12 on values <= 16"""
    for i, (name, x) in enumerate(cases()):
        a, b = LM.limit_f64(x, SR, CEILING_DB, W=W), _ref(i, W)
        assert a["W"] == W and a["c"] == CEIL
        for k in ("e", "r", "m", "g", "y"):
            assert a[k].shape == b[k].shape and np.abs(a[k] - b[k]).max(initial=0.0) <= 1e-12, (name, k)
        assert np.array_equal(a["xp"], b["xp"]) and a["n_limited"] == b["n_limited"], name
        assert abs(a["min_gain"] - b["min_gain"]) <= 1e-12


@pytest.mark.parametrize("W", WINDOWS)
def test_invariants_of_the_definition(W):
    limited = 0
    for i, (name, x) in enumerate(cases()):
        d = LM.limit_f64(x, SR, CEILING_DB, W=W)
        assert (d["g"] <= d["r"]).all() and (d["g"] > 0).all(), name
        assert np.abs(d["y"]).max(initial=0.0) <= float(CEIL) * (1.0 + 2.0 ** -51), name     # (c / e) e in float64: two roundings
        if d["e"].max(initial=0.0) <= float(CEIL):
            assert (d["g"] == 1.0).all() and d["n_limited"] == 0 and np.array_equal(d["y"], d["xp"].astype(np.float64)), name
        limited += d["n_limited"] > 0
        # a peak is announced W - 1 samples ahead and released W - 1 samples after: g < 1 exactly within W - 1 of a sample with r < 1
        near = np.convolve(np.append(d["r"] < 1.0, False).astype(np.float64), np.ones(2 * W - 1))[W - 1:W - 1 + len(x)] > 0
        assert np.array_equal(d["g"] < 1.0, near), name
    assert limited >= 15
    names = [n for n, _ in cases()]
    assert LM.limit_f64(cases()[names.index("quiet")][1], SR, CEILING_DB, W=W)["n_limited"] == 0


def test_scaling_the_input_against_the_gain_changes_nothing():
    """x / k with the gain k: x' is the same fp32 array for k a power of two, so everything after it is"""
    x = cases()[[n for n, _ in cases()].index("loud")][1]
    a = LM.limit_f64(x, SR, CEILING_DB, W=96)
    b = LM.limit_f64((x * np.float32(0.25)).astype(np.float32), SR, CEILING_DB, W=96, gain=4.0)
    assert np.array_equal(a["y"], b["y"]) and np.array_equal(a["g"], b["g"])
    # any other k: x' differs by the fp32 roundings of the quotient and of the product, |dx'| <= 2 u |x|. Then |de| <= 2 u S max|x| with
    # S = sum |w| <= 2.57, |dr| <= |de| / c (r = c / e only where e >= c), and |dy| <= |dr| |x'| + 2 u |x'|
    k, u, mx = np.float32(1.7), 2.0 ** -24, float(np.abs(x).max())
    c = LM.limit_f64((x / k).astype(np.float32), SR, CEILING_DB, W=96, gain=k)
    assert np.abs(c["y"] - a["y"]).max() <= (2 * 2.57 * mx / float(CEIL) + 2) * u * mx * 1.01


def test_inter_sample_peak_of_the_fs4_sine_reads_within_the_interpolators_error():
    """A sine at fs / 4 with phase 45 degrees has samples of +0.70711 twice, -0.70711 twice, ...: a true peak of 1 half way between the two equal
    samples (phase 2 of the bank, seen by the envelope of the first of them) and a zero crossing between the two others. The interpolator's own
    error at the peak, measured against the analytic value: 4.2e-8 (tests/resample_ref.py reports <= 2e-6 in band for this bank)."""
    x = inter_sample_sine(3000)
    assert abs(np.abs(x).max() - math.sqrt(0.5)) < 1e-6
    e = LM.envelope_f64(x.astype(np.float64), SR)
    mid = e[200:-200:2]   # the samples followed by a peak; away from the ends, where the truncated signal is not a sine
    err = np.abs(mid - 1.0).max()
    print(f"fs/4 sine: envelope before a peak {mid.min():.9f} .. {mid.max():.9f}, |e - 1| <= {err:.3e}")
    assert err <= 2e-6
    assert np.abs(e[201:-200:2] - math.sqrt(0.5)).max() < 1e-6, "before a zero crossing nothing exceeds the sample itself"
    d = LM.limit_f64(x, SR, CEILING_DB, W=96)
    assert d["n_limited"] == len(x) and abs(d["g"][200:-200] - float(CEIL)).max() <= 2e-6    # limited, though no SAMPLE exceeds the ceiling


@pytest.mark.parametrize("W", WINDOWS)
def test_every_gpu_input_has_a_count_the_reference_alone_decides(W):
    for i, (name, x) in enumerate(cases()):
        assert _ref(i, W)["decided"], name


def test_the_measured_gain_case_is_decided_and_fires_the_peak_rule():
    xs, target, gs = gain_case()
    for x, g in zip(xs, gs):
        assert len(x) >= 0.4 * SR and np.float32(g * np.abs(x).max()) > 1, "ss_loudness_apply would divide this item by its peak"
        ref = limiter_ref(x, SR, CEIL, 96, gain=g, with_bound=True)
        assert ref["decided"] and 0 < ref["n_limited"] < len(x)
        assert np.array_equal(ref["g"], LM.limit_f64(x, SR, CEILING_DB, W=96, gain=g)["g"]) or \
            np.abs(ref["g"] - LM.limit_f64(x, SR, CEILING_DB, W=96, gain=g)["g"]).max() <= 1e-12


def test_arguments_are_refused_before_a_device_is_touched():
    import torch
    host = torch.zeros(1, 100)
    for bad in (0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="ceiling_db"):
            LM.limit_batch(host, [100], SR, bad)
    with pytest.raises(ValueError, match="LIMIT_MAX_W"):
        LM.limit_batch(host, [100], SR, -1.0, lookahead_ms=1000.0 * (LM.LIMIT_MAX_W + 1) / SR)
    for bad in (float("nan"), -1.0):
        with pytest.raises(ValueError, match="lookahead_ms"):
            LM.limit_batch(host, [100], SR, -1.0, lookahead_ms=bad)
    from stylesinger_amd.lib import StyleSingerHipError
    with pytest.raises(StyleSingerHipError, match="device tensors"):
        LM.limit_batch(host, [100], SR, -1.0)
    assert LM.window_samples(48000) == 96 and LM.window_samples(48000, 0.0) == 1 and LM.window_samples(22050, 2.0) == 44
    assert LM.window_samples(SR, 1000.0 * LM.LIMIT_MAX_W / SR) == LM.LIMIT_MAX_W
    assert LM.ceiling_f32(0.0) == 1.0 and LM.ceiling_f32(-1.0) == np.float32(10.0 ** -0.05)


def test_hparams_and_the_out_wav_norm_exclusion():
    from stylesinger_amd.infer import StyleSingerInfer
    hp = config.make_hparams(None)
    assert hp["out_true_peak_db"] is None and hp["out_limiter_lookahead_ms"] == 2.0
    assert config.make_hparams(dict(out_true_peak_db=-1.0, out_limiter_lookahead_ms=1.0))["out_true_peak_db"] == -1.0
    with pytest.raises(ValueError, match="out_true_peak_db and out_wav_norm exclude each other"):
        StyleSingerInfer(dict(out_true_peak_db=-1.0, out_wav_norm=True), device="cpu")
    with pytest.raises(ValueError, match="ceiling_db"):
        StyleSingerInfer(dict(out_true_peak_db=3.0), device="cpu")
    with pytest.raises(ValueError, match="LIMIT_MAX_W"):
        StyleSingerInfer(dict(out_true_peak_db=-1.0, out_limiter_lookahead_ms=50.0), device="cpu")


def test_header_declares_the_entry_and_the_abi_version_stays():
    from stylesinger_amd import lib
    decl = abi.declarations()
    assert "ss_limit_true_peak" in decl and "ss_limit_workspace_bytes" in decl
    assert decl["ss_limit_workspace_bytes"] == (C.c_int64, [C.c_int, C.c_int])
    assert len(decl["ss_limit_true_peak"][1]) == 20 and decl["ss_limit_true_peak"][1][8:10] == [C.c_float, C.c_int]
    assert abi.DEFINES["SS_LIMIT_MAX_W"] == LM.LIMIT_MAX_W == 512
    l = lib.load()
    assert l.ss_abi_version() == 20 == abi.DEFINES["SS_ABI_VERSION"], "the export is additive"
    bank_copy = (256 // 4 + 1) * 16 * 4   # the tap-major copy of the bank behind the per-tile partials (rounded up to 64 bytes)
    assert l.ss_limit_workspace_bytes(3, 2048) == 64 + bank_copy and l.ss_limit_workspace_bytes(9, 2049) == 192 + bank_copy
    assert l.ss_limit_workspace_bytes(0, 5) < 0
    p = 0x1000   # placeholder non-null pointers: every refusal below comes before anything is dereferenced or launched

    def call(x=p, W=96, c=0.5, y=2 * p, taps=127, wsb=64 + bank_copy):
        return l.ss_limit_true_peak(x, 16, 16, p, None, p, taps, 63, c, W, y, 16, 16, p, p, None, 1, p, wsb, None)
    assert call(x=None) != 0 and b"null argument" in l.ss_last_error()
    assert call(W=513) != 0 and b"look-ahead window of 513 samples" in l.ss_last_error()
    assert call(W=0) != 0 and call(c=1.5) != 0 and b"bad ceiling" in l.ss_last_error()
    assert call(taps=300) != 0 and b"bad filter" in l.ss_last_error()
    assert call(wsb=63 + bank_copy) != 0 and b"workspace" in l.ss_last_error()
    assert call(y=p) != 0 and b"must not alias" in l.ss_last_error()
    assert call(y=p + 32) != 0 and b"must not alias" in l.ss_last_error(), "overlapping row ranges, not merely equal pointers"
