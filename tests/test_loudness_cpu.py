"""The loudness meter's host side (no GPU): stylesinger_amd/loudness.py against the independent restatement (tests/loudness_ref.py), known
answers (a 997 Hz full-scale sine, the coefficient tables of BS.1770-4), scaling, the short-item and silence rules, the opt-in resolver and the
argument checks of `ss_loudness_measure` / `ss_loudness_apply`. Parity with pyloudnorm itself is UNPINNED (the package is un-vendored); what is
held here is the definition in stylesinger_amd/loudness.py."""
import math

import numpy as np
import pytest

from loudness_ref import coefficients, gated_signal, loudness_ref, normalize_ref
from stylesinger_amd import lib
from stylesinger_amd import loudness as LD

RATES = (48000, 22050)


def _lengths(rate):
    return [int(0.4 * rate), int(0.4 * rate) + 1, int(0.46 * rate), int(0.44 * rate), int(2.93 * rate) + 17]


@pytest.mark.parametrize("rate", RATES)
def test_module_matches_the_restatement_on_the_gated_signal(rate):
    for n in _lengths(rate):
        x = gated_signal(n, rate)
        ref, got = loudness_ref(x, rate), LD.loudness_details_f64(x, rate)
        print(f"{rate} Hz n={n}: {len(ref['z'])} blocks, J1 {len(ref['J1'])}, J2 {len(ref['J2'])}, L {ref['L']:.6f}, |dL| {abs(ref['L'] - got['L']):.2e}")
        assert [tuple(int(v) for v in r) for r in LD.block_bounds(n, rate)] == ref["bounds"]
        assert [tuple(int(v) for v in r) for r in got["bounds"]] == ref["bounds"]
        assert list(got["J1"]) == ref["J1"] and list(got["J2"]) == ref["J2"]
        assert abs(got["L"] - ref["L"]) <= 1e-9
        assert LD.integrated_loudness_f64(x, rate) == got["L"]
        y, L_, g = LD.normalize_f32(x, rate)
        yr, Lr, gr = normalize_ref(x, rate)
        assert g == gr and np.array_equal(y, yr)
    long_ = loudness_ref(gated_signal(_lengths(rate)[-1], rate), rate)
    assert (len(long_["z"]), len(long_["J1"]), len(long_["J2"])) == (26, 24, 14 if rate == 48000 else 13)
    assert len(loudness_ref(gated_signal(_lengths(rate)[2], rate), rate)["z"]) == 2, "the last block reaches past the end"
    assert loudness_ref(gated_signal(_lengths(rate)[2], rate), rate)["bounds"][-1][1] > _lengths(rate)[2]
    assert len(loudness_ref(gated_signal(_lengths(rate)[3], rate), rate)["z"]) == 1, "rounded down to one block"


def test_the_scan_does_not_depend_on_its_chunk_length():
    """Two chunk lengths are two float64 orderings of the same recurrence. The high pass has a double pole at r = 1 - 2 pi 38 / rate (0.9892 at
    22.05 kHz): a rounding error of 2^-53 |y| made at one sample is seen again through sum_k (k + 1) r^k = 1 / (1 - r)^2 = 8.5e3, so the
    orderings may differ by about 2 * 2^-53 * 8.5e3 = 1.9e-12 of the signal's peak."""
    x = gated_signal(30011, 22050).astype(np.float64)
    a, b = LD.k_filter_f64(x, 22050, 64), LD.k_filter_f64(x, 22050, 4096)
    r = 1.0 - 2.0 * np.pi * 38.0 / 22050
    print(f"chunk 64 vs 4096: {np.abs(a - b).max() / np.abs(a).max():.2e} of the peak")
    assert np.abs(a - b).max() <= 2.0 * 2.0 ** -53 / (1.0 - r) ** 2 * np.abs(a).max()


@pytest.mark.parametrize("rate,measured", [(48000, -3.052), (44100, -3.052), (22050, -3.066), (16000, -3.083)])
def test_full_scale_997_hz_sine_reads_minus_3_01_within_the_compliance_tolerance(rate, measured):
    """+-0.1 LU is the compliance tolerance of the ITU test material (BS.2217); this filter design's high pass has b = 0.99504 (1, -2, 1) at 48 kHz,
    so the reading is -3.052 there, not -3.01."""
    t = np.arange(5 * rate) / rate
    got = LD.integrated_loudness_f64(np.sin(2 * np.pi * 997.0 * t), rate)
    print(f"{rate} Hz: {got:.4f} LKFS")
    assert abs(got - (-3.01)) <= 0.1
    assert abs(got - measured) <= 1e-3
    assert abs(loudness_ref(np.sin(2 * np.pi * 997.0 * t), rate)["L"] - got) <= 1e-9


def test_coefficients_at_48_khz_against_the_bs1770_tables():
    (b1, a1), (b2, a2) = LD.k_weighting(48000)
    t1b, t1a = [1.53512485958697, -2.69169618940638, 1.19839281085285], [1.0, -1.69065929318241, 0.73248077421585]
    t2a = [1.0, -1.99004745483398, 0.99007225036621]
    assert np.abs(b1 - t1b).max() <= 1.1e-4 and np.abs(a1 - t1a).max() <= 1.1e-4
    assert np.abs(a2 - t2a).max() <= 2.9e-5
    assert np.abs(b2 - 0.99504 * np.array([1.0, -2.0, 1.0])).max() <= 1e-5, "the high pass' numerator is NOT (1, -2, 1) in this design"
    for (b, a), (rb, ra) in zip(LD.k_weighting(48000), coefficients(48000)):
        assert np.allclose(b, rb, rtol=0, atol=1e-15) and np.allclose(a, ra, rtol=0, atol=1e-15)


@pytest.mark.parametrize("k", [0.5, 3.0])
def test_scaling_the_input_moves_the_loudness_by_20_log10_k(k):
    x = gated_signal(_lengths(48000)[-1], 48000).astype(np.float64)
    assert abs(LD.integrated_loudness_f64(k * x, 48000) - LD.integrated_loudness_f64(x, 48000) - 20.0 * math.log10(k)) <= 1e-9


@pytest.mark.parametrize("rate", RATES + (16000,))
def test_short_items_and_silence(rate):
    n = int(0.4 * rate)
    x = gated_signal(n, rate)
    with pytest.raises(ValueError, match="fewer than one"):
        LD.integrated_loudness_f64(x[:n - 1], rate)
    assert LD.n_blocks(n - 1, rate) == 0 and LD.segment_edges(n - 1, rate) == []
    assert len(LD.block_bounds(n, rate)) == 1 and LD.n_blocks(n, rate) == 1
    assert math.isfinite(LD.integrated_loudness_f64(x, rate))
    z = np.zeros(2 * n, dtype=np.float32)
    assert LD.integrated_loudness_f64(z, rate) == -math.inf
    y, L_, g = LD.normalize_f32(z, rate)
    assert g == np.float32(1.0) and np.array_equal(y, z)
    e = LD.segment_edges(int(0.46 * rate), rate)
    assert len(e) == 2 + 4 and e[-1] == int(0.46 * rate) and e[0] == 0 and all(b > a for a, b in zip(e, e[1:]))


def test_the_opt_in_resolver():
    assert LD.resolve_loudness(dict(loud_norm=True), "bs1770") is True
    with pytest.raises(NotImplementedError, match="loud_norm") as ei:
        LD.resolve_loudness(dict(loud_norm=True))
    assert 'loudness="bs1770"' in str(ei.value) and "unpinned" in str(ei.value)
    assert LD.resolve_loudness(dict(loud_norm=False), "bs1770") is False and LD.resolve_loudness(None, "bs1770") is False
    assert LD.resolve_loudness(None) is False and LD.resolve_loudness({}) is False
    for bad in ("pyloudnorm", "BS1770", True, 1770):
        with pytest.raises(ValueError, match="loudness="):
            LD.resolve_loudness(dict(loud_norm=True), bad)
    from stylesinger_amd.infer import StyleSingerInfer
    with pytest.raises(ValueError, match="loudness="):
        StyleSingerInfer(dict(loud_norm=True), device="cuda", loudness="ebu")       # refused before anything touches a device
    with pytest.raises(ValueError, match="out_wav_norm"):
        StyleSingerInfer(dict(out_loudness_lufs=-16.0, out_wav_norm=True), device="cuda")


def test_device_entry_points_refuse_host_tensors():
    import torch
    for fn in (LD.measure_batch, LD.normalize_batch):
        with pytest.raises(lib.StyleSingerHipError, match="device tensors"):
            fn(torch.zeros(1, 48000), [48000], 48000)
        with pytest.raises(lib.StyleSingerHipError, match="device tensors"):
            fn(np.zeros((1, 48000), dtype=np.float32), [48000], 48000)


def test_device_table_holds_the_chunk_transition_powers():
    tab = LD.device_table(22050, 64)
    assert tab.shape == (108,) and tab[10] == 0.4 * 22050
    M = tab[12:28].reshape(4, 4)
    for i in range(6):
        assert np.allclose(tab[12 + 16 * i:28 + 16 * i].reshape(4, 4), np.linalg.matrix_power(M, 2 ** i), rtol=1e-12, atol=1e-300)
    # M is the state after one chunk of zeros: run the restatement's two stages on an impulse response basis
    (b, a), (g, d) = LD.k_weighting(22050)
    A = np.array([[-a[1], 1, 0, 0], [-a[2], 0, 0, 0], [g[1] - d[1] * g[0], 0, -d[1], 1], [g[2] - d[2] * g[0], 0, -d[2], 0]])
    assert np.allclose(M, np.linalg.matrix_power(A, 64), rtol=1e-10, atol=1e-300)


def test_loudness_argument_errors_are_reported_before_a_device_is_touched():
    l = lib.load()
    for name in ("ss_loudness_measure", "ss_loudness_apply", "ss_loudness_workspace_bytes"):
        assert name in lib.declared_symbols()
    p = 0x1000   # placeholder non-null pointers: every refusal below comes before anything is dereferenced or launched
    need = l.ss_loudness_workspace_bytes(2, 1000, 256)
    assert need == 2 * 4 * (10 * 8) + 2 * 4 * 4 and l.ss_loudness_workspace_bytes(2, 1000, 100) < 0

    def measure(x=p, ldx=1000, Lx=1000, n=p, nb=p, edges=p, lde=8, B=2, tab=p, C=256, target=-22.0, lufs=p, gain=p, peak=p, z=p, ldz=4, ws=p, wsb=need):
        return l.ss_loudness_measure(x, ldx, Lx, n, nb, edges, lde, B, tab, C, target, lufs, gain, peak, z, ldz, ws, wsb, None)
    assert measure(x=None) != 0 and b"ss_loudness_measure: null argument" in l.ss_last_error()
    assert measure(z=None) != 0 and b"null argument" in l.ss_last_error()
    assert measure(ldx=999) != 0 and b"bad dims" in l.ss_last_error()
    assert measure(B=65536) != 0 and b"bad dims" in l.ss_last_error()
    assert measure(lde=4) != 0 and b"bad dims" in l.ss_last_error()
    assert measure(C=100) != 0 and b"bad chunk" in l.ss_last_error()
    assert measure(C=8192) != 0 and b"bad chunk" in l.ss_last_error()
    assert measure(target=float("nan")) != 0 and b"bad target" in l.ss_last_error()
    assert measure(wsb=need - 1) != 0 and b"workspace" in l.ss_last_error()
    assert measure(ws=p + 4) != 0 and b"workspace" in l.ss_last_error()

    def apply(x=p, ldx=8, Lx=8, n=p, gain=p, peak=p, y=2 * p, ldy=8, Ly=8, B=1):
        return l.ss_loudness_apply(x, ldx, Lx, n, gain, peak, y, ldy, Ly, B, None)
    assert apply(gain=None) != 0 and b"ss_loudness_apply: null argument" in l.ss_last_error()
    assert apply(ldy=4) != 0 and b"bad dims" in l.ss_last_error()
    assert apply(B=0) != 0 and b"bad dims" in l.ss_last_error()
    assert apply(y=p) != 0 and b"alias" in l.ss_last_error()
    assert l.ss_abi_version() == 20, "the export is additive"
