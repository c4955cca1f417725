"""Pitch control, host side (no GPU): the two exports and their argument checks, the float64 definition of the contour fit
(stylesinger_amd/pitch.py::contour_fit) against hand-computed values, and the argument checks of StyleSingerHIP.forward that fire before any
device work."""
import numpy as np
import pytest
import torch

from stylesinger_amd import config, lib
from stylesinger_amd.pitch import contour_fit

# six source frames with one unvoiced gap (frames 2 and 3)
SRC = np.array([100.0, 200.0, 0.0, 0.0, 400.0, 800.0])


def test_exports_are_declared_and_refuse_bad_arguments_before_a_device_is_touched():
    l = lib.load()
    names = lib.declared_symbols()
    assert "ss_pitch_given" in names and "ss_contour_fit" in names
    p = 0x1000   # placeholder non-null pointers: every refusal below comes before anything is dereferenced or launched
    assert l.ss_pitch_given(None, None, None, None, None, None, 1, None) != 0 and b"ss_pitch_given" in l.ss_last_error()
    assert l.ss_pitch_given(p, p, p, p, p, None, 8, None) != 0 and b"ss_pitch_given: null pointer" in l.ss_last_error()
    assert l.ss_pitch_given(p, p, p, p, p, p, 0, None) != 0 and b"ss_pitch_given: n=0" in l.ss_last_error()
    assert l.ss_pitch_given(p, p, p, p, p, p, -3, None) != 0 and b"ss_pitch_given: n=-3" in l.ss_last_error()
    assert l.ss_contour_fit(None, 0, 0, None, None, 0.0, None, 0, 0, 1, None) != 0 and b"ss_contour_fit" in l.ss_last_error()
    assert l.ss_contour_fit(p, 8, 8, p, None, 0.0, 2 * p, 8, 8, 1, None) != 0 and b"ss_contour_fit: null pointer" in l.ss_last_error()
    assert l.ss_contour_fit(p, 8, 8, p, p, 0.0, 2 * p, 8, 8, 0, None) != 0 and b"bad dims" in l.ss_last_error()
    assert l.ss_contour_fit(p, 4, 8, p, p, 0.0, 2 * p, 8, 8, 1, None) != 0 and b"bad dims" in l.ss_last_error()       # ldc < Lc
    assert l.ss_contour_fit(p, 8, 8, p, p, 0.0, 2 * p, 4, 8, 1, None) != 0 and b"bad dims" in l.ss_last_error()       # ldo < T
    assert l.ss_contour_fit(p, 8, 8, p, p, 49.0, 2 * p, 8, 8, 1, None) != 0 and b"semitones" in l.ss_last_error()
    assert l.ss_contour_fit(p, 8, 8, p, p, float("nan"), 2 * p, 8, 8, 1, None) != 0 and b"semitones" in l.ss_last_error()
    assert l.ss_contour_fit(p, 8, 8, p, p, 0.0, p, 8, 8, 1, None) != 0 and b"alias" in l.ss_last_error()
    assert l.ss_abi_version() == 20, "the exports are additive"


def test_contour_fit_is_the_identity_at_equal_lengths():
    rng = np.random.default_rng(0)
    f = rng.uniform(80.0, 800.0, 57)
    f[rng.random(57) < 0.3] = 0.0
    assert np.array_equal(contour_fit(f, 57), f)           # bit for bit: no log2 / exp2 round trip
    assert np.array_equal(contour_fit(SRC, 6), SRC)
    assert contour_fit(SRC, 0).shape == (0,) and np.array_equal(contour_fit(np.zeros(0), 4), np.zeros(4))
    assert np.array_equal(contour_fit(np.zeros(9), 5), np.zeros(5))      # nothing voiced stays nothing voiced


def test_contour_fit_two_to_one_and_three_to_two_by_hand():
    # 6 -> 3: s = 2 t + 0.5 = 0.5, 2.5, 4.5: every frame is a tie, which goes to the later source frame; both neighbours voiced -> the
    # geometric mean (log2-linear at fr = 1/2); frames 2 | 3 are both unvoiced -> 0
    want3 = np.array([np.sqrt(100.0 * 200.0), 0.0, np.sqrt(400.0 * 800.0)])
    assert np.allclose(contour_fit(SRC, 3), want3, rtol=1e-14, atol=0)
    assert contour_fit(SRC, 3)[1] == 0.0
    # 6 -> 4: s = 1.5 t + 0.25 = 0.25, 1.75, 3.25, 4.75
    #   t = 0: i0 = 0, fr = 1/4, nearest 0 (voiced), both voiced -> 100 * 2^(1/4)
    #   t = 1: i0 = 1, fr = 3/4, nearest 2 (unvoiced)            -> 0
    #   t = 2: i0 = 3, fr = 1/4, nearest 3 (unvoiced)            -> 0
    #   t = 3: i0 = 4, fr = 3/4, nearest 5 (voiced), both voiced -> 400 * 2^(3/4)
    want4 = np.array([100.0 * 2 ** 0.25, 0.0, 0.0, 400.0 * 2 ** 0.75])
    assert np.allclose(contour_fit(SRC, 4), want4, rtol=1e-14, atol=0)
    # 6 -> 12 (1:2): s = t / 2 - 0.25 clamped at both ends; next to the gap the value is the voiced neighbour's, not an interpolation with 0
    want12 = np.array([100.0, 100.0 * 2 ** 0.25, 100.0 * 2 ** 0.75, 200.0, 0.0, 0.0, 0.0, 0.0, 400.0, 400.0 * 2 ** 0.25, 400.0 * 2 ** 0.75, 800.0])
    got12 = contour_fit(SRC, 12)
    assert np.allclose(got12, want12, rtol=1e-14, atol=0)
    assert got12[0] == 100.0 and got12[3] == 200.0 and got12[8] == 400.0 and got12[11] == 800.0   # clamped ends / lone voiced neighbour: exact


def test_contour_fit_shift_of_an_octave_doubles_the_voiced_values():
    for n_t in (6, 4, 12, 7):
        base, up, down = contour_fit(SRC, n_t), contour_fit(SRC, n_t, shift=12), contour_fit(SRC, n_t, shift=-12)
        assert np.array_equal(up, 2.0 * base) and np.array_equal(down, 0.5 * base)
        assert np.array_equal(up > 0, base > 0)
    one = contour_fit(SRC, 6, shift=1.0)
    assert np.allclose(one[SRC > 0], SRC[SRC > 0] * 2 ** (1 / 12), rtol=1e-15) and np.array_equal(one[SRC == 0], np.zeros(2))


def test_contour_fit_voicing_follows_the_nearest_source_frame():
    rng = np.random.default_rng(5)
    for n_c, n_t in ((40, 40), (40, 80), (40, 20), (37, 100), (100, 37), (6, 3), (5, 9)):
        f = rng.uniform(80.0, 800.0, n_c)
        f[rng.random(n_c) < 0.4] = 0.0
        got = contour_fit(f, n_t)
        s = np.clip((np.arange(n_t) + 0.5) * n_c / n_t - 0.5, 0, n_c - 1)      # the definition's position, in floating point
        near = np.minimum(np.floor(s + 0.5).astype(int), n_c - 1)             # ties (x.5) go up; exact in float64 at these sizes
        assert np.array_equal(got > 0, f[near] > 0), (n_c, n_t)
        lo, hi = np.floor(s).astype(int), np.minimum(np.floor(s).astype(int) + 1, n_c - 1)
        v = got > 0
        both = v & (f[lo] > 0) & (f[hi] > 0)
        assert (got[both] >= np.minimum(f[lo], f[hi])[both] * (1 - 1e-12)).all() and (got[both] <= np.maximum(f[lo], f[hi])[both] * (1 + 1e-12)).all()
        assert np.array_equal(got[v & ~both], f[near][v & ~both])              # a lone voiced neighbour's value, untouched


def test_forward_argument_checks_fire_before_any_device_work():
    """A model built on the CPU (no device, no packed weights): the refusals below come from the argument checks at the top of forward."""
    from stylesinger_amd.model import StyleSingerHIP
    m = StyleSingerHIP(None, hparams=config.make_hparams(dict(timesteps=2, K_step=2, f0_timesteps=2)))
    m.eval()
    txt = torch.ones(1, 3, dtype=torch.long)
    f0, uv, hz = torch.full((1, 8), 8.0), torch.zeros(1, 8), torch.full((1, 8), 220.0)
    with pytest.raises(ValueError, match="f0 without uv"):
        m(txt, f0=f0, infer=True)
    with pytest.raises(ValueError, match="uv without f0"):
        m(txt, uv=uv, infer=True)
    with pytest.raises(ValueError, match="pitch_hz.*f0|f0.*pitch_hz"):
        m(txt, f0=f0, uv=uv, infer=True, pitch_hz=(hz, [8]))
    with pytest.raises(ValueError, match="pitch_shift"):
        m(txt, infer=True, pitch_shift=2.0)
    with pytest.raises(ValueError, match="pitch_hz"):
        m(txt, infer=True, pitch_hz=hz)
    with pytest.raises(NotImplementedError):
        m(txt, f0=f0, uv=uv, infer=False)
    with pytest.raises(NotImplementedError):
        m(txt, infer=False)
