"""Inputs shared by tests/test_evaluate_cpu.py and tests/test_gpu_evaluate.py: quantised cepstra, mels and contours small enough to check by hand or
by the scalar definition (stylesinger_amd/evaluate.py), built from a seed."""
import numpy as np

VMIN, VMAX = -6.0, 1.5        # config.DEFAULT_HPARAMS mel_vmin / mel_vmax
KP = 24


def random_q(rng, n, Kp=KP, amp=4000):
    """|q| <= 4000: S <= 24 * 8000^2 = 1.5e9 < 2^31 and every difference fits int16."""
    return rng.integers(-amp, amp + 1, (n, Kp)).astype(np.int16)


def tie_q(rng, n, Kp=KP, distinct=3):
    """Few distinct frames in long runs (silence against silence, a held vowel): zero costs and equal costs on most cells, so the path is
    decided by the tie order."""
    book = rng.integers(-300, 301, (distinct, Kp)).astype(np.int16)
    out, t = np.zeros((n, Kp), dtype=np.int16), 0
    while t < n:
        run = int(rng.integers(1, 12))
        out[t:t + run] = book[int(rng.integers(0, distinct))]
        t += run
    return out


def doubled(q):
    """Every frame twice."""
    return np.repeat(q, 2, axis=0)


def corner_mel(rng, n, n_mels=80):
    """Every bin at one end of the clip range or beyond it (+-1000 clip to the corners): the largest ||c_a - c_b|| the definition allows."""
    pick = rng.integers(0, 4, (n, n_mels))
    return np.choose(pick, [VMIN, VMAX, -1000.0, 1000.0]).astype(np.float32)


def wide_mel(rng, n, n_mels=80):
    """Log-mel-like values that reach beyond [VMIN, VMAX] on both sides."""
    return rng.uniform(VMIN - 2.0, VMAX + 2.0, (n, n_mels)).astype(np.float32)


def random_f0(rng, n):
    """Hz with unvoiced stretches; ratios of two such contours are spread over an octave (no pair closer than the float64 noise of a log2)."""
    f = rng.uniform(110.0, 440.0, n).astype(np.float32)
    f[rng.random(n) < 0.3] = 0.0
    return f


def boundary_contours():
    """(fa, fb, want): nine frames against each other frame by frame, with the fp32 values that sit exactly on and next to the 20 % rule.
    fl32(0.2) * 100 = 20.0000003 rounds to 20 in fp32, so |120 - 100| = 20 is NOT beyond it and the next fp32 above 120 is; the same below."""
    up = np.nextafter(np.float32(120.0), np.float32(np.inf))
    down = np.nextafter(np.float32(80.0), np.float32(-np.inf))
    fa = np.asarray([120.0, up, 80.0, down, 0.0, 100.0, 0.0, 100.0, 300.0], dtype=np.float32)
    fb = np.asarray([100.0, 100.0, 100.0, 100.0, 100.0, 0.0, 0.0, 100.0, 100.0], dtype=np.float32)
    return fa, fb, dict(P=9, n_both=6, n_vde=2, n_gpe=3)


THREADS = 512                 # evaluate.hip: EV_DTW_THREADS
# (n_a, n_b, band): tests/test_gpu_contour_align.py::SHAPES - the smallest shapes that reach a distinct path of the sweep
SHAPES = [(1, 1, None), (1, 7, None), (7, 1, None),
          (37, 53, None), (53, 37, 4),
          (66, 62, 16), (62, 66, None), (66, 62, None), (62, 66, 16),
          (THREADS + 3, THREADS - 3, 16), (THREADS - 3, THREADS + 3, None),
          (THREADS + 3, THREADS - 3, None), (THREADS - 3, THREADS + 3, 16)]
