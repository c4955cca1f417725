"""The inputs of the limiter tests (tests/test_limiter_cpu.py checks them on the reference alone, tests/test_gpu_limiter.py runs the kernel on
them): built once per process, never modified. 48 kHz, ceiling -1 dBFS; the kernel's tile is 1856 samples, the filter's left wing 63 taps.

Every signal is SETTLED: scaled by the first factor 1 + 0.004 i at which `n_limited` is decided by the reference alone at the widest window (no
e[t] within the fp32 bound of the ceiling, no r[t] closer to 1 than a sum of LIMIT_MAX_W fp32 minima can resolve - tests/limiter_ref.py). A
narrower window asks for less, so one scale serves every W."""
import functools

import numpy as np

from limiter_ref import count_decided, envelope_ref
from stylesinger_amd.limiter import LIMIT_MAX_W, ceiling_f32

SR = 48000
CEILING_DB = -1.0
C = ceiling_f32(CEILING_DB)
TILE = 1856
LEFT = 63
WINDOWS = (1, 2, 96, LIMIT_MAX_W)
N_LONG = 2 * TILE + 517          # two tiles plus a remainder


def settle(x, gain=None):
    x = np.asarray(x, dtype=np.float32)
    for i in range(200):
        xk = (np.float32(1.0 + 0.004 * i) * x).astype(np.float32)
        xp = xk if gain is None else (np.float32(gain) * xk).astype(np.float32)
        e, de = envelope_ref(xp.astype(np.float64), SR)
        if count_decided(e, de, float(C), LIMIT_MAX_W):
            return xk
    raise AssertionError("no scale settles this signal")


def _peaks(n, where):
    x = np.zeros(n, dtype=np.float32)
    for k, t in enumerate(where):
        x[t] = 1.0 if k % 2 == 0 else -0.97
    return x


def bursty(rng, n, density=0.02):
    """a floor of +-0.1 with sparse bursts of +-1.6 .. 2.2 (at least one): peaks above the ceiling whose filter tails stay well under it, so that
    few envelope values fall near the ceiling and a scale that settles the signal exists"""
    x = 0.1 * rng.uniform(-1.0, 1.0, n)
    hit = rng.uniform(size=n) < density
    if n:
        hit[rng.integers(n)] = True
    x[hit] = rng.choice([-1.0, 1.0], hit.sum()) * rng.uniform(1.6, 2.2, hit.sum())
    return x.astype(np.float32)


def inter_sample_sine(n, amp=1.0):
    """fs / 4 at 45 degrees: samples of +-amp / sqrt 2, a true peak of amp between them"""
    return (amp * np.sin(0.5 * np.pi * np.arange(n) + 0.25 * np.pi)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def cases():
    """-> [(name, x float32)]"""
    rng = np.random.default_rng(20261020)
    out = []
    # lengths: empty, one sample, shorter than the left wing, shorter than the 96-sample window, around one tile, two tiles and a remainder
    for n in (0, 1, 40, 80, TILE - 1, TILE, TILE + 1, N_LONG):
        out.append((f"len_{n}", settle(bursty(rng, n))))
    # one full-scale sample: first, last, the first and the last sample of a tile, either side of a tile boundary within every window >= 96
    for name, where in (("first", [0]), ("last", [N_LONG - 1]), ("tile_start", [TILE]), ("tile_end", [TILE - 1]), ("before_tile", [TILE - 40]),
                        ("after_tile", [TILE + 40]), ("both_sides", [TILE - 30, TILE + 25]),
                        # two peaks closer than W (1 < 2; 50 < 96), between W and 2 W apart (3: W = 2; 150: W = 96; 800: W = 512)
                        ("apart_1", [3000, 3001]), ("apart_3", [3000, 3003]), ("apart_50", [1000, 1050]), ("apart_150", [1000, 1150]),
                        ("apart_800", [500, 1300])):
        out.append(("peak_" + name, settle(_peaks(N_LONG, where))))
    out.append(("sine_fs4", settle(inter_sample_sine(3000))))
    out.append(("loud", settle((rng.choice([-1.0, 1.0], N_LONG) * rng.uniform(1.5, 4.0, N_LONG)).astype(np.float32))))
    out.append(("quiet", settle((0.01 * rng.standard_normal(N_LONG)).astype(np.float32))))
    for _, x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def gain_case():
    """-> ([x0, x1] float32, target LUFS, [g0, g1] fp32): two items long enough for the BS.1770 meter (>= 0.4 s) and quiet enough that the gain to
    `target` lifts their bursts over the ceiling. Scaling x does not move x' = gain x here (the gain undoes it), so the signal is settled by
    the TARGET: the first -14 - 0.05 i LUFS at which both counts are decided. The gains are the host definition's (`loudness.gain_f32`)."""
    from stylesinger_amd import loudness as LD
    rng = np.random.default_rng(7)
    xs = [(0.05 * bursty(rng, n, density=0.003)).astype(np.float32) for n in (19600, 19300)]   # a high crest factor
    Ls = [LD.integrated_loudness_f64(x, SR) for x in xs]
    for i in range(200):
        target = -14.0 - 0.05 * i
        gs = [LD.gain_f32(L_, target) for L_ in Ls]
        ok = True
        for x, g in zip(xs, gs):
            e, de = envelope_ref((g * x).astype(np.float32).astype(np.float64), SR)
            ok = ok and count_decided(e, de, float(C), LIMIT_MAX_W)
        if ok:
            for x in xs:
                x.setflags(write=False)
            return xs, target, gs
    raise AssertionError("no target settles the gain case")
