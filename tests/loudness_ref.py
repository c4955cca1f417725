"""Independent restatement of the BS.1770 integrated loudness that stylesinger_amd/loudness.py defines (parity with pyloudnorm UNPINNED: the
package is un-vendored): scipy's `lfilter` per biquad stage, the gating blocks as a literal loop, the gates as list comprehensions. Nothing is
imported from the module under test."""
import math

import numpy as np
from scipy.signal import lfilter

T_G, STEP = 0.4, 0.25


def coefficients(rate):
    """[(b, a) high shelf, (b, a) high pass], each divided by its a0"""
    out = []
    G, Q, fc = 4.0, 1.0 / math.sqrt(2.0), 1500.0
    A = 10.0 ** (G / 40.0)
    w0 = 2.0 * math.pi * fc / rate
    alpha, c = math.sin(w0) / (2.0 * Q), math.cos(w0)
    s = 2.0 * math.sqrt(A) * alpha
    b = [A * ((A + 1) + (A - 1) * c + s), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - s)]
    a = [(A + 1) - (A - 1) * c + s, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - s]
    out.append(([v / a[0] for v in b], [v / a[0] for v in a]))
    Q, fc = 0.5, 38.0
    w0 = 2.0 * math.pi * fc / rate
    alpha, c = math.sin(w0) / (2.0 * Q), math.cos(w0)
    b = [(1 + c) / 2, -(1 + c), (1 + c) / 2]
    a = [1 + alpha, -2 * c, 1 - alpha]
    out.append(([v / a[0] for v in b], [v / a[0] for v in a]))
    return out


def loudness_ref(x, rate):
    """-> dict(L, z, l, J1, J2, bounds) for a mono signal; ValueError when it is shorter than one block"""
    y = np.asarray(x, dtype=np.float64)
    n = len(y)
    if n < T_G * rate:
        raise ValueError("shorter than one gating block")
    for b, a in coefficients(rate):
        y = lfilter(b, a, y)
    nb = int(np.round((n / rate - T_G) / (T_G * STEP)) + 1)
    bounds, z = [], []
    for j in range(nb):
        lo = int(T_G * (j * STEP) * rate)
        hi = int(T_G * (j * STEP + 1) * rate)
        bounds.append((lo, hi))
        acc = y[lo:hi]          # (a slice past the end is truncated)
        z.append(float(np.sum(acc * acc)) / (T_G * rate))
    l = [-0.691 + 10.0 * math.log10(v) if v > 0 else -math.inf for v in z]
    J1 = [j for j in range(nb) if l[j] >= -70.0]
    if not J1:
        return dict(L=-math.inf, z=z, l=l, J1=J1, J2=[], bounds=bounds)
    rel = -0.691 + 10.0 * math.log10(sum(z[j] for j in J1) / len(J1)) - 10.0
    J2 = [j for j in range(nb) if l[j] > rel and l[j] > -70.0]
    L = -0.691 + 10.0 * math.log10(sum(z[j] for j in J2) / len(J2)) if J2 else -math.inf
    return dict(L=L, z=z, l=l, J1=J1, J2=J2, bounds=bounds, rel=rel)


def normalize_ref(x32, rate, target=-22.0):
    """numpy 1.21 semantics spelled out in fp32: -> (y, L, g32)"""
    x32 = np.asarray(x32, dtype=np.float32)
    L = loudness_ref(x32, rate)["L"]
    g = np.float32(10.0 ** ((target - L) / 20.0)) if math.isfinite(L) else np.float32(1.0)
    y = (g * x32).astype(np.float32)
    P = np.float32(g * np.float32(np.abs(x32).max()))
    if P > 1:
        y = (y / P).astype(np.float32)
    return y, L, g


def gated_signal(n, rate):
    """noise + DC + a 20 Hz component (the high pass' carry across chunks) under a three-level envelope: full scale, -30 dB, 1e-5"""
    rng = np.random.default_rng(n)
    t = np.arange(n) / rate
    x = 0.1 * rng.standard_normal(n) + 0.05 + 0.05 * np.sin(2 * np.pi * 20.0 * t)
    env = np.full(n, 1e-5)
    env[:int(0.8 * n)] = 10.0 ** (-30.0 / 20.0)
    env[:int(0.45 * n)] = 1.0
    return (x * env).astype(np.float32)
