"""Independent float64 restatement of the true-peak limiter's definition (stylesinger_amd/limiter.py's docstring), in literal loops: nothing is
shared with that module beyond `resample.polyphase_bank_f64`. With `with_bound` it also carries the fp32 forward-error bound of the device form
through every step (the derivation the GPU test asserts against), and says whether the item's `n_limited` is decided by the reference alone.

Bound, u = 2^-24 (x' = fl32(G x) and c = fl32(10^(dB / 20)) are the SAME fp32 values on both sides, so they carry no error):
  e   the device sums `taps` products of fp32-rounded weights in one FMA chain per phase: |e_dev - e| <= de = (taps + 2) u max_p sum_k |w_pk| |x'|
      (one roundoff per rounded weight, taps for the chain: the bound tests/test_gpu_resample.py derives; |x'[t]| itself is exact, and
      |max a - max b| <= max |a_i - b_i|).
  r   e + de <= c: both sides give exactly 1, dr = 0. Otherwise |c / e_dev - c / e| <= c de / (e (e - de)), plus u for the rounded division
      (r <= 1), and min(1, .) does not expand a distance: dr = min(1, c de / (e (e - de)) + u).
  m   a minimum over a window does not expand the sup distance: dm[j] = max of dr over [j, j + W - 1].
  g   the device adds the W minima in one fp32 chain and divides once: |mean_dev - mean| <= mean(dm) + gamma (mean(m) + mean(dm)) with
      gamma = (W + 1) u / (1 - (W + 1) u); min(r, mean) again does not expand: dg = max(dr, that).
  y   y_dev = fl32(g_dev x'): dy = dg |x'| + u (g + dg) |x'|.
n_limited is decided when every r[t] is either surely 1 on the device (e + de <= c) or surely below 1 by more than the fp32 sum of W minima can
swallow: r + dr <= 1 - 2 W (W + 2) u (a sum of W terms <= 1 of which one is <= 1 - d rounds below W, and its quotient below 1, once
d > W (W + 1) u; twice that is asked for)."""
import numpy as np

from stylesinger_amd.resample import polyphase_bank_f64

U = 2.0 ** -24


def envelope_ref(xp, sr):
    """x' float64 [n] -> (e, de): the peak envelope and the fp32 forward bound of the device's."""
    bank, up, down, taps, left = polyphase_bank_f64(int(sr), 4 * int(sr))
    assert (up, down) == (4, 1)
    n = len(xp)
    xz = np.zeros(n + taps)                 # xz[i] = x'[i - left]
    xz[left:left + n] = xp
    e = np.abs(xp)
    de = np.zeros(n)
    w32 = np.abs(bank.astype(np.float32).astype(np.float64))
    for p in range(4):
        acc, sab = np.zeros(n), np.zeros(n)
        for k in range(taps):
            acc += bank[p, k] * xz[k:k + n]
            sab += w32[p, k] * np.abs(xz[k:k + n])
        e = np.maximum(e, np.abs(acc))
        de = np.maximum(de, (taps + 2) * U * sab)
    return e, de


def gain_bound(e, de, c):
    """-> (sure_one, dr): where the device's r is exactly 1, and the bound on |r_dev - r| elsewhere."""
    sure_one = e + de <= c
    with np.errstate(divide="ignore", invalid="ignore"):
        dr = np.where(e - de > 0.0, c * de / (e * (e - de)) + U, 1.0)
    return sure_one, np.where(sure_one, 0.0, np.minimum(1.0, dr))


def count_decided(e, de, c, W):
    sure_one, dr = gain_bound(e, de, c)
    with np.errstate(divide="ignore"):
        r = np.minimum(1.0, c / e)
    return bool(np.all(sure_one | (r + dr <= 1.0 - 2.0 * W * (W + 2) * U)))


def limiter_ref(x, sr, c, W, gain=None, with_bound=False):
    """x float32 [n], c the fp32 ceiling (linear), W samples, gain None or an fp32 scalar ->
    dict(xp, e, r, m (t = -(W - 1) .. n - 1), g, y, min_gain, n_limited[, de, dr, dg, dy, decided])"""
    x = np.asarray(x, dtype=np.float32)
    xp32 = x if gain is None else (np.float32(gain) * x).astype(np.float32)
    xp = xp32.astype(np.float64)
    n, c, W = len(xp), float(c), int(W)
    e, de = envelope_ref(xp, sr)
    r = np.ones(n)
    for t in range(n):
        if e[t] > 0.0:
            r[t] = min(1.0, c / e[t])
    H = W - 1
    m = np.ones(n + H)                      # m[i] = the minimum over the samples [i - H, i] that lie inside the item
    for i in range(n + H):
        lo, hi = max(i - H, 0), min(i + 1, n)
        if hi > lo:
            m[i] = min(1.0, r[lo:hi].min())
    g = np.ones(n)
    for t in range(n):
        g[t] = min(r[t], m[t:t + W].sum() / W)   # the minima of the windows that start at t - H .. t
    out = dict(xp=xp32, e=e, r=r, m=m, g=g, y=g * xp, min_gain=float(g.min()) if n else 1.0, n_limited=int((g < 1.0).sum()), c=c, W=W)
    if with_bound:
        sure_one, dr = gain_bound(e, de, c)
        dm = np.zeros(n + H)
        for i in range(n + H):
            lo, hi = max(i - H, 0), min(i + 1, n)
            if hi > lo:
                dm[i] = dr[lo:hi].max()
        gamma = (W + 1) * U / (1.0 - (W + 1) * U)
        dg = np.zeros(n)
        for t in range(n):
            a, b = dm[t:t + W].mean(), m[t:t + W].mean()
            dg[t] = max(dr[t], a + gamma * (a + b))
        dy = dg * np.abs(xp) + U * (g + dg) * np.abs(xp)
        out.update(de=de, dr=dr, dg=dg, dy=dy, decided=count_decided(e, de, c, W))
    return out
