"""Float64 restatement of the resampler's definition for the tests (stylesinger_amd/resample.py's docstring; resampy's `kaiser_best` form): the
direct loop over the outputs, each one interpolating the filter table on the fly for its two wings - NOT through `polyphase_bank`, so that the
bank builder is checked against an independent statement. Only the time of an output is taken as exact integers (t * down / up) where the package
accumulates a float."""
import functools
import math

import numpy as np


@functools.lru_cache(maxsize=None)
def _table():
    num_zeros, num_table = 64, 512
    n = num_table * num_zeros
    win = np.kaiser(2 * n + 1, 14.769656459379492)[n:] * 0.9475937167399596 * np.sinc(0.9475937167399596 * np.linspace(0, num_zeros, n + 1))
    return win, num_table


def resample_f64(x, sr_in, sr_out, with_bound=False):
    """x float64 [n_in] -> y float64 [ceil(n_in * sr_out / sr_in)] (the last sample zero where the product is no integer); with_bound: also
    sum_j |w_j| |x_j| per output, the scale of the fp32 forward error bound."""
    x = np.asarray(x, dtype=np.float64)
    if sr_in == sr_out:
        return (x, np.abs(x)) if with_bound else x
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    win, num_table = _table()
    ratio = sr_out / sr_in
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    nwin = len(win)
    scale = min(1.0, ratio)
    step = int(scale * num_table)
    n_in = len(x)
    n_out = -((-n_in * up) // down)
    y, s = np.zeros(n_out), np.zeros(n_out)
    ax = np.abs(x)
    for t in range(n_in * up // down):
        q = t * down
        n, fr = q // up, (q % up) / up
        # left wing: inputs n, n - 1, ...
        idx = scale * fr * num_table
        off = int(idx)
        eta = idx - off
        i = np.arange(min(n + 1, (nwin - off) // step))
        w = win[off + i * step] + eta * delta[off + i * step]
        acc, sacc = np.dot(w, x[n - i]), np.dot(np.abs(w), ax[n - i])
        # right wing: inputs n + 1, n + 2, ...
        idx = (scale - scale * fr) * num_table
        off = int(idx)
        eta = idx - off
        k = np.arange(max(0, min(n_in - n - 1, (nwin - off) // step)))
        w = win[off + k * step] + eta * delta[off + k * step]
        y[t] = acc + np.dot(w, x[n + 1 + k])
        s[t] = sacc + np.dot(np.abs(w), ax[n + 1 + k])
    return (y, s) if with_bound else y
