"""Seeded synthetic items for the "lrt" voice-activity decision (stylesinger_amd/vadtrim.py::lrt_statistic, `ss_vad_lrt`), shared by
tests/test_vad_lrt_cpu.py and tests/test_gpu_vad_lrt.py. There are no recordings here: every item is a sum of harmonics with raised-cosine
edges around its pauses plus white noise at a stated level (None = none: digital silence in the pauses), at the nominal 16 kHz of the emotion
branch (30 ms windows of 480 samples)."""
import functools

import numpy as np

SPW = 480


def harmonic_item(n, voiced, noise_dbfs, seed, f0=220.0, amp=0.3, edge=160, sr=16000, n_harm=6):
    """n samples: harmonics h = 1 .. n_harm of f0 (amplitude 1 / h, seeded phases), scaled to a peak of about `amp`, switched on inside the
    sample ranges `voiced` = [(a, b), ...] with raised-cosine edges of `edge` samples inside each range, plus white noise of `noise_dbfs`
    dB re full scale (rms). float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / sr
    sig = np.zeros(n)
    for h in range(1, n_harm + 1):
        sig += np.sin(2.0 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi)) / h
    sig *= amp / 1.8
    env = np.zeros(n)
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(edge) + 0.5) / edge)
    for a, b in voiced:
        env[a:b] = 1.0
        e = min(edge, (b - a) // 2)
        env[a:a + e] = ramp[:e]
        env[b - e:b] = ramp[:e][::-1]
    x = sig * env
    if noise_dbfs is not None:
        x = x + rng.standard_normal(n) * 10.0 ** (noise_dbfs / 20.0)
    return x.astype(np.float32)


def expected_windows(n, voiced, edge=160):
    """(indices of the windows that lie wholly inside a voiced range, its edges excluded; indices of the windows that touch no voiced range)."""
    nw = n // SPW
    on, off = [], []
    for w in range(nw):
        lo, hi = w * SPW, (w + 1) * SPW
        if any(a + edge <= lo and hi <= b - edge for a, b in voiced):
            on.append(w)
        if all(hi <= a or lo >= b for a, b in voiced):
            off.append(w)
    return np.array(on, dtype=np.int64), np.array(off, dtype=np.int64)


def _w(*ranges):
    return [(a * SPW, b * SPW) for a, b in ranges]


# name -> (n samples, voiced ranges, noise dBFS, seed, keyword overrides, kind). kind: "clean" = the flags must follow the pauses;
# "all" = every window must be flagged; "none" = no window may be flagged; "any" = only the comparison with the device is made
_SPECS = {
    "nw0": (479, [(0, 479)], None, 1, {}, "none"),
    "nw1": (SPW + 17, [(0, SPW + 17)], None, 2, {}, "all"),
    "nw9": (9 * SPW + 100, _w((0, 5)), None, 3, {}, "clean"),                 # q = 1
    "nw10": (10 * SPW + 479, _w((3, 8)), None, 4, {}, "clean"),               # q = 1
    "nw11": (11 * SPW + 1, _w((0, 4), (8, 11)), None, 5, {}, "clean"),        # q = 2
    "nw33": (33 * SPW + 240, _w((2, 12), (24, 33)), -60.0, 6, {}, "any"),     # q = 4: too few noise windows for a stable noise spectrum
    "nw1000": (1000 * SPW + 333, _w((20, 180), (240, 400), (470, 700), (760, 990)), -60.0, 7, {}, "clean"),
    "pauses": (166 * SPW + 320, _w((10, 60), (104, 157)), -60.0, 8, {}, "clean"),   # 5 s with a pause of 44 windows = 1.32 s
    "silence": (33 * SPW + 7, [], None, 9, {}, "none"),                       # all E tie: index order decides
    "nopause": (100 * SPW, [(0, 100 * SPW)], -60.0, 10, {}, "all"),           # the peak rule fires
    "snr20": (200 * SPW, _w((20, 90), (120, 180)), -36.8, 11, {}, "all"),     # 20 dB SNR (the tone's rms is -16.8 dBFS): the peak rule again
    "clip": (60 * SPW + 5, _w((5, 25), (40, 55)), -60.0, 12, dict(amp=1.8), "clean"),   # samples outside [-1, 1]
}
CASES = tuple(_SPECS)
BATCH3 = ("pauses", "nw33", "nw11")      # three unequal lengths in one buffer


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (wav float32 [n], n, voiced ranges, kind)"""
    n, voiced, noise, seed, kw, kind = _SPECS[name]
    x = harmonic_item(n, voiced, noise, seed, **kw)
    x.setflags(write=False)
    return x, n, voiced, kind


def dft_power(wav, n):
    """`vadtrim.lrt_power` with a direct float64 DFT (one dot product per bin) in place of numpy's FFT: the second evaluation of the definition."""
    from stylesinger_amd import vadtrim as V
    x = np.asarray(wav, dtype=np.float32)
    nw = n // SPW
    p = np.clip(np.rint(x[:nw * SPW].astype(np.float64) * 32767.0), -32768.0, 32767.0).reshape(nw, SPW)
    k = np.arange(V.LRT_K_LO, V.LRT_K_HI + 1)
    ang = -2.0 * np.pi * ((k[:, None] * np.arange(SPW)[None, :]) % V.LRT_N_FFT) / V.LRT_N_FFT
    fr = p * V.lrt_window(SPW)
    re, im = fr @ np.cos(ang).T, fr @ np.sin(ang).T
    return re * re + im * im


@functools.lru_cache(maxsize=None)
def host(name):
    """-> (stat, flags) of `lrt_statistic` for the case: computed once, shared, read-only"""
    from stylesinger_amd import vadtrim as V
    x, n, _, _ = case(name)
    stat, flags = V.lrt_statistic(x, n)
    stat.setflags(write=False)
    flags.setflags(write=False)
    return stat, flags


@functools.lru_cache(maxsize=None)
def definition_spread():
    """The float64 spread of the definition itself: the largest |stat_fft - stat_dft| / (1 + |stat_fft|) over all cases, `stat` evaluated once
    with numpy's FFT (`lrt_statistic`) and once with the direct DFT above. -> (spread, {case: its own})"""
    from stylesinger_amd import vadtrim as V
    per = {}
    for name in CASES:
        x, n, _, _ = case(name)
        a = host(name)[0]
        b, _ = V.lrt_from_power(dft_power(x, n))
        per[name] = float(np.max(np.abs(a - b) / (1.0 + np.abs(a)))) if len(a) else 0.0
    return max(per.values()), per


def tol():
    """TOL of the device comparison: 16 x the spread of the definition (the factor covers a third summation order, the kernel's)."""
    return 16.0 * definition_spread()[0]


def batch_buffer(names, junk):
    """The items `names` as rows of one float32 buffer [B, longest + 2 * SPW]; what lies at and beyond each item's length is `junk`
    (0.0, or e.g. 1000.0: then +-1000 alternating). -> (buffer, lengths)"""
    items = [case(k) for k in names]
    L = max(n for _, n, _, _ in items) + 2 * SPW
    buf = np.zeros((len(items), L), dtype=np.float32)
    if junk:
        buf[:] = junk * (1 - 2 * (np.arange(L) % 2)).astype(np.float32)
    for i, (x, n, _, _) in enumerate(items):
        buf[i, :n] = x
    return buf, [n for _, n, _, _ in items]
