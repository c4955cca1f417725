"""Shared inputs, references and helpers of the f0 tracker's per-stage tests (CPU only: numpy + oracle/praat_pitch.py).

`tests/test_gpu_f0track_stages.py` calls `ss_f0track` (csrc/f0track.hip) with a workspace it owns and reads every stage back from it;
`tests/test_f0track_stages_cpu.py` checks what this module claims about its own inputs and constants. Nothing here touches a device.

The stages and what each is held to:
  gpeak, intensity   float64 numpy with the mean's sum in np.longdouble. Every input here is fp16-valued, so the sums are exact and gpeak must be
                     EQUAL; intensity within 4 ulp; the markers (0.0 silent item, -1.0 silent frame) exact.
  R[k]               direct summation of the windowed frame in np.longdouble / (r0 * window_r[k]), every lag 0 .. nlag, against the DERIVED bound
                     |dR[k]| <= 2 * nsamp_window * 2^-53 / window_r[k]  (`r_bound`): nsamp_window fma accumulations in the numerator and in r0, each
                     with relative error <= 2^-53 of sum_j |f_j f_{j+k}| <= r0 (Cauchy-Schwarz), and |R[k]| <= 1 / window_r[k].
  candidates         n_cand and the integer lags slot by slot EQUAL to the restatement's; frequency and strength within 10 x the SPREAD of the
                     restatement itself when its own r is perturbed by uniform noise of the R bound (`perturbation_trials`, committed as `SPREAD`). The
                     factor 10 is for what the perturbation of R does not model: the device's sin / cos / log2 differ from the host's by ulps
                     over the 140-term interpolation sum.
  viterbi            the device's own candidates, read back, through `praat_pitch.path_finder` on the host: the device contour must be float32 of
                     that selection on every frame.
  end to end         `praat_pitch.to_pitch_ac` at column lpad: zero voicing flips, frequency within the candidate bar + half an fp32 ulp.

INPUT CONDITION (`perturbation_trials(...)["stable"]`): an input is used for the exact assertions only if the restatement's own candidate count, candidate lags and
selected candidate per frame do not change under the perturbation trials. The CPU file asserts it for every input.

NOT BUILT - a frame on which the path must choose between "unvoiced" and a candidate at or above the ceiling. Such a frame cannot exist: the
path treats a candidate with f >= ceiling exactly as it treats the unvoiced one (same strength `unv`, same transition costs, the same float64
operations in the same order), so its path value EQUALS that of slot 0 bit for bit, and both the restatement's `val > best` and the device's
pick the lowest index on a tie: slot 0 always wins. The candidates at or above the ceiling of the 1500 Hz tone do run through that branch
(`v2 == false && f2 > 0` in f0t_viterbi_kernel) as nodes of the lattice, which the Viterbi-in-isolation test covers.
"""
import functools
import math

import numpy as np

from oracle import praat_pitch as P
from stylesinger_amd import f0track as FT

MAXC = 15
TRIALS = 8           # perturbation trials per input (seeds 0 .. TRIALS - 1)
GPU_MARGIN = 10.0    # device bar = GPU_MARGIN x SPREAD

# name -> (sr, hop, pitch_floor); nlag 899, 899, 825, 449, 299, 1013
GEOMETRIES = {
    "default": (48000, 256, 80.0),
    "hop128": (48000, 128, 80.0),
    "sr44100": (44100, 256, 80.0),
    "sr24000": (24000, 128, 80.0),
    "sr16000": (16000, 128, 80.0),
    "floor71": (48000, 256, 71.0),
}
GEOMETRY_NLAG = {"default": 899, "hop128": 899, "sr44100": 825, "sr24000": 449, "sr16000": 299, "floor71": 1013}
CEILING, VOICING_THRESHOLD = 800.0, 0.6


def _fp16(w):
    """what process_audio hands the tracker: samples rounded through fp16, as float32"""
    return np.asarray(w, dtype=np.float64).astype(np.float16).astype(np.float32)


def _t(n, sr):
    return np.arange(n) / float(sr)


def _complex(n, sr, f0, harmonics):
    t = _t(n, sr)
    return sum(0.25 / h * np.sin(2 * np.pi * f0 * h * t + 0.3 * h) for h in range(1, harmonics + 1))


def _silent_stretch(n):
    """eight-harmonic 220 Hz complex with a noise burst and a run of exact zeros longer than the window: silent frames inside a live item"""
    rng = np.random.default_rng(11)
    w = _complex(n, 48000, 220.0, 8) + 0.001 * rng.standard_normal(n)
    w[2560:3840] = 0.05 * rng.standard_normal(1280)
    w[6144:6144 + 3072] = 0.0
    return w


def _breathy(n):
    """the "breathy" signal of tests/test_gpu_round5.py: voicing hovers around the threshold"""
    rng = np.random.default_rng(7)
    t = _t(n, 48000)
    return sum(0.08 / h * np.sin(2 * np.pi * 240 * h * t) for h in range(1, 6)) * (0.6 + 0.4 * np.sin(2 * np.pi * 3 * t)) + 0.05 * rng.standard_normal(n)


def _quiet_on_dc(n):
    """a 207 Hz tone that drops to -60 dB of its level after a third of the item, on a DC offset: frames whose intensity is below the silence
    threshold's knee (0.03 / 1.6 x 2), so the `2 - intensity / ...` term of the unvoiced strength is positive. NOT 200 Hz: its period is 240
    samples exactly, and the windowed-sinc interpolant is discontinuous at integer lags (its 2 x 70 samples shift by one, and the raised-cosine
    window does not reach zero at its ends: a step of ~1e-6 x r). A maximum ON such a step has no well-defined Brent result - the device and
    the restatement, both correct, ended 1e-2 samples apart there (8e-3 Hz) - so no input here puts a peak on an integer lag."""
    t = _t(n, 48000)
    amp = np.where(np.arange(n) < n // 3, 0.3, 0.0003)
    return 0.0625 + amp * np.sin(2 * np.pi * 207.0 * t)


def _tone1500(n):
    """A 1500 Hz tone: a peak every 32 lags, 18 of them below maximum_lag, so all 15 places fill. On the PURE tone the four latecomers are all
    rejected (equal strengths, and the octave cost favours the early, high candidates), so a 125 Hz component at -14 dB weakens the peaks half
    its period away (lags 192, 224): per frame two latecomers REPLACE them in place (the lags end up out of order) and two are rejected."""
    t = _t(n, 48000)
    return 0.3 * np.sin(2 * np.pi * 1500.0 * t) + 0.06 * np.sin(2 * np.pi * 125.0 * t + 0.5)


def _make(name):
    if name == "tone1500":
        return _tone1500(40 * 256)
    if name == "tone1500_noise":
        return _tone1500(40 * 256) + 0.003 * np.random.default_rng(3).standard_normal(40 * 256)
    if name == "silent_stretch":
        return _silent_stretch(57 * 256)
    if name == "constant":
        return np.full(40 * 256, 0.25)
    if name == "zeros":
        return np.zeros(40 * 256)
    if name == "quiet_on_dc":
        return _quiet_on_dc(48 * 256)
    if name == "breathy":
        return _breathy(40 * 256)
    if name in ("frames0", "frames1", "frames2"):
        return _complex({"frames0": 1536, "frames1": 256 * 8, "frames2": 256 * 9}[name], 48000, 220.0, 8)
    if name.startswith("geom_"):
        sr, hop, _ = GEOMETRIES[name[5:]]
        n = {"hop128": 50, "sr44100": 40, "sr24000": 44, "sr16000": 40, "floor71": 41}[name[5:]] * hop
        return _complex(n, sr, 220.0, 4) + 0.002 * np.random.default_rng(5).standard_normal(n)
    raise KeyError(name)


# every input of the GPU file: name -> geometry
INPUTS = {n: "default" for n in ("tone1500", "tone1500_noise", "silent_stretch", "constant", "zeros", "quiet_on_dc", "breathy", "frames0", "frames1",
                                 "frames2")}
INPUTS.update({"geom_" + k: k for k in GEOMETRIES if k != "default"})
DEFAULT_SINGLES = ("tone1500", "tone1500_noise", "silent_stretch", "constant", "zeros", "quiet_on_dc")
RAGGED = ("frames0", "frames1", "frames2", "breathy", "constant", "silent_stretch")    # 0, 1, 2, 33, 33 (constant), 50 frames


@functools.lru_cache(maxsize=None)
def signal(name):
    w = _fp16(_make(name))
    w.setflags(write=False)
    return w


def time_step(geom):
    sr, hop, _ = GEOMETRIES[geom]
    return hop / sr * 1000 / 1000


@functools.lru_cache(maxsize=None)
def tables(geom):
    """the window and its normalised autocorrelation the device is handed (float64, host copies), and the device-side geometry"""
    sr, hop, floor = GEOMETRIES[geom]
    g = FT.geometry(sr, time_step(geom), floor, CEILING)
    w, wr = FT._window_tables(g, "cpu")
    return g, w.numpy(), wr.numpy()


def r_bound(geom):
    """|dR[k]| <= 2 * nsamp_window * 2^-53 / window_r[k], k = 0 .. nlag (see the module docstring)"""
    g, _, wr = tables(geom)
    return 2.0 * g["nsamp_window"] * 2.0 ** -53 / wr


# ---- the workspace of ss_f0track, by the layout documented at ss_f0track_workspace_bytes -------------------------------------------------

def workspace_layout(B, max_frames, nlag):
    """[(region, byte offset, dtype, shape)], contiguous and in this order, and the total size in bytes"""
    rows = B * max_frames
    regions = [("gpeak", np.float64, (B,)), ("R", np.float64, (rows, nlag + 1)), ("intensity", np.float64, (rows,)),
               ("cand_f", np.float64, (rows, MAXC)), ("cand_s", np.float64, (rows, MAXC)), ("cand_i", np.int32, (rows, MAXC)),
               ("n_cand", np.int32, (rows,)), ("psi", np.uint8, (rows, MAXC))]
    out, off = [], 0
    for name, dt, shape in regions:
        out.append((name, off, dt, shape))
        off += int(np.prod(shape)) * np.dtype(dt).itemsize
    return out, off


def decode_workspace(raw, B, max_frames, nlag):
    """raw: the workspace as a uint8 numpy array -> {region: array [B, max_frames, ...]} (gpeak: [B])"""
    layout, total = workspace_layout(B, max_frames, nlag)
    assert raw.dtype == np.uint8 and raw.size >= total
    out = {}
    for name, off, dt, shape in layout:
        a = raw[off:off + int(np.prod(shape)) * np.dtype(dt).itemsize].view(dt).reshape(shape)
        out[name] = a if name == "gpeak" else a.reshape((B, max_frames) + shape[1:])
    return out


def written_mask(ws, n_frames):
    """{region: bool array} of the entries the kernels are specified to write, for a decoded workspace `ws` and the items' frame counts.
    Left unwritten on purpose: rows of frames i >= n_frames[b], R of silent frames and silent items, candidate slots >= n_cand, psi of frame 0."""
    B, mf = ws["intensity"].shape
    row = np.arange(mf)[None, :] < np.asarray(n_frames)[:, None]
    slot = row[:, :, None] & (np.arange(MAXC)[None, None, :] < np.where(row, ws["n_cand"], 0)[:, :, None])
    psi = slot.copy()
    psi[:, 0, :] = False
    live = row & (np.where(row, ws["intensity"], 0.0) > 0.0)
    return dict(gpeak=np.ones(B, bool), intensity=row, n_cand=row, R=np.broadcast_to(live[:, :, None], ws["R"].shape), cand_f=slot, cand_s=slot,
                cand_i=slot, psi=psi)


# ---- references -------------------------------------------------------------------------------------------------------------------------

def sums_are_exact(x):
    """True if every partial sum of x, in any order, is exact in float64: x on the fp16 grid (multiples of 2^-24) and sum |x| < 2^29"""
    s = np.asarray(x, dtype=np.float64) * 2.0 ** 24
    return bool((s == np.rint(s)).all() and np.abs(s).sum() < 2.0 ** 53)


def _mean(x):
    """mean of float64 samples: the sum in np.longdouble; where that sum is a float64 (always, for `sums_are_exact` inputs) the one rounding
    of float64 sum / n is what an exact-sum implementation gives"""
    s = np.sum(x.astype(np.longdouble))
    return float(s) / len(x) if np.longdouble(float(s)) == s else float(s / len(x))


def stats_reference(name):
    """(gpeak, intensity [n_frames] with the markers 0.0 = silent item / -1.0 = silent frame, windowed frames [n_frames][nsamp_window] float64)"""
    geom = INPUTS[name]
    g, window, _ = tables(geom)
    x = signal(name).astype(np.float64)
    nf, left = FT.frame_grid(g, len(x))
    gpeak = float(np.max(np.abs(x - _mean(x)))) if len(x) else 0.0
    nw, hw, nper, hper = g["nsamp_window"], g["halfnsamp_window"], g["nsamp_period"], g["halfnsamp_period"]
    lo, hi = max(hw + 1 - hper, 1), min(hw + hper, nw)
    intens, frames = np.zeros(nf), np.zeros((nf, nw))
    for i in range(nf):
        right = left + 1 + i * g["hop"]
        frames[i] = (x[right - hw:right - hw + nw] - _mean(x[right - nper:right + nper])) * window
        if gpeak == 0.0:
            continue
        lpeak = float(np.max(np.abs(frames[i, lo - 1:hi])))
        intens[i] = -1.0 if lpeak == 0.0 else (1.0 if lpeak > gpeak else lpeak / gpeak)
    return gpeak, intens, frames


def autocorr_reference(frame, window_r):
    """R[0 .. nlag] of one windowed frame by direct summation in np.longdouble (not the FFT), as np.longdouble"""
    f = frame.astype(np.longdouble)
    nlag = len(window_r) - 1
    a = np.array([np.dot(f[:len(f) - k], f[k:]) for k in range(nlag + 1)], dtype=np.longdouble)
    r = a / (a[0] * window_r.astype(np.longdouble))
    r[0] = 1.0
    return r


@functools.lru_cache(maxsize=None)
def restatement(name):
    """oracle/praat_pitch.py on the input, once: dict(g, frames, intens, r, lags, f0, places) - None for an item shorter than the window"""
    sr, hop, floor = GEOMETRIES[INPUTS[name]]
    x = signal(name).astype(np.float64)
    try:
        g, frames, intens, r, lags = P.analyse_frames(x, sr, time_step(INPUTS[name]), floor, CEILING, VOICING_THRESHOLD, with_lags=True)
    except ValueError as e:
        assert "shorter than the analysis window" in str(e)
        return None
    f0, delta, psi, places = P.path_finder(frames, intens, g, VOICING_THRESHOLD, with_nodes=True)
    return dict(g=g, frames=frames, intens=intens, r=r, lags=lags, f0=f0, places=places)


def perturbation_trials(name, trials=TRIALS):
    """The restatement's candidates and path re-run `trials` times on its OWN r plus uniform noise of the R bound (seeded).
    -> dict(df, ds: largest change of a candidate's frequency (Hz) / strength; stable: candidate count, lags and selected candidate per frame
    unchanged in every trial; frames: how many frames had candidates to perturb)"""
    ref = restatement(name)
    if ref is None:
        return dict(df=0.0, ds=0.0, stable=True, frames=0)
    g = ref["g"]
    bound = r_bound(INPUTS[name])
    df = ds = 0.0
    stable, live = True, [i for i, (fs, _) in enumerate(ref["frames"]) if ref["r"][i].any()]
    for seed in range(trials):
        rng = np.random.default_rng(seed)
        frames = list(ref["frames"])
        for i in live:
            r = ref["r"][i] + rng.uniform(-1.0, 1.0, len(bound)) * bound
            r[0] = 1.0
            f, s, k = P.frame_candidates(r, g, VOICING_THRESHOLD, with_lags=True)
            f0s, s0s = ref["frames"][i]
            if [0] + k != ref["lags"][i]:
                stable = False
                continue
            df = max([df] + [abs(a - b) for a, b in zip(f, f0s[1:])])
            ds = max([ds] + [abs(a - b) for a, b in zip(s, s0s[1:])])
            frames[i] = ([0.0] + f, [0.0] + s)
        if stable:
            _, _, _, places = P.path_finder(frames, ref["intens"], g, VOICING_THRESHOLD, with_nodes=True)
            stable = bool((places == ref["places"]).all())
    return dict(df=df, ds=ds, stable=stable, frames=len(live))


# SPREAD[name] = (Hz, strength): `perturbation_trials(name)` at TRIALS = 8, rounded UP to two significant digits. Recomputed and checked by
# tests/test_f0track_stages_cpu.py (constants must not be below the measurement). Inputs without a live frame have no spread.
SPREAD = {
    "tone1500": (1.4e-09, 6.9e-13),
    "tone1500_noise": (1.4e-08, 6.9e-13),
    "silent_stretch": (4.0e-08, 8.6e-13),
    "quiet_on_dc": (4.6e-06, 8.4e-13),
    "breathy": (4.9e-08, 1.2e-12),
    "frames1": (1.7e-09, 5.5e-13),
    "frames2": (1.7e-09, 6.7e-13),
    "geom_hop128": (1.2e-08, 9.4e-13),
    "geom_sr44100": (7.2e-09, 6.6e-13),
    "geom_sr24000": (1.8e-08, 3.6e-13),
    "geom_sr16000": (7.2e-09, 2.8e-13),
    "geom_floor71": (8.7e-09, 1.3e-12),
}


def round_up_2(v):
    if v <= 0.0:
        return 0.0
    e = math.floor(math.log10(v)) - 1
    return math.ceil(v / 10.0 ** e) * 10.0 ** e


def candidate_bars(name):
    """(Hz, strength) bars of the device's refined candidates for this input"""
    df, ds = SPREAD[name]
    return GPU_MARGIN * df, GPU_MARGIN * ds


def contour_bar(name, f_hz):
    """end-to-end bar of a frame whose reference frequency is f_hz: the candidate bar plus half an fp32 ulp of the frequency"""
    return candidate_bars(name)[0] + 0.5 * float(np.spacing(np.float32(f_hz)))
