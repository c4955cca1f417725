"""Look-ahead true-peak limiter of the output on the GPU (hparams['out_true_peak_db'], `infer_batch(out_true_peak_db=)`, `--out-true-peak DB`): the
last stage of the output chain - vocoder, `vocoder_denoise_c`, the loudness target, THIS, the PCM16 writer or the stitched song. The reference has
no such stage: with a loudness target it divides a whole item by its peak wherever `gain * peak > 1` (the "peak rule" of `loudness.py`), so an item
whose crest factor does not fit under the target silently misses it; with the limiter on, the loudness gain is applied in full and only the peaks
are turned down. An explicit opt-in: with `out_true_peak_db=None` nothing here runs.

NOT CLAIMED: conformance with a standard true-peak meter. The BS.1770 Annex 2 coefficient table is not available to this project, so the
inter-sample estimate below is the project's own, on the 4x interpolator it already has (`resample.polyphase_bank_f64(sr, 4 sr)`: the ratio reduces
to 4/1 at every rate, so there is one bank of 4 x 127 weights; no new filter constants). The constants (2 ms, the window shape) are unassessed on
recordings. Attack and release are symmetric (one window); longer release curves, multiband, stereo linking and oversampled output are out of
scope, and so is correcting the loudness the limiter takes away (measured: DESIGN.md 3.4g2).

Definition (float64 on the host, `limit_f64`), per item x[0 .. n) with a linear pre-gain G (1 without a loudness target; fp32, as
`ss_loudness_measure` writes it), the ceiling c = fl32(10^(ceiling_db / 20)), ceiling_db <= 0, and the window
W = max(1, round(lookahead_ms sr / 1000)) samples (W > LIMIT_MAX_W is refused, never truncated). x' = fl32(G x) - the one fp32 rounding of the
gain, numpy 1.21 semantics as in `loudness.py` - and x' = 0 outside [0, n):
  a. peak envelope   e[t] = max(|x'[t]|, max over p = 0 .. 3 of |sum_k bank[p][k] x'[t + k - left]|). The term |x'[t]| is deliberate: phase 0 of
                     the bank is not an identity (rolloff 0.9476), and the SAMPLE peak must be bounded exactly.
  b. required gain   r[t] = min(1, c / e[t]); 1 where e[t] = 0 and 1 outside [0, n).
  c. look-ahead min  m[t] = min of r over [t, t + W - 1], for every t >= -(W - 1).
  d. smoothing       g[t] = min(r[t], (1 / W) sum over j = t - W + 1 .. t of m[j]). Every m[j] of that sum covers t, so the mean is <= r[t]
                     already in exact arithmetic; the outer min makes that survive rounding. The gain falls over W samples BEFORE a peak
                     and recovers over W samples after it.
  e. output          y[t] = g[t] x'[t] for t < n, exact zeros from n to the buffer's end.
  report             min_gain = min over t of g, n_limited = #{t : g[t] < 1}.
`ss_limit_true_peak` (csrc/limiter.hip) is the device form: fp32, every sum in a fixed order, one workgroup per tile of 1856 samples with the
halo in LDS; LIMIT_MAX_W is what that layout holds."""
import numpy as np
import torch

from . import lib as L
from .resample import _cached, polyphase_bank, polyphase_bank_f64

LIMIT_MAX_W = L.abi.DEFINES["SS_LIMIT_MAX_W"]
DEFAULT_LOOKAHEAD_MS = 2.0


def ceiling_f32(ceiling_db):
    """c = fl32(10^(ceiling_db / 20)); ValueError for a ceiling above 0 dBFS or a non-finite one."""
    db = float(ceiling_db)
    if not np.isfinite(db) or db > 0.0:
        raise ValueError(f"limiter: ceiling_db={ceiling_db!r}: expected a finite level <= 0 dBFS")
    c = np.float32(10.0 ** (db / 20.0))
    if not c > 0:
        raise ValueError(f"limiter: ceiling_db={ceiling_db!r} is below the fp32 range")
    return c


def window_samples(sr, lookahead_ms=DEFAULT_LOOKAHEAD_MS):
    """W = max(1, round(lookahead_ms sr / 1000)); ValueError when it is not finite, negative, or beyond LIMIT_MAX_W (never truncated)."""
    ms, sr = float(lookahead_ms), int(sr)
    if sr <= 0:
        raise ValueError(f"limiter: the sample rate must be positive (got {sr})")
    if not np.isfinite(ms) or ms < 0.0:
        raise ValueError(f"limiter: lookahead_ms={lookahead_ms!r}: expected a finite time >= 0")
    W = max(1, int(round(ms * sr / 1000.0)))
    if W > LIMIT_MAX_W:
        raise ValueError(f"limiter: lookahead_ms={ms} at {sr} Hz is a window of {W} samples, more than LIMIT_MAX_W = {LIMIT_MAX_W} (the tile and "
                         f"its halo live in LDS); at most {LIMIT_MAX_W * 1000.0 / sr:.3f} ms at this rate")
    return W


def bank4_f64(sr):
    """-> (bank float64 [4, taps], taps, left): the project's 4x interpolator at this rate."""
    bank, up, down, taps, left = polyphase_bank_f64(int(sr), 4 * int(sr))
    if (up, down) != (4, 1):
        raise AssertionError("limiter: sr -> 4 sr must reduce to 4 / 1")
    return bank, taps, left


def envelope_f64(xp, sr):
    """Step a for x' (float64 [n]) -> e [n]."""
    bank, taps, left = bank4_f64(sr)
    xp = np.asarray(xp, dtype=np.float64)
    e = np.abs(xp)
    if len(xp):
        pad = np.concatenate([np.zeros(left), xp, np.zeros(taps - 1 - left)])
        for p in range(4):
            e = np.maximum(e, np.abs(np.correlate(pad, bank[p], mode="valid")))
    return e


def limit_f64(x, sr, ceiling_db, lookahead_ms=DEFAULT_LOOKAHEAD_MS, gain=None, W=None):
    """The host definition for one item -> dict(y, g, r, e, m (for t = -(W - 1) .. n - 1) float64, xp = x' (float32), c, W, min_gain, n_limited).
    `W` overrides the window length in samples (the tests' form)."""
    c = ceiling_f32(ceiling_db)
    W = window_samples(sr, lookahead_ms) if W is None else int(W)
    if W < 1 or W > LIMIT_MAX_W:
        raise ValueError(f"limiter: a window of {W} samples outside [1, {LIMIT_MAX_W}]")
    x = np.asarray(x, dtype=np.float32)
    xp = x if gain is None else (np.float32(gain) * x).astype(np.float32)
    n = len(xp)
    e = envelope_f64(xp, sr)
    with np.errstate(divide="ignore"):
        r = np.minimum(1.0, np.float64(c) / e)
    ext = np.concatenate([np.ones(W - 1), r, np.ones(W - 1)])
    win = np.lib.stride_tricks.sliding_window_view
    m = win(ext, W).min(axis=-1) if n else np.ones(W - 1)     # [n + W - 1]: t = -(W - 1) .. n - 1
    g = np.minimum(r, win(m, W).sum(axis=-1) / W) if n else np.ones(0)
    y = g * xp.astype(np.float64)
    return dict(y=y, g=g, r=r, e=e, m=m, xp=xp, c=c, W=W, min_gain=float(g.min()) if n else 1.0, n_limited=int((g < 1.0).sum()))


# ---- device ---------------------------------------------------------------------------------------------------------------------------------
@torch.no_grad()
def limit_batch(wav, lens, sr, ceiling_db, lookahead_ms=DEFAULT_LOOKAHEAD_MS, gain=None, W=None, with_gain_curve=False):
    """wav [B, L] fp32 on the device, lens host ints (samples past lens[b] are padding, whatever they hold), `gain` None or a device fp32 [B] (what
    `loudness.measure_batch` returns as 'gain') -> (y [B, L] fp32, exact zeros past lens[b]; dict(min_gain [B] fp32, n_limited [B] int32) on the
    device). No host sync; after one eager call per (rate, lens) no host-to-device copy: graph-capturable. Bad arguments (ceiling_db > 0 or
    non-finite, a window beyond LIMIT_MAX_W) are refused before a device is touched. `W` overrides the window in samples;
    `with_gain_curve` adds 'g' [B, L] (the gain the kernel applied: g[t] for t < lens[b], 1 after it)."""
    c, W_ = ceiling_f32(ceiling_db), window_samples(sr, lookahead_ms)
    if W is not None:
        W_ = int(W)
        if W_ < 1 or W_ > LIMIT_MAX_W:
            raise ValueError(f"limiter: a window of {W_} samples outside [1, {LIMIT_MAX_W}]")
    if not torch.is_tensor(wav) or wav.device.type != "cuda":
        raise L.StyleSingerHipError("limit_batch needs device tensors: there is no CPU path")
    lens = [int(v) for v in lens]
    if wav.dim() != 2 or len(lens) != wav.shape[0]:
        raise ValueError(f"limit_batch: wav must be [B, L] with one length per row (got {tuple(wav.shape)}, {len(lens)} lengths)")
    x = wav if wav.dtype == torch.float32 and wav.stride(1) == 1 and wav.stride(0) >= wav.shape[1] else wav.float().contiguous()
    B, Lx = x.shape
    if B < 1 or Lx < 1 or B > 65535 or Lx >= 2 ** 31 or min(lens) < 0 or max(lens) > Lx:
        raise ValueError(f"limit_batch: lengths {lens} outside the buffer of {Lx} samples, or an empty / oversized batch")
    dev = x.device
    if gain is not None:
        if not torch.is_tensor(gain) or gain.device != dev or gain.dtype != torch.float32 or gain.shape != (B,) or not gain.is_contiguous():
            raise ValueError("limit_batch: gain must be a contiguous fp32 [B] tensor on the audio's device")
    sr = int(sr)
    bank, _, _, taps, left = polyphase_bank(sr, 4 * sr)
    bank_d = _cached(("bank", sr, 4 * sr, dev), lambda: torch.from_numpy(bank.copy()).to(dev))
    n_d = _cached(("limit_lens", dev, tuple(lens)), lambda: torch.tensor(lens, dtype=torch.int32).to(dev))
    lib = L.load()
    y = torch.empty(B, Lx, device=dev, dtype=torch.float32)
    g = torch.empty(B, Lx, device=dev, dtype=torch.float32) if with_gain_curve else None
    rep = dict(min_gain=torch.empty(B, device=dev, dtype=torch.float32), n_limited=torch.empty(B, device=dev, dtype=torch.int32))
    nbytes = int(lib.ss_limit_workspace_bytes(B, Lx))
    ws = torch.empty(max(1, nbytes // 8), device=dev, dtype=torch.float64)
    L.ops.ss_limit_true_peak(x, x.stride(0), Lx, n_d, gain, bank_d, taps, left, float(c), W_, y, Lx, Lx,
                             rep["min_gain"], rep["n_limited"], g, B, ws, nbytes)
    if g is not None:
        rep["g"] = g
    return y, rep
