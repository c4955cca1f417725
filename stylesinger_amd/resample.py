"""Sample-rate conversion of the reference audio on the GPU: `librosa.core.load(wav_path, sr=audio_sample_rate)` (utils/audios/__init__.py:52)
resamples a file of another rate with resampy's `kaiser_best` filter. librosa and resampy are UN-VENDORED dependencies of the reference, so this
file restates the package's published algorithm (Smith's band-limited interpolation over a tabulated Kaiser-windowed sinc) - parity with
`librosa.load` is UNPINNED: there is no golden of the real packages to check against, and the filter constants below are quoted from resampy's
documentation. What IS pinned: the bank builder against an independent float64 statement of the same definition (tests/resample_ref.py), that
statement against analytically resampled tones (<= 2e-6 in band), and the kernel against it within the fp32 forward bound.

Definition (float64 on the host):
  table   num_zeros = 64 zero crossings, 2^9 = 512 samples per crossing: win[k] = kaiser(2n + 1, beta)[n + k] * rolloff * sinc(rolloff * k / 512),
          k = 0 .. n = 512 * 64 (one wing, 32769 entries), multiplied by ratio = sr_out / sr_in when that is < 1; delta[k] = win[k + 1] - win[k].
  output t sits at input position t * down / up = n + p / up (up / down = the reduced ratio; exact integers, where the package accumulates a float).
          With scale = min(1, ratio), step = int(scale * 512), fr = p / up:
            left wing,  input n - i:      idx = scale * fr * 512,           off = int(idx), eta = idx - off, w = win[off + i step] + eta delta[off + i step]
            right wing, input n + 1 + k:  idx = (scale - scale * fr) * 512, the same
          while i (k) < (32769 - off) // step; inputs outside the signal contribute nothing.
  length  librosa 0.8: n_out = ceil(n_in * sr_out / sr_in); the outputs t < floor(n_in * sr_out / sr_in) are computed, a possible last one is the
          zero `fix_length` appends. Equal rates return the input untouched (librosa short-circuits too; the filter is not an identity).
The weights depend on t only through the phase p: `polyphase_bank` tabulates them per phase ([up, taps], rounded once to fp32) and the device
kernel `ss_resample_poly` (csrc/resample.hip) is the banked sum."""
import functools
import math

import numpy as np
import torch

from . import lib as L

NUM_ZEROS = 64
PRECISION = 9
NUM_TABLE = 1 << PRECISION
ROLLOFF = 0.9475937167399596
KAISER_BETA = 14.769656459379492
MAX_UP = 4096


@functools.lru_cache(maxsize=None)
def _half_window():
    n = NUM_TABLE * NUM_ZEROS
    win = np.kaiser(2 * n + 1, KAISER_BETA)[n:] * ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, n + 1))
    win.setflags(write=False)
    return win


def _ratio(sr_in, sr_out):
    sr_in, sr_out = int(sr_in), int(sr_out)
    if sr_in <= 0 or sr_out <= 0:
        raise ValueError(f"resample: sample rates must be positive (got {sr_in} -> {sr_out} Hz)")
    g = math.gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_len(n_in, sr_in, sr_out):
    """Length of `librosa.resample(y[:n_in], sr_in, sr_out)` (0.8: ceil, integers here)."""
    up, down = _ratio(sr_in, sr_out)
    return -((-int(n_in) * up) // down)


def computed_len(n_in, sr_in, sr_out):
    """How many of the `out_len` samples the interpolation produces (floor); one beyond it is `fix_length`'s zero."""
    up, down = _ratio(sr_in, sr_out)
    return int(n_in) * up // down


@functools.lru_cache(maxsize=32)
def polyphase_bank_f64(sr_in, sr_out):
    up, down = _ratio(sr_in, sr_out)
    if up > MAX_UP:
        raise ValueError(f"resample {sr_in} -> {sr_out} Hz: the reduced ratio {up}/{down} needs {up} filter phases, more than {MAX_UP} "
                         f"(every standard rate to 48 kHz needs at most 640)")
    win = _half_window()
    ratio = up / down
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    nwin = len(win)
    scale = min(1.0, ratio)
    step = int(scale * NUM_TABLE)
    wings = []
    for p in range(up):
        fr = p / up
        pair = []
        for idx in (scale * fr * NUM_TABLE, (scale - scale * fr) * NUM_TABLE):
            off = int(idx)
            eta = idx - off
            k = off + step * np.arange((nwin - off) // step)
            pair.append(win[k] + eta * delta[k])
        wings.append(pair)
    left = max(len(lw) for lw, _ in wings) - 1       # the left wing starts AT input n (i = 0)
    right = max(len(rw) for _, rw in wings)
    taps = left + 1 + right
    bank = np.zeros((up, taps), dtype=np.float64)
    for p, (lw, rw) in enumerate(wings):
        bank[p, left - np.arange(len(lw))] = lw
        bank[p, left + 1 + np.arange(len(rw))] = rw
    bank.setflags(write=False)
    return bank, up, down, taps, left


@functools.lru_cache(maxsize=32)
def polyphase_bank(sr_in, sr_out):
    """-> (bank float32 [up, taps], up, down, taps, left): row p = the weights of phase p for the inputs n - left ... n - left + taps - 1, zero
    where a wing has ended, computed in float64 and rounded once. Cached per rate pair. ValueError when the reduced ratio needs > 4096 phases."""
    bank, up, down, taps, left = polyphase_bank_f64(int(sr_in), int(sr_out))
    b32 = bank.astype(np.float32)
    b32.setflags(write=False)
    return b32, up, down, taps, left


_dev_cache = {}


def _cached(key, make, limit=64):
    """Small device-side tables that repeat from call to call (the bank of a rate pair, the length vectors of a batch): uploaded once, so that a
    repeated call issues no host-to-device copy and can be captured into a hipGraph after one eager call."""
    hit = _dev_cache.get(key)
    if hit is None:
        while len(_dev_cache) >= limit:
            _dev_cache.pop(next(iter(_dev_cache)))
        hit = _dev_cache[key] = make()
    return hit


@torch.no_grad()
def resample_batch(wavs, lens, sr_in, sr_out):
    """wavs [B, L] fp32 on the device, lens host ints (samples of the buffer past lens[b] are padding, whatever they hold) -> ([B, max n_out] fp32
    on the device, zero beyond each item's length; the lengths `out_len(lens[b])` as host ints). Equal rates return the arguments untouched."""
    sr_in, sr_out = int(sr_in), int(sr_out)
    lens = [int(v) for v in lens]
    if sr_in == sr_out:
        return wavs, lens
    if not torch.is_tensor(wavs) or wavs.device.type != "cuda":
        raise L.StyleSingerHipError("resample_batch needs device tensors: there is no CPU path")
    bank, up, down, taps, left = polyphase_bank(sr_in, sr_out)
    if wavs.dim() != 2 or len(lens) != wavs.shape[0]:
        raise ValueError(f"resample_batch: wavs must be [B, L] with one length per row (got {tuple(wavs.shape)}, {len(lens)} lengths)")
    x = wavs if wavs.dtype == torch.float32 and wavs.stride(1) == 1 and wavs.stride(0) >= wavs.shape[1] else wavs.float().contiguous()
    B, Lx = x.shape
    if min(lens) < 0 or max(lens) > Lx:
        raise ValueError(f"resample_batch: lengths {lens} outside the buffer of {Lx} samples")
    n_out = [out_len(n, sr_in, sr_out) for n in lens]
    n_cmp = [computed_len(n, sr_in, sr_out) for n in lens]
    Ly = max(1, max(n_out))
    if Ly >= 2 ** 31:
        raise ValueError("resample_batch: output longer than 2^31 samples")
    dev = x.device
    bank_d = _cached(("bank", sr_in, sr_out, dev), lambda: torch.from_numpy(bank.copy()).to(dev))
    meta = _cached(("lens", sr_in, sr_out, dev, tuple(lens)), lambda: torch.tensor([lens, n_cmp, n_out], dtype=torch.int32).to(dev))
    y = torch.empty(B, Ly, device=dev, dtype=torch.float32)
    L.ops.ss_resample_poly(x, x.stride(0), Lx, meta[0], y, Ly, Ly, meta[1], meta[2], B, bank_d, up, down, taps, left)
    return y, n_out
