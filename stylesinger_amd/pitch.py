"""Reference-f0 conditioning: mirror of `utils/pitch_utils.py:34-62` (`norm_f0`, `norm_interp_f0`).

`inference/StyleSinger.py:152` feeds the tracker's contour (Hz, 0 = unvoiced) through `norm_interp_f0` before the model sees
it: log2(f0 + 1e-8) (`pitch_norm: log`), unvoiced frames replaced by a linear interpolation between their voiced neighbours
(`np.interp`: held flat beyond the first / last voiced frame), all-unvoiced contours become 0.

Two forms with the same contract:
  * `norm_interp_f0(f0, hparams)`      host numpy, what `StyleSingerInfer.input_to_batch` calls for one utterance;
  * `norm_interp_f0_device(f0, lens)`  `[B, T]` on the GPU (`ss_norm_interp_f0`), what `preprocess_batch` uses so a batch
                                       goes from tracker output to `infer_batch` without a host round trip.

Pitch control (`StyleSingerHIP.forward(pitch_hz=...)`): a caller's contour in Hz lives on a frame grid of its own, the score's frame count is only
known inside forward. `contour_fit` is the float64 definition of the fit between the two grids, `contour_fit_device` the kernel (`ss_contour_fit`,
csrc/pitch_fit.hip) that runs it from device lengths.
"""
import numpy as np
import torch

from . import lib as L


def norm_f0(f0, uv, hparams):
    """utils/pitch_utils.py:34-45 for numpy input. Returns a new array."""
    f0 = np.array(f0, copy=True)
    if hparams.get("pitch_norm", "log") == "standard":
        f0 = (f0 - hparams.get("f0_mean", 400)) / hparams.get("f0_std", 100)
    if hparams.get("pitch_norm", "log") == "log":
        f0 = np.log2(f0 + 1e-8)
    if uv is not None and hparams.get("use_uv", True):
        f0[uv > 0] = 0
    return f0


def norm_interp_f0(f0, hparams):
    """utils/pitch_utils.py:47-62: f0 [T] in Hz (numpy or torch, any float dtype; the arithmetic runs in the input's dtype
    as numpy does there) -> (f0 [T] float32 tensor, uv [T] float32 tensor)."""
    is_torch = isinstance(f0, torch.Tensor)
    device = f0.device if is_torch else None
    x = f0.detach().cpu().numpy() if is_torch else np.asarray(f0)
    uv = x == 0
    y = norm_f0(x, uv, hparams)
    n_uv = int(uv.sum())
    if n_uv == len(y):
        y[uv] = 0
    elif n_uv > 0:
        y[uv] = np.interp(np.where(uv)[0], np.where(~uv)[0], y[~uv])
    f0_t = torch.from_numpy(np.asarray(y, dtype=np.float32))
    uv_t = torch.from_numpy(uv.astype(np.float32))
    if is_torch:
        f0_t, uv_t = f0_t.to(device), uv_t.to(device)
    return f0_t, uv_t


@torch.no_grad()
def norm_interp_f0_device(f0_hz, lens=None, hparams=None):
    """f0_hz fp32 [B, T] on the device (0 = unvoiced), lens int32 [B] valid frames per item (default T) ->
    (f0 [B, T], uv [B, T]) fp32: per item `norm_interp_f0` of its first lens[b] frames; frames >= lens[b] are 0. Contract: the entry takes
    FP32 Hz, i.e. what numpy computes on a float32 contour (log2 and the interpolation weights in double, the interpolation endpoints rounded to
    fp32 first); against the reference's float64 tracker output that is within 1 fp32 ulp of values in [6, 10] (tests allow 2e-6), not
    bit-identical to the host path `norm_interp_f0` of this module, which `input_to_batch` uses on the float64 contour."""
    hp = hparams or {}
    if hp.get("pitch_norm", "log") != "log" or not hp.get("use_uv", True):
        raise NotImplementedError("norm_interp_f0_device: only pitch_norm='log' with use_uv (the reference's setting)")
    if f0_hz.device.type != "cuda":
        raise L.StyleSingerHipError("norm_interp_f0_device needs device tensors: there is no CPU path")
    x = f0_hz.float().contiguous()
    B, T = x.shape
    out = torch.empty_like(x)
    uv = torch.empty_like(x)
    lp = None if lens is None else lens.to(device=x.device, dtype=torch.int32).contiguous()
    L.check(L.load().ss_norm_interp_f0(L.ptr(x), L.ptr(lp), L.ptr(out), L.ptr(uv), B, T, L.stream_ptr()), "ss_norm_interp_f0")
    return out, uv


def contour_fit(f0_hz, n_t, shift=0.0):
    """The definition of the contour fit (float64): f0_hz [n_c] in Hz (0 = unvoiced) -> [n_t] in Hz on a grid of n_t frames over the same time span.
    Output frame t sits at source position s = (t + 0.5) * n_c / n_t - 0.5, clamped to [0, n_c - 1] (the frame centres of both grids on one time
    axis); s is held as the exact fraction num / (2 n_t). With i0 = floor(s), fr = s - i0, i1 = min(i0 + 1, n_c - 1):
      * the frame is voiced iff the NEAREST source frame is voiced (fr >= 1/2 -> i1: a tie goes to the later frame), else 0;
      * its value is exp2((1 - fr) log2 f[i0] + fr log2 f[i1]) when both neighbours are voiced, otherwise the nearest frame's value (then the only
        voiced neighbour), times 2^(shift / 12) (shift in semitones);
      * fr == 0 takes f[i0] itself, so with shift == 0 equal lengths return the contour unchanged, bit for bit."""
    f = np.asarray(f0_hz, dtype=np.float64)
    n_c, n_t = len(f), int(n_t)
    out = np.zeros(n_t, dtype=np.float64)
    if n_c == 0 or n_t == 0:
        return out
    t = np.arange(n_t, dtype=np.int64)
    den = 2 * n_t
    num = np.clip((2 * t + 1) * n_c - n_t, 0, (n_c - 1) * den)
    i0, rem = num // den, num % den
    i1 = np.minimum(i0 + 1, n_c - 1)
    a, c = f[i0], f[i1]
    near = np.where(2 * rem >= den, c, a)
    fr = rem / den
    both = (a > 0) & (c > 0) & (rem != 0)
    with np.errstate(divide="ignore"):
        la, lc = np.log2(np.where(both, a, 1.0)), np.log2(np.where(both, c, 1.0))
    val = np.where(both, np.exp2(la + fr * (lc - la)), near)
    voiced = near > 0
    out[voiced] = val[voiced] * (2.0 ** (float(shift) / 12.0) if shift else 1.0)
    return out


@torch.no_grad()
def contour_fit_device(f0_hz, lens_c, lens_t, T, shift=0.0):
    """f0_hz fp32 [B, Lc] on the device (Hz, 0 = unvoiced), lens_c [B] valid source frames (host ints or a device tensor; None = Lc), lens_t int32 [B] ON THE
    DEVICE (target frames per item: no host sync) -> [B, T] fp32: `contour_fit` of each item's first lens_c[b] frames to lens_t[b] frames, 0 beyond."""
    if not torch.is_tensor(f0_hz) or f0_hz.device.type != "cuda":
        raise L.StyleSingerHipError("contour_fit_device needs device tensors: there is no CPU path")
    x = f0_hz if f0_hz.dtype == torch.float32 and f0_hz.stride(1) == 1 and f0_hz.stride(0) >= f0_hz.shape[1] else f0_hz.float().contiguous()
    B, Lc = x.shape
    dev = x.device
    lc = torch.full((B,), Lc, dtype=torch.int32) if lens_c is None else torch.as_tensor(lens_c)
    lc = lc.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    lt = lens_t.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if lc.numel() != B or lt.numel() != B:
        raise ValueError(f"contour_fit_device: {lc.numel()} source lengths and {lt.numel()} target lengths for {B} contours")
    out = torch.empty(B, int(T), device=dev, dtype=torch.float32)
    L.check(L.load().ss_contour_fit(L.ptr(x), x.stride(0), Lc, L.ptr(lc), L.ptr(lt), float(shift), L.ptr(out), out.stride(0), int(T), B,
                                    L.stream_ptr()), "ss_contour_fit")
    return out
