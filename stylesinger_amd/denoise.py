"""Vocoder output denoise on the GPU: the last step of the reference's vocoder plugin (tasks/tts/vocoder_infer/hifigan_nsf.py:14-22, 73-74),
    if hparams.get('vocoder_denoise_c', 0.0) > 0: wav_out = denoise(wav_out, v=hparams['vocoder_denoise_c'])
    denoise: spec = librosa.stft(wav, n_fft=fft_size, hop_length=hop_size, win_length=win_size, pad_mode='constant')
             librosa.istft(clip(|spec| - v, 0) * exp(1j * angle(spec)), hop_length=hop_size, win_length=win_size)
- a spectral subtraction that takes the generator's constant hiss out of rests and note tails. librosa is an UN-VENDORED dependency of the
reference, so this file restates the published algorithm of librosa 0.8 - parity with librosa is UNPINNED: there is no golden of the real package
to check against. What IS pinned: an independent float64 statement (tests/denoise_ref.py) against torch's float64 stft / istft to 1e-12, and the
kernel against that statement within the project's fp32 waveform bar (1e-5).

Definition (N = fft_size = win_size, H = hop_size, an item of n samples):
  frames    F = 1 + n // H; frame i = samples i H - N/2 ... i H + N/2 - 1, zeros outside [0, n)           (center=True, pad_mode='constant')
  window    periodic Hann, w[k] = 0.5 - 0.5 cos(2 pi k / N)
  subtract  X = rfft(w frame); m = |X|; Y = X (m - v) / m where m > v, else 0 - the reference's clip(m - v, 0) exp(j angle(X)) without the atan2
  inverse   t = w irfft(Y); frame i added at offset i H of a signal of N + H (F - 1) samples; divided by the envelope sum w^2 wherever that exceeds
            float32 tiny; N/2 samples cut from each end
  length    H (n // H)
`ss_wav_denoise` (csrc/denoise.hip) is the device form: one launch, the transform in LDS, the overlap-add in a fixed order. fp32, except with
hop_size == fft_size: there the envelope w^2 falls to 0 at every frame edge, the division amplifies rounding by 1 / w, and the kernel runs in float64."""
import numpy as np
import torch

from . import lib as L
from .resample import _cached

N_MIN, N_MAX, H_MIN = 256, 2048, 64
GEOMETRY_DEFAULTS = dict(fft_size=1024, win_size=1024, hop_size=256)   # egs/egs_bases/tts/base.yaml; the mel front end's defaults


def check_geometry(n_fft, hop, win):
    """The geometries `ss_wav_denoise` computes (pure: no device). Raises StyleSingerHipError naming the offending hparams key."""
    def bad(key, val, why):
        raise L.StyleSingerHipError(f"vocoder_denoise_c: {key}={val!r} is not supported: {why}")

    def is_int(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not is_int(n_fft) or not N_MIN <= n_fft <= N_MAX or n_fft & (n_fft - 1):
        bad("fft_size", n_fft, f"a power of two in [{N_MIN}, {N_MAX}]")
    if not is_int(win) or win != n_fft:
        bad("win_size", win, f"must equal fft_size ({n_fft})")
    if not is_int(hop) or not H_MIN <= hop <= n_fft or n_fft % hop:
        bad("hop_size", hop, f"a divisor of fft_size ({n_fft}), at least {H_MIN}")
    return int(n_fft), int(hop)


def resolve_denoise(hparams):
    """-> v (float > 0) when the output is to be denoised, None for a missing key or a value <= 0 (the reference's default 0.0: nothing changes).
    With v > 0 the geometry keys are validated here, before a device is touched."""
    v = (hparams or {}).get("vocoder_denoise_c", 0.0)
    if v is None or float(v) <= 0:
        return None
    if not np.isfinite(float(v)):
        raise L.StyleSingerHipError(f"vocoder_denoise_c={v!r} is not supported: must be finite")
    geometry(hparams)
    return float(v)


def geometry(hparams):
    """(fft_size, hop_size) of the hparams, validated (`check_geometry`)."""
    g = {k: (hparams or {}).get(k, d) for k, d in GEOMETRY_DEFAULTS.items()}
    return check_geometry(g["fft_size"], g["hop_size"], g["win_size"])


def table_f64(n_fft):
    """3 N float64: N complex twiddles by butterfly span, [2 (s + j)], [2 (s + j) + 1] = cos, -sin of 2 pi j / (2 s) (W_{2s}^j) for s = 1, 2, 4,
    ..., N / 2 and j < s (entry 0 is unused), then the periodic Hann window w[0 .. N)."""
    t = np.zeros(3 * n_fft, dtype=np.float64)
    s = 1
    while s < n_fft:
        j = np.arange(s, dtype=np.float64)
        t[2 * s:4 * s:2] = np.cos(2.0 * np.pi * j / (2 * s))
        t[2 * s + 1:4 * s:2] = -np.sin(2.0 * np.pi * j / (2 * s))
        s *= 2
    t[2 * n_fft:] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft)
    return t


def device_table(n_fft, device):
    """The table `ss_wav_denoise` reads: `table_f64` followed by the same values rounded once to float32; uploaded once per (device, N)."""
    def make():
        t = table_f64(n_fft)
        raw = np.frombuffer(t.tobytes() + t.astype(np.float32).tobytes(), dtype=np.uint8).copy()
        return torch.from_numpy(raw).to(device)
    return _cached(("denoise_table", int(n_fft), device), make)


@torch.no_grad()
def denoise_batch(wav, lens_samples, n_fft, hop, win, v):
    """wav [B, L] fp32 on the device; lens_samples: int32 [B] on the device, host ints, or None (whole rows) - samples of a row at or beyond its
    length count as zero, whatever the row holds -> (wav_out [B, hop (L // hop)] fp32, zero beyond each item's n_out; n_out int32 [B] on the device
    = hop (lens // hop)). v >= 0 (v = 0 is the identity up to rounding). No host synchronisation, no CPU path."""
    n_fft, hop = check_geometry(n_fft, hop, win)
    v = float(v)
    if not (np.isfinite(v) and v >= 0):
        raise ValueError(f"denoise_batch: v must be finite and >= 0 (got {v})")
    if not torch.is_tensor(wav) or wav.device.type != "cuda":
        raise L.StyleSingerHipError("denoise_batch needs device tensors: there is no CPU path")
    if wav.dim() != 2 or wav.shape[1] < 1:
        raise ValueError(f"denoise_batch: wav must be [B, L] (got {tuple(wav.shape)})")
    x = wav if wav.dtype == torch.float32 and wav.stride(1) == 1 and wav.stride(0) >= wav.shape[1] else wav.float().contiguous()
    B, Lx = x.shape
    dev = x.device
    if lens_samples is None:
        lens_samples = [Lx] * B
    if torch.is_tensor(lens_samples):
        n = lens_samples if lens_samples.dtype == torch.int32 and lens_samples.is_contiguous() else lens_samples.to(torch.int32).contiguous()
        if n.device != dev or n.numel() != B:
            raise ValueError("denoise_batch: lens_samples must be one device value per row")
    else:
        lens = [int(t) for t in lens_samples]
        if len(lens) != B or min(lens) < 0 or max(lens) > Lx:
            raise ValueError(f"denoise_batch: lengths {lens} do not fit {B} rows of {Lx} samples")
        n = _cached(("denoise_lens", dev, tuple(lens)), lambda: torch.tensor(lens, dtype=torch.int32).to(dev))
    Ly = max(1, Lx // hop * hop)
    lib = L.load()
    ws_bytes = lib.ss_wav_denoise_workspace_bytes(B, Lx, n_fft, hop)
    if ws_bytes < 0:
        raise L.StyleSingerHipError(f"ss_wav_denoise_workspace_bytes refused B={B} Lx={Lx} fft_size={n_fft} hop_size={hop}")
    ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8) if ws_bytes else None
    y = torch.empty(B, Ly, device=dev, dtype=torch.float32)
    n_out = torch.empty(B, device=dev, dtype=torch.int32)
    table = L.ptr(device_table(n_fft, dev))   # a byte buffer (float64 table, then its float32 copy) behind the `const double*`: by address, the cache owns it
    L.ops.ss_wav_denoise(x, x.stride(0), Lx, n, y, Ly, Ly, n_out, B, n_fft, hop, v, table, ws, ws_bytes)
    return (y if Lx >= hop else y[:, :0]), n_out
