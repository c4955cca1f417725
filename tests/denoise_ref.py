"""The yardstick of the vocoder output denoise (`ss_wav_denoise`, stylesinger_amd/denoise.py): a float64 numpy statement of the algorithm, written
from its definition - librosa 0.8 `stft(center=True, pad_mode='constant')`, spectral subtraction, `istft(center=True, length=None)` - with
literal loops over the frames. Parity with librosa itself is UNPINNED (the package is un-vendored); tests/test_denoise_cpu.py holds this file
against torch's float64 stft / istft.

  frames    F = 1 + n // H; frame i = samples i H - N/2 ... i H + N/2 - 1 of the item, zeros outside [0, n)
  window    periodic Hann, w[k] = 0.5 - 0.5 cos(2 pi k / N)
  forward   X = rfft(w * frame)
  subtract  m = |X|; Y = X * (m - v) / m where m > v, else 0
  inverse   t = w * irfft(Y)   (irfft ignores the imaginary parts of bins 0 and N/2)
  add       frame i at offset i H of a signal of N + H (F - 1) samples, divided by the envelope sum w^2 (laid out the same way) wherever that exceeds
            float32 tiny, undivided elsewhere; N/2 samples cut from each end -> H (n // H) samples."""
import numpy as np

TINY = float(np.finfo(np.float32).tiny)


def hann(N):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N, dtype=np.float64) / N)


def envelope(n, N, H):
    """sum of w^2 over the frames, as long as the overlap-added signal: N + H (F - 1) float64 values"""
    F = 1 + n // H
    w2 = hann(N) ** 2
    env = np.zeros(N + H * (F - 1))
    for i in range(F):
        env[i * H:i * H + N] += w2
    return env


def denoise_ref(x, N, H, v):
    """x: 1-D array (the item's own samples, nothing else) -> float64 array of H (len(x) // H) samples."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    F = 1 + n // H
    w = hann(N)
    xp = np.concatenate([np.zeros(N // 2), x, np.zeros(N)])   # (the tail zeros cover the last frame)
    out = np.zeros(N + H * (F - 1))
    for i in range(F):
        X = np.fft.rfft(w * xp[i * H:i * H + N])
        m = np.abs(X)
        s = np.zeros_like(m)
        keep = m > v
        s[keep] = (m[keep] - v) / m[keep]
        out[i * H:i * H + N] += w * np.fft.irfft(X * s, N)
    env = envelope(n, N, H)
    big = env > TINY
    out[big] /= env[big]
    return out[N // 2:N // 2 + H * (n // H)]


def zero_envelope(n, N, H):
    """bool [H (n // H)]: the output samples whose envelope does not exceed float32 tiny (they are left undivided: with H = N every N-th one)"""
    return ~(envelope(n, N, H) > TINY)[N // 2:N // 2 + H * (n // H)]


def sine_noise(n, seed, sr=48000, f=440.0, amp=0.6, sigma=0.05):
    """a sine plus white noise, clipped to |x| <= 1, float32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = amp * np.sin(2 * np.pi * f * t + 0.7) + sigma * rng.standard_normal(n)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def denoise_f32_emulation(x, N, H, v):
    """The same steps with every array held in float32 and torch's fp32 FFT, frame by frame: what an fp32 transform can reach at a geometry. It is
    what decides that hop_size == fft_size runs in float64 on the device (tests/test_denoise_cpu.py holds the figures)."""
    import torch
    xt = torch.from_numpy(np.asarray(x, dtype=np.float32))
    n = len(xt)
    F = 1 + n // H
    w = torch.from_numpy(hann(N).astype(np.float32))
    xp = torch.cat([torch.zeros(N // 2), xt, torch.zeros(N)])
    out = torch.zeros(N + H * (F - 1))
    for i in range(F):
        X = torch.fft.fft((w * xp[i * H:i * H + N]).to(torch.complex64))
        m = X.abs()
        s = torch.where(m > v, (m - v) / m.clamp(min=1e-30), torch.zeros_like(m))
        out[i * H:i * H + N] += w * torch.fft.ifft(X * s).real
    env = torch.from_numpy(envelope(n, N, H).astype(np.float32))
    big = env > TINY
    out[big] /= env[big]
    return out[N // 2:N // 2 + H * (n // H)].numpy()
