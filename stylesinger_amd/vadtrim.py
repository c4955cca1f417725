"""`trim_long_silences` of the emotion branch (data_gen/tts/emotion/audio.py:58-100, called by `preprocess_wav`, :38) around VAD flags, and a
voice-activity decision of this project's own for callers who cannot run the reference's.

The reference asks `webrtcvad.Vad(mode=3).is_speech` for one flag per 30 ms window of the volume-normalised 16-bit PCM. webrtcvad is an un-vendored
C library (a fixed-point GMM over sub-band energies; its model tables are not in the reference tree and there is no published text to restate), so
that DECISION stays the caller's: `flags[b, w] = vad.is_speech(pcm16(window w of item b), 16000)`. Everything around it - cutting the waveform to whole
windows, the moving average of width 8 rounded half to even, the dilation by 6 windows, the compaction of the kept windows - runs on the device
(`ss_vad_trim`) and is pinned bit-exactly against the REAL function run with injected flags (`tests/golden/vad_trim.pt`).

`vad_flags="lrt"` (opt-in; nothing changes for callers who do not ask for it) takes the flags from `ss_vad_lrt` (csrc/vad_lrt.hip) instead, on
the device: a per-window likelihood-ratio test in the maximum-likelihood form of Sohn, Kim & Sung, "A statistical model-based voice activity
detection" (IEEE SPL 6(1), 1999), against a noise spectrum taken offline from the item's own quietest windows (the file is there whole: nothing
needs to be causal). `lrt_statistic` below - not the paper - is the definition; the kernel is checked against it (exact flags, the statistic
within 16 x the float64 spread of the definition itself). Like `loudness="bs1770"` beside pyloudnorm this is NOT the reference's decision: parity
with webrtcvad is neither claimed nor wanted, and the constants are UNASSESSED ON RECORDINGS - they were set on synthetic harmonic tone bursts
with pauses and white noise at -70 to -30 dBFS (noise-only windows 0.05-0.3, voiced windows 6e2-1e5, digital silence 0; at 20 dB SNR the peak rule
flags every window: a recording without pauses, or a noisy one, fails towards "everything is voice" = the opt-out, never towards cutting singing).
"""
import numpy as np
import torch

from . import lib as L

# data_gen/tts/emotion/params_data.py
VAD_WINDOW_MS = 30
VAD_MOVING_AVERAGE_WIDTH = 8
VAD_MAX_SILENCE_LENGTH = 6
SAMPLING_RATE = 16000

# the "lrt" decision (`lrt_statistic`): passed to `ss_vad_lrt` as arguments; not user options
LRT_N_FFT = 512                  # the 480-sample window zero-padded
LRT_K_LO, LRT_K_HI = 3, 127      # bins of the statistic: about 94 Hz to 3.97 kHz at the nominal 16 kHz
LRT_Q_DIV = 10                   # the noise spectrum is the mean over the quietest ceil(nW / 10) windows
LRT_PEAK_DB = 30.0               # ... and at most this far below the loudest window's energy
LRT_N_MIN = 1.0                  # floor of a noise bin (16-bit PCM units squared)
LRT_ETA = 1.0                    # a window is voiced when its statistic exceeds this


def window_mask(flags, avg_width=VAD_MOVING_AVERAGE_WIDTH, max_silence=VAD_MAX_SILENCE_LENGTH):
    """Host mirror (integer logic) of the reference's smoothing + dilation: flags [nW] (0/1) -> kept-window mask [nW] bool."""
    f = np.asarray(flags).astype(np.int64)
    n = len(f)
    lp, rp = (avg_width - 1) // 2, avg_width // 2
    pad = np.concatenate([np.zeros(lp, np.int64), f, np.zeros(rp, np.int64)])
    cnt = np.array([pad[i:i + avg_width].sum() for i in range(n)], dtype=np.int64)
    m1 = 2 * cnt > avg_width                      # np.round(cnt / width): exactly one half rounds to the even 0
    o = (max_silence + 1) // 2                    # binary_dilation(mask, ones(max_silence + 1)): origin at the centre
    out = np.zeros(n, dtype=bool)
    for i in range(n):
        lo, hi = i - max_silence + o, i + o       # j = i - k + o for k = 0 .. max_silence
        out[i] = m1[max(lo, 0):min(hi, n - 1) + 1].any() if hi >= 0 and lo <= n - 1 else False
    return out


def have_webrtcvad():
    try:
        import webrtcvad  # noqa: F401
        return True
    except Exception:
        return False


def webrtc_flags(wavs, lens, sr=SAMPLING_RATE):
    """The reference's own decision loop (data_gen/tts/emotion/audio.py:66-81) on the HOST with the webrtcvad package: per item the waveform cut
    to whole 30 ms windows, `round(wav * 32767)` as 16-bit PCM, `Vad(mode=3).is_speech(window, sample_rate)` per window. wavs [B, L] (device or
    host; the volume-normalised audio), lens host ints -> uint8 [B, max windows] (0 beyond an item's windows). The package is un-vendored: this
    raises ImportError where it is missing (callers then pass flags or opt out explicitly)."""
    import struct
    import webrtcvad
    spw = VAD_WINDOW_MS * sr // 1000
    x = wavs.detach().float().cpu().numpy() if torch.is_tensor(wavs) else np.asarray(wavs, dtype=np.float32)
    ns = [min(int(n), x.shape[1]) for n in lens]
    max_w = max(1, max(n // spw for n in ns))
    out = np.zeros((len(ns), max_w), dtype=np.uint8)
    for b, n in enumerate(ns):
        nw = n // spw
        w = x[b, :nw * spw]
        pcm = struct.pack("%dh" % len(w), *(np.round(w * 32767)).astype(np.int16))
        vad = webrtcvad.Vad(mode=3)
        for i in range(nw):
            out[b, i] = 1 if vad.is_speech(pcm[i * spw * 2:(i + 1) * spw * 2], sample_rate=sr) else 0
    return out


def lrt_window(spw, dtype=np.float64):
    """The periodic Hann window of the "lrt" decision, 0.5 - 0.5 cos(2 pi k / spw)."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(spw, dtype=dtype) / spw)).astype(dtype)


def lrt_power(wav, n, sr=SAMPLING_RATE):
    """First half of `lrt_statistic`: wav (one item, float) and its length n -> P float64 [nW, bins]: the power spectrum of every whole 30 ms
    window of the item's 16-bit PCM, p = clip(rint(float64(float32(wav)) * 32767), -32768, 32767), times the periodic Hann window, zero-padded
    to LRT_N_FFT, at the bins LRT_K_LO .. LRT_K_HI."""
    spw = VAD_WINDOW_MS * sr // 1000
    x = np.asarray(wav, dtype=np.float32).reshape(-1)
    nw = min(int(n), len(x)) // spw
    p = np.clip(np.rint(x[:nw * spw].astype(np.float64) * 32767.0), -32768.0, 32767.0).reshape(nw, spw)
    X = np.fft.rfft(p * lrt_window(spw), n=LRT_N_FFT, axis=1)[:, LRT_K_LO:LRT_K_HI + 1]
    return X.real * X.real + X.imag * X.imag


def lrt_from_power(P):
    """Second half of `lrt_statistic`: P float64 [nW, bins] -> (stat float64 [nW], flags uint8 [nW]). Every sum runs in the stated order
    (np.cumsum adds one term after the other; np.sum would add pairwise)."""
    P = np.asarray(P, dtype=np.float64)
    nw, nb = P.shape
    if nw == 0:
        return np.zeros(0, np.float64), np.zeros(0, np.uint8)
    E = np.cumsum(P, axis=1)[:, -1]                                   # ascending k
    q = max(1, -(-nw // LRT_Q_DIV))
    quiet = np.sort(np.argsort(E, kind="stable")[:q])                 # the q smallest, ties to the smaller index; then ascending window index
    N = np.cumsum(P[quiet], axis=0)[-1] / q
    n_sum, thr = np.cumsum(N)[-1], E.max() * 10.0 ** (-LRT_PEAK_DB / 10.0)
    if n_sum > thr:                                                   # no pauses, or noisy: towards "everything is voice"
        N = N * (thr / n_sum)
    N = np.maximum(N, LRT_N_MIN)
    g = P / N
    over = g > 1.0
    term = np.where(over, (g - np.log(np.where(over, g, 1.0))) - 1.0, 0.0)
    stat = np.cumsum(term, axis=1)[:, -1] / nb
    return stat, (stat > LRT_ETA).astype(np.uint8)


def lrt_statistic(wav, n, sr=SAMPLING_RATE):
    """THE DEFINITION of the "lrt" voice-activity decision (host, float64, numpy only) for one item: wav (float), its length n ->
    (stat float64 [nW], flags uint8 [nW]), nW = n // 480 windows of 30 ms at the nominal 16 kHz. A likelihood-ratio test per window in the
    maximum-likelihood form of Sohn, Kim & Sung (1999); this function, not the paper, is what `ss_vad_lrt` computes:
      p        = clip(rint(float64(float32(wav)) * 32767), -32768, 32767): the 16-bit PCM `webrtc_flags` hands the package
      P[w][k]  = |rfft(p[480 w : 480 (w + 1)] * hann, 512)|^2 for k = 3 .. 127 (periodic Hann, zero-padded), E[w] = sum_k P[w][k] in ascending k
      N[k]     = mean of P[w][k] over the q = max(1, ceil(nW / 10)) windows of smallest E (ties to the smaller index), summed in ascending w
                 if sum_k N[k] > max_w E[w] * 10^(-LRT_PEAK_DB / 10): every N[k] scaled by the ratio; then N[k] = max(N[k], LRT_N_MIN)
      stat[w]  = (1 / 125) sum_k (g - ln g - 1 if g > 1 else 0), g = P[w][k] / N[k];   flags[w] = stat[w] > LRT_ETA
    nW == 0: empty outputs. The constants are unassessed on recordings; parity with webrtcvad is neither claimed nor wanted (module docstring)."""
    return lrt_from_power(lrt_power(wav, n, sr))


def lrt_table_f64(n_fft=LRT_N_FFT, spw=VAD_WINDOW_MS * SAMPLING_RATE // 1000):
    """The float64 table `ss_vad_lrt` reads: n_fft complex twiddles by butterfly span (the layout of `denoise.table_f64`: [2 (s + j)],
    [2 (s + j) + 1] = cos, -sin of 2 pi j / (2 s) for s = 1, 2, ..., n_fft / 2 and j < s; entry 0 unused), then the spw window values."""
    t = np.zeros(2 * n_fft + spw, dtype=np.float64)
    s = 1
    while s < n_fft:
        j = np.arange(s, dtype=np.float64)
        t[2 * s:4 * s:2] = np.cos(2.0 * np.pi * j / (2 * s))
        t[2 * s + 1:4 * s:2] = -np.sin(2.0 * np.pi * j / (2 * s))
        s *= 2
    t[2 * n_fft:] = lrt_window(spw)
    return t


@torch.no_grad()
def lrt_flags_device(wavs, lens, sr=SAMPLING_RATE):
    """`lrt_statistic` for a batch on the device (`ss_vad_lrt`: two launches, float64, no host synchronisation): wavs fp32 [B, L] on the device
    (the volume-normalised audio), lens host ints or an int32 device tensor [B] -> (flags uint8 [B, max_w], stat float64 [B, max_w]) on the
    device, 0 at and beyond an item's windows; max_w = max(1, L // spw) when the lengths are a device tensor (no read-back), else
    max(1, longest item // spw) as `trim_long_silences_device` counts them. What a row holds at or beyond its length is never read."""
    from .resample import _cached
    if not torch.is_tensor(wavs) or wavs.device.type != "cuda":
        raise L.StyleSingerHipError("lrt_flags_device needs device tensors: there is no CPU path")
    spw = VAD_WINDOW_MS * sr // 1000
    x = wavs if wavs.dtype == torch.float32 and wavs.dim() == 2 and wavs.stride(1) == 1 and wavs.stride(0) >= wavs.shape[1] else wavs.float().contiguous()
    if x.dim() != 2:
        raise ValueError(f"lrt_flags_device: wavs must be [B, L] (got {tuple(x.shape)})")
    B, Lx = x.shape
    dev = x.device
    if torch.is_tensor(lens):
        meta = lens.to(device=dev, dtype=torch.int32).clamp(max=Lx).contiguous()
        max_w = max(1, Lx // spw)
    else:
        ns = [min(int(n), Lx) for n in lens]
        meta = torch.tensor(ns, dtype=torch.int32).to(dev)
        max_w = max(1, max(n // spw for n in ns))
    if meta.numel() != B:
        raise ValueError("lrt_flags_device: one length per row")
    lib = L.load()
    ws_bytes = int(lib.ss_vad_lrt_workspace_bytes(B, max_w))
    if ws_bytes <= 0:
        raise L.StyleSingerHipError(f"ss_vad_lrt_workspace_bytes refused B={B} windows={max_w}")
    ws = torch.empty(ws_bytes // 8, device=dev, dtype=torch.float64)
    table = _cached(("vad_lrt_table", LRT_N_FFT, spw, dev), lambda: torch.from_numpy(lrt_table_f64(LRT_N_FFT, spw)).to(dev))
    flags = torch.empty(B, max_w, device=dev, dtype=torch.uint8)
    stat = torch.empty(B, max_w, device=dev, dtype=torch.float64)
    L.ops.ss_vad_lrt(x, x.stride(0), meta, B, max_w, spw, LRT_N_FFT, LRT_K_LO, LRT_K_HI, LRT_Q_DIV, LRT_PEAK_DB, LRT_N_MIN, LRT_ETA, table, flags,
                     max_w, stat, max_w, ws, ws_bytes)
    for t in (meta, ws):
        t.record_stream(torch.cuda.current_stream(dev))
    return flags, stat


@torch.no_grad()
def trim_long_silences_device(wavs, lens, flags, sr=SAMPLING_RATE):
    """wavs fp32 [B, L] on the device (zero beyond lens[b]; host ints), flags [B, nW] (0/1, a host array or a device tensor - that one is used where it lies; window w = samples [w * spw, (w + 1) * spw), spw = 30 ms)
    -> (trimmed [B, L'] fp32 zero padded, kept lengths as a list of host ints... computed on the device: int32 tensor [B])."""
    if wavs.device.type != "cuda":
        raise L.StyleSingerHipError("trim_long_silences_device needs device tensors: there is no CPU path")
    spw = VAD_WINDOW_MS * sr // 1000
    wavs = wavs.float().contiguous()
    B, Lx = wavs.shape
    ns = [min(int(n), Lx) for n in lens]
    max_w = max(1, max(n // spw for n in ns))
    if torch.is_tensor(flags) and flags.device.type == "cuda":   # e.g. `lrt_flags_device`'s: they stay where they are
        fl = flags if flags.dtype == torch.uint8 else flags.to(torch.uint8)
    else:
        fl = torch.as_tensor(np.asarray(flags)).to(torch.uint8)
    if fl.dim() != 2 or fl.shape[0] != B or fl.shape[1] < max_w:
        raise ValueError(f"trim_long_silences_device: flags must be [B, >= {max_w}] (one per {spw}-sample window), got {tuple(fl.shape)}")
    fl = fl.contiguous().to(wavs.device)
    if Lx < max_w * spw:
        raise ValueError("trim_long_silences_device: waveform buffer shorter than its windows")
    meta = torch.tensor(ns, dtype=torch.int32).to(wavs.device)
    out = torch.empty(B, max_w * spw, device=wavs.device, dtype=torch.float32)
    out_lens = torch.empty(B, device=wavs.device, dtype=torch.int32)
    win_dst = torch.empty(B, max_w, device=wavs.device, dtype=torch.int32)
    L.ops.ss_vad_trim(wavs, Lx, meta, fl, fl.shape[1], B, max_w, spw, VAD_MOVING_AVERAGE_WIDTH, VAD_MAX_SILENCE_LENGTH, out, out.shape[1], out_lens,
                      win_dst)
    for t in (meta, fl, win_dst):
        t.record_stream(torch.cuda.current_stream(wavs.device))
    return out, out_lens
