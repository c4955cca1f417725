"""What the vocoder output denoise costs on the device: `denoise.denoise_batch` (one ss_wav_denoise launch) at 8 x 8 s and 32 x 30 s of 48 kHz
audio (N = 1024, H = 256), next to the bytes it has to move (one read of the waveform, one write: there is no workspace) and the share of the HBM
roof that is (8.0 TB/s peak). For context, `torch.stft -> subtraction -> torch.istft` of the same rows on the same device. Device events on the
stream around every call, after warm-up; the median of --iters calls (min .. max), WARM (back to back on the same input) - DESIGN.md 3.5b.
    python tools/denoise_timing.py [--iters 20] [--json profiles/denoise_timing.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import denoise as DN  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

HBM_PEAK = 8.0e12
RATE = 48000


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def torch_route(x, n_fft, hop, v):
    """whole rows (no per-item lengths: torch has none), fp32"""
    w = torch.hann_window(n_fft, periodic=True, device=x.device)
    S = torch.stft(x, n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="constant", return_complex=True)
    m = S.abs()
    return torch.istft(S * (torch.clamp(m - v, min=0.0) / m.clamp(min=1e-30)), n_fft, hop_length=hop, win_length=n_fft, window=w, center=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fft-size", type=int, default=1024)
    ap.add_argument("--hop-size", type=int, default=256)
    ap.add_argument("--v", type=float, default=0.1)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H = a.fft_size, a.hop_size
    rows = []
    for B, secs in ((8, 8), (32, 30)):
        n = secs * RATE
        g = torch.Generator(device=dev).manual_seed(B)
        x = 0.1 * torch.randn(B, n, device=dev, generator=g)
        lens = torch.tensor([n - 7 * H * b for b in range(B)], dtype=torch.int32, device=dev)
        y, n_out = DN.denoise_batch(x, lens, N, H, N, a.v)      # uploads the table
        assert torch.isfinite(y).all() and torch.equal(n_out, lens)
        ref = torch_route(x[:1], N, H, a.v)
        err = (y[0, :ref.shape[1]] - ref[0]).abs().max().item()
        frames = int((lens // H + 1).sum())
        nbytes = int(2 * 4 * lens.sum())
        for name, fn in (("ss_wav_denoise", lambda: DN.denoise_batch(x, lens, N, H, N, a.v)), ("torch_stft_istft", lambda: torch_route(x, N, H, a.v))):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = timed(fn, a.iters)
            row = dict(call=name, B=B, seconds=secs, rate=RATE, fft_size=N, hop_size=H, v=a.v, frames=frames, mode="warm", iters=a.iters, median_ms=med,
                       min_ms=lo, max_ms=hi, bytes=nbytes, hbm_floor_ms=nbytes / HBM_PEAK * 1e3, share_of_hbm_roof=nbytes / HBM_PEAK * 1e3 / med,
                       max_abs_diff_to_torch_fp32_item0=err)
            rows.append(row)
            print(f"{name:17s} {B:2d} x {secs:2d} s ({frames} frames): {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})   {nbytes / 1e6:8.1f} MB -> "
                  f"{nbytes / med / 1e6:7.1f} GB/s = {100 * row['share_of_hbm_roof']:.1f} % of the 8.0 TB/s roof", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
