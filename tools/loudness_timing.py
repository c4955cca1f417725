"""What loudness normalisation costs on the device: `loudness.normalize_batch` (ss_loudness_measure + ss_loudness_apply) at 8 x 8 s and 32 x 30 s of
48 kHz audio, next to the bytes each pass has to move and the share of the HBM roof that is (8.0 TB/s peak; a float4 copy reaches 6.29 TB/s).
Device events on the stream around every call, after warm-up; the median of --iters calls (min .. max), COLD (a 512 MiB buffer is rewritten
before every timed call, so neither the audio nor the workspace is in a cache) and WARM (back to back on the same input) - DESIGN.md 3.4.
    python tools/loudness_timing.py [--iters 20] [--chunk 256] [--json profiles/loudness_timing.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import loudness as LD  # noqa: E402

HBM_PEAK = 8.0e12
RATE = 48000


def bytes_moved(B, n, C):
    """What the algorithm needs per call, from the shapes: both chunk passes read the audio (the second one re-runs the cascade instead of storing
    the float64 output), the per-chunk workspace (end state 32 B + max 4 B written, read once; carry 32 B written, read once; (pre, post) 16 B
    written, read ~once), and the apply pass reads the audio and writes the result."""
    nch = -(-n // C)
    measure = B * (2 * 4 * n + nch * (2 * 32 + 2 * 4 + 2 * 32 + 2 * 16))
    apply = B * 2 * 4 * n
    return measure, apply


def timed(fn, iters, flush):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        if flush is not None:
            flush.add_(1.0)
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk", type=int, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    C = a.chunk or LD.DEFAULT_CHUNK
    flush = torch.zeros(128 * 1024 * 1024, device=dev)   # 512 MiB: twice the last-level cache
    rows = []
    for B, secs in ((8, 8), (32, 30)):
        n = secs * RATE
        g = torch.Generator(device=dev).manual_seed(B)
        x = 0.1 * torch.randn(B, n, device=dev, generator=g)
        lens = [n - 7 * b for b in range(B)]
        y, m = LD.normalize_batch(x, lens, RATE, chunk=C)      # uploads the tables and the block bounds
        assert torch.isfinite(m["lufs"]).all() and torch.isfinite(y).all()
        cases = dict(normalize=lambda: LD.normalize_batch(x, lens, RATE, chunk=C), measure=lambda: LD.measure_batch(x, lens, RATE, chunk=C))
        by_m, by_a = bytes_moved(B, n, C)
        for name, fn in cases.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            nbytes = by_m + (by_a if name == "normalize" else 0)
            for mode, fl in (("cold", flush), ("warm", None)):
                med, lo, hi = timed(fn, a.iters, fl)
                row = dict(call=name, B=B, seconds=secs, rate=RATE, chunk=C, mode=mode, iters=a.iters, median_ms=med, min_ms=lo, max_ms=hi, bytes=nbytes,
                           hbm_floor_ms=nbytes / HBM_PEAK * 1e3, share_of_hbm_roof=nbytes / HBM_PEAK * 1e3 / med)
                rows.append(row)
                print(f"{name:9s} {B:2d} x {secs:2d} s  chunk {C}  {mode}: {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})   {nbytes / 1e6:8.1f} MB -> "
                      f"{nbytes / med / 1e6:7.1f} GB/s = {100 * row['share_of_hbm_roof']:.1f} % of the 8.0 TB/s roof")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
