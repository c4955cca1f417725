"""What the "lrt" voice-activity decision costs on the device: `vadtrim.lrt_flags_device` alone (two `ss_vad_lrt` launches, workspace allocation
and the upload of the lengths included) and followed by `vadtrim.trim_long_silences_device` (`ss_vad_trim`), at 8 x 8 s and 32 x 30 s of
nominal-16 kHz audio (266 and 1000 windows of 30 ms per item). Device events on the stream around every call, after warm-up; the median of
--iters calls (min .. max), WARM (back to back on the same input) - DESIGN.md 3.4e2. Where the webrtcvad package is importable the host loop
the reference runs (`vadtrim.webrtc_flags`: device -> host copy, one call per window) is timed on the wall clock next to it; otherwise the rows say
that it was not measured. Recorded, not gated: the rows of the shapes given are merged into the JSON file.
    python tools/vad_lrt_timing.py [--shapes 8x8 32x30] [--iters 20] [--json profiles/vad_lrt_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import vadtrim as V  # noqa: E402

RATE = V.SAMPLING_RATE


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def batch(B, secs, dev):
    """B items of `secs` seconds (item b shorter by 7 b windows): harmonics in bursts of 1.5 s with pauses of 0.6 s, white noise at -60 dBFS"""
    n = secs * RATE
    rng = np.random.default_rng(B)
    t = np.arange(n) / RATE
    x = np.zeros((B, n), dtype=np.float32)
    for b in range(B):
        f0 = 180.0 + 10.0 * b
        sig = sum(np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 6.28)) / h for h in range(1, 7)) * (0.3 / 1.8)
        gate = ((t + 0.1 * b) % 2.1) < 1.5
        x[b] = sig * gate + rng.standard_normal(n) * 1e-3
    lens = [n - 7 * 480 * b for b in range(B)]
    for b, m in enumerate(lens):
        x[b, m:] = 0
    return torch.from_numpy(x).to(dev), lens


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", nargs="+", default=["8x8", "32x30"], help="items x seconds")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for shape in a.shapes:
        B, secs = (int(v) for v in shape.split("x"))
        x, lens = batch(B, secs, dev)
        flags, stat = V.lrt_flags_device(x, lens)      # uploads the table
        windows = sum(m // 480 for m in lens)
        host = np.stack([np.pad(V.lrt_statistic(x[b].cpu().numpy(), lens[b])[1], (0, flags.shape[1] - lens[b] // 480)) for b in (0, B - 1)])
        assert np.array_equal(flags[[0, B - 1]].cpu().numpy(), host), "flags differ from the definition"
        voiced = float(flags.sum().item()) / windows
        calls = (("lrt_flags_device", lambda: V.lrt_flags_device(x, lens)),
                 ("lrt_flags_device+trim_long_silences_device", lambda: V.trim_long_silences_device(x, lens, V.lrt_flags_device(x, lens)[0])))
        for name, fn in calls:
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = timed(fn, a.iters)
            rows.append(dict(call=name, B=B, seconds=secs, rate=RATE, windows=windows, share_flagged=voiced, mode="warm", iters=a.iters, median_ms=med,
                             min_ms=lo, max_ms=hi))
            print(f"{name:44s} {B:2d} x {secs:2d} s ({windows} windows, {100 * voiced:.0f} % flagged): {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})", flush=True)
        if V.have_webrtcvad():
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                V.webrtc_flags(x, lens)
                t.append((time.perf_counter() - t0) * 1e3)
            rows.append(dict(call="webrtc_flags (host loop, wall clock)", B=B, seconds=secs, rate=RATE, windows=windows, mode="warm", iters=3,
                             median_ms=statistics.median(t), min_ms=min(t), max_ms=max(t)))
            print(f"webrtc_flags host loop: {statistics.median(t):.2f} ms", flush=True)
        else:
            rows.append(dict(call="webrtc_flags (host loop, wall clock)", B=B, seconds=secs, rate=RATE, windows=windows,
                             not_measured="the webrtcvad package is not importable on this machine"))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        doc = dict(rows=[])
        if os.path.exists(a.json):
            with open(a.json) as fh:
                doc = json.load(fh)
        keep = [r for r in doc.get("rows", []) if (r["B"], r["seconds"]) not in {(r2["B"], r2["seconds"]) for r2 in rows}]
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=keep + rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
