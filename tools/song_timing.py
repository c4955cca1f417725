"""What stitching a song costs on the device: `ss_song_offsets` + three `ss_song_place` per batch (waveform with joint fades, mel, f0) for 32
segments x 12 s at 48 kHz rendered as 4 batches of 8 rows, next to `torch.cat` of the cropped rows of the same inputs (which needs the lengths on
the host and fades nothing). Device events around every call, after warm-up; the WARM median of --iters calls (min .. max) - DESIGN.md 3.4h.
    python tools/song_timing.py [--iters 20] [--json profiles/song_timing.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import song  # noqa: E402

HBM_PEAK = 8.0e12
RATE, HOP = 48000, 256


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
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
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=12.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--fade-ms", type=float, default=5.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, T = a.segments, int(a.seconds * RATE / HOP)
    g = torch.Generator().manual_seed(S)
    lens_h = torch.randint(int(0.8 * T), T + 1, (S,), generator=g).tolist()      # ragged: 80 .. 100 % of the row
    order = sorted(range(S), key=lambda s: -lens_h[s])
    rows = [order[i:i + a.batch] for i in range(0, S, a.batch)]
    gd = torch.Generator(device=dev).manual_seed(1)
    res = [dict(wav=torch.randn(len(r), T * HOP, device=dev, generator=gd), mel=torch.randn(len(r), T, 80, device=dev, generator=gd),
                f0=torch.randn(len(r), T, device=dev, generator=gd)) for r in rows]
    segs = [torch.tensor(r, dtype=torch.int32, device=dev) for r in rows]
    lens = torch.tensor(lens_h, dtype=torch.int32, device=dev)
    F = sum(lens_h)
    fade = int(round(a.fade_ms * RATE / 1000))
    win = torch.from_numpy(song.fade_window(fade)).to(dev)
    wav, mel, f0 = (torch.empty(F * u, device=dev) for u in (HOP, 80, 1))
    offsets = torch.empty(S + 1, dtype=torch.int64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)

    def stitch():
        song.song_offsets(lens, out=offsets)
        for seg, r in zip(segs, res):
            song.song_place(r["wav"], seg, lens, offsets, HOP, wav, win=win, flags=flags)
            song.song_place(r["mel"], seg, lens, offsets, 80, mel, flags=flags)
            song.song_place(r["f0"], seg, lens, offsets, 1, f0, flags=flags)

    where = {s: (i, k) for i, r in enumerate(rows) for k, s in enumerate(r)}

    def cat():
        parts = [(res[i], k, lens_h[s]) for s in range(S) for i, k in (where[s],)]
        return (torch.cat([r["wav"][k, :n * HOP] for r, k, n in parts]), torch.cat([r["mel"][k, :n] for r, k, n in parts]),
                torch.cat([r["f0"][k, :n] for r, k, n in parts]))

    stitch()
    w2, m2, f2 = cat()
    torch.cuda.synchronize()
    assert flags.item() == 0 and torch.equal(mel.view(F, 80), m2) and torch.equal(f0, f2)
    assert int((wav != w2).sum()) <= 2 * fade * (S - 1), "the waveform differs from the plain concatenation only inside the joint fades"
    nbytes = 2 * 4 * F * (HOP + 80 + 1)      # every float of the song read once and written once
    out = []
    for name, fn in (("stitch", stitch), ("torch_cat", cat)):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        med, lo, hi = timed(fn, a.iters)
        out.append(dict(call=name, segments=S, seconds=a.seconds, batch=a.batch, rate=RATE, fade=fade, frames=F, mode="warm", iters=a.iters, median_ms=med,
                        min_ms=lo, max_ms=hi, bytes=nbytes, share_of_hbm_roof=nbytes / HBM_PEAK * 1e3 / med,
                        launches=1 + 3 * len(rows) if name == "stitch" else 3))
        print(f"{name:9s} {S} x {a.seconds:g} s in batches of {a.batch}, warm: {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})   {nbytes / 1e6:8.1f} MB -> "
              f"{nbytes / med / 1e6:7.1f} GB/s = {100 * out[-1]['share_of_hbm_roof']:.1f} % of the 8.0 TB/s roof")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=out), fh, indent=1)
    return out


if __name__ == "__main__":
    main()
