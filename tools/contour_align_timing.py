"""What the contour alignment costs on the device: `pitch.contour_align_device` (one ss_contour_align launch, workspace allocation included) at
8 x (T = Lc = 1500) in a 375-frame band (2 s at 48 kHz / hop 256), the same on the full matrix, and 32 x (T = Lc = 5625) in the band. Device events
around every call, after warm-up; the median of --iters calls (min .. max), WARM - DESIGN.md 3.2.
Every shape is timed on two inputs whose dynamic programme is the same work but whose walk back differs: "ramp" (every frame its own note, guide =
score: the path is the diagonal, n - 1 steps) and "flat" (one note throughout: all costs 0, the tie order sends the walk up and left in turn,
2 n - 2 steps). Their difference over n - 1 is the cost of one step of the serial walk (a dependent byte load by one lane); what is left of the
ramp time is the sweep (one workgroup barrier per diagonal, 2 n - 1 diagonals).
    python tools/contour_align_timing.py [--iters 20] [--json profiles/contour_align_timing.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import pitch as P  # noqa: E402


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
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for B, n, band in ((8, 1500, 375), (8, 1500, None), (32, 5625, 375)):
        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
        per = {}
        for content in ("ramp", "flat"):
            if content == "ramp":   # a note per frame, cycling through four octaves in steps of a semitone: neighbours always differ
                midi = (36 + torch.arange(n, device=dev) % 48).repeat(B, 1).contiguous()
            else:
                midi = torch.full((B, n), 60, dtype=torch.int64, device=dev)
            hz = (440.0 * torch.exp2((midi.double() - 69.0) / 12.0)).float().contiguous()
            fn = lambda: P.contour_align_device(hz, None, midi, lens, n, band=band)
            out, idx, cost, status = fn()
            torch.cuda.synchronize()
            assert status.abs().sum().item() == 0 and cost.abs().sum().item() == 0 and torch.equal(out, hz)
            steps = int((idx[0, 1:] != idx[0, :-1]).sum().item())
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            med, lo, hi = timed(fn, a.iters)
            per[content] = med
            ws = int(L.load().ss_contour_align_workspace_bytes(B, n, n, band or 0))
            rows.append(dict(call="contour_align_device", B=B, T=n, Lc=n, band=band, content=content, mode="warm", iters=a.iters, median_ms=med, min_ms=lo,
                             max_ms=hi, workspace_bytes=ws, diagonals=2 * n - 1, distinct_guide_frames_item0=steps + 1))
            print(f"contour_align_device {B:2d} x {n} band {band or 'full'} {content}: {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})  workspace {ws / 1e6:.1f} MB",
                  flush=True)
        step_us = (per["flat"] - per["ramp"]) / (n - 1) * 1e3       # flat walks n - 1 steps more than ramp
        walk_ramp = step_us * (n - 1) / 1e3
        rows.append(dict(call="split", B=B, T=n, band=band, walk_step_us=step_us, walk_ms_ramp=walk_ramp, walk_ms_flat=2 * walk_ramp,
                         sweep_ms=per["ramp"] - walk_ramp, sweep_us_per_diagonal=(per["ramp"] - walk_ramp) / (2 * n - 1) * 1e3))
        print(f"  -> one step of the walk {step_us:.3f} us; walk {walk_ramp:.3f} ms (ramp) / {2 * walk_ramp:.3f} ms (flat); sweep "
              f"{per['ramp'] - walk_ramp:.3f} ms = {(per['ramp'] - walk_ramp) / (2 * n - 1) * 1e3:.3f} us per diagonal", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
