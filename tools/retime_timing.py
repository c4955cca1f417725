"""What singing in the guide's timing adds on the device (forward(pitch_timing="guide")): `pitch.retime_device` (one ss_retime_mel2ph launch, its
four outputs allocated) alone, and the alignment + retime pair next to the alignment alone (`pitch.contour_align_device`, unchanged), at
8 x (T = Lc = 1500) and 32 x (T = Lc = 5625) in a 375-frame band (2 s at 48 kHz / hop 256). Device events around every call, after warm-up; the
median of --iters calls (min .. max), WARM - DESIGN.md 3.2.
Two inputs per shape: "notes" (a new note every 20 frames, guide = score: n / 20 anchors, what a score looks like) and "ramp" (every frame its own
note: n anchors, the most the scans and the binary search can be given).
    python tools/retime_timing.py [--iters 20] [--json profiles/retime_timing.json]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import pitch as P  # noqa: E402
from tools.contour_align_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for B, n, band in ((8, 1500, 375), (32, 5625, 375)):
        lens = torch.full((B,), n, dtype=torch.int32, device=dev)
        mel2ph = (1 + torch.arange(n, device=dev) // 5).repeat(B, 1).contiguous()          # a phone every 5 frames
        for content, hold in (("notes", 20), ("ramp", 1)):
            midi = (36 + (torch.arange(n, device=dev) // hold) % 48).repeat(B, 1).contiguous()
            hz = (440.0 * torch.exp2((midi.double() - 69.0) / 12.0)).float().contiguous()
            align = lambda: P.contour_align_device(hz, None, midi, lens, n, band=band)
            _, idx, cost, st_a = align()
            retime = lambda: P.retime_device(mel2ph, lens, midi, idx, st_a, None, n)

            def both():
                _, i, _, s = align()
                return P.retime_device(mel2ph, lens, midi, i, s, None, n)
            out, src, status, n_spans = both()
            torch.cuda.synchronize()
            anchors = (n + hold - 1) // hold
            assert status.abs().sum().item() == 0 and cost.abs().sum().item() == 0 and torch.equal(out, mel2ph) and (n_spans == anchors).all()
            per = {}
            for name, fn in (("retime_device", retime), ("contour_align_device", align), ("contour_align_device + retime_device", both)):
                for _ in range(a.warmup):
                    fn()
                torch.cuda.synchronize()
                med, lo, hi = timed(fn, a.iters)
                per[name] = med
                rows.append(dict(call=name, B=B, T=n, Lc=n, band=band, content=content, anchors=anchors, mode="warm", iters=a.iters, median_ms=med,
                                 min_ms=lo, max_ms=hi))
                print(f"{name:38s} {B:2d} x {n} band {band} {content:5s}: {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})", flush=True)
            rows.append(dict(call="share", B=B, T=n, band=band, content=content,
                             retime_share_of_pair=per["retime_device"] / per["contour_align_device + retime_device"]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
