"""What the f0 / uv pair loop costs at a chosen number of steps: the captured hipGraph of `Plans._run_f0_pair` at the C2 shape (8 x 1500 frames in
the 1536-frame bucket, fp32, both denoisers in one grouped loop, synthetic weights, f0_timesteps = 100, no vocoder) - through the default entry
(ss_f0diff_sample, all 100 network times) and through the strided entry (ss_f0diff_sample_strided) at n in {100, 50, 25, 10}, eta = 1. Device events
around every replay (the x_T fill and the condition precompute are inside the graph, as in forward), after warm-up; the median of --iters replays.
The default entry is measured --repeats times, interleaved with nothing else, and max - min of those medians is its run-to-run spread: the strided
entry at n = 100 is compared against the default entry's FIRST median plus that spread, and every n's time per step is stated next to the default
entry's, all from this one run - DESIGN.md 3.2.
    python tools/f0_strided_timing.py [--iters 20] [--json profiles/f0_strided_timing.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    hp = config.make_hparams()
    S = hp["f0_timesteps"]
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 1234))
    model.eval().to(dev)
    model._ensure_packed()
    B, T = a.batch, model.bucket_frames(a.frames)
    pl = model._plan(B, T, dev)
    g = torch.Generator().manual_seed(1)
    pl.lens2.fill_(a.frames)
    pl.cond2.copy_((torch.randn(2 * B, T, hp["hidden_size"], generator=g) * 0.5).to(dev))
    pl.cond2[:, a.frames:] = 0
    mid = torch.rand(2 * B, T, generator=g) * 2 - 1
    pl.lo2.copy_((mid - 0.25).to(dev))
    pl.hi2.copy_((mid + 0.25).to(dev))
    pl.seed.fill_(1234)

    def graph_of(ts):
        fn = lambda: model._run_f0_pair(pl, ts=ts, eta=1.0)
        pl.uv2.zero_()
        gr = model._capture(fn)

        def replay():
            pl.uv2.zero_()   # outside the graph, as forward's `prepare`
            gr.replay()
        return replay

    rows = []

    def measure(name, ts, n):
        run = graph_of(ts)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(pl.f02[:, :a.frames]).all())
        med, lo, hi = timed(run, a.iters)
        rows.append(dict(call=name, B=B, frames=a.frames, T=T, f0_timesteps=S, n=n, eta=1.0, mode="warm, hipGraph replay", iters=a.iters, median_ms=med,
                         min_ms=lo, max_ms=hi, ms_per_step=med / n))
        print(f"{name:28s} n = {n:3d}: {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})  {med / n:.4f} ms per step", flush=True)
        return med

    base = [measure("ss_f0diff_sample", None, S) for _ in range(a.repeats)]
    spread = max(base) - min(base)
    per_n = {n: measure("ss_f0diff_sample_strided", model.f0_strided_timesteps(n), len(model.f0_strided_timesteps(n))) for n in (100, 50, 25, 10)}
    rows.append(dict(call="summary", default_median_ms=base[0], default_medians_ms=base, default_spread_ms=spread, strided_n100_ms=per_n[100],
                     strided_n100_minus_default_ms=per_n[100] - base[0], strided_n100_within_default_plus_spread=per_n[100] <= base[0] + spread,
                     default_ms_per_step=base[0] / S, strided_ms_per_step={str(n): v / n for n, v in per_n.items()}))
    print(f"default entry {base[0]:.3f} ms (repeated medians {min(base):.3f} .. {max(base):.3f}: spread {spread:.3f}); strided n = 100 "
          f"{per_n[100]:.3f} ms = default {per_n[100] - base[0]:+.3f} ms", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
