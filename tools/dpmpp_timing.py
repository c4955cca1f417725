"""What the mel stage costs per sampler: q_sample ... denorm (`Plans._run_mel` + ss_mel_denorm) as a captured hipGraph at the C2 shape (8 x 1500
frames in the 1536-frame bucket, fp32, synthetic weights, K_step = timesteps = 100, no vocoder), warm, the median of --iters replays between device
events, all in one process:
  * the reference's ancestral loop (ss_meldiff_sample, 100 network evaluations, batch halves on two streams as forward runs it);
  * DDIM with eta = 0 (ss_meldiff_sample_ddim) and DPM-Solver++ order 2 (ss_meldiff_sample_dpmpp) on the SAME log-SNR list
    (plans.logsnr_timesteps) for n in {10, 20, 50}.
The yardstick of the multistep sampler is DDIM on the same list in the same run: the same network evaluations, and per transition (all but the
last) one more launch that moves 5 x B*T*80*4 bytes. Reported: the ratio and the difference per transition - DESIGN.md 3.2.
    python tools/dpmpp_timing.py [--iters 20] [--json profiles/dpmpp_timing.json]"""
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=1500)
    ap.add_argument("--steps", type=int, nargs="+", default=[10, 20, 50])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    hp = config.make_hparams()
    K, M = hp["K_step"], hp["audio_num_mel_bins"]
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 1234))
    model.eval().to(dev)
    model._ensure_packed()
    pk = model._pk
    B, T = a.batch, model.bucket_frames(a.frames)
    pl = model._plan(B, T, dev)
    g = torch.Generator().manual_seed(1)
    pl.lens.fill_(a.frames)
    pl.cond_mel.copy_((torch.randn(B, T, hp["hidden_size"], generator=g) * 0.5).to(dev))
    smin, smax = pk["spec_min"], pk["spec_max"]
    pl.coarse_mel.copy_(smin + (smax - smin) * torch.rand(B, T, M, generator=g).to(dev))
    pl.seed.fill_(1234)
    mel_out = torch.empty(B, T, M, device=dev)
    model._dpmpp_buffers(pl)
    rows = []

    def measure(name, n_asked, ts, **kw):
        def fn():
            model._run_mel(pl, **kw)
            L.ops.ss_mel_denorm(pl.xm, smin, smax, mel_out, B, T, M, pl.lens, None)
        gr = model._capture(fn)
        for _ in range(a.warmup):
            gr.replay()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(mel_out).all())
        med, lo, hi = timed(gr.replay, a.iters)
        n = K if ts is None else len(ts)
        rows.append(dict(sampler=name, B=B, frames=a.frames, T=T, K_step=K, n_asked=n_asked, evaluations=n, ts=None if ts is None else list(ts),
                         mode="warm, hipGraph replay", iters=a.iters, median_ms=med, min_ms=lo, max_ms=hi, ms_per_evaluation=med / n))
        print(f"{name:6s} n = {n_asked:3d} ({n:3d} evaluations): {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})  {med / n:.4f} ms per evaluation", flush=True)
        return med

    ddpm = measure("ddpm", K, None)
    summary = dict(sampler="summary", ddpm_ms=ddpm, per_n={})
    for n in a.steps:
        ts = model.mel_timesteps(n, "logsnr")
        ddim = measure("ddim", n, ts, ddim_ts=ts, eta=0.0)
        dpm = measure("dpmpp", n, ts, dpmpp=(ts, 2))
        ddim2 = measure("ddim", n, ts, ddim_ts=ts, eta=0.0)     # the yardstick again: its own run-to-run spread
        per = (dpm - ddim) / max(len(ts) - 1, 1)
        summary["per_n"][str(n)] = dict(evaluations=len(ts), ddim_ms=ddim, dpmpp_ms=dpm, ddim_again_ms=ddim2, dpmpp_over_ddim=dpm / ddim,
                                        ddim_again_over_ddim=ddim2 / ddim, extra_ms_per_transition=per, ddpm_over_dpmpp=ddpm / dpm)
        print(f"n = {n}: dpmpp / ddim = {dpm / ddim:.4f} (ddim repeated: {ddim2 / ddim:.4f}); {per * 1e3:+.1f} us per transition; ddpm / dpmpp = {ddpm / dpm:.2f}",
              flush=True)
    rows.append(summary)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
