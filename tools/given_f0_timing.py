"""What a caller who brings the f0 contour saves: StyleSingerHIP.forward at the C2 shape (8 x 1500 frames, 100 mel + 2 x 100 f0 steps, fp32, hipGraphs
on) with the f0 predicted, and with the same contour GIVEN (f0= / uv= of the first forward's pitch_pred: no ss_f0_bounds, no f0 pair loop). One
batch at a time, the model alone (no vocoder). Warm-up, then the median of --iters timed forwards each.
    python tools/given_f0_timing.py [--B 8] [--T 1500] [--steps 100] [--iters 7]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=1500)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    hp = config.make_hparams(dict(timesteps=a.steps, K_step=a.steps, f0_timesteps=a.steps))
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 1234))
    model.eval().to(dev)
    model.use_graphs = "on"
    Tp, Tr = max(2, a.T * 28 // 1500), min(a.T, 1500)     # the benchmark's score and reference lengths
    b = {k: v.to(dev) for k, v in synth.synth_batch(a.B, a.T, Tp, Tr, hp, 1234).items()}

    def fwd(**kw):
        return model(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"],
                     ref_f0=b["ref_f0"], global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"],
                     seed=1234, **kw)

    def timed(**kw):
        for _ in range(a.warmup):
            fwd(**kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(5, a.iters)):
            t0 = time.perf_counter()
            fwd(**kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms), min(ms), max(ms)
    pred = fwd()
    f0, uv = pred["pitch_pred"][..., 0].contiguous(), pred["pitch_pred"][..., 1].contiguous()
    same = torch.equal(fwd(f0=f0, uv=uv)["mel_out"], pred["mel_out"])
    p = timed()
    g = timed(f0=f0, uv=uv)
    print(f"forward at {a.B} x {a.T} frames, {a.steps} mel + 2 x {a.steps} f0 steps, hipGraphs on, median of {max(5, a.iters)} (min .. max), ms:")
    print(f"  f0 predicted   {p[0]:8.2f}  ({p[1]:.2f} .. {p[2]:.2f})")
    print(f"  f0 given       {g[0]:8.2f}  ({g[1]:.2f} .. {g[2]:.2f})   saves {p[0] - g[0]:.2f} ms = {100 * (p[0] - g[0]) / p[0]:.1f} %")
    print(f"  mel_out of the given-f0 forward bit-equal to the predicted one it was fed from: {same}")
    return p, g


if __name__ == "__main__":
    main()
