"""What the pitch expression controls add on the device (forward(pitch_correct=, vibrato_scale=, vibrato_add=)): `pitch.pitch_edit_device` - one
ss_pitch_edit_runs launch, one ss_pitch_edit launch and its small statistics launch - at 8 x 1500 and 32 x 5625 frames, W = 31 (the default 333 ms
window at 187.5 frames/s), with and without a synthetic vibrato: warm, then the median of 20 calls, each waited for. Next to it, from the same run,
the time of the default f0 pair loop the edit follows (a predicted-f0 forward minus the same forward with its contour given, as
tools/given_f0_timing.py measures it) at 8 x 1500, so that a reader sees the share. Writes profiles/pitch_edit_timing.json.
    python tools/pitch_edit_timing.py [--iters 20] [--steps 100] [--no-loop]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import pitch as P  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

SHAPES = ((8, 1500), (32, 5625))
W, FPS = 31, 187.5
VIBRATO = (5.5, 30.0, 47, 28)   # rate Hz, depth cents, delay and fade in frames (250 / 150 ms)


def _inputs(B, T, dev):
    """A note staircase (40-frame notes, every eighth a rest) carrying a 6 Hz / 50-cent vibrato; every item full length."""
    rng = np.random.default_rng(B * T)
    notes = rng.integers(55, 75, (B, T // 40 + 1))
    notes[:, 7::8] = 0
    midi = np.repeat(notes, 40, axis=1)[:, :T].astype(np.int64)
    t = np.arange(T)
    cents = P.EDIT_K0 + 100.0 * (np.where(midi > 0, midi, 69) - 69) + 50.0 * np.sin(2 * np.pi * 6.0 * t / FPS)[None, :]
    f = torch.from_numpy((cents / 1200.0).astype(np.float32)).to(dev)
    return f, torch.zeros(B, T, device=dev), torch.from_numpy(midi).to(dev), torch.full((B,), T, dtype=torch.int32, device=dev)


def _median_ms(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def _f0_loop_ms(B, T, steps, dev, iters=5):
    hp = config.make_hparams(dict(timesteps=steps, K_step=steps, f0_timesteps=steps))
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(synth.synth_acoustic_state_dict(hp, 1234))
    model.eval().to(dev)
    model.use_graphs = "on"
    b = {k: v.to(dev) for k, v in synth.synth_batch(B, T, max(2, T * 28 // 1500), min(T, 1500), hp, 1234).items()}
    fwd = lambda **kw: model(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"],
                             ref_f0=b["ref_f0"], global_steps=320000, infer=True, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"],
                             seed=1234, skip_decoder=True, **kw)
    pred = fwd()
    f0, uv = pred["pitch_pred"][..., 0].contiguous(), pred["pitch_pred"][..., 1].contiguous()
    p, g = _median_ms(fwd, iters, 3), _median_ms(lambda: fwd(f0=f0, uv=uv), iters, 3)
    e = _median_ms(lambda: fwd(pitch_correct=0.7, vibrato_scale=0.5), iters, 3)
    return dict(steps=steps, forward_to_pitch_predicted_ms=p["median_ms"], forward_to_pitch_given_ms=g["median_ms"],
                forward_to_pitch_predicted_edited_ms=e["median_ms"], f0_pair_loop_ms=p["median_ms"] - g["median_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--no-loop", action="store_true", help="skip the f0 pair loop's time")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch_edit_timing.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), W=W, iters=a.iters, vibrato=list(VIBRATO), shapes=[],
               note="wall time of one pitch_edit_device call (three launches and their allocations) including the wait for it; warm, median of iters")
    for B, T in SHAPES:
        f, u, midi, lens = _inputs(B, T, dev)
        row = dict(B=B, T=T, workgroups=B * ((T + P.EDIT_TILE - 1) // P.EDIT_TILE))
        row["correct_scale"] = _median_ms(lambda: P.pitch_edit_device(f, u, midi, lens, W, 0.7, 0.5), a.iters)
        row["with_vibrato_add"] = _median_ms(lambda: P.pitch_edit_device(f, u, midi, lens, W, 0.7, 0.5, VIBRATO, fps=FPS), a.iters)
        res["shapes"].append(row)
        print(f"{B} x {T}: correct + scale {row['correct_scale']['median_ms']:.3f} ms, with vibrato_add {row['with_vibrato_add']['median_ms']:.3f} ms "
              f"({row['workgroups']} workgroups)")
    if not a.no_loop:
        B, T = SHAPES[0]
        res["f0_pair_loop"] = dict(B=B, T=T, **_f0_loop_ms(B, T, a.steps, dev))
        loop = res["f0_pair_loop"]["f0_pair_loop_ms"]
        res["f0_pair_loop"]["edit_share_percent"] = 100.0 * res["shapes"][0]["with_vibrato_add"]["median_ms"] / loop
        print(f"{B} x {T}: default f0 pair loop ({a.steps} steps, hipGraphs on) {loop:.2f} ms; the edit is "
              f"{res['f0_pair_loop']['edit_share_percent']:.3f} % of it")
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    return res


if __name__ == "__main__":
    main()
