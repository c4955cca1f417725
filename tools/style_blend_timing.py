"""What a pool of references costs in the aligned-style stage (model._align_style: both CrossAttenLayers - q / kv GEMMs, attention, out
projection, two layernorms and the FFN each) at the C2 shape, B = 8, T = 1500 frames, Tr = 1500 frames per reference:
  * "plain": one reference through `ss_attention` (a style cache from encode_style: the path every single-reference call takes);
  * "seg R": a blend cache of R = 1, 2, 4 references through `ss_attention_seg` (Ts = 1504: Tr padded to the 32-key tile);
and, for the attention launch alone on the same q / kv, `ss_attention_seg` over R segments next to R separate `ss_attention` launches over
the same clips (what one would run without the segmented form; their outputs would still have to be merged). Random weights and activations: the
cost does not depend on the values. Device events around every call, after warm-up; the median of --iters calls (min .. max), WARM - DESIGN.md 3.2.
    python tools/style_blend_timing.py [--iters 20] [--json profiles/style_blend_timing.json]"""
import argparse
import json
import math
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import synth  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402
from tools.contour_align_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, T, Tr, H = 8, 1500, 1500, 256
    Ts = (Tr + 31) // 32 * 32
    model = StyleSingerHIP(None)
    model.load_state_dict(synth.synth_acoustic_state_dict(model.hp, 5), strict=True)
    model.eval().to(dev)
    model._ensure_packed()
    g = torch.Generator(device=dev).manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    dec = rnd(B, T, H)
    passthrough = {k: torch.zeros(B, 1, device=dev) for k in ("ref_f0", "style_pre_rq", "rq_codes", "style_rq")}

    def stage(cache):
        c = types.SimpleNamespace(ret={}, dev=dev, ctl=types.SimpleNamespace(style_cache=cache, ref_weights=None), B=B, T=T, dec=dec, f32=dict(device=dev, dtype=torch.float32))
        model._align_style(c, None, None)
        return c.style

    caches = {"plain": dict(sty=rnd(B, Tr, H), lens_r=torch.full((B,), Tr, dtype=torch.int32, device=dev), **passthrough)}
    for R in (1, 2, 4):
        caches[f"seg R={R}"] = dict(sty=rnd(B, R * Ts, H), seg_lens=torch.full((B, R), Tr, dtype=torch.int32, device=dev),
                                    seg_logw=torch.full((B, R), math.log(1.0 / R), device=dev), **passthrough)
    rows, per = [], {}

    def measure(name, fn, **info):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        med, lo, hi = timed(fn, a.iters)
        per[name] = med
        rows.append(dict(call=name, B=B, T=T, Tr=Tr, mode="warm", iters=a.iters, median_ms=med, min_ms=lo, max_ms=hi, **info))
        print(f"{name:46s}: {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})", flush=True)

    for name, cache in caches.items():
        assert torch.isfinite(stage(cache)).all()
        measure("align_style stage, " + name, lambda cache=cache: stage(cache), keys=int(cache["sty"].shape[1]))
    # the attention launch alone
    q = rnd(B, T, H)
    att = torch.empty(B, T, H, device=dev)
    scale = (H // 2) ** -0.5
    for R in (1, 2, 4):
        kv = rnd(B, R * Ts, 2 * H)
        cache = caches[f"seg R={R}"]
        common = dict(B=B, H=2, D=H // 2, Tq=T, ldq=H, ldk=2 * H, ldv=2 * H, ldo=H, q_bs=T * H, k_bs=R * Ts * 2 * H, v_bs=R * Ts * 2 * H, o_bs=T * H,
                      scale=scale)
        seg = lambda: L.attention_seg(q, kv, kv[:, :, H:], att, R=R, Ts=Ts, seg_lens=cache["seg_lens"], seg_logw=cache["seg_logw"], **common)
        lens = caches["plain"]["lens_r"]

        def separate():
            for r in range(R):
                clip = kv[:, r * Ts:(r + 1) * Ts]
                L.attention(q, clip, clip[:, :, H:], att, Tk=Ts, klens=lens, **common)
        measure(f"ss_attention_seg, R={R}", seg, keys=R * Tr)
        measure(f"{R} x ss_attention, one clip each", separate, keys=R * Tr)
    rows.append(dict(call="ratios", seg_R1_stage_over_plain_stage=per["align_style stage, seg R=1"] / per["align_style stage, plain"],
                     seg_R2_stage_over_R1=per["align_style stage, seg R=2"] / per["align_style stage, seg R=1"],
                     seg_R4_stage_over_R1=per["align_style stage, seg R=4"] / per["align_style stage, seg R=1"],
                     seg_R4_launch_over_R1=per["ss_attention_seg, R=4"] / per["ss_attention_seg, R=1"],
                     seg_R4_launch_over_4_plain_launches=per["ss_attention_seg, R=4"] / per["4 x ss_attention, one clip each"]))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), rows=rows), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
