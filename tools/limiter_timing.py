"""What the true-peak limiter costs on the device: `limiter.limit_batch` (ss_limit_true_peak) at 8 x 8 s and 32 x 30 s of 48 kHz audio, alone and as
the chain "measure + limit" next to today's "measure + apply" (`loudness.normalize_batch`), re-measured here in the same run; a torch composition
of the same definition on the same device (conv1d with the bank, max_pool1d of -r, avg_pool1d) for comparison; the share of the HBM roof at the 8
bytes per sample the limiter has to move (8.0 TB/s peak); and what bounds the launch: the same audio through banks cut to fewer taps moves the
same bytes, so a time that follows the tap count is interpolation FMA work, not memory. Device events on the stream around every call, after
warm-up, WARM (back to back on the same input, one batch at a time); the median of --iters calls (min .. max). Last, the loudness a high-crest item
ends at when the target is followed by the limiter (`measure_batch` on the output) - DESIGN.md 3.4g2.
    python tools/limiter_timing.py [--iters 20] [--json profiles/limiter_timing.json]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import limiter as LM  # noqa: E402
from stylesinger_amd import loudness as LD  # noqa: E402
from stylesinger_amd.resample import polyphase_bank  # noqa: E402

HBM_PEAK = 8.0e12
FMA_PEAK = 256 * 4 * 16 * 2.4e9     # fp32 FMAs per second, unpacked: 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz (v_pk_fma_f32 doubles it)
RATE = 48000
CEILING_DB = -1.0
TILE = 1856


def timed(fn, iters):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return statistics.median(ms), min(ms), max(ms)


def torch_composition(x, bank, left, c, W):
    """the definition with torch operators (full-length items: no per-item length)"""
    taps = bank.shape[1]
    it = F.conv1d(F.pad(x[:, None, :], (left, taps - 1 - left)), bank[:, None, :])
    e = torch.maximum(x.abs(), it.abs().amax(dim=1))
    r = torch.clamp(c / e, max=1.0)
    m = -F.max_pool1d(-F.pad(r[:, None, :], (W - 1, W - 1), value=1.0), W, stride=1)
    g = torch.minimum(r, F.avg_pool1d(m, W, stride=1)[:, 0, :])
    return g * x


def raw_limit(x, n_d, bank_d, taps, left, c, W, y, rep, ws, nbytes):
    B, Lx = x.shape
    L.check(L.load().ss_limit_true_peak(L.ptr(x), x.stride(0), Lx, L.ptr(n_d), None, L.ptr(bank_d), taps, left, float(c), W, L.ptr(y), Lx, Lx,
                                        L.ptr(rep[0]), L.ptr(rep[1]), None, B, L.ptr(ws), nbytes, L.stream_ptr()), "ss_limit_true_peak")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    c, W = float(LM.ceiling_f32(CEILING_DB)), LM.window_samples(RATE)
    bank, _, _, taps, left = polyphase_bank(RATE, 4 * RATE)
    bank_d = torch.from_numpy(bank.copy()).to(dev)
    rows = []

    def row(call, B, secs, med, lo, hi, **kw):
        nbytes = 8 * B * secs * RATE
        r = dict(call=call, B=B, seconds=secs, rate=RATE, W=W, iters=a.iters, median_ms=med, min_ms=lo, max_ms=hi, **kw)
        if call.startswith("limit"):
            r.update(bytes=nbytes, hbm_floor_ms=nbytes / HBM_PEAK * 1e3, share_of_hbm_roof=nbytes / HBM_PEAK * 1e3 / med)
        rows.append(r)
        print(f"{call:28s} {B:2d} x {secs:2d} s: {med:8.4f} ms  ({lo:.4f} .. {hi:.4f})  " + "  ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}"
                                                                                                  for k, v in r.items() if k not in ("call", "B", "seconds", "rate", "W", "iters", "median_ms", "min_ms", "max_ms")))
        return r

    for B, secs in ((8, 8), (32, 30)):
        n = secs * RATE
        g = torch.Generator(device=dev).manual_seed(B)
        x = 0.1 * torch.randn(B, n, device=dev, generator=g)
        x[:, ::997] *= 12.0                                    # sparse peaks over the ceiling
        lens = [n - 7 * b for b in range(B)]
        y, rep = LM.limit_batch(x, lens, RATE, CEILING_DB)     # uploads the bank and the lengths
        full = [n] * B
        yt = torch_composition(x, bank_d, left, c, W)
        yk, _ = LM.limit_batch(x, full, RATE, CEILING_DB)
        dev_vs_torch = float((yk - yt).abs().max())
        assert dev_vs_torch < 1e-3, dev_vs_torch
        m = LD.measure_batch(x, lens, RATE, target=-14.0)
        cases = {
            "limit": lambda: LM.limit_batch(x, lens, RATE, CEILING_DB),
            "limit(gain)": lambda: LM.limit_batch(x, lens, RATE, CEILING_DB, gain=m["gain"]),
            "measure": lambda: LD.measure_batch(x, lens, RATE, target=-14.0),
            "measure + apply": lambda: LD.normalize_batch(x, lens, RATE, target=-14.0),
            "measure + limit": lambda: LM.limit_batch(x, lens, RATE, CEILING_DB, gain=LD.measure_batch(x, lens, RATE, target=-14.0)["gain"]),
            "torch composition": lambda: torch_composition(x, bank_d, left, c, W),
        }
        med = {}
        for name, fn in cases.items():
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            med[name], lo, hi = timed(fn, a.iters)
            extra = {}
            if name == "limit":
                fmas = 4 * taps * B * n * (TILE + 2 * (W - 1)) / TILE      # every tile interpolates its halo too
                extra = dict(interp_fmas=fmas, fma_floor_ms_unpacked=fmas / FMA_PEAK * 1e3, n_limited=int(rep["n_limited"].sum()))
            if name == "torch composition":
                extra = dict(ratio_to_limit=med[name] / med["limit"], max_abs_diff_to_kernel=dev_vs_torch)
            row(name, B, secs, med[name], lo, hi, **extra)
        # what bounds the launch: the same bytes through shorter filters (the bank's middle taps: the numbers mean nothing, the work does)
        n_d = torch.tensor(lens, dtype=torch.int32, device=dev)
        nbytes = int(L.load().ss_limit_workspace_bytes(B, n))
        ws = torch.empty(nbytes // 8, device=dev, dtype=torch.float64)
        out = torch.empty_like(x)
        rp = (torch.empty(B, device=dev), torch.empty(B, device=dev, dtype=torch.int32))
        for tp in (taps, 63, 31, 7):
            lf = (tp - 1) // 2
            sub = bank_d[:, left - lf:left - lf + tp].contiguous()
            fn = lambda: raw_limit(x, n_d, sub, tp, lf, c, W, out, rp, ws, nbytes)
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t, lo, hi = timed(fn, a.iters)
            row(f"limit, bank cut to {tp} taps", B, secs, t, lo, hi, taps=tp)
    # achieved loudness: the target, then the limiter, on a high-crest item (10 s: a quiet floor with a burst every 50 ms)
    n = 10 * RATE
    g = torch.Generator(device=dev).manual_seed(3)
    x = 0.02 * torch.randn(1, n, device=dev, generator=g)
    x[:, ::2400] = 0.9
    loud = []
    for target in (-23.0, -16.0, -14.0):
        m = LD.measure_batch(x, [n], RATE, target=target)
        y, rep = LM.limit_batch(x, [n], RATE, CEILING_DB, gain=m["gain"])
        after = LD.measure_batch(y, [n], RATE, target=target)
        ya, _ = LD.normalize_batch(x, [n], RATE, target=target)
        rule = LD.measure_batch(ya, [n], RATE, target=target)
        d = dict(target_lufs=target, input_lufs=float(m["lufs"][0]), crest_db=20 * np.log10(float(m["peak"][0])) - float(m["lufs"][0]),
                 gain_times_peak=float(m["gain"][0] * m["peak"][0]), limiter_lufs=float(after["lufs"][0]), shortfall_lu=target - float(after["lufs"][0]),
                 peak_rule_lufs=float(rule["lufs"][0]), peak_rule_shortfall_lu=target - float(rule["lufs"][0]), n_limited=int(rep["n_limited"][0]),
                 min_gain=float(rep["min_gain"][0]), out_peak=float(y.abs().max()))
        loud.append(d)
        print("achieved loudness: " + "  ".join(f"{k} {v:.4f}" if isinstance(v, float) else f"{k} {v}" for k, v in d.items()))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=L.load().ss_abi_version(), ceiling_db=CEILING_DB, rows=rows,
                           achieved_loudness=loud), fh, indent=1)
    return rows


if __name__ == "__main__":
    main()
