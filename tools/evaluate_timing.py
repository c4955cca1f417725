"""What the objective metrics cost on the device, and how far their float sums sit from the definition.
Parity: `align_device` + `reduce_device` against `evaluate.dtw_path` / `path_metrics` (path, cost and counts exact; the largest relative error of
the two float64 sums against math.fsum) and `ss_cosine_rows` in fp32 ulp of the float64 value -> evaluate_parity.json.
Timing: `score_pairs` (warm, median of 20, host wall including its one sync) at 8 x 1500 and 32 x 5625 frames, in the 2 s band and on the full
matrix, split per launch with device events, with `contour_align_device` at the same sizes in the same session as the yardstick
-> evaluate_timing.json.
    python tools/evaluate_timing.py [--out-dir profiles]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import evaluate_cases as K  # noqa: E402
from stylesinger_amd import evaluate as E  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import pitch as P  # noqa: E402

DEV = torch.device("cuda:0")
OUT = os.path.join(ROOT, "profiles")


def parity():
    rows, worst_d, worst_c = [], 0.0, 0.0
    for n_a, n_b, band, content in ((37, 53, None, "random"), (66, 62, 16, "ties"), (515, 509, None, "random"), (509, 515, 16, "ties"), (1500, 1400, 64, "random")):
        rng = np.random.default_rng(n_a)
        make = K.tie_q if content == "ties" else K.random_q
        qa, qb = make(rng, n_a), make(rng, n_b)
        fa, fb = K.random_f0(rng, n_a), K.random_f0(rng, n_b)
        dqa, dqb = torch.from_numpy(qa)[None].to(DEV), torch.from_numpy(qb)[None].to(DEV)
        al = E.align_device(dqa, [n_a], dqb, [n_b], band)
        counts, sums = E.reduce_device(dqa, torch.from_numpy(fa)[None].to(DEV), [n_a], dqb, torch.from_numpy(fb)[None].to(DEV), [n_b], al["path"], al["plen"])
        torch.cuda.synchronize()
        path, Pn, cost, status = E.dtw_path(qa, qb, band)
        want = E.path_metrics(qa, qb, fa, fb, path)
        got = sums.cpu().numpy()[0]
        rd = abs(got[0] - want["dist_sum"]) / want["dist_sum"]
        rc = abs(got[1] - want["cents_sq_sum"]) / want["cents_sq_sum"]
        worst_d, worst_c = max(worst_d, rd), max(worst_c, rc)
        exact = bool(np.array_equal(al["path"][0, :Pn].cpu().numpy(), path) and al["cost"].item() == cost and counts.cpu().numpy()[0].tolist() ==
                     [want["P"], want["n_both"], want["n_vde"], want["n_gpe"]])
        rows.append(dict(n_a=n_a, n_b=n_b, band=band, content=content, P=Pn, cost=cost, path_cost_counts_exact=exact, dist_sum_rel_err=rd,
                         dist_sum_bound=Pn * 2.0 ** -52, cents_sq_sum_rel_err=rc, cents_sq_sum_bound=(8 + 2 * Pn) * 2.0 ** -52))
    worst_u = 0.0
    for C in (1, 256):
        rng = np.random.default_rng(C)
        a, b = rng.standard_normal((64, C)).astype(np.float32), rng.standard_normal((64, C)).astype(np.float32)
        got = E.cosine_rows_device(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)).cpu().numpy()
        want = np.asarray([E.singer_cos(x, y) for x, y in zip(a, b)])
        ulp = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), 2.0 ** -126).astype(np.float32))
        worst_u = max(worst_u, float(ulp.max()))
    rep = dict(device=torch.cuda.get_device_name(0), lib_abi=int(L.load().ss_abi_version()), rows=rows, dist_sum_max_rel_err=worst_d,
               cents_sq_sum_max_rel_err=worst_c, cosine_max_fp32_ulp=worst_u)
    with open(os.path.join(OUT, "evaluate_parity.json"), "w") as fh:
        json.dump(rep, fh, indent=1)
    print(json.dumps({k: v for k, v in rep.items() if k != "rows"}))


def _median_ms(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def timing():
    rows = []
    lib = L.load()
    for B, T in ((8, 1500), (32, 5625)):
        g = torch.Generator(device="cpu").manual_seed(T)
        mel_a = (torch.randn(B, T, 80, generator=g) * 1.2 - 3.0).to(DEV)
        mel_b = (mel_a + 0.05 * torch.randn(B, T, 80, generator=g).to(DEV)).contiguous()
        f0_a = (220.0 + 60.0 * torch.rand(B, T, generator=g)).to(DEV)
        f0_b = (f0_a * 1.01).contiguous()
        lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
        hp = dict(audio_sample_rate=48000, hop_size=256)
        for band_s in (2.0, 0.0):
            band = E.band_frames(band_s, 48000, 256)
            med, lo, hi = _median_ms(lambda: E.score_pairs(mel_a, f0_a, lens, mel_b, f0_b, lens, align="dtw", band_s=band_s, hparams=hp))
            res = E.score_pairs(mel_a, f0_a, lens, mel_b, f0_b, lens, align="dtw", band_s=band_s, hparams=hp)
            rows.append(dict(call="score_pairs", B=B, T=T, band=band or None, mode="warm, host wall incl. the one sync", iters=20, median_ms=med, min_ms=lo,
                             max_ms=hi, plen_item0=int(res["plen"][0].item()), mcd_db_mean=res["mean"]["mcd_db"],
                             workspace_bytes=int(lib.ss_eval_dtw_workspace_bytes(B, T, T, band))))
            # split per launch
            qa, qb = E.mcep_q_device(mel_a, lens, hp), E.mcep_q_device(mel_b, lens, hp)
            ws_bytes = int(lib.ss_eval_dtw_workspace_bytes(B, T, T, band))
            ws = torch.empty(ws_bytes, device=DEV, dtype=torch.uint8)
            path = torch.empty(B, 2 * T, 2, device=DEV, dtype=torch.int32)
            plen, cost, status = (torch.empty(B, device=DEV, dtype=torch.int32) for _ in range(3))
            split = {}
            split["ss_eval_mcep (one side)"] = _median_ms(lambda: E.mcep_q_device(mel_a, lens, hp))[0]
            split["ss_eval_cost_band"] = _median_ms(lambda: L.check(lib.ss_eval_cost_band(L.ptr(qa), L.ptr(lens), L.ptr(qb), L.ptr(lens), 24, band, T, T, B, L.ptr(ws),
                                                                                     ws_bytes, L.stream_ptr()), "cost"))[0]
            split["ss_eval_dtw"] = _median_ms(lambda: L.check(lib.ss_eval_dtw(L.ptr(lens), L.ptr(lens), band, L.ptr(path), L.ptr(plen), L.ptr(cost), L.ptr(status), T, T, B,
                                                                         L.ptr(ws), ws_bytes, L.stream_ptr()), "dtw"))[0]
            split["ss_eval_reduce"] = _median_ms(lambda: E.reduce_device(qa, f0_a, lens, qb, f0_b, lens, path, plen))[0]
            rows.append(dict(call="split per launch (device events, median of 20)", B=B, T=T, band=band or None, **{k + "_ms": v for k, v in split.items()},
                             dtw_us_per_diagonal=1000.0 * split["ss_eval_dtw"] / (2 * T - 1)))
            del ws, path
            # the yardstick: ss_contour_align at the same sizes in the same session (ramp content: the path is the diagonal)
            midi = (48 + (torch.arange(T) // 40) % 24).to(torch.int64)[None].repeat(B, 1).to(DEV)
            hz = (440.0 * torch.exp2((midi.double() - 69.0) / 12.0)).float().contiguous()
            med, lo, hi = _median_ms(lambda: P.contour_align_device(hz, None, midi, lens, T, band=band or None))
            rows.append(dict(call="contour_align_device (yardstick, same session)", B=B, T=T, band=band or None, iters=20, median_ms=med, min_ms=lo, max_ms=hi))
            print(json.dumps(rows[-3:]))
            torch.cuda.empty_cache()
    with open(os.path.join(OUT, "evaluate_timing.json"), "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), lib_abi=int(lib.ss_abi_version()), rows=rows), fh, indent=1)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=OUT)
    OUT = os.path.abspath(ap.parse_args().out_dir)
    os.makedirs(OUT, exist_ok=True)
    parity()
    timing()
