"""Diffusion plans of `StyleSingerHIP`: the static device buffers of the sampler loops for one (B, T bucket), the LRU cache
that owns them, and how a sampler loop runs on a plan - from a recorded noise tape, as a captured hipGraph, or eagerly.

`Plans` is a mixin of the model (uses `self._pk`, `self.hp`, `self._plans` and the graph / stream settings of the constructor)."""
import contextlib
import ctypes

import numpy as np
import torch

from . import lib as L

_lib = L.load


class _DiffPlan:
    """Static device buffers (+ optional captured hipGraphs) of the three diffusion loops for one (B, T).

    The loops are ~13 000 launches per pass; for small batches they are launch-bound, so the launch sequence is
    captured once per shape with `torch.cuda.CUDAGraph` (the raw HIP launches go to the capture stream) and replayed.
    Noise stays fresh across replays through the device seed word (`seed_dev` of the C-ABI)."""

    def __init__(self, model, B, T, dev):
        hp, pk, lib = model.hp, model._pk, _lib()
        H, M = hp["hidden_size"], hp["audio_num_mel_bins"]
        f32 = dict(device=dev, dtype=torch.float32)
        self.B, self.T = B, T
        self.seed = torch.zeros(1, device=dev, dtype=torch.int64)
        self.nonfinite = torch.zeros(1, device=dev, dtype=torch.int32)   # set by ss_mel_denorm when a valid frame is NaN / inf
        # f0 pair: items [0,B) = agnostic net, [B,2B) = specific net (grouped launches)
        self.lens2 = torch.zeros(2 * B, device=dev, dtype=torch.int32)
        self.lens = self.lens2[:B]
        self.cond2 = torch.empty(2 * B, T, H, **f32)
        self.cond_a, self.cond_b = self.cond2[:B], self.cond2[B:]
        self.lo2 = torch.empty(2 * B, T, **f32)
        self.hi2 = torch.empty(2 * B, T, **f32)
        self.f02 = torch.empty(2 * B, T, **f32)
        self.uv2 = torch.zeros(2 * B, T, device=dev, dtype=torch.int32)
        self.f0 = [self.f02[:B], self.f02[B:]]
        self.uv = [self.uv2[:B], self.uv2[B:]]
        self.ws_f0_bytes = lib.ss_wavenet_workspace_bytes(ctypes.byref(pk["f0_pair"]["net"]), 2 * B, T)
        self.ws_f0 = torch.empty(self.ws_f0_bytes, device=dev, dtype=torch.uint8)
        self.coarse_mel = torch.empty(B, T, M, **f32)
        self.cond_mel = torch.empty(B, T, H, **f32)
        self.xm = torch.empty(B, T, M, **f32)
        nsplit = 2 if (model.n_streams >= 2 and B >= 2) else 1
        self.bounds = [B * i // nsplit for i in range(nsplit + 1)]
        self.ws_mel = []
        for i in range(nsplit):
            nb = self.bounds[i + 1] - self.bounds[i]
            wsb = lib.ss_wavenet_workspace_bytes(ctypes.byref(pk["mel"]["net"]), nb, T)
            self.ws_mel.append((wsb, torch.empty(wsb, device=dev, dtype=torch.uint8)))
        self.ws_prodiff = None   # full-batch workspace of the ProDiff decoder when ws_mel is split (allocated on first use, plan-owned)
        # captured loops: "f0" (the f0 pair), ("f0", n_steps, eta) (its strided sampler), "mel" (DDPM or ProDiff), ("ddim", n_steps or times, eta),
        # ("dpmpp", times, order)
        self.graphs = {}
        self.plms_hist = None
        self.dpmpp_hist = None   # eps scratch + x0 history of the DPM-Solver++ sampler (allocated on first use, plan-owned: its graphs replay into it)
        self.uses = 0   # forwards that asked for this shape (auto mode captures on the second one)
        self.recount()

    g_f0 = property(lambda self: self.graphs.get("f0"))
    g_mel = property(lambda self: self.graphs.get("mel"))

    def recount(self):
        """Bytes this plan keeps alive, each storage once (cond_a / cond_b / lens / f0[i] / uv[i] are views of the pair buffers)."""
        seen, total = set(), 0

        def add(t):
            nonlocal total
            if not torch.is_tensor(t):
                return
            st = t.untyped_storage()
            if st.data_ptr() not in seen:
                seen.add(st.data_ptr())
                total += st.nbytes()
        for v in vars(self).values():
            if torch.is_tensor(v):
                add(v)
            elif isinstance(v, (list, tuple)):
                for e in v:
                    if isinstance(e, (list, tuple)):
                        for ee in e:
                            add(ee)
                    else:
                        add(e)
        self.bytes = total


def _capture(fn):
    """Warm up `fn` on a side stream, then capture it into a CUDAGraph (hipGraph)."""
    cur = torch.cuda.current_stream()
    s = torch.cuda.Stream()
    s.wait_stream(cur)
    with torch.cuda.stream(s):
        fn()
    cur.wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def strided_timesteps(S, n):
    """n network times of a schedule of S, strictly decreasing from S-1 to 0 at a uniform stride; n is clipped to [1, S] (n = S: all of them,
    n = 1: time 0 alone - linspace's first point)."""
    return sorted({int(round(v)) for v in np.linspace(0, S - 1, max(1, min(int(n), S)))}, reverse=True)


def logsnr_timesteps(ac64, K, n):
    """Network times of the first K of a schedule (ac64 = cumprod(1 - betas) in float64), spaced uniformly in the half log-SNR
    lambda_t = 1/2 log(ac_t / (1 - ac_t)) rather than in t: a grid of min(max(n, 2), K) points from lambda_{K-1} to lambda_0, each snapped to the
    nearest network time (numpy's first minimum on ties), together with both ends K-1 and 0, strictly decreasing. Several grid points may snap to
    one time - the list is then shorter than n. n = 1 is time K-1 alone (one evaluation there and the jump to x_0)."""
    K, n = int(K), int(n)
    if n <= 1 or K <= 1:
        return [K - 1]
    ac = np.asarray(ac64, np.float64)[:K]
    lam = 0.5 * np.log(ac / (1.0 - ac))
    grid = np.linspace(lam[K - 1], lam[0], min(max(n, 2), K))
    return sorted({int(np.argmin(np.abs(lam - g))) for g in grid} | {K - 1, 0}, reverse=True)


class Plans:
    """Mixin of StyleSingerHIP: the plan cache and the sampler loops that run on a plan."""

    def bucket_frames(self, T):
        b = self.t_bucket
        return T if b <= 1 else (T + b - 1) // b * b

    def _plan(self, B, T, dev, slot=0):
        """LRU cache of diffusion plans keyed by (B, T, device, slot), bounded by `plan_bytes` of workspace. `slot` separates
        the workspaces of forwards that run CONCURRENTLY on different HIP streams (forward(plan_slot=...))."""
        key = (B, T, dev.index) if slot == 0 else (B, T, dev.index, slot)
        pl = self._plans.get(key)
        self.plan_lookups += 1
        if pl is None:
            self.plan_misses += 1
            pl = _DiffPlan(self, B, T, dev)
            self._plans[key] = pl
            total = sum(p.bytes for p in self._plans.values())
            synced = False
            while total > self.plan_bytes and len(self._plans) > 1:
                if not synced:   # another slot's stream may still be replaying the victim's graph into its workspace
                    if torch.cuda.is_available():
                        torch.cuda.synchronize(dev)
                    synced = True
                _, old = self._plans.popitem(last=False)   # least recently used
                total -= old.bytes
                self.plan_evictions += 1
        else:
            self._plans.move_to_end(key)
        return pl

    def _want_graphs(self, pl):
        if self.use_graphs in ("1", "on", "true", True):
            return True
        if self.use_graphs in ("0", "off", "false", False):
            return False
        # auto (north_star: "the diffusion inner loop captured as a hipGraph"): capture once a shape comes back
        return pl.uses >= 2

    def _capture(self, fn):
        self.n_captures += 1
        return _capture(fn)

    def _run_loop(self, pl, slot, fn, *, tape=None, graphs=False, prepare=None):
        """Run one sampler loop: `fn(tape)` eagerly when recorded noise is given; else, when `graphs`, capture `fn()` once under
        `pl.graphs[slot]` and replay it; else `fn()` eagerly. `prepare()` (buffer resets that must stay OUTSIDE the captured graph)
        runs before every execution and again after a capture, whose warm-up and recording passes dirtied the buffers."""
        if prepare is not None:
            prepare()
        if tape is not None:
            fn(tape)
        elif graphs:
            if slot not in pl.graphs:
                pl.graphs[slot] = self._capture(fn)
                if prepare is not None:
                    prepare()
            pl.graphs[slot].replay()
        else:
            fn()

    @contextlib.contextmanager
    def _q4_guard(self, pl, eager):
        """"fp16q4": the kernels behind the mode convert their fp16 operand to fp4 on a FIXED scale (q_scale_gate / q_scale_z): on the first
        (eager) forward of every plan the library reduces max |a| / (6 q_scale) over every operand those launches read (ss_set_q4_guard);
        a checkpoint whose stream leaves the scale's range is refused instead of silently degrading the second product."""
        if not (eager and self.q4 and pl.uses <= 1):
            yield
            return
        lib = _lib()
        guard = torch.zeros(2, device=pl.xm.device, dtype=torch.int32)
        L.check(lib.ss_set_q4_guard(L.ptr(guard)), "ss_set_q4_guard")
        try:
            yield
        finally:
            L.check(lib.ss_set_q4_guard(None), "ss_set_q4_guard")
        worst = guard.view(torch.float32).cpu()
        if float(worst.max()) > 1.0:
            raise L.StyleSingerHipError(
                f"mfma_precision=fp16q4: an operand of the fp4 second product leaves its fixed scale (max |a| / (6 q_scale): gate "
                f"{float(worst[0]):.3g}, skip GEMM {float(worst[1]):.3g}; the stream x + dstep must stay within +-{6 * 2.0:g}) - this checkpoint "
                f"needs mfma_precision='fp16x2' (no fixed activation scale)")

    def _full_batch_ws(self, pl, keep=False):
        """(bytes, buffer) of a mel-denoiser workspace for the WHOLE batch (DDIM, PLMS and ProDiff do not split it over streams):
        ws_mel[0] unless the plan split it. Then `keep=False` gives a per-call temporary and `keep=True` a plan-owned one:
        ProDiff's workspace must outlive the call, because a captured graph replays into it (a per-call temporary would be freed
        and its address reused by the allocator while pl.graphs["mel"] still writes there)."""
        if len(pl.ws_mel) == 1:
            return pl.ws_mel[0]
        if keep and pl.ws_prodiff is not None:
            return pl.ws_prodiff
        wsb = _lib().ss_wavenet_workspace_bytes(ctypes.byref(self._pk["mel"]["net"]), pl.B, pl.T)
        ws = (wsb, torch.empty(wsb, device=pl.xm.device, dtype=torch.uint8))
        if keep:
            pl.ws_prodiff = ws
            pl.recount()
        return ws

    def _streams(self, n):
        """Side HIP streams: independent launch sequences (the two f0 samplers, batch halves of the mel sampler) run
        concurrently so that one sequence's kernel tails/launch gaps are filled by the other's blocks."""
        if not hasattr(self, "_side_streams") or len(self._side_streams) < n:
            self._side_streams = [torch.cuda.Stream() for _ in range(n)]
        return self._side_streams[:n]

    # Philox keys: the host part of every key is a CONSTANT per call site and all per-call variation comes from the device
    # word pl.seed, so that a captured graph (host arguments frozen at capture) and the eager launches draw the same noise
    # for the same `seed`, whatever was run before.
    def _run_f0_pair(self, pl, tape=None, ts=None, eta=1.0):
        """Both joint f0/uv samplers in ONE grouped loop (they are independent given their conditions). `ts` (network times, strictly
        decreasing) switches to the strided sampler `ss_f0diff_sample_strided` with `eta` = 0 deterministic Gaussian half ... 1 ancestral;
        tapes keep the reference's [S]... layout and are indexed by network time."""
        pk = self._pk
        B, T = pl.B, pl.T
        sdp = pl.seed
        net = pk["f0_pair"]["net"]
        sched = pk["f0_pair"]["sched"]
        if ts is not None and sched["strided_error"] is not None:   # the checkpoint's tables do not belong to its betas (packing.f0_strided_guard)
            raise L.StyleSingerHipError(sched["strided_error"])
        zs = us = None
        if tape is not None:
            zs, us = tape  # [S][2B][T], [S][2B][2][T]
        else:
            L.ops.ss_fill_normal_rows(pl.f02, 2 * B, T, T, 11, sdp)
        if ts is not None:
            ts = np.ascontiguousarray(np.asarray(ts, dtype=np.int32))
            L.ops.ss_f0diff_sample_strided(net, pl.f02, pl.uv2, pl.cond2, pl.lo2, pl.hi2, pl.lens2, 2 * B, T, ts, len(ts), 0, len(ts),
                                           sched["betas_f64"], float(eta), zs, us, 17, sdp, 1, pl.ws_f0, pl.ws_f0_bytes)
            return
        L.ops.ss_f0diff_sample(net, pl.f02, pl.uv2, pl.cond2, pl.lo2, pl.hi2, pl.lens2, 2 * B, T, zs, us, 17, sdp, 0, net.steps, 1, pl.ws_f0,
                               pl.ws_f0_bytes)

    def ddim_timesteps(self, n):
        """n network times, strictly decreasing from K-1 to 0 (uniform stride)."""
        return strided_timesteps(self.hp["K_step"], n)

    def f0_strided_timesteps(self, n):
        """The same rule over the f0 pair's schedule: n of its f0_timesteps network times, S-1 ... 0 (n = S: every time). One point cannot be
        both ends: n = 1 is time S-1 alone (the state IS x_{S-1}: one evaluation there and the jump to x_0), where the rule's single point is 0."""
        S = self.hp["f0_timesteps"]
        return [S - 1] if int(n) <= 1 else strided_timesteps(S, n)

    def _dpmpp_buffers(self, pl):
        """(hist, (bytes, workspace)) of the DPM-Solver++ sampler on this plan, both plan-owned: a captured graph replays into them, so they are
        allocated before `_run_loop` captures, never inside the loop function."""
        if pl.dpmpp_hist is None:
            pl.dpmpp_hist = torch.empty(2 * pl.B * pl.T * self.hp["audio_num_mel_bins"], device=pl.xm.device, dtype=torch.float32)
            pl.recount()
        return pl.dpmpp_hist, self._full_batch_ws(pl, keep=True)

    def _run_mel(self, pl, tape=None, ddim_ts=None, plms_interval=None, eta=0.0, dpmpp=None):
        """q_sample + the shallow reverse loop (batch halves on two streams); `ddim_ts` switches to the strided
        DDIM sampler (BASELINE config 5; `eta` = 0 deterministic ... 1 ancestral), `plms_interval` to the reference's PLMS sampler (pndm_speedup),
        `dpmpp` = (network times, order) to DPM-Solver++ multistep (`ss_meldiff_sample_dpmpp`; deterministic: of the tape only z_q is read)."""
        pk, hp = self._pk, self.hp
        B, T, M = pl.B, pl.T, hp["audio_num_mel_bins"]
        net = pk["mel"]["net"]
        K = hp["K_step"]
        sa = float(pk["mel"]["sched"]["sqrt_alphas_cumprod"][K - 1])
        s1 = float(pk["mel"]["sched"]["sqrt_one_minus_alphas_cumprod"][K - 1])
        sdp = pl.seed
        zq_n, zs_n = tape if tape is not None else (None, None)
        L.ops.ss_mel_qsample(pl.coarse_mel, pk["spec_min"], pk["spec_max"], sa, s1, zq_n, 23, sdp, pl.xm, B, T, M)
        if dpmpp is not None:
            ts = np.ascontiguousarray(np.asarray(dpmpp[0], dtype=np.int32))
            hist, (wsb, wsp) = self._dpmpp_buffers(pl)
            L.ops.ss_meldiff_sample_dpmpp(net, pl.xm, pl.cond_mel, pl.lens, B, T, ts, len(ts), 0, len(ts), pk["mel"]["sched"]["alphas_cumprod_f64"],
                                          int(dpmpp[1]), hist, 1, wsp, wsb)
            return
        if ddim_ts is not None or plms_interval is not None:
            ac = pk["mel"]["sched"]["alphas_cumprod_np"]  # host table, read by the loop driver at launch time
            wsb, wsp = self._full_batch_ws(pl)
        if plms_interval is not None:
            if pl.plms_hist is None:
                pl.plms_hist = torch.empty(6 * B * T * M, device=pl.xm.device, dtype=torch.float32)
                pl.recount()
            L.ops.ss_meldiff_sample_plms(net, pl.xm, pl.cond_mel, pl.lens, B, T, K, int(plms_interval), ac, 1, pl.plms_hist, wsp, wsb)
            return
        if ddim_ts is not None:
            ts = np.ascontiguousarray(np.asarray(ddim_ts, dtype=np.int32))
            ac64 = pk["mel"]["sched"]["alphas_cumprod_f64"]
            L.ops.ss_meldiff_sample_ddim(net, pl.xm, pl.cond_mel, pl.lens, B, T, ts, len(ts), ac64, float(eta), zs_n, 31, sdp, 1, wsp, wsb)
            return
        nsplit = len(pl.ws_mel)
        main = torch.cuda.current_stream()
        side = self._streams(nsplit) if nsplit > 1 else [main]
        zparts = [zs_n[:, pl.bounds[i]:pl.bounds[i + 1]].contiguous() if (zs_n is not None and nsplit > 1) else zs_n for i in range(nsplit)]
        for sd_ in set(side) - {main}:
            sd_.wait_stream(main)
        for i, strm in enumerate(side):
            b0, nb = pl.bounds[i], pl.bounds[i + 1] - pl.bounds[i]
            wsb, wsp = pl.ws_mel[i]
            with torch.cuda.stream(strm):
                L.ops.ss_meldiff_sample(net, pl.xm[b0:], pl.cond_mel[b0:], pl.lens[b0:], nb, T, zparts[i], 29 + 7919 * b0, sdp, 0, K, 1, wsp, wsb)
        for sd_ in set(side) - {main}:
            main.wait_stream(sd_)
