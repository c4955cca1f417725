"""`StyleSingerHIP` — host-side mirror of `modules/StyleSinger/stylesinger.py::StyleSinger` for inference.

Same constructor (`StyleSingerHIP(dictionary, out_dims=None)`), same `forward(...) -> dict` keys, and it
loads the reference `state_dict` unchanged (names + shapes are the weight contract), so
`inference/StyleSinger.py::build_model` / `tasks/StyleSinger/stylesinger.py::build_tts_model` can swap
the class and keep `load_ckpt(model, ..., 'model', strict=False)`.

All arithmetic runs in libstylesinger_hip.so (hand-written gfx950 kernels) through `lib.py`; torch is
used for device buffers, views/concats (data movement only) and the stream.  There is no CPU path.
"""
import collections
import math
import types

import torch

from . import controls
from . import lib as L
from . import spec as _spec
from .config import make_hparams
from .packing import Packing, _sin_table
from .plans import Plans, logsnr_timesteps


def _pad_frames(x, T, dim=-1):
    """Zero-pad axis `dim` of x to T frames (hipGraph bucket padding; padded frames are masked everywhere)."""
    n = x.shape[dim]
    if n == T:
        return x
    pad = [0, 0] * x.dim()
    pad[2 * (x.dim() - 1 - (dim % x.dim())) + 1] = T - n
    return torch.nn.functional.pad(x, pad)


def _noise_btm(x, dev, shape, T):
    """Recorded noise in the reference layout, `shape` = (*lead, B, M, T_out) once its unit axis is dropped -> device fp32
    [*lead, B, T, M], the frame axis zero-padded to the bucket T."""
    return _pad_frames(x.to(dev).float().reshape(*shape), T).transpose(-1, -2).contiguous()


def resolve_ref_weights(ref_weights, B, R):
    """The prior weights of a pool of R references per item -> (logw fp32 [B, R], p float64 [B, R]) as host numpy arrays: p = w / sum(w) in
    float64, logw = float32(log p) with -inf where p == 0 (R = 1 gives 0.0 exactly). `ref_weights`: None (equal weights), a length-R sequence
    (the same weights for every item) or [B, R]; host values - a device tensor is copied to the host. Refused with ValueError before a device is
    touched: another shape, a negative or non-finite weight, a row that sums to zero."""
    import numpy as np
    if B < 1 or R < 1:
        raise ValueError(f"ref_weights: {R} references for a batch of {B}: at least one each")
    if ref_weights is None:
        w = np.ones((B, R), dtype=np.float64)
    else:
        if torch.is_tensor(ref_weights):
            ref_weights = ref_weights.detach().cpu().numpy()
        w = np.array(ref_weights, dtype=np.float64)
        if w.ndim == 1 and w.shape[0] == R:
            w = np.broadcast_to(w, (B, R)).copy()
        if w.shape != (B, R):
            raise ValueError(f"ref_weights: shape {tuple(w.shape)} for {R} references and a batch of {B}: expected [{R}] or [{B}, {R}]")
    if not np.isfinite(w).all():
        raise ValueError("ref_weights: every weight must be finite")
    if (w < 0).any():
        raise ValueError("ref_weights: every weight must be >= 0")
    with np.errstate(over="ignore"):
        total = w.sum(axis=1, keepdims=True)
    if not (total > 0).all():
        raise ValueError("ref_weights: the weights of an item must not all be zero")
    p = w / total
    if not (p.sum(axis=1) > 0).all() or not np.isfinite(p).all():   # (w / sum(w) of huge weights: inf / inf)
        raise ValueError("ref_weights: the weights of an item do not normalise in float64")
    with np.errstate(divide="ignore"):
        logw = np.log(p).astype(np.float32)
    return logw, p


def blend_embeds(e, p):
    """The embedding of a reference pool: e [B, R, C] unit-norm embeddings, p [B, R] normalised weights (a tensor or host values) ->
    l2norm(sum_r p_r e_r) [B, C] fp32, divided by max(norm, 1e-12). Torch ops on e's device, no host sync."""
    e = e.float()
    p = torch.as_tensor(p).to(device=e.device, dtype=torch.float32)
    if e.dim() != 3 or tuple(p.shape) != tuple(e.shape[:2]):
        raise ValueError(f"blend_embeds: embeddings {tuple(e.shape)} with weights {tuple(p.shape)}: expected [B, R, C] and [B, R]")
    m = (e * p[:, :, None]).sum(dim=1)
    return m / m.norm(dim=1, keepdim=True).clamp_min(1e-12)


class StyleSingerHIP(Packing, Plans, torch.nn.Module):
    def __init__(self, dictionary=None, out_dims=None, hparams=None):
        super().__init__()
        hp = make_hparams(hparams)
        if dictionary is not None:
            hp["vocab_size"] = len(dictionary)
        self.hp = hp
        self.prodiff = hp.get("decoder", "diffsinger") == "prodiff"
        self.hidden_size = hp["hidden_size"]
        self.out_dims = out_dims or hp["audio_num_mel_bins"]
        self._names = []
        for name, shape in _spec.acoustic_spec(hp):
            self._names.append(name)
            self.register_buffer(self._mangle(name), torch.zeros(tuple(shape)), persistent=True)
        self._packed_version = -1
        self._weights_version = 0
        self._pk = None
        self._pos_table = None
        self.training = False
        import os
        self.n_streams = int(os.environ.get("SS_STREAMS", "1"))  # 2 = split the mel batch over two streams (slower at C2: half-size launches balance worse)
        # hipGraph capture of the diffusion loops: "auto"/"on" = capture per (B, T) on first use, "off" = eager launches
        self.use_graphs = os.environ.get("SS_GRAPHS", "auto")
        # Winograd form of the denoisers' 3-tap dilated convs (fewer matrix ops, fp32-rounding-equal results); SS_WINO=0: direct conv
        self.use_wino = os.environ.get("SS_WINO", "1") not in ("0", "off", "false")
        # Winograd output tile of the dilated conv: 4 = F(4,3) (6 products per 4 frames), 2 = F(2,3) (4 per 2); direct form = 6 per 2
        self.wino_m = int(os.environ.get("SS_WINO_M", "4"))
        assert self.wino_m in (2, 4), "SS_WINO_M must be 2 or 4"
        # per-layer output projection = residual half only; skip sum of all layers as one K = L*C GEMM per step
        self.defer_skip = os.environ.get("SS_DEFER_SKIP", "1") not in ("0", "off", "false")
        prec = os.environ.get("SS_PRECISION", hp.get("mfma_precision", "fp32"))
        if prec not in ("fp32", "bf16", "bf16x2", "fp16x2", "fp16q4", "fp16sd", "bf16x3"):
            raise ValueError(f"mfma_precision={prec!r}: expected fp32 | bf16 | bf16x2 | fp16x2 | fp16q4 | fp16sd | bf16x3")
        # "bf16x2" (BASELINE config 4 at fp32-grade parity): the bf16 mode's data path (hidden GEMMs on the bf16 matrix cores, operands bf16
        # in HBM) with every operand a (hi, mid) PAIR of bf16 terms and three products hi*hi + hi*mid + mid*hi per GEMM; the step-invariant
        # conditioner projection in exact fp32, skip_projection folded into the K = L*C skip GEMM as in fp32 mode. Measured on the reference's
        # 1000-step golden: plain bf16 operands 2.5e-3 mel L1 (bar 1e-4), this mode 4e-6 (oracle/bf16x3_numerics.py, tools/../study in DESIGN 3.1h).
        # "fp16x2": the same data path with FP16 terms and only the WEIGHTS split (hi, lo of w * 2^FP16_WSHIFT): two products a*hi + a*lo per
        # GEMM instead of three. Over 1000 steps the weight rounding is the coherent error, the activation rounding averages out and fp16's is
        # 8x smaller than bf16's: 1.9e-5 on the same golden (oracle/bf16x2_numerics.py; plain fp16 operands 1.9e-4, bf16 with these two
        # products 1.6e-4). The residual stream is a true fp16 pair (22 bits).
        # "fp16q4": fp16x2 with the second product of the mel gate and of the skip GEMM on the block-scaled fp4 matrix instruction where the launch
        # fills the chip (ss_gemm_bf16_gate128q / _tile256q; validated on hardware in round 5: 2.6e-5 vs the real reference at T = 5625 x 1000 steps);
        # oracle contract set_matmul_rounding("fp16q4")
        # "fp16sd" (round 6): fp16x2's data path with ONE fp16 weight term per element - half the matrix work and half the weight bytes - and the weight
        # rounding NOISE-SHAPED over the loop's network evaluations: evaluation j uses weight set j % N, the N sets being a first-order sigma-delta
        # sequence of fp16 roundings of the same weight (their sum is N w up to one rounding), so the rounding averages out over the steps instead
        # of adding up coherently: 2.2e-5 on the reference's 1000-step golden with N = 32 (plain one-product fp16: 1.94e-4; fp16x2: 1.9e-5;
        # oracle/dither_numerics.py, oracle contract set_matmul_rounding("fp16sd")). The f0 denoisers keep bf16x2 as in the other fp16 modes.
        self.sd = prec == "fp16sd"
        self.sd_sets = max(1, int(os.environ.get("SS_SD_SETS", hp.get("fp16sd_sets", 32)))) if self.sd else 0
        # the step-invariant conditioner addend of the fused layer launch as fp16 sigma-delta sets cycled over the evaluations (0 = the fp32 slab)
        self.sd_e_sets = min(64, max(0, int(os.environ.get("SS_SD_E_SETS", hp.get("fp16sd_e_sets", 8))))) if self.sd else 0
        self.q4 = prec == "fp16q4"
        self.f16 = prec in ("fp16x2", "fp16q4", "fp16sd")
        self.split = prec in ("bf16x2", "fp16x2", "fp16q4", "fp16sd")
        self.bf16 = prec in ("bf16", "bf16x2", "fp16x2", "fp16q4", "fp16sd")
        # opt-in "bf16x3": fp32 products of the F(4,3) gate from operands split into three bf16 terms on the bf16 matrix cores
        # (ss_wino43_gate16x; fp32-grade results, oracle/bf16x3_numerics.py); everything else as the fp32 mode
        self.x3 = prec == "bf16x3"
        # fold skip_projection / sqrt(L) into the skip-all weights (fp32 mode only: in bf16 mode the operand rounding of the
        # two separate GEMMs is part of the stated arithmetic)
        self.fold_skip = self.defer_skip and (not self.bf16 or self.split) and os.environ.get("SS_FOLD_SKIP", "1") not in ("0", "off", "false")
        # bf16 mode: hidden-layer weights AND activations as bf16 in HBM (ss_gemm_bf16; SS_BF16_HBM=0 keeps the round-1 form
        # that rounds fp32 operands inside the fp32 kernel's BF16 template mode); needs the deferred-skip layout
        self.bf16_hbm = self.bf16 and self.defer_skip and (self.split or os.environ.get("SS_BF16_HBM", "1") not in ("0", "off", "false"))
        if self.split and not (self.defer_skip and self.fold_skip):
            raise ValueError(f"mfma_precision={prec} needs the deferred, folded skip form (SS_DEFER_SKIP / SS_FOLD_SKIP left on)")
        if self.bf16:
            self.use_wino = False  # the transform would amplify the operand rounding; the matrix pipe is not the limit in bf16
        # diffusion plans (workspaces + captured hipGraphs) are keyed by (B, T bucket): frames are padded up to a multiple of
        # `t_bucket` (padding = mel2ph 0, masked everywhere, so the valid frames are unchanged) and the cache is an LRU bounded
        # by bytes; in "auto" mode a shape is captured on its SECOND use (the first use of a shape runs eagerly: capture costs
        # a warm-up pass + ~13k recorded launches, which a one-off shape never earns back).
        self.t_bucket = max(1, int(os.environ.get("SS_T_BUCKET", hp.get("t_bucket", 64))))
        self.plan_bytes = int(float(os.environ.get("SS_PLAN_GIB", "24")) * 2 ** 30)
        self._plans = collections.OrderedDict()
        self.n_captures = 0
        self.plan_lookups = self.plan_misses = self.plan_evictions = 0

    # ---- state_dict contract ------------------------------------------------------------------
    @staticmethod
    def _mangle(name):
        return "p__" + name.replace(".", "__")

    def state_dict(self, *args, **kwargs):
        return {n: getattr(self, self._mangle(n)) for n in self._names}

    def load_state_dict(self, state_dict, strict=True):
        missing = [n for n in self._names if n not in state_dict]
        unexpected = [k for k in state_dict if k not in set(self._names)]
        if strict and (missing or unexpected):
            raise RuntimeError(f"StyleSingerHIP.load_state_dict: missing={missing[:5]} unexpected={unexpected[:5]}")
        with torch.no_grad():
            for n in self._names:
                if n in state_dict:
                    dst = getattr(self, self._mangle(n))
                    src = state_dict[n]
                    if tuple(src.shape) != tuple(dst.shape):
                        raise RuntimeError(f"size mismatch for {n}: {tuple(src.shape)} vs {tuple(dst.shape)}")
                    dst.copy_(src)
        self._weights_version += 1
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def p(self, name):
        return getattr(self, self._mangle(name))

    def train(self, mode=True):
        if mode:
            raise RuntimeError("StyleSingerHIP is an inference-only drop-in (training is out of scope, SURVEY.md §8)")
        return super().train(False)

    def _pos(self, n, dev):
        if self._pos_table is None or self._pos_table.shape[0] < n:
            # a blocking host->device copy (pageable source): complete on return, whichever stream built it, so forwards running
            # on other streams may read it without an event. A table that is being REPLACED may still be read by a forward in flight
            # on another stream: keep the old one alive until the device is idle.
            old = self._pos_table
            self._pos_table = _sin_table(max(n, 2048), self.hp["hidden_size"]).to(dev)
            if old is not None and old.is_cuda:
                torch.cuda.synchronize(dev)
        return self._pos_table

    def warm_caches(self, max_frames, device):
        """Build the lazily created shared state (packed weights, sinusoidal table) BEFORE forwards fork onto side streams."""
        self._ensure_packed()
        self._pos(int(max_frames) + 2, torch.device(device))

    # ---- op helpers -----------------------------------------------------------------------------
    def _gemm(self, x, pk, out, B, T, *, taps=None, lens=None, act=L.ACT_NONE, pre_scale=1.0, R=None, mask_rows=True,
              N=None, **kw):
        if taps is None:
            taps = [(j - (pk.k - 1) // 2) for j in range(pk.k)]
        N = pk.Cout if N is None else N
        L.conv_gemm(x, pk.W, out, B=B, T=T, Cin=pk.Cin, N=N, Np=pk.Np, Kp=pk.Kp, taps=taps, lens=lens, bias=pk.bias,
                    act=act, pre_scale=pre_scale, R=R, ldr=(N if R is not None else 0), mask_rows=mask_rows, **kw)
        return out

    def _fft_blocks(self, pkb, x, B, T, lens, ffn_wino=False):
        """4 x EncSALayer + final LN (tts_modules.py:281-306, common_layers.py:649-673), in place on x [B,T,H].
        ffn_wino: the first FFN conv as grouped Winograd F(4,3) where a pack exists (fp32 mode). The frame-level decoder asks for it; the
        phoneme-level encoder (~28 rows against the kernel's 256-frame tile) stays on the direct kernel for that geometric reason, not a
        measured one. The choice is per stack, never per T: a forward padded to its frame bucket must equal the unpadded one bit for bit."""
        H = self.hp["hidden_size"]
        nh = self.hp["num_heads"]
        D = H // nh
        dev = x.device
        h = torch.empty(B, T, H, device=dev)
        qkv = torch.empty(B, T, 3 * H, device=dev)
        att = torch.zeros(B, T, H, device=dev)
        ff = torch.empty(B, T, 4 * H, device=dev)
        for ly in pkb["layers"]:
            L.layernorm(x, *ly["ln1"], B=B, T=T, C_=H, out=h)
            self._gemm(h, ly["qkv"], qkv, B, T, lens=lens, mask_rows=False)
            L.attention(qkv, qkv[:, :, H:], qkv[:, :, 2 * H:], att, B=B, H=nh, D=D, Tq=T, Tk=T, ldq=3 * H, ldk=3 * H, ldv=3 * H,
                        ldo=H, q_bs=T * 3 * H, k_bs=T * 3 * H, v_bs=T * 3 * H, o_bs=T * H, qlens=lens, klens=lens, scale=D ** -0.5)
            self._gemm(att, ly["out"], x, B, T, lens=lens, R=x)
            L.layernorm(x, *ly["ln2"], B=B, T=T, C_=H, out=h)
            f1 = ly["ffn1"]
            if ffn_wino and f1.W43 is not None:
                L.wino43_conv(h, f1.W43, ff, k=f1.k, dilation=1, B=B, T=T, Cin=f1.Cin, N=f1.Cout, Np=f1.Np, Kp=f1.Kp, lens=lens, bias=f1.bias,
                              act=L.ACT_GELU, pre_scale=f1.k ** -0.5, mask_rows=False)
            else:
                self._gemm(h, f1, ff, B, T, lens=lens, act=L.ACT_GELU, pre_scale=f1.k ** -0.5, mask_rows=False)
            self._gemm(ff, ly["ffn2"], x, B, T, lens=lens, R=x)
        L.layernorm(x, *pkb["ln"], B=B, T=T, C_=H, out=x, lens=lens, mask_rows=True)
        return x

    @torch.no_grad()
    def mel_stage(self, coarse_mel, cond, lens=None, z_q=None, z_steps=None, sampler="ddpm", ddim_steps=None, plms_interval=None, seed=1234,
                  eta=0.0, mel_steps=None, mel_order=None, mel_spacing=None):
        """The shallow mel diffusion alone (a11 output -> a12): coarse mel [B,T,80] + condition [B,T,256] -> mel [B,T,80].
        z_q [B,1,80,T] / z_steps [K,B,1,80,T]: optional recorded noise (reference layout); default device Philox.
        `sampler` and its arguments as in forward ("dpmpp": mel_steps, mel_order, mel_spacing; runs eagerly); the hparams defaults are not read."""
        sm = self._mel_sampler_args(dict(sampler=sampler, ddim_steps=ddim_steps, plms_interval=plms_interval, eta=eta, mel_steps=mel_steps,
                                         mel_order=mel_order, mel_spacing=mel_spacing), use_hparams=False)
        self._ensure_packed()
        pk, hp = self._pk, self.hp
        dev = coarse_mel.device
        B, T, M = coarse_mel.shape
        K = hp["K_step"]
        pl = self._plan(B, T, dev)
        pl.lens.copy_(lens if lens is not None else torch.full((B,), T, device=dev, dtype=torch.int32))
        pl.seed.fill_(seed)
        pl.cond_mel.copy_(cond)
        pl.coarse_mel.copy_(coarse_mel)
        zq_n = None if z_q is None else _noise_btm(z_q, dev, (B, M, T), T)
        zs_n = None if z_steps is None else _noise_btm(z_steps, dev, (K, B, M, T), T)
        ts = self.mel_timesteps(sm.steps, sm.spacing) if sm.steps is not None else None
        self._run_mel(pl, (zq_n, zs_n), ddim_ts=ts if sm.name == "ddim" else None, plms_interval=sm.interval, eta=sm.eta,
                      dpmpp=(ts, sm.order) if sm.name == "dpmpp" else None)
        mel_out = torch.empty(B, T, M, device=dev, dtype=torch.float32)
        L.ops.ss_mel_denorm(pl.xm, pk["spec_min"], pk["spec_max"], mel_out, B, T, M, pl.lens, None)
        return mel_out

    # ---- forward ----------------------------------------------------------------------------------
    @torch.no_grad()
    def encode_style(self, ref_mels, ref_f0):
        """Residual Style Adaptor + RQ lookup + `l1` (a5, a6 and the first line of a7; lse.py:103-129, RQ.py:226-270,
        stylesinger.py:189-196) for a batch of references. The result depends on the reference only, so a style-transfer
        sweep (BASELINE config 5) computes it once per reference and passes it to forward(style_cache=...)."""
        self._ensure_packed()
        hp, pk = self.hp, self._pk
        H = hp["hidden_size"]
        dev = ref_mels.device
        B = ref_mels.shape[0]
        f32 = dict(device=dev, dtype=torch.float32)
        ref_mels = ref_mels.contiguous().float()
        Tr = ref_mels.shape[1]
        if ref_f0.dim() == 1:
            ref_f0 = ref_f0[None]
        ref_f0 = ref_f0.contiguous().float()
        lens_r = torch.empty(B, device=dev, dtype=torch.int32)
        L.ops.ss_ref_lens(ref_mels, B, Tr, 80, lens_r)
        xr = ref_mels.clone()
        acts = torch.empty(B, Tr, 80, **f32)
        wn_out = torch.zeros(B, Tr, 80, **f32)
        for i, w in enumerate(pk["wn"]):
            inl = w["inl"]
            L.conv_gemm(xr, inl.W, acts, B=B, T=Tr, Cin=80, N=80, Np=inl.Np, Kp=inl.Kp, taps=(-1, 0, 1), lens=lens_r,
                        epi=L.EPI_GATE, gate_mode=1, bias=inl.bias, ldc=80, mask_rows=False)
            if w["res"] is not None:
                self._gemm(acts, w["res"], xr, B, Tr, lens=lens_r, R=xr)
            self._gemm(acts, w["skip"], wn_out, B, Tr, lens=lens_r, accumulate=True)
        L.ops.ss_add_rowscalar(wn_out, ref_f0, B, Tr, 80, lens_r)
        h80 = torch.empty(B, Tr, 80, **f32)
        h160 = torch.empty(B, Tr, 160, **f32)
        for blk in pk["cb"]:
            L.layernorm(wn_out, *blk["ln"], B=B, T=Tr, C_=80, out=h80)
            self._gemm(h80, blk["c1"], h160, B, Tr, lens=lens_r, act=L.ACT_GELU, pre_scale=blk["c1"].k ** -0.5, mask_rows=False)
            self._gemm(h160, blk["c2"], wn_out, B, Tr, lens=lens_r, R=wn_out)
        L.layernorm(wn_out, *pk["cb_ln"], B=B, T=Tr, C_=80, out=h80, lens=lens_r, mask_rows=True)
        pre_rq = torch.empty(B, Tr, H, **f32)
        self._gemm(h80, pk["cb_post"], pre_rq, B, Tr, lens=lens_r)
        zq = torch.empty(B, Tr, H, **f32)
        codes = torch.empty(B, Tr, hp["rq_depth"], device=dev, dtype=torch.int64)
        L.ops.ss_rq_lookup(pre_rq, pk["codebooks"], zq, codes, B * Tr, H, hp["nRQ"], hp["rq_depth"])
        cat = torch.empty(B, Tr, 2 * H, **f32)
        cat[:, :, :H].copy_(zq)
        pos_r = torch.empty(B, Tr, device=dev, dtype=torch.int32)
        tabr = self._pos(Tr + 2, dev)
        L.ops.ss_make_positions(None, zq, H, Tr * H, pos_r, B, Tr)
        L.ops.ss_table_add(pos_r, tabr, tabr.shape[0], L.ptr(cat) + 4 * H, 2 * H, Tr * 2 * H, B, Tr, H, None, 1.0, 0)
        sty = torch.empty(B, Tr, H, **f32)
        self._gemm(cat, pk["l1"], sty, B, Tr, mask_rows=False)
        return dict(sty=sty, lens_r=lens_r, ref_f0=ref_f0, style_pre_rq=pre_rq, rq_codes=codes, style_rq=zq)

    @torch.no_grad()
    def encode_style_blend(self, ref_mels, ref_f0, ref_weights=None):
        """The style of a POOL of R references per item, weighted: ref_mels [B, R, Tr, 80], ref_f0 [B, R, Tr], ref_weights None (equal), a length-R
        sequence or [B, R] host values (`resolve_ref_weights`: w >= 0, normalised per item). Every reference is encoded on its own by
        `encode_style` (one pass over the flat [B * R] batch; positions restart per reference), its frame axis zero-padded to Ts, a multiple of
        the attention's 32-key tile. The result is a style cache for forward(style_cache=...) whose tensors all lead with B: `sty` [B, R * Ts, H]
        with reference r in rows [r * Ts, r * Ts + seg_lens[b, r]), `seg_lens` int32 [B, R], `seg_logw` fp32 [B, R] = log of the normalised
        weight (-inf = weight 0), and `ref_f0`, `style_pre_rq`, `rq_codes`, `style_rq` as [B, R * Ts, ...]. The style-to-content attention then
        runs over all references at once with seg_logw added to the scores (`ss_attention_seg`): the weights are PRIORS on the attention over the
        pooled frames - equal weights = the clips concatenated, (1, 0) = the first clip alone - not a linear mix of outputs. The speaker and
        emotion embeddings are blended separately (`blend_embeds`); how a checkpoint renders blended embeddings is unassessed."""
        if ref_mels.dim() != 4 or ref_f0.dim() != 3 or tuple(ref_f0.shape) != tuple(ref_mels.shape[:3]):
            raise ValueError(f"encode_style_blend: ref_mels {tuple(ref_mels.shape)} / ref_f0 {tuple(ref_f0.shape)}: expected [B, R, Tr, 80] and [B, R, Tr]")
        B, R, Tr, M = ref_mels.shape
        logw, _p = resolve_ref_weights(ref_weights, B, R)
        Ts = (Tr + 31) // 32 * 32
        sc = self.encode_style(_pad_frames(ref_mels.float(), Ts, dim=2).reshape(B * R, Ts, M), _pad_frames(ref_f0.float(), Ts).reshape(B * R, Ts))
        out = {k: sc[k].reshape(B, R * Ts, *sc[k].shape[2:]) for k in ("sty", "ref_f0", "style_pre_rq", "rq_codes", "style_rq")}
        out["seg_lens"] = sc["lens_r"].reshape(B, R)
        out["seg_logw"] = torch.from_numpy(logw).to(ref_mels.device)
        return out

    @torch.no_grad()
    def forward(self, txt_tokens, mel2ph=None, spk_embed=None, emo_embed=None, ref_mels=None, ref_f0=None, f0=None, uv=None,
                skip_decoder=False, global_steps=0, infer=False, note=None, note_dur=None, note_type=None, **kwargs):
        """Mirror of StyleSinger.forward (modules/StyleSinger/stylesinger.py:119-187), inference branch only.

        Extra keyword arguments: `noise` (dict from synth.draw_acoustic_noise: a recorded noise tape for
        parity tests; default = on-device Philox), `seed` (Philox seed), `sampler="ddim", ddim_steps=n, eta=0.0` (strided
        DDIM mel sampler, BASELINE config 5; eta = 0 deterministic, eta = 1 with ddim_steps = K_step IS the reference's ancestral
        sampler; default = the reference's 100-step ancestral sampler),
        `sampler="dpmpp", mel_steps=n, mel_order=2, mel_spacing="logsnr"|"uniform"` (DPM-Solver++ multistep, data prediction, over at most n
        network times - `ss_meldiff_sample_dpmpp`: order 2 = "2M" with a first-order first and last transition, order 1 = DDIM with eta = 0 bit
        for bit; deterministic after q_sample; "logsnr" spaces the times uniformly in the half log-SNR (`plans.logsnr_timesteps`: the list may be
        shorter than n) and is this sampler's default, `sampler="ddim"` honours `mel_spacing` too and defaults to "uniform"; `mel_steps` is
        also read by "ddim" where `ddim_steps` is absent). Without `sampler` the hparams decide: `mel_sampler` / `mel_sample_steps` /
        `mel_sample_order` / `mel_sample_spacing` / `mel_sample_eta`, then `pndm_speedup`, then the reference's loop.
        `ret["mel_sampler"]` = dict(name, ts, order) names the list whenever a strided sampler ran. What a checkpoint renders at a given n is
        unassessed,
        `f0_steps=n, f0_eta=1.0` (strided sampler of the two f0 / uv diffusions: n of the f0_timesteps network times, `ss_f0diff_sample_strided`;
        f0_eta = 0 deterministic Gaussian half ... 1 ancestral, n = f0_timesteps with f0_eta = 1 IS the reference's loop to fp32 rounding of the
        coefficients; defaults hparams['f0_sample_steps'] = None - the reference's full loop, unchanged - and hparams['f0_sample_eta']),
        `sampler="plms", plms_interval=n` (the reference's PLMS sampler, hparams['pndm_speedup'],
        shallow_diffusion_tts.py:165-197), `plan_slot` (workspace/graph set to use: give concurrent forwards on different streams
        different slots), `style_cache` (the dict encode_style() returned for these references: skips
        the style encoder).

        Several references per item: `ref_mels` [B, R, Tr, 80] with `ref_f0` [B, R, Tr] (+ `ref_weights`: None = equal, a length-R sequence or
        [B, R] host values >= 0) is a weighted pool - `encode_style_blend` encodes every reference on its own and the style-to-content attention
        runs over all of them at once with log(weight) added to the scores (`ss_attention_seg`): priors on the attention, not a linear mix of
        outputs. A `style_cache` from `encode_style_blend` does the same without the encoder. `spk_embed` / `emo_embed` stay [B, 256]: blend
        them with `blend_embeds` (unassessed on a checkpoint). 3-D `ref_mels` behave exactly as before.

        Pitch control (infer=True only): sing on a GIVEN f0 contour instead of the two f0 diffusions' output. Two forms:
          * `f0=, uv=` [B, T_out] - the reference's own form (hparams['use_gt_f0'], tasks/StyleSinger/stylesinger.py:176-188): what
            sample['f0'] / sample['uv'] hold, i.e. `norm_interp_f0` output (log2 Hz interpolated through unvoiced frames; uv > 0 = unvoiced,
            any dtype). T_out = mel2ph.shape[1] when mel2ph is given, else the predicted frame count; another length is a ValueError.
          * `pitch_hz=(contour_hz [B, Lc], lens_c)` (+ `pitch_shift=<semitones>`): a contour in Hz (0 = unvoiced) on a frame grid of its own,
            fitted on the device to each item's frame count once that is known (`ss_contour_fit`, pitch.contour_fit), normalised with
            `norm_interp_f0_device`, then used as above. An item whose fitted contour has no voiced frame is sung unvoiced, as
            `norm_interp_f0` treats an all-unvoiced contour (f0 = 0, uv = 1 on every frame).
            `pitch_align="dtw"` (+ `pitch_align_band=<guide frames | None = full>`): the contour is a guide with a timing of its own (a sung take).
            In place of the linear fit it is warped onto the score's per-frame notes by dynamic time warping (`ss_contour_align`,
            pitch.contour_align: cents distance, band around the linear fit's diagonal; `pitch_shift` puts the guide into the score's key BEFORE the
            comparison). `ret` gains `pitch_align_idx` [B, T] (guide frame per score frame, -1 beyond the item), `pitch_align_cost` [B] and
            `pitch_align_status` [B] (1 = the item was not aligned and got the linear fit: more than `band` guide frames per score frame) as
            device tensors, no sync. Default `None`: the linear fit, exactly as before.
            `pitch_timing="guide"`: sing in the GUIDE's timing instead of the score's. The contour is taken to be on the model's frame grid (hop_size /
            audio_sample_rate: what tracking `pitch_audio` gives; a contour on another grid must be resampled by the caller). Once the score's mel2ph
            exists (predicted durations or a given `mel2ph`) the guide is aligned to it as above (`pitch_align` may be omitted or "dtw";
            `pitch_align_band` and `pitch_shift` apply to the alignment), and `ss_retime_mel2ph` (pitch.retime_to_guide) lays the phones out on the
            guide's frames: note onsets where the guide has them, the phones inside a note in their proportions. The call then continues as if the
            caller had passed that mel2ph: T_out = Lc (the render lines up with the take frame for frame), and the contour is used one-to-one.
            `ret['mel2ph']` is the retimed one; `ret` gains `mel2ph_score`, `pitch_retime_src` [B, Lc] (score frame under every guide frame, -1
            beyond the item), `pitch_retime_status` [B] (1 = not retimed, the linear stretch: the alignment refused the item, or the guide has fewer
            frames than the score has pitch changes) and `pitch_align_idx` / `_cost` / `_status` on the SCORE's frame axis. The alignment is
            pitch-only: it carries no timing information inside a held note or between repeated equal notes, where the phones are spread linearly.
            Default `None`: the paths above, bit for bit.
        Both skip `ss_f0_bounds` and the f0 pair loop (and its hipGraph) and run `ss_pitch_given` in place of `ss_pitch_post`; everything from
        `pitch_embed` on is unchanged, and the mel loop draws the same noise as a predicted-f0 forward with the same `seed`. `ret` carries
        `pitch_pred`, `f0_denorm`, `f0_denorm_pred` (= `f0_denorm`, as stylesinger.py:241 yields for a given contour) and `pitch_coarse`, and
        no `f0_a` / `uv_a` / `f0_b` / `uv_b`. The note-rest rule (uv[midi == 0] = 1) belongs to the predicted branch and is not applied. The
        reference's `mdiff*` / `gdiff*` / `nll*` on this branch are training losses of the f0 nets (:305-307): they are not produced. A
        recorded `noise` dict needs no `f0_a` / `f0_b` entries in these forms.

        Pitch expression controls, in every branch above (predicted, `f0=` / `uv=`, `pitch_hz` fitted, aligned or in the guide's timing):
        `pitch_correct=a` in [0, 1] pulls the pitch trend toward the score's notes, `vibrato_scale=k` >= 0 scales what rides on the trend (0 = flat,
        1 = as sung), `vibrato_add=(rate_hz, depth_cents[, delay_ms = 250[, fade_ms = 150]])` puts a synthetic vibrato on held notes long enough for
        delay + two fades, `pitch_smooth_ms` (default 333) is the length of the Hann window that defines the trend (pitch.pitch_edit: this project's own
        definition). Defaults: hparams of the same names; an explicit value wins over hparams, hparams over neutral. The edit sits between the pitch
        tail and `pitch_embed` (`ss_pitch_edit_runs` + `ss_pitch_edit`, then `ss_pitch_given` on the edited contour with the merged voicing), so the
        decoder, the mel diffusion and the vocoder's source all see the edited contour. `ret` gains `pitch_pred_raw` / `f0_denorm_raw` (the
        unedited ones) and `pitch_edit` [B, 6] float64 (voiced sung frames; rms of the vibrato in cents; mean and mean absolute distance of the trend
        from the notes; largest change in cents; frames carrying synthetic vibrato). No host sync. Neutral or absent (0, 1, no vibrato_add or depth
        0): no launch, no allocation, no new keys, the bits as before.
        `pitch_correct=1, vibrato_scale=0` is the hard-tuned effect by construction; what a checkpoint renders from an edited contour is unassessed.

        Which combinations and values of these controls are refused (ValueError, before anything is launched): `controls.py`."""
        if not infer:
            raise NotImplementedError("StyleSingerHIP implements the inference path only (infer=True)")
        ctl = controls.resolve(kwargs, self.hp, self.f0_strided_timesteps, f0, uv, ref_mels, ref_f0)   # refusals here, before anything is launched
        if ctl.ref_weights is not None:
            resolve_ref_weights(ctl.ref_weights, ref_mels.shape[0], ref_mels.shape[1])
        self._ensure_packed()
        # c: the per-call state the stages share (shapes, lengths, intermediate activations, the plan) and the result dict
        c = types.SimpleNamespace(ret={}, dev=txt_tokens.device, ctl=ctl, midi=None)
        c.f32 = dict(device=c.dev, dtype=torch.float32)
        self._encode_text(c, txt_tokens, note, note_dur, note_type, spk_embed, emo_embed)
        self._regulate_length(c, mel2ph, f0, uv)
        self._align_style(c, ref_mels, ref_f0)
        self._pitch(c, f0, uv)
        if not skip_decoder:
            if self.prodiff:
                self._decode_prodiff(c)
            else:
                self._decode_fft(c)
                if global_steps > self.hp["diff_start"]:
                    self._refine_mel(c)
                else:
                    c.ret["mel_out"] = c.coarse_mel
        ret = self._crop_frames(c.ret, c.T, c.T_out)
        ret.update(c.score_axis)
        return ret

    def _f0_sampler_args(self, kwargs, contour_given):
        return controls.f0_sampler(kwargs, self.hp, contour_given, self.f0_strided_timesteps)

    def _mel_sampler_args(self, kwargs, use_hparams=True):
        return controls.mel_sampler(kwargs, self.hp, use_hparams)

    def mel_timesteps(self, n, spacing="uniform"):
        """n network times of the shallow mel loop, K_step-1 ... 0: "uniform" in t (`ddim_timesteps`) or "logsnr" (`plans.logsnr_timesteps` over
        the checkpoint's float64 schedule; the list may come out shorter than n). Needs the packed schedule for "logsnr"."""
        if spacing == "uniform":
            return self.ddim_timesteps(n)
        self._ensure_packed()
        return logsnr_timesteps(self._pk["mel"]["sched"]["alphas_cumprod_f64"], self.hp["K_step"], n)

    def _encode_text(self, c, txt_tokens, note, note_dur, note_type, spk_embed, emo_embed):
        """Phoneme encoder (a1) + note encoder (a2) + speaker / emotion projections -> c.enc [B,Tp,H], c.spk, c.emo [B,H]."""
        hp, pk, ret = self.hp, self._pk, c.ret
        H, dev, f32 = hp["hidden_size"], c.dev, c.f32
        B, Tp = c.B, c.Tp = txt_tokens.shape
        c.txt_tokens = txt_tokens = txt_tokens.contiguous()
        c.lens_p = lens_p = torch.empty(B, device=dev, dtype=torch.int32)
        L.ops.ss_count_nonzero_i64(txt_tokens, lens_p, B, Tp)
        x = torch.empty(B, Tp, H, **f32)
        pos_p = torch.empty(B, Tp, device=dev, dtype=torch.int32)
        tab = self._pos(max(Tp, 8) + 2, dev)
        L.ops.ss_embedding(txt_tokens, self.p("encoder.embed_tokens.weight"), x, B * Tp, H, hp["vocab_size"], math.sqrt(H), 0)
        L.ops.ss_make_positions(txt_tokens, None, 0, 0, pos_p, B, Tp)
        L.ops.ss_table_add(pos_p, tab, tab.shape[0], x, H, Tp * H, B, Tp, H, None, 1.0, 1)
        L.ops.ss_add_bcast_mask(x, None, None, None, None, x, B, Tp, H, lens_p)
        c.enc = enc = self._fft_blocks(pk["enc"], x, B, Tp, lens_p)
        ret["encoder_out_text"] = enc.clone()
        note_out = torch.empty(B, Tp, H, **f32)
        c.note = note = note.contiguous()
        note_type, note_dur = note_type.contiguous(), note_dur.contiguous().float()
        L.ops.ss_embedding(note, self.p("note_encoder.emb.weight"), note_out, B * Tp, H, 100, math.sqrt(H), 0)
        L.ops.ss_note_dur_add(note_dur, self.p("note_encoder.dur_ln.weight").reshape(-1).contiguous(), self.p("note_encoder.dur_ln.bias"), note_out,
                              B * Tp, H)
        L.ops.ss_embedding(note_type, self.p("note_encoder.type_emb.weight"), note_out, B * Tp, H, 5, math.sqrt(H), 1)
        L.ops.ss_add_bcast_mask(enc, None, note_out, None, None, enc, B, Tp, H, None)
        c.spk = spk = torch.empty(B, H, **f32)
        c.emo = emo = torch.empty(B, H, **f32)
        self._gemm(spk_embed.contiguous().float(), pk["spk"], spk, 1, B, mask_rows=False)
        self._gemm(emo_embed.contiguous().float(), pk["emo"], emo, 1, B, mask_rows=False)
        ret["spk_embed"], ret["emo_embed"] = spk[:, None, :], emo[:, None, :]

    def _regulate_length(self, c, mel2ph, f0, uv):
        """Duration predictor + length regulator (a3) -> c.mel2ph [B,T], c.T (bucket), c.T_out (the caller's frames), c.lens_t, c.dec [B,T,H]."""
        pk, ret = self._pk, c.ret
        H, dev, f32 = self.hp["hidden_size"], c.dev, c.f32
        B, Tp, enc, lens_p, txt_tokens = c.B, c.Tp, c.enc, c.lens_p, c.txt_tokens
        dur_inp = torch.empty(B, Tp, H, **f32)
        L.ops.ss_add_bcast_mask(enc, c.spk, None, c.emo, None, dur_inp, B, Tp, H, lens_p)
        hbuf = torch.empty(B, Tp, H, **f32)
        cur = dur_inp
        for lyr in pk["dur"]:
            self._gemm(cur, lyr["conv"], hbuf, B, Tp, lens=lens_p, act=L.ACT_RELU, mask_rows=False)
            cur = L.layernorm(hbuf, *lyr["ln"], B=B, T=Tp, C_=H, out=torch.empty_like(hbuf), lens=lens_p, mask_rows=True)
        logdur = torch.empty(B, Tp, 4, **f32)
        L.conv_gemm(cur, pk["dur_lin"].W, logdur, B=B, T=Tp, Cin=H, N=1, Np=pk["dur_lin"].Np, Kp=pk["dur_lin"].Kp, lens=lens_p,
                    bias=pk["dur_lin"].bias, ldc=4, mask_rows=True)
        logdur = logdur[:, :, 0].contiguous()
        c.lens_t = lens_t = torch.empty(B, device=dev, dtype=torch.int32)
        if mel2ph is None:
            dur = torch.empty(B, Tp, device=dev, dtype=torch.int64)
            L.ops.ss_length_regulate(logdur, txt_tokens, dur, None, lens_t, B, Tp, 0)
            T = int(lens_t.max().item())  # host sync: the frame count is data dependent
            if T <= 0:
                raise L.StyleSingerHipError("predicted durations are all zero")
            mel2ph = torch.empty(B, T, device=dev, dtype=torch.int64)
            L.ops.ss_length_regulate(logdur, txt_tokens, dur, mel2ph, lens_t, B, Tp, T)
            ret["dur"], ret["dur_choice"] = logdur[:, :, None], dur
        else:
            mel2ph = mel2ph.contiguous()
            T = mel2ph.shape[1]
            ret["dur"] = logdur
        c.score_axis = {}   # results that stay on the score's frame axis when the render does not (pitch_timing="guide")
        if c.ctl.timing is not None:
            mel2ph, T = self._retime_to_guide(c, mel2ph, T)   # from here on as if the caller had passed this mel2ph: T = the contour's width
        # hipGraph bucket: run the frame axis padded to a multiple of t_bucket (padding = mel2ph 0 -> masked like any
        # batch padding); the plan/graph cache is then keyed by the bucket and every frame-level output is cropped back.
        c.T_out = T_out = T
        if f0 is not None and (tuple(f0.shape) != (B, T_out) or tuple(uv.shape) != (B, T_out)):
            raise ValueError(f"forward: f0 {tuple(f0.shape)} / uv {tuple(uv.shape)} given for {T_out} frames "
                             f"({'mel2ph' if 'dur_choice' not in ret else 'predicted durations'}): expected [{B}, {T_out}]")
        c.T = T = self.bucket_frames(T_out)
        if T != T_out:
            mel2ph = _pad_frames(mel2ph, T).contiguous()
        L.ops.ss_count_nonzero_i64(mel2ph, lens_t, B, T)
        ret["mel2ph"] = c.mel2ph = mel2ph
        c.dec = torch.empty(B, T, H, **f32)
        L.ops.ss_gather_expand(enc, mel2ph, c.dec, B, Tp, T, H)
        # UMLN (a4): DistributionUncertainty returns x unchanged when not training (umln.py:48-50)

    def _retime_to_guide(self, c, mel2ph, T):
        """pitch_timing="guide": the score's mel2ph [B, T] laid out on the guide contour's frame axis -> (mel2ph' [B, Lc], Lc). The guide is aligned to
        the score's note per frame (ss_contour_align, with pitch_align_band / pitch_shift as for pitch_align="dtw"), then ss_retime_mel2ph puts the
        note onsets where the guide has them (pitch.retime_to_guide). Lengths stay on the device; Lc is the contour's shape: no host sync."""
        from .pitch import contour_align_device, retime_device
        hz, lens_c = c.ctl.pitch_hz
        B, dev = c.B, c.dev
        if hz.dim() != 2 or hz.shape[0] != B:
            raise ValueError(f"forward: pitch_hz contour {tuple(hz.shape)} for a batch of {B}: expected [{B}, Lc]")
        hz, Lc = hz.to(dev), hz.shape[1]
        shift = c.ctl.pitch_shift
        L.ops.ss_count_nonzero_i64(mel2ph, c.lens_t, B, T)
        midi = torch.empty(B, T, device=dev, dtype=torch.int64)
        L.ops.ss_gather_expand_i64(c.note, mel2ph, midi, B, c.Tp, T)
        _, a_idx, a_cost, a_status = contour_align_device(hz, lens_c, midi, c.lens_t, T, band=c.ctl.align_band,
                                                          shift=0.0 if shift is None else float(shift))
        out, src, status, _ = retime_device(mel2ph, c.lens_t, midi, a_idx, a_status, lens_c, Lc)
        c.score_axis = dict(mel2ph_score=mel2ph, pitch_align_idx=a_idx, pitch_align_cost=a_cost, pitch_align_status=a_status)
        c.ret["pitch_retime_src"], c.ret["pitch_retime_status"] = src, status
        return out, Lc

    def _align_style(self, c, ref_mels, ref_f0):
        """Residual Style Adaptor (a5,a6; encode_style, or the caller's style_cache) + style-to-content attention (a7) -> c.style [B,T,H]."""
        pk, ret, f32 = self._pk, c.ret, c.f32
        B, T, H = c.B, c.T, self.hp["hidden_size"]
        sc = c.ctl.style_cache
        if sc is None:
            if ref_mels.dim() == 4:   # a pool of references per item (checked by forward): the weighted blend
                sc = self.encode_style_blend(ref_mels, ref_f0, c.ctl.ref_weights)
            else:
                sc = self.encode_style(ref_mels, ref_f0)
        seg_lens = sc.get("seg_lens")   # a blend cache (encode_style_blend): R segments of Ts key rows, one ss_attention_seg launch per layer
        sty, lens_r, Tr = sc["sty"], sc.get("lens_r"), sc["sty"].shape[1]
        if seg_lens is not None:
            R = seg_lens.shape[1]
            if tuple(seg_lens.shape) != (B, R) or tuple(sc["seg_logw"].shape) != (B, R) or Tr % R or (Tr // R) % 32:
                raise ValueError(f"forward: style_cache of a blend: sty {tuple(sty.shape)}, seg_lens {tuple(seg_lens.shape)}, seg_logw "
                                 f"{tuple(sc['seg_logw'].shape)} for a batch of {B}: expected [B, R * Ts, H] with Ts a multiple of 32 and [B, R] twice")
            seg_lens, seg_logw = seg_lens.contiguous(), sc["seg_logw"].contiguous()
        ret["ref_f0"], ret["style_pre_rq"] = sc["ref_f0"], sc["style_pre_rq"]
        ret["rq_codes"], ret["style_rq"], ret["rq_loss"] = sc["rq_codes"], sc["style_rq"], 0.0
        xs = c.dec.clone()
        q = torch.empty(B, T, H, **f32)
        kv = torch.empty(B, Tr, 2 * H, **f32)
        att = torch.zeros(B, T, H, **f32)
        ffh = torch.empty(B, T, 2048, **f32)
        for al in pk["align"]:
            self._gemm(xs, al["q"], q, B, T, mask_rows=False)
            self._gemm(sty, al["kv"], kv, B, Tr, mask_rows=False)
            if seg_lens is not None:
                L.attention_seg(q, kv, kv[:, :, H:], att, B=B, H=2, D=H // 2, Tq=T, R=R, Ts=Tr // R, ldq=H, ldk=2 * H, ldv=2 * H, ldo=H,
                                q_bs=T * H, k_bs=Tr * 2 * H, v_bs=Tr * 2 * H, o_bs=T * H, qlens=None, seg_lens=seg_lens, seg_logw=seg_logw,
                                scale=(H // 2) ** -0.5)
            else:
                L.attention(q, kv, kv[:, :, H:], att, B=B, H=2, D=H // 2, Tq=T, Tk=Tr, ldq=H, ldk=2 * H, ldv=2 * H, ldo=H,
                            q_bs=T * H, k_bs=Tr * 2 * H, v_bs=Tr * 2 * H, o_bs=T * H, qlens=None, klens=lens_r, scale=(H // 2) ** -0.5)
            self._gemm(att, al["out"], xs, B, T, R=xs, mask_rows=False)
            L.layernorm(xs, *al["n1"], B=B, T=T, C_=H)
            self._gemm(xs, al["l1"], ffh, B, T, act=L.ACT_RELU, mask_rows=False)
            self._gemm(ffh, al["l2"], xs, B, T, R=xs, mask_rows=False)
            L.layernorm(xs, *al["n2"], B=B, T=T, C_=H)
        ret["style"] = c.style = xs
        ret["gloss"] = 0.0

    def _pitch(self, c, f0, uv):
        """Pitch: a given contour, or the two joint Gaussian/multinomial diffusions (a8) + post-processing (a9); then the pitch
        embedding and decoder_inp -> c.dec_inp [B,T,H]. Opens the call's diffusion plan (c.pl, c.graphs)."""
        ret = c.ret
        B, T, H, dev, f32 = c.B, c.T, self.hp["hidden_size"], c.dev, c.f32
        c.pl = pl = self._plan(B, T, dev, c.ctl.plan_slot)
        pl.uses += 1
        pl.lens2[:B].copy_(c.lens_t)
        pl.seed.fill_(c.ctl.seed)
        c.graphs = c.ctl.noise is None and self._want_graphs(pl)
        out = (torch.empty(B, T, 2, **f32), torch.empty(B, T, **f32), torch.empty(B, T, device=dev, dtype=torch.int64))
        if f0 is not None or c.ctl.pitch_hz is not None:
            self._pitch_given(c, f0, uv, out)
        else:
            self._pitch_predicted(c, out)
        if c.ctl.edit is not None:
            out = self._pitch_edit(c, out)
        pitch_pred, f0_denorm, coarse = out
        ret["pitch_pred"], ret["f0_denorm"], ret["f0_denorm_pred"] = pitch_pred, f0_denorm, f0_denorm
        ret["pitch_coarse"] = coarse
        pitch_emb = torch.empty(B, T, H, **f32)
        L.ops.ss_embedding(coarse, self.p("pitch_embed.weight"), pitch_emb, B * T, H, 300, 1.0, 0)
        c.dec_inp = dec_inp = torch.empty(B, T, H, **f32)
        L.ops.ss_add_bcast_mask(c.dec, c.spk, pitch_emb, c.emo, c.style, dec_inp, B, T, H, c.lens_t)
        ret["decoder_inp"] = dec_inp

    def _pitch_edit(self, c, out):
        """Pitch expression controls (pitch.pitch_edit; c.ctl.edit from controls.resolve_pitch_edit): the merged log2-f0 of either branch, corrected toward
        the score's note per frame / its vibrato scaled / a synthetic one added (ss_pitch_edit_runs + ss_pitch_edit), then the pitch tail again
        on the edited contour (ss_pitch_given: x/2 + x/2 is exact, the voicing is the merged one) -> the new (pitch_pred, f0_denorm, coarse). The
        unedited pair stays in ret as pitch_pred_raw / f0_denorm_raw, the statistics [B, 6] as pitch_edit. No host sync."""
        from .pitch import pitch_edit_device
        B, T, dev, pe = c.B, c.T, c.dev, c.ctl.edit
        raw_pred, raw_denorm, _ = out
        if c.midi is None:   # the branch did not build it (a given f0 / uv, the linear fit, the guide's timing: its midi is on the score's axis)
            c.midi = torch.empty(B, T, device=dev, dtype=torch.int64)
            L.ops.ss_gather_expand_i64(c.note, c.mel2ph, c.midi, B, c.Tp, T)
        f, u = raw_pred[:, :, 0].contiguous(), raw_pred[:, :, 1].contiguous()
        f_e, stats, _, _ = pitch_edit_device(f, u, c.midi, c.lens_t, pe["W"], pe["alpha"], pe["kappa"], pe["vibrato"], fps=pe["fps"])
        new = (torch.empty(B, T, 2, **c.f32), torch.empty(B, T, **c.f32), torch.empty(B, T, device=dev, dtype=torch.int64))
        L.ops.ss_pitch_given(f_e, u, c.mel2ph, *new, B * T)
        c.ret["pitch_pred_raw"], c.ret["f0_denorm_raw"], c.ret["pitch_edit"] = raw_pred, raw_denorm, stats
        return new

    def _pitch_given(self, c, f0, uv, out):
        """A given contour: no clamp bounds, no f0 pair loop (pl.graphs["f0"] stays untouched); the mel loop's Philox keys are per call site
        (constant + pl.seed) and its counters per (step, element), so it draws what a predicted-f0 forward with this seed draws."""
        B, T, T_out, dev, lens_t, pitch_hz = c.B, c.T, c.T_out, c.dev, c.lens_t, c.ctl.pitch_hz
        if pitch_hz is not None:
            from .pitch import contour_fit_device, norm_interp_f0_device
            if pitch_hz[0].dim() != 2 or pitch_hz[0].shape[0] != B:
                raise ValueError(f"forward: pitch_hz contour {tuple(pitch_hz[0].shape)} for a batch of {B}: expected [{B}, Lc]")
            shift = 0.0 if c.ctl.pitch_shift is None else float(c.ctl.pitch_shift)
            if c.ctl.align is None or c.ctl.timing is not None:   # retimed: the frames ARE the guide's, a 1:1 copy
                hz = contour_fit_device(pitch_hz[0].to(dev), pitch_hz[1], lens_t, T, shift)
            else:   # "dtw": warp the guide onto the score's note per frame (the midi of _pitch_predicted)
                from .pitch import contour_align_device
                c.midi = midi = torch.empty(B, T, device=dev, dtype=torch.int64)
                L.ops.ss_gather_expand_i64(c.note, c.mel2ph, midi, B, c.Tp, T)
                hz, a_idx, a_cost, a_status = contour_align_device(pitch_hz[0].to(dev), pitch_hz[1], midi, lens_t, T,
                                                                   band=c.ctl.align_band, shift=shift)
                c.ret["pitch_align_idx"], c.ret["pitch_align_cost"], c.ret["pitch_align_status"] = a_idx, a_cost, a_status
            f0_g, uv_g = norm_interp_f0_device(hz, lens_t, self.hp)   # frames >= lens_t[b]: f0 = 0, uv = 0 - masked by mel2ph == 0 below
        else:  # bucket padding: f0 = 0, uv = 1 (mel2ph is 0 there anyway)
            f0_g = _pad_frames(f0.to(dev).float(), T).contiguous()
            uv_g = uv.to(dev).float()
            uv_g = uv_g.contiguous() if T == T_out else torch.nn.functional.pad(uv_g, (0, T - T_out), value=1.0)
        pitch_pred, f0_denorm, coarse = out
        L.ops.ss_pitch_given(f0_g, uv_g, c.mel2ph, pitch_pred, f0_denorm, coarse, B * T)

    def _pitch_predicted(self, c, out):
        """The f0 pair loop (a8: agnostic + specific denoiser, one grouped loop) and ss_pitch_post (a9)."""
        ret, pl = c.ret, c.pl
        B, T, Tp, H, dev, lens_t, mel2ph = c.B, c.T, c.Tp, self.hp["hidden_size"], c.dev, c.lens_t, c.mel2ph
        c.midi = midi = torch.empty(B, T, device=dev, dtype=torch.int64)
        L.ops.ss_gather_expand_i64(c.note, mel2ph, midi, B, Tp, T)
        pl.lens2[B:].copy_(lens_t)
        L.ops.ss_f0_bounds(midi, pl.lo2, pl.hi2, B * T)
        pl.lo2[B:].copy_(pl.lo2[:B])
        pl.hi2[B:].copy_(pl.hi2[:B])
        pl.cond_a.copy_(c.dec)  # = decoder_inp * tgt_nonpadding (the gather already wrote 0 on padding)
        L.ops.ss_add_bcast_mask(c.dec, c.spk, None, c.emo, c.style, pl.cond_b, B, T, H, lens_t)

        ts, eta = c.ctl.f0_ts, c.ctl.f0_eta   # None: the reference's full loop; else the strided sampler (its tapes: the same [S]... layout, row = network time)

        def run(noise=None):
            if noise is None:
                return self._run_f0_pair(pl, ts=ts, eta=eta)
            S = self._pk["f0_pair"]["net"].steps
            tape_t = lambda x: _pad_frames(x.to(dev).float(), T)  # recorded noise [..., T_out] (reference layout) -> device fp32, bucket-padded
            na, nb_ = noise["f0_a"], noise["f0_b"]
            pl.f0[0].copy_(tape_t(na["z0"]).reshape(B, T))
            pl.f0[1].copy_(tape_t(nb_["z0"]).reshape(B, T))
            zs = torch.cat([tape_t(na["z_steps"]).reshape(S, B, T), tape_t(nb_["z_steps"]).reshape(S, B, T)], 1).contiguous()
            us = torch.cat([tape_t(na["u_steps"]).reshape(S, B, 2, T), tape_t(nb_["u_steps"]).reshape(S, B, 2, T)], 1).contiguous()
            self._run_f0_pair(pl, (zs, us), ts=ts, eta=eta)
        # uv2 is reset outside the graph: before the capture (its warm-up and recording passes accumulate into it) and before every run.
        # One captured graph per sampler: "f0" = the default loop, ("f0", number of steps, eta) = a strided one
        self._run_loop(pl, "f0" if ts is None else ("f0", len(ts), eta), run, tape=c.ctl.noise, graphs=c.graphs, prepare=pl.uv2.zero_)
        f0_a, uv_a, f0_b, uv_b = pl.f0[0].clone(), pl.uv[0].clone(), pl.f0[1].clone(), pl.uv[1].clone()
        ret["gdiff1"] = ret["mdiff1"] = ret["gdiff2"] = ret["mdiff2"] = 0.0
        pitch_pred, f0_denorm, coarse = out
        L.ops.ss_pitch_post(f0_a, uv_a, f0_b, uv_b, midi, mel2ph, pitch_pred, f0_denorm, coarse, B * T)
        ret["f0_a"], ret["uv_a"], ret["f0_b"], ret["uv_b"] = f0_a, uv_a, f0_b, uv_b

    def _decode_prodiff(self, c):
        """ProDiff teacher decoder (stylesinger.py:175-177, modules/diff/prodiff.py:205-221): decoder_inp is the condition."""
        hp, pk, pl = self.hp, self._pk, c.pl
        B, T, M, S = c.B, c.T, hp["audio_num_mel_bins"], int(hp["timesteps"])
        pl.cond_mel.copy_(c.dec_inp)
        sch = pk["prodiff_sched"]
        wsb, wsp = self._full_batch_ws(pl, keep=True)

        def run(noise=None):
            zs = None
            if noise is None:
                L.ops.ss_fill_normal_rows(pl.xm, B, T * M, T * M, 31, pl.seed)
            else:
                pl.xm.copy_(_noise_btm(noise["mel"]["z_q"], c.dev, (B, M, c.T_out), T))
                zs = _noise_btm(noise["mel"]["z_steps"], c.dev, (S, B, M, c.T_out), T)
            L.ops.ss_prodiff_sample(pk["mel"]["net"], pl.xm, pl.cond_mel, pl.lens, B, T, zs, 37, pl.seed, S, sch["c1"], sch["c2"], sch["sigma"], 1,
                                    wsp, wsb)
        self._run_loop(pl, "mel", run, tape=c.ctl.noise, graphs=c.graphs)
        mel_out = torch.empty(B, T, M, **c.f32)
        # the reference leaves padded frames unmasked (prodiff.py:219-220); frames past lens[b] are written as 0 here
        L.ops.ss_add_bcast_mask(pl.xm, None, None, None, None, mel_out, B, T, M, c.lens_t)
        c.ret["mel_out"] = mel_out
        c.ret["lens"] = c.lens_t

    def _decode_fft(self, c):
        """FFT decoder -> coarse mel (a10) -> c.coarse_mel [B,T,M]."""
        hp, pk, ret = self.hp, self._pk, c.ret
        B, T, H, dev, dec_inp = c.B, c.T, hp["hidden_size"], c.dev, c.dec_inp
        xd = dec_inp.clone()
        pos_t = torch.empty(B, T, device=dev, dtype=torch.int32)
        tabt = self._pos(T + 2, dev)
        L.ops.ss_make_positions(None, dec_inp, H, T * H, pos_t, B, T)
        L.ops.ss_table_add(pos_t, tabt, tabt.shape[0], xd, H, T * H, B, T, H, self.p("decoder.pos_embed_alpha"), 1.0, 1)
        xd = self._fft_blocks(pk["dec"], xd, B, T, c.lens_t, ffn_wino=True)
        ret["decoder_out"] = xd
        c.coarse_mel = torch.empty(B, T, hp["audio_num_mel_bins"], **c.f32)
        self._gemm(xd, pk["mel_out"], c.coarse_mel, B, T, lens=c.lens_t)
        ret["fs2_mel"] = c.coarse_mel
        ret["x_mask"] = (c.mel2ph > 0).float()[:, :, None]

    def _refine_mel(self, c):
        """Condition projection (a11) + shallow mel diffusion (a12): DDPM by default, `sampler="ddim"` / `"plms"` on request."""
        hp, pk, ret, pl = self.hp, self._pk, c.ret, c.pl
        B, T, M, K, dev, noise = c.B, c.T, hp["audio_num_mel_bins"], hp["K_step"], c.dev, c.ctl.noise
        gcat = torch.cat([c.coarse_mel, c.dec_inp, c.spk[:, None, :].expand(-1, T, -1), c.emo[:, None, :].expand(-1, T, -1), c.style], -1).contiguous()
        self._gemm(gcat, pk["ln_proj"], pl.cond_mel, B, T, mask_rows=False)
        ret["diff_cond"] = pl.cond_mel.clone()
        pl.coarse_mel.copy_(c.coarse_mel)
        sm = c.ctl.mel   # resolved and checked by forward before anything ran (controls.mel_sampler)
        eta = sm.eta
        ts = self.mel_timesteps(sm.steps, sm.spacing) if sm.steps is not None else None
        if ts is not None:
            ret["mel_sampler"] = dict(name=sm.name, ts=list(ts), order=sm.order if sm.name == "dpmpp" else 1)

        def tape(nz, steps):  # recorded mel noise -> (z_q, z_steps or None) on the device
            return (_noise_btm(nz["z_q"], dev, (B, M, c.T_out), T), _noise_btm(nz["z_steps"], dev, (K, B, M, c.T_out), T) if steps else None)
        if sm.name == "plms":   # never captured
            self._run_mel(pl, (None, None) if noise is None else tape(noise["mel"], False), plms_interval=sm.interval)
        elif sm.name == "ddim":   # one captured graph per (B, T bucket, number of sampler steps, eta); off the uniform stride, per list of times
            run = lambda n=None: self._run_mel(pl, n and tape(n["mel"], eta > 0.0 and "z_steps" in n["mel"]), ddim_ts=ts, eta=eta)
            self._run_loop(pl, ("ddim", len(ts) if sm.spacing == "uniform" else tuple(ts), eta), run, tape=noise, graphs=c.graphs)
        elif sm.name == "dpmpp":   # one captured graph per (B, T bucket, list of times, order); draws nothing after q_sample: only z_q is read
            self._dpmpp_buffers(pl)   # plan-owned and allocated out here: the captured graph replays into them
            run = lambda n=None: self._run_mel(pl, n and tape(n["mel"], False), dpmpp=(ts, sm.order))
            self._run_loop(pl, ("dpmpp", tuple(ts), sm.order), run, tape=noise, graphs=c.graphs)
        else:
            with self._q4_guard(pl, eager=not c.graphs):
                self._run_loop(pl, "mel", lambda n=None: self._run_mel(pl, n and tape(n["mel"], True)), tape=noise, graphs=c.graphs)
        mel_out = torch.empty(B, T, M, **c.f32)
        # the reference does not mask padded frames here (shallow_diffusion_tts.py:305-306); with per-item
        # lengths the frames past lens[b] are not part of the utterance, so they are written as 0.
        pl.nonfinite.zero_()
        L.ops.ss_mel_denorm(pl.xm, pk["spec_min"], pk["spec_max"], mel_out, B, T, M, c.lens_t, pl.nonfinite)
        # fp16 terms carry the residual stream x + dstep and the gate outputs inside the stack: unlike the bf16 modes they overflow beyond 65504.
        # The denorm kernel flags a non-finite valid frame on EVERY forward (ret["nonfinite"], a device word: `check_finite(ret)` wherever the
        # caller synchronises anyway - infer.py does); the first forward of every plan checks it here (one host sync).
        ret["nonfinite"] = pl.nonfinite.clone()
        if self.f16 and pl.uses <= 1:
            self.check_finite(ret)
        ret["mel_out"] = mel_out
        ret["diff"] = 0.0
        ret["lens"] = c.lens_t

    def check_finite(self, ret):
        """Raise if the forward that produced `ret` wrote a non-finite valid mel frame (reads one device word: a host sync)."""
        flag = ret.get("nonfinite")
        if flag is not None and int(flag.item()) != 0:
            if self.f16:
                raise L.StyleSingerHipError("mfma_precision=fp16x2: non-finite mel after the diffusion loop - the residual stream of this checkpoint "
                                            "leaves the fp16 range (|x + dstep| > 65504); use mfma_precision='bf16x2' (fp32 exponent range)")
            raise L.StyleSingerHipError("non-finite mel after the diffusion loop")

    _FRAME_KEYS = ("mel2ph", "style", "pitch_pred", "f0_denorm", "f0_denorm_pred", "pitch_coarse", "f0_a", "uv_a", "f0_b", "uv_b",
                   "decoder_inp", "decoder_out", "fs2_mel", "x_mask", "diff_cond", "mel_out", "pitch_align_idx", "pitch_pred_raw", "f0_denorm_raw")

    @classmethod
    def _crop_frames(cls, ret, T, T_out):
        """Undo the bucket padding: frame-level outputs back to the caller's frame count."""
        if T != T_out:
            for k in cls._FRAME_KEYS:
                if k in ret:
                    ret[k] = ret[k][:, :T_out].contiguous()
        return ret
