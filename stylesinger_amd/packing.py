"""Weight packing of `StyleSingerHIP`: the reference `state_dict` -> the layouts the HIP kernels read (`model._pk`).

`Packing` is a mixin of the model: `pack()` runs lazily (`_ensure_packed()`) on the first forward after the weights changed."""
import math

import numpy as np
import torch

from . import lib as L


class _Packed:
    """A conv/linear weight in the MFMA kernel's layout + its metadata."""
    __slots__ = ("W", "bias", "Cout", "Cin", "k", "Np", "Kp", "half", "W43")

    def __init__(self, W, bias, Cout, Cin, k, half=0):
        self.W, self.bias, self.Cout, self.Cin, self.k, self.half = W, bias, Cout, Cin, k, half
        self.Np, self.Kp = W.shape[0], W.shape[1] // k
        self.W43 = None   # the same conv as grouped F(4,3) tap groups (ss_wino43_conv), where one was packed


def _sin_table(n, dim):
    """SinusoidalPositionalEmbedding.get_embedding (common_layers.py:107-124), host fp32, padding row 0 zeroed."""
    half = dim // 2
    e = math.log(10000) / (half - 1)
    e = torch.exp(torch.arange(half, dtype=torch.float) * -e)
    e = torch.arange(n, dtype=torch.float).unsqueeze(1) * e.unsqueeze(0)
    e = torch.cat([torch.sin(e), torch.cos(e)], dim=1).view(n, -1)
    e[0, :] = 0
    return e


def _step_emb_table(steps, dim):
    """SinusoidalPosEmb(t) for t = 0..steps-1 (modules/diff/net.py:32-44)."""
    half = dim // 2
    e = math.log(10000) / (half - 1)
    e = torch.exp(torch.arange(half) * -e)
    e = torch.arange(steps)[:, None].float() * e[None, :]
    return torch.cat((e.sin(), e.cos()), dim=-1).contiguous()


F0_COEF_NAMES = ("recip", "recipm1", "c1", "c2", "sigma", "log_alpha_t", "log_1m_alpha_t", "log_cp_tm1", "log_1m_cp_tm1")   # F0StepCoef
F0_STRIDED_RTOL = 1e-6


def f0_strided_coef(betas64, t, s, eta):
    """The nine fp32 coefficients of the transition t -> s (s = -1: final) of the strided f0 / uv sampler (`ss_f0_strided_coef`: host only)."""
    betas64 = np.ascontiguousarray(betas64, dtype=np.float64)
    out = np.empty(9, np.float32)
    L.check(L.load().ss_f0_strided_coef(L.hptr(betas64), len(betas64), int(t), int(s), float(eta), L.hptr(out)), "ss_f0_strided_coef")
    return out


def f0_table_coef(tables, t):
    """What `ss_f0diff_sample` reads from the checkpoint's fp32 tables at network time t, under the same nine names. The two prior entries are
    not read at t = 0 (None)."""
    g = lambda k: float(np.asarray(tables[k], np.float32)[t])
    p = lambda k: float(np.asarray(tables[k], np.float32)[t - 1]) if t > 0 else None
    sigma = float(np.exp(np.float32(0.5) * np.float32(g("posterior_log_variance_clipped")))) if t > 0 else 0.0
    return (g("sqrt_recip_alphas_cumprod"), g("sqrt_recipm1_alphas_cumprod"), g("posterior_mean_coef1"), g("posterior_mean_coef2"), sigma,
            g("log_alpha"), g("log_1_min_alpha"), p("log_cumprod_alpha"), p("log_1_min_cumprod_alpha"))


def f0_strided_guard(tables):
    """Do the checkpoint's f0 schedule tables belong to its betas? The stride-1, eta = 1 coefficients of every network time, computed from
    `betas` widened to float64, against the fp32 tables `ss_f0diff_sample` reads - all nine names, the four multinomial tables included.
    `tables`: reference buffer name -> 1-D array. Returns (betas float64, worst relative deviation, (name, t) of the worst, error text or None):
    a deviation above F0_STRIDED_RTOL means the strided sampler would not continue the sampler the checkpoint was trained with."""
    betas = np.ascontiguousarray(np.asarray(tables["betas"], np.float32).astype(np.float64))
    worst, where = 0.0, None
    for t in range(len(betas)):
        mine, ref = f0_strided_coef(betas, t, t - 1, 1.0), f0_table_coef(tables, t)
        for name, a, b in zip(F0_COEF_NAMES, mine, ref):
            if b is None:
                continue
            dev = abs(float(a) - b) / abs(b) if b != 0.0 else (0.0 if float(a) == 0.0 else float("inf"))
            if not dev <= worst:   # also a NaN
                worst, where = dev, (name, t)
    err = None
    if not worst <= F0_STRIDED_RTOL:
        err = (f"the f0 schedule tables of this checkpoint do not belong to its f0_gen.betas: {where[0]} at network time {where[1]} deviates by "
               f"{worst:.3g} (relative; limit {F0_STRIDED_RTOL:g}) from the value the betas give - strided f0 sampling (f0_steps) is refused for "
               f"this checkpoint; the default sampler reads the tables as they are and is unaffected")
    return betas, worst, where, err


class Packing:
    """Mixin of StyleSingerHIP: builds `self._pk` from the registered weights (uses `self.p`, `self.hp` and the precision-mode flags)."""
    # "fp16x2": the weights' power-of-two shift. |w| 2^8 < 65504 for |w| < 255; lo = RNE16(w 2^8 - hi) stays a NORMAL fp16 number for every
    # |w| >= 2^-10 and below that is exact to 2^-32 in absolute terms (fp16 subnormals are fixed point) - no reliance on how the matrix cores
    # treat subnormal inputs for any weight that matters. oracle/restatement.py uses the same constant.
    FP16_WSHIFT = 8

    def _split_w(self, w, f0=False):
        """packed fp32 weight -> split 16-bit pack of the precision mode (pairs interleaved by 32 along every row). The two f0 denoisers keep the
        three-product bf16 form in "fp16x2" mode: their outputs feed DISCRETE voicing decisions (one flipped in 11 250 at T = 5625 with two
        products, none with three) and their 200 steps are ~1 % of a C4 batch."""
        if not self.f16 or f0:
            return L.split_bf16(w)
        if float(w.abs().max()) * 2.0 ** self.FP16_WSHIFT >= 32768.0:
            raise ValueError("mfma_precision=fp16x2: a hidden-layer weight exceeds 128 in magnitude (fp16 range after the 2^8 shift)")
        return L.split_f16(w, scale=2.0 ** self.FP16_WSHIFT)

    def _sd_sets(self, w):
        """"fp16sd": packed fp32 weight [rows][K] -> fp16 [N][rows][2 K], the N noise-shaped one-term weight sets in the pair layout with ZERO lo terms
        (the two-product kernels then compute the one-product result exactly). Sigma-delta in the scaled domain: r_0 = 0, W_k = RNE16(w 2^s + r_k),
        r_(k+1) = r_k + (w 2^s - W_k): sum_k W_k = N w 2^s - r_N, |r_N| <= half an fp16 ulp."""
        if float(w.abs().max()) * 2.0 ** self.FP16_WSHIFT >= 32768.0:
            raise ValueError("mfma_precision=fp16sd: a hidden-layer weight exceeds 128 in magnitude (fp16 range after the 2^8 shift)")
        ws = w.float() * 2.0 ** self.FP16_WSHIFT
        r = torch.zeros_like(ws)
        sets = []
        for _ in range(self.sd_sets):
            wk = (ws + r).to(torch.float16).float()
            r = r + (ws - wk)
            sets.append(L.split_f16(wk, scale=1.0))    # hi = W_k exactly (it is an fp16 number), lo = 0
        return torch.stack(sets).contiguous()

    def _pack_conv(self, wname, bname=None, *, half=0, scale0=None, row_scale=1.0, bias2=None):
        w = self.p(wname)
        if w.dim() == 2:
            Cout, Cin, k = w.shape[0], w.shape[1], 1
        else:
            Cout, Cin, k = w.shape
        W = L.pack_conv_weight(w, scale0=scale0, interleave_half=half, row_scale=row_scale)
        bias = None
        if bname is not None:
            bias = L.pack_bias(self.p(bname), b2=bias2, interleave_half=half)
        return _Packed(W, bias, Cout, Cin, k, half)

    def _pack_wn_conv(self, prefix, *, half=0):
        v, g = self.p(prefix + ".weight_v"), self.p(prefix + ".weight_g")
        s0 = L.weight_norm_scale(v, g)
        Cout, Cin, k = v.shape
        W = L.pack_conv_weight(v, scale0=s0, interleave_half=half)
        bias = L.pack_bias(self.p(prefix + ".bias"), interleave_half=half)
        return _Packed(W, bias, Cout, Cin, k, half)

    def _wino_form(self, C, cycle):
        """Which Winograd form a denoiser's dilated convs take, decided ONCE at pack time from what the kernels accept: F(4,3)
        (ss_wino43_gate / ss_wino43_gate16) needs C % 32 == 0 and dilations 2^(l % cycle) <= 64; otherwise F(2,3)."""
        return 4 if (self.wino_m == 4 and C % 32 == 0 and (1 << (max(int(cycle), 1) - 1)) <= 64) else 2

    def _pack_wavenet_tensors(self, prefix, C, Lyr, steps, f0, cycle=4):
        """Packed device tensors of one denoiser (DiffNet / DDiffNet), keyed like the ss_wavenet fields."""
        dev = self.p(prefix + ".mlp.0.weight").device
        t = {}
        if f0:
            t["w_in"] = self.p(prefix + ".input_projection.weight").reshape(-1).contiguous()
            t["b_in"] = self.p(prefix + ".input_projection.bias").contiguous()
            t["uv_embed"] = self.p(prefix + ".uv_embed.weight").contiguous()
        else:
            pin = self._pack_conv(prefix + ".input_projection.weight", prefix + ".input_projection.bias")
            t["w_in"], t["b_in"] = pin.W, pin.bias
        # dstep[s][l][:] = diffusion_projection_l(mlp(SinusoidalPosEmb(s)))  (net.py:66,118-119) — weights-only table
        emb = _step_emb_table(steps, C).to(dev)
        m0 = self._pack_conv(prefix + ".mlp.0.weight", prefix + ".mlp.0.bias")
        m2 = self._pack_conv(prefix + ".mlp.2.weight", prefix + ".mlp.2.bias")
        h1 = torch.empty(steps, 4 * C, device=dev)
        h2 = torch.empty(steps, C, device=dev)
        L.conv_gemm(emb, m0.W, h1, B=1, T=steps, Cin=C, N=4 * C, Np=m0.Np, Kp=m0.Kp, bias=m0.bias, act=L.ACT_MISH, mask_rows=False)
        L.conv_gemm(h1, m2.W, h2, B=1, T=steps, Cin=4 * C, N=C, Np=m2.Np, Kp=m2.Kp, bias=m2.bias, mask_rows=False)
        dstep = torch.empty(steps, Lyr, C, device=dev)
        wc_rows, bc_rows = [], []
        for l in range(Lyr):
            p = f"{prefix}.residual_layers.{l}"
            dp = self._pack_conv(p + ".diffusion_projection.weight", p + ".diffusion_projection.bias")
            L.conv_gemm(h2, dp.W, dstep[:, l], B=1, T=steps, Cin=C, N=C, Np=dp.Np, Kp=dp.Kp, bias=dp.bias, ldc=Lyr * C,
                        mask_rows=False)
            dil = self._pack_conv(p + ".dilated_conv.weight", None, half=C)
            out = self._pack_conv(p + ".output_projection.weight", p + ".output_projection.bias")
            cnd = self._pack_conv(p + ".conditioner_projection.weight", p + ".conditioner_projection.bias", half=C,
                                  bias2=self.p(p + ".dilated_conv.bias"))
            t[f"w_dil.{l}"], t[f"w_out.{l}"], t[f"b_out.{l}"] = dil.W, out.W, out.bias
            if self.defer_skip and not self.bf16 and C % 64 == 0:   # residual half in the fetch order of ss_gemm16_res
                t[f"w_out16.{l}"] = L.pack_gemm16_weights(out.W[:C].contiguous(), out.Kp)
            if self.use_wino:
                wsrc = self.p(p + ".dilated_conv.weight").contiguous()
                wt = L.wino43_weight(wsrc) if self._wino_form(C, cycle) == 4 else L.wino_weight(wsrc)
                t[f"w_dil_wino.{l}"] = L.pack_conv_weight(wt, interleave_half=C)
                if self._wino_form(C, cycle) == 4 and t[f"w_dil_wino.{l}"].shape[0] % 64 == 0:   # the 16x16x4 kernel's fetch order
                    t[f"w_dil_wino16.{l}"] = L.pack_gate16_weights(t[f"w_dil_wino.{l}"], dil.Kp)
                if self.x3 and self._wino_form(C, cycle) == 4:
                    t[f"w_dil_x3.{l}"] = L.split3_weights(t[f"w_dil_wino.{l}"], dil.Kp)
            if self.bf16_hbm:  # bf16 weight copies (rounded once, RNE): the operands of ss_gemm_bf16
                to_h = (lambda w_: self._split_w(w_, f0)) if self.split else L.to_bf16   # split: pairs interleaved by 32 along every row
                if self.sd and not f0:   # N one-term weight sets per tensor ([N][rows][2 K]; set 0 first)
                    to_h = self._sd_sets
                t[f"w_dil_h.{l}"] = to_h(dil.W)
                t[f"w_out_h.{l}"] = to_h(out.W)
                if self.q4 and not f0 and C == 256:   # the fp4 lo plane in the lane order of ss_gemm_bf16_gate128q
                    t[f"w_dil_q.{l}"] = L.pack_gate_q4(dil.W, shift=self.FP16_WSHIFT)[0]
                if self.f16 and not f0 and C == 256 and tuple(t[f"w_dil_h.{l}"].shape[-2:]) == (512, 3 * 256 * 2):
                    # the same terms in the fragment order ss_layer512 streams (one launch per layer at many-round sizes); fp16sd: one term, N sets
                    if self.sd:
                        t[f"w_dil_f.{l}"] = torch.stack([L.layer512_pack_gate(w_, 1) for w_ in t[f"w_dil_h.{l}"]]).contiguous()
                        t[f"w_out_f.{l}"] = torch.stack([L.layer512_pack_res(w_, 1) for w_ in t[f"w_out_h.{l}"]]).contiguous()
                    else:
                        t[f"w_dil_f.{l}"] = L.layer512_pack_gate(t[f"w_dil_h.{l}"])
                        t[f"w_out_f.{l}"] = L.layer512_pack_res(t[f"w_out_h.{l}"])
            wc_rows.append(cnd.W)
            bc_rows.append(cnd.bias)
        if self.defer_skip:  # skip halves of all output projections side by side: [C][L*C], column l*C + ci
            wsk = torch.cat([self.p(f"{prefix}.residual_layers.{l}.output_projection.weight")[C:, :, 0] for l in range(Lyr)], dim=1)
            bsk = torch.stack([self.p(f"{prefix}.residual_layers.{l}.output_projection.bias")[C:] for l in range(Lyr)]).sum(0)
            if self.fold_skip:  # skip_projection(sum/sqrt(L)) is linear in the g_l: fold it into the weights (float64 product)
                ws_ = self.p(prefix + ".skip_projection.weight")[:, :, 0].double()
                bs_ = self.p(prefix + ".skip_projection.bias").double()
                r = 1.0 / math.sqrt(Lyr)
                bsk = (ws_ @ bsk.double() * r + bs_).float()
                wsk = (ws_ @ wsk.double() * r).float()
            t["w_skipall"] = L.pack_conv_weight(wsk[:, :, None].contiguous())
            if self.x3 and self.fold_skip:
                t["w_skipall_x3"] = L.split3_gemm16_weights(t["w_skipall"], t["w_skipall"].shape[1])
            t["b_skipall"] = L.pack_bias(bsk.contiguous())
        t["dstep"] = dstep
        if self.f16 and not f0 and float(dstep.abs().max()) >= 16384.0:
            # activation-range contract of the fp16 modes: the stream enters every layer as fp16(x + dstep_l); a step embedding this large
            # leaves no headroom below 65504 (the bf16 modes have the fp32 exponent range)
            raise ValueError("mfma_precision=fp16x2: a diffusion-step embedding exceeds 16384 in magnitude - fp16 activations would overflow; use bf16x2")
        t["w_cond"] = torch.cat(wc_rows, 0).contiguous()
        t["b_cond"] = torch.cat(bc_rows, 0).contiguous()
        if self.bf16_hbm:
            t["w_cond_h"] = L.to_bf16(t["w_cond"])     # (unused in split mode: the hoisted projection runs in fp32 there)
            t["w_skipall_h"] = (self._sd_sets(t["w_skipall"]) if (self.sd and not f0) else self._split_w(t["w_skipall"], f0)) if self.split else L.to_bf16(t["w_skipall"])
            if self.sd and not f0 and t["w_skipall"].shape[1] % 64 == 0:   # the same sets without the zero plane: [N][Np][L C] (ss_wavenet.w_skipall_c)
                t["w_skipall_c"] = L.split_planes(t["w_skipall_h"])[0].to(torch.float16).contiguous()
            if self.q4 and not f0 and t["w_skipall"].shape[1] % 64 == 0:   # the fp4 lo plane in the lane order of ss_gemm_bf16_tile256q
                t["w_skipall_q"] = L.pack_skip_q4(t["w_skipall"], shift=self.FP16_WSHIFT)[0]
        skip = self._pack_conv(prefix + ".skip_projection.weight", prefix + ".skip_projection.bias")
        fin = self._pack_conv(prefix + ".output_projection.weight", prefix + ".output_projection.bias")
        t["w_skip"], t["b_skip"], t["w_final"], t["b_final"] = skip.W, skip.bias, fin.W, fin.bias
        torch.cuda.synchronize()
        return t

    def _pack_wavenet(self, prefixes, gen, C, Lyr, cycle, steps, in_dim, out_dim, f0):
        """Build the ss_wavenet descriptor of one net, or of a PAIR of same-shaped nets (grouped launches: every
        weight tensor is stacked [2][...] so that net g sits gs_* floats after net 0)."""
        hp = self.hp
        packs = [self._pack_wavenet_tensors(pf, C, Lyr, steps, f0, cycle) for pf in prefixes]
        keep = []
        net = L.WaveNet()
        net.C, net.L, net.cond_dim, net.dil_cycle, net.in_dim, net.out_dim, net.steps = C, Lyr, hp["hidden_size"], cycle, in_dim, out_dim, steps
        net.n_groups = len(packs)

        def place(key):
            if len(packs) == 1:
                tt = packs[0][key].contiguous()
                gs = 0
            else:
                tt = torch.stack([pk_[key] for pk_ in packs]).contiguous()
                gs = packs[0][key].numel()
            keep.append(tt)   # the descriptor holds the address, `keep` the tensor
            return L.member_address(net, key.split(".")[0], tt), gs

        for key in ("w_in", "b_in", "dstep", "w_cond", "b_cond", "w_skip", "b_skip", "w_final", "b_final") + (("uv_embed",) if f0 else ()) \
                + (("w_skipall", "b_skipall") if self.defer_skip else ()):
            ptr_, gs = place(key)
            setattr(net, key, ptr_)
            setattr(net, "gs_" + key, gs)
        for l in range(Lyr):
            for key, arr in (("w_dil", net.w_dil), ("w_out", net.w_out), ("b_out", net.b_out)):
                ptr_, gs = place(f"{key}.{l}")
                arr[l] = ptr_
                setattr(net, "gs_" + key, gs)
            if self.use_wino:
                ptr_, gs = place(f"w_dil_wino.{l}")
                net.w_dil_wino[l] = ptr_
                net.gs_w_dil_wino = gs
                net.wino_m = self._wino_form(C, cycle)
            if f"w_out16.{l}" in packs[0]:
                net.w_out16[l], net.gs_w_out16 = place(f"w_out16.{l}")
            if self.use_wino:
                if f"w_dil_wino16.{l}" in packs[0]:
                    net.w_dil_wino16[l], _ = place(f"w_dil_wino16.{l}")
                if self.x3 and f"w_dil_x3.{l}" in packs[0]:
                    ptr_, gs = place(f"w_dil_x3.{l}")
                    net.w_dil_x3[l] = ptr_
                    net.gs_w_dil_x3 = gs
                    net.mfma_x3 = 1
            if self.bf16_hbm:
                for key, arr in (("w_dil_h", net.w_dil_h), ("w_out_h", net.w_out_h)):
                    ptr_, gs = place(f"{key}.{l}")
                    arr[l] = ptr_
                    setattr(net, "gs_" + key, gs)
        if "w_skipall_x3" in packs[0]:
            net.w_skipall_x3, net.gs_w_skipall_x3 = place("w_skipall_x3")
        if self.bf16_hbm:
            for key in ("w_cond_h", "w_skipall_h"):
                ptr_, gs = place(key)
                setattr(net, key, ptr_)
                setattr(net, "gs_" + key, gs)
        net.mfma_bf16 = 1 if self.bf16 else 0
        net.mfma_split = (2 if (self.f16 and not f0) else 1) if self.split else 0
        net.mfma_out_scale = 2.0 ** -self.FP16_WSHIFT if (self.f16 and not f0) else 1.0
        self._place_mode_extras(net, packs, place, Lyr, f0)
        net.skipall_folded = 1 if self.fold_skip else 0
        return dict(net=net, keep=keep, sched=self._host_schedules(net, gen, f0, keep), packs=packs)

    def _place_mode_extras(self, net, packs, place, Lyr, f0):
        """Descriptor fields of the fp16sd weight sets, the fp16q4 fp4 planes and the ss_layer512 fragment order (mel denoiser only)."""
        if self.sd and not f0:   # every w_*_h / w_*_f tensor is [N][...]: pointer = set 0, ws_* = elements between sets
            assert len(packs) == 1
            net.n_wsets, net.mfma_products = self.sd_sets, 1
            net.n_esets = self.sd_e_sets
            net.ws_w_dil_h, net.ws_w_out_h = packs[0]["w_dil_h.0"][0].numel(), packs[0]["w_out_h.0"][0].numel()
            net.ws_w_skipall_h = packs[0]["w_skipall_h"][0].numel()
            if "w_skipall_c" in packs[0]:
                net.w_skipall_c, _ = place("w_skipall_c")
                net.ws_w_skipall_c = packs[0]["w_skipall_c"][0].numel()
            if "w_dil_f.0" in packs[0]:
                net.ws_w_dil_f, net.ws_w_out_f = packs[0]["w_dil_f.0"][0].numel(), packs[0]["w_out_f.0"][0].numel()
        if self.q4 and not f0:
            for l in range(Lyr):
                if f"w_dil_q.{l}" in packs[0]:
                    net.w_dil_q[l], net.gs_w_dil_q = place(f"w_dil_q.{l}")
            net.q_scale_gate = 2.0   # the stream x + dstep on a fixed fp4 scale (oracle/second_product_numerics.py)
            if "w_skipall_q" in packs[0]:
                net.w_skipall_q, net.gs_w_skipall_q = place("w_skipall_q")
                net.q_scale_z = 0.25   # gate outputs in (-1, 1)
        if len(packs) == 1 and all(f"w_dil_f.{l}" in packs[0] for l in range(Lyr)):
            for l in range(Lyr):
                net.w_dil_f[l], _ = place(f"w_dil_f.{l}")
                net.w_out_f[l], _ = place(f"w_out_f.{l}")

    def _host_schedules(self, net, gen, f0, keep):
        """Schedule tables live on the host (the loop driver passes per-step scalars by value): fills net's table pointers, returns `sched`."""
        def host(name):
            arr = np.ascontiguousarray(self.p(f"{gen}.{name}").detach().cpu().numpy().astype(np.float32))
            keep.append(arr)
            return arr.ctypes.data
        net.sqrt_recip_ac, net.sqrt_recipm1_ac = host("sqrt_recip_alphas_cumprod"), host("sqrt_recipm1_alphas_cumprod")
        net.post_c1, net.post_c2 = host("posterior_mean_coef1"), host("posterior_mean_coef2")
        net.post_logvar = host("posterior_log_variance_clipped")
        if f0:
            net.log_alpha, net.log_1m_alpha = host("log_alpha"), host("log_1_min_alpha")
            net.log_cumprod_alpha, net.log_1m_cumprod_alpha = host("log_cumprod_alpha"), host("log_1_min_cumprod_alpha")
        sched = {k: self.p(f"{gen}.{k}").detach().cpu() for k in ("sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")}
        if f0:   # the strided sampler builds its coefficients from the betas in float64 (ss_f0diff_sample_strided); refused where the tables disagree
            names = ("betas", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
                     "posterior_log_variance_clipped", "log_alpha", "log_1_min_alpha", "log_cumprod_alpha", "log_1_min_cumprod_alpha")
            try:
                sched["betas_f64"], sched["strided_dev"], _, sched["strided_error"] = f0_strided_guard(
                    {k: self.p(f"{gen}.{k}").detach().cpu().numpy() for k in names})
            except L.StyleSingerHipError as e:   # a beta outside (0, 1)
                sched["betas_f64"], sched["strided_dev"], sched["strided_error"] = None, float("inf"), f"strided f0 sampling is refused: {e}"
        if not f0:
            sched["alphas_cumprod_np"] = np.ascontiguousarray(self.p(f"{gen}.alphas_cumprod").detach().cpu().numpy().astype(np.float32))
            # DDIM coefficients need 1 - alphas_cumprod at small t: rebuilt in float64 from the betas buffer as the reference builds its
            # own tables (shallow_diffusion_tts.py:77-80: np.cumprod(1 - betas)); the float32 buffer has only ~3 digits of 1 - ac_0
            betas64 = self.p(f"{gen}.betas").detach().cpu().numpy().astype(np.float64)
            sched["alphas_cumprod_f64"] = np.ascontiguousarray(np.cumprod(1.0 - betas64))
        return sched

    def _pack_ffn1(self, p, wino):
        """The k-tap first FFN conv; wino (the decoder, fp32 mode): also its grouped Winograd F(4,3) pack when ss_wino43_conv covers the shape."""
        pk = self._pack_conv(p + ".ffn.ffn_1.weight", p + ".ffn.ffn_1.bias")
        if wino and self.use_wino and pk.k >= 3 and L.load().ss_wino43_conv_ok4(pk.Cin, pk.Cout, pk.k, 1):
            pk.W43 = L.pack_conv_weight(L.wino43_group_weight(self.p(p + ".ffn.ffn_1.weight")))
        return pk

    def _pack_fft(self, prefix, n_layers, ffn_wino=False):
        layers = []
        for i in range(n_layers):
            p = f"{prefix}.layers.{i}.op"
            layers.append(dict(
                ln1=(self.p(p + ".layer_norm1.weight"), self.p(p + ".layer_norm1.bias")),
                qkv=self._pack_conv(p + ".self_attn.in_proj_weight"),
                out=self._pack_conv(p + ".self_attn.out_proj.weight"),
                ln2=(self.p(p + ".layer_norm2.weight"), self.p(p + ".layer_norm2.bias")),
                ffn1=self._pack_ffn1(p, ffn_wino),
                ffn2=self._pack_conv(p + ".ffn.ffn_2.weight", p + ".ffn.ffn_2.bias")))
        return dict(layers=layers, ln=(self.p(prefix + ".layer_norm.weight"), self.p(prefix + ".layer_norm.bias")))

    def pack(self):
        """(Re)build every packed weight on the current device; called lazily by forward."""
        hp = self.hp
        dev = self.p("mel_out.weight").device
        if not dev.type == "cuda":
            raise L.StyleSingerHipError("StyleSingerHIP needs its weights on a GPU (model.to('cuda')): there is no CPU path")
        pk = {}
        pk["enc"] = self._pack_fft("encoder", hp["enc_layers"])
        pk["dec"] = self._pack_fft("decoder", hp["dec_layers"], ffn_wino=True)
        pk["mel_out"] = self._pack_conv("mel_out.weight", "mel_out.bias")
        pk["spk"] = self._pack_conv("spk_embed_proj.weight", "spk_embed_proj.bias")
        pk["emo"] = self._pack_conv("emo_embed_proj.weight", "emo_embed_proj.bias")
        pk["dur"] = [dict(conv=self._pack_conv(f"dur_predictor.conv.{i}.1.weight", f"dur_predictor.conv.{i}.1.bias"),
                          ln=(self.p(f"dur_predictor.conv.{i}.3.weight"), self.p(f"dur_predictor.conv.{i}.3.bias")))
                     for i in range(hp["dur_predictor_layers"])]
        pk["dur_lin"] = self._pack_conv("dur_predictor.linear.weight", "dur_predictor.linear.bias")
        # RSA
        wn = []
        for i in range(4):
            inl = self._pack_wn_conv(f"style_extractor.wavenet.in_layers.{i}", half=80)
            v, g = self.p(f"style_extractor.wavenet.res_skip_layers.{i}.weight_v"), self.p(f"style_extractor.wavenet.res_skip_layers.{i}.weight_g")
            s0 = L.weight_norm_scale(v, g)
            b = self.p(f"style_extractor.wavenet.res_skip_layers.{i}.bias")
            if i < 3:
                res = _Packed(L.pack_conv_weight(v[:80], scale0=s0[:80].contiguous()), L.pack_bias(b[:80]), 80, 80, 1)
                skp = _Packed(L.pack_conv_weight(v[80:], scale0=s0[80:].contiguous()), L.pack_bias(b[80:]), 80, 80, 1)
            else:
                res = None
                skp = _Packed(L.pack_conv_weight(v, scale0=s0), L.pack_bias(b), 80, 80, 1)
            wn.append(dict(inl=inl, res=res, skip=skp))
        pk["wn"] = wn
        cb = []
        for rb in range(5):
            for blk in range(2):
                p = f"style_extractor.encoder.res_blocks.{rb}.blocks.{blk}"
                cb.append(dict(ln=(self.p(p + ".0.weight"), self.p(p + ".0.bias")), c1=self._pack_conv(p + ".1.weight", p + ".1.bias"),
                               c2=self._pack_conv(p + ".4.weight", p + ".4.bias")))
        pk["cb"] = cb
        pk["cb_ln"] = (self.p("style_extractor.encoder.last_norm.weight"), self.p("style_extractor.encoder.last_norm.bias"))
        pk["cb_post"] = self._pack_conv("style_extractor.encoder.post_net1.weight", "style_extractor.encoder.post_net1.bias")
        pk["codebooks"] = torch.stack([self.p(f"style_extractor.rqvae.codebooks.{d}.weight") for d in range(hp["rq_depth"])]).contiguous()
        pk["l1"] = self._pack_conv("l1.weight", "l1.bias")
        al = []
        H = hp["hidden_size"]
        for i in range(2):
            p = f"align.layers.{i}"
            w, b = self.p(p + ".multihead_attn.in_proj_weight"), self.p(p + ".multihead_attn.in_proj_bias")
            al.append(dict(
                q=_Packed(L.pack_conv_weight(w[:H]), L.pack_bias(b[:H]), H, H, 1),
                kv=_Packed(L.pack_conv_weight(w[H:]), L.pack_bias(b[H:]), 2 * H, H, 1),
                out=self._pack_conv(p + ".multihead_attn.out_proj.weight", p + ".multihead_attn.out_proj.bias"),
                n1=(self.p(p + ".norm1.weight"), self.p(p + ".norm1.bias")), n2=(self.p(p + ".norm2.weight"), self.p(p + ".norm2.bias")),
                l1=self._pack_conv(p + ".linear1.weight", p + ".linear1.bias"), l2=self._pack_conv(p + ".linear2.weight", p + ".linear2.bias")))
        pk["align"] = al
        f0_args = (hp["f0_residual_channels"], hp["f0_residual_layers"], hp["f0_dilation_cycle_length"], hp["f0_timesteps"], 1, 3, True)
        # the two f0 denoisers have identical shapes and schedules -> one grouped descriptor (items [0,B): agnostic
        # net, [B,2B): specific net): every launch of the f0 loops carries 2x the blocks.
        pk["f0_pair"] = self._pack_wavenet(["gm_diffnet", "gm_diffnet_inpainte"], "f0_gen", *f0_args)
        mel_args = (hp["residual_channels"], hp["residual_layers"], hp["dilation_cycle_length"], hp["timesteps"],
                    hp["audio_num_mel_bins"], hp["audio_num_mel_bins"], False)
        if self.prodiff:  # hparams['decoder'] == 'prodiff' (stylesinger.py:111-117): the DiffNet conditioned on decoder_inp itself
            pk["mel"] = self._pack_wavenet(["diff_decoder.denoise_fn"], "diff_decoder", *mel_args)
            g = lambda k: np.ascontiguousarray(self.p("diff_decoder." + k).detach().cpu().numpy().astype(np.float32))
            pk["prodiff_sched"] = dict(c1=g("posterior_mean_coef1"), c2=g("posterior_mean_coef2"),
                                       sigma=np.ascontiguousarray(np.exp(0.5 * g("posterior_log_variance_clipped")).astype(np.float32)))
        else:
            pk["mel"] = self._pack_wavenet(["postdiff.denoise_fn"], "postdiff", *mel_args)
            pk["ln_proj"] = self._pack_conv("ln_proj.weight", "ln_proj.bias")
            pk["spec_min"] = self.p("postdiff.spec_min").reshape(-1).contiguous()
            pk["spec_max"] = self.p("postdiff.spec_max").reshape(-1).contiguous()
        self._pk = pk
        self._packed_version = self._weights_version
        self._pack_device = dev
        self._pos_table = None
        # captured hipGraphs carry the OLD packed-weight pointers in their kernel arguments: drop every plan with them
        self._plans.clear()
        torch.cuda.synchronize()

    def _ensure_packed(self):
        dev = self.p("mel_out.weight").device
        if self._pk is None or self._packed_version != self._weights_version or self._pack_device != dev:
            self.pack()
