"""Statements of the reference blend (segment-weighted style attention) for the tests: torch on the CPU, in the dtype of their inputs - float64 is
the definition the kernel is held to, float32 says what fp32 arithmetic gives on the same inputs (the "4 x rule" of test_gpu_small_kernels.py).
tests/test_style_blend_refs_cpu.py checks `seg_attention` in float64 against stock `torch.nn.functional.multi_head_attention_forward` (the op behind
the reference's nn.MultiheadAttention, lse.py:19,41) with `key_padding_mask` for the holes and `attn_mask` for the bias.

Definition: item b has R segments of Ts key rows; segment r holds seg_lens[b, r] valid rows (rows [r * Ts, r * Ts + seg_lens[b, r])) and a log prior
weight seg_logw[b, r] (-inf = the segment is out). Per head:
    O[q] = sum_{r,k} softmax_{(r,k)}( scale * Q[q] . K[r,k] + seg_logw[b, r] ) V[r,k]
over the valid keys of the segments with finite seg_logw; a row without any such key is 0; rows q >= qlens[b] are not written."""
import math

import torch
import torch.nn.functional as F


def key_layout(R, Ts, seg_lens, seg_logw):
    """-> (valid [B, R * Ts] bool, bias [B, R * Ts] float64): which key rows take part and what is added to their scores."""
    seg_lens = torch.as_tensor(seg_lens, dtype=torch.int64).reshape(-1, R)
    seg_logw = torch.as_tensor(seg_logw, dtype=torch.float64).reshape(-1, R)
    pos = torch.arange(Ts)[None, None, :]
    live = torch.isfinite(seg_logw)
    valid = (pos < seg_lens.clamp(max=Ts)[:, :, None]) & live[:, :, None]
    bias = torch.where(live, seg_logw, torch.zeros_like(seg_logw))[:, :, None].expand(-1, -1, Ts)
    B = seg_lens.shape[0]
    return valid.reshape(B, R * Ts), bias.reshape(B, R * Ts).contiguous()


def seg_attention(q, k, v, *, H, D, scale, R, Ts, seg_lens, seg_logw, qlens=None):
    """q [B, Tq, H * D], k / v [B, R * Ts, H * D] (torch, any float dtype; what rows outside the segments' lengths hold is never read) ->
    (out [B, Tq, H * D] in that dtype, written [B, Tq] bool)."""
    B, Tq = q.shape[0], q.shape[1]
    valid, bias = key_layout(R, Ts, seg_lens, seg_logw)
    out = torch.zeros(B, Tq, H * D, dtype=q.dtype)
    written = torch.zeros(B, Tq, dtype=torch.bool)
    for b in range(B):
        m = Tq if qlens is None else min(int(qlens[b]), Tq)
        written[b, :m] = True
        idx = torch.nonzero(valid[b])[:, 0]
        if idx.numel() == 0:
            continue
        for h in range(H):
            c = slice(h * D, (h + 1) * D)
            s = (q[b, :m, c] * scale) @ k[b, idx][:, c].T + bias[b, idx].to(q.dtype)[None, :]
            out[b, :m, c] = torch.softmax(s, dim=-1) @ v[b, idx][:, c]
    return out, written


def stock_mha(q, k, v, *, H, D, R, Ts, seg_lens, seg_logw):
    """The same through stock F.multi_head_attention_forward with identity projections (scale = D ** -0.5 is the op's own): key_padding_mask = the
    holes, attn_mask = the bias. Items without a key are NaN there, as torch defines a fully masked row. -> out [B, Tq, H * D]"""
    B, Tq, E = q.shape
    valid, bias = key_layout(R, Ts, seg_lens, seg_logw)
    eye = torch.eye(E, dtype=q.dtype)
    mask = bias.to(q.dtype)[:, None, None, :].expand(B, H, Tq, R * Ts).reshape(B * H, Tq, R * Ts)
    kk, vv = (torch.where(valid[:, :, None], a, torch.zeros_like(a)) for a in (k, v))   # (the op multiplies masked rows by 0: no NaN may sit there)
    o, _ = F.multi_head_attention_forward(q.transpose(0, 1), kk.transpose(0, 1), vv.transpose(0, 1), E, H, torch.cat([eye, eye, eye]),
                                          torch.zeros(3 * E, dtype=q.dtype), None, None, False, 0.0, eye, torch.zeros(E, dtype=q.dtype),
                                          training=False, key_padding_mask=~valid, need_weights=False, attn_mask=mask)
    assert math.isclose(D ** -0.5, (E // H) ** -0.5)
    return o.transpose(0, 1)


def align_layers(sd, content, sty, *, R, Ts, seg_lens, seg_logw, dtype):
    """The two CrossAttenLayers of the ProsodyAligner (lse.py:28-81; oracle/restatement.py::prosody_aligner) on content [B, T, H] and the pooled style
    sequence sty [B, R * Ts, H] (after `l1`), the attention in the segmented form above, everything in `dtype`. -> [B, T, H]"""
    H = content.shape[-1]
    w = lambda name: sd[name].to(dtype)
    x, sty = content.to(dtype), sty.to(dtype)
    for i in range(2):
        p = f"align.layers.{i}"
        w_in, b_in = w(p + ".multihead_attn.in_proj_weight"), w(p + ".multihead_attn.in_proj_bias")
        q = F.linear(x, w_in[:H], b_in[:H])
        k = F.linear(sty, w_in[H:2 * H], b_in[H:2 * H])
        v = F.linear(sty, w_in[2 * H:], b_in[2 * H:])
        o, _ = seg_attention(q, k, v, H=2, D=H // 2, scale=(H // 2) ** -0.5, R=R, Ts=Ts, seg_lens=seg_lens, seg_logw=seg_logw)
        a = F.linear(o, w(p + ".multihead_attn.out_proj.weight"), w(p + ".multihead_attn.out_proj.bias"))
        x = F.layer_norm(x + a, (H,), w(p + ".norm1.weight"), w(p + ".norm1.bias"), 1e-5)
        f = F.linear(F.relu(F.linear(x, w(p + ".linear1.weight"), w(p + ".linear1.bias"))), w(p + ".linear2.weight"), w(p + ".linear2.bias"))
        x = F.layer_norm(x + f, (H,), w(p + ".norm2.weight"), w(p + ".norm2.bias"), 1e-5)
    return x
