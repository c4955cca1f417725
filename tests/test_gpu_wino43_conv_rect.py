"""ss_wino43_conv at the shapes it gained: the 32-column tile (C = 32, the last HiFi-GAN stage of the default generator) and rectangular convs
(Cin != N, any odd k = 3..11, GELU epilogue, mask_rows = 0: the first FFN conv of the FFT decoder blocks).

Every launch is compared with torch's float64 conv1d on the zero-extended items and with ss_conv_gemm on the SAME arguments. Bound: 4 x the
larger of (a) the direct kernel's error and (b) the error of the CPU emulation of the grouped F(4,3) arithmetic
(oracle.wino_vocoder_numerics.conv1d_wino43), both against float64 on the same case - the rule of tests/vocoder_shape_cases.py - and at
least 2 fp32 ulp at the output's scale. The input buffer holds garbage behind lens[b]: both kernels must read those rows as 0."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import record_measurement  # noqa: E402
from oracle.wino_vocoder_numerics import conv1d_wino43  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

DEV = "cuda:0"
TAIL = 1024
SENT = -77.25
ULP = 2.0 ** -23


def _out_buf(init):
    """[B, T, N] values followed by a sentinel tail, as one flat device buffer; returns (flat, view)."""
    flat = torch.full((init.numel() + TAIL,), SENT, device=DEV, dtype=torch.float32)
    flat[:init.numel()] = init.reshape(-1).to(DEV)
    return flat, flat[:init.numel()].view(init.shape)


def _epilogue(y, dt, bias, pre, act, R, post, prev, n, T, mask):
    """y [1, n', N] conv output without bias (n' = n when masked, T otherwise) -> the STORE epilogue in dtype dt, padded to T rows."""
    y = (y + bias.to(dt)) * pre
    if act == "lrelu":
        y = F.leaky_relu(y, 0.1)
    elif act == "gelu":
        y = F.gelu(y)
    rows = y.shape[1]
    if R is not None:
        y = y + R[:, :rows].to(dt)
    y = y * post
    if prev is not None:
        y = y + prev[:, :rows].to(dt)
    return F.pad(y, (0, 0, 0, T - rows))


def _references(x, lens_l, w, bias, k, d, slope_in, pre, act, R, post, prev, mask):
    """(float64 reference, fp32 CPU emulation of the grouped F(4,3) form), each [B, T, N]; rows >= lens[b] of the INPUT are zero padding."""
    B, T, _ = x.shape
    pad = (k - 1) // 2 * d
    r64, emu = [], []
    for b, n in enumerate(lens_l):
        rows = n if mask else T
        xi = torch.zeros(1, rows, x.shape[2])
        xi[:, :min(n, rows)] = x[b:b + 1, :n]
        if slope_in != 1.0:
            xi = F.leaky_relu(xi, slope_in)
        Rb = None if R is None else R[b:b + 1]
        Pb = None if prev is None else prev[b:b + 1]
        y64 = F.conv1d(xi.double().transpose(1, 2), w.double(), None, padding=pad, dilation=d).transpose(1, 2)
        r64.append(_epilogue(y64, torch.float64, bias, pre, act, Rb, post, Pb, n, T, mask))
        ye = conv1d_wino43(xi.transpose(1, 2).contiguous(), w, None, d).transpose(1, 2)
        emu.append(_epilogue(ye, torch.float32, bias, torch.tensor(pre, dtype=torch.float32).item(), act, Rb,
                             torch.tensor(post, dtype=torch.float32).item(), Pb, n, T, mask))
    return torch.cat(r64), torch.cat(emu)


def _check(tag, got_flat, got, direct, r64, emu, lens_l, mask):
    torch.cuda.synchronize()
    assert bool((got_flat[-TAIL:] == SENT).all()), f"{tag}: written past the end of the output"
    g, dk = got.cpu().double(), direct.cpu().double()
    e_w, e_d, e_e = (g - r64).abs().max().item(), (dk - r64).abs().max().item(), (emu.double() - r64).abs().max().item()
    floor = 2.0 * ULP * r64.abs().max().item()
    bound = max(4.0 * max(e_d, e_e), floor)
    print(f"{tag}: grouped F(4,3) err {e_w:.3e}; direct kernel {e_d:.3e}, CPU emulation {e_e:.3e}, bound {bound:.3e} (floor {floor:.3e})")
    record_measurement("wino43_rect_" + tag, err=e_w, err_direct=e_d, err_emulation=e_e, bound=bound)
    assert e_w <= bound, (tag, e_w, bound)
    if mask:
        for b, n in enumerate(lens_l):
            assert bool((got[b, n:] == 0).all()), f"{tag}: rows behind lens[{b}] = {n} are not exactly 0"
    return e_w


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [3, 7, 11])
def test_c32_stage_convs_on_the_32_column_tile(k, d):
    """C = 32: one column tile of 32, two waves over 64 quads. T = 300 = one full 256-frame tile + a partial one; lens = [T, 37]."""
    C, B, T = 32, 2, 300
    lens_l = [T, 37]
    g = torch.Generator().manual_seed(3200 + 10 * k + d)
    x = torch.randn(B, T, C, generator=g)      # rows >= lens[b] stay garbage in the device buffer
    w = torch.randn(C, C, k, generator=g) / math.sqrt(C * k)
    bias = torch.randn(C, generator=g) * 0.3
    res = torch.randn(B, T, C, generator=g)
    prev = torch.randn(B, T, C, generator=g)
    for b, n in enumerate(lens_l):             # what an accumulating launch finds behind lens: the 0 an earlier masked launch wrote
        prev[b, n:] = 0
    assert L.load().ss_wino43_conv_ok(C, k, d) == 1
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    Ww = L.pack_conv_weight(L.wino43_group_weight(w.to(DEV)))
    Wd = L.pack_conv_weight(w.to(DEV))
    bp = L.pack_bias(bias.to(DEV))
    kw = dict(B=B, T=T, Cin=C, N=C, Np=C, Kp=C, lens=lens, bias=bp, ldc=C, mask_rows=True)
    taps = [(j - (k - 1) // 2) * d for j in range(k)]
    tag = f"C32_k{k}_d{d}"

    # (1) input leaky-relu, output leaky-relu
    r64, emu = _references(x, lens_l, w, bias, k, d, 0.1, 1.0, "lrelu", None, 1.0, None, True)
    flat, got = _out_buf(torch.full((B, T, C), 9.0))
    L.wino43_conv(xd, Ww, got, k=k, dilation=d, a_lrelu=0.1, act=L.ACT_LRELU, act_slope=0.1, **kw)
    _, direct = _out_buf(torch.full((B, T, C), 7.0))
    L.conv_gemm(xd, Wd, direct, taps=taps, a_lrelu=0.1, act=L.ACT_LRELU, act_slope=0.1, **kw)
    _check(tag + "_lrelu", flat, got, direct, r64, emu, lens_l, True)
    # (2) residual in place (R == C)
    r64, emu = _references(x, lens_l, w, bias, k, d, 1.0, 1.0, None, res, 1.0, None, True)
    flat, got = _out_buf(res)
    L.wino43_conv(xd, Ww, got, k=k, dilation=d, R=got, ldr=C, **kw)
    _, direct = _out_buf(res)
    L.conv_gemm(xd, Wd, direct, taps=taps, R=direct, ldr=C, **kw)
    _check(tag + "_inplace", flat, got, direct, r64, emu, lens_l, True)
    # (3) residual, post_scale = 1/3, accumulate
    r64, emu = _references(x, lens_l, w, bias, k, d, 1.0, 1.0, None, res, 1.0 / 3.0, prev, True)
    resd = res.to(DEV)
    flat, got = _out_buf(prev)
    L.wino43_conv(xd, Ww, got, k=k, dilation=d, R=resd, ldr=C, post_scale=1.0 / 3.0, accumulate=True, **kw)
    _, direct = _out_buf(prev)
    L.conv_gemm(xd, Wd, direct, taps=taps, R=resd, ldr=C, post_scale=1.0 / 3.0, accumulate=True, **kw)
    _check(tag + "_accumulate", flat, got, direct, r64, emu, lens_l, True)


@pytest.mark.parametrize("Np", [160, 192])
def test_rectangular_k9_conv_with_gelu_and_unmasked_rows(Np):
    """Cin = 96 (three K chunks) -> N = 160, k = 9, GELU((conv + bias) / 3), mask_rows = 0, lens = [300, 5]: rows behind lens are the conv of
    the zero-extended item. Np = 160 (what ss_pack_conv_weight leaves: five 32-column tiles) and Np = 192 (zero rows appended: three 64-column
    tiles, the last one partial)."""
    Cin, N, k, d, B, T = 96, 160, 9, 1, 2, 300
    lens_l = [300, 5]
    g = torch.Generator().manual_seed(9600 + Np)
    x = torch.randn(B, T, Cin, generator=g)
    w = torch.randn(N, Cin, k, generator=g) / math.sqrt(Cin * k) * 3.0
    bias = torch.randn(N, generator=g) * 0.3
    assert L.load().ss_wino43_conv_ok4(Cin, N, k, d) == 1 and L.load().ss_wino43_conv_ok(Cin, k, d) == 0
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    xd = x.to(DEV)
    Ww = L.pack_conv_weight(L.wino43_group_weight(w.to(DEV)))
    Wd = L.pack_conv_weight(w.to(DEV))
    assert Ww.shape == (160, 3 * 6 * Cin)
    if Np > Ww.shape[0]:
        Ww = torch.cat([Ww, torch.zeros(Np - Ww.shape[0], Ww.shape[1], device=DEV)]).contiguous()
    bp = L.pack_bias(bias.to(DEV))
    kw = dict(B=B, T=T, Cin=Cin, N=N, Kp=Cin, lens=lens, bias=bp, ldc=N, mask_rows=False, act=L.ACT_GELU, pre_scale=1.0 / 3.0)
    r64, emu = _references(x, lens_l, w, bias, k, d, 1.0, 1.0 / 3.0, "gelu", None, 1.0, None, False)
    flat, got = _out_buf(torch.full((B, T, N), 9.0))
    L.wino43_conv(xd, Ww, got, k=k, dilation=d, Np=Np, **kw)
    _, direct = _out_buf(torch.full((B, T, N), 7.0))
    L.conv_gemm(xd, Wd, direct, taps=[j - 4 for j in range(k)], Np=160, **kw)
    _check(f"Cin96_N160_Np{Np}_k9_gelu", flat, got, direct, r64, emu, lens_l, False)
