"""ss_wino44_conv (grouped Winograd F(4,4), k = 7 | 11) against torch's float64 conv1d on the zero-extended items.

Bound, built as tests/test_gpu_wino43_conv_rect.py builds it: 4 x the larger of (a) the direct kernel's error (ss_conv_gemm on the SAME
arguments) and (b) the error of the fp32 CPU emulation of the grouped F(4,3) form, both against float64 on the same case, at least 2 fp32
ulp at the output's scale. Shapes: C = 64 (one 64-column tile) and 128 (two), C = 32 (the 32-column tile; one K chunk, so two or three
K steps: the odd count) and 96 (three 32-column tiles, nine steps at k = 11); T = 37 (shorter than one tile, no multiple of 4 d) and T = 259
(just over one 256-frame tile: the tap-group halo of tile 0 is real data, that of tile 1 runs past the item); B = 2 with ragged lens. The
input holds garbage behind lens[b]; every buffer the launch is given is followed by a sentinel tail."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_wino43_conv_rect as RT  # noqa: E402  (reference builder, sentinel buffers)
from conftest import record_measurement  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

DEV, TAIL, SENT, ULP = RT.DEV, RT.TAIL, RT.SENT, RT.ULP
LENS = {37: [37, 11], 259: [259, 101]}


def _in_buf(t):
    """A read-only operand followed by a sentinel tail: (flat, view)."""
    return RT._out_buf(t)


def _check(tag, flats, got, direct, r64, emu, lens_l, mask):
    torch.cuda.synchronize()
    for name, flat in flats.items():
        assert bool((flat[-TAIL:] == SENT).all()), f"{tag}: the tail behind {name} was written"
    g, dk = got.cpu().double(), direct.cpu().double()
    e_w, e_d, e_e = (g - r64).abs().max().item(), (dk - r64).abs().max().item(), (emu.double() - r64).abs().max().item()
    floor = 2.0 * ULP * r64.abs().max().item()
    bound = max(4.0 * max(e_d, e_e), floor)
    print(f"{tag}: grouped F(4,4) err {e_w:.3e}; direct kernel {e_d:.3e}, F(4,3) CPU emulation {e_e:.3e}, bound {bound:.3e} (floor {floor:.3e})")
    record_measurement("wino44_" + tag, err=e_w, err_direct=e_d, err_emulation=e_e, bound=bound)
    assert e_w <= bound, (tag, e_w, bound)
    if mask:
        for b, n in enumerate(lens_l):
            assert bool((got[b, n:] == 0).all()), f"{tag}: rows behind lens[{b}] = {n} are not exactly 0"


@pytest.mark.parametrize("T", [37, 259])
@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [7, 11])
@pytest.mark.parametrize("C", [32, 64, 96, 128])
def test_wino44_conv_matches_float64_in_every_epilogue_form(C, k, d, T):
    B, lens_l = 2, LENS[T]
    g = torch.Generator().manual_seed(4400 + 1000 * (C // 32) + 100 * k + 10 * d + T)
    x = torch.randn(B, T, C, generator=g)      # rows >= lens[b] stay garbage in the device buffer
    w = torch.randn(C, C, k, generator=g) / math.sqrt(C * k)
    bias = torch.randn(C, generator=g) * 0.3
    res = torch.randn(B, T, C, generator=g)
    prev_m = torch.randn(B, T, C, generator=g)
    prev_u = prev_m.clone()                    # unmasked launches accumulate onto whatever is there
    for b, n in enumerate(lens_l):             # what a masked accumulating launch finds behind lens: the 0 an earlier masked launch wrote
        prev_m[b, n:] = 0
    assert L.wino44_conv_ok(C, k, d) == 1
    lens = torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    x_flat, xd = _in_buf(x)
    r_flat, resd = _in_buf(res)
    Ww = L.pack_conv_weight(L.wino44_group_weight(w.to(DEV)))
    assert Ww.shape == (C, 7 * ((k + 3) // 4) * C)
    Wd = L.pack_conv_weight(w.to(DEV))
    bp = L.pack_bias(bias.to(DEV))
    taps = [(j - (k - 1) // 2) * d for j in range(k)]
    for mask in (True, False):
        kw = dict(B=B, T=T, Cin=C, N=C, Np=C, Kp=C, lens=lens, bias=bp, ldc=C, mask_rows=mask)
        tag = f"C{C}_k{k}_d{d}_T{T}_{'masked' if mask else 'unmasked'}"
        prev = prev_m if mask else prev_u
        # (1) input leaky-relu, output leaky-relu
        r64, emu = RT._references(x, lens_l, w, bias, k, d, 0.1, 1.0, "lrelu", None, 1.0, None, mask)
        flat, got = RT._out_buf(torch.full((B, T, C), 9.0))
        L.wino44_conv(xd, Ww, got, k=k, dilation=d, a_lrelu=0.1, act=L.ACT_LRELU, act_slope=0.1, **kw)
        _, direct = RT._out_buf(torch.full((B, T, C), 7.0))
        L.conv_gemm(xd, Wd, direct, taps=taps, a_lrelu=0.1, act=L.ACT_LRELU, act_slope=0.1, **kw)
        _check(tag + "_lrelu", dict(out=flat, x=x_flat), got, direct, r64, emu, lens_l, mask)
        # (2) residual in place (R == C)
        r64, emu = RT._references(x, lens_l, w, bias, k, d, 1.0, 1.0, None, res, 1.0, None, mask)
        flat, got = RT._out_buf(res)
        L.wino44_conv(xd, Ww, got, k=k, dilation=d, R=got, ldr=C, **kw)
        _, direct = RT._out_buf(res)
        L.conv_gemm(xd, Wd, direct, taps=taps, R=direct, ldr=C, **kw)
        _check(tag + "_inplace", dict(out=flat, x=x_flat), got, direct, r64, emu, lens_l, mask)
        # (3) residual, post_scale = 1/3, accumulate
        r64, emu = RT._references(x, lens_l, w, bias, k, d, 1.0, 1.0, None, res, 1.0 / 3.0, prev, mask)
        flat, got = RT._out_buf(prev)
        L.wino44_conv(xd, Ww, got, k=k, dilation=d, R=resd, ldr=C, post_scale=1.0 / 3.0, accumulate=True, **kw)
        _, direct = RT._out_buf(prev)
        L.conv_gemm(xd, Wd, direct, taps=taps, R=resd, ldr=C, post_scale=1.0 / 3.0, accumulate=True, **kw)
        _check(tag + "_accumulate", dict(out=flat, x=x_flat, R=r_flat), got, direct, r64, emu, lens_l, mask)
    assert torch.equal(xd.cpu(), x) and torch.equal(resd.cpu(), res), "an input operand was modified"


def test_wino44_conv_refuses_what_the_rule_excludes():
    C, T = 64, 16
    x = torch.zeros(1, T, C, device=DEV)
    out = torch.zeros(1, T, C, device=DEV)
    W = torch.zeros(C, 14 * C, device=DEV)
    for k, d in ((3, 1), (9, 1), (7, 2)):
        with pytest.raises(L.StyleSingerHipError):
            L.wino44_conv(x, W, out, k=k, dilation=d, B=1, T=T, Cin=C, N=C, Np=C, Kp=C)
    with pytest.raises(L.StyleSingerHipError):   # C = 16: no multiple of 32
        L.wino44_conv(x, W, out, k=7, dilation=1, B=1, T=T, Cin=16, N=16, Np=32, Kp=32, lda=C, ldc=C)
