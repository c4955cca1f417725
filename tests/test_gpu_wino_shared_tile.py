"""ss_wino44_conv with the transformed input tile shared between the tap groups: the halo rows and the shifted fragment reads.

One A tile of 64 + (G - 1) d quad rows per K chunk serves all G tap groups (group g reads the tile rows g d further), so what is new is
the halo behind the 64 quads of a tile and the row shift of the fragment reads. B = 3 items back to back, T = 531, lens = [531, 256, 7]:
three row tiles at d = 1; item 1 ends exactly on a 256-frame tile boundary, so the halo of its first tile is all zero padding although the
buffer holds garbage there; item 2 ends inside the first quad group; the halo of an item's last tile lies in front of the next item's rows
and must read 0, never those rows. C = 64 (one 64-column tile, two K chunks), 128 (two column tiles), 32 (the 32-column tile, one K chunk:
the odd sub-position counts) and 96 (three 32-column tiles, three K chunks). Reference and bound are those of
tests/test_gpu_wino44_conv.py: 4 x the larger of the direct kernel's and the F(4,3) CPU emulation's error against float64, at least 2 fp32
ulp at the output's scale. The input holds garbage behind lens[b]; every buffer is followed by a sentinel tail. A launch with T padded to
768 must give the same bits on the rows < lens[b]."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_wino43_conv_rect as RT  # noqa: E402  (reference builder, sentinel buffers)
from conftest import record_measurement  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

DEV, TAIL, SENT, ULP = RT.DEV, RT.TAIL, RT.SENT, RT.ULP
B, T, TPAD = 3, 531, 768
LENS = [531, 256, 7]


def _check(tag, flats, got, direct, r64, emu, mask):
    torch.cuda.synchronize()
    for name, flat in flats.items():
        assert bool((flat[-TAIL:] == SENT).all()), f"{tag}: the tail behind {name} was written"
    g, dk = got.cpu().double(), direct.cpu().double()
    e_w, e_d, e_e = (g - r64).abs().max().item(), (dk - r64).abs().max().item(), (emu.double() - r64).abs().max().item()
    floor = 2.0 * ULP * r64.abs().max().item()
    bound = max(4.0 * max(e_d, e_e), floor)
    print(f"{tag}: shared-tile F(4,4) err {e_w:.3e}; direct kernel {e_d:.3e}, F(4,3) CPU emulation {e_e:.3e}, bound {bound:.3e} (floor {floor:.3e})")
    record_measurement("wino_shared_" + tag, err=e_w, err_direct=e_d, err_emulation=e_e, bound=bound)
    assert e_w <= bound, (tag, e_w, bound)
    if mask:
        for b, n in enumerate(LENS):
            assert bool((got[b, n:] == 0).all()), f"{tag}: rows behind lens[{b}] = {n} are not exactly 0"


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [7, 11])
@pytest.mark.parametrize("C", [32, 64, 96, 128])
def test_shared_tile_halo_and_shifted_reads(C, k, d):
    g = torch.Generator().manual_seed(9900 + 1000 * (C // 32) + 100 * k + 10 * d)
    x = torch.randn(B, T, C, generator=g)      # rows >= lens[b] stay garbage in the device buffer
    w = torch.randn(C, C, k, generator=g) / math.sqrt(C * k)
    bias = torch.randn(C, generator=g) * 0.3
    res = torch.randn(B, T, C, generator=g)
    assert L.wino44_conv_ok(C, k, d) == 1
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    x_flat, xd = RT._out_buf(x)
    xp = torch.randn(B, TPAD, C, generator=g) * 50.0   # the padded launch: other garbage behind lens[b], the same rows in front of it
    for b, n in enumerate(LENS):
        xp[b, :n] = x[b, :n]
    xp_flat, xpd = RT._out_buf(xp)
    Ww = L.pack_conv_weight(L.wino44_group_weight(w.to(DEV)))
    Wd = L.pack_conv_weight(w.to(DEV))
    bp = L.pack_bias(bias.to(DEV))
    taps = [(j - (k - 1) // 2) * d for j in range(k)]
    for mask in (True, False):
        kw = dict(B=B, T=T, Cin=C, N=C, Np=C, Kp=C, lens=lens, bias=bp, ldc=C, mask_rows=mask)
        tag = f"C{C}_k{k}_d{d}_{'masked' if mask else 'unmasked'}"
        # (1) the leaky-relu form: input leaky-relu, output leaky-relu
        r64, emu = RT._references(x, LENS, w, bias, k, d, 0.1, 1.0, "lrelu", None, 1.0, None, mask)
        flat, got = RT._out_buf(torch.full((B, T, C), 9.0))
        L.wino44_conv(xd, Ww, got, k=k, dilation=d, a_lrelu=0.1, act=L.ACT_LRELU, act_slope=0.1, **kw)
        _, direct = RT._out_buf(torch.full((B, T, C), 7.0))
        L.conv_gemm(xd, Wd, direct, taps=taps, a_lrelu=0.1, act=L.ACT_LRELU, act_slope=0.1, **kw)
        _check(tag + "_lrelu", dict(out=flat, x=x_flat), got, direct, r64, emu, mask)
        # the same launch with T padded to 768: the rows < lens[b] depend on the item's rows alone
        pflat, pgot = RT._out_buf(torch.full((B, TPAD, C), 5.0))
        L.wino44_conv(xpd, Ww, pgot, k=k, dilation=d, a_lrelu=0.1, act=L.ACT_LRELU, act_slope=0.1, **dict(kw, T=TPAD))
        torch.cuda.synchronize()
        assert bool((pflat[-TAIL:] == SENT).all()) and bool((xp_flat[-TAIL:] == SENT).all()), f"{tag}: padded launch wrote a tail"
        for b, n in enumerate(LENS):
            assert torch.equal(pgot[b, :n], got[b, :n]), f"{tag}: item {b}: T = {TPAD} and T = {T} differ on rows < {n}"
            if mask:
                assert bool((pgot[b, n:] == 0).all()), f"{tag}: padded launch: rows behind lens[{b}] are not exactly 0"
        # (2) the in-place-residual form (R == C)
        r64, emu = RT._references(x, LENS, w, bias, k, d, 1.0, 1.0, None, res, 1.0, None, mask)
        flat, got = RT._out_buf(res)
        L.wino44_conv(xd, Ww, got, k=k, dilation=d, R=got, ldr=C, **kw)
        _, direct = RT._out_buf(res)
        L.conv_gemm(xd, Wd, direct, taps=taps, R=direct, ldr=C, **kw)
        _check(tag + "_inplace", dict(out=flat, x=x_flat), got, direct, r64, emu, mask)
    assert torch.equal(xd.cpu(), x) and torch.equal(xpd.cpu(), xp), "an input operand was modified"
