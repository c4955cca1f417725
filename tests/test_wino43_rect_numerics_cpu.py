"""The grouped F(4,3) arithmetic of ss_wino43_conv at the two shapes it gained, on the CPU: the emulation
(oracle.wino_vocoder_numerics.conv1d_wino43, general in k and in Co != Ci) and plain fp32 conv1d against float64. The two error pairs are what
tests/test_gpu_wino43_conv_rect.py and the decoder test build their bounds from on their own cases; here they are recorded and held against an
a-priori bound.

A-priori bound. A direct fp32 dot product of K terms is off by at most K u S, u = 2^-24, S = sum |x_i| |w_i| (Higham, Accuracy and Stability,
3.1). The F(4,3) form computes the same sum from transformed operands: input rows combined with coefficients of absolute sum <= 10
(4 + 5 + 1), weights with absolute sum <= 1, outputs with coefficients <= 8, so every product it rounds is at most 80 times as large as the
term it stands for, plus the roundings of the transforms themselves (a few u on values of the same size): 80 (K + 8) u S covers it."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import record_measurement
from oracle.wino_vocoder_numerics import conv1d_wino43

U = 2.0 ** -24


@pytest.mark.parametrize("name,Ci,Co,k,d,T", [("ffn1_256_1024_k9", 256, 1024, 9, 1, 64), ("c32_k11_d5", 32, 32, 11, 5, 300)])
def test_grouped_f43_error_next_to_direct_fp32(name, Ci, Co, k, d, T):
    g = torch.Generator().manual_seed(4300 + k)
    x = torch.randn(2, Ci, T, generator=g)
    w = torch.randn(Co, Ci, k, generator=g) / math.sqrt(Ci * k)
    b = torch.randn(Co, generator=g) * 0.3
    pad = (k - 1) // 2 * d
    ref = F.conv1d(x.double(), w.double(), b.double(), padding=pad, dilation=d)
    e_wino = (conv1d_wino43(x, w, b, d).double() - ref).abs().max().item()
    e_direct = (F.conv1d(x, w, b, padding=pad, dilation=d).double() - ref).abs().max().item()
    S = F.conv1d(x.double().abs(), w.double().abs(), b.double().abs(), padding=pad, dilation=d).max().item()
    K = Ci * k
    print(f"{name}: grouped F(4,3) fp32 {e_wino:.3e}, direct fp32 {e_direct:.3e} vs float64; K u S = {K * U * S:.3e}")
    record_measurement("wino43_numerics_" + name, err_wino=e_wino, err_direct=e_direct, KuS=K * U * S)
    assert e_direct <= (K + 1) * U * S
    assert e_wino <= 80.0 * (K + 8) * U * S
