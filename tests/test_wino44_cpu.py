"""Grouped Winograd F(4,4) (stylesinger_amd/csrc/wino44_conv.hip) on the CPU: the algebra of the three matrices, the weight transform of the
binding, a float32 emulation of the grouped arithmetic next to the forms in use today, and the shape rule shared by pack and forward.

Point set chosen: {0, 1, -1, 2, -2, 1/2, inf} (tests/wino44_emulation.py). Max emulation error against float64 at C = 64, T = 300, input =
leaky-relu(0.1) of unit-variance noise, weights ~ N(0, 1 / (C k)), range over d = 1, 3, 5 (torch fp32 on the CPU):
    k = 7:  F(4,4) groups 2.6e-6 .. 3.4e-6   F(4,3) groups 2.4e-6 .. 2.8e-6   direct fp32 0.7e-6 .. 0.9e-6
    k = 11: F(4,4) groups 2.7e-6 .. 3.2e-6   F(4,3) groups 2.5e-6 .. 3.0e-6   direct fp32 1.1e-6 .. 1.2e-6
The test prints the figures of its own run before it asserts."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wino44_emulation as W44
from conftest import record_measurement
from oracle.wino_vocoder_numerics import conv1d_wino43
from stylesinger_amd import lib as L


def test_f44_matrices_reproduce_a_four_tap_correlation():
    AT, G, BT = W44.f44_matrices()
    assert AT.shape == (4, 7) and G.shape == (7, 4) and BT.shape == (7, 7)
    rng = np.random.default_rng(44)
    for _ in range(16):
        d, g = rng.standard_normal(7), rng.standard_normal(4)
        y = AT @ ((G @ g) * (BT @ d))
        ref = np.array([sum(g[k] * d[i + k] for k in range(4)) for i in range(4)])
        assert np.abs(y - ref).max() <= 1e-13
    # the output transform of the kernel's header comment: powers of two only
    assert np.array_equal(AT, np.array([[1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0.5, 0], [0, 1, 1, 4, 4, 0.25, 0], [0, 1, -1, 8, -8, 0.125, 1]], dtype=np.float64))


def test_shared_term_input_transform_is_the_b_matrix():
    """The terms the kernel forms (Pu, Pv, Qu, Qv, c5, F0, E2) against B^T d in float64."""
    BT = torch.from_numpy(W44.f44_matrices()[2])
    d = torch.randn(7, 5, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    c = torch.stack(W44.input_transform(list(d)))
    assert (c - torch.einsum("js,sab->jab", BT, d)).abs().max().item() <= 1e-13


@pytest.mark.parametrize("k", [7, 11])
def test_group_weight_is_the_g_matrix_in_float64_rounded_once(k):
    G = W44.f44_matrices()[1]
    assert np.abs(np.array(L.WINO44_G, dtype=np.float64) - G).max() <= 2.0 ** -53
    w = torch.randn(6, 5, k, generator=torch.Generator().manual_seed(k))
    got = L.wino44_group_weight(w)
    Gn = (k + 3) // 4
    assert got.shape == (6, 5, 7 * Gn) and got.dtype == torch.float32
    want = W44.group_weight64(w)
    # one rounding of the float64 value: at most half an ulp; the two float64 evaluations differ by a few 2^-53 relative
    assert ((got.double() - want).abs() <= want.abs() * (2.0 ** -24 + 2.0 ** -48) + 1e-300).all()
    # the zero tap behind k: the last group of k = 7 / 11 has three real taps
    wp = torch.zeros(6, 5, 4 * Gn, dtype=torch.float64)
    wp[..., :k] = w.double()
    last = torch.einsum("jt,oit->oij", torch.from_numpy(G[:, :3]), wp[..., 4 * (Gn - 1):4 * (Gn - 1) + 3])
    assert (want[..., 7 * (Gn - 1):] - last).abs().max().item() <= 1e-15


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [7, 11])
def test_grouped_f44_emulation_within_four_times_the_forms_in_use(k, d):
    C, T = 64, 300
    g = torch.Generator().manual_seed(4400 + 10 * k + d)
    x = F.leaky_relu(torch.randn(2, C, T, generator=g), 0.1)
    w = torch.randn(C, C, k, generator=g) / math.sqrt(C * k)
    pad = (k - 1) // 2 * d
    ref = F.conv1d(x.double(), w.double(), None, padding=pad, dilation=d)
    e44 = (W44.conv1d_wino44(x, w, None, d).double() - ref).abs().max().item()
    e43 = (conv1d_wino43(x, w, None, d).double() - ref).abs().max().item()
    e_direct = (F.conv1d(x, w, None, padding=pad, dilation=d).double() - ref).abs().max().item()
    print(f"k={k} d={d}: F(4,4) groups {e44:.3e}, F(4,3) groups {e43:.3e}, direct fp32 {e_direct:.3e} vs float64 (points 0, +-1, +-2, 1/2, inf)")
    record_measurement(f"wino44_numerics_k{k}_d{d}", err_f44=e44, err_f43=e43, err_direct=e_direct)
    assert e44 <= 4.0 * max(e_direct, e43)


def test_shape_rule():
    lib = L.load()
    for C in (32, 64, 96, 128, 256):
        for k in (7, 11):
            for d in (1, 3, 5):
                assert lib.ss_wino44_conv_ok(C, k, d) == 1 == L.wino44_conv_ok(C, k, d)
                assert lib.ss_wino43_conv_ok(C, k, d) == 1
    for k in (3, 5, 9):
        assert lib.ss_wino44_conv_ok(64, k, 1) == 0
    assert lib.ss_wino44_conv_ok(16, 7, 1) == 0 and lib.ss_wino44_conv_ok(48, 7, 1) == 0 and lib.ss_wino44_conv_ok(0, 11, 3) == 0
    assert lib.ss_wino44_conv_ok(64, 7, 2) == 0 and lib.ss_wino44_conv_ok(64, 11, 0) == 0
    # ss_wino43_conv_ok answers as before
    assert [lib.ss_wino43_conv_ok(C, k, d) for C, k, d in ((32, 3, 1), (64, 7, 3), (256, 11, 5), (16, 3, 1), (64, 5, 1), (64, 9, 1), (64, 7, 2))] == [1, 1, 1, 0, 0, 0, 0]
    assert lib.ss_wino43_conv_ok4(256, 1024, 9, 1) == 1
    for name in ("ss_wino44_conv", "ss_wino44_conv_ok"):
        assert name in L.declared_symbols()
