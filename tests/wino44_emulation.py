"""The grouped Winograd F(4,4) arithmetic of stylesinger_amd/csrc/wino44_conv.hip, restated for the CPU tests and the GPU test bounds.

Point set (recorded here as the one chosen): {0, 1, -1, 2, -2, 1/2, inf}. With it the output transform A^T has only powers of two. The three
matrices are built from the points by the Cook-Toom rule in exact fractions (f44_matrices); conv1d_wino44 runs the grouped form in float32 with
the shared-term input transform the kernel uses (same terms, same fma grouping), not a matrix product."""
from fractions import Fraction as Fr

import numpy as np
import torch
import torch.nn.functional as F

POINTS = (Fr(0), Fr(1), Fr(-1), Fr(2), Fr(-2), Fr(1, 2))   # and the point at infinity


def _polymul(a, b):
    r = [Fr(0)] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] += x * y
    return r


def f44_matrices():
    """(A^T [4][7], G [7][4], B^T [7][7]) as float64 arrays, exact up to the final conversion: y = A^T [(G g) * (B^T d)] is the 4-tap
    correlation y_i = sum_k g_k d_(i+k), i = 0..3, of seven inputs."""
    n = len(POINTS)
    BT, G = [], []
    for j, p in enumerate(POINTS):
        poly, norm = [Fr(1)], Fr(1)
        for l, q in enumerate(POINTS):
            if l != j:
                poly = _polymul(poly, [-q, Fr(1)])   # coefficients by rising power
                norm *= p - q
        BT.append(poly + [Fr(0)])
        G.append([p ** i / norm for i in range(4)])
    poly = [Fr(1)]
    for q in POINTS:
        poly = _polymul(poly, [-q, Fr(1)])
    BT.append(poly)
    G.append([Fr(0), Fr(0), Fr(0), Fr(1)])
    AT = [[p ** i for p in POINTS] + [Fr(1) if i == 3 else Fr(0)] for i in range(4)]
    assert len(BT) == n + 1 == 7
    return tuple(np.array([[float(v) for v in row] for row in m], dtype=np.float64) for m in (AT, G, BT))


def _fma(c, a, b):
    """c * a + b elementwise; float32 tensors, one rounding where the backend fuses (as the kernel's v_fma_f32), two otherwise."""
    return torch.addcmul(b, a, torch.tensor(c, dtype=a.dtype))


def input_transform(r):
    """seven raw rows r[0..6] -> the seven components c[0..6], by the shared terms of wino44_conv.hip."""
    Pv = _fma(2.0, r[1], _fma(-4.0, r[2], _fma(-0.5, r[3], r[4])))
    Pu = _fma(2.0, r[2], _fma(-4.0, r[3], _fma(-0.5, r[4], r[5])))
    Qv = _fma(0.5, r[1], _fma(-0.5, r[3], r[4] - r[2]))
    Qu = _fma(0.5, r[2], _fma(-0.5, r[4], r[5] - r[3]))
    c5 = _fma(4.0, r[1], _fma(-5.0, r[3], r[5]))
    F0 = _fma(4.0, r[0], _fma(-5.0, r[2], r[4]))
    E2 = _fma(4.0, r[2], _fma(-5.0, r[4], r[6]))
    return [_fma(-0.5, F0, c5), Pu + Pv, Pu - Pv, _fma(2.0, Qv, Qu), _fma(-2.0, Qv, Qu), c5, _fma(-0.5, c5, E2)]


def group_weight64(w):
    """[Co][Ci][k] -> [Co][Ci][7 * ceil(k/4)] in float64: the G matrix on every group of four taps (zero padded at the end)."""
    Co, Ci, k = w.shape
    Gn = (k + 3) // 4
    wp = torch.zeros(Co, Ci, 4 * Gn, dtype=torch.float64)
    wp[..., :k] = w.double()
    Gm = torch.from_numpy(f44_matrices()[1])
    return torch.einsum("jt,oigt->oigj", Gm, wp.view(Co, Ci, Gn, 4)).reshape(Co, Ci, 7 * Gn)


def conv1d_wino44(x, w, bias, dilation):
    """x [B, Ci, T], w [Co, Ci, k] (k odd), 'same' padding: grouped F(4,4) in fp32 - quads (t, t+d, t+2d, t+3d) inside groups of 4 d frames,
    seven accumulators over all tap groups and channels, one output transform."""
    B, Ci, T = x.shape
    Co, _, k = w.shape
    d = dilation
    Gn = (k + 3) // 4
    gw = group_weight64(w).float().view(Co, Ci, Gn, 7)
    Tq = -(-T // (4 * d)) * 4 * d
    lo = (k - 1) // 2 * d
    hi = (4 * Gn - 1) * d - lo + 3 * d + (Tq - T)
    xp = F.pad(x, (lo, hi))
    t = torch.arange(Tq).view(-1, 4, d)[:, 0, :].reshape(-1)
    acc = [torch.zeros(B, Co, t.numel(), dtype=torch.float32) for _ in range(7)]
    for g in range(Gn):
        c = input_transform([xp[:, :, t + (4 * g + i) * d] for i in range(7)])   # frames t - lo + (4 g + i) d of the unpadded signal
        for j in range(7):
            acc[j] = acc[j] + torch.einsum("oc,bcq->boq", gw[:, :, g, j], c[j])
    m = acc
    s12, d12 = m[1] + m[2], m[1] - m[2]
    s34, d34 = m[3] + m[4], m[3] - m[4]
    z0 = (m[0] + s12) + (s34 + m[5])
    z1 = _fma(0.5, m[5], _fma(2.0, d34, d12))
    z2 = _fma(0.25, m[5], _fma(4.0, s34, s12))
    z3 = _fma(0.125, m[5], _fma(8.0, d34, d12)) + m[6]
    out = torch.empty(B, Co, Tq, dtype=torch.float32)
    for o, z in enumerate((z0, z1, z2, z3)):
        out[:, :, t + o * d] = z
    out = out[:, :, :T]
    return out + bias.view(1, -1, 1) if bias is not None else out
