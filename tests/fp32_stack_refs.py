"""Plain float64 statements of the fp32 denoiser stack's three launches per residual layer - the F(4,3) / F(2,3) / direct gate, the residual
projection and the skip (store) GEMM - written from the contract in include/stylesinger_hip.h, not from the kernels, for
tests/test_gpu_fp32_stack_edges.py. No GPU, no HIP library; tests/test_fp32_stack_refs_cpu.py checks the statements against a second
statement, asserts from `CASES` alone that the table reaches the forms and row edges it claims, and that the bars of the GPU test can see the
faults the cases exist for.

The operation (ss_conv_gemm_args):
  A' = a + a_bias on rows in [0, len) of an item and exactly 0 elsewhere (gate cases; the other launches take no a_bias)
  gate:       C = gate_mode(conv3_dilated(A', w) + bias + E), every row of [0, T) when mask_rows = 0 (rows in [len, T) are the gate of what the
              zero-extended input and E give there), 0 in rows >= len when mask_rows = 1
  projection: C = (R + A' . W^T + bias) * post_scale (C aliases R); RESSKIP also writes the skip half C2 (+)= A' . W2^T + bias2
  store:      C = act(A' . W^T + bias)
What the A operand holds in rows >= len never reaches a result: `reference` zero-extends the item ITSELF.

Geometry, from the sources (frames = rows of an item):
  ss_wino43_gate        wino43_gate.hip  BQ = 64 quads per row tile = 256 frames
  ss_wino43_gate16 / x  wino43_gate16.hip / wino43_gate16x.hip  BQ = 16 * MT quads, MT in 1, 2, 3 (mt = 0: ss_wino43_gate16_pick)
  ss_wino_gate          wino_gate.hip  BP = 64 pairs = 128 frames
  ss_gemm16_*           gemm16.hip  BM = 16 * MT rows, MT in 2 (projection only), 4, 6, 8 (mt = 0: ss_gemm16_pick)
  ss_conv_gemm          conv_gemm_kernel.h launch_tile: SS_TILE_128x128 / 128x64 / 128x32 = 128 rows, SS_TILE_64x128 / 64x64 = 64 rows
  quad -> frames        device_prims.h wino43_frame(q, d) = q + 3 * (q & ~(d - 1)): quads are formed inside groups of 4 d frames, quad q of group
                        g = q / d covers the frames 4 d g + q % d + {0, d, 2 d, 3 d}; a tile of BQ quads is 4 BQ contiguous frames when d divides BQ
                        (F(2,3): groups of 2 d frames, pairs t, t + d).
"""
import math
import zlib

import torch
import torch.nn.functional as F

from hgemm_refs import pack_addend as _pack_addend32

POISON = 1000.0
SENTINEL = 7.0
POST_SCALE = 0.5 ** 0.5
N_CU = 256                       # compute units of the MI355X: what the two pick models below are evaluated with (the GPU test asserts the library agrees)
WINO43 = ("gate16", "gate16x", "gate43")
WINO = WINO43 + ("wino23",)
CONV_TILE_ROWS = {1: 128, 2: 64, 3: 64, 4: 128, 5: 128}   # SS_TILE_* -> BM

# the transform matrices (tools/wino43_numerics.py; wino43_gate.hip / wino_gate.hip state the same rows): input B^T, weights G, output A^T
BT4 = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], dtype=torch.float64)
AT4 = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)
BT2 = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
G2 = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
AT2 = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------------------
# the pick models (wino43_gate16.hip ss_wino43_gate16_pick, gemm16.hip ss_gemm16_pick) at N_CU compute units
# ------------------------------------------------------------------------------------------------------------------------------
def gate16_pick(B, T, Np, d, n_cu=N_CU):
    quads, n_tiles = cdiv(T, 4 * d) * d, Np // 64

    def layers(bq):
        return cdiv(cdiv(quads, bq) * B * n_tiles, n_cu)
    if layers(64) >= 6:
        return 0
    best, best_cost = 0, 4 * layers(64)
    tiny = cdiv(quads, 32) * B * n_tiles <= n_cu
    for mt in range(3, 0 if tiny else 1, -1):
        cost = mt * layers(16 * mt)
        if cost < best_cost or (cost == best_cost and best != 0):
            best, best_cost = mt, cost
    return best


def gemm16_pick(B, T, N, n_cu=N_CU):
    n_tiles = cdiv(N, 64)
    tiny = cdiv(T, 64) * B * n_tiles * 2 <= n_cu
    best, best_cost = 4, -1
    for mt in range(8, 1 if tiny else 3, -2):
        cost = mt * cdiv(cdiv(T, 16 * mt) * B * n_tiles, n_cu)
        if best_cost < 0 or cost < best_cost:
            best, best_cost = mt, cost
    return best


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
CASES = {}


def _add(name, family, kernel, *, B, T, lens, K, N, d=0, mt=0, tile=0, ksplit=0, Np=None, group_size=0, gate_mode=0, mask_rows=False, bias=True,
         a_bias=False, act="none", accumulate=False, seed=0, scale=None):
    assert name not in CASES, name
    assert lens is None or (len(lens) == B and all(1 <= n <= T for n in lens)), (name, lens, T)
    if Np is None:
        Np = 2 * cdiv(N, 32) * 32 if family == "gate" else cdiv(N, 32) * 32
    if scale is None:      # see make_inputs
        scale = 1.0 if kernel not in WINO43 else 0.5 if K <= 64 else 0.25
    CASES[name] = dict(name=name, family=family, kernel=kernel, B=B, T=T, lens=None if lens is None else tuple(lens), K=K, N=N, Np=Np, d=d, mt=mt,
                       tile=tile, ksplit=ksplit, group_size=group_size, gate_mode=gate_mode, mask_rows=mask_rows, bias=bias, a_bias=a_bias, act=act,
                       accumulate=accumulate, seed=seed, scale=scale)


def case_lens(case):
    return list(case["lens"]) if case["lens"] is not None else [case["T"]] * case["B"]


def n_groups(case):
    return cdiv(case["B"], case["group_size"]) if case["group_size"] else 1


def item_group(case, b):
    return b // case["group_size"] if case["group_size"] else 0


def effective_mt(case):
    """the row-tile count the launch runs with (mt = 0: the library's pick; 0 from the gate's pick = the 32x32x2 kernel; the store kernels
    have no 32-row tile)"""
    k, mt = case["kernel"], case["mt"]
    if k in ("gate16", "gate16x") and mt == 0:
        mt = gate16_pick(case["B"], case["T"], case["Np"], case["d"])
        if k == "gate16x" and mt in (0, 1):
            mt = 3
    if k in ("res", "store", "splitk", "store16x") and mt == 0:
        mt = 4 if k == "splitk" else gemm16_pick(case["B"], case["T"], case["N"])
        if k != "res" and mt == 2:
            mt = 4 if k != "store16x" else 8
    return mt


def tile_frames(case):
    """frames (rows) of one row tile of the kernel form the case runs on"""
    k = case["kernel"]
    if k in ("gate16", "gate16x"):
        mt = effective_mt(case)
        return 256 if mt == 0 else 64 * mt
    if k == "gate43":
        return 256
    if k == "wino23":
        return 128
    if k in ("conv_gate", "resskip", "conv_store"):
        return CONV_TILE_ROWS[case["tile"]]
    return 16 * effective_mt(case)


def group_frames(case):
    """frames of one Winograd frame group (4 d for F(4,3), 2 d for F(2,3)); the row tile for the other kernels"""
    k = case["kernel"]
    return 4 * case["d"] if k in WINO43 else 2 * case["d"] if k == "wino23" else tile_frames(case)


def n_row_tiles(case):
    k, T, B = case["kernel"], case["T"], case["B"]
    if k in WINO:
        g = group_frames(case)
        per = g // case["d"]                                          # frames per quad / pair
        return cdiv(cdiv(T, g) * case["d"], tile_frames(case) // per) * B
    return cdiv(T, tile_frames(case)) * B


def form(case):
    """the kernel form a case runs on: what the coverage tests group by"""
    k = case["kernel"]
    if k in ("gate16", "gate16x", "res", "store", "store16x"):
        return f"{k}-mt{case['mt']}"
    if k == "splitk":
        return f"splitk-k{case['ksplit']}"
    if k in ("wino23", "conv_gate", "resskip", "conv_store"):
        return f"{k}-tile{case['tile']}"
    return k


def place(case, t):
    """frame t -> (row tile, frame group, position in the group) as the kernel of the case forms them"""
    k = case["kernel"]
    if k in WINO:
        g, d = group_frames(case), case["d"]
        unit = (t // g) * d + t % d                                      # quad / pair index (wino43_frame inverted)
        return unit // (tile_frames(case) // (g // d)), t // g, t % g
    f = tile_frames(case)
    return t // f, t // f, t % f


def worst_row(case, err_rows):
    """err_rows: list per item of per-row errors [T] -> (error, item, frame, tile, frame group, position in group) of the worst row"""
    e, b, t = max((float(v.max()), b, int(v.argmax())) for b, v in enumerate(err_rows))
    return (e, b, t) + place(case, t)


def _edge_lens(f, d):
    """two items x three lens around the joints of a row tile of f frames at dilation d (d = 0: one tap): production form and masked form.
    Together: len on a joint, one past it (the last tile reached only through the halo), 1 (< d), and len mod 4 d in each quarter."""
    if d == 0:
        return (f, f + 1, 1), (2 * f - 1, 1, f)
    return (f, f + 1, 2 * f - d), (1, f + d, f + 2 * d + d // 2)


def _gate_forms():
    out = [("gate16", dict(mt=m)) for m in (1, 2, 3, 0)] + [("gate43", {})] + [("wino23", dict(tile=t)) for t in (2, 3)]
    return out + [("gate16x", dict(mt=m)) for m in (2, 3)]


def _build_cases():
    # ---- gate: every Winograd kernel form x dilation in production form (no bias, no row mask, a_bias) and masked form (bias, row mask)
    for kern, sel in _gate_forms():
        tag = form(dict(kernel=kern, mt=sel.get("mt", 0), tile=sel.get("tile", 0)))
        for d in (1, 2, 4, 8):
            probe = dict(kernel=kern, B=3, T=1, Np=128, d=d, mt=sel.get("mt", 0), tile=sel.get("tile", 0))
            f = tile_frames(dict(probe, T=3 * 64))                        # mt = 0 picks the 16-quad tiling at every size of this table
            T = 2 * f + 4 * d + 3
            assert tile_frames(dict(probe, T=T)) == f
            prod, masked = _edge_lens(f, d)
            C = 256 if (d == 4 and kern in ("gate16", "gate43") and sel.get("mt", 2) == 2) else 64
            _add(f"gate-{tag}-d{d}-prod", "gate", kern, B=3, T=T, lens=prod, K=C, N=C, d=d, bias=False, a_bias=True, mask_rows=False,
                 gate_mode=1 if d == 2 else 0, **sel)
            _add(f"gate-{tag}-d{d}-masked", "gate", kern, B=3, T=T, lens=masked, K=C, N=C, d=d, bias=True, a_bias=True, mask_rows=True,
                 gate_mode=1 if d == 8 else 0, **sel)
        f = tile_frames(dict(kernel=kern, B=2, T=192, Np=128, d=2, mt=sel.get("mt", 0), tile=sel.get("tile", 0)))
        _add(f"gate-{tag}-d2-prod-nolens", "gate", kern, B=2, T=f + 9, lens=None, K=64, N=64, d=2, bias=False, a_bias=True, **sel)
        _add(f"gate-{tag}-d4-prod-groups", "gate", kern, B=3, T=f + 21, lens=(f, f + 21, 5), K=192, N=192, d=4, bias=True, a_bias=True, group_size=2, **sel)
        # N < Cin with a whole column tile (and, in the first, whole lanes) beyond N: the col_ok path
        _add(f"gate-{tag}-d1-prod-narrow", "gate", kern, B=2, T=f + 6, lens=(f + 6, f - 3), K=64, N=24, Np=128, d=1, bias=False, a_bias=True, **sel)
    # the frame group larger than the tile (mt = 1, d = 16 and 32) and a tile that is no whole number of groups (mt = 3, d = 32: 48 quads = 1.5
    # groups) resp. three whole groups per tile (mt = 3, d = 16)
    _add("gate-gate16-mt1-d16-prod", "gate", "gate16", B=3, T=2 * 64 + 35, lens=(64, 65, 15), K=64, N=64, d=16, mt=1, bias=False, a_bias=True)
    _add("gate-gate16-mt1-d32-prod", "gate", "gate16", B=3, T=2 * 128 + 67, lens=(128, 161, 31), K=64, N=64, d=32, mt=1, bias=False, a_bias=True)
    _add("gate-gate16-mt3-d16-prod", "gate", "gate16", B=3, T=192 + 64 + 35, lens=(192, 193, 15), K=64, N=64, d=16, mt=3, bias=False, a_bias=True)
    _add("gate-gate16-mt3-d32-masked", "gate", "gate16", B=3, T=2 * 128 + 67, lens=(192, 129, 31), K=64, N=64, d=32, mt=3, bias=True, a_bias=True,
         mask_rows=True)
    # the direct conv (taps -d, 0, d) on its three gate tiles
    for tile in (1, 2, 4):
        f = CONV_TILE_ROWS[tile]
        for d in (1, 8):
            prod, masked = _edge_lens(f, d)
            _add(f"gate-conv_gate-tile{tile}-d{d}-prod", "gate", "conv_gate", B=3, T=2 * f + 4 * d + 3, lens=prod, K=64, N=64, d=d, tile=tile,
                 bias=False, a_bias=True, gate_mode=1 if d == 1 else 0)
            _add(f"gate-conv_gate-tile{tile}-d{d}-masked", "gate", "conv_gate", B=3, T=2 * f + 4 * d + 3, lens=masked, K=64, N=64, d=d, tile=tile,
                 bias=True, a_bias=True, mask_rows=True, gate_mode=1 if d == 8 else 0)
        _add(f"gate-conv_gate-tile{tile}-d2-prod-nolens", "gate", "conv_gate", B=2, T=f + 9, lens=None, K=64, N=64, d=2, tile=tile, bias=False, a_bias=True)
        _add(f"gate-conv_gate-tile{tile}-d4-prod-groups", "gate", "conv_gate", B=3, T=f + 21, lens=(f, f + 21, 5), K=192, N=192, d=4, tile=tile,
             bias=True, a_bias=True, group_size=2)
    # ---- residual projection: ss_gemm16_res (and, in the GPU test, its fetch-order form) and ss_conv_gemm RESSKIP
    for mt in (0, 2, 4, 6, 8):
        f = 16 * effective_mt(dict(kernel="res", mt=mt, B=3, T=64, N=192))
        for K in (192, 256):
            for mask in (False, True):
                lens = _edge_lens(f, 0)[int(mask)]
                _add(f"proj-res-mt{mt}-k{K}-{'masked' if mask else 'prod'}", "proj", "res", B=3, T=2 * f + 13, lens=lens, K=K, N=K, mt=mt, mask_rows=mask,
                     group_size=2 if K == 192 else 0)
        _add(f"proj-res-mt{mt}-k256-prod-nolens", "proj", "res", B=2, T=f + 5, lens=None, K=256, N=256, mt=mt)
    for tile in (1, 2, 3, 4):
        f = CONV_TILE_ROWS[tile]
        for acc in (False, True):
            K = 256 if acc else 192
            _add(f"proj-resskip-tile{tile}-k{K}-acc{int(acc)}", "proj", "resskip", B=3, T=2 * f + 13, lens=_edge_lens(f, 0)[int(acc)], K=K, N=2 * K,
                 tile=tile, accumulate=acc, mask_rows=acc, group_size=0 if acc else 2)
        _add(f"proj-resskip-tile{tile}-k192-acc1-prod-nolens", "proj", "resskip", B=2, T=f + 5, lens=None, K=192, N=384, tile=tile, accumulate=True)
    # ---- skip / store GEMM: K = 32 (1 chunk), 96 (3), 640 (20); N = 64, 80 (partial column tile), 192
    shapes = [(32, 64, "none", True), (96, 80, "relu", False), (640, 192, "relu", True), (640, 80, "none", False)]
    forms = [("store", dict(mt=m)) for m in (0, 4, 6, 8)] + [("store16x", dict(mt=4))] + [("conv_store", dict(tile=t)) for t in (1, 2, 3, 4, 5)]
    forms += [("splitk", dict(ksplit=2)), ("splitk", dict(ksplit=5))]
    for kern, sel in forms:
        probe = dict(kernel=kern, mt=sel.get("mt", 0), tile=sel.get("tile", 0), ksplit=sel.get("ksplit", 0), B=3, T=64, N=64)
        f, tag = tile_frames(probe), form(probe)
        for K, N, act, mask in shapes:
            if kern == "splitk" and K // 32 < sel["ksplit"]:
                continue
            _add(f"store-{tag}-k{K}-n{N}-{act}-{'masked' if mask else 'prod'}", "store", kern, B=3, T=2 * f + 13, lens=_edge_lens(f, 0)[int(mask)], K=K, N=N,
                 act=act, mask_rows=mask, group_size=2 if (K, N) == (640, 192) else 0, **sel)
        _add(f"store-{tag}-k640-n64-relu-prod-nolens", "store", kern, B=2, T=f + 5, lens=None, K=640, N=64, act="relu", **sel)


_build_cases()


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (seeded, CPU) with the distributions of the kernels' other unit tests
# ------------------------------------------------------------------------------------------------------------------------------
def data_key(case):
    """everything of a case but the kernel form it runs on"""
    return repr(sorted((k, v) for k, v in case.items() if k not in ("name", "kernel", "mt", "tile", "ksplit")))


def make_inputs(case):
    """x ~ N(0, 1) and a_bias ~ N(0, 1), both times case["scale"]; w ~ N(0, 1) / sqrt(taps K); bias ~ 0.3 N (gate) or 0.1 N; E ~ N(0, 1); R ~ N(0, 1).
    scale: 1 but for the F(4,3) kernels. Their fp32 transforms alone (output transform: 8 x the difference of two accumulators) put the worst of
    10^5 outputs at 4e-6 .. 1e-5 with unit inputs, K = 64 .. 256 - at the 1e-5 bar itself, which the kernels' other unit tests meet at their
    sizes with nothing to spare. A failure of the GPU test has to be the kernel's, not the data's (the fp32 restatement stays within half the bar:
    tests/test_fp32_stack_refs_cpu.py), so the activations are scaled, 0.5 at K = 64 and 0.25 at K >= 192, and the bar stays. E keeps the gate
    away from saturation; a wrong coefficient, tap, row or column still moves an output by 1e-2 and more."""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(data_key(case).encode()))
    B, T, K, N, G, fam = case["B"], case["T"], case["K"], case["N"], n_groups(case), case["family"]
    if fam == "gate":
        d = dict(x=torch.randn(B, T, K, generator=g) * case["scale"], w=torch.randn(G, 2 * N, K, 3, generator=g) / math.sqrt(3 * K),
                 E=torch.randn(B, T, 2 * N, generator=g))
        d["bias"] = torch.randn(G, 2 * N, generator=g) * 0.3 if case["bias"] else None
        d["a_bias"] = torch.randn(G, K, generator=g) * case["scale"] if case["a_bias"] else None
        return d
    d = dict(x=torch.randn(B, T, K, generator=g), w=torch.randn(G, N, K, generator=g) / math.sqrt(K), bias=torch.randn(G, N, generator=g) * 0.1)
    if fam == "proj":
        d["R"] = torch.randn(B, T, K, generator=g)
        if case["kernel"] == "resskip":
            d["C2"] = torch.randn(B, T, N - K, generator=g)
    return d


def pack_addend(E, N, Np=None):
    """[..., 2 N] (first gate operand | second) -> the packed column order [..., Np]: block 2 p = channels [32 p, 32 p + 32) of the first half,
    block 2 p + 1 = the same channels of the second; channels >= N of the last pair of blocks are 0. N % 32 == 0: hgemm_refs.pack_addend."""
    Np = 2 * cdiv(N, 32) * 32 if Np is None else Np
    if N % 32 == 0 and Np == 2 * N:
        return _pack_addend32(E, N)
    out = torch.zeros(*E.shape[:-1], Np, dtype=E.dtype)
    for p in range(cdiv(N, 32)):
        n = min(32, N - 32 * p)
        out[..., 64 * p:64 * p + n] = E[..., 32 * p:32 * p + n]
        out[..., 64 * p + 32:64 * p + 32 + n] = E[..., N + 32 * p:N + 32 * p + n]
    return out


def tail_mask(case):
    """[B, T] bool: rows >= lens[b]"""
    return torch.arange(case["T"])[None, :] >= torch.tensor(case_lens(case))[:, None]


def with_tail(case, x, poison):
    """x [B, T, W] with rows >= lens[b] zeroed (poison = False) or filled with +-POISON in a checkerboard (sign alternating by row + column)"""
    x = x.clone()
    m = tail_mask(case)
    if poison:
        sign = 1.0 - 2.0 * ((torch.arange(x.shape[1])[:, None] + torch.arange(x.shape[2])[None, :]) % 2).to(x.dtype)
        x[m] = (POISON * sign).expand(x.shape[0], -1, -1)[m]
    else:
        x[m] = 0.0
    return x


# ------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------
def _gate(z, N, gate_mode):
    if gate_mode == 0:
        return torch.sigmoid(z[..., :N]) * torch.tanh(z[..., N:])
    return torch.tanh(z[..., :N]) * torch.sigmoid(z[..., N:])


def padded_input(case, inp, x, b, dtype=torch.float64, *, leak=False, tail_bias=False):
    """A' of item b, [T, K]: x + a_bias on rows < len, 0 elsewhere. Deliberately wrong variants: leak = rows in [len, T) are read as they are;
    tail_bias = rows in [len, T) hold a_bias (the validity sums of the input transform counting padding rows)"""
    n, g = case_lens(case)[b], item_group(case, b)
    a = x[b].to(dtype)
    ab = inp["a_bias"][g].to(dtype) if inp.get("a_bias") is not None else None
    live = (torch.arange(case["T"]) < n)[:, None]
    v = a + ab if ab is not None else a
    if leak:
        return torch.where(live, v, a)
    if tail_bias and ab is not None:
        return torch.where(live, v, ab.expand_as(a))
    return torch.where(live, v, torch.zeros((), dtype=dtype))


def _conv_taps(ap, w, d, drop=None):
    """explicit tap loop: z[t] = sum_j A'[t + (j - 1) d] . w[:, :, j]^T; drop = (frames, tap): that tap is left out at those frames"""
    T = ap.shape[0]
    z = torch.zeros(T, w.shape[0], dtype=ap.dtype)
    for j in range(3):
        src = torch.arange(T) + (j - 1) * d
        ok = (src >= 0) & (src < T)
        if drop is not None and drop[1] == j:
            ok = ok & ~drop[0]
        z += torch.where(ok[:, None], ap[src.clamp(0, T - 1)], torch.zeros((), dtype=ap.dtype)) @ w[:, :, j].t()
    return z


def joint_frames(case):
    """[T] bool: the first frame past every row-tile joint (and frame 0 of no tile: t > 0)"""
    t = torch.arange(case["T"])
    f = tile_frames(case)
    return (t % f == 0) & (t > 0)


def reference(case, inp, x=None, *, how="conv1d", leak=False, drop_tap=False, tail_bias=False):
    """float64 outputs of the case, dict name -> [B, T, N] (C; RESSKIP also C2). x: the A operand (default inp["x"]); what it holds in rows >=
    len must not matter. how: "conv1d" / "taps" (gate), "matmul" / "rows" (the others): two statements of the same operation.
    Deliberately wrong variants (tests/test_fp32_stack_refs_cpu.py): leak, tail_bias (see padded_input; without an a_bias tail_bias leaves the
    epilogue bias out of the rows >= len), drop_tap (tap -d missing at the first frame past every tile joint)."""
    x = inp["x"] if x is None else x
    B, T, K, N, fam = case["B"], case["T"], case["K"], case["N"], case["family"]
    lens = case_lens(case)
    out = {}
    for b in range(B):
        g = item_group(case, b)
        live = (torch.arange(T) < lens[b])[:, None]
        keep = live if case["mask_rows"] else torch.ones(T, 1, dtype=torch.bool)
        zero = torch.zeros((), dtype=torch.float64)
        ap = padded_input(case, inp, x, b, leak=leak, tail_bias=tail_bias)
        w = inp["w"][g].double()
        bias = inp["bias"][g].double() if inp.get("bias") is not None else None
        if bias is not None and tail_bias and inp.get("a_bias") is None:
            bias = torch.where(live, bias.expand(T, -1), zero)
        if fam == "gate":
            d = case["d"]
            if how == "taps" or drop_tap:
                z = _conv_taps(ap, w, d, drop=(joint_frames(case), 0) if drop_tap else None)
            else:
                z = F.conv1d(ap.t()[None], w, None, padding=d, dilation=d)[0].t()
            if bias is not None:
                z = z + bias
            res = dict(C=_gate(z + inp["E"][b].double(), N, case["gate_mode"]))
        else:
            if how == "rows":
                v = torch.zeros(T, N, dtype=torch.float64)
                v[:lens[b]] = torch.einsum("tk,nk->tn", ap[:lens[b]], w)
            else:
                v = ap @ w.t()
            v = v + bias
            if fam == "store":
                res = dict(C=torch.relu(v) if case["act"] == "relu" else v)
            elif case["kernel"] == "res":
                res = dict(C=(inp["R"][b].double() + v) * POST_SCALE)
            else:
                res = dict(C=(inp["R"][b].double() + v[:, :K]) * POST_SCALE, C2=v[:, K:] + (inp["C2"][b].double() if case["accumulate"] else 0.0))
        for k, v in res.items():
            out.setdefault(k, []).append(torch.where(keep, v, zero))
    return {k: torch.stack(v) for k, v in out.items()}


def fp32_restatement(case, inp):
    """the arithmetic of the kernel family in fp32 on the CPU: Winograd kernels = input, weight and output transforms in fp32, products and sums
    in fp32 (one matmul per component); the others = plain fp32 matmul / conv. Same outputs as `reference`, as fp32 tensors."""
    B, T, K, N, fam, k = case["B"], case["T"], case["K"], case["N"], case["family"], case["kernel"]
    lens = case_lens(case)
    out = {}
    for b in range(B):
        g = item_group(case, b)
        live = (torch.arange(T) < lens[b])[:, None]
        keep = live if case["mask_rows"] else torch.ones(T, 1, dtype=torch.bool)
        ap = padded_input(case, inp, inp["x"], b, dtype=torch.float32)
        w = inp["w"][g]
        bias = inp["bias"][g] if inp.get("bias") is not None else None
        if fam == "gate":
            d = case["d"]
            if k in WINO:
                BT, G, AT = (BT4, G4, AT4) if k in WINO43 else (BT2, G2, AT2)
                m, a = AT.shape
                wt = torch.einsum("ak,nck->anc", G.float(), w)
                grp = m * d
                Tp = cdiv(T, grp) * grp
                xp = F.pad(ap, (0, 0, d, Tp - T + (a - 2) * d))
                t0 = (torch.arange(Tp // grp)[:, None] * grp + torch.arange(d)[None, :]).reshape(-1)
                rows = torch.stack([xp[t0 + i * d] for i in range(a)], 0)
                comp = torch.einsum("ji,iqc->jqc", BT.float(), rows)
                mm = torch.einsum("jqc,jnc->jqn", comp, wt)
                y = torch.einsum("oj,jqn->oqn", AT.float(), mm)
                z = torch.zeros(Tp, 2 * N)
                for o in range(m):
                    z[t0 + o * d] = y[o]
                z = z[:T]
            else:
                z = F.conv1d(ap.t()[None], w, None, padding=d, dilation=d)[0].t()
            if bias is not None:
                z = z + bias
            res = dict(C=_gate(z + inp["E"][b], N, case["gate_mode"]))
        else:
            v = ap @ w.t() + bias
            if fam == "store":
                res = dict(C=torch.relu(v) if case["act"] == "relu" else v)
            elif k == "res":
                res = dict(C=(inp["R"][b] + v) * torch.tensor(POST_SCALE, dtype=torch.float32))
            else:
                res = dict(C=(inp["R"][b] + v[:, :K]) * torch.tensor(POST_SCALE, dtype=torch.float32),
                           C2=v[:, K:] + (inp["C2"][b] if case["accumulate"] else 0.0))
        for kk, v in res.items():
            out.setdefault(kk, []).append(torch.where(keep, v, torch.zeros(())))
    return {kk: torch.stack(v) for kk, v in out.items()}


# ------------------------------------------------------------------------------------------------------------------------------
# the bars of the GPU test: the ones the project already uses for the same kernel (max abs against float64)
# ------------------------------------------------------------------------------------------------------------------------------
def bars(case):
    """F(4,3) gate in any fp32 form 1e-5 (tests/test_gpu_kernels.py, outputs <= 500 k); F(2,3) gate 5e-6 (same file); ss_conv_gemm GATE / STORE /
    RESSKIP 2e-5; ss_gemm16_res 2e-5, ss_gemm16_store, its split-K form and ss_gemm16x_store 3e-5 (tests/test_gpu_round3.py, test_gpu_round4.py);
    ss_wino43_gate16x 2e-5 (test_gate16x_split_bf16_products_are_fp32_grade)."""
    k = case["kernel"]
    assert case["B"] * case["T"] * case["N"] <= 500000
    if k in ("gate16", "gate43"):
        return 1e-5
    if k == "wino23":
        return 5e-6
    if k in ("conv_gate", "conv_store", "resskip", "res", "gate16x"):
        return 2e-5
    return 3e-5
