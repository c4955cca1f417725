"""Plain float64 statements of the 16-bit matrix-core GEMM family (ss_gemm_bf16 and its many-round forms ss_gemm_bf16_gate256 / _gate128 /
_tile256), written from the contract in include/stylesinger_hip.h - not from the kernels - for tests/test_gpu_hgemm_edges.py.

No GPU, no HIP library. tests/test_hgemm_refs_cpu.py checks these statements against the exact float64 operation on the unsplit operands,
and asserts from `CASES` alone that the table reaches the tile edges it claims and that the tolerances of the GPU test can see the faults
the cases exist for.

What is stated here:
  * the operand forms, bit for bit: `to_bf16_cpu` (ss_to_bf16), `split_bf16_cpu` (ss_split_bf16), `split_f16_cpu` (ss_split_f16): RNE to the
    16-bit format, second term = RNE(v - hi), the weights' power-of-two shift, and the physical layout "pairs interleaved by 32";
  * `pack_addend`: the packed (gate-interleaved) column order of the conditioner addend, of the GATE bias and of the packed weight rows;
  * `reference`: float64 "of the same terms" for GATE, RESX (fp32 stream and pair-only stream) and STORE:
        split 0: the rounded operands;  split 1: hi*hi + hi*mid + mid*hi;  split 2: (a_hi*w_hi + a_hi*w_lo) * out_scale;
        one_product: a_hi*w_hi only;  split 3 ("fp16q4", ss_gemm_bf16_gate128q / _tile256q): (a_hi*w_hi + fp4(a_hi / q_scale)*q_scale*lo_q) * out_scale
        with lo_q = the block-scaled fp4 image of the weights' lo plane (stylesinger_amd.lib.pack_gate_q4 / pack_skip_q4, which run on the host;
        the block order comes from the built library's ss_gate128q_kindex / ss_tile256q_kindex, so these cases need the library - not a GPU).
    It zero-pads outside [0, len) of every item ITSELF: what the input holds in rows >= len never reaches the result.
  * `CASES`: name -> the launch (kernel, split, epilogue, shape, lens, taps, groups, gate_mode, mask_rows), iterated by both test files.
"""
import math
import zlib

import torch

WSHIFT = 8                       # the weights' shift of the fp16 forms (StyleSingerHIP.FP16_WSHIFT): W = split_f16(w * 2^8), out_scale = 2^-8
HALO = 8                         # halo rows of the 256-row gate kernels = their largest dilation
POISON = 1000.0                  # finite, exact in bf16 and fp16
SENTINEL = 7.0
POST_SCALE = 0.5 ** 0.5


# ------------------------------------------------------------------------------------------------------------------------------
# operand forms
# ------------------------------------------------------------------------------------------------------------------------------
def _rne(v, dtype):
    return v.to(dtype).float()


def split_terms(x, dtype, scale=1.0):
    """fp32 x -> (hi, lo) fp32 tensors: hi = RNE_dtype(v), lo = RNE_dtype(v - hi) of v = x * scale (fp32 arithmetic, as the kernel)"""
    v = x.float() * torch.tensor(scale, dtype=torch.float32)
    hi = _rne(v, dtype)
    return hi, _rne(v - hi, dtype)


def interleave32(hi, lo):
    """logical planes [..., C] -> physical [..., 2 C]: per 32-channel chunk its 32 hi terms, then its 32 second terms"""
    C = hi.shape[-1]
    assert C % 32 == 0
    return torch.stack([hi.reshape(*hi.shape[:-1], C // 32, 32), lo.reshape(*lo.shape[:-1], C // 32, 32)], dim=-2).reshape(*hi.shape[:-1], 2 * C)


def planes(y):
    """physical [..., 2 C] -> (hi, second) logical planes as fp32"""
    v = y.float().reshape(*y.shape[:-1], y.shape[-1] // 64, 2, 32)
    return v[..., 0, :].reshape(*y.shape[:-1], -1), v[..., 1, :].reshape(*y.shape[:-1], -1)


def to_bf16_cpu(x):
    return x.float().to(torch.bfloat16)


def split_bf16_cpu(x):
    hi, lo = split_terms(x, torch.bfloat16)
    return interleave32(hi, lo).to(torch.bfloat16)


def split_f16_cpu(x, scale=1.0):
    hi, lo = split_terms(x, torch.float16, scale)
    return interleave32(hi, lo).to(torch.float16)


def pack_addend(E, N):
    """[..., 2 N] (sigmoid half | tanh half) -> the packed column order: block 2 p = channels [32 p, 32 p + 32) of the first half, block
    2 p + 1 = the same channels of the second half"""
    a, b = E[..., :N].reshape(*E.shape[:-1], N // 32, 32), E[..., N:].reshape(*E.shape[:-1], N // 32, 32)
    return torch.stack([a, b], dim=-2).reshape(*E.shape[:-1], 2 * N).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
EDGE256 = dict(B=4, T=520, lens=(520, 257, 256, 7))
EDGE128_GATE = dict(B=4, T=4104, lens=(4104, 3841, 3840, 7))
EDGE128_TAP1 = dict(B=8, T=4104, lens=(4104, 3841, 3840, 7) * 2)
EDGE128_NOLENS = dict(B=4, T=4104, lens=None)
PARTIAL = dict(B=2, T=255, lens=None)
ONE_ROW = dict(B=1, T=1, lens=(1,))

CASES = {}


Q_SCALE_GATE = 2.0               # the fixed fp4 scale of the gate's A operand (the stream x + dstep; ss_wavenet.q_scale_gate)
Q_SCALE_STORE = 2.0 ** -2        # ... of the skip GEMM's (gate outputs in (-1, 1))


def _add(name, kernel, split, epi, shape, *, taps, K=256, N=256, group_size=0, gate_mode=0, mask_rows=True, act="none", one_product=0,
         a_compact=False):
    assert name not in CASES, name
    CASES[name] = dict(name=name, kernel=kernel, split=split, epi=epi, B=shape["B"], T=shape["T"], lens=shape["lens"], taps=tuple(taps), K=K, N=N,
                       Np=2 * N if epi == "gate" else N, group_size=group_size, gate_mode=gate_mode, mask_rows=mask_rows, act=act,
                       one_product=one_product, a_compact=a_compact)
    if split == 3:   # (a key of the fp16q4 cases only: the other cases keep their data_key, that is their inputs)
        CASES[name]["q_scale"] = Q_SCALE_GATE if epi == "gate" else Q_SCALE_STORE


def _gate_kernels():
    return [("generic", s) for s in (0, 1, 2)] + [("gate256", s) for s in (0, 1, 2)] + [("gate128", 2), ("gate128q", 3)]


def _build_cases():
    for kern, s in _gate_kernels():   # every dilation of the network at every tile edge; d = 16 > HALO is legal for the generic kernel only
        for d in (1, 2, 4, 8) + ((16,) if kern == "generic" else ()):
            _add(f"gate-{kern}-s{s}-d{d}-edge256", kern, s, "gate", EDGE256, taps=(-d, 0, d))
        _add(f"gate-{kern}-s{s}-d8-partial-nolens", kern, s, "gate", PARTIAL, taps=(-8, 0, 8))
        _add(f"gate-{kern}-s{s}-d8-onerow", kern, s, "gate", ONE_ROW, taps=(-8, 0, 8))
    for s in (0, 1, 2):
        for d in (1, 8):
            _add(f"gate-generic-s{s}-d{d}-edge128", "generic", s, "gate", EDGE128_GATE, taps=(-d, 0, d))
    _add("gate-generic-s2-d8-edge128-nolens", "generic", 2, "gate", EDGE128_NOLENS, taps=(-8, 0, 8))
    # one tap: RESX on the fp32 stream, RESX on the pair-only stream, STORE
    for tag, shape in (("edge256", EDGE256), ("edge128", EDGE128_TAP1)):
        for s in (0, 1, 2):
            _add(f"resx-generic-s{s}-{tag}", "generic", s, "resx", shape, taps=(0,))
        for s in (1, 2):
            _add(f"resxpair-generic-s{s}-{tag}", "generic", s, "resx_pair", shape, taps=(0,))
        for s, act in ((0, "relu"), (1, "none"), (2, "relu")):
            _add(f"store-generic-s{s}-{act}-{tag}", "generic", s, "store", shape, taps=(0,), K=512, act=act)
        _add(f"store-generic-s2-one1-none-{tag}", "generic", 2, "store", shape, taps=(0,), K=512, act="none", one_product=1)
    for s in (1, 2):
        _add(f"resxpair-tile256-s{s}-edge256", "tile256", s, "resx_pair", EDGE256, taps=(0,))
    _add("store-tile256-s1-relu-edge256", "tile256", 1, "store", EDGE256, taps=(0,), K=512, act="relu")
    _add("store-tile256-s1-none-edge256", "tile256", 1, "store", EDGE256, taps=(0,), K=512, act="none")
    _add("store-tile256-s2-relu-edge256", "tile256", 2, "store", EDGE256, taps=(0,), K=512, act="relu")
    _add("store-tile256-s2-one1-none-edge256", "tile256", 2, "store", EDGE256, taps=(0,), K=512, act="none", one_product=1)
    _add("store-tile256-s2-compact-dense-none-edge256", "tile256", 2, "store", EDGE256, taps=(0,), K=512, act="none", one_product=2, a_compact=True)
    _add("store-tile256-s2-compact-k192-relu-edge256", "tile256", 2, "store", EDGE256, taps=(0,), K=192, act="relu", one_product=2, a_compact=True)
    _add("resxpair-tile256-s2-partial-nolens", "tile256", 2, "resx_pair", PARTIAL, taps=(0,))
    _add("store-tile256-s2-relu-partial-nolens", "tile256", 2, "store", PARTIAL, taps=(0,), K=512, act="relu")
    # the fp16q4 skip GEMM (256-row tiles, as gemm_bf16_tile256q.hip's BM)
    _add("store-tile256q-s3-relu-edge256", "tile256q", 3, "store", EDGE256, taps=(0,), K=512, act="relu")
    _add("store-tile256q-s3-k192-none-edge256", "tile256q", 3, "store", EDGE256, taps=(0,), K=192, act="none")
    _add("store-tile256q-s3-relu-partial-nolens", "tile256q", 3, "store", PARTIAL, taps=(0,), K=512, act="relu")
    for s in (0, 2):   # the ntaps = 4 loop with a partial column tile
        _add(f"store-generic-s{s}-4taps-edge256", "generic", s, "store", EDGE256, taps=(-3, 0, 1, 5), K=64, N=96, act="none")
    # weight groups: two items per group, two weight / bias / next_bias / cur_bias sets
    for kern in ("generic", "gate256", "gate128"):
        _add(f"gate-{kern}-s2-d2-groups", kern, 2, "gate", EDGE256, taps=(-2, 0, 2), group_size=2)
    _add("resx-generic-s2-groups", "generic", 2, "resx", EDGE256, taps=(0,), group_size=2)
    _add("resxpair-tile256-s2-groups", "tile256", 2, "resx_pair", EDGE256, taps=(0,), group_size=2)
    _add("store-tile256-s2-relu-groups", "tile256", 2, "store", EDGE256, taps=(0,), K=512, act="relu", group_size=2)
    for kern in ("generic", "gate256", "gate128"):
        _add(f"gate-{kern}-s2-d1-mode1", kern, 2, "gate", EDGE256, taps=(-1, 0, 1), gate_mode=1)
        _add(f"gate-{kern}-s2-d8-nomask", kern, 2, "gate", EDGE256, taps=(-8, 0, 8), mask_rows=False)
    # both fp16q4 launchers accept weight groups, ss_gemm_bf16_gate128q gate_mode = 1 and mask_rows = 0 as well: cases, not refusals
    _add("gate-gate128q-s3-d2-groups", "gate128q", 3, "gate", EDGE256, taps=(-2, 0, 2), group_size=2)
    _add("gate-gate128q-s3-d1-mode1", "gate128q", 3, "gate", EDGE256, taps=(-1, 0, 1), gate_mode=1)
    _add("gate-gate128q-s3-d8-nomask", "gate128q", 3, "gate", EDGE256, taps=(-8, 0, 8), mask_rows=False)
    _add("store-tile256q-s3-relu-groups", "tile256q", 3, "store", EDGE256, taps=(0,), K=512, act="relu", group_size=2)


_build_cases()


def case_lens(case):
    return list(case["lens"]) if case["lens"] is not None else [case["T"]] * case["B"]


def n_groups(case):
    return -(-case["B"] // case["group_size"]) if case["group_size"] else 1


def item_group(case, b):
    return b // case["group_size"] if case["group_size"] else 0


def tile_rows(case):
    """row-tile height of the kernel the case runs on: the 256-row kernels, or the generic kernel's 64 x 128 / 128 x 128 form (launch_tiles_s:
    the 128-row form when ceil(T / 128) * B * ceil(cols / 128) >= 512; cols = Np for GATE, N otherwise)"""
    if case["kernel"] != "generic":
        return 256
    cols = case["Np"] if case["epi"] == "gate" else case["N"]
    return 128 if -(-case["T"] // 128) * case["B"] * -(-cols // 128) >= 512 else 64


def n_row_tiles(case):
    return -(-case["T"] // tile_rows(case)) * case["B"]


def term_dtype(case):
    return torch.float16 if case["split"] >= 2 else torch.bfloat16


def out_scale(case):
    return 2.0 ** -WSHIFT if case["split"] >= 2 else 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# inputs (seeded, CPU): activations x 3, weights ~ 1 / sqrt(fan-in), as the kernels' other unit tests
# ------------------------------------------------------------------------------------------------------------------------------
def data_key(case):
    """everything of a case but the kernel it runs on: cases that differ in the kernel alone get the same inputs (cross-kernel identities)"""
    return repr(sorted((k, v) for k, v in case.items() if k not in ("name", "kernel")))


def make_inputs(case):
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(data_key(case).encode()))
    B, T, K, N, G = case["B"], case["T"], case["K"], case["N"], n_groups(case)
    nt, rows_out = len(case["taps"]), (2 * N if case["epi"] == "gate" else N)
    d = dict(x=torch.randn(B, T, K, generator=g) * 3.0 if not (case["split"] == 3 and case["epi"] == "store") else
             torch.rand(B, T, K, generator=g) * 2.0 - 1.0,                 # the fp16q4 skip GEMM's operand is a gate output: (-1, 1) against q_scale = 2^-2
             w=torch.randn(G, rows_out, K, nt, generator=g) / (nt * K) ** 0.5,
             bias=torch.randn(G, rows_out, generator=g) * 0.1)
    if case["epi"] == "gate":
        d["E"] = torch.randn(B, T, 2 * N, generator=g) * 0.5
    if case["epi"] in ("resx", "resx_pair"):
        d["X0"] = torch.randn(B, T, N, generator=g)
        d["next_bias"] = torch.randn(G, N, generator=g)
        d["cur_bias"] = torch.randn(G, N, generator=g)
    return d


def tail_mask(case):
    """[B, T] bool: rows >= lens[b]"""
    t = torch.arange(case["T"])[None, :]
    return t >= torch.tensor(case_lens(case))[:, None]


def with_tail(case, x, poison):
    """x with rows >= lens[b] zeroed (poison = False) or filled with +-POISON (sign alternating by row + channel)"""
    x = x.clone()
    m = tail_mask(case)
    if poison:
        sign = 1.0 - 2.0 * ((torch.arange(x.shape[1])[:, None] + torch.arange(x.shape[2])[None, :]) % 2).float()
        x[m] = (POISON * sign).expand(x.shape[0], -1, -1)[m]
    else:
        x[m] = 0.0
    return x


def stream_in(case, inp):
    """the pair-only stream before the launch: Y0 = pair(X0 + cur_bias) (fp32 sum, then split) as (hi, second) fp32 planes"""
    cb = torch.stack([inp["cur_bias"][item_group(case, b)] for b in range(case["B"])])[:, None, :]
    return split_terms(inp["X0"] + cb, term_dtype(case))


# ------------------------------------------------------------------------------------------------------------------------------
# the references
# ------------------------------------------------------------------------------------------------------------------------------
def products(case, x, w, exact=False):
    """[(a_term, w_term)] in float64 and the accumulator scale: the products the matrix cores run for this case (exact: the unsplit operands)"""
    if exact:
        return [(x.double(), w.double())], 1.0
    s = case["split"]
    if s == 0:
        return [(_rne(x, torch.bfloat16).double(), _rne(w, torch.bfloat16).double())], 1.0
    if s == 1:
        (ah, am), (wh, wm) = split_terms(x, torch.bfloat16), split_terms(w, torch.bfloat16)
        return [(ah.double(), wh.double()), (ah.double(), wm.double()), (am.double(), wh.double())], 1.0
    ah = _rne(x, torch.float16).double()
    wh, wl = split_terms(w, torch.float16, 2.0 ** WSHIFT)
    if s == 3:
        from stylesinger_amd import lib
        qs = case["q_scale"]
        _, mag = lib.fp4_rne(_rne(x, torch.float16) / qs)
        aq = (mag * torch.sign(ah.float()) * qs).double()
        return [(ah, wh.double()), (aq, lo_q4(case, w).double())], 2.0 ** -WSHIFT
    if case["one_product"]:
        return [(ah, wh.double())], 2.0 ** -WSHIFT
    return [(ah, wh.double()), (ah, wl.double())], 2.0 ** -WSHIFT


_LO_Q = {}


def unpack_addend(Ep, N):
    """inverse of pack_addend"""
    v = Ep.reshape(*Ep.shape[:-1], N // 32, 2, 32)
    return torch.cat([v[..., 0, :].reshape(*Ep.shape[:-1], N), v[..., 1, :].reshape(*Ep.shape[:-1], N)], dim=-1)


def lo_q4(case, w):
    """w [rows_out, K, ntaps] -> the values the block-scaled product sees for the weights' lo plane, in w's own index order. The packers work
    on the packed matrix [Np][ntaps * K] (gate: packed row order, tap-major columns) and quantise per 32-element block of the kernel's order."""
    from stylesinger_amd import lib
    key = (case["epi"], tuple(w.shape), float(w.double().sum()), float(w.double().abs().sum()))
    if key not in _LO_Q:
        rows, K, nt = w.shape
        if case["epi"] == "gate":
            Wp = pack_addend(w.permute(2, 1, 0), rows // 2).permute(2, 0, 1).reshape(rows, nt * K).contiguous()    # [packed row][tap * K + c]
            lo = lib.pack_gate_q4(Wp, shift=WSHIFT)[1].reshape(rows, nt, K).permute(1, 2, 0)                         # [tap][c][packed row]
            _LO_Q[key] = unpack_addend(lo, rows // 2).permute(2, 1, 0).contiguous()
        else:
            _LO_Q[key] = lib.pack_skip_q4(w[:, :, 0].contiguous(), shift=WSHIFT)[1][:, :, None]
    return _LO_Q[key]


def accumulate(case, x, w, *, exact=False, rows=None, taps=None, pad=True, leak=False, other_group=False):
    """sum over taps and channels for the rows `rows` (list per item of 1-D index tensors; None = all rows) -> list per item of float64
    [len(rows[b]), rows_out]. Rows of the item outside [0, len) read 0 whatever x holds there.
    Deliberately wrong variants (tests/test_hgemm_refs_cpu.py): taps = other offsets; pad = False: the rows [len, T) are read as they are;
    leak: rows >= T read the next item's first rows; other_group: the other weight set."""
    B, T = case["B"], case["T"]
    lens, taps = case_lens(case), (case["taps"] if taps is None else taps)
    out = []
    for b in range(B):
        r = torch.arange(T) if rows is None else rows[b]
        g = item_group(case, b)
        if other_group:
            g = (g + 1) % n_groups(case)
        prods, scale = products(case, torch.cat([x[b], x[b + 1] if b + 1 < B else torch.zeros_like(x[b])]), w[g], exact)
        acc = torch.zeros(len(r), w.shape[1], dtype=torch.float64)
        for j, o in enumerate(taps):
            src = r + o
            ok = (src >= 0) & (src < (lens[b] if pad else T))
            if leak and b + 1 < B:
                ok = ok | (src >= T)
            idx = src.clamp(0, 2 * T - 1)
            for a_t, w_t in prods:
                acc += torch.where(ok[:, None], a_t[idx], torch.zeros((), dtype=torch.float64)) @ w_t[:, :, j].t()
        out.append(acc * scale)
    return out


def _gate(z, N, gate_mode):
    if gate_mode == 0:
        return torch.sigmoid(z[..., :N]) * torch.tanh(z[..., N:])
    return torch.tanh(z[..., :N]) * torch.sigmoid(z[..., N:])


def reference(case, inp, x=None, *, rows=None, gate_mode=None, **variant):
    """float64 outputs of the case, dict name -> list per item of [len(rows[b]), N]:
      gate:      C = gate(acc + bias + E), 0 in rows >= len under mask_rows
      resx:      X = (X0 + acc + bias) * post_scale, Y = X + next_bias; both 0 in rows >= len
      resx_pair: Y = ((y0 - cur_bias) + acc + bias) * post_scale + next_bias with y0 = hi + second of the stream as it was; 0 in rows >= len
      store:     C = act(acc + bias), 0 in rows >= len
    x: the A operand's fp32 source (default inp["x"]); what it holds in rows >= len must not matter."""
    x = inp["x"] if x is None else x
    B, T, N = case["B"], case["T"], case["N"]
    lens = case_lens(case)
    acc = accumulate(case, x, inp["w"], rows=rows, **variant)
    other = variant.get("other_group", False)
    if case["epi"] == "resx_pair":
        yh, ym = stream_in(case, inp)
    out = {}
    for b in range(B):
        r = torch.arange(T) if rows is None else rows[b]
        g = item_group(case, b)
        if other:
            g = (g + 1) % n_groups(case)
        z = acc[b] + inp["bias"][g].double()
        live = (r < lens[b])[:, None] if case["mask_rows"] else torch.ones(len(r), 1, dtype=torch.bool)
        zero = torch.zeros((), dtype=torch.float64)
        if case["epi"] == "gate":
            res = dict(C=_gate(z + inp["E"][b][r].double(), N, case["gate_mode"] if gate_mode is None else gate_mode))
        elif case["epi"] == "store":
            res = dict(C=torch.relu(z) if case["act"] == "relu" else z)
        elif case["epi"] == "resx":
            xn = (inp["X0"][b][r].double() + z) * POST_SCALE
            res = dict(X=xn, Y=xn + inp["next_bias"][g].double())
        else:
            y0 = yh[b][r].double() + ym[b][r].double()
            res = dict(Y=((y0 - inp["cur_bias"][g].double()) + z) * POST_SCALE + inp["next_bias"][g].double())
        for k, v in res.items():
            out.setdefault(k, []).append(torch.where(live, v, zero))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# tolerances of the GPU test (the bars the kernels' other unit tests already use) and row bookkeeping
# ------------------------------------------------------------------------------------------------------------------------------
def gpu_bars(case):
    """output name -> max-abs bar against `reference` (GATE with split 0 additionally: mean |C - bf16(ref)| <= 2e-4, asserted by the test)"""
    s, K = case["split"], len(case["taps"]) * case["K"]
    if case["epi"] == "gate":
        return dict(C={0: 4e-3 + 1e-6, 1: 2e-5, 2: 3e-4, 3: 3e-4}[s])     # 3: the bar of tests/test_gpu_fp16q4.py
    if case["epi"] == "store":
        return dict(C=2e-5 * math.sqrt(K))
    y = 0.04 if s == 0 else 1e-4 if s == 1 else 1e-5    # split 0: Y is ONE bf16 term of |y| < 8 (half an ulp = 2^-7 = 0.008; the bar of tests/test_gpu_round2.py)
    if case["epi"] == "resx":
        return dict(X=4e-6 * math.sqrt(K), Y=y)
    return dict(Y=y)


def exact_bar(case):
    """bar of `reference` against the exact float64 operation on the unsplit operands. GATE with split 1 / 2: the project's bars (2e-4 / 4e-3).
    Elsewhere from the formats: every product a * w carries the relative rounding errors of its terms, uniform in +- u -> rms u / sqrt(3) each;
    the sum over the fan-in F of terms a ~ 3, w ~ 1 / sqrt(F) has rms error 3 * u_eff (the 1 / sqrt(F) of the weights cancels the sqrt(F) of the
    random walk); the bar is 8 rms (a million outputs stay under 5.5 rms), times post_scale < 1 or a gate slope <= 1.
      split 0: both operands to bf16: u_eff = sqrt(2) * 2^-9 / sqrt(3)
      split 1: mid * mid dropped (2^-18 relative) and the second terms rounded (2^-17 relative to the value, both operands): u_eff = 2^-16
      split 2: activations to fp16 (2^-11), weights a 22-bit pair: u_eff = 2^-11 / sqrt(3); one weight term: sqrt(2) * 2^-11 / sqrt(3)
      split 3: the second product runs on fp4 images: of the weights' lo plane (2 to 3 bits of a 2^-11 correction) and of the activations
               (which saturate at 6 q_scale), so it recovers PART of the lo plane: bounded by the one-term form. GATE: the project's 4e-3 too
               (tests/test_gpu_fp16q4.py). The STORE operand is uniform in (-1, 1): rms 1 / sqrt(3) instead of 3."""
    s = case["split"]
    if case["epi"] == "gate" and s in (1, 2, 3):
        return 2e-4 if s == 1 else 4e-3
    u = {0: math.sqrt(2.0) * 2.0 ** -9 / math.sqrt(3.0), 1: 2.0 ** -16,
         2: (math.sqrt(2.0) if case["one_product"] else 1.0) * 2.0 ** -11 / math.sqrt(3.0), 3: math.sqrt(2.0) * 2.0 ** -11 / math.sqrt(3.0)}[s]
    return 8.0 * (3.0 if s != 3 else 1.0 / math.sqrt(3.0)) * u


def edge_rows(case):
    """per item the rows within max|tap| + 1 of row 0, of every row-tile joint, of len and of T (sorted, unique, inside [0, T))"""
    T, tile, reach = case["T"], tile_rows(case), max(abs(o) for o in case["taps"]) + 1
    out = []
    for n in case_lens(case):
        marks = set(range(0, T + tile, tile)) | {n, T}
        rows = sorted({t for m in marks for t in range(m - reach, m + reach + 1) if 0 <= t < T})
        out.append(torch.tensor(rows, dtype=torch.long))
    return out


def worst_row(case, err_rows):
    """err_rows: list per item of per-row errors [T] -> (error, item, row, tile, row in tile) of the worst row"""
    tile = tile_rows(case)
    e, b, t = max((float(v.max()), b, int(v.argmax())) for b, v in enumerate(err_rows))
    return e, b, t, t // tile, t % tile
