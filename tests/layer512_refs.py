"""Plain host statements of ss_layer512 (one launch per residual layer of the fp16x2 mel denoiser), of ss_layer512_entry and of the two addend
tilers, written from the contract in include/stylesinger_hip.h - not from the kernel, and independent of the helpers in stylesinger_amd/lib.py -
for tests/test_gpu_layer512_edges.py.

No GPU, no HIP library. tests/test_layer512_refs_cpu.py checks these statements against the exact float64 operation on the unsplit operands and
asserts from `CASES` alone that the table reaches the edges it claims and that the GPU test's bars can see the faults the cases exist for.

What is stated here:
  * the layouts, bit for bit, over the WHOLE padded buffers (rows [T, 128 ceil(T / 128)) included): H in slot-major tiles, P = the fp16 remainder
    in accumulator order, the tiled addend in its fp32 form and as fp16 sigma-delta sets - encoders and decoders; `entry_cpu` (ss_layer512_entry),
    `tile_addend_cpu`, `tile_addend_f16_cpu`;
  * `reference`: float64 "of the same terms" for ONE launch, taken from the decoded stream (Hin, P) and addend slab the launch actually receives:
    G, x', H' = fp16(x' + next_bias), R' = fp16(x' - (H' - next_bias)). It zero-pads outside [0, len) of every item ITSELF: what Hin holds in
    rows >= len never reaches the result. Deliberately wrong variants (leak / stale / taps) for the fault-visibility test;
  * `exact_chain`: the exact float64 operation on the unsplit operands;
  * `CASES`: name -> shape, lens, form and the launches of the case (one, or a chain of three).
"""
import math
import zlib

import torch

C = 256                          # channels: fixed by the kernel
BM = 128                         # rows per tile
HALO = 8                         # largest dilation
WSHIFT = 8                       # the weights' shift: W = split_f16(w * 2^8), out_scale = 2^-8
OUT_SCALE = 2.0 ** -WSHIFT
POST_SCALE = 0.5 ** 0.5
POISON = 1000.0
SENTINEL = 7.0
LAYER_SLOTS = 3                  # G sits in the middle slot of a three-layer row
G_BAR = 3e-4                     # the bars of tests/test_gpu_layer512.py
STREAM_TOL = 8e-6
N_ESETS, ESET = 5, 3             # the e_f16 cases read set 3 of 5
K_SIG = torch.tensor(-1.44269504088896340736, dtype=torch.float32)     # the gate's exp2 constants, as the tilers apply them (fp32)
K_TANH = K_SIG * 2.0


def n_tiles(T):
    return -(-T // BM)


def padded(T):
    return BM * n_tiles(T)


def pad_rows(v, T=None):
    """[B, T, n] -> [B, padded(T), n] with +0 rows appended"""
    B, T0, n = v.shape
    out = torch.zeros(B, padded(T0 if T is None else T), n, dtype=v.dtype)
    out[:, :T0] = v
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# layouts ([B, Tp, n] logical <-> the flat buffers)
# ------------------------------------------------------------------------------------------------------------------------------
def h_encode(v):
    """[B, Tp, 256] -> H: [tile = b * tiles + t / 128][slot 32][row 128][8 channels] (slot s = channels 8 s .. 8 s + 7)"""
    B, Tp, _ = v.shape
    return v.reshape(B, Tp // BM, BM, 32, 8).permute(0, 1, 3, 2, 4).reshape(-1).contiguous()


def h_decode(flat, B, T):
    return flat.reshape(B, n_tiles(T), 32, BM, 8).permute(0, 1, 3, 2, 4).reshape(B, padded(T), C)


def p_encode(v):
    """[B, Tp, 256] -> P: [tile][m 4][q 4][wave 8][lane 64 = (lh 2, l31 32)][4]: channels 32 wave + 8 q + 4 lh .. + 3 of row 32 m + l31"""
    B, Tp, _ = v.shape
    return v.reshape(B, Tp // BM, 4, 32, 8, 4, 2, 4).permute(0, 1, 2, 5, 4, 6, 3, 7).reshape(-1).contiguous()   # b tile m l31 w q lh e -> b tile m q w lh l31 e


def p_decode(flat, B, T):
    return flat.reshape(B, n_tiles(T), 4, 4, 8, 2, 32, 4).permute(0, 1, 2, 6, 4, 3, 5, 7).reshape(B, padded(T), C)


def e_encode(v):
    """[B, Tp, 512 packed columns] -> the fp32 slab [tile][nb 2][m 4][q 4][wave 8][lane 64][4]: packed columns 64 wave + 32 nb + 8 q + 4 lh .. + 3"""
    B, Tp, _ = v.shape
    return v.reshape(B, Tp // BM, 4, 32, 8, 2, 4, 2, 4).permute(0, 1, 5, 2, 6, 4, 7, 3, 8).reshape(-1).contiguous()   # b tile m l31 w nb q lh e -> b tile nb m q w lh l31 e


def e_decode(flat, B, T):
    return flat.reshape(B, n_tiles(T), 2, 4, 4, 8, 2, 32, 4).permute(0, 1, 3, 7, 5, 2, 4, 6, 8).reshape(B, padded(T), 2 * C)


def e16_encode(v):
    """[B, Tp, 512] -> one fp16 set [tile][m 4][q 4][wave 8][lane 64] x (4 values of nb 0 | 4 of nb 1)"""
    B, Tp, _ = v.shape
    return v.reshape(B, Tp // BM, 4, 32, 8, 2, 4, 2, 4).permute(0, 1, 2, 6, 4, 7, 3, 5, 8).reshape(-1).contiguous()   # -> b tile m q w lh l31 nb e


def e16_decode(flat, B, T):
    return flat.reshape(B, n_tiles(T), 4, 4, 8, 2, 32, 2, 4).permute(0, 1, 2, 6, 4, 7, 3, 5, 8).reshape(B, padded(T), 2 * C)


def pack_cols(E):
    """[..., 512] (sigmoid half | tanh half) -> the packed column order: 32-column blocks alternate"""
    a, b = E[..., :C].reshape(*E.shape[:-1], C // 32, 32), E[..., C:].reshape(*E.shape[:-1], C // 32, 32)
    return torch.stack([a, b], dim=-2).reshape(*E.shape[:-1], 2 * C).contiguous()


def unpack_cols(Ep):
    v = Ep.reshape(*Ep.shape[:-1], C // 32, 2, 32)
    return torch.cat([v[..., 0, :].reshape(*Ep.shape[:-1], C), v[..., 1, :].reshape(*Ep.shape[:-1], C)], dim=-1)


def k_cols():
    """[512] fp32: the exp2 constant of every packed column"""
    return torch.where((torch.arange(2 * C) // 32) % 2 == 0, K_SIG, K_TANH)


# ------------------------------------------------------------------------------------------------------------------------------
# host statements of the three producers
# ------------------------------------------------------------------------------------------------------------------------------
def _live(lens, B, T, Tp):
    n = torch.full((B,), T, dtype=torch.long) if lens is None else torch.tensor(list(lens), dtype=torch.long).clamp(0, T)
    return torch.arange(Tp)[None, :, None] < n[:, None, None]


def entry_cpu(x, bias, lens):
    """ss_layer512_entry: x fp32 [B, T, 256] -> (H, P) flat fp16: H = RNE16(x + bias), R = RNE16(x - (H - bias)) in fp32 arithmetic; every row >= len,
    padded rows included, is zero bits"""
    B, T, _ = x.shape
    xp = pad_rows(x.float())
    b = torch.zeros(C) if bias is None else bias.float()
    hh = (xp + b).to(torch.float16)
    rr = (xp - (hh.float() - b)).to(torch.float16)
    live = _live(lens, B, T, xp.shape[1])
    zero = torch.zeros((), dtype=torch.float16)
    return h_encode(torch.where(live, hh, zero)), p_encode(torch.where(live, rr, zero))


def tile_addend_cpu(Ep):
    """ss_layer512_tile_addend: Ep fp32 [B, T, 512 packed columns] -> the slab of exp2 arguments (fp32 product with the column's constant;
    rows >= T hold 0 * k)"""
    return e_encode(pad_rows(Ep.float()) * k_cols())


def tile_addend_f16_cpu(Ep, n_sets):
    """ss_layer512_tile_addend_f16: the first-order sigma-delta roundings r_0 = 0, E_k = RNE16(e + r_k), r_(k+1) = r_k + (e - E_k) of the scaled
    addend (fp32 arithmetic) -> [n_sets, elems] fp16; rows >= T hold +0"""
    v = pad_rows(Ep.float() * k_cols())
    r = torch.zeros_like(v)
    sets = []
    for _ in range(n_sets):
        h = (v + r).to(torch.float16)
        r = r + (v - h.float())
        sets.append(e16_encode(h))
    return torch.stack(sets)


# ------------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------------
CASES = {}


def edge_shape(d):
    return dict(B=4, T=272, lens=(272, 128 + d, 128 - d, d))


TAIL8 = dict(B=4, T=264, lens=(264, 129, 128, 7))
PARTIAL = dict(B=2, T=255, lens=None)


def _add(name, shape, ds, *, last_fused=True, n_products=2, e_f16=False, g_compact=False, x_scale=1.0, addend="random"):
    assert name not in CASES, name
    layers = [dict(d=d, fused=(last_fused or i + 1 < len(ds))) for i, d in enumerate(ds)]
    CASES[name] = dict(name=name, B=shape["B"], T=shape["T"], lens=shape["lens"], layers=layers, n_products=n_products, e_f16=e_f16,
                       g_compact=g_compact, x_scale=x_scale, addend=addend)


def _build_cases():
    for d in range(1, 9):
        _add(f"edge-d{d}", edge_shape(d), (d,))
    _add("tail8-d8", TAIL8, (8,))
    _add("zero-len-d4", dict(B=3, T=130, lens=(130, 0, 1)), (4,))
    _add("onerow-d8", dict(B=1, T=1, lens=(1,)), (8,))
    _add("partial-nolens-d8", PARTIAL, (8,))
    for d in (1, 8):
        _add(f"gateonly-d{d}", edge_shape(d), (d,), last_fused=False)
        _add(f"one-product-d{d}", edge_shape(d), (d,), n_products=1)
        _add(f"one-product-e16-d{d}", edge_shape(d), (d,), n_products=1, e_f16=True)
        _add(f"compact-d{d}", edge_shape(d), (d,), g_compact=True)
    _add("saturate-d2", TAIL8, (2,), x_scale=8.0, addend="saturate")
    _add("chain-a", edge_shape(8), (3, 8, 1), last_fused=False)      # the form run_stack_fused16 uses: the last layer is gate-only
    _add("chain-b", PARTIAL, (3, 8, 1), last_fused=False)


_build_cases()


def case_lens(case):
    return list(case["lens"]) if case["lens"] is not None else [case["T"]] * case["B"]


def form(case):
    if case["g_compact"]:
        return "g_compact"
    if case["e_f16"]:
        return "one_product_e16"
    if case["n_products"] == 1:
        return "one_product"
    return "fused" if case["layers"][-1]["fused"] else "gate_only"


def make_inputs(case):
    """seeded from the case's name; scaled as tests/test_gpu_layer512.py does. Per layer l: w [512 = sigmoid | tanh, 256, 3], wo [512, 256, 1]
    (residual half = rows [0, 256)), bo [256], E [B, T, 512] (sigmoid | tanh); dstep [n_layers + 1, 256]: cur_bias of layer l = dstep[l],
    next_bias = dstep[l + 1]"""
    g = torch.Generator(device="cpu").manual_seed(zlib.crc32(case["name"].encode()))
    B, T, nl = case["B"], case["T"], len(case["layers"])
    d = dict(x=torch.randn(B, T, C, generator=g) * 2.0 * case["x_scale"], dstep=torch.randn(nl + 1, C, generator=g), layers=[])
    for _ in range(nl):
        lay = dict(w=torch.randn(2 * C, C, 3, generator=g) / (3 * C) ** 0.5, wo=torch.randn(2 * C, C, 1, generator=g) / C ** 0.5,
                   bo=torch.randn(C, generator=g) * 0.1, E=torch.randn(B, T, 2 * C, generator=g) * 0.5)
        if case["addend"] == "saturate":   # +-200 and +-60, alternating over columns and rows: exp2 arguments of +-288 / +-577 (inf) and +-87 / +-173
            t, c = torch.arange(T)[:, None], torch.arange(2 * C)[None, :]
            mag = torch.where((t + c) % 2 == 0, 200.0, 60.0)
            sign = 1.0 - 2.0 * (((t // 2) + (c // 2)) % 2).float()
            lay["E"] = (mag * sign).expand(B, T, 2 * C).contiguous()
        d["layers"].append(lay)
    return d


def with_tail(case, v, poison):
    """v [B, T, n] with rows >= lens[b] zeroed or filled with +-POISON (sign alternating by row + column)"""
    v = v.clone()
    m = torch.arange(case["T"])[None, :] >= torch.tensor(case_lens(case))[:, None]
    if poison:
        sign = 1.0 - 2.0 * ((torch.arange(v.shape[1])[:, None] + torch.arange(v.shape[2])[None, :]) % 2).float()
        v[m] = (POISON * sign).expand(v.shape[0], -1, -1)[m]
    else:
        v[m] = 0.0
    return v


def split_terms(x, scale=1.0):
    """fp32 -> (hi, lo) fp32: hi = RNE16(v), lo = RNE16(v - hi) of v = x * scale (ss_split_f16)"""
    v = x.float() * torch.tensor(scale, dtype=torch.float32)
    hi = v.to(torch.float16).float()
    return hi, (v - hi).to(torch.float16).float()


def addend_slab(case, inp, layer, E=None):
    """the slab the launch of `layer` reads, from the host tilers: the fp32 form, or set ESET of N_ESETS"""
    Ep = pack_cols(inp["layers"][layer]["E"] if E is None else E)
    return tile_addend_f16_cpu(Ep, N_ESETS)[ESET] if case["e_f16"] else tile_addend_cpu(Ep)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference of one launch
# ------------------------------------------------------------------------------------------------------------------------------
def reference(case, inp, Hin, P, layer=0, slab=None, g16=None, *, mask_rows=True, taps=None, leak=False, stale=None):
    """float64 of the terms the matrix cores see, for launch `layer` of the case, from the buffers the launch receives: Hin (flat fp16), P (flat
    fp16, or None for a gate-only launch), slab (default: the host tiler's). -> dict of float64 [B, T, 256]: G always; x, H, R for a fused launch
    (x = x', H = fp16(x' + next_bias), R = fp16(x' - (H - next_bias))). Rows of Hin outside [0, len) are read as 0 whatever they hold.
    g16: the fp16 gate outputs to project (default fp16(G)): the GPU test hands over the kernel's own, so that the projection is checked on its
    own operand. mask_rows = False (gate-only form): rows [len, T) of G are computed, from zero rows.
    Deliberately wrong variants: taps = other offsets; leak: the halo rows outside the item's tiles read the neighbouring item's H tile (as the
    buffer holds it); stale [B, Tp, 256]: rows [len, len + d) of Hin hold these values instead of zeros."""
    lay, li = case["layers"][layer], inp["layers"][layer]
    B, T, d = case["B"], case["T"], lay["d"]
    Tp, lens = padded(T), case_lens(case)
    taps = (-d, 0, d) if taps is None else taps
    R = max(abs(o) for o in taps)
    h = h_decode(Hin, B, T).double()
    live = _live(lens, B, T, Tp)
    hz = torch.where(live, h, torch.zeros((), dtype=torch.float64))
    if stale is not None:
        for b in range(B):
            hz[b, lens[b]:min(lens[b] + d, Tp)] = stale[b, lens[b]:min(lens[b] + d, Tp)].double()
    wh, wl = (t.double() for t in split_terms(li["w"], 2.0 ** WSHIFT))
    prods = [wh] if case["n_products"] == 1 else [wl, wh]
    slab = addend_slab(case, inp, layer) if slab is None else slab
    es = (e16_decode(slab, B, T) if slab.dtype == torch.float16 else e_decode(slab, B, T)).double() / k_cols().double()
    e = unpack_cols(es)
    G = torch.zeros(B, T, C, dtype=torch.float64)
    for b in range(B):
        src = torch.zeros(Tp + 2 * R, C, dtype=torch.float64)
        src[R:R + Tp] = hz[b]
        if leak:
            if b > 0:
                src[:R] = h[b - 1, Tp - R:]
            if b + 1 < B:
                src[R + Tp:] = h[b + 1, :R]
        acc = torch.zeros(Tp, 2 * C, dtype=torch.float64)
        for j, o in enumerate(taps):
            a = src[R + o:R + o + Tp]
            for w in prods:
                acc += a @ w[:, :, j].t()
        z = acc * OUT_SCALE + e[b]
        g = torch.sigmoid(z[:, :C]) * torch.tanh(z[:, C:])
        n = min(lens[b], T) if mask_rows else T
        G[b, :n] = g[:n]
    out = dict(G=G)
    if not lay["fused"] or P is None:
        return out
    gh = G.to(torch.float16).double() if g16 is None else g16.double()
    woh, wol = (t.double() for t in split_terms(li["wo"][:C, :, 0], 2.0 ** WSHIFT))
    proj = (gh @ wol.t() if case["n_products"] == 2 else 0.0) + gh @ woh.t()
    cb, nb = inp["dstep"][layer].double(), inp["dstep"][layer + 1].double()
    x = (h[:, :T] - cb) + p_decode(P, B, T).double()[:, :T]
    xn = (x + (proj * OUT_SCALE + li["bo"].double())) * POST_SCALE
    Hn = (xn + nb).to(torch.float16).double()
    Rn = (xn - (Hn - nb)).to(torch.float16).double()
    zero = torch.zeros((), dtype=torch.float64)
    m = live[:, :T]
    out.update(x=torch.where(m, xn, zero), H=torch.where(m, Hn, zero), R=torch.where(m, Rn, zero))
    return out


def stream_fp32(case, inp, Hin, P, layer, g16, order="small_first"):
    """the stream update in FP32 with one rounding per operation, in either order of the same five operations; the projection's accumulator is the
    exactly summed float64 value rounded once. -> x' as its (H', R') pair gives it back, float64 [B, T, 256].
      order = "small_first" (the header's, what the kernel does): s = (R - cur_bias) + (acc * out_scale + bias_r); x' = fma(H, post_scale,
              s * post_scale); H' = RNE16(x' + next_bias); R' = RNE16((x' - H') + next_bias) - one rounding at the stream's magnitude;
      order = "stream_first" (the kernel's former order): x = (H - cur_bias) + R; x' = (x + (acc * out_scale + bias_r)) * post_scale;
              R' = RNE16(x' - (H' - next_bias)) - four.
    What the FORMAT and fp32 cost against float64, without any kernel: tests/test_layer512_refs_cpu.py holds STREAM_TOL against both."""
    li, B, T = inp["layers"][layer], case["B"], case["T"]
    gh = g16.double()
    woh, wol = (t.double() for t in split_terms(li["wo"][:C, :, 0], 2.0 ** WSHIFT))
    acc = ((gh @ wol.t() if case["n_products"] == 2 else 0.0) + gh @ woh.t()).float()
    cb, nb = inp["dstep"][layer].float(), inp["dstep"][layer + 1].float()
    h, r = h_decode(Hin, B, T)[:, :T].float(), p_decode(P, B, T)[:, :T].float()
    f = torch.addcmul(li["bo"].float().expand_as(acc), acc, torch.tensor(OUT_SCALE, dtype=torch.float32))      # out_scale is a power of two: the fma's value
    post = torch.tensor(POST_SCALE, dtype=torch.float32)
    if order == "small_first":
        sm = ((r - cb) + f) * post
        xn = (h.double() * post.double() + sm.double()).float()      # the fma: H * post_scale is exact in float64 (11 x 24 bits)
        hh = (xn + nb).to(torch.float16)
        rr = ((xn - hh.float()) + nb).to(torch.float16)
    else:
        xn = (((h - cb) + r) + f) * post
        hh = (xn + nb).to(torch.float16)
        rr = (xn - (hh.float() - nb)).to(torch.float16)
    x1 = (hh.double() - nb.double()) + rr.double()
    return torch.where(_live(case_lens(case), B, T, T), x1, torch.zeros((), dtype=torch.float64))


def next_stream(ref):
    """the (Hin, P) buffers the next launch of a chain receives from a reference's H' and R'"""
    return h_encode(pad_rows(ref["H"].to(torch.float16))), p_encode(pad_rows(ref["R"].to(torch.float16)))


def run_chain(case, inp, lens="case", **variant_of_layer):
    """every launch of the case on the host, each fed with its predecessor's H' and R' -> list per launch of (Hin, P, reference). lens = None: the
    UNMASKED streams (what the rows >= len would hold if nothing masked them)."""
    c = case if lens == "case" else dict(case, lens=lens)
    Hin, P = entry_cpu(inp["x"], inp["dstep"][0], c["lens"])
    out = []
    for l in range(len(case["layers"])):
        ref = reference(c, inp, Hin, P, l)
        out.append((Hin, P, ref))
        if c["layers"][l]["fused"]:
            Hin, P = next_stream(ref)
    return out


def exact_chain(case, inp):
    """the exact float64 operation on the unsplit operands (net.py:66-78 per layer): list per launch of dict(G, x) [B, T, 256]"""
    B, T, lens = case["B"], case["T"], case_lens(case)
    m = _live(lens, B, T, T)
    zero = torch.zeros((), dtype=torch.float64)
    x = torch.where(m, inp["x"].double(), zero)
    out = []
    for l, lay in enumerate(case["layers"]):
        li, d = inp["layers"][l], lay["d"]
        y = torch.where(m, x + inp["dstep"][l].double(), zero)
        z = torch.nn.functional.conv1d(y.transpose(1, 2), li["w"].double(), padding=d, dilation=d).transpose(1, 2) + li["E"].double()
        G = torch.where(m, torch.sigmoid(z[..., :C]) * torch.tanh(z[..., C:]), zero)
        res = dict(G=G)
        if lay["fused"]:
            x = torch.where(m, (x + G @ li["wo"][:C, :, 0].double().t() + li["bo"].double()) * POST_SCALE, zero)
            res["x"] = x
        out.append(res)
    return out


def exact_bar(case, layer=0):
    """bar of `reference` against `exact_chain`, from the fp16 term widths. The conv operand is ONE fp16 term of y = x + dstep: relative rounding
    error uniform in +- 2^-11, rms 2^-11 / sqrt(3); the sum over the fan-in F = 768 of terms y ~ rms_y, w ~ 1 / sqrt(F) has rms error
    rms_y * 2^-11 / sqrt(3) (the weights' 1 / sqrt(F) cancels the random walk's sqrt(F)); one weight term adds the same again (sqrt(2)); the
    weight PAIR (22 bits) and the stream's 22 bits add nothing visible. The fp16 addend set adds half an fp16 ulp of |e k| < 8: 2^-9 / k in z. The gate's slope
    is <= 1, the residual projection (fan-in 256, w ~ 1 / 16) has unit gain on the gate's error + the fp16 rounding of G (2^-12), post_scale < 1.
    8 rms (a million outputs stay under 5.5); every layer of a chain adds its own."""
    rms_y = math.sqrt(4.0 * case["x_scale"] ** 2 + 1.0)
    per_layer = rms_y * 2.0 ** -11 / math.sqrt(3.0) * (math.sqrt(2.0) if case["n_products"] == 1 else 1.0) + 2.0 ** -12
    return 8.0 * per_layer * (layer + 1) + (2.0 ** -9 / 1.4426950408889634 if case["e_f16"] else 0.0)


def worst_row(err_rows):
    """err_rows: list per item of per-row errors -> (error, item, row, tile, row in tile) of the worst row"""
    e, b, t = max((float(v.max()), b, int(v.argmax())) for b, v in enumerate(err_rows) if v.numel())
    return e, b, t, t // BM, t % BM
