"""ss_layer512, ss_layer512_entry and the two addend tilers at every edge of tests/layer512_refs.py's `CASES` table (tests/test_layer512_refs_cpu.py
checks the table and the references without a GPU).

Unlike the rest of the 16-bit GEMM family this kernel does not own its zero padding: its DMA fetches rows >= lens[b] of Hin like any other, so
the invariant "every producer of H writes zero bits past len, padded rows included" is what keeps a chain of launches right. Per case, per launch:
  * entry and tilers equal the host statements bit for bit over the padded buffers, on zeroed and on poisoned (+-1000) rows >= len of X / E. The
    tilers take no lens, so for E the tail-blindness is the LAUNCH's: G, Hout and P are the same bits whichever slab it reads;
  * parity, per row, at the bars of tests/test_gpu_layer512.py against float64 of the stream the launch actually received;
  * written zeros: Hout starts as a sentinel, rows >= len of P as +-1000, G's buffer as 7.0 - afterwards rows >= len of Hout / P over the whole
    padded tiles are zero BITS, rows >= len of G are zero, G's second plane and the neighbouring layer slots still 7.0;
  * item independence: every item launched alone (B = 1, same T) gives the bits it has in the batched launch;
  * chains: Hout of launch l is Hin of launch l + 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import layer512_refs as R  # noqa: E402
from conftest import record_measurement  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

CASES = R.CASES
DEV = "cuda:0"
C = R.C
H_SENTINEL = 5.0


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _poison_rows(v, lens):
    """[B, Tp, n] fp16 (host) with every row >= lens[b], padded rows included, set to +-POISON"""
    v = v.clone()
    sign = (1.0 - 2.0 * ((torch.arange(v.shape[1])[:, None] + torch.arange(v.shape[2])[None, :]) % 2).float()) * R.POISON
    for b, n in enumerate(lens):
        v[b, n:] = sign[n:].to(v.dtype)
    return v


def _weights(case, inp, l):
    li = inp["layers"][l]
    Ws = L.split_f16(L.pack_conv_weight(li["w"].to(DEV), interleave_half=C), scale=2.0 ** R.WSHIFT)
    Wos = L.split_f16(L.pack_conv_weight(li["wo"].to(DEV)), scale=2.0 ** R.WSHIFT)
    return L.layer512_pack_gate(Ws, case["n_products"]), L.layer512_pack_res(Wos, case["n_products"])


def _wide(Ep):
    """the layer's 512 packed addend columns in the middle of a three-layer row (device)"""
    B, T, _ = Ep.shape
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + T)
    Eall = torch.randn(B, T, R.LAYER_SLOTS * 2 * C, generator=g)
    Eall[..., 2 * C:4 * C] = Ep
    return Eall.to(DEV)


def _device_slabs(case, E):
    """(fp32 slab, fp16 sets) of the device tilers for the addend E [B, T, 512] (sigmoid | tanh)"""
    B, T = case["B"], case["T"]
    Eall = _wide(R.pack_cols(E))
    lde = R.LAYER_SLOTS * 2 * C
    return (L.layer512_tile_addend(Eall[..., 2 * C:], B=B, T=T, lde=lde), L.layer512_tile_addend_f16(Eall[..., 2 * C:], R.N_ESETS, B=B, T=T, lde=lde))


def _launch(case, inp, l, Hin, P, slab, Wg, Wr, *, B=None, lens="case", fused=None, mask_rows=True, **over):
    """one launch of layer l on device buffers -> dict(GA, Hout, P): G's whole buffer (sentinel 7.0 around the middle slot), Hout (from a sentinel),
    P (a copy, updated in place). B / lens: a sub-batch (item independence)."""
    B = case["B"] if B is None else B
    T, lay = case["T"], case["layers"][l]
    lens = case["lens"] if lens == "case" else lens
    lens_d = None if lens is None else torch.tensor(list(lens), dtype=torch.int32, device=DEV)
    fused = lay["fused"] if fused is None else fused
    pl = 1 if case["g_compact"] else 2
    GA = torch.full((B, T, pl * R.LAYER_SLOTS * C), R.SENTINEL, device=DEV, dtype=torch.float16)
    Hout = torch.full_like(Hin, H_SENTINEL) if fused else None
    Pw = P.clone() if fused else None
    kw = dict(B=B, T=T, d=lay["d"], lens=lens_d, out_scale=R.OUT_SCALE, ldg=pl * R.LAYER_SLOTS * C, g_bs=T * pl * R.LAYER_SLOTS * C, mask_rows=mask_rows,
              n_products=case["n_products"], g_compact=case["g_compact"], e_f16=case["e_f16"])
    if fused:
        kw.update(Hout=Hout, P=Pw, Wr=Wr, cur_bias=inp["dstep"][l].to(DEV), next_bias=inp["dstep"][l + 1].to(DEV), bias_r=inp["layers"][l]["bo"].to(DEV))
    kw.update(over)
    L.layer512(Hin, Wg, slab, GA[..., pl * C:], **kw)
    torch.cuda.synchronize()
    return dict(GA=GA, Hout=Hout, P=Pw)


def _g_values(case, GA):
    """G's buffer (host) -> fp16 [B, T, 256] after the sentinel checks"""
    pl = 1 if case["g_compact"] else 2
    assert torch.all(GA[..., :pl * C] == R.SENTINEL) and torch.all(GA[..., 2 * pl * C:] == R.SENTINEL), "the neighbouring layer slots are untouched"
    mine = GA[..., pl * C:2 * pl * C]
    if case["g_compact"]:
        return mine
    v = mine.reshape(*mine.shape[:-1], C // 32, 2, 32)
    assert torch.all(v[..., 1, :] == R.SENTINEL), "the gate output's second plane is not written"
    return v[..., 0, :].reshape(*mine.shape[:-1], C)


def _check_launch(case, inp, l, Hin, P, slab, out, *, tag=""):
    """parity per row and written zeros of one launch (all host tensors: the buffers the launch received and what it left) -> (worst error / bar
    per output, parity misses). A parity miss is raised by the caller at the END of the case, so that the bit-exact checks still run."""
    B, T, lens, lay = case["B"], case["T"], R.case_lens(case), case["layers"][l]
    name = f"{case['name']}{tag} launch {l} (d = {lay['d']})"
    g16 = _g_values(case, out["GA"])
    for b in range(B):
        assert int((g16[b, lens[b]:].view(torch.int16) != 0).sum()) == 0, f"{name}: rows >= len of G, item {b}, are not zero"
    assert bool(torch.isfinite(g16.float()).all()) and float(g16.float().abs().max()) <= 1.0, f"{name}: G finite and |G| <= 1"
    ref = R.reference(case, inp, Hin, P, l, slab, g16=g16)
    ratios, misses = {}, []

    def per_row(what, err_rows, bar):
        e, b, t, tile, rt = R.worst_row(err_rows)
        print(f"{name} {what}: max err {e:.3e} (bar {bar:.1e}) at item {b} row {t} = tile {tile} row {rt}")
        if not e <= bar:
            misses.append(f"{name} {what}: {e:.3e} > {bar:.1e} at item {b}, row {t} (tile {tile}, row {rt} of 128; len {lens[b]})")
        ratios[what] = e / bar

    per_row("G", [(g16[b].double() - ref["G"][b]).abs().amax(-1) for b in range(B)], R.G_BAR)
    if not lay["fused"]:
        assert out["Hout"] is None
        return ratios, misses
    h, r = R.h_decode(out["Hout"], B, T), R.p_decode(out["P"], B, T)
    for b in range(B):
        for what, v in (("Hout", h), ("P", r)):
            bad = (v[b, lens[b]:].view(torch.int16) != 0).any(-1).nonzero()
            assert bad.numel() == 0, (f"{name}: rows >= len of {what} are not zero bits: item {b} (len {lens[b]}), first at row {lens[b] + int(bad[0])} "
                                      f"of the {h.shape[1]} padded rows, {bad.numel()} rows")
    assert bool(torch.isfinite(h.float()).all()) and bool(torch.isfinite(r.float()).all())
    nb = inp["dstep"][l + 1].double()
    x1 = (h[:, :T].double() - nb) + r[:, :T].double()
    live = torch.arange(T)[None, :, None] < torch.tensor(lens)[:, None, None]
    x1 = torch.where(live, x1, torch.zeros((), dtype=torch.float64))
    per_row("stream", [(x1[b] - ref["x"][b]).abs().amax(-1) for b in range(B)], R.STREAM_TOL)
    want = torch.where(live, ref["x"] + nb, torch.zeros((), dtype=torch.float64))
    slack = (h[:, :T].double() - want).abs() / (want.abs() * 2.0 ** -11 + 2 * R.STREAM_TOL)     # one fp16 rounding of x' + next_bias
    per_row("Hout", [slack[b].amax(-1) for b in range(B)], 1.0)
    return ratios, misses


def _same_bits(a, b, what):
    for k in ("GA", "Hout", "P"):
        if a[k] is None:
            assert b[k] is None
            continue
        if not torch.equal(_bits(a[k]), _bits(b[k])):
            n = int((_bits(a[k]) != _bits(b[k])).sum())
            pytest.fail(f"{what}: {k} differs in {n} bytes")


def _run_case(case):
    """the whole protocol of the module docstring for one case -> worst ratio per output over its launches"""
    inp = R.make_inputs(case)
    B, T, lens = case["B"], case["T"], R.case_lens(case)
    lens_d = None if case["lens"] is None else torch.tensor(lens, dtype=torch.int32, device=DEV)
    name = case["name"]
    # ---- entry: the host statement's bits, whatever rows >= len of X hold
    Hh, Ph = R.entry_cpu(inp["x"], inp["dstep"][0], case["lens"])
    for poison in (False, True):
        Hd, Pd = L.layer512_entry(R.with_tail(case, inp["x"], poison).to(DEV), inp["dstep"][0].to(DEV), B=B, T=T, lens=lens_d)
        assert Hd.numel() == Hh.numel() and Pd.numel() == 2 * Ph.numel()
        assert torch.equal(_bits(Hd).cpu(), _bits(Hh)), f"{name}: ss_layer512_entry H (poison = {poison})"
        assert torch.equal(_bits(Pd).cpu(), _bits(Ph)), f"{name}: ss_layer512_entry P (poison = {poison})"
    Hin, P = Hd, Pd
    worst, misses = {}, []
    for l, lay in enumerate(case["layers"]):
        # ---- both tilers: the host statements' bits, on the zeroed and on the poisoned addend
        slabs = {}
        for poison in (False, True):
            E = R.with_tail(case, inp["layers"][l]["E"], poison)
            s32, s16 = _device_slabs(case, E)
            assert torch.equal(_bits(s32).cpu(), _bits(R.tile_addend_cpu(R.pack_cols(E)))), f"{name}: ss_layer512_tile_addend (poison = {poison})"
            assert torch.equal(_bits(s16).cpu(), _bits(R.tile_addend_f16_cpu(R.pack_cols(E), R.N_ESETS))), f"{name}: ss_layer512_tile_addend_f16 (poison = {poison})"
            slabs[poison] = s16[R.ESET].contiguous() if case["e_f16"] else s32
        Wg, Wr = _weights(case, inp, l)
        # rows >= len of P (padded rows included) hold +-1000 before the launch
        P_in = R.p_encode(_poison_rows(R.p_decode(P.cpu().view(torch.float16), B, T), lens)) if lay["fused"] else None
        P_dev = P_in.to(DEV).view(torch.uint8) if lay["fused"] else None
        out = _launch(case, inp, l, Hin, P_dev, slabs[False], Wg, Wr)
        host = {k: (None if v is None else (v.cpu().view(torch.float16) if k == "P" else v.cpu())) for k, v in out.items()}
        ratios, missed = _check_launch(case, inp, l, Hin.cpu(), P_in, slabs[False].cpu(), host)
        misses += missed
        for k, v in ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
        # ---- the launch is blind to what rows >= len of E hold
        _same_bits(out, _launch(case, inp, l, Hin, P_dev, slabs[True], Wg, Wr), f"{name} launch {l}: zeroed against poisoned rows >= len of E")
        # ---- item independence
        for b in range(B):
            item = lambda t: None if t is None else t.view(B, -1)[b].contiguous()
            alone = _launch(case, inp, l, item(Hin), item(P_dev), item(slabs[False]), Wg, Wr, B=1, lens=None if case["lens"] is None else [lens[b]])
            part = dict(GA=out["GA"][b:b + 1], Hout=item(out["Hout"]), P=item(out["P"]))
            _same_bits(part, alone, f"{name} launch {l}: item {b} (len {lens[b]}) alone against the batched launch")
        if lay["fused"]:
            Hin, P = out["Hout"], out["P"]           # the chain: this launch's Hout is the next one's Hin
    record_measurement("layer512_edges", case=name, **{f"{k}_over_bar": v for k, v in worst.items()})
    assert not misses, "; ".join(misses)
    return worst


@pytest.mark.parametrize("name", [n for n in CASES if n != "saturate-d2"])
def test_layer512_edge_case(name):
    _run_case(CASES[name])


def test_layer512_gate_saturation():
    """saturate-d2: addend +-200 / +-60 (exp2 arguments of +-288 / +-577: ea = inf, eb capped at 2^30) and activations x 8. Every output finite,
    |G| <= 1, written zeros, independence - and parity at the SAME bars as every other case (asserted inside _run_case).

    This case found a fault of precision. The stream reaches |x'| = 51 here, and the stream epilogue used to round four times at that magnitude
    ((H - cur_bias) + R, + the projection, * post_scale, H' - next_bias): 8.567e-6 against STREAM_TOL = 8e-6 at item 0, row 190 - exactly what
    the host's fp32 statement of that order gives (layer512_refs.stream_fp32(order="stream_first")). The epilogue now sums the small terms
    first, the same five operations with one rounding at the stream's magnitude; the host statement of that order gives 5.9e-6 here
    (test_layer512_refs_cpu.py::test_what_the_stream_format_and_fp32_cost_against_the_stream_bar derives the bound)."""
    _run_case(CASES["saturate-d2"])


def test_gate_only_form_accepts_mask_rows_0():
    """gate-only, mask_rows = 0: rows < len are the mask_rows = 1 bits, the rest finite (computed from the zero rows the stream holds there). The
    fused form without lens accepts it too: every row is live."""
    case = CASES["gateonly-d8"]
    inp = R.make_inputs(case)
    B, T, lens = case["B"], case["T"], R.case_lens(case)
    Hd, _ = L.layer512_entry(inp["x"].to(DEV), inp["dstep"][0].to(DEV), B=B, T=T, lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    slab = _device_slabs(case, inp["layers"][0]["E"])[0]
    Wg, Wr = _weights(case, inp, 0)
    masked = _g_values(case, _launch(case, inp, 0, Hd, None, slab, Wg, Wr)["GA"].cpu())
    free = _g_values(case, _launch(case, inp, 0, Hd, None, slab, Wg, Wr, mask_rows=False)["GA"].cpu())
    ref = R.reference(case, inp, Hd.cpu(), None, 0, slab.cpu(), mask_rows=False)["G"]
    for b, n in enumerate(lens):
        assert torch.equal(free[b, :n].view(torch.int16), masked[b, :n].view(torch.int16)), f"item {b}: rows < len"
        assert bool(torch.isfinite(free[b, n:].float()).all())
        assert n == T or float(free[b, n:].float().abs().max()) > 0.0, "the rows past len are computed, not masked"
    assert float((free.double() - ref).abs().max()) <= R.G_BAR
    case = CASES["partial-nolens-d8"]
    inp = R.make_inputs(case)
    Hd, Pd = L.layer512_entry(inp["x"].to(DEV), inp["dstep"][0].to(DEV), B=case["B"], T=case["T"])
    slab = _device_slabs(case, inp["layers"][0]["E"])[0]
    Wg, Wr = _weights(case, inp, 0)
    _same_bits(_launch(case, inp, 0, Hd, Pd, slab, Wg, Wr), _launch(case, inp, 0, Hd, Pd, slab, Wg, Wr, mask_rows=False), "no lens: mask_rows is moot")


def test_refusals_launch_nothing():
    case = CASES["edge-d8"]
    inp = R.make_inputs(case)
    B, T, lens = case["B"], case["T"], R.case_lens(case)
    Hd, Pd = L.layer512_entry(inp["x"].to(DEV), inp["dstep"][0].to(DEV), B=B, T=T, lens=torch.tensor(lens, dtype=torch.int32, device=DEV))
    s32, s16 = _device_slabs(case, inp["layers"][0]["E"])
    Wg, Wr = _weights(case, inp, 0)
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    GA = torch.full((B, T + 1, 2 * C), R.SENTINEL, device=DEV, dtype=torch.float16)
    Hout = torch.full((Hd.numel() + 8,), H_SENTINEL, device=DEV, dtype=torch.float16)
    P = Pd.clone()
    base = dict(B=B, T=T, d=8, lens=lens_d, Hout=Hout[:-8], P=P, Wr=Wr, cur_bias=inp["dstep"][0].to(DEV), next_bias=inp["dstep"][1].to(DEV),
                bias_r=inp["layers"][0]["bo"].to(DEV), out_scale=R.OUT_SCALE, ldg=2 * C, g_bs=T * 2 * C)
    refused = dict(d0=dict(d=0), d9=dict(d=9), hout_is_hin=dict(Hout=Hd), ldg_504_pair=dict(ldg=504), ldg_248_compact=dict(ldg=248, g_compact=True),
                   e_f16_two_products=dict(e_f16=True, n_products=2, E512=s16[0]), fused_lens_mask_rows_0=dict(mask_rows=False),
                   hin_off_16=dict(Hin=Hd[4:]), hout_off_16=dict(Hout=Hout[4:-4]), g_off_16=dict(G=GA.view(-1)[4:]), e_off_16=dict(E512=s32[2:]),
                   wg_off_16=dict(Wg=Wg[4:]), p_off_16=dict(P=P[8:]))
    for what, over in refused.items():
        kw = dict(base, **over)
        a = dict(Hin=kw.pop("Hin", Hd), Wg=kw.pop("Wg", Wg), E512=kw.pop("E512", s32), G=kw.pop("G", GA))
        with pytest.raises(L.StyleSingerHipError):
            L.layer512(a["Hin"], a["Wg"], a["E512"], a["G"], **kw)
            pytest.fail(f"{what} was accepted")
    torch.cuda.synchronize()
    assert torch.all(GA == R.SENTINEL) and torch.all(Hout == H_SENTINEL) and torch.equal(P, Pd), "a refused call launches nothing"
    try:   # the message of the new refusal says why
        L.layer512(Hd, Wg, s32, GA, **dict(base, mask_rows=False))
    except L.StyleSingerHipError as e:
        assert "mask_rows" in str(e) and "zero rows past lens" in str(e)


def test_layer512_ok_table():
    lib = L.load()
    ncu = torch.cuda.get_device_properties(0).multi_processor_count

    def knob(v):
        L.check(lib.ss_set_tuning(b"layer512", v), "ss_set_tuning(layer512)")
    try:
        knob(2)                                                    # any size: what is refused here is refused for its geometry
        assert lib.ss_layer512_ok(1, 1, 256, 8, 512) == 1 and lib.ss_layer512_ok(4, 272, 256, 1, 256 * 6) == 1
        for bad in ((4, 272, 128, 8, 512), (4, 272, 512, 8, 512), (4, 272, 256, 0, 512), (4, 272, 256, 9, 512), (4, 272, 256, 8, 516),
                    (4, 272, 256, 8, 504), (0, 272, 256, 8, 512), (4, 0, 256, 8, 512)):
            assert lib.ss_layer512_ok(*bad) == 0, bad
        knob(1)                                                    # default: at least four rounds of 128-row tiles per CU
        for B, T, want in ((ncu, 512, 1), (ncu, 511, 1), (ncu, 385, 1), (ncu, 384, 0), (ncu - 1, 512, 0), (4 * ncu, 1, 1), (4 * ncu - 1, 128, 0),
                           (4, 272, 0)):
            assert lib.ss_layer512_ok(B, T, 256, 8, 512) == want, (B, T, want, ncu)
            assert want == (1 if -(-T // 128) * B >= 4 * ncu else 0)
        assert lib.ss_layer512_ok(ncu, 512, 256, 9, 512) == 0 and lib.ss_layer512_ok(ncu, 512, 192, 8, 512) == 0
    finally:
        knob(1)
