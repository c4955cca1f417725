"""The fp32 denoiser stack's three launches per residual layer in the form the sampler loop uses, at every dilation and row edge: the F(4,3)
gate (ss_wino43_gate16 / 16w with mt 1, 2, 3 and 0, ss_wino43_gate, ss_wino43_gate16x), the F(2,3) gate (ss_wino_gate), the direct conv
(ss_conv_gemm GATE), the residual projection (ss_gemm16_res / resw, ss_conv_gemm RESSKIP) and the skip GEMM (ss_gemm16_store, its split-K and
bf16x3 forms, ss_conv_gemm STORE) against the float64 references of tests/fp32_stack_refs.py, over its `CASES` table
(tests/test_fp32_stack_refs_cpu.py checks the table and the references without a GPU).

The production form of the gate - bias=None (folded into E), mask_rows false, a_bias given, the weights in fetch order, the addend e_tiled, the
output in a column slot of a wider buffer - selects the kernel's FAST epilogue, which no other unit test holds against a reference.

Every case is launched twice: with rows >= lens[b] of the A operand zeroed, and with them holding +-1000. The kernels read zeros outside
[0, len) by contract (the buffer range check is the only thing between the tail and the valid frames when mask_rows = 0), so every output
buffer - sentinel regions included - must be the same bits in both runs. Then the clean run is held against the reference at the bar the
project already uses for the kernel, per row, so that a failure names (item, frame, tile, frame group, position in group)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp32_stack_refs as S  # noqa: E402
from conftest import record_measurement  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

CASES = S.CASES
DEV = "cuda:0"


def _bits(t):
    return t.view(torch.int32)


def _dev_lens(case):
    return None if case["lens"] is None else torch.tensor(S.case_lens(case), dtype=torch.int32, device=DEV)


def _pad_rows(W, Np):
    return W if W.shape[0] == Np else torch.cat([W, torch.zeros(Np - W.shape[0], W.shape[1], device=W.device)])


def _group_kw(case, **strides):
    return dict(group_size=case["group_size"], **strides) if case["group_size"] else {}


def _gate16_layouts(case, mt):
    """(W16, e_tiled, gate16_ks) combinations of one ss_wino43_gate16 launch; the first is what the case's other comparisons use. The production
    form runs in all of them; mt = 0 cannot take a tiled addend (it is laid out for one tiling) and mt = 1 exists only K-staged."""
    ks_now = L.load().ss_get_tuning(b"gate16_ks")
    if case["bias"] or case["mask_rows"]:
        return [(False, False, 1 if mt == 1 else ks_now)]
    out = []
    for ks in (1,) if mt == 1 else (1, 0):
        for w16 in (True, False):
            for e_tiled in (True, False) if mt != 0 else (False,):
                out.append((w16, e_tiled, ks))
    return out


def _launch_gate(case, inp, poison, kernel, mt, layout):
    B, T, K, N, Np, d, G = case["B"], case["T"], case["K"], case["N"], case["Np"], case["d"], S.n_groups(case)
    x = S.with_tail(case, inp["x"], poison).to(DEV)
    ws = [inp["w"][g].to(DEV) for g in range(G)]
    if kernel in S.WINO43:
        Wt = torch.stack([_pad_rows(L.pack_conv_weight(L.wino43_weight(w), interleave_half=N), Np) for w in ws]).contiguous()
    elif kernel == "wino23":
        Wt = torch.stack([_pad_rows(L.pack_conv_weight(L.wino_weight(w), interleave_half=N), Np) for w in ws]).contiguous()
    else:
        Wt = torch.stack([_pad_rows(L.pack_conv_weight(w, interleave_half=N), Np) for w in ws]).contiguous()
    slot = S.cdiv(N, 32) * 32
    out = torch.full((B, T, 3 * slot), S.SENTINEL, device=DEV)                    # [B][T][3 layer slots]: this launch writes the middle one
    slab = torch.full((B, T, 3 * Np), 5.0)                                        # the conditioner slab of three layers
    slab[..., Np:2 * Np] = S.pack_addend(inp["E"], N, Np)
    slab = slab.to(DEV)
    E = slab[:, :, Np:]
    kw = dict(B=B, T=T, Cin=K, N=N, Np=Np, Kp=K, lens=_dev_lens(case), a_bias=None if inp["a_bias"] is None else inp["a_bias"].contiguous().to(DEV),
              bias=None if inp["bias"] is None else S.pack_addend(inp["bias"], N, Np).contiguous().to(DEV), E=E, lde=3 * Np, e_bs=T * 3 * Np,
              ldc=3 * slot, mask_rows=case["mask_rows"], gate_mode=case["gate_mode"])
    kw.update(_group_kw(case, w_gs=Wt[0].numel(), bias_gs=Np, a_bias_gs=K))
    C = out[:, :, slot:]
    W = Wt if G > 1 else Wt[0]
    if kernel == "gate16":
        w16, e_tiled, ks = layout
        lib = L.load()
        before = lib.ss_get_tuning(b"gate16_ks")
        try:
            L.check(lib.ss_set_tuning(b"gate16_ks", ks), "ss_set_tuning")
            W16 = torch.stack([L.pack_gate16_weights(Wt[g], K) for g in range(G)]).contiguous() if w16 else None
            if e_tiled:
                kw.update(E=L.gate16_tile_addend(E, B=B, T=T, Np=Np, lde=3 * Np, e_bs=T * 3 * Np, dilation=d, mt=mt), e_tiled=True)
            L.wino43_gate16(x, W, C, dilation=d, mt=mt, W16=None if W16 is None else (W16 if G > 1 else W16[0]), **kw)
        finally:
            L.check(lib.ss_set_tuning(b"gate16_ks", before), "ss_set_tuning")
    elif kernel == "gate43":
        L.wino43_gate(x, W, C, dilation=d, **kw)
    elif kernel == "wino23":
        L.wino_gate(x, W, C, dilation=d, tile=case["tile"], **kw)
    elif kernel == "gate16x":
        Wx = torch.stack([L.split3_weights(Wt[g], K) for g in range(G)]).contiguous()
        if G > 1:
            kw["w_gs"] = Wx[0].numel()
        L.wino43_gate16x(x, Wx if G > 1 else Wx[0], C, dilation=d, mt=mt, **kw)
    else:
        L.conv_gemm(x, W, C, epi=L.EPI_GATE, taps=(-d, 0, d), tile=case["tile"], **kw)
    return dict(C=out)


def _launch_proj(case, inp, poison, kernel, mt, w16):
    B, T, K, N, G = case["B"], case["T"], case["K"], case["N"], S.n_groups(case)
    wide = torch.randn(B, T, 3 * K, generator=torch.Generator().manual_seed(3))   # the gate outputs of three layers: A is the middle column slice
    wide[..., K:2 * K] = inp["x"]
    wide = S.with_tail(case, wide, poison).to(DEV)
    A = wide[:, :, K:]
    ld = K + 8
    X = torch.full((B, T, ld), S.SENTINEL, device=DEV)                            # the residual stream, updated in place (C aliases R)
    X[..., :K] = inp["R"].to(DEV)
    Wp = torch.stack([L.pack_conv_weight(inp["w"][g].to(DEV)) for g in range(G)]).contiguous()
    bp = torch.stack([L.pack_bias(inp["bias"][g].to(DEV)) for g in range(G)]).contiguous()
    kw = dict(B=B, T=T, Cin=K, N=N, Np=Wp.shape[1], Kp=Wp.shape[2], lda=3 * K, a_bs=T * 3 * K, lens=_dev_lens(case), bias=bp, R=X, ldr=ld, r_bs=T * ld,
              ldc=ld, c_bs=T * ld, post_scale=S.POST_SCALE, mask_rows=case["mask_rows"])
    kw.update(_group_kw(case, w_gs=Wp[0].numel(), bias_gs=bp[0].numel()))
    if kernel == "res":
        W16 = None
        if w16:
            W16 = torch.stack([L.pack_gemm16_weights(Wp[g][:N].contiguous(), K) for g in range(G)]).contiguous()
            if G > 1:
                kw["w_gs"] = W16[0].numel()
        L.gemm16_res(A, Wp, X, mt=mt, W16=W16, **kw)
        return dict(C=X)
    S2 = torch.full((B, T, ld), S.SENTINEL, device=DEV)                           # the skip sum of the layers so far
    S2[..., :K] = inp["C2"].to(DEV) if case["accumulate"] else -3.0
    L.conv_gemm(A, Wp, X, epi=L.EPI_RESSKIP, Nh=K, C2=S2, ldc2=ld, c2_bs=T * ld, tile=case["tile"], accumulate=case["accumulate"], **kw)
    return dict(C=X, C2=S2)


def _launch_store(case, inp, poison, kernel, mt, ksplit):
    B, T, K, N, G = case["B"], case["T"], case["K"], case["N"], S.n_groups(case)
    A = S.with_tail(case, inp["x"], poison).to(DEV)
    out = torch.full((B, T, N + 8), S.SENTINEL, device=DEV)
    Wp = torch.stack([L.pack_conv_weight(inp["w"][g].to(DEV)) for g in range(G)]).contiguous()
    bp = torch.stack([L.pack_bias(inp["bias"][g].to(DEV)) for g in range(G)]).contiguous()
    kw = dict(B=B, T=T, Cin=K, N=N, Np=Wp.shape[1], Kp=Wp.shape[2], lens=_dev_lens(case), bias=bp, act=L.ACT_RELU if case["act"] == "relu" else L.ACT_NONE,
              mask_rows=case["mask_rows"], ldc=N + 8)
    kw.update(_group_kw(case, w_gs=Wp[0].numel(), bias_gs=bp[0].numel()))
    if kernel == "store":
        L.gemm16_store(A, Wp, out, mt=mt, **kw)
    elif kernel == "splitk":
        L.gemm16_store_splitk(A, Wp, out, ksplit=ksplit, mt=mt, **kw)
    elif kernel == "store16x":
        Wx = torch.stack([L.split3_gemm16_weights(Wp[g], K) for g in range(G)]).contiguous()
        if G > 1:
            kw["w_gs"] = Wx[0].numel()
        L.gemm16x_store(A, Wp, Wx, out, mt=mt, **kw)
    else:
        L.conv_gemm(A, Wp, out, tile=case["tile"], **kw)
    return dict(C=out)


def _launch(case, inp, poison, *, kernel=None, mt=None, ksplit=None, layout=None):
    """one launch of the case -> dict of the raw output buffers (device), whole buffers with their sentinel regions. poison: what rows >= len
    of A hold. kernel / mt / ksplit: run the case's inputs on another kernel form. layout: (W16, e_tiled, gate16_ks) of ss_wino43_gate16, or
    True for ss_gemm16_resw."""
    kernel = case["kernel"] if kernel is None else kernel
    mt = case["mt"] if mt is None else mt
    if case["family"] == "gate":
        if kernel == "gate16" and layout is None:
            layout = _gate16_layouts(case, mt)[0]
        raw = _launch_gate(case, inp, poison, kernel, mt, layout)
    elif case["family"] == "proj":
        raw = _launch_proj(case, inp, poison, kernel, mt, bool(layout))
    else:
        raw = _launch_store(case, inp, poison, kernel, mt, case["ksplit"] if ksplit is None else ksplit)
    torch.cuda.synchronize()
    return raw


def _values(case, raw):
    """raw device buffers -> dict name -> float64 CPU [B, T, N], after the sentinel checks: neighbouring layer slots, columns >= N and the ldc
    padding are untouched; with mask_rows the rows >= len are exactly 0"""
    N, K = case["N"], case["K"]
    out = {}
    for k, t in raw.items():
        if case["family"] == "gate":
            slot = t.shape[-1] // 3
            assert torch.all(t[..., :slot] == S.SENTINEL) and torch.all(t[..., 2 * slot:] == S.SENTINEL), f"{case['name']}: a neighbouring layer slot was written"
            assert torch.all(t[..., slot + N:2 * slot] == S.SENTINEL), f"{case['name']}: columns >= N were written"
            v = t[..., slot:slot + N]
        else:
            n = K if case["family"] == "proj" else N
            assert torch.all(t[..., n:] == S.SENTINEL), f"{case['name']} {k}: the padding columns of a row (ldc > N) were written"
            v = t[..., :n]
        out[k] = v.double().cpu()
        if case["mask_rows"]:
            assert float(out[k][S.tail_mask(case)].abs().sum()) == 0.0, f"{case['name']} {k}: rows >= len are not 0"
    return out


_CLEAN = {}


def _clean(name):
    """(raw buffers, values) of the clean run of a case in its first layout, kept for the cross-form comparisons"""
    if name not in _CLEAN:
        case = CASES[name]
        raw = _launch(case, S.make_inputs(case), False)
        _CLEAN[name] = raw, _values(case, raw)
    return _CLEAN[name]


def _same_bits(case, a, b, what):
    """every buffer of two runs holds the same bits; a failure names the first differing (item, frame, tile, frame group, position in group)"""
    for k in a:
        if torch.equal(_bits(a[k]), _bits(b[k])):
            continue
        diff = (_bits(a[k]) != _bits(b[k])).any(-1).cpu()
        bb, t = (int(v) for v in diff.nonzero()[0])
        tile, grp, pos = S.place(case, t)
        pytest.fail(f"{case['name']} {k}: {what}; first at item {bb} frame {t} (tile {tile}, frame group {grp}, position {pos}; len {S.case_lens(case)[bb]}, "
                    f"d {case['d']}), {int(diff.sum())} rows differ")


def _check_against(case, got, want, bar, what):
    """per-row max error of every output against `want` under `bar`; returns the worst error"""
    worst = 0.0
    for k in got:
        e, b, t, tile, grp, pos = S.worst_row(case, list((got[k] - want[k]).abs().amax(-1)))
        worst = max(worst, e)
        print(f"{case['name']} {what} {k}: max err {e:.3e} (bar {bar:.1e}) at item {b} frame {t} = tile {tile}, group {grp}, position {pos}")
        assert e <= bar, (f"{case['name']} {what} {k}: {e:.3e} > {bar:.1e} at item {b}, frame {t} (tile {tile} of {S.tile_frames(case)} frames, frame group {grp}, "
                          f"position {pos}; len {S.case_lens(case)[b]}, d {case['d']})")
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_stack_case(name):
    """poisoned run == clean run, bit for bit, in every operand layout of the launch, and the layouts among each other; the sentinels stand; clean
    run against the float64 reference, per row."""
    case = CASES[name]
    inp = S.make_inputs(case)
    raw, got = _clean(name)
    if case["kernel"] == "gate16":
        layouts = _gate16_layouts(case, case["mt"])
    else:
        layouts = [None, True] if case["kernel"] == "res" else [None]       # ss_gemm16_res and ss_gemm16_resw
    for i, layout in enumerate(layouts):
        if i > 0:
            other = _launch(case, inp, False, layout=layout)
            _same_bits(case, raw, other, f"the operand layout {layout} is not bit-identical to {layouts[0]}")
        _same_bits(case, raw, _launch(case, inp, True, layout=layout), f"what rows >= len of A hold reaches the output (layout {layout})")
    bar = S.bars(case)
    err = _check_against(case, got, S.reference(case, inp), bar, "vs float64")
    record_measurement("fp32_stack_edges", case=name, form=S.form(case), err=err, bar=bar)


def _named(kernel, *, pred=lambda c: True):
    return [n for n, c in CASES.items() if c["kernel"] == kernel and pred(c)]


def test_the_table_launches_the_forms_the_sampler_loop_uses():
    """what test_fp32_stack_case runs, said once in plain words: ss_wino43_gate16 with bias=None, mask_rows false, a_bias, W16 and e_tiled at
    mt = 1, 2, 3 and every dilation of the cycle; ss_gemm16_res with mt = 2 (and 0, 4, 6, 8), mask_rows false and true"""
    for mt in (1, 2, 3):
        for d in (1, 2, 4, 8):
            mine = [c for c in CASES.values() if c["kernel"] == "gate16" and c["mt"] == mt and c["d"] == d and not c["bias"] and not c["mask_rows"] and c["a_bias"]]
            assert mine and all((True, True, 1) in _gate16_layouts(c, mt) for c in mine), (mt, d)     # (W16, e_tiled, gate16_ks = 1)
    for mt in (0, 2, 4, 6, 8):
        assert {c["mask_rows"] for c in CASES.values() if c["kernel"] == "res" and c["mt"] == mt} == {False, True}, mt


@pytest.mark.parametrize("name", _named("gate16"))
def test_gate16_agrees_with_the_32x32x2_kernel(name):
    """same arithmetic up to the summation order over K: 1e-5 on gate outputs"""
    case = CASES[name]
    _, got = _clean(name)
    other = _values(case, _launch(case, S.make_inputs(case), False, kernel="gate43"))
    _check_against(case, got, other, 1e-5, "vs ss_wino43_gate")


@pytest.mark.parametrize("name", _named("gate16", pred=lambda c: c["mt"] == 0))
def test_gate16_with_mt_0_is_the_launch_of_the_picked_tiling(name):
    case = CASES[name]
    lib = L.load()
    pick = lib.ss_wino43_gate16_pick(case["B"], case["T"], case["Np"], case["d"])
    assert pick == S.gate16_pick(case["B"], case["T"], case["Np"], case["d"]), "the table's pick model is the library's on this device"
    if pick == 1 and not lib.ss_get_tuning(b"gate16_ks"):
        pick = 2
    raw, _ = _clean(name)
    layout = _gate16_layouts(case, 0)[0]
    other = _launch(case, S.make_inputs(case), False, kernel="gate16" if pick else "gate43", mt=pick, layout=layout)
    _same_bits(case, raw, other, f"mt = 0 is not the launch with mt = {pick}")


@pytest.mark.parametrize("name", _named("res", pred=lambda c: c["mt"] == 0))
def test_gemm16_res_with_mt_0_is_the_launch_of_the_picked_tiling(name):
    case = CASES[name]
    pick = L.load().ss_gemm16_pick(case["B"], case["T"], case["N"])
    assert pick == S.gemm16_pick(case["B"], case["T"], case["N"]) == S.effective_mt(case)
    _same_bits(case, _clean(name)[0], _launch(case, S.make_inputs(case), False, mt=pick), f"mt = 0 is not the launch with mt = {pick}")


@pytest.mark.parametrize("name", _named("splitk"))
def test_split_k_agrees_with_the_unsplit_kernel_and_other_slice_counts(name):
    case = CASES[name]
    inp = S.make_inputs(case)
    _, got = _clean(name)
    _check_against(case, got, _values(case, _launch(case, inp, False, kernel="store")), 3e-5, "vs ss_gemm16_store")
    for ks in (1, 3):
        _check_against(case, got, _values(case, _launch(case, inp, False, ksplit=ks)), 3e-5, f"vs ksplit {ks}")


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: no launch happens
# ------------------------------------------------------------------------------------------------------------------------------
def test_launches_the_kernels_cannot_run_are_refused_and_write_nothing():
    lib = L.load()
    g = torch.Generator().manual_seed(5)
    B, T, K = 1, 40, 64
    x = torch.randn(B, T, K, generator=g).to(DEV)
    w = (torch.randn(2 * K, K, 3, generator=g) / (3 * K) ** 0.5).to(DEV)
    Wt = L.pack_conv_weight(L.wino43_weight(w), interleave_half=K)
    W23 = L.pack_conv_weight(L.wino_weight(w), interleave_half=K)
    Np = Wt.shape[0]
    E = torch.randn(B, T, Np, generator=g).to(DEV)
    out = torch.full((B, T, K), S.SENTINEL, device=DEV)
    kw = dict(B=B, T=T, Cin=K, N=K, Np=Np, Kp=K, E=E, lde=Np, e_bs=T * Np, ldc=K, mask_rows=False)
    E16 = L.gate16_tile_addend(E, B=B, T=T, Np=Np, lde=Np, e_bs=T * Np, dilation=2, mt=2)
    with pytest.raises(L.StyleSingerHipError):                                  # a tiled addend is laid out for one tiling
        L.wino43_gate16(x, Wt, out, dilation=2, mt=0, **dict(kw, E=E16, e_tiled=True))
    before = lib.ss_get_tuning(b"gate16_ks")
    try:
        L.check(lib.ss_set_tuning(b"gate16_ks", 0), "ss_set_tuning")
        with pytest.raises(L.StyleSingerHipError):                              # the 16-quad tiling exists only K-staged
            L.wino43_gate16(x, Wt, out, dilation=2, mt=1, **kw)
    finally:
        L.check(lib.ss_set_tuning(b"gate16_ks", before), "ss_set_tuning")
    w32 = (torch.randn(64, 32, 3, generator=g) / 96 ** 0.5).to(DEV)
    Wt32 = L.pack_conv_weight(L.wino43_weight(w32), interleave_half=32)
    with pytest.raises(L.StyleSingerHipError):                                  # ... which needs two K chunks
        L.wino43_gate16(x[:, :, :32].contiguous(), Wt32, out, dilation=2, mt=1, **dict(kw, Cin=32, N=32, Np=64, Kp=32))
    Wx = L.split3_weights(Wt, K)
    for launch in (lambda: L.wino43_gate16(x, Wt, out, dilation=3, mt=2, **kw), lambda: L.wino43_gate(x, Wt, out, dilation=3, **kw),
                   lambda: L.wino_gate(x, W23, out, dilation=6, **kw), lambda: L.wino43_gate16x(x, Wx, out, dilation=12, mt=2, **kw)):
        with pytest.raises(L.StyleSingerHipError):                              # a dilation that is no power of two
            launch()
    Kr, Nr = 192, 96
    A = torch.randn(B, T, Kr, generator=g).to(DEV)
    Wp = L.pack_conv_weight((torch.randn(Nr, Kr, generator=g) / Kr ** 0.5).to(DEV))
    X = torch.full((B, T, Nr), S.SENTINEL, device=DEV)
    with pytest.raises(L.StyleSingerHipError):                                  # the fetch-order weights are whole 64-column tiles
        L.gemm16_res(A, Wp, X, mt=4, W16=torch.zeros(128 * Kr, device=DEV), R=X, B=B, T=T, Cin=Kr, N=Nr, Np=Wp.shape[0], Kp=Kr, ldr=Nr, ldc=Nr,
                     post_scale=S.POST_SCALE, mask_rows=False)
    torch.cuda.synchronize()
    assert torch.all(out == S.SENTINEL) and torch.all(X == S.SENTINEL)
