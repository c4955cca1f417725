"""tests/hgemm_refs.py without a GPU: the float64 references of the 16-bit GEMM family are the right operation, the `CASES` table reaches the
tile edges it claims (computed from the table), the GPU test's tolerances can see the faults the cases exist for (a condition on the references
alone), and what an input holds in rows >= len never reaches a reference."""
import numpy as np
import pytest
import torch

import hgemm_refs as H

CASES = H.CASES
GATE_CASES = [n for n, c in CASES.items() if c["epi"] == "gate"]


def _rows(case):
    """all rows of small cases; of the long ones the edge rows and every 9th row (the references are row-wise: nothing is lost but time)"""
    if case["T"] <= 1000:
        return None
    return [torch.unique(torch.cat([r, torch.arange(0, case["T"], 9)])) for r in H.edge_rows(case)]


def _maxdiff(a, b):
    return max(float((u - v).abs().max()) for k in a for u, v in zip(a[k], b[k]) if u.numel())


# ------------------------------------------------------------------------------------------------------------------------------
# operand forms
# ------------------------------------------------------------------------------------------------------------------------------
def _bf16_bits_rne(x):
    """RNE to bf16 in integer arithmetic on the fp32 bit pattern (finite inputs)"""
    u = x.numpy().view(np.uint32).astype(np.uint64)
    return torch.from_numpy((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.int32))


def test_operand_forms_are_the_documented_terms_and_layout():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 7, 96, generator=g) * 3.0
    assert torch.equal(H.to_bf16_cpu(x).view(torch.int16).int() & 0xFFFF, _bf16_bits_rne(x))
    for dtype, split, u in ((torch.bfloat16, H.split_bf16_cpu, 2.0 ** -9), (torch.float16, H.split_f16_cpu, 2.0 ** -12)):
        y = split(x)
        assert y.dtype == dtype and tuple(y.shape) == (3, 7, 192)
        hi, lo = H.planes(y)
        assert torch.equal(hi, x.to(dtype).float()) and torch.equal(lo, (x - hi).to(dtype).float())
        assert float((hi + lo - x).abs().max()) <= 16.0 * u * u * 2                  # the pair carries twice the significand
        assert torch.equal(y[..., 64:96].float(), hi[..., 32:64]) and torch.equal(y[..., 32:64].float(), lo[..., :32])   # pairs interleaved by 32
    w = torch.randn(64, 32, generator=g) / 32 ** 0.5
    wh, wl = H.planes(H.split_f16_cpu(w, 2.0 ** H.WSHIFT))
    assert torch.equal(wh, (w * 256.0).half().float()) and float((wl != 0).float().mean()) > 0.9
    assert float(((wh.double() + wl.double()) / 256.0 - w.double()).abs().max()) <= 2.0 ** -22 * float(w.abs().max())
    E = torch.arange(2 * 64, dtype=torch.float32)[None, :]
    Ep = H.pack_addend(E, 64)
    assert Ep[0, :32].tolist() == list(range(32)) and Ep[0, 32:64].tolist() == list(range(64, 96)) and Ep[0, 64:96].tolist() == list(range(32, 64))


@pytest.mark.parametrize("name", ["gate-gate128q-s3-d4-edge256", "store-tile256q-s3-k192-none-edge256"])
def test_fp4_image_of_the_lo_plane_sits_in_the_weights_own_index_order(name):
    """lo_q4 maps the packers' [packed row][tap-major K] image back to w's [row][channel][tap]: element by element it must be the fp4 image of
    THAT element's lo term (a permuted image would still pass every bar of a 2^-11 correction)"""
    case = CASES[name]
    w = H.make_inputs(case)["w"][0]
    ws = w.float() * 2.0 ** H.WSHIFT
    lo = (ws - ws.half().float()).double()
    lo_q = H.lo_q4(case, w).double()
    assert lo_q.shape == lo.shape
    rel = float((lo_q - lo).abs().max() / lo.abs().max())
    assert rel <= 0.26, rel                                  # the bound tests/test_gpu_fp16q4.py holds the packers to
    assert float((lo_q - lo).pow(2).mean().sqrt() / lo.pow(2).mean().sqrt()) <= 0.15
    prods, scale = H.products(case, H.make_inputs(case)["x"][0], w)
    assert len(prods) == 2 and scale == 2.0 ** -H.WSHIFT
    ah, aq = prods[0][0], prods[1][0]
    inside = ah.abs() <= 4.0 * case["q_scale"]               # the grid steps by at most 1 below 4: half a step
    assert bool(inside.any()) and float((aq - ah).abs()[inside].max()) <= 0.5 * case["q_scale"]
    assert float(aq.abs().max()) <= 6.0 * case["q_scale"]    # ... and saturates at 6


# ------------------------------------------------------------------------------------------------------------------------------
# the references are the right operation, and blind to the tails
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_reference_of_the_terms_is_the_exact_operation_and_ignores_the_tails(name):
    case = CASES[name]
    inp = H.make_inputs(case)
    rows = _rows(case)
    ref = H.reference(case, inp, rows=rows)
    exact = H.reference(case, inp, rows=rows, exact=True)
    err, bar = _maxdiff(ref, exact), H.exact_bar(case)
    assert err <= bar, (name, err, bar)
    if case["epi"] == "gate" or case["epi"] == "store":     # ... and not vacuous: the operation is not zero
        assert max(float(v.abs().max()) for v in exact["C"]) > 0.5
    for poison in (False, True):                            # poison independence, bit for bit
        other = H.reference(case, inp, H.with_tail(case, inp["x"], poison), rows=rows)
        for k in ref:
            for u, v in zip(ref[k], other[k]):
                assert torch.equal(u, v), (name, k, poison)
    lens = H.case_lens(case)
    if case["mask_rows"]:
        for k in ref:
            for b, v in enumerate(ref[k]):
                r = torch.arange(case["T"]) if rows is None else rows[b]
                assert float(v[r >= lens[b]].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the table covers what it claims
# ------------------------------------------------------------------------------------------------------------------------------
def _forms():
    forms = {}
    for c in CASES.values():
        key = c["kernel"] if c["kernel"] != "generic" else f"generic{H.tile_rows(c)}"
        forms.setdefault(key, []).append(c)
    return forms


def test_the_generic_cases_land_on_both_tile_forms():
    assert set(_forms()) == {"generic64", "generic128", "gate256", "gate128", "tile256", "gate128q", "tile256q"}


@pytest.mark.parametrize("form", ["generic64", "generic128", "gate256", "gate128", "tile256", "gate128q", "tile256q"])
def test_every_kernel_form_meets_every_tile_edge(form):
    cases = _forms()[form]
    tile = H.tile_rows(cases[0])
    hit = dict(len_on_joint=False, len_one_past_joint=False, last_tile_within_halo=False, tile_beyond_len=False, len_below_halo=False,
               no_lens=False, tiles_not_multiple_of_8=False)
    for c in cases:
        assert H.tile_rows(c) == tile
        hit["no_lens"] |= c["lens"] is None
        hit["tiles_not_multiple_of_8"] |= H.n_row_tiles(c) % 8 != 0
        reach = max(abs(o) for o in c["taps"])
        for n in H.case_lens(c):
            hit["len_on_joint"] |= n % tile == 0 and 0 < n < c["T"]
            hit["len_one_past_joint"] |= n % tile == 1 and n > 1
            hit["last_tile_within_halo"] |= 0 < (n % tile) <= H.HALO and n > tile
            hit["tile_beyond_len"] |= any(t0 >= n for t0 in range(0, c["T"], tile))
            hit["len_below_halo"] |= n < H.HALO and (n < reach or len(c["taps"]) == 1)
    assert all(hit.values()), (form, hit)


def test_every_gate_kernel_sees_every_dilation_and_every_mode():
    for kern, s in H._gate_kernels():
        mine = [c for c in CASES.values() if c["epi"] == "gate" and c["kernel"] == kern and c["split"] == s]
        on_edges = {c["taps"][2] for c in mine if c["lens"] == H.EDGE256["lens"]}
        assert {1, 2, 4, 8} <= on_edges, (kern, s, on_edges)
        assert all(c["taps"][2] <= H.HALO for c in mine) or kern == "generic"
        assert any(c["T"] == 1 for c in mine) and any(c["lens"] is None for c in mine)
    for kern in ("generic", "gate256", "gate128", "gate128q"):
        mine = [c for c in CASES.values() if c["epi"] == "gate" and c["kernel"] == kern]
        assert any(c["gate_mode"] == 1 for c in mine) and any(not c["mask_rows"] for c in mine) and any(c["group_size"] for c in mine), kern
    assert any(c["taps"][-1] > H.HALO for c in CASES.values() if c["kernel"] == "generic" and c["epi"] == "gate")
    assert any(len(c["taps"]) == 4 and c["N"] % 128 for c in CASES.values())
    for c in CASES.values():
        if c["group_size"]:
            assert H.n_groups(c) == 2 and c["B"] == 4


# ------------------------------------------------------------------------------------------------------------------------------
# the tolerances can see the faults
# ------------------------------------------------------------------------------------------------------------------------------
def _fault_rows(case, kind):
    """per item a bool mask over edge_rows(case): the rows on which the wrong reference `kind` must show"""
    T, B, taps, lens = case["T"], case["B"], case["taps"], H.case_lens(case)
    out = []
    for b, r in enumerate(H.edge_rows(case)):
        live = (r < lens[b]) if case["mask_rows"] else torch.ones_like(r, dtype=torch.bool)
        src = [r + o for o in taps]
        if kind == "tap_shift":         # the last tap one row further: shows wherever the true tap reads a row of the item
            m = live & (src[-1] < lens[b])
        elif kind == "no_pad":          # some tap lands in [len, T): the poison there
            m = live & torch.stack([(s >= lens[b]) & (s < T) for s in src]).any(0)
        elif kind == "leak":            # some tap lands past T and there is a next item
            m = live & torch.stack([s >= T for s in src]).any(0) & (b + 1 < B)
        elif kind == "other_group":
            m = live & bool(case["group_size"])
        else:
            m = live
        out.append(m)
    return out


FAULTS = ("tap_shift", "no_pad", "leak", "other_group", "gate_mode")


@pytest.mark.parametrize("name", GATE_CASES)
def test_wrong_gate_references_stand_ten_tolerances_off(name):
    """Five deliberately wrong references per GATE case, on every row the fault reaches: max over the row's channels >= 10 x the GPU bar."""
    case = CASES[name]
    inp = H.make_inputs(case)
    rows = H.edge_rows(case)
    xp = H.with_tail(case, inp["x"], True)
    true = H.reference(case, inp, xp, rows=rows)["C"]
    d = case["taps"][2]
    wrong = dict(tap_shift=lambda: H.reference(case, inp, xp, rows=rows, taps=(-d, 0, d + 1)),
                 no_pad=lambda: H.reference(case, inp, xp, rows=rows, pad=False),
                 leak=lambda: H.reference(case, inp, xp, rows=rows, leak=True),
                 other_group=lambda: H.reference(case, inp, xp, rows=rows, other_group=True),
                 gate_mode=lambda: H.reference(case, inp, xp, rows=rows, gate_mode=1 - case["gate_mode"]))
    need = 10.0 * H.gpu_bars(case)["C"]
    for kind in FAULTS:
        masks = _fault_rows(case, kind)
        if not any(bool(m.any()) for m in masks):
            continue
        got = wrong[kind]()["C"]
        for b, m in enumerate(masks):
            if m.any():
                per_row = (got[b] - true[b]).abs().amax(-1)[m]
                assert float(per_row.min()) >= need, (name, kind, b, int(rows[b][m][per_row.argmin()]), float(per_row.min()), need)
    # rows the fault does not reach are untouched by it (the variants are faults at the edges, not other operations)
    got = wrong["no_pad"]()["C"]
    for b, m in enumerate(_fault_rows(case, "no_pad")):
        assert torch.equal(got[b][~m], true[b][~m])


def test_every_fault_kind_is_reached_on_every_gate_kernel():
    for kern in ("generic", "gate256", "gate128", "gate128q"):
        for kind in FAULTS:
            assert any(bool(m.any()) for n in GATE_CASES if CASES[n]["kernel"] == kern for m in _fault_rows(CASES[n], kind)), (kern, kind)
