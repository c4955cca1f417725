"""tests/fp32_stack_refs.py without a GPU: the float64 references of the fp32 denoiser launches (gate, residual projection, skip GEMM) agree
with a second statement of the same operation and are blind to what the input holds in rows >= len; the `CASES` table reaches the kernel
forms, dilations and row edges it claims (computed from the table alone); an fp32 restatement of each kernel family's arithmetic stays within
half the GPU test's bar on every case (so a GPU failure is the kernel's, not the data's); and the bars can see the faults the cases exist for."""
import pytest
import torch

import fp32_stack_refs as S
import hgemm_refs as H

CASES = S.CASES
FORMS = sorted({S.form(c) for c in CASES.values()})
GATE_W43 = [f"gate16-mt{m}" for m in (1, 2, 3, 0)] + ["gate43"] + [f"gate16x-mt{m}" for m in (2, 3)]
GATE_W = GATE_W43 + ["wino23-tile2", "wino23-tile3"]
GATE_CONV = [f"conv_gate-tile{t}" for t in (1, 2, 4)]
PROJ = [f"res-mt{m}" for m in (0, 2, 4, 6, 8)] + [f"resskip-tile{t}" for t in (1, 2, 3, 4)]
STORE = [f"store-mt{m}" for m in (0, 4, 6, 8)] + ["store16x-mt4", "splitk-k2", "splitk-k5"] + [f"conv_store-tile{t}" for t in (1, 2, 3, 4, 5)]


def _of(form):
    return [c for c in CASES.values() if S.form(c) == form]


def _contiguous(case):
    """the row tiles of the case are runs of tile_frames(case) consecutive frames (always, but for a Winograd tile that is no whole number of
    frame groups)"""
    if case["kernel"] not in S.WINO:
        return True
    per = S.group_frames(case) // case["d"]
    return (S.tile_frames(case) // per) % case["d"] == 0


def test_the_table_holds_exactly_the_kernel_forms_it_claims():
    assert FORMS == sorted(GATE_W + GATE_CONV + PROJ + STORE)
    for c in CASES.values():
        assert c["B"] <= 3 and c["K"] in (32, 64, 96, 192, 256, 640) and c["T"] <= (600 if S.tile_frames(c) == 256 else 450), c["name"]
        if c["kernel"] == "gate16" and c["mt"] == 0:
            assert S.tile_frames(c) == 64, c["name"]                       # single-layer launches: the pick model returns the 16-quad tiling


def test_packed_order_is_the_16_bit_family_s_where_both_are_defined():
    E = torch.arange(2 * 3 * 64, dtype=torch.float32).reshape(2, 3, 64)
    assert torch.equal(S.pack_addend(E, 32), H.pack_addend(E, 32))
    P = S.pack_addend(torch.arange(48, dtype=torch.float32)[None], 24, 128)[0]
    assert P[:24].tolist() == list(range(24)) and P[32:56].tolist() == list(range(24, 48)) and float(P[24:32].abs().sum() + P[56:].abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the references are the right operation, and blind to the tails
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_two_statements_agree_and_the_tails_are_ignored(name):
    case = CASES[name]
    inp = S.make_inputs(case)
    ref = S.reference(case, inp)
    other = S.reference(case, inp, how="taps" if case["family"] == "gate" else "rows")
    tail = S.tail_mask(case)
    for k in ref:
        assert tuple(ref[k].shape) == (case["B"], case["T"], ref[k].shape[-1])
        scale = float(ref[k].abs().max())
        assert scale > 0.5 and float((ref[k] - other[k]).abs().max()) <= 1e-12 * scale, (name, k)
        if case["mask_rows"]:
            assert float(ref[k][tail].abs().sum()) == 0.0
        elif tail.any():                                                   # ... and the rows past len of the unmasked form are not vacuous
            assert float(ref[k][tail].abs().amax(-1).min()) > 0.0, (name, k)
    for poison in (False, True):
        again = S.reference(case, inp, S.with_tail(case, inp["x"], poison))
        for k in ref:
            assert torch.equal(ref[k], again[k]), (name, k, poison)
    xp = S.with_tail(case, inp["x"], True)
    assert tail.any() == bool((xp.abs() == S.POISON).any()) and torch.equal(xp[~tail], inp["x"][~tail])


# ------------------------------------------------------------------------------------------------------------------------------
# the table covers what it claims
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_every_kernel_form_meets_every_row_edge(form):
    cases = _of(form)
    taps = cases[0]["family"] == "gate"
    hit = dict(len_on_joint=False, len_one_past_joint=False, len_one=False, no_lens=False, tile_beyond_len=False, t_not_a_multiple=False,
               tiles_not_multiple_of_8=False)
    if taps:
        hit.update(len_below_d=False, last_tile_within_halo=False)
    for c in cases:
        f, g = S.tile_frames(c), S.group_frames(c)
        hit["no_lens"] |= c["lens"] is None
        hit["tiles_not_multiple_of_8"] |= S.n_row_tiles(c) % 8 != 0
        hit["t_not_a_multiple"] |= c["T"] % f != 0 and c["T"] % g != 0
        if not _contiguous(c):
            continue
        for n in S.case_lens(c):
            hit["len_on_joint"] |= n % f == 0 and 0 < n < c["T"]
            hit["len_one_past_joint"] |= n % f == 1 and n > 1
            hit["len_one"] |= n == 1
            hit["tile_beyond_len"] |= any(t0 >= n for t0 in range(0, c["T"], f))
            if taps:
                hit["len_below_d"] |= n < c["d"]
                hit["last_tile_within_halo"] |= 0 < n % f <= c["d"] and n > f
    assert all(hit.values()), (form, hit)


@pytest.mark.parametrize("form", GATE_W + GATE_CONV)
def test_every_gate_form_has_the_production_and_the_masked_launch_at_every_dilation(form):
    cases = _of(form)
    for d in (1, 2, 4, 8) if form in GATE_W else (1, 8):
        mine = [c for c in cases if c["d"] == d and len(S.case_lens(c)) == 3 and not c["group_size"]]
        assert any(not c["bias"] and not c["mask_rows"] and c["a_bias"] for c in mine), (form, d, "production form")
        assert any(c["bias"] and c["mask_rows"] for c in mine), (form, d, "masked form")
        if form in GATE_W43:      # len mod 4 d in each quarter of the frame group: each of the six raw rows is the first invalid one somewhere
            quarters = {(n % (4 * d)) // d for c in mine for n in c["lens"]}
            assert quarters == {0, 1, 2, 3}, (form, d, quarters)
    assert any(c["gate_mode"] == 1 and not c["mask_rows"] for c in cases) and any(c["gate_mode"] == 1 and c["mask_rows"] for c in cases), form
    assert any(c["group_size"] and c["K"] == 192 and c["bias"] and c["a_bias"] and S.n_groups(c) == 2 for c in cases), form
    assert any(c["K"] == 64 for c in cases) and any(c["K"] == 192 for c in cases)        # two K chunks (no steady-state loop) and six
    if form in GATE_W:
        assert any(c["N"] < c["K"] and c["Np"] >= 64 * (1 + -(-2 * c["N"] // 64)) for c in cases), (form, "N < Cin with a column tile beyond N")


def test_the_16x16x4_gate_meets_frame_groups_that_are_no_divisor_of_its_tile():
    g16 = [c for c in CASES.values() if c["kernel"] == "gate16"]
    assert any(c["mt"] == 1 and c["d"] == 16 for c in g16) and any(c["mt"] == 1 and c["d"] == 32 and not _contiguous(c) for c in g16)
    assert any(c["mt"] == 3 and c["d"] == 16 for c in g16) and any(c["mt"] == 3 and not _contiguous(c) for c in g16)
    assert any(c["K"] == 256 for c in g16) and any(c["K"] == 256 for c in CASES.values() if c["kernel"] == "gate43")
    for mt in (1, 2, 3):                                                   # the production form is there to be run in every operand layout
        assert any(c["mt"] == mt and not c["bias"] and not c["mask_rows"] for c in g16)


@pytest.mark.parametrize("form", PROJ)
def test_every_projection_form_has_both_k_both_masks_and_groups(form):
    cases = _of(form)
    assert {c["K"] for c in cases} == {192, 256} and {c["mask_rows"] for c in cases} == {False, True}
    assert any(c["group_size"] for c in cases) and any(not c["group_size"] for c in cases)
    if form.startswith("resskip"):
        assert {c["accumulate"] for c in cases} == {False, True} and all(c["N"] == 2 * c["K"] for c in cases)
    else:
        assert {(c["K"], c["mask_rows"]) for c in cases} == {(192, False), (192, True), (256, False), (256, True)}


@pytest.mark.parametrize("form", STORE)
def test_every_store_form_has_the_chunk_counts_the_column_edges_and_both_epilogues(form):
    cases = _of(form)
    ks = {c["K"] for c in cases}
    assert ks == ({640} if form == "splitk-k5" else {96, 640} if form == "splitk-k2" else {32, 96, 640}), (form, ks)
    assert {c["N"] for c in cases} >= ({64, 80, 192} if form != "splitk-k5" else {64, 80, 192})
    assert {c["act"] for c in cases} == {"none", "relu"} and {c["mask_rows"] for c in cases} == {False, True}
    assert any(c["N"] % 64 for c in cases)
    if form.startswith("splitk"):
        assert all(c["K"] // 32 >= c["ksplit"] and c["N"] % 4 == 0 for c in cases)


# ------------------------------------------------------------------------------------------------------------------------------
# the bars: met by the arithmetic itself with a factor two to spare, and able to see the faults
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_fp32_restatement_of_the_arithmetic_stays_within_half_the_bar(name):
    case = CASES[name]
    inp = S.make_inputs(case)
    ref, got = S.reference(case, inp), S.fp32_restatement(case, inp)
    for k in ref:
        e, b, t, tile, grp, pos = S.worst_row(case, list((got[k].double() - ref[k]).abs().amax(-1)))
        assert e <= 0.5 * S.bars(case), (name, k, e, S.bars(case), (b, t, tile, grp, pos))


def _reach(case, b):
    """[T] bool: some tap of the row lands in [len, T) of item b"""
    T, n = case["T"], S.case_lens(case)[b]
    t = torch.arange(T)
    offs = (-case["d"], 0, case["d"]) if case["family"] == "gate" else (0,)
    return torch.stack([(t + o >= n) & (t + o < T) for o in offs]).any(0)


def _fault_rows(case, kind):
    """list per item of [T] bool: the rows on which the wrong reference `kind` must show"""
    T, lens = case["T"], S.case_lens(case)
    t = torch.arange(T)
    out = []
    for b, n in enumerate(lens):
        kept = (t < n) if case["mask_rows"] else torch.ones(T, dtype=torch.bool)
        if kind == "leak":
            m = kept & _reach(case, b)
        elif kind == "drop_tap":
            m = kept & S.joint_frames(case) & (t - case["d"] < n) if case["family"] == "gate" else torch.zeros(T, dtype=torch.bool)
        elif case["family"] == "gate":                                     # tail_bias: the padding rows hold a_bias
            m = kept & _reach(case, b) if case["a_bias"] else torch.zeros(T, dtype=torch.bool)
        else:                                                              # tail_bias: the rows >= len miss the bias
            m = kept & (t >= n)
        out.append(m)
    return out


FAULTS = ("leak", "drop_tap", "tail_bias")


@pytest.mark.parametrize("name", list(CASES))
def test_wrong_references_stand_ten_bars_off_on_the_rows_the_case_exists_for(name):
    """Three deliberately wrong references per case - a tail row leaking in at weight 1, tap -d dropped at the first frame past a tile joint,
    the (input) bias applied with the wrong meaning of rows >= len - on every row the fault reaches: max over the row's channels >= 10 bars;
    the rows it does not reach are untouched."""
    case = CASES[name]
    inp = S.make_inputs(case)
    xp = S.with_tail(case, inp["x"], True)
    how = "taps" if case["family"] == "gate" else "matmul"                  # (drop_tap is a variant of the tap loop)
    true = S.reference(case, inp, xp, how=how)
    for kind in FAULTS:
        masks = _fault_rows(case, kind)
        if not any(bool(m.any()) for m in masks):
            continue
        wrong = S.reference(case, inp, xp, how=how, **{kind: True})
        k = "C2" if "C2" in true and kind == "tail_bias" else "C"
        per_row = (wrong[k] - true[k]).abs().amax(-1)
        for b, m in enumerate(masks):
            if m.any():
                assert float(per_row[b][m].min()) >= 10.0 * S.bars(case), (name, kind, b, int(torch.arange(case["T"])[m][per_row[b][m].argmin()]))
            assert float(per_row[b][~m].max() if (~m).any() else 0.0) == 0.0, (name, kind, b)


@pytest.mark.parametrize("form", FORMS)
def test_every_fault_kind_is_reached_on_every_kernel_form(form):
    cases = _of(form)
    for kind in FAULTS:
        if kind == "drop_tap" and cases[0]["family"] != "gate":
            continue
        assert any(bool(m.any()) for c in cases for m in _fault_rows(c, kind)), (form, kind)
