"""tests/layer512_refs.py without a GPU: the layout statements invert each other, entry_cpu is the documented pair with zero bits past len, the
float64 reference of ss_layer512 is the right operation and blind to what rows >= len hold, the `CASES` table reaches the edges it claims
(computed from the table), and the GPU test's bars can see the faults the cases exist for (a condition on the references alone)."""
import math

import pytest
import torch

import layer512_refs as R

CASES = R.CASES
_CHAIN = {}


def _chain(name):
    if name not in _CHAIN:
        case = CASES[name]
        inp = R.make_inputs(case)
        _CHAIN[name] = inp, R.run_chain(case, inp)
    return _CHAIN[name]


# ------------------------------------------------------------------------------------------------------------------------------
# layouts and producers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T", [(1, 1), (2, 255), (3, 272)])
def test_layout_statements_invert_each_other_and_place_what_the_header_says(B, T):
    Tp = R.padded(T)
    ids = torch.arange(B * Tp * R.C, dtype=torch.int32).reshape(B, Tp, R.C)
    for enc, dec in ((R.h_encode, R.h_decode), (R.p_encode, R.p_decode)):
        flat = enc(ids)
        assert flat.numel() == ids.numel() and torch.equal(dec(flat, B, T), ids) and sorted(flat.tolist()) == list(range(ids.numel()))
    ids2 = torch.arange(B * Tp * 2 * R.C, dtype=torch.int32).reshape(B, Tp, 2 * R.C)
    for enc, dec in ((R.e_encode, R.e_decode), (R.e16_encode, R.e16_decode)):
        flat = enc(ids2)
        assert torch.equal(dec(flat, B, T), ids2) and sorted(flat.tolist()) == list(range(ids2.numel()))
    # the documented index maps, spelled out element by element on a few probes
    b, tile, row, ch = B - 1, R.n_tiles(T) - 1, 37 % min(Tp, 128), 203
    t = tile * 128 + row
    tg = b * R.n_tiles(T) + tile
    assert R.h_encode(ids)[((tg * 32 + ch // 8) * 128 + row) * 8 + ch % 8] == ids[b, t, ch]
    m, l31, w, q, lh, e = row // 32, row % 32, ch // 32, (ch % 32) // 8, (ch % 8) // 4, ch % 4
    assert R.p_encode(ids)[((((tg * 4 + m) * 4 + q) * 8 + w) * 64 + lh * 32 + l31) * 4 + e] == ids[b, t, ch]
    col = 64 * w + 32 * 1 + 8 * q + 4 * lh + e
    assert R.e_encode(ids2)[(((((tg * 2 + 1) * 4 + m) * 4 + q) * 8 + w) * 64 + lh * 32 + l31) * 4 + e] == ids2[b, t, col]
    assert R.e16_encode(ids2)[(((((tg * 4 + m) * 4 + q) * 8 + w) * 64 + lh * 32 + l31) * 2 + 1) * 4 + e] == ids2[b, t, col]
    E = torch.arange(2 * R.C, dtype=torch.float32)[None, :]
    assert torch.equal(R.unpack_cols(R.pack_cols(E)), E) and R.pack_cols(E)[0, 32:64].tolist() == list(range(256, 288))
    assert R.k_cols()[31] == R.K_SIG and R.k_cols()[32] == R.K_TANH and R.k_cols()[64] == R.K_SIG


@pytest.mark.parametrize("name", ["edge-d3", "zero-len-d4", "onerow-d8", "partial-nolens-d8", "saturate-d2"])
def test_entry_is_the_22_bit_pair_with_zero_bits_past_len(name):
    case = CASES[name]
    inp = R.make_inputs(case)
    B, T, lens, bias = case["B"], case["T"], R.case_lens(case), inp["dstep"][0]
    Hf, Pf = R.entry_cpu(inp["x"], bias, case["lens"])
    assert Hf.dtype == torch.float16 and Hf.numel() == Pf.numel() == B * R.padded(T) * R.C
    h, r = R.h_decode(Hf, B, T), R.p_decode(Pf, B, T)
    for poison in (False, True):       # what rows >= len of x hold never reaches the stream
        H2, P2 = R.entry_cpu(R.with_tail(case, inp["x"], poison), bias, case["lens"])
        assert torch.equal(H2.view(torch.int16), Hf.view(torch.int16)) and torch.equal(P2.view(torch.int16), Pf.view(torch.int16))
    for b in range(B):
        assert int((h[b, lens[b]:].view(torch.int16) != 0).sum()) == 0, "rows >= len of H, padded rows included, are zero BITS"
        assert int((r[b, lens[b]:].view(torch.int16) != 0).sum()) == 0
        if lens[b] == 0:
            continue
        x = inp["x"][b, :lens[b]].double()
        back = (h[b, :lens[b]].double() - bias.double()) + r[b, :lens[b]].double()
        assert float((back - x).abs().max()) <= float((x + bias.double()).abs().max()) * 2.0 ** -22       # (H - bias) + R = x to 22 bits
        assert torch.equal(h[b, :lens[b]], (inp["x"][b, :lens[b]] + bias).to(torch.float16))


def test_addend_tilers_are_the_scaled_values_and_their_sigma_delta_sets():
    case = CASES["partial-nolens-d8"]
    inp = R.make_inputs(case)
    B, T = case["B"], case["T"]
    Ep = R.pack_cols(inp["layers"][0]["E"])
    want = Ep * R.k_cols()
    slab = R.e_decode(R.tile_addend_cpu(Ep), B, T)
    assert torch.equal(slab[:, :T], want) and float(slab[:, T:].abs().sum()) == 0.0
    sets = R.tile_addend_f16_cpu(Ep, R.N_ESETS)
    acc = torch.zeros_like(want, dtype=torch.float64)
    for k in range(R.N_ESETS):
        v = R.e16_decode(sets[k], B, T)
        assert int((v[:, T:].view(torch.int16) != 0).sum()) == 0
        acc += v[:, :T].double()
        ulp = torch.clamp(want.abs(), min=2.0 ** -14) * 2.0 ** -10
        assert bool(((acc / (k + 1) - want.double()).abs() <= 0.5 * ulp / (k + 1) + 1e-7).all()), k
    assert torch.equal(R.e16_decode(sets[0], B, T)[:, :T], want.to(torch.float16))


# ------------------------------------------------------------------------------------------------------------------------------
# the reference is the right operation, and blind to the tails
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_reference_of_the_terms_is_the_exact_operation_and_ignores_the_tails(name):
    case = CASES[name]
    inp, chain = _chain(name)
    exact = R.exact_chain(case, inp)
    lens = R.case_lens(case)
    for l, (Hin, P, ref) in enumerate(chain):
        bar = R.exact_bar(case, l)
        for k in exact[l]:
            err = float((ref[k] - exact[l][k]).abs().max())
            assert err <= bar, (name, l, k, err, bar)
        if max(lens) > 16 and case["addend"] == "random":
            assert float(exact[l]["G"].abs().max()) > 0.5            # not vacuous
        assert float(ref["G"].abs().max()) <= 1.0
        # poison in rows >= len of Hin / P / E: the same bits
        h = R.h_decode(Hin, case["B"], case["T"]).clone()
        Tp = h.shape[1]
        sign = (1.0 - 2.0 * ((torch.arange(Tp)[:, None] + torch.arange(R.C)[None, :]) % 2).float()).to(torch.float16) * R.POISON
        for b in range(case["B"]):
            h[b, lens[b]:] = sign[lens[b]:]
        slab_p = R.addend_slab(case, inp, l, R.with_tail(case, inp["layers"][l]["E"], True))
        other = R.reference(case, inp, R.h_encode(h), P, l, slab_p)
        for k in ref:
            assert torch.equal(ref[k], other[k]), (name, l, k)
            for b in range(case["B"]):
                assert float(ref[k][b, lens[b]:].abs().sum()) == 0.0
        assert all(torch.isfinite(v).all() for v in ref.values())


def test_what_the_stream_format_and_fp32_cost_against_the_stream_bar():
    """STREAM_TOL = 8e-6 is worded for |x + dstep| <~ 16. On saturate-d2 the activations are x 8 and |x'| reaches 51, where half an fp32 ulp is
    1.9e-6 and half an ulp of the fp16 remainder 3.8e-6. Without any kernel: the order of operations that rounds ONCE at the stream's magnitude
    (the header's, "small_first") stays under the bar there, by a bound derived from the formats; the order that rounds four times there (the
    kernel's former one) does not - 8.57e-6, which is what the kernel gave before it summed the small terms first."""
    for name in ("edge-d8", "saturate-d2"):
        case = CASES[name]
        inp, chain = _chain(name)
        Hin, P, ref = chain[0]
        g16 = ref["G"].to(torch.float16)
        xmax = float(ref["x"].abs().max())
        assert xmax < 64.0
        err = {o: float((R.stream_fp32(case, inp, Hin, P, 0, g16, o) - ref["x"]).abs().max()) for o in ("small_first", "stream_first")}
        print(f"{name}: fp32 statements of the stream update vs float64 {err}, |x'| <= {xmax:.1f}")
        ulp32 = 2.0 ** (math.floor(math.log2(xmax)) - 23)                 # of x'
        ulp_h = 2.0 ** (math.floor(math.log2(xmax + 4.0)) - 10)           # of H' = fp16(x' + next_bias), |next_bias| < 4
        ulp_r = 2.0 ** (math.log2(ulp_h / 2) - 1 - 10)                    # of R', |R'| <= half an ulp of H'
        derived = 0.5 * ulp32 + 0.5 * ulp_r + xmax * 2.0 ** -25 + 4 * 2.0 ** -24     # one fma rounding, R', post_scale's own rounding, the small terms
        assert err["small_first"] <= derived <= R.STREAM_TOL, (name, err, derived)
    assert err["stream_first"] > R.STREAM_TOL        # saturate-d2, the former order


def test_gate_only_without_mask_rows_equals_the_masked_rows_below_len():
    case = CASES["gateonly-d8"]
    inp, chain = _chain("gateonly-d8")
    Hin, P, ref = chain[0]
    free = R.reference(case, inp, Hin, P, 0, mask_rows=False)["G"]
    for b, n in enumerate(R.case_lens(case)):
        assert torch.equal(free[b, :n], ref["G"][b, :n])
        assert n == case["T"] or float(free[b, n:].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the table reaches what it claims
# ------------------------------------------------------------------------------------------------------------------------------
def test_the_table_reaches_every_dilation_length_edge_and_form():
    ds = {lay["d"] for c in CASES.values() for lay in c["layers"]}
    assert ds == set(range(1, 9))
    fused_single = [c for c in CASES.values() if len(c["layers"]) == 1 and R.form(c) == "fused"]
    for d in range(1, 9):                     # every dilation meets len = 0, +-1, +-d (mod 128) on the plain fused form
        res = set()
        for c in fused_single:
            if c["layers"][0]["d"] == d:
                res |= {n % 128 for n in R.case_lens(c) if n > 0}
        for c in fused_single:                # the residues 0 and +-1 do not depend on d: any dilation's case counts when it is >= d (the halo reaches)
            if c["layers"][0]["d"] >= d:
                res |= {n % 128 for n in R.case_lens(c) if n > 0 and n % 128 in (0, 1, 127)}
        need = {0, 1, 127, d % 128, (128 - d) % 128}
        assert need <= res, (d, sorted(need - res))
    all_lens = [(c, n) for c in CASES.values() for n in R.case_lens(c)]
    assert any(0 < n < R.HALO for c, n in all_lens) and any(n == 0 for c, n in all_lens) and any(c["T"] == 1 for c in CASES.values())
    assert any(0 < n < c["layers"][0]["d"] for c, n in all_lens), "a length below the dilation itself"
    assert {8, 16, 127} <= {c["T"] % 128 for c in CASES.values()}
    assert any(c["lens"] is None for c in CASES.values())
    assert {R.form(c) for c in CASES.values()} == {"fused", "gate_only", "one_product", "one_product_e16", "g_compact"}
    for f in ("gate_only", "one_product", "one_product_e16", "g_compact"):
        assert {1, 8} <= {c["layers"][0]["d"] for c in CASES.values() if R.form(c) == f and len(c["layers"]) == 1}, f
    chains = [c for c in CASES.values() if len(c["layers"]) == 3]
    assert len(chains) == 2 and all([lay["fused"] for lay in c["layers"]] == [True, True, False] for c in chains)
    assert any(c["lens"] is None for c in chains) and any(c["lens"] is not None for c in chains)
    assert all(c["B"] * c["T"] <= 4 * 272 for c in CASES.values())
    sat = CASES["saturate-d2"]
    e = R.make_inputs(sat)["layers"][0]["E"]
    assert float(e.abs().max()) * 1.4426950408889634 > 128.0 and sat["x_scale"] == 8.0      # exp2 overflows fp32: 1 + ea = inf is reached
    assert {float(v) for v in e.abs().unique()} == {60.0, 200.0} and float(e[0, 0, :4].sum()) != 4 * float(e[0, 0, 0])


# ------------------------------------------------------------------------------------------------------------------------------
# the bars can see the faults
# ------------------------------------------------------------------------------------------------------------------------------
FAULT_CASES = [n for n in CASES if n.startswith("edge-") or n.startswith("chain-")]
FAULTS = ("leak", "stale", "tap")


def _fault_reach(case, layer, kind):
    """does the fault change any row the launch writes? computed from the shape alone"""
    T, Tp, d, lens = case["T"], R.padded(case["T"]), case["layers"][layer]["d"], R.case_lens(case)
    if kind == "leak":      # a live row within d of the item's first / last TILE row whose neighbour tile row is live
        for b, n in enumerate(lens):
            up = b > 0 and n > 0 and min(lens[b - 1], T) > Tp - d                      # row t < d reads row Tp - d + t of the item before
            down = b + 1 < case["B"] and lens[b + 1] > 0 and n > Tp - d                # row t >= Tp - d reads row t + d - Tp of the item after
            if up or down:
                return True
        return False
    if kind == "stale":     # a live row within d of len < T
        return any(0 < n < T for n in lens)
    return any(n > d for n in lens)      # the last tap one row further: some live row's true tap reads a live row


@pytest.mark.parametrize("name", FAULT_CASES)
def test_wrong_references_stand_ten_bars_off(name):
    """three deliberately wrong references per launch: the halo of an item's first / last tile reads the neighbouring item's H tile; rows
    [len, len + d) of Hin hold the unmasked stream; the last tap uses d + 1. Worst row >= 10 x the GPU bar for G, wherever the fault reaches."""
    case = CASES[name]
    inp, chain = _chain(name)
    unmasked = R.run_chain(case, inp, lens=None)
    need = 10.0 * R.G_BAR
    for l, (Hin, P, ref) in enumerate(chain):
        d = case["layers"][l]["d"]
        wrong = dict(leak=lambda: R.reference(case, inp, Hin, P, l, leak=True),
                     stale=lambda: R.reference(case, inp, Hin, P, l, stale=R.h_decode(unmasked[l][0], case["B"], case["T"])),
                     tap=lambda: R.reference(case, inp, Hin, P, l, taps=(-d, 0, d + 1)))
        for kind in FAULTS:
            got = wrong[kind]()["G"]
            off = float((got - ref["G"]).abs().amax(-1).max())
            if _fault_reach(case, l, kind):
                assert off >= need, (name, l, kind, off, need)
            else:
                assert off == 0.0, (name, l, kind, off)


def test_every_fault_kind_is_reached():
    for kind in FAULTS:
        hit = [(n, l) for n in FAULT_CASES + ["partial-nolens-d8"] for l in range(len(CASES[n]["layers"])) if _fault_reach(CASES[n], l, kind)]
        assert hit, kind
    # the neighbour's row is zero padding wherever T leaves more than d padded rows: the leak shows on the T = 255 shape (chain-b, partial-nolens) only
    assert not any(_fault_reach(CASES[n], 0, "leak") for n in CASES if n.startswith("edge-"))
    assert _fault_reach(CASES["chain-b"], 0, "leak") and _fault_reach(CASES["chain-b"], 1, "leak") and _fault_reach(CASES["partial-nolens-d8"], 0, "leak")
