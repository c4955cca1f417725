"""The 16-bit matrix-core GEMM family at every dilation and tile edge: ss_gemm_bf16 (generic kernel, 64 x 128 and 128 x 128 tiles),
ss_gemm_bf16_gate256 (<4,0>, <8,1>, <8,2>), ss_gemm_bf16_gate128, ss_gemm_bf16_tile256 and the fp16q4 pair ss_gemm_bf16_gate128q / _tile256q against the float64 references "of the same terms"
in tests/hgemm_refs.py, over its `CASES` table (tests/test_hgemm_refs_cpu.py checks the table and the references without a GPU).

Every case is launched twice: with rows >= lens[b] of the A operand zeroed, and with them holding +-1000 (in the fp16 forms the A operand's
never-fetched second plane is poisoned as well). The kernels read zeros outside [0, len) by contract, so every output must be the same bits
in both runs - the tolerance-free test of the range checks and halo fetches. Then the clean run is held against the reference at the bars the
kernels' other unit tests use, per row, so that a failure names (item, row, tile, row in tile)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import hgemm_refs as H  # noqa: E402
from conftest import record_measurement  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402

CASES = H.CASES
DEV = "cuda:0"
SELECT = dict(generic=False, gate256=True, gate128=128, tile256=True, gate128q=128, tile256q=True)   # lib.gemm_bf16's gate256= selector (+ split = 3)
OK_FNS = ("ss_gemm_bf16_gate128_ok", "ss_gemm_bf16_gate256_ok", "ss_gemm_bf16_tile256_ok")


class _Spy:
    """the library with ss_gemm_bf16 wrapped: records what the three dispatch predicates say about the very arguments of the launch"""

    def __init__(self, real):
        self._real, self.oks = real, None

    def __getattr__(self, name):
        return getattr(self._real, name)

    def ss_gemm_bf16(self, args, stream):
        self.oks = tuple(getattr(self._real, f)(args) for f in OK_FNS)
        return self._real.ss_gemm_bf16(args, stream)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _operand(case, x):
    return L.to_bf16(x) if case["split"] == 0 else L.split_bf16(x) if case["split"] == 1 else L.split_f16(x)   # split 2 and 3: the fp16 pair


def _weights(case, inp):
    """device weight sets [G][Np][row] in the operand form of the case, stacked so that set g starts g * w_gs elements in"""
    sets = []
    for g in range(H.n_groups(case)):
        Wp = L.pack_conv_weight(inp["w"][g].to(DEV), interleave_half=case["N"] if case["epi"] == "gate" else 0)
        assert Wp.shape[0] == case["Np"]
        if case["split"] == 0:
            W = L.to_bf16(Wp)
        elif case["split"] == 1:
            W = L.split_bf16(Wp)
        elif case["split"] == 3:   # the lo plane as block-scaled fp4 in the kernel's lane order
            W = (L.pack_gate_q4 if case["epi"] == "gate" else L.pack_skip_q4)(Wp, shift=H.WSHIFT)[0]
        else:
            W = L.split_f16(Wp, scale=2.0 ** H.WSHIFT)
            if case["one_product"]:
                hi = L.split_planes(W)[0]
                W = hi.to(torch.float16).contiguous() if case["one_product"] == 2 else L.split_f16(hi, scale=1.0)   # compact [Np][K] | lo terms zero
        sets.append(W)
    W = torch.stack(sets).contiguous()
    return W, W.shape[1] * W.shape[2]


def _per_group(case, t):
    """[G, n] fp32 -> device tensor and its group stride"""
    t = t.contiguous().to(DEV)
    return t, t.shape[1]


def _launch(case, inp, poison, lib_spy=None):
    """one launch of the case -> dict of the raw output buffers (device). poison: what rows >= len of A (and A's dead plane) hold."""
    B, T, K, N, s = case["B"], case["T"], case["K"], case["N"], case["split"]
    lens_l = H.case_lens(case)
    lens = None if case["lens"] is None else torch.tensor(lens_l, dtype=torch.int32, device=DEV)
    A = _operand(case, H.with_tail(case, inp["x"], False).to(DEV))
    if case["a_compact"]:
        A = L.split_planes(A)[0].to(torch.float16).contiguous()            # [B, T, K]: the hi terms only
    if poison:
        A = A.clone()
        cols = torch.arange(A.shape[-1], device=DEV)
        for b in range(B):
            n = T - lens_l[b]
            if n:
                sign = 1.0 - 2.0 * ((torch.arange(n, device=DEV)[:, None] + cols[None, :]) % 2).float()
                A[b, lens_l[b]:] = (H.POISON * sign).to(A.dtype)
        if s >= 2 and not case["a_compact"]:
            A.view(B, T, -1, 64)[..., 32:] = H.POISON                      # the second plane of EVERY row: never fetched
    W, w_gs = _weights(case, inp)
    kw = dict(B=B, T=T, K=K, taps=case["taps"], N=N, Np=case["Np"], lens=lens, split=s, out_scale=H.out_scale(case), gate256=SELECT[case["kernel"]],
              mask_rows=case["mask_rows"], gate_mode=case["gate_mode"], one_product=case["one_product"], a_compact=case["a_compact"],
              group_size=case["group_size"], w_gs=w_gs if case["group_size"] else 0, q_scale=case.get("q_scale", 0.0))
    out = {}
    if case["epi"] == "gate":
        bias, bgs = _per_group(case, H.pack_addend(inp["bias"], N))
        E = H.pack_addend(inp["E"], N).to(DEV)
        slot = 2 * N if s else N                                           # 16-bit elements per layer slot
        GA = torch.full((B, T, 2 * slot), H.SENTINEL, device=DEV, dtype=torch.bfloat16 if s < 2 else torch.float16)
        kw.update(epi=L.HEPI_GATE, E=E, lde=2 * N, bias=bias, bias_gs=bgs if case["group_size"] else 0, out=GA[..., slot:], ldc=2 * slot,
                  c_bs=T * 2 * slot)
        out["C"] = GA
    elif case["epi"] == "store":
        bias, bgs = _per_group(case, inp["bias"])
        S = torch.full((B, T, N + 8), H.SENTINEL, device=DEV)
        kw.update(epi=L.HEPI_STORE, bias=bias, bias_gs=bgs if case["group_size"] else 0, out=S, ldc=N + 8, c_bs=T * (N + 8),
                  act=L.ACT_RELU if case["act"] == "relu" else L.ACT_NONE)
        out["C"] = S
    else:
        bias, bgs = _per_group(case, inp["bias"])
        nb, ngs = _per_group(case, inp["next_bias"])
        kw.update(epi=L.HEPI_RESX, bias=bias, bias_gs=bgs if case["group_size"] else 0, next_bias=nb, next_bias_gs=ngs if case["group_size"] else 0,
                  post_scale=H.POST_SCALE)
        if case["epi"] == "resx":
            X = inp["X0"].to(DEV).clone()
            Y = torch.full((B, T, 2 * N if s else N), H.SENTINEL, device=DEV, dtype=torch.bfloat16 if s < 2 else torch.float16)
            kw.update(X=X, Y=Y)
            out["X"], out["Y"] = X, Y
        else:
            cb, cgs = _per_group(case, inp["cur_bias"])
            cb_item = torch.stack([inp["cur_bias"][H.item_group(case, b)] for b in range(B)])[:, None, :]
            Y = _operand(case, (inp["X0"] + cb_item).to(DEV))
            yh, ym = H.stream_in(case, inp)
            assert torch.equal(_bits(Y).cpu(), _bits(H.interleave32(yh, ym).to(Y.dtype))), "the stream before the launch is the CPU restatement's"
            kw.update(X=None, Y=Y, cur_bias=cb, cur_bias_gs=cgs if case["group_size"] else 0)
            out["Y"] = Y
    if lib_spy is not None:
        real = L.load()
        spy = _Spy(real)
        lib_spy.setattr(L, "load", lambda: spy)
        try:
            L.gemm_bf16(A, W, **kw)
        finally:
            lib_spy.setattr(L, "load", lambda: real)
        assert spy.oks == (0, 0, 0), f"{case['name']} is meant for the generic kernel, the dispatch predicates say {dict(zip(OK_FNS, spy.oks))}"
    else:
        L.gemm_bf16(A, W, **kw)
    torch.cuda.synchronize()
    return out


def _values(case, raw):
    """raw device buffers -> dict name -> float64 CPU [B, T, N] (a pair's two terms summed), after the sentinel checks"""
    N, s = case["N"], case["split"]
    out = {}
    for k, t in raw.items():
        if case["epi"] == "gate":
            slot = 2 * N if s else N
            assert torch.all(t[..., :slot].float() == H.SENTINEL), "the neighbouring layer slot is untouched"
            mine = t[..., slot:]
            if s == 0:
                out[k] = mine.double().cpu()
            else:
                hi, lo = (p.double().cpu() for p in L.split_planes(mine))
                if s >= 2:
                    assert torch.all(lo == H.SENTINEL), "the gate output's second plane is not written in the fp16 forms"
                out[k] = hi + lo if s == 1 else hi
        elif case["epi"] == "store":
            assert torch.all(t[..., N:] == H.SENTINEL), "columns beyond N are untouched"
            out[k] = t[..., :N].double().cpu()
        elif k == "X" or s == 0:
            out[k] = t.double().cpu()
        else:
            hi, lo = (p.double().cpu() for p in L.split_planes(t))
            out[k] = hi + lo
    return out


_CLEAN = {}


def _clean_values(name, lib_spy=None):
    """(raw buffers, values) of the clean run of a case; the short cases are kept for the cross-kernel comparisons"""
    if name not in _CLEAN or lib_spy is not None:
        case = CASES[name]
        raw = _launch(case, H.make_inputs(case), False, lib_spy)
        res = raw, _values(case, raw)
        if case["T"] > 1000:
            return res
        _CLEAN[name] = res
    return _CLEAN[name]


def _check_against(case, got, want, bars, what):
    """per-row max error of every output against `want` (list per item) under `bars`; returns the worst error relative to its bar"""
    worst = {}
    for k, bar in bars.items():
        rows = [(got[k][b] - want[k][b]).abs().amax(-1) for b in range(case["B"])]
        e, b, t, tile, rt = H.worst_row(case, rows)
        worst[k] = e
        print(f"{case['name']} {what} {k}: max err {e:.3e} (bar {bar:.1e}) at item {b} row {t} = tile {tile} row {rt}")
        assert e <= bar, f"{case['name']} {what} {k}: {e:.3e} > {bar:.1e} at item {b}, row {t} (tile {tile}, row {rt} of {H.tile_rows(case)}; len {H.case_lens(case)[b]})"
    return worst


@pytest.mark.parametrize("split", [0, 1, 2])
def test_operand_forms_are_bit_equal_to_the_cpu_restatement(split):
    g = torch.Generator(device="cpu").manual_seed(11 + split)
    x = torch.randn(3, 41, 96, generator=g) * 3.0
    w = torch.randn(64, 3 * 96, generator=g) / (3 * 96) ** 0.5
    if split == 0:
        assert torch.equal(_bits(L.to_bf16(x.to(DEV))).cpu(), _bits(H.to_bf16_cpu(x)))
        assert torch.equal(_bits(L.to_bf16(w.to(DEV))).cpu(), _bits(H.to_bf16_cpu(w)))
    elif split == 1:
        assert torch.equal(_bits(L.split_bf16(x.to(DEV))).cpu(), _bits(H.split_bf16_cpu(x)))
        assert torch.equal(_bits(L.split_bf16(w.to(DEV))).cpu(), _bits(H.split_bf16_cpu(w)))
    else:
        assert torch.equal(_bits(L.split_f16(x.to(DEV))).cpu(), _bits(H.split_f16_cpu(x)))
        assert torch.equal(_bits(L.split_f16(w.to(DEV), scale=2.0 ** H.WSHIFT)).cpu(), _bits(H.split_f16_cpu(w, 2.0 ** H.WSHIFT)))
        hi, lo = L.split_planes(L.split_f16(x.to(DEV)))
        assert torch.equal(hi.cpu(), H.planes(H.split_f16_cpu(x))[0]) and torch.equal(lo.cpu(), H.planes(H.split_f16_cpu(x))[1])
    # the packed row order of a gate weight is the addend's column order
    wg = torch.randn(128, 32, 3, generator=g)
    Wp = L.pack_conv_weight(wg.to(DEV), interleave_half=64).cpu()
    assert torch.equal(Wp, H.pack_addend(wg.permute(2, 1, 0), 64).permute(2, 0, 1).reshape(128, 96))


@pytest.mark.parametrize("name", list(CASES))
def test_hgemm_case(name, monkeypatch):
    """poisoned run == clean run, bit for bit; clean run against the float64 reference of the same terms, per row; rows >= len exactly 0."""
    case = CASES[name]
    inp = H.make_inputs(case)
    raw, got = _clean_values(name, monkeypatch if case["kernel"] == "generic" else None)
    raw_p = _launch(case, inp, True)
    for k in raw:
        same = torch.equal(_bits(raw[k]), _bits(raw_p[k]))
        if not same:
            diff = (_bits(raw[k]) != _bits(raw_p[k])).flatten(2).any(-1).cpu()
            b, t = (int(v) for v in diff.nonzero()[0])
            tile = H.tile_rows(case)
            pytest.fail(f"{name} {k}: what rows >= len of A hold reaches the output; first at item {b} row {t} (tile {t // tile}, row {t % tile}; "
                        f"len {H.case_lens(case)[b]}), {int(diff.sum())} rows differ")
    ref = H.reference(case, inp)
    worst = _check_against(case, got, ref, H.gpu_bars(case), "vs float64 of the same terms")
    lens = H.case_lens(case)
    if case["mask_rows"]:
        for k, v in got.items():
            for b in range(case["B"]):
                assert float(v[b, lens[b]:].abs().sum()) == 0.0, f"{name} {k}: rows >= len of item {b} are not 0"
    if case["split"] == 0 and case["epi"] in ("gate", "resx"):      # one bf16 term: almost always the reference's own bf16
        k, mean_bar = ("C", 2e-4) if case["epi"] == "gate" else ("Y", 1e-3)
        m = sum(float((got[k][b] - ref[k][b].float().to(torch.bfloat16).double()).abs().sum()) for b in range(case["B"])) / got[k].numel()
        print(f"{name}: mean |{k} - bf16(ref)| {m:.3e}")
        assert m <= mean_bar, (name, m)
    record_measurement("hgemm_edges", case=name, err=max(worst.values()), **{f"err_{k}": v for k, v in worst.items()})


def _siblings(kernel, of):
    """(case on `kernel`, the case that differs from it in the kernel alone and runs on `of`)"""
    by_key = {(H.data_key(c), c["kernel"]): n for n, c in CASES.items()}
    out = []
    for n, c in CASES.items():
        if c["kernel"] == kernel and c["T"] <= 1000 and (H.data_key(c), of) in by_key:
            out.append((n, by_key[(H.data_key(c), of)]))
    return out


@pytest.mark.parametrize("a,b", _siblings("gate128", "gate256"))
def test_gate128_equals_gate256_bit_for_bit(a, b):
    (ra, _), (rb, _) = _clean_values(a), _clean_values(b)
    assert torch.equal(_bits(ra["C"]), _bits(rb["C"])), f"{a} vs {b}: same steps, same tiles per accumulator, same epilogue arithmetic"


@pytest.mark.parametrize("a,b", _siblings("gate256", "generic") + _siblings("tile256", "generic"))
def test_many_round_kernels_equal_the_generic_kernel(a, b):
    """same arithmetic contract, results equal up to the K summation order: the bars of the reference comparison. The fp16 GATE writes ONE
    fp16 term, and 3e-4 is half an ulp of values in [0.5, 1) + the activations' error: two such outputs meet it against each other only as the
    same bits wherever their fp32 values lie near a rounding boundary. They are the same bits: the generic kernel feeds its accumulators in the
    order of gate256_kernel<8, 2> (chunk_tap in gemm_bf16.hip; with the tap-major order it had before, these pairs were 2^-11 = 4.883e-04 apart
    in a few elements of every case with T > 1), so a launch does not depend on the kernel the dispatcher picks for its size."""
    case = CASES[a]
    (_, va), (_, vb) = _clean_values(a), _clean_values(b)
    _check_against(case, va, {k: [v[i] for i in range(case["B"])] for k, v in vb.items()}, H.gpu_bars(case), f"vs {b}")
    if case["epi"] == "gate" and case["split"] == 2:
        ra, rb = _clean_values(a)[0]["C"], _clean_values(b)[0]["C"]
        n = int((_bits(ra) != _bits(rb)).sum())
        assert n == 0, f"{a} vs {b}: {n} of {ra.numel()} fp16 terms differ (same K order, same epilogue arithmetic: bit-identical)"


def test_the_table_pairs_every_many_round_gate_case_with_its_generic_twin():
    assert len(_siblings("gate128", "gate256")) >= 7 and len(_siblings("gate256", "generic")) >= 18 and len(_siblings("tile256", "generic")) >= 4


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: no launch happens
# ------------------------------------------------------------------------------------------------------------------------------
def _big_gate_args(**over):
    """a fp16x2 GATE launch of the production size (64 x 8192 rows: every dispatch predicate takes it); pointers are never followed by the predicates"""
    a = L.GemmBf16Args()
    a.A = a.W = a.C = a.E = 1 << 20
    a.B, a.T, a.K, a.N, a.Np = 64, 8192, 256, 256, 512
    a.lda, a.a_batch_stride, a.ldc, a.c_batch_stride, a.lde, a.e_batch_stride = 512, 8192 * 512, 512, 8192 * 512, 512, 8192 * 512
    a.ntaps, a.epi, a.split, a.out_scale, a.mask_rows = 3, L.HEPI_GATE, 2, 2.0 ** -8, 1
    taps = over.pop("taps", (-8, 0, 8))
    for i, o in enumerate(taps):
        a.tap_off[i] = o
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_gate_kernels_refuse_what_their_halo_cannot_hold():
    lib = L.load()
    for fn in (lib.ss_gemm_bf16_gate256_ok, lib.ss_gemm_bf16_gate128_ok):
        assert fn(C.byref(_big_gate_args())) == 1                      # the predicate is live at this size ...
        assert fn(C.byref(_big_gate_args(taps=(-9, 0, 9)))) == 0        # ... and refuses d > HALO,
        assert fn(C.byref(_big_gate_args(K=192, lda=384))) == 0         # K != 256
        assert fn(C.byref(_big_gate_args(taps=(-3, 0, 5)))) == 0        # and asymmetric taps
        assert fn(C.byref(_big_gate_args(taps=(-4, 1, 4)))) == 0
    B, T, N = 1, 64, 256
    A = torch.zeros(B, T, 2 * N, device=DEV, dtype=torch.float16)
    W = torch.zeros(2 * N, 2 * 3 * N, device=DEV, dtype=torch.float16)
    G = torch.full((B, T, 2 * N), H.SENTINEL, device=DEV, dtype=torch.float16)
    for sel in (True, 128):
        with pytest.raises(L.StyleSingerHipError):
            L.gemm_bf16(A, W, B=B, T=T, K=N, taps=(-9, 0, 9), N=N, Np=2 * N, epi=L.HEPI_GATE, out=G, split=2, out_scale=2.0 ** -8, gate256=sel)
    torch.cuda.synchronize()
    assert torch.all(G == H.SENTINEL)
