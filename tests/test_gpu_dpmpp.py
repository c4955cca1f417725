"""GPU parity of the DPM-Solver++ multistep mel sampler (ss_meldiff_sample_dpmpp: mel_eps + dpmpp_update_kernel of csrc/mel_sampler.hip, the
last transition through the fused DDPM epilogue) through the C-ABI and through forward / mel_stage, against the float64 statements of
tests/dpmpp_refs.py (themselves checked, with the wrong variants they catch, by tests/test_dpmpp_refs_cpu.py).

The nets and helpers are those of tests/test_gpu_sampler_steps.py / tests/test_gpu_mel_sampler_steps.py: production C = 256, L = 20, M = 80,
K_step = 4; B = 2, T = 9, lens = (9, 5); every state buffer (x and the sampler's hist) carries a sentinel tail.

Tolerances (none taken from a kernel's output):
  * controlled dyadic net (eps exact in fp32 in any summation order): per element dpmpp_refs.dpmpp_step_bound - the step's own roundings plus
    the bounds of x and of the stored x0 pushed through the coefficients, chained over the list, the last transition by MR.mel_step_bound;
    padded rows of x and of the stored x0 exactly 0.
  * order 1 against ss_meldiff_sample_ddim(eta = 0), and a cut loop against the whole one: torch.equal.
  * real weights: 4 x the fp32-CPU restatement's own error against float64 on the same inputs, never less than 2 ulp of the largest value.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpmpp_refs as DR  # noqa: E402
import mel_step_refs as MR  # noqa: E402
import test_gpu_mel_sampler_steps as MS  # noqa: E402  (its helpers: _tables, _controlled_model, _extreme, _fresh, _take, _four_x, _sd_pair, _default_dtype)
import test_gpu_sampler_steps as GS  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import restatement as R  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd import plans  # noqa: E402

DEV, SENT, TAIL = GS.DEV, GS.SENT, GS.TAIL
F64, f32 = np.float64, np.float32
K, M = MR.K_MEL, MR.M_MEL
B, T, LENS = 2, 9, [9, 5]
N = B * T * M
VALID = np.arange(T)[None, :] < np.asarray(LENS)[:, None]
_d = GS._d


def _ac64(model):
    return np.ascontiguousarray(model._pk["mel"]["sched"]["alphas_cumprod_f64"])


class _Run:
    """ss_meldiff_sample_dpmpp on one set of inputs: device copies made once, one workspace and one hist (sentinel tail) kept across calls"""

    def __init__(self, model, cond, b=B, t=T, lens=LENS):
        self.net = model._pk["mel"]["net"]
        self.ac64 = _ac64(model)
        self.B, self.T, self.n = b, t, b * t * M
        self.cond, self.lens = _d(cond), _d(np.asarray(lens, np.int32))
        self.wsb = L.load().ss_wavenet_workspace_bytes(ctypes.addressof(self.net), b, t)
        assert self.wsb > 0
        self.ws = torch.empty(self.wsb, device=DEV, dtype=torch.uint8)
        self.hist = torch.full((2 * self.n + TAIL,), SENT, device=DEV)

    def __call__(self, x, ts, order, i_lo=0, i_hi=None, precompute=1):
        ts_h = np.ascontiguousarray(np.asarray(ts, np.int32))
        L.ops.ss_meldiff_sample_dpmpp(self.net, x, self.cond, self.lens, self.B, self.T, ts_h, len(ts_h), i_lo, len(ts_h) if i_hi is None else i_hi, self.ac64,
                                      order, self.hist, precompute, self.ws, self.wsb)
        torch.cuda.synchronize()
        assert bool((self.hist[2 * self.n:] == SENT).all()), "elements beyond 2*B*T*M of hist were written"

    def x0(self):
        return self.hist[self.n:2 * self.n].cpu().numpy().reshape(self.B, self.T, M)

    def ddim(self, x, ts):
        ts_h = np.ascontiguousarray(np.asarray(ts, np.int32))
        L.ops.ss_meldiff_sample_ddim(self.net, x, self.cond, self.lens, self.B, self.T, ts_h, len(ts_h), self.ac64, 0.0, None, 31, None, 1, self.ws, self.wsb)
        torch.cuda.synchronize()


def _case(tables, t0, seed):
    return MR.controlled_mel_case(dict(name="dpmpp", B=B, T=T, lens=LENS, seed=seed), tables, steps=(t0,))


def _judge(what, out, ref, bound, **tags):
    ratio, bad = MR.over_bound(out, ref, bound)
    err = float(np.abs(out.astype(F64) - ref)[np.isfinite(out)].max(initial=0.0))
    record_measurement("dpmpp_" + what, err=err, bound_max=float(bound.max()), err_over_bound=ratio, elements_beyond=bad, **tags)
    print(f"[{what} {tags}] err {err:.3e}, bound max {float(bound.max()):.3e}, {ratio:.3f} x bound, {bad} elements beyond")
    assert np.all(out[~VALID] == 0.0), f"{what} {tags}: rows >= lens are not exactly 0"
    assert bad == 0, f"{what} {tags}: {bad} elements beyond their bound, the worst {ratio:.3g} x"


def _controlled_whole_loop(model, tables, ts, what, seed):
    case = _case(tables, ts[0], seed)
    run = _Run(model, case["cond"])
    buf = MS._fresh(case["x"][ts[0]])
    run(buf, ts, 2)
    out = MS._take(buf, (B, T, M))
    ref = DR.run_dpmpp(case["x"][ts[0]], case["eps"], run.ac64, ts, 2, tables, lens=LENS, e_net=case["e_eps"])
    assert np.all(case["e_eps"] == 0.0) and np.all(ref["e_x"][~VALID] == 0.0)
    _judge(what, out, ref["x"], ref["e_x"], ts=list(ts))
    _judge(what + "_x0", run.x0(), ref["x0"], ref["e_x0"], ts=list(ts))
    return case, ref


# ------------------------------------------------------------------------------------------------
# 1. controlled dyadic net, the whole loop
# ------------------------------------------------------------------------------------------------
def test_controlled_net_whole_loop_order_two():
    """ts = [3, 2, 1, 0], order 2: a first-order first transition, two multistep ones and the final one through the fused epilogue. Every element
    of x within the chained bound, the stored x0 (of position 2) within its own, padded rows of both exactly 0, the sentinels behind x and hist
    intact; the bound is some 1e-6 at the most. What this net cannot show: its eps is the same at every time, so the x0 prediction repeats
    itself from one position to the next (x' = alpha_s x0 + sigma_s eps reproduces x0 where the clamp is idle, and stays beyond the same rail
    where it is not) and only b0 + b1 = c1 is visible, not the split between them - that is the real-weights test's part."""
    tables = MS._tables()
    model = MS._controlled_model()
    assert np.array_equal(_ac64(model), np.cumprod(1.0 - tables["betas"]))
    case, ref = _controlled_whole_loop(model, tables, [3, 2, 1, 0], "controlled", 65)
    assert ref["clamped"] and ref["e_x"].max() < 1e-5


# ------------------------------------------------------------------------------------------------
# 2. order 1 is DDIM with eta = 0, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [[3, 2, 1, 0], [3, 1]])
def test_order_one_equals_ddim_bit_for_bit(ts):
    tables = MS._tables()
    model = MS._controlled_model()
    case = _case(tables, ts[0], 66)
    run = _Run(model, case["cond"])
    a, b = MS._fresh(case["x"][ts[0]]), MS._fresh(case["x"][ts[0]])
    run(a, ts, 1)
    run.ddim(b, ts)
    MS._take(a, (B, T, M))
    ndiff = int((a != b).sum())
    record_measurement("dpmpp_order1_vs_ddim", ts=list(ts), elements_differing=ndiff)
    assert bool(torch.isfinite(a).all()) and float((a[:N] - _d(case["x"][ts[0]]).reshape(-1)).abs().max()) > 1e-2
    assert torch.equal(a, b), f"order 1 on {ts}: {ndiff} elements differ from ss_meldiff_sample_ddim(eta = 0)"
    if len(ts) == 2:
        c = MS._fresh(case["x"][ts[0]])
        run(c, ts, 2)
        assert torch.equal(a, c), "a list of two has a first and a last transition only: first order either way"


# ------------------------------------------------------------------------------------------------
# 3. loop cut
# ------------------------------------------------------------------------------------------------
def test_loop_cut_is_bit_identical():
    """(0, 2) + (2, 4), the second call without the precompute, against the whole list: the second call's first position is second order and
    finds x0 of position 1 in hist. Real weights too (eps depends on x there)."""
    for model, tables, what in ((MS._controlled_model(), MS._tables(), "controlled"), (GS._model("real", GS._base_sd()), MS._tables(), "real")):
        case = _case(tables, 3, 67)
        ts = [3, 2, 1, 0]
        whole_run, cut_run = _Run(model, case["cond"]), _Run(model, case["cond"])
        whole = MS._fresh(case["x"][3])
        whole_run(whole, ts, 2)
        cut = MS._fresh(case["x"][3])
        cut_run(cut, ts, 2, 0, 2, 1)
        mid = cut.clone()
        cut_run(cut, ts, 2, 2, 4, 0)
        MS._take(cut, (B, T, M))
        ndiff = int((cut != whole).sum())
        record_measurement("dpmpp_cut", net=what, elements_differing=ndiff)
        assert not torch.equal(mid, whole)
        assert torch.equal(cut, whole), f"{what}: {ndiff} elements differ from the one-call loop"
        assert torch.equal(cut_run.hist[N:], whole_run.hist[N:]), f"{what}: the stored x0 differs"


def test_fp16sd_mode_cut_and_order_one():
    """mfma_precision = "fp16sd" (3 weight sets and 3 addend sets over 4 evaluations, the shape of test_fp16sd_loop_cut_is_bit_identical): the
    stack leaves its fp32 output in G in every precision mode and evaluation i reads set i % n whichever call it falls into, so the entry
    runs there as it is - finite, cut == whole and order 1 == DDIM(eta = 0), bit for bit."""
    model = GS._model("fp16sd", GS._base_sd(), mfma_precision="fp16sd", fp16sd_sets=3, fp16sd_e_sets=3)
    assert model._pk["mel"]["net"].n_wsets == 3
    inp = GS._mel_inputs()
    b, t, n = inp["B"], inp["T"], inp["B"] * inp["T"] * M
    ts = [3, 2, 1, 0]
    runs = [_Run(model, inp["cond"], b, t, inp["lens"]) for _ in range(2)]
    whole, cut, o1, dd = (MS._fresh(inp["x"]) for _ in range(4))
    runs[0](whole, ts, 2)
    runs[1](cut, ts, 2, 0, 2, 1)
    runs[1](cut, ts, 2, 2, 4, 0)
    assert bool((whole[n:] == SENT).all()) and bool(torch.isfinite(whole).all()) and float((whole[:n] - _d(inp["x"]).reshape(-1)).abs().max()) > 1e-2
    assert torch.equal(cut, whole), f"{int((cut != whole).sum())} elements differ from the one-call loop"
    runs[0](o1, ts, 1)
    runs[0].ddim(dd, ts)
    assert torch.equal(o1, dd), f"{int((o1 != dd).sum())} elements differ from ss_meldiff_sample_ddim(eta = 0)"
    assert not torch.equal(o1, whole)


# ------------------------------------------------------------------------------------------------
# 4. the 1000-step schedule, log-SNR spacing
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_step", [1000, 100])
def test_extreme_schedule_logsnr_list_order_two(k_step):
    """The 1000-step schedule with logsnr_timesteps(., K_step, 6), order 2, within the derived bound per element.
    K_step = 1000: gaps of hundreds of network times next to gaps of tens, coefficients from 1e-5 to 1.5 and sqrt(1 / ac - 1) ~ 5e6 at ts[0]. There
    the x0 prediction is a difference of two values of order 5e6 and the bound on an element inside the rails is of order 1 - a worst case
    the chain carries along, since the next x0 prediction multiplies x by 1 / alpha_s again; it holds the elements beyond a rail, the padded
    rows and the sentinels tightly and the rest loosely. K_step = 100 (a shallow depth inside the same schedule: the entry reads K_step from
    the list alone) starts at sqrt(1 / ac - 1) < 1: the bound is some 1e-6 everywhere and a coefficient off in its last digits shows."""
    model, tables = MS._extreme()
    ac64 = _ac64(model)
    assert model._pk["mel"]["net"].steps == 1000 and len(ac64) == 1000
    ts = plans.logsnr_timesteps(ac64, k_step, 6)
    assert len(ts) == 6 and ts[0] == k_step - 1 and ts[-1] == 0 and min(np.diff(ts[::-1])) * 4 < max(np.diff(ts[::-1])), ts
    case, ref = _controlled_whole_loop(model, tables, ts, "extreme", 68)
    if k_step == 100:
        assert ref["e_x"].max() < 1e-5


# ------------------------------------------------------------------------------------------------
# 5. real weights against a float64 loop
# ------------------------------------------------------------------------------------------------
def _oracle_net(sd, cond, tt):
    """eps = oracle.diffnet per item on its valid frames (the kernels mask rows >= lens, which is the network on the shorter sequence)"""
    np_dt = F64 if tt == torch.float64 else f32

    def net(x, t):
        eps = np.zeros((B, T, M), np_dt)
        with MS._default_dtype(tt):
            for b in range(B):
                n = LENS[b]
                o = R.diffnet(sd, GS._hp(), torch.from_numpy(np.ascontiguousarray(x[b:b + 1, :n])).to(tt), torch.full((1,), t, dtype=torch.long),
                              torch.from_numpy(cond[b:b + 1, :n]).to(tt))
                eps[b, :n] = o[0].numpy()
        return eps
    return net


def test_real_weights_whole_loop_against_float64():
    """Unmodified synthetic weights, ts = [3, 2, 1, 0], order 2: the float64 loop of dpmpp_refs.run_dpmpp around oracle.restatement.diffnet against
    the device, per element within 4 x the error of the same loop in fp32 on the CPU (never less than 2 ulp of the largest value). Here eps
    depends on x and on t: the x0 history is different at every position, and which slot holds what is visible."""
    sd32, sd64 = MS._sd_pair()
    model = GS._model("real", sd32)
    tables = MS._tables()
    r = np.random.default_rng(69)
    x = r.standard_normal((B, T, M)).astype(f32)
    x[~VALID] = 0.0
    cond = (r.standard_normal((B, T, 256)) * 0.5).astype(f32)
    ts = [3, 2, 1, 0]
    run = _Run(model, cond)
    buf = MS._fresh(x)
    run(buf, ts, 2)
    out = MS._take(buf, (B, T, M))
    ref64 = DR.run_dpmpp(x, _oracle_net(sd64, cond, torch.float64), run.ac64, ts, 2, tables, lens=LENS)
    ref32 = DR.run_dpmpp(x, _oracle_net(sd32, cond, torch.float32), run.ac64, ts, 2, tables, lens=LENS, dtype=f32)
    first = DR.run_dpmpp(x, _oracle_net(sd64, cond, torch.float64), run.ac64, ts, 1, tables, lens=LENS)
    assert np.abs(first["x"] - ref64["x"])[VALID].max() > 1e-3, "order 1 and order 2 agree in float64: the history carries no load"
    MS._four_x("dpmpp", out, ref64["x"], ref32["x"].astype(F64), VALID, ts=ts, order=2)
    MS._four_x("dpmpp_x0", run.x0(), ref64["x0"], ref32["x0"].astype(F64), VALID, ts=ts, order=2)


# ------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_untouched():
    lib = L.load()
    tables = MS._tables()
    model = MS._controlled_model()
    case = _case(tables, 3, 70)
    run = _Run(model, case["cond"])
    x = MS._fresh(case["x"][3])
    before = x.clone()
    ok = dict(net=ctypes.addressof(run.net), x=L.ptr(x), cond=L.ptr(run.cond), lens=L.ptr(run.lens), ts=[3, 2, 1, 0], i_lo=0, i_hi=None, ac=run.ac64, order=2,
              hist=L.ptr(run.hist), ws=L.ptr(run.ws), wsb=run.wsb)
    rows = [(dict(net=None), "null pointer"), (dict(x=None), "null pointer"), (dict(cond=None), "null pointer"), (dict(ts=None, n_ts=4), "null pointer"),
            (dict(ac=None), "null pointer"), (dict(hist=None), "null pointer"), (dict(ws=None), "null pointer"),
            (dict(n_ts=0), "n_ts"), (dict(ts=[3, 3, 0]), "strictly decreasing"), (dict(ts=[1, 3]), "strictly decreasing"), (dict(ts=[4, 0]), "strictly decreasing"),
            (dict(ts=[3, -1]), "strictly decreasing"), (dict(i_lo=-1), "position range"), (dict(i_lo=3, i_hi=2), "position range"), (dict(i_hi=5), "position range"),
            (dict(order=0), "order"), (dict(order=3), "order"), (dict(x=L.ptr(x) + 4), "aligned"), (dict(hist=L.ptr(run.hist) + 8), "aligned"),
            (dict(wsb=run.wsb - 1), "workspace too small")]
    for over, text in rows:
        a = dict(ok, **over)
        ts = None if a["ts"] is None else np.ascontiguousarray(np.asarray(a["ts"], np.int32))
        n_ts = a.get("n_ts", 0 if ts is None else len(ts))
        rc = lib.ss_meldiff_sample_dpmpp(a["net"], a["x"], a["cond"], a["lens"], B, T, None if ts is None else L.hptr(ts), n_ts, a["i_lo"],
                                         n_ts if a["i_hi"] is None else a["i_hi"], None if a["ac"] is None else L.hptr(a["ac"]), a["order"], a["hist"], 1, a["ws"],
                                         a["wsb"], L.stream_ptr())
        msg = lib.ss_last_error().decode()
        torch.cuda.synchronize()
        assert rc != 0 and msg.startswith("ss_meldiff_sample_dpmpp: ") and text in msg, (over, rc, msg)
        assert torch.equal(x, before), f"{over}: x was written"
        assert bool((run.hist == SENT).all()), f"{over}: hist was written"


# ------------------------------------------------------------------------------------------------
# 7. through forward
# ------------------------------------------------------------------------------------------------
def test_forward_dpmpp_eager_graph_mel_stage_and_the_default_afterwards():
    """forward(sampler = "dpmpp", mel_steps = 3): eager == captured-and-replayed == replayed again, bit for bit, under the graph slot
    ("dpmpp", times, 2); ret["mel_sampler"] names the list; mel_stage on the forward's own coarse mel and condition gives the same bits; the
    hparams route (mel_sampler / mel_sample_steps) is the same call; and the default forward on the same plan gives, after all that, the bits it
    gave before."""
    from oracle import harness
    from stylesinger_amd.model import StyleSingerHIP
    case = harness.load_case("acoustic_tiny_s4")
    hp, sd, batch = harness.case_setup(case["meta"])
    model = StyleSingerHIP(None, hparams=hp)
    model.load_state_dict(sd, strict=True)
    model.eval().to(DEV)
    bt = {k: v.to(DEV) for k, v in batch.items()}
    c = dict(txt=bt["txt_tokens"], kw=dict(mel2ph=bt["mel2ph"], spk_embed=bt["spk_embed"], emo_embed=bt["emo_embed"], ref_mels=bt["ref_mels"], ref_f0=bt["ref_f0"],
                                           global_steps=320000, infer=True, note=bt["note"], note_dur=bt["note_dur"], note_type=bt["note_type"]))
    seed = 77

    def fwd(m, cc, **kw):     # golden acoustic_tiny_s4 on a model of this test's own (as tests/test_gpu_f0_strided.py builds it): its plans stay here
        ret = m(cc["txt"], **{**cc["kw"], **kw})
        torch.cuda.synchronize()
        return ret
    bucket, graphs = model.t_bucket, model.use_graphs
    try:
        model.t_bucket = 1          # the forward's frame count is the mel_stage call's: one plan, the same launches
        model.use_graphs = "on"
        default_before = fwd(model, c, seed=seed)
        ac64 = _ac64(model)
        ts = plans.logsnr_timesteps(ac64, model.hp["K_step"], 3)
        assert 2 <= len(ts) <= 3
        model.use_graphs = "off"
        eager = fwd(model, c, seed=seed, sampler="dpmpp", mel_steps=3)
        assert eager["mel_sampler"] == dict(name="dpmpp", ts=ts, order=2)
        assert bool(torch.isfinite(eager["mel_out"]).all()) and not torch.equal(eager["mel_out"], default_before["mel_out"])
        staged = model.mel_stage(eager["fs2_mel"], eager["diff_cond"], lens=eager["lens"], sampler="dpmpp", mel_steps=3, seed=seed)
        torch.cuda.synchronize()
        assert torch.equal(staged, eager["mel_out"]), "mel_stage and forward differ"
        model.use_graphs = "on"
        first = fwd(model, c, seed=seed, sampler="dpmpp", mel_steps=3)
        again = fwd(model, c, seed=seed, sampler="dpmpp", mel_steps=3)
        pl = next(p for p in model._plans.values() if ("dpmpp", tuple(ts), 2) in p.graphs)
        assert pl.dpmpp_hist is not None and pl.dpmpp_hist.numel() == 2 * pl.B * pl.T * M
        assert torch.equal(eager["mel_out"], first["mel_out"]) and torch.equal(eager["mel_out"], again["mel_out"])
        other = fwd(model, c, seed=seed + 1, sampler="dpmpp", mel_steps=3)
        assert not torch.equal(other["mel_out"], eager["mel_out"]), "the replay ignores the seed"
        # order 1 is another loop, DDIM's: the same list through sampler="ddim"
        o1 = fwd(model, c, seed=seed, sampler="dpmpp", mel_steps=3, mel_order=1)
        dd = fwd(model, c, seed=seed, sampler="ddim", mel_steps=3, mel_spacing="logsnr")
        assert dd["mel_sampler"] == dict(name="ddim", ts=ts, order=1) and torch.equal(o1["mel_out"], dd["mel_out"])
        # the hparams route
        hp = model.hp
        try:
            model.hp = dict(hp, mel_sampler="dpmpp", mel_sample_steps=3)
            via_hp = fwd(model, c, seed=seed)
        finally:
            model.hp = hp
        assert via_hp["mel_sampler"] == eager["mel_sampler"] and torch.equal(via_hp["mel_out"], eager["mel_out"])
        default_after = fwd(model, c, seed=seed)
        assert "mel_sampler" not in default_after
        for k in ("mel_out", "f0_denorm", "pitch_pred"):
            assert torch.equal(default_before[k], default_after[k]), k
    finally:
        model.t_bucket, model.use_graphs = bucket, graphs
