"""The float64 statements of tests/sampler_step_refs.py checked on their own (no GPU) against the oracle, so that a wrong reference cannot pass a
wrong kernel; the input conditions tests/test_gpu_sampler_steps.py relies on, asserted from the reference alone (which frames' voicing decisions
are too close to call, and that every named edge regime keeps decided frames); and an fp32 numpy emulation of the sampler step that shows each
hand mutation of the step failing the very check the GPU test applies to the kernel."""
import math

import numpy as np
import pytest
import torch

import sampler_step_refs as SR
from oracle import restatement as O
from stylesinger_amd import config, synth

F64 = np.float64
STEPS = (SR.S_F0 - 1, 1, 0)


def _hp():
    return config.make_hparams(dict(timesteps=4, K_step=4, f0_timesteps=SR.S_F0))


_SD = {}


def _sd():
    if not _SD:
        _SD["sd"] = synth.synth_acoustic_state_dict(_hp(), 77)
    return _SD["sd"]


def _tables():
    hp = _hp()
    t = {**synth.multinomial_schedule(hp["f0_timesteps"], hp["f0_max_beta"]), **synth.gaussian_schedule(hp["f0_timesteps"], hp["f0_max_beta"])}
    return {k: v.numpy() for k, v in t.items() if v.dim() == 1}


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = SR.controlled_case(name, _tables())
    return _CASES[name]


# ------------------------------------------------------------------------------------------------
# the statements against the oracle
# ------------------------------------------------------------------------------------------------
def test_tables_are_the_state_dicts():
    sd, t = _sd(), _tables()
    for k, v in t.items():
        assert np.array_equal(sd["f0_gen." + k].numpy(), v), k


@pytest.mark.parametrize("net", ["gm_diffnet", "gm_diffnet_inpainte"])
def test_f0_joint_step_follows_gm_sample_step_by_step(net):
    """oracle.gm_sample with a trace, and the statement fed the oracle's own network outputs (ddiffnet on the state before each step) and the
    same tape: the classes are identical at every step, f0 is within the fp32 roundings of the oracle's own arithmetic (f0_step_bound, e_eps = 0:
    both read the same fp32 eps)."""
    hp, sd = _hp(), _sd()
    B, T, seed = 2, 37, 5
    g = torch.Generator().manual_seed(3)
    cond = torch.randn(B, T, hp["hidden_size"], generator=g) * 0.5
    mid = torch.rand(B, T, generator=g) * 2 - 1
    lo, hi = mid - 0.25, mid + 0.25
    trace = []
    with torch.no_grad():
        O.gm_sample(sd, hp, "f0_gen", net, cond, lo, hi, synth.NoiseTape(seed), trace=trace)
    tape = synth.NoiseTape(seed)
    tape.rand(B, 1, T)
    f0, uv = tape.randn(B, 1, T)[:, 0], torch.zeros(B, T, dtype=torch.long)
    tables = {k: sd["f0_gen." + k].numpy() for k in _tables()}
    worst, min_margin = 0.0, np.inf
    for (i, f0_or, uv_or) in trace:
        with torch.no_grad():
            out = O.ddiffnet(sd, hp, f0, uv, torch.full((B,), i, dtype=torch.long), cond, net)
        z, u = tape.randn(B, 1, T)[:, 0], tape.rand(B, 2, T)
        coef = SR.f0_coef(tables, i)
        f0n, uvn, margin, _ = SR.f0_joint_step(f0, uv, out[..., 0], out[..., 1:], lo, hi, z, u, coef, i)
        assert np.array_equal(uvn, uv_or.numpy()), f"step {i}: classes differ from the oracle's"
        bound = SR.f0_step_bound(f0, out[..., 0], lo, hi, z, coef, i, 0.0)
        worst = max(worst, float((np.abs(f0n - f0_or.double().numpy()) / bound).max()))
        min_margin = min(min_margin, float(np.abs(margin).min()))
        f0, uv = f0_or, uv_or
    assert len(trace) == SR.S_F0 and worst <= 1.0, worst
    assert min_margin > 1e-4     # the identity above is not luck: no frame of this case sits on a tie


def test_f0_input_row_is_ddiffnet_input():
    """the two lines of oracle.ddiffnet that build the stack's input (net.py:249-252)"""
    hp, sd = _hp(), _sd()
    p = "gm_diffnet"
    g = torch.Generator().manual_seed(4)
    f0, uv = torch.randn(2, 9, generator=g), torch.randint(0, 2, (2, 9), generator=g)
    a = O.conv1d_cl(f0[:, :, None], sd[p + ".input_projection.weight"], sd[p + ".input_projection.bias"])
    ref = torch.cat([a, sd[p + ".uv_embed.weight"][uv]], dim=-1).double().numpy()
    X = SR.f0_input_row(f0, uv, sd[p + ".input_projection.weight"].reshape(-1), sd[p + ".input_projection.bias"], sd[p + ".uv_embed.weight"], lens=[9, 4])
    assert X.shape == (2, 9, hp["f0_residual_channels"])
    assert np.all(X[1, 4:] == 0) and np.abs(X[0] - ref[0]).max() < 4e-7 and np.abs(X[1, :4] - ref[1, :4]).max() < 4e-7
    assert np.array_equal(X[..., 96:][0], sd[p + ".uv_embed.weight"][uv[0]].double().numpy())


def test_mel_pair_against_mel_diffusion():
    """oracle.mel_diffusion at K_step = 4 with the denoiser's output projection zeroed (eps = 0): its first traced state is
    c1 clamp(recip x) + c2 x + sigma z of the q-sample x (c2[3] ~ 0.5: nothing is lost in the clamp), its return value the denorm of its last."""
    hp = _hp()
    sd = dict(_sd())
    for k in ("postdiff.denoise_fn.output_projection.weight", "postdiff.denoise_fn.output_projection.bias"):
        sd[k] = torch.zeros_like(sd[k])
    B, T, M, K = 1, 6, 80, hp["K_step"]
    g = torch.Generator().manual_seed(6)
    coarse = (torch.randn(B, T, M, generator=g) * 0.8 - 3.0)
    cond = torch.randn(B, T, hp["hidden_size"], generator=g) * 0.5
    trace = []
    with torch.no_grad():
        mel = O.mel_diffusion(sd, hp, coarse, cond, synth.NoiseTape(8), trace=trace)
    tape = synth.NoiseTape(8)
    zq = tape.randn(B, 1, M, T)[:, 0].transpose(1, 2)
    z1 = tape.randn(B, 1, M, T)[:, 0].transpose(1, 2).double().numpy()
    t = lambda k: sd["postdiff." + k].double().numpy()
    smin, smax = t("spec_min")[0, 0], t("spec_max")[0, 0]
    x, _ = SR.mel_qsample(coarse, smin, smax, t("sqrt_alphas_cumprod")[K - 1], t("sqrt_one_minus_alphas_cumprod")[K - 1], zq)
    i = K - 1
    assert t("posterior_mean_coef2")[i] > 0.1
    x1 = t("posterior_mean_coef1")[i] * np.clip(t("sqrt_recip_alphas_cumprod")[i] * x, -1, 1) + t("posterior_mean_coef2")[i] * x \
        + math.exp(0.5 * t("posterior_log_variance_clipped")[i]) * z1
    assert trace[0][0] == i and np.abs(x1 - trace[0][1].double().numpy()).max() < 2e-6
    out, _ = SR.mel_denorm(trace[-1][1], smin, smax, lens=[4])
    assert np.all(out[0, 4:] == 0) and np.abs(out[0, :4] - mel[0, :4].double().numpy()).max() < 2e-6
    assert np.abs(out[0, :4]).max() > 1.0


def test_argmax_takes_the_first_maximum():
    s = torch.tensor([0.25, 0.5, 0.5])
    assert SR.first_argmax2(s, torch.tensor([0.25, 0.5, 0.75])).tolist() == [0, 0, 1]
    assert torch.stack([s, s], -1).argmax(-1).tolist() == [0, 0, 0]      # what torch's argmax gives the reference on a tie


# ------------------------------------------------------------------------------------------------
# input conditions of the GPU test
# ------------------------------------------------------------------------------------------------
def _variants(name):
    if name == "reduced":   # the shape of test_controlled_net_reduced_skip_source, from the library's own host-side pick
        from stylesinger_amd import lib as L
        pick = L.load().ss_gemm16_ksplit_pick
        T = next(t for t in range(1, 4000) if t % 16 and pick(16, t, SR.C_F0, 10 * SR.C_F0) == 1)
        return [SR.controlled_case(SR.reduced_spec(16, T), _tables())]
    c = _case(name)
    return [c, SR.swapped_items(c)] if SR.CASES[name]["paired"] else [c]


@pytest.mark.parametrize("name", sorted(SR.CASES) + ["reduced"])
def test_controlled_cases_keep_their_regimes_and_few_undecided_frames(name):
    tables = _tables()
    wset = SR.CASES[name]["wset"] if name in SR.CASES else "near0"
    for case in _variants(name):
        reg, valid = case["regimes"], case["valid"]
        n_valid = int(valid.sum())
        seen, seen_target = set(), set()
        for step in STEPS:
            ref = SR.controlled_step(case, tables, step)
            cpu = SR.controlled_step(case, tables, step, dtype=torch.float32)
            chk = SR.check_controlled_step(case, tables, step, cpu["f0"], cpu["uv"])
            und = chk["undecided"]
            assert int(und.sum()) <= 0.01 * n_valid, (case["name"], step, int(und.sum()), n_valid)
            assert chk["flips"] == 0 and chk["f0_ratio"] <= 1.0, "the fp32 CPU step itself must pass the GPU test's check"
            assert float(chk["thr"].max()) < 0.2 * SR.TARGET_DELTA
            dec = ~und
            masks = dict(uv0=reg["uv0"], uv1=reg["uv1"], pin=reg["pin"], band=reg["band"], idle=reg["idle"], edge0=reg["edge0"][step],
                         edge1=reg["edge1"][step], target=reg["target"][step])
            if (~valid).any():
                masks["padded"] = reg["padded"]
            for g in set(case["net_of_item"].tolist()):
                masks[f"net{g}"] = np.broadcast_to((case["net_of_item"] == g)[:, None], valid.shape)
            if not reg["target"].any():    # the swapped variant
                del masks["target"]
            for k, m in masks.items():
                assert int((m & dec & valid).sum() if k not in ("padded", "target") else (m & dec).sum()) >= 3, (case["name"], step, k)
            for e in SR.U_EDGE:   # every edge value, in either slot
                assert ((case["u"][step][:, 0] == np.float32(e)) & reg["edge0"][step] & dec & valid).any()
                assert ((case["u"][step][:, 1] == np.float32(e)) & reg["edge1"][step] & dec & valid).any()
            # the regimes do what their names say
            coef = SR.f0_coef(tables, step)
            raw = coef["recip"] * case["f0"].astype(F64) - coef["recipm1"] * ref["eps"]
            lo, hi = case["lo"].astype(F64), case["hi"].astype(F64)
            assert np.all(lo[reg["pin"]] == hi[reg["pin"]]) and np.all((raw > lo + 1.0) & (raw < hi - 1.0) | ~reg["idle"])
            clipped = (raw < lo) | (raw > hi)
            assert clipped[reg["band"] & valid].any() and (~clipped)[reg["band"] & valid].any()
            assert np.all(np.abs(ref["margin"][reg["target"][step]]) > 0.5 * SR.TARGET_DELTA)
            assert np.all(np.abs(ref["margin"][reg["target"][step]]) < 2.0 * SR.TARGET_DELTA)
            seen |= set(ref["uv"][valid].tolist())
            seen_target |= set(ref["uv"][reg["target"][step]].tolist())
        # both classes come out, on targeted frames too (at step 0 a +-40 net leaves one class only)
        assert seen == {0, 1} and (seen_target == {0, 1} or not reg["target"].any())
        d = ref["logits"][..., 0] - ref["logits"][..., 1]
        for g in set(case["net_of_item"].tolist()):
            want = SR.WEIGHT_SETS[wset][g]
            sel = valid & (case["net_of_item"] == g)[:, None]
            assert np.all(np.abs(d[sel] - want) < 1e-4 * max(1.0, abs(want)))
        assert np.all(ref["logits"][~valid] == 0) and np.all(ref["eps"][~valid] == 0)
    if wset == "pm40":
        assert np.exp(np.float32(-39.9)) * np.float32(2 ** 24) < 1e-9     # the smaller softmax term is far below an fp32 ulp of the larger


def test_the_two_nets_of_a_weight_set_differ_everywhere():
    for wset in SR.WEIGHT_SETS:
        a, b = SR.controlled_weights(wset)
        for k in ("beta", "w_final", "b_final"):
            assert not np.any(a[k] == b[k]), (wset, k)
        assert (a["beta"] > 0).sum() > 50 and (a["beta"] < 0).sum() > 50
        assert abs(float(a["b_final"][0])) > 0.1 and abs(float(b["b_final"][0])) > 0.1     # a padded frame given b_final would show in f0


# ------------------------------------------------------------------------------------------------
# hand mutations of an fp32 emulation of the step, judged by the GPU test's own check
# ------------------------------------------------------------------------------------------------
f32 = np.float32


def _lae(a, b):
    m = np.maximum(a, b)
    return (m + np.log(np.exp(a - m) + np.exp(b - m))).astype(f32)


def _emulate_step(case, tables, step, mut=None, slices=True):
    """The tail launch of one step in fp32 numpy, device memory laid out as the packer does (net g sits gs_* floats after net 0; the packed final
    projection is padded to 32 rows), with one optional mutation. slices: the stack's output is read as split-K slices (all zero here) + bias +
    ReLU; else from the reduced tensor the GEMM wrote."""
    B, T, C = case["B"], case["T"], SR.C_F0
    ws = case["weights"]
    gs_bskip, gs_wf, gs_bf = C, 32 * C, 32
    bskip = np.concatenate([w["beta"] for w in ws] + [np.zeros(C, f32)])
    wfin, bfin = np.zeros(2 * gs_wf, f32), np.zeros(2 * gs_bf, f32)
    for g, w in enumerate(ws):
        wfin[g * gs_wf:g * gs_wf + 3 * C] = w["w_final"].ravel()
        bfin[g * gs_bf:g * gs_bf + 3] = w["b_final"]
    tm1 = step if mut == "tm1_is_t" else max(step - 1, 0)
    tab = lambda k, i: f32(tables[k][i])
    recip, recipm1, c1, c2 = (tab(k, step) for k in ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2"))
    sigma = f32(np.exp(f32(0.5) * tab("posterior_log_variance_clipped", step))) if step > 0 else f32(0)
    la, l1a, lcp, l1cp = tab("log_alpha", step), tab("log_1_min_alpha", step), tab("log_cumprod_alpha", tm1), tab("log_1_min_cumprod_alpha", tm1)
    LOG2, TINY = f32(0.6931471805599453), f32(-69.07755278982137)
    f0o, uvo = np.zeros((B, T), f32), np.zeros((B, T), np.int32)
    for b in range(B):
        g = int(case["net_of_item"][b])
        masked = np.arange(T) >= case["lens"][b]
        off = g * (gs_bf if mut == "gs_bf_for_gs_bskip" else gs_bskip)
        gv = np.maximum(bskip[off:off + C], 0) if slices else np.maximum(ws[g]["beta"], 0)
        a = wfin[g * gs_wf:g * gs_wf + 3 * C].reshape(3, C) @ gv
        out = (a + bfin[g * gs_bf:g * gs_bf + 3]).astype(f32)
        keep_bias = mut == "masked_get_b_final"
        eps, l0, l1 = (np.where(masked, bfin[g * gs_bf + j] if keep_bias else f32(0), out[j]).astype(f32) for j in range(3))
        u0, u1 = case["u"][step][b, 0], case["u"][step][b, 1]
        if mut == "swap_u":
            u0, u1 = u1, u0
        x, lo, hi, z = case["f0"][b], case["lo"][b], case["hi"][b], case["z"][step][b]
        if mut == "lo_hi_swapped":
            lo, hi = hi, lo
        x0 = np.minimum(np.maximum(recip * x - recipm1 * eps, lo), hi)
        f0o[b] = (c1 * x0 + c2 * x) + sigma * z
        cls = case["uv"][b] != 0
        lx0, lx1 = np.where(cls, TINY, f32(0)), np.where(cls, f32(0), TINY)
        m = np.maximum(l0, l1)
        lse = np.log(np.exp(l0 - m) + np.exp(l1 - m))
        p0, p1 = (l0 - m) - lse, (l1 - m) - lse
        if step == 0 and mut != "no_step0_branch":
            ev0, ev1 = p0, p1
        else:
            ev0, ev1 = _lae(p0 + lcp, np.full(T, l1cp - LOG2, f32)), _lae(p1 + lcp, np.full(T, l1cp - LOG2, f32))
        un0 = ev0 + _lae(lx0 + la, np.full(T, l1a - LOG2, f32))
        un1 = ev1 + _lae(lx1 + la, np.full(T, l1a - LOG2, f32))
        mm = np.maximum(un0, un1)
        nl = mm + np.log(np.exp(un0 - mm) + np.exp(un1 - mm))
        q0, q1 = un0 - nl, un1 - nl
        g0 = -np.log(-np.log(u0 + f32(1e-30)) + f32(1e-30))
        g1 = -np.log(-np.log(u1 + f32(1e-30)) + f32(1e-30))
        s0, s1 = (g0 + q0).astype(f32), (g1 + q1).astype(f32)
        uvo[b] = (s1 >= s0) if mut == "ge_argmax" else (s1 > s0)
    return f0o, uvo


def _passes(case, tables, step, f0o, uvo):
    chk = SR.check_controlled_step(case, tables, step, f0o, uvo)
    return chk["f0_ratio"] <= 1.0 and chk["flips"] == 0, chk


STEP_MUTATIONS = {   # mutation -> the steps at which it must be caught (every one is caught at one of the GPU test's three steps)
    "tm1_is_t": (SR.S_F0 - 1, 1), "no_step0_branch": (0,), "swap_u": STEPS, "gs_bf_for_gs_bskip": STEPS, "masked_get_b_final": STEPS,
    "lo_hi_swapped": STEPS,
}


# at step 0 of the near0 nets the prior mixing of the missing branch moves the margin by 3.6e-4 at most (log cp_0 = -1e-4), less than the targeted
# frames' 5e-3: only a net with a strong preference (pm40: ev = -40 against log((1 - cp_0) / 2) = -9.9) shows it
NOT_VISIBLE = {("near0_rem14", "no_step0_branch")}


@pytest.mark.parametrize("name", ["pm40_b4", "near0_rem14"])
def test_emulated_step_passes_and_each_mutation_fails(name):
    tables = _tables()
    for case in _variants(name):
        for step in STEPS:
            for slices in (True, False):
                ok, chk = _passes(case, tables, step, *_emulate_step(case, tables, step, slices=slices))
                assert ok, (case["name"], step, slices, chk["f0_ratio"], chk["flips"])
        for mut, steps in STEP_MUTATIONS.items():
            if (name, mut) in NOT_VISIBLE or case is not _case(name):    # the swapped variant has no targeted frames
                continue
            for step in steps:
                ok, chk = _passes(case, tables, step, *_emulate_step(case, tables, step, mut=mut))
                assert not ok, f"{case['name']}: mutation {mut} passes at step {step}"
                print(f"{case['name']} step {step} {mut}: f0 {chk['f0_ratio']:.3g} x bound, {chk['flips']} decided frames flipped")
    # the strides only bear load in the slices form: the reduced tensor already carries each net's bias
    case = _case(name)
    assert _passes(case, tables, 1, *_emulate_step(case, tables, 1, mut="gs_bf_for_gs_bskip", slices=False))[0]


def test_tie_break_mutation_needs_the_samplers_own_arithmetic():
    """`>=` for `>` changes a frame only on an exact fp32 tie of g1 + q1 and g0 + q0 - two different expressions, so a tie is a property of one
    implementation's libm and cannot be placed from the float64 statement (a frame that close is 'undecided' by construction). Shown on the
    emulation: a uniform found by scanning the fp32 grid ties in the emulation, the mutation flips exactly that frame, and the check (rightly)
    does not see it. The statement's own tie rule is test_argmax_takes_the_first_maximum."""
    tables = _tables()
    base = _case("near0_rem14")
    step, N, t = 1, 20001, 1
    tile = lambda a: np.ascontiguousarray(np.broadcast_to(a[..., t:t + 1], a.shape[:-1] + (N,)))
    # one frame's inputs N times over. The class the posterior favours by |m| gets g = 0 (u = 1/e, where one grid step moves g by less than an
    # fp32 ulp of the sum, so a sign change of the margin passes through an exact tie) and is scanned; the other class gets g = |m|
    case = dict(base, B=1, T=N, lens=np.array([N], np.int32), net_of_item=base["net_of_item"][:1], valid=np.ones((1, N), bool),
                **{k: tile(base[k][:1]) for k in ("f0", "uv", "lo", "hi")}, z=tile(base["z"][:, :1]), u=tile(base["u"][:, :1]).copy())
    case["u"][step] = 0.5
    m = SR.controlled_step(case, tables, step)["margin"][0, 0]      # g1 = g0: q1 - q0
    hi_slot = 1 if m < 0 else 0
    u_hi = f32(SR._gumbel_inv(abs(m)))
    case["u"][step, 0, 1 - hi_slot] = (math.exp(-1.0) + (np.arange(N) - N // 2) * SR.U24).astype(f32)
    ties = []
    for j in range(16):
        case["u"][step, 0, hi_slot] = f32(u_hi + j * SR.U24)
        assert 0.5 < case["u"][step, 0, hi_slot].max() < 1.0
        a, b = _emulate_step(case, tables, step), _emulate_step(case, tables, step, mut="ge_argmax")
        assert a[1][0, 0] != a[1][0, -1], "the margin does not change sign over the scanned grid"
        ties = np.flatnonzero(a[1][0] != b[1][0])
        if len(ties):
            break
    assert 1 <= len(ties) < 50, "no exact tie on the fp32 grid"
    assert np.all(a[1][0, ties] == 0) and np.all(b[1][0, ties] == 1)
    chk = SR.check_controlled_step(case, tables, step, *b)
    assert np.all(chk["undecided"][0, ties]) and chk["flips"] == 0


# ---- the X hand-over: a two-step loop over a toy network of the input row ----
def _toy_net(X, P):
    return np.tanh(X @ P) * np.array([1.0, 3.0, 3.0], X.dtype)


def _input_row32(f0, uv, w):
    half = SR.C_F0 // 2
    X = np.concatenate([w["w_in"][None, None, :] * f0[..., None] + w["b_in"], w["emb"][(uv != 0).astype(int)]], -1).astype(f32)
    assert X.shape[-1] == 2 * half
    return X


def _emulate_loop(case, tables, w, cuts, mut=None):
    """fp32 loop over steps S-1 .. S-2 in the calls `cuts` = [(lo, hi), ...]: the first evaluation of a call reads the input kernel's row, later
    ones the row the previous step's tail wrote - with `x_before_update`, from the f0 / uv it read rather than the ones it wrote."""
    f0, uv = case["f0"].copy(), case["uv"].copy()
    for lo_s, hi_s in cuts:
        X = None
        for step in reversed(range(lo_s, hi_s)):
            if step == hi_s - 1:
                X = _input_row32(f0, uv, w)
            out = _toy_net(X, w["P"]).astype(f32)
            c = dict(case, f0=f0, uv=uv)
            f0n, uvn, _, _ = SR.f0_joint_step(f0, uv, out[..., 0], out[..., 1:], case["lo"], case["hi"], case["z"][step], case["u"][step],
                                              SR.f0_coef(tables, step), step, dtype=torch.float32)
            f0n, uvn = f0n.astype(f32), uvn.astype(np.int32)
            X = _input_row32(*((f0, uv) if mut == "x_before_update" else (f0n, uvn)), w)
            f0, uv = f0n, uvn
            del c
    return f0, uv


def test_x_handover_mutation_breaks_the_loop_cut_identity():
    """What the GPU test's loop-cut cases assert, on the emulation: one call over two steps equals two calls of one step bit for bit, and a tail
    that writes the next input row before its own update does not."""
    tables = _tables()
    case = _case("near0_rem14")
    r = np.random.default_rng(9)
    half = SR.C_F0 // 2
    w = dict(w_in=r.standard_normal(half).astype(f32), b_in=r.standard_normal(half).astype(f32) * f32(0.1),
             emb=r.standard_normal((2, half)).astype(f32), P=(r.standard_normal((SR.C_F0, 3)) / 14).astype(f32))
    S = SR.S_F0
    whole = _emulate_loop(case, tables, w, [(S - 2, S)])
    cut = _emulate_loop(case, tables, w, [(S - 1, S), (S - 2, S - 1)])
    assert np.array_equal(whole[0], cut[0]) and np.array_equal(whole[1], cut[1])
    bad = _emulate_loop(case, tables, w, [(S - 2, S)], mut="x_before_update")
    assert not np.array_equal(bad[0], cut[0]) and not np.array_equal(bad[1], cut[1])
