"""The float64 statements of tests/small_kernel_refs.py checked on their own (no GPU), so that a wrong reference cannot pass a wrong kernel,
plus the input conditions the GPU test relies on: the share of pitch_post frames near a coarse-bin boundary and the length regulator's
distance from every rounding tie."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_kernel_refs as R
from oracle import restatement as O


def _rng(seed):
    return np.random.default_rng(seed)


@pytest.mark.parametrize("Tq,Tk,qlens,klens", [(9, 13, None, None), (40, 37, [40, 17], [37, 5]), (5, 8, [5, 3], [0, 8])])
def test_attention_matches_sdpa_with_a_key_mask(Tq, Tk, qlens, klens):
    g = _rng(1)
    B, H, D = 2, 2, 16
    q, k, v = g.standard_normal((B, Tq, H * D)), g.standard_normal((B, Tk, H * D)), g.standard_normal((B, Tk, H * D))
    scale = D ** -0.5
    out, written = R.attention(q, k, v, H=H, D=D, scale=scale, qlens=qlens, klens=klens)
    for b in range(B):
        m = Tq if qlens is None else qlens[b]
        n = Tk if klens is None else klens[b]
        assert written[b].tolist() == [t < m for t in range(Tq)]
        assert np.all(out[b, m:] == 0)
        if n == 0:
            assert np.all(out[b] == 0)
            continue
        tq, tk, tv = (torch.from_numpy(a[b]).view(-1, H, D).transpose(0, 1) for a in (q, k, v))   # [H, T, D] float64
        mask = (torch.arange(Tk) < n)[None, None, :].expand(H, Tq, Tk)
        ref = F.scaled_dot_product_attention(tq, tk, tv, attn_mask=mask, scale=scale).transpose(0, 1).reshape(Tq, H * D)
        assert np.abs(out[b, :m] - ref.numpy()[:m]).max() < 1e-13


@pytest.mark.parametrize("n", [1, 2, 7])
def test_lstm_matches_torch_lstm(n):
    from stylesinger_amd.emotion import pack_whh
    torch.manual_seed(3)
    H, P, cin = 256, 3, 40
    m = torch.nn.LSTM(cin, H, 1, batch_first=True).double()
    x = torch.randn(P, n, cin, dtype=torch.float64)
    with torch.no_grad():
        ref, (h_n, _) = m(x)
        xproj = x @ m.weight_ih_l0.t() + m.bias_ih_l0 + m.bias_hh_l0
    got = R.lstm_layer(xproj.numpy(), m.weight_hh_l0.detach().numpy())
    assert np.abs(got - ref.numpy()).max() < 1e-13
    assert np.abs(got[:, -1] - h_n[0].numpy()).max() < 1e-13
    # the kernel-side layouts are pure re-indexings of the same numbers
    xi = R.interleave_gates(xproj.numpy())
    assert xi.shape == (P, n, H, 4) and xi[1, n - 1, 5, 2] == xproj[1, n - 1, 2 * H + 5].item()
    wp = pack_whh(m.weight_hh_l0.detach(), H)
    assert tuple(wp.shape) == (H, H, 4) and wp.is_contiguous()
    for (kk, j, gate) in [(0, 0, 0), (3, 200, 1), (255, 7, 2), (17, 255, 3)]:
        assert wp[kk, j, gate] == m.weight_hh_l0[gate * H + j, kk]


@pytest.mark.parametrize("C", [1, 63, 130, 512])
def test_layernorm_matches_torch(C):
    g = _rng(4)
    x = g.standard_normal((2, 5, C)) * 3 + 1
    ga, be = g.standard_normal(C) + 1, g.standard_normal(C)
    ref = F.layer_norm(torch.from_numpy(x), (C,), torch.from_numpy(ga), torch.from_numpy(be), 1e-5).numpy()
    assert np.abs(R.layernorm(x, ga, be) - ref).max() < 1e-12
    y = R.layernorm(x, ga, be, lens=[5, 2], mask_rows=True)
    assert np.all(y[1, 2:] == 0) and np.array_equal(y[0], R.layernorm(x, ga, be)[0])
    assert np.array_equal(R.layernorm(x, ga, be, lens=None, mask_rows=True), R.layernorm(x, ga, be))


@pytest.mark.parametrize("n,pad", [(10, 3), (10, 9), (4, 9), (3, 20), (2, 5), (1, 4)])
def test_reflect_pad_matches_numpy_pad(n, pad):
    x = _rng(5).standard_normal((2, 12)).astype(np.float32)
    Ly = 12 + 2 * pad + 3
    y = R.reflect_pad(x, [n, 0], Ly, pad)
    assert np.array_equal(y[0, :n + 2 * pad], np.pad(x[0, :n], pad, mode="reflect"))
    assert np.all(y[0, n + 2 * pad:] == 0) and np.all(y[1] == 0)
    # the definition: index i - pad folded with period 2 (n - 1), the edge sample not repeated (n == 1: the sample itself)
    for i in range(n + 2 * pad):
        s = 0
        if n > 1:
            s = (i - pad) % (2 * (n - 1))
            s = s if s < n else 2 * (n - 1) - s
        assert y[0, i] == x[0, s]


@pytest.mark.parametrize("Tp", R.LR_TPS)
def test_length_regulator_matches_the_oracle_and_a_literal_loop(Tp):
    logdur, tokens, target = R.length_regulator_inputs(Tp)
    dur, none, lens = R.length_regulate(logdur, tokens, 0)
    assert none is None
    # durations: the oracle's out2dur (restatement.duration_predictor's last line) on the same numbers, pads zeroed
    od = torch.clamp(torch.round(torch.from_numpy(logdur).double().exp() - 1.0), min=0).long().numpy() * (tokens != 0)
    assert np.array_equal(dur, od)
    assert np.array_equal(dur, np.where(tokens != 0, np.maximum(np.rint(target), 0), 0).astype(np.int64))   # the integer targets come back
    T = int(lens.max())
    ref = O.length_regulator(torch.from_numpy(dur), torch.from_numpy(tokens == 0)).numpy()
    if T > 0:
        _, m2p, lens_t = R.length_regulate(logdur, tokens, T)
        assert np.array_equal(m2p, ref) and np.array_equal(lens_t, lens)
    if T > 5:
        _, m2p, lens_c = R.length_regulate(logdur, tokens, T - 5)
        assert np.array_equal(m2p, ref[:, :T - 5]) and np.array_equal(lens_c, np.minimum(lens, T - 5))
    # a literal loop
    for b in range(tokens.shape[0]):
        frames = []
        for i in range(Tp):
            frames += [i + 1] * int(dur[b, i])
        assert lens[b] == len(frames)
        assert frames == [int(v) for v in ref[b, :len(frames)]]
    assert lens[-1] == 0 and np.all(dur[-1] == 0)   # the all-pad item


@pytest.mark.parametrize("Tp", R.LR_TPS)
def test_length_regulator_inputs_keep_their_distance_from_every_tie(Tp):
    """§4 of the issue: nothing is excluded, because no entry sits within 0.25 of a tie (1e-6: the fp32 rounding of logdur)."""
    logdur, tokens, _ = R.length_regulator_inputs(Tp)
    margin = R.tie_margin(logdur)
    assert (margin < 0.25 - 1e-6).sum() == 0, margin.min()
    if Tp >= 8:
        assert logdur[0, 1] < 0 and logdur[0, 2] == 0 and tokens[0, 4] == 0 and tokens[1, -1] == 0 and tokens[0, -1] != 0
    assert np.all(tokens[-1] == 0)


@pytest.mark.parametrize("T", [1, 64, 65, 200])
def test_positions_match_the_oracle(T):
    nz = _rng(6).random((3, T)) < 0.7
    ref = O.make_positions(torch.from_numpy(nz)).numpy()
    assert np.array_equal(R.make_positions(nz), ref)


def test_pitch_statements_match_the_oracle():
    f0_a, uv_a, f0_b, uv_b, midi, mel2ph = R.pitch_post_inputs()
    t = lambda a: torch.from_numpy(a)   # noqa: E731
    pp, hz, coarse = O.pitch_post(t(f0_a).double(), t(uv_a), t(f0_b).double(), t(uv_b), t(midi), t(mel2ph))
    rp, rhz, rc, coord = R.pitch_post(f0_a, uv_a, f0_b, uv_b, midi, mel2ph)
    assert np.abs(rp - pp.numpy()).max() < 1e-12 and np.abs(rhz - hz.numpy()).max() < 1e-9
    keep = ~R.coarse_band(coord, 1e-9)
    assert np.array_equal(rc[keep], coarse.numpy()[keep])
    m = np.arange(257) % 128
    lo, hi = O.f0_bounds(t(m).double())
    rlo, rhi = R.f0_bounds(m)
    assert np.abs(rlo - lo.numpy()).max() < 1e-12 and np.abs(rhi - hi.numpy()).max() < 1e-12
    assert rlo.min() == -1 and rhi.max() == 1 and np.all(rlo <= rhi)


def test_pitch_post_inputs_meet_the_exclusion_cap_and_hit_both_clamps():
    """§4 of the issue: `coarse` is compared where the float64 bin coordinate is farther than 1e-3 from a .5 boundary; at most 1 % of the frames
    may be excluded, by the float64 reference alone. The clamp cases sit well inside their bins."""
    f0_a, uv_a, f0_b, uv_b, midi, mel2ph = R.pitch_post_inputs()
    pp, hz, coarse, coord = R.pitch_post(f0_a, uv_a, f0_b, uv_b, midi, mel2ph)
    share = R.coarse_band(coord).mean()
    assert share <= 0.01, share
    assert np.all(coarse[:4] == 1) and np.all(coarse[4:8] == 255) and np.all(hz[:8] > 0)
    assert not R.coarse_band(coord)[:14].any()
    assert pp[:, 0].min() < 5.7 and pp[:, 0].max() > 10.3                      # f0 spans [-1.2, 1.2] -> log2 Hz [5.6, 10.4]
    assert sorted(set(pp[:, 1].tolist())) == [0.0, 0.5, 1.0]
    assert pp[12, 1] == 1.0 and hz[12] == 0 and hz[13] == 0 and pp[13, 1] == 0.0   # the rest and the padding frame
    assert ((midi == 0) & (mel2ph > 0)).sum() > 20 and ((mel2ph == 0) & (midi > 0)).sum() > 20
    voiced = hz > 0
    assert voiced.sum() > 200 and coarse[voiced].min() == 1 and coarse[voiced].max() == 255


def test_one_line_statements():
    g = _rng(8)
    src = g.standard_normal((2, 5, 4)).astype(np.float32)
    m2p = np.array([[0, 1, 5, 6, -2, 3], [2, 2, 0, 5, 1, 7]])
    out = R.gather_expand(src, m2p)
    ref = O.expand_states(torch.from_numpy(src), torch.from_numpy(m2p.clip(0, 5))).numpy()
    ref[(m2p < 0) | (m2p > 5)] = 0
    assert np.array_equal(out, ref)
    assert np.array_equal(R.gather_expand(np.arange(10).reshape(2, 5), m2p), [[0, 0, 4, 0, 0, 2], [6, 6, 0, 9, 5, 0]])
    tab = g.standard_normal((6, 4))
    assert np.array_equal(R.embedding([-1, 0, 5, 6], tab, 2.0), 2.0 * tab[[0, 0, 5, 5]])
    assert np.array_equal(R.table_add([0, 5, 6, 9], tab, 0.5, prev=np.ones((4, 4))), 0.5 * tab[[0, 5, 5, 5]] + 1)
    x = np.array([[[1.0, 0.0], [0.0, 3.0], [2.0, 0.0], [0.0, 0.0]], [[0.0, 1.0], [0.0, 2.0], [0.0, 0.0], [0.0, 5.0]]])
    assert R.ref_lens(x).tolist() == [3, 0]
    assert R.count_positive(np.array([[1, 0, -3, 7], [0, 0, 0, 0]])).tolist() == [2, 0]
    assert np.array_equal(R.mask_rows_by_ref(np.ones((3, 2)), [1.0, 0.0, -2.0]), [[1, 1], [0, 0], [1, 1]])
    assert np.array_equal(R.add_rowscalar(np.zeros((1, 3, 2)), np.array([[1.0, 2.0, 3.0]]), lens=[2]), [[[1, 1], [2, 2], [0, 0]]])
    v = np.array([[10.0, 20.0]])
    got = R.add_bcast_mask(np.ones((1, 2, 2)), v1=v, y2=np.full((1, 2, 2), 0.5), lens=[1])
    assert np.array_equal(got, [[[11.5, 21.5], [0, 0]]])
    S = np.array([[3.0, 0.0, 9.0, 4.0, 1.0, 9.0]])
    assert np.array_equal(R.spec_magnitude(S, 2, 3, 4), [[5, 1, 0, 0]]) and np.array_equal(R.spec_magnitude(S, 2, 3, 4, power=True), [[25, 1, 0, 0]])
    assert np.array_equal(R.log10_floor([1e-12, 1e-10, 100.0], 1e-10), [-10, -10, 2])
    wav = np.zeros((4, 8)); wav[0, :4] = 1e-3; wav[0, 4:] = 0.5; wav[1] = 0.5; wav[3] = 0.1
    gain = R.normalize_volume_gain(wav, [4, 8, 8, 0], -30.0)
    assert abs(gain[0] - 10 ** 1.5) < 1e-9 and gain[1] == 1 and gain[2] == 1 and gain[3] == 1
    xf = np.array([[1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.0, 65520.0, 1e-8, 3.0]], np.float32)
    y = R.round_f16_rows(xf, [5], [6], 8)
    assert y[0, :4].tolist() == [1.0, 1 + 2.0 ** -9, 65504.0, float("inf")] and y[0, 4] == np.float32(np.float16(1e-8)) and np.all(y[0, 5:] == 0)
    nd = R.note_dur_add(np.ones((2, 2)), [2.0, 3.0], [0.5, 1.0], [1.0, -1.0])
    assert np.array_equal(nd, [[3.0, 2.0], [3.5, 3.0]])
    assert abs(R.mean_l2norm(np.array([[3.0, 0.0], [3.0, 8.0]]))[1] - 0.8) < 1e-15 and np.allclose(R.l2norm_rows(np.array([[3.0, 4.0]])), [[0.6, 0.8]])
