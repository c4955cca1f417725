"""GPU unit parity of the encoder-side and producer kernels at the shapes production calls them with: each one through the C-ABI against the
float64 statement of the same op in tests/small_kernel_refs.py (itself checked by tests/test_small_kernel_refs_cpu.py).

Every output buffer is filled with a sentinel (7.0 / -7) before the call, so that an element the kernel should have written but did not, or one
it should have left alone but wrote, shows.

Tolerances (none of them derived from a kernel's output):
  * copies, gathers, masks and integer work: bit-exact;
  * one or two fp32 operations per element (embedding, table_add, note_dur_add, add_rowscalar): each rounds by at most half an ulp of its own
    result, so the output stays within 1 ulp of fp32 at the largest magnitude the element passes through (`_assert_ulps`; the inputs are chosen so
    that no more than two operations round, see the tests);
  * fp32 arithmetic (layernorm, LSTM, norms, spec, log10, volume, f0 bounds, pitch_pred / f0_denorm, attention at large logits): the same op is
    run in fp32 torch on the CPU; the kernel's error against float64 may be 4 x the CPU's own (a different but legitimate summation order, libm
    differences), never less than 2 ulp of the output's magnitude (`_check_derived`). Kernel error, CPU error and bound are recorded;
  * attention at unit-variance scores keeps the project's 1e-5, layernorm at C = 80 / 256 its 5e-6 where that is tighter.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import small_kernel_refs as R  # noqa: E402
from conftest import record_measurement  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.emotion import pack_whh  # noqa: E402

SENT = 7.0


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _sent(*shape, dtype=torch.float32, value=SENT):
    return torch.full(shape, value, dtype=dtype, device=dev())


def _np(t):
    return t.detach().cpu().numpy()


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(g, *shape, scale=1.0):
    return (g.standard_normal(shape) * scale).astype(np.float32)


def _check_derived(name, out, cpu32, ref64, cap=None, **info):
    """the 4 x rule of the module docstring; `cap` = an existing project tolerance that holds where it is tighter"""
    out, cpu32, ref64 = np.asarray(out, np.float64), np.asarray(cpu32, np.float64), np.asarray(ref64, np.float64)
    err = float(np.abs(out - ref64).max()) if np.isfinite(out).all() else float("inf")
    cpu_err = float(np.abs(cpu32 - ref64).max())
    floor = 2.0 * float(np.spacing(np.float32(np.abs(ref64).max())))
    bound = max(4.0 * cpu_err, floor)
    if cap is not None:
        bound = min(bound, cap)
    record_measurement("small_" + name, kernel_err=err, cpu_fp32_err=cpu_err, bound=bound, ratio=err / bound, **info)
    print(f"[{name}] kernel {err:.3e} cpu-fp32 {cpu_err:.3e} bound {bound:.3e}")
    assert err <= bound, (name, err, cpu_err, bound)


def _assert_ulps(out, ref64, mag, n=1):
    """|out - ref64| <= n ulp of fp32 at magnitude `mag` (elementwise: the largest value the element passes through)"""
    mag = np.maximum(np.abs(np.asarray(mag, np.float64)), np.abs(ref64)).astype(np.float32)
    tol = n * np.spacing(np.maximum(mag, np.float32(2.0 ** -100))).astype(np.float64)
    bad = np.abs(np.asarray(out, np.float64) - ref64) > tol
    assert not bad.any(), (int(bad.sum()), float(np.abs(out - ref64).max()))


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
H_ATT, D_ATT = 2, 128
HD = H_ATT * D_ATT


def _attention(q, k, v, o, *, Tq, Tk, qlens, klens, scale):
    """q / k / v / o are (possibly column-block) views of device buffers [B, T, ld]"""
    B = q.shape[0]
    ql = None if qlens is None else _d(np.asarray(qlens, np.int32))
    kl = None if klens is None else _d(np.asarray(klens, np.int32))
    L.attention(q, k, v, o, B=B, H=H_ATT, D=D_ATT, Tq=Tq, Tk=Tk, ldq=q.stride(1), ldk=k.stride(1), ldv=v.stride(1), ldo=o.stride(1),
                q_bs=q.stride(0), k_bs=k.stride(0), v_bs=v.stride(0), o_bs=o.stride(0),
                qlens=ql, klens=kl, scale=scale)
    torch.cuda.synchronize()


def _attention_cpu32(q, k, v, scale, qlens, klens):
    out = torch.zeros(q.shape[0], q.shape[1], HD)
    q, k, v = (torch.from_numpy(a) for a in (q, k, v))
    for b in range(q.shape[0]):
        m, n = int(qlens[b]), int(klens[b])
        for h in range(H_ATT):
            c = slice(h * D_ATT, (h + 1) * D_ATT)
            if n:
                out[b, :m, c] = torch.softmax((q[b, :m, c] * scale) @ k[b, :n, c].t(), -1) @ v[b, :n, c]
    return out.numpy()


def _check_attention_rows(o, ref, written, tol):
    o = _np(o)
    assert np.all(o[~written] == SENT), "a row >= qlen was written"
    err = np.abs(o[written].astype(np.float64) - ref[written]).max()
    assert np.isfinite(o[written]).all() and err < tol, err
    return err


def test_attention_fused_qkv_self():
    """model.py's self-attention form: Q, K, V are the three column blocks of ONE [B,T,3H] buffer (ld = 3H), qlens and klens both given."""
    B, T = 3, 130
    lens = [130, 97, 1]
    qkv = _f32(_rng(101), B, T, 3 * HD)
    buf = _d(qkv)
    att = _sent(B, T, HD)
    scale = D_ATT ** -0.5
    _attention(buf[:, :, :HD], buf[:, :, HD:2 * HD], buf[:, :, 2 * HD:], att, Tq=T, Tk=T, qlens=lens, klens=lens, scale=scale)
    ref, written = R.attention(qkv[..., :HD], qkv[..., HD:2 * HD], qkv[..., 2 * HD:], H=H_ATT, D=D_ATT, scale=scale, qlens=lens, klens=lens)
    err = _check_attention_rows(att, ref, written, 1e-5)
    record_measurement("small_attention_fused_qkv", kernel_err=float(err), bound=1e-5, ratio=float(err) / 1e-5)


def test_attention_cross_strides_and_qlen_on_a_block_boundary():
    """model.py's cross-attention form: ldq = H, K and V the two halves of a [B,Tk,2H] buffer, Tq != Tk, qlen = 128 = one query block."""
    B, Tq, Tk = 2, 257, 45
    qlens, klens = [257, 128], [45, 33]
    g = _rng(102)
    q, kv = _f32(g, B, Tq, HD), _f32(g, B, Tk, 2 * HD)
    qd, kvd = _d(q), _d(kv)
    att = _sent(B, Tq, HD)
    scale = D_ATT ** -0.5
    _attention(qd, kvd[:, :, :HD], kvd[:, :, HD:], att, Tq=Tq, Tk=Tk, qlens=qlens, klens=klens, scale=scale)
    ref, written = R.attention(q, kv[..., :HD], kv[..., HD:], H=H_ATT, D=D_ATT, scale=scale, qlens=qlens, klens=klens)
    err = _check_attention_rows(att, ref, written, 1e-5)
    record_measurement("small_attention_cross", kernel_err=float(err), bound=1e-5, ratio=float(err) / 1e-5)


def test_attention_item_without_keys_gives_exact_zeros():
    B, Tq, Tk = 2, 40, 8
    qlens, klens = [33, 40], [0, 5]
    g = _rng(103)
    q, k, v = _f32(g, B, Tq, HD), _f32(g, B, Tk, HD), _f32(g, B, Tk, HD)
    att = _sent(B, Tq, HD)
    scale = D_ATT ** -0.5
    _attention(_d(q), _d(k), _d(v), att, Tq=Tq, Tk=Tk, qlens=qlens, klens=klens, scale=scale)
    ref, written = R.attention(q, k, v, H=H_ATT, D=D_ATT, scale=scale, qlens=qlens, klens=klens)
    _check_attention_rows(att, ref, written, 1e-5)
    o = _np(att)
    assert np.all(o[0, :33] == 0.0) and np.isfinite(o[0, :33]).all()


def test_attention_key_tile_edges():
    """klen just below, at and just above the 32-key tile"""
    B, Tq, Tk = 3, 35, 40
    klens = [31, 32, 33]
    g = _rng(104)
    q, k, v = _f32(g, B, Tq, HD), _f32(g, B, Tk, HD), _f32(g, B, Tk, HD)
    att = _sent(B, Tq, HD)
    scale = D_ATT ** -0.5
    _attention(_d(q), _d(k), _d(v), att, Tq=Tq, Tk=Tk, qlens=None, klens=klens, scale=scale)
    ref, written = R.attention(q, k, v, H=H_ATT, D=D_ATT, scale=scale, klens=klens)
    _check_attention_rows(att, ref, written, 1e-5)
    # the keys at and past klen carry weight in no row: moving them changes nothing
    k2, v2 = k.copy(), v.copy()
    for b, n in enumerate(klens):
        k2[b, n:] += 50.0
        v2[b, n:] -= 50.0
    att2 = _sent(B, Tq, HD)
    _attention(_d(q), _d(k2), _d(v2), att2, Tq=Tq, Tk=Tk, qlens=None, klens=klens, scale=scale)
    assert torch.equal(att, att2)


def test_attention_large_logits():
    """Q scaled so that the scores reach +-60: the online-softmax rescale across key tiles. Bound: the 4 x rule."""
    B, Tq, Tk = 2, 130, 100
    klens = [100, 77]
    g = _rng(105)
    q, k, v = _f32(g, B, Tq, HD, scale=15.0), _f32(g, B, Tk, HD), _f32(g, B, Tk, HD)
    scale = D_ATT ** -0.5
    s = np.einsum("bqc,bkc->bqk", q[..., :D_ATT].astype(np.float64), k[..., :D_ATT].astype(np.float64)) * scale
    assert s.max() > 60 and s.min() < -60, (s.min(), s.max())
    att = _sent(B, Tq, HD)
    _attention(_d(q), _d(k), _d(v), att, Tq=Tq, Tk=Tk, qlens=None, klens=klens, scale=scale)
    ref, _ = R.attention(q, k, v, H=H_ATT, D=D_ATT, scale=scale, klens=klens)
    _check_derived("attention_large_logits", _np(att), _attention_cpu32(q, k, v, scale, [Tq] * B, klens), ref)


# ------------------------------------------------------------------------------------------------
# layernorm
# ------------------------------------------------------------------------------------------------
def _layernorm(x_flat, y_flat, gamma, beta, *, B, T, C, ldx, ldy, xbs, ybs, lens, mask_rows, eps=1e-5):
    L.check(L.load().ss_layernorm(L.ptr(x_flat), L.ptr(y_flat), L.ptr(gamma), L.ptr(beta), B, T, C, ldx, ldy, xbs, ybs, eps,
                                  L.ptr(lens), int(mask_rows), L.stream_ptr()), "ss_layernorm")
    torch.cuda.synchronize()


def _ln_cpu32(x, ga, be):
    return F.layer_norm(torch.from_numpy(x), (x.shape[-1],), torch.from_numpy(ga), torch.from_numpy(be), 1e-5).numpy()


@pytest.mark.parametrize("C", [1, 63, 65, 80, 130, 256, 257, 384, 512])
def test_layernorm_strided_masked_every_width(C):
    """every instantiation (C <= 128, <= 256, <= 512), widths that are no multiple of 64, ldx = C + 4 with their own batch strides, B * T = 21 rows
    (no multiple of the 4 rows per block), mask_rows with lens (one item empty) and without."""
    B, T = 3, 7
    g = _rng(200 + C)
    x = (_f32(g, B, T, C) * 3 + 1).astype(np.float32)
    ga, be = (_f32(g, C) + 1).astype(np.float32), _f32(g, C)
    ldx, ldy = C + 4, C + 8
    xbs, ybs = T * ldx + 8, T * ldy + 12
    xs = np.full((B, xbs), 1e6, np.float32)
    for b in range(B):
        xs[b, :T * ldx].reshape(T, ldx)[:, :C] = x[b]
    xd, gd, bd = _d(xs), _d(ga), _d(be)
    ref = R.layernorm(x, ga, be)
    cpu = _ln_cpu32(x, ga, be)
    lens = np.array([7, 0, 4], np.int32)
    keep = (np.arange(T)[None, :] < lens[:, None])[..., None]
    for form, (lens_d, mask_rows, want, cpu_want) in {
            "lens": (_d(lens), 1, ref * keep, cpu * keep), "mask_rows_without_lens": (None, 1, ref, cpu), "no_mask": (_d(lens), 0, ref, cpu)}.items():
        y = _sent(B, ybs)
        _layernorm(xd, y, gd, bd, B=B, T=T, C=C, ldx=ldx, ldy=ldy, xbs=xbs, ybs=ybs, lens=lens_d, mask_rows=mask_rows)
        yn = _np(y)
        rows = yn[:, :T * ldy].reshape(B, T, ldy)
        assert np.all(rows[:, :, C:] == SENT) and np.all(yn[:, T * ldy:] == SENT), "wrote outside the C columns of a row"
        if form == "lens":
            assert np.all(rows[1, :, :C] == 0) and np.all(rows[2, 4:, :C] == 0)
        _check_derived(f"layernorm_C{C}_{form}", rows[:, :, :C], cpu_want, want, cap=5e-6 if C in (80, 256) else None)


@pytest.mark.parametrize("C", [130, 512])
def test_layernorm_in_place(C):
    B, T = 2, 9
    g = _rng(230 + C)
    x = (_f32(g, B, T, C) * 2 - 0.5).astype(np.float32)
    ga, be = (_f32(g, C) + 1).astype(np.float32), _f32(g, C)
    xd = _d(x)
    _layernorm(xd, xd, _d(ga), _d(be), B=B, T=T, C=C, ldx=C, ldy=C, xbs=T * C, ybs=T * C, lens=None, mask_rows=0)
    _check_derived(f"layernorm_C{C}_in_place", _np(xd), _ln_cpu32(x, ga, be), R.layernorm(x, ga, be))


def test_layernorm_large_mean_small_spread():
    """rows with mean 1e3 and spread 1e-2: only a two-pass variance survives (E[x^2] - E[x]^2 in fp32 has no digit left)"""
    B, T, C = 1, 33, 384
    g = _rng(260)
    x = (1e3 + 1e-2 * g.standard_normal((B, T, C))).astype(np.float32)
    ga, be = (_f32(g, C) + 1).astype(np.float32), _f32(g, C)
    y = _sent(B, T, C)
    _layernorm(_d(x), y, _d(ga), _d(be), B=B, T=T, C=C, ldx=C, ldy=C, xbs=T * C, ybs=T * C, lens=None, mask_rows=0)
    xt = torch.from_numpy(x)
    mu = xt.mean(-1, keepdim=True)
    cpu = ((xt - mu) / torch.sqrt(((xt - mu) ** 2).mean(-1, keepdim=True) + 1e-5) * torch.from_numpy(ga) + torch.from_numpy(be)).numpy()
    _check_derived("layernorm_large_mean", _np(y), cpu, R.layernorm(x, ga, be))


# ------------------------------------------------------------------------------------------------
# positions / length regulator
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 64, 65, 200])
def test_positions_both_probe_forms(T):
    """zeros on both sides of every 64-lane chunk border: the carry across chunks, per item. The float form reads column 0 of a [B,T,256] tensor
    (the other columns are non-zero where column 0 is zero, so that a wrong column or stride shows)."""
    B, ldp = 3, 256
    g = _rng(300 + T)
    nz = g.random((B, T)) < 0.75
    for b, border in enumerate([(63, 128), (64, 127), (63, 64, 127, 128)]):
        for t in border:
            if t < T:
                nz[b, t] = False
        nz[b, [t for t in (62, 65, 126, 129) if t < T]] = True
    ref = R.make_positions(nz).astype(np.int32)
    lib = L.load()
    tok = _d(np.where(nz, g.integers(1, 50, (B, T)), 0).astype(np.int64))
    pos = _sent(B, T, dtype=torch.int32, value=-7)
    L.check(lib.ss_make_positions(L.ptr(tok), None, 0, 0, L.ptr(pos), B, T, L.stream_ptr()), "ss_make_positions")
    assert np.array_equal(_np(pos), ref)
    probe = g.standard_normal((B, T, ldp)).astype(np.float32)
    probe[:, :, 0] = np.where(nz, probe[:, :, 0] + 3.0 * np.sign(probe[:, :, 0]), 0.0)
    probe[:, :, 1:][probe[:, :, 1:] == 0] = 1.0
    pd = _d(probe)
    pos = _sent(B, T, dtype=torch.int32, value=-7)
    L.check(lib.ss_make_positions(None, L.ptr(pd), ldp, T * ldp, L.ptr(pos), B, T, L.stream_ptr()), "ss_make_positions")
    assert np.array_equal(_np(pos), ref)


@pytest.mark.parametrize("Tp", R.LR_TPS)
def test_length_regulator_three_tmax_forms(Tp):
    """Tmax = 0 (durations + lens), Tmax = the longest item, Tmax = 5 short of it (truncation; nothing past B * Tmax is written). Bit-exact: no
    entry is within 0.25 of a rounding tie (asserted in float64 by the CPU test)."""
    B = R.LR_B
    logdur, tokens, _ = R.length_regulator_inputs(Tp)
    lib = L.load()
    ld, tk = _d(logdur), _d(tokens)
    dur_ref, _, tot = R.length_regulate(logdur, tokens, 0)
    dur = _sent(B, Tp, dtype=torch.int64, value=-7)
    lens = _sent(B, dtype=torch.int32, value=-7)
    L.check(lib.ss_length_regulate(L.ptr(ld), L.ptr(tk), L.ptr(dur), None, L.ptr(lens), B, Tp, 0, L.stream_ptr()), "ss_length_regulate")
    assert np.array_equal(_np(dur), dur_ref) and np.array_equal(_np(lens), tot)
    Tfull = int(tot.max())
    for Tmax in (Tfull, Tfull - 5):
        if Tmax <= 0:
            continue
        _, m_ref, l_ref = R.length_regulate(logdur, tokens, Tmax)
        dur = _sent(B, Tp, dtype=torch.int64, value=-7)
        lens = _sent(B, dtype=torch.int32, value=-7)
        m2p = _sent(B * Tmax + 64, dtype=torch.int64, value=-7)
        L.check(lib.ss_length_regulate(L.ptr(ld), L.ptr(tk), L.ptr(dur), L.ptr(m2p), L.ptr(lens), B, Tp, Tmax, L.stream_ptr()), "ss_length_regulate")
        m = _np(m2p)
        assert np.array_equal(m[:B * Tmax].reshape(B, Tmax), m_ref)
        assert np.all(m[B * Tmax:] == -7), "wrote past B * Tmax"
        assert np.array_equal(_np(dur), dur_ref) and np.array_equal(_np(lens), l_ref)


# ------------------------------------------------------------------------------------------------
# gathers and lookups
# ------------------------------------------------------------------------------------------------
def test_gather_expand_both_types():
    B, Tsrc, T, C = 2, 70, 300, 256
    g = _rng(400)
    m2p = g.integers(0, Tsrc + 1, (B, T)).astype(np.int64)
    m2p[0, :5] = [0, 1, Tsrc, Tsrc + 1, -3]
    m2p[1, -5:] = [-1, Tsrc + 1, Tsrc, 1, 0]
    src = _f32(g, B, Tsrc, C)
    src_i = g.integers(-2 ** 40, 2 ** 40, (B, Tsrc)).astype(np.int64)
    lib = L.load()
    md, sd, sid = _d(m2p), _d(src), _d(src_i)
    out = _sent(B, T, C)
    L.check(lib.ss_gather_expand(L.ptr(sd), L.ptr(md), L.ptr(out), B, Tsrc, T, C, L.stream_ptr()), "ss_gather_expand")
    assert np.array_equal(_np(out), R.gather_expand(src, m2p))
    out_i = _sent(B, T, dtype=torch.int64, value=-7)
    L.check(lib.ss_gather_expand_i64(L.ptr(sid), L.ptr(md), L.ptr(out_i), B, Tsrc, T, L.stream_ptr()), "ss_gather_expand_i64")
    assert np.array_equal(_np(out_i), R.gather_expand(src_i, m2p))


@pytest.mark.parametrize("accumulate", [0, 1])
def test_embedding_clamps_scale_accumulate(accumulate):
    """ids -1 and n clamp to the first / last row. scale * table is one fp32 rounding (bit-exact); with accumulate a second one: 1 ulp."""
    rows, C, n = 77, 256, 50
    g = _rng(410)
    ids = g.integers(0, n, rows).astype(np.int64)
    ids[:4] = [-1, 0, n - 1, n]
    ids[-2:] = [n + 7, -9]
    table, prev = _f32(g, n, C), _f32(g, rows, C)
    scale = math.sqrt(256)
    out = _d(prev) if accumulate else _sent(rows, C)
    idd, td = _d(ids), _d(table)
    L.check(L.load().ss_embedding(L.ptr(idd), L.ptr(td), L.ptr(out), rows, C, n, scale, accumulate, L.stream_ptr()), "ss_embedding")
    ref = R.embedding(ids, table, scale, prev if accumulate else None)
    if accumulate:
        _assert_ulps(_np(out), ref, R.embedding(ids, table, scale))
    else:
        assert np.array_equal(_np(out), ref.astype(np.float32))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("with_alpha_dev", [False, True])
def test_table_add_into_a_column_block(accumulate, with_alpha_dev):
    """the output is the right-hand H columns of a [B,T,2H] buffer (ldo = 2H): the left half keeps its sentinel. pos >= table_rows clamps to the last
    row. alpha = 0.5 * alpha_dev[0] = 0.375 exactly, so the product rounds once and the accumulate once: 1 ulp."""
    B, T, H, n = 2, 37, 256, 40
    g = _rng(420)
    pos = g.integers(0, n, (B, T)).astype(np.int32)
    pos[0, :3] = [0, n - 1, n]
    pos[1, -1] = n + 100
    table, prev = _f32(g, n, H), _f32(g, B, T, H)
    cat = _sent(B, T, 2 * H)
    if accumulate:
        cat[:, :, H:] = _d(prev)
    pd, td = _d(pos), _d(table)
    adev = _d(np.array([0.75], np.float32)) if with_alpha_dev else None
    alpha = 0.5
    L.check(L.load().ss_table_add(L.ptr(pd), L.ptr(td), n, L.ptr(cat) + 4 * H, 2 * H, T * 2 * H, B, T, H, L.ptr(adev), alpha, accumulate, L.stream_ptr()),
            "ss_table_add")
    a = 0.375 if with_alpha_dev else 0.5
    o = _np(cat)
    assert np.all(o[:, :, :H] == SENT), "the left column block was written"
    ref = R.table_add(pos, table, a, prev if accumulate else None)
    _assert_ulps(o[:, :, H:], ref, R.table_add(pos, table, a))
    if not accumulate:
        assert np.array_equal(o[:, :, H:], ref.astype(np.float32))   # one rounding: exact


@pytest.mark.parametrize("C", [80, 1])
def test_add_bcast_mask_every_presence_combination(C):
    """all 16 combinations of v1 / y1 / v2 / y2, each with lens and without: bit-equal to the fp32 sum in the documented order (no
    multiplication: nothing to contract). C = 1 is the waveform mask of the mel front end. Then all four in place."""
    B, T = 2, 37
    g = _rng(430 + C)
    x, y1, y2 = _f32(g, B, T, C), _f32(g, B, T, C, scale=100.0), _f32(g, B, T, C, scale=1e-3)
    v1, v2 = _f32(g, B, C, scale=10.0), _f32(g, B, C)
    lens = np.array([37, 20], np.int32)
    lib = L.load()
    dx, dv1, dy1, dv2, dy2, dl = _d(x), _d(v1), _d(y1), _d(v2), _d(y2), _d(lens)
    for mask in range(16):
        use = [bool(mask >> i & 1) for i in range(4)]
        for ln, ld in ((lens, dl), (None, None)):
            out = _sent(B, T, C)
            L.check(lib.ss_add_bcast_mask(L.ptr(dx), L.ptr(dv1) if use[0] else None, L.ptr(dy1) if use[1] else None, L.ptr(dv2) if use[2] else None,
                                          L.ptr(dy2) if use[3] else None, L.ptr(out), B, T, C, L.ptr(ld), L.stream_ptr()), "ss_add_bcast_mask")
            ref = R.add_bcast_mask(x, v1 if use[0] else None, y1 if use[1] else None, v2 if use[2] else None, y2 if use[3] else None, ln, dtype=np.float32)
            assert np.array_equal(_np(out), ref), (mask, ln is None)
    L.check(lib.ss_add_bcast_mask(L.ptr(dx), L.ptr(dv1), L.ptr(dy1), L.ptr(dv2), L.ptr(dy2), L.ptr(dx), B, T, C, L.ptr(dl), L.stream_ptr()), "in place")
    assert np.array_equal(_np(dx), R.add_bcast_mask(x, v1, y1, v2, y2, lens, dtype=np.float32))


def test_add_rowscalar_mask_rows_by_ref_note_dur_add():
    B, T, C = 2, 37, 80
    g = _rng(440)
    lib = L.load()
    x, s = _f32(g, B, T, C), _f32(g, B, T, scale=5.0)
    lens = np.array([37, 11], np.int32)
    sd = _d(s)
    for ln in (lens, None):
        xd, lnd = _d(x), None if ln is None else _d(ln)
        L.check(lib.ss_add_rowscalar(L.ptr(xd), L.ptr(sd), B, T, C, L.ptr(lnd), L.stream_ptr()), "ss_add_rowscalar")
        assert np.array_equal(_np(xd), R.add_rowscalar(x, s, ln).astype(np.float32))   # one fp32 add: exact; rows >= lens untouched
    # mask_rows_by_ref: the per-frame mask is column 0 of a [rows, ldref] tensor whose other columns are non-zero
    rows, ldref = B * T, 80
    ref_t = _f32(g, rows, ldref)
    ref_t[ref_t == 0] = 1.0
    zero_rows = [0, 5, 36, 37, rows - 1]
    ref_t[zero_rows, 0] = 0.0
    ref_t[6, 0] = -0.0
    xd, rd = _d(x), _d(ref_t)
    L.check(lib.ss_mask_rows_by_ref(L.ptr(xd), L.ptr(rd), ldref, rows, C, L.stream_ptr()), "ss_mask_rows_by_ref")
    assert np.array_equal(_np(xd).reshape(rows, C), R.mask_rows_by_ref(x.reshape(rows, C), ref_t[:, 0]))
    # note_dur_add: dur on a grid of quarters and w on a grid of 2^-10, so dur * w is exact in fp32 and two additions round: 1 ulp
    dur = (g.integers(0, 41, rows) / 4.0).astype(np.float32)
    w = (g.integers(-2048, 2049, C) / 1024.0).astype(np.float32)
    b = _f32(g, C)
    prev = x.reshape(rows, C)
    od, dd, wd, bd = _d(prev), _d(dur), _d(w), _d(b)
    L.check(lib.ss_note_dur_add(L.ptr(dd), L.ptr(wd), L.ptr(bd), L.ptr(od), rows, C, L.stream_ptr()), "ss_note_dur_add")
    mag = np.maximum(np.abs(dur[:, None].astype(np.float64) * w[None, :]) + np.abs(b)[None, :], np.abs(prev))
    _assert_ulps(_np(od), R.note_dur_add(prev, dur, w, b), mag)


@pytest.mark.parametrize("T", [1, 64, 65, 300])
def test_count_nonzero_and_ref_lens(T):
    B, C = 4, 80
    g = _rng(450 + T)
    lib = L.load()
    m2p = g.integers(-1, 3, (B, T)).astype(np.int64)   # negatives do not count
    m2p[1] = 0
    md = _d(m2p)
    lens = _sent(B, dtype=torch.int32, value=-7)
    L.check(lib.ss_count_nonzero_i64(L.ptr(md), L.ptr(lens), B, T, L.stream_ptr()), "ss_count_nonzero_i64")
    assert np.array_equal(_np(lens), R.count_positive(m2p))
    # ref_lens: interior zero frames (item 0), trailing zeros (item 1), an all-zero column 0 (item 2), a full item (item 3)
    mel = _f32(g, B, T, C)
    mel[mel == 0] = 1.0
    mel[0, ::3, 0] = 0.0
    if T > 2:
        mel[1, T - T // 3:, 0] = 0.0
        mel[1, T // 2, 0] = 0.0
    mel[2, :, 0] = 0.0
    want = R.ref_lens(mel)
    assert want[2] == 0 and want[3] == T and want[1] == T - T // 3 and want[0] == (T - 1 if (T - 1) % 3 == 0 else T)
    meld = _d(mel)
    lens = _sent(B, dtype=torch.int32, value=-7)
    L.check(lib.ss_ref_lens(L.ptr(meld), B, T, C, L.ptr(lens), L.stream_ptr()), "ss_ref_lens")
    assert np.array_equal(_np(lens), want)


# ------------------------------------------------------------------------------------------------
# the second trip of the grid-stride loops (grids are capped at 8192 blocks x 256 threads = 2 097 152 work items)
# ------------------------------------------------------------------------------------------------
GRID_CAP_ITEMS = 8192 * 256


def _tail_and_sample(a):
    a = a.reshape(-1)
    return np.concatenate([a[-4096:], a[::251]])


def test_grid_cap_add_bcast_mask():
    B, T, C = 2, 4100, 256
    assert B * T * C > GRID_CAP_ITEMS
    g = _rng(500)
    x, y1 = _f32(g, B, T, C), _f32(g, B, T, C)
    lens = np.array([T, T - 100], np.int32)
    dx, dy, dl = _d(x), _d(y1), _d(lens)
    out = _sent(B, T, C)
    L.check(L.load().ss_add_bcast_mask(L.ptr(dx), None, L.ptr(dy), None, None, L.ptr(out), B, T, C, L.ptr(dl), L.stream_ptr()), "ss_add_bcast_mask")
    ref = R.add_bcast_mask(x, y1=y1, lens=lens, dtype=np.float32)
    assert np.array_equal(_tail_and_sample(_np(out)), _tail_and_sample(ref))


def test_grid_cap_gather_table_add_embedding():
    """one float4 per work item: C = 1024 puts B * T * C / 4 just above the cap"""
    B, T, C, Tsrc, n = 2, 4100, 1024, 70, 90
    assert B * T * C // 4 > GRID_CAP_ITEMS
    g = _rng(510)
    lib = L.load()
    src = _f32(g, B, Tsrc, C)
    m2p = g.integers(0, Tsrc + 1, (B, T)).astype(np.int64)
    m2p[1, -4:] = [Tsrc, 1, Tsrc, 2]
    sd, md = _d(src), _d(m2p)
    out = _sent(B, T, C)
    L.check(lib.ss_gather_expand(L.ptr(sd), L.ptr(md), L.ptr(out), B, Tsrc, T, C, L.stream_ptr()), "ss_gather_expand")
    assert np.array_equal(_tail_and_sample(_np(out)), _tail_and_sample(R.gather_expand(src, m2p)))
    table = _f32(g, n, C)
    pos = g.integers(1, n, (B, T)).astype(np.int32)
    td, pd = _d(table), _d(pos)
    out.fill_(SENT)
    L.check(lib.ss_table_add(L.ptr(pd), L.ptr(td), n, L.ptr(out), C, T * C, B, T, C, None, 1.0, 0, L.stream_ptr()), "ss_table_add")
    assert np.array_equal(_tail_and_sample(_np(out)), _tail_and_sample(table[pos]))
    ids = g.integers(0, n, B * T).astype(np.int64)
    idd = _d(ids)
    out.fill_(SENT)
    L.check(lib.ss_embedding(L.ptr(idd), L.ptr(td), L.ptr(out), B * T, C, n, 1.0, 0, L.stream_ptr()), "ss_embedding")
    assert np.array_equal(_tail_and_sample(_np(out)), _tail_and_sample(table[ids]))


def test_grid_cap_spec_magnitude():
    rows, nbins, ldp, lds = 3856, 513, 544, 1088
    assert rows * ldp > GRID_CAP_ITEMS
    S = _f32(_rng(520), rows, lds)
    Sd = _d(S)
    P = _sent(rows, ldp)
    L.check(L.load().ss_spec_magnitude(L.ptr(Sd), L.ptr(P), rows, lds, ldp, nbins, ldp, L.stream_ptr()), "ss_spec_magnitude")
    St = torch.from_numpy(S)
    cpu = np.zeros((rows, ldp), np.float32)
    cpu[:, :nbins] = torch.sqrt(St[:, :nbins] * St[:, :nbins] + St[:, ldp:ldp + nbins] * St[:, ldp:ldp + nbins]).numpy()
    ref = R.spec_magnitude(S, nbins, ldp, ldp)
    o = _np(P)
    assert np.all(o[:, nbins:] == 0)
    _check_derived("spec_magnitude_grid_cap", _tail_and_sample(o), _tail_and_sample(cpu), _tail_and_sample(ref))


# ------------------------------------------------------------------------------------------------
# emotion encoder pieces
# ------------------------------------------------------------------------------------------------
def _lstm_cpu32(xproj, w_hh):
    xp, w = torch.from_numpy(xproj), torch.from_numpy(w_hh)
    P, n, H4 = xp.shape
    H = H4 // 4
    h, c = torch.zeros(P, H), torch.zeros(P, H)
    out = torch.zeros(P, n, H)
    for t in range(n):
        a = xp[:, t] + h @ w.t()
        i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
        c = f * c + i * g
        h = o * torch.tanh(c)
        out[:, t] = h
    return out.numpy()


@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("n", [1, 2, 7, 160])
def test_lstm_layer(P, n):
    """gate order i, f, g, o; h_seq only, h_last only and both give the same numbers; h_last is h_seq's last step bit for bit"""
    H = 256
    g = _rng(600 + n + P)
    w_hh = g.uniform(-1 / 16, 1 / 16, (4 * H, H)).astype(np.float32)
    xproj = _f32(g, P, n, 4 * H)
    xd = _d(R.interleave_gates(xproj))
    wd = pack_whh(_d(w_hh), H)
    lib = L.load()
    seq_a, seq_b = _sent(P, n, H), _sent(P, n, H)
    last_a, last_b = _sent(P, H), _sent(P, H)
    L.check(lib.ss_lstm_layer(L.ptr(xd), L.ptr(wd), L.ptr(seq_a), None, P, n, H, L.stream_ptr()), "ss_lstm_layer")
    L.check(lib.ss_lstm_layer(L.ptr(xd), L.ptr(wd), None, L.ptr(last_a), P, n, H, L.stream_ptr()), "ss_lstm_layer")
    L.check(lib.ss_lstm_layer(L.ptr(xd), L.ptr(wd), L.ptr(seq_b), L.ptr(last_b), P, n, H, L.stream_ptr()), "ss_lstm_layer")
    torch.cuda.synchronize()
    assert torch.equal(seq_a, seq_b) and torch.equal(last_a, last_b) and torch.equal(last_b, seq_b[:, -1])
    _check_derived(f"lstm_P{P}_n{n}", _np(seq_b), _lstm_cpu32(xproj, w_hh), R.lstm_layer(xproj, w_hh))


@pytest.mark.parametrize("rows", [1, 3, 40])
def test_mean_l2norm(rows):
    C = 256
    x = (_f32(_rng(620 + rows), rows, C) + 0.3).astype(np.float32)
    xd = _d(x)
    out = _sent(C)
    L.check(L.load().ss_mean_l2norm(L.ptr(xd), L.ptr(out), rows, C, L.stream_ptr()), "ss_mean_l2norm")
    m = torch.from_numpy(x).mean(0)
    _check_derived(f"mean_l2norm_rows{rows}", _np(out), (m / m.norm()).numpy(), R.mean_l2norm(x))


@pytest.mark.parametrize("rows,C", [(1, 256), (5, 256), (1, 100), (5, 100)])
def test_l2norm_rows(rows, C):
    x = _f32(_rng(630 + rows + C), rows, C)
    xd = _d(x)
    out = _sent(rows + 1, C)
    L.check(L.load().ss_l2norm_rows(L.ptr(xd), L.ptr(out), rows, C, L.stream_ptr()), "ss_l2norm_rows")
    o = _np(out)
    assert np.all(o[rows] == SENT)
    xt = torch.from_numpy(x)
    _check_derived(f"l2norm_rows{rows}_C{C}", o[:rows], (xt / xt.norm(dim=-1, keepdim=True)).numpy(), R.l2norm_rows(x))


# ------------------------------------------------------------------------------------------------
# pitch
# ------------------------------------------------------------------------------------------------
def test_f0_bounds_every_midi_note():
    n = 257
    midi = (np.arange(n) % 128).astype(np.int64)
    md = _d(midi)
    lo, hi = _sent(n + 3), _sent(n + 3)
    L.check(L.load().ss_f0_bounds(L.ptr(md), L.ptr(lo), L.ptr(hi), n, L.stream_ptr()), "ss_f0_bounds")
    lo, hi = _np(lo), _np(hi)
    assert np.all(lo[n:] == SENT) and np.all(hi[n:] == SENT)
    rlo, rhi = R.f0_bounds(midi)

    def cpu(note):
        x = torch.clamp(torch.log2(2 ** ((note - 69) / 12) * 440), max=10.0)
        return ((x - 6) / (10 - 6) * 2 - 1).clamp(-1, 1).numpy()
    m = torch.from_numpy(midi).float()
    _check_derived("f0_bounds_lo", lo[:n], cpu(m - 3), rlo)
    _check_derived("f0_bounds_hi", hi[:n], cpu(m + 3), rhi)
    assert np.all(lo[:n] >= -1) and np.all(hi[:n] <= 1)


def test_pitch_post():
    """pitch_pred / f0_denorm by the 4 x rule; the voicing column and the zeroed frames exactly; coarse bit-exact wherever the float64 bin coordinate is
    farther than 1e-3 from a bin boundary (<= 1 % of the frames are not, asserted on the float64 reference by the CPU test)."""
    n = R.PITCH_POST_N
    f0_a, uv_a, f0_b, uv_b, midi, mel2ph = R.pitch_post_inputs()
    dv = [_d(a) for a in (f0_a, uv_a, f0_b, uv_b, midi, mel2ph)]
    pp, hz, coarse = _sent(n + 1, 2), _sent(n + 1), _sent(n + 1, dtype=torch.int64, value=-7)
    L.check(L.load().ss_pitch_post(*[L.ptr(a) for a in dv], L.ptr(pp), L.ptr(hz), L.ptr(coarse), n, L.stream_ptr()), "ss_pitch_post")
    pp, hz, coarse = _np(pp), _np(hz), _np(coarse)
    assert np.all(pp[n] == SENT) and hz[n] == SENT and coarse[n] == -7
    rp, rhz, rc, coord = R.pitch_post(f0_a, uv_a, f0_b, uv_b, midi, mel2ph)
    t = torch.from_numpy
    rest = t(midi) == 0
    ua, ub = (t(uv_a) != 0).float().masked_fill(rest, 1.0), (t(uv_b) != 0).float().masked_fill(rest, 1.0)
    f32 = ((t(f0_b) + 1) / 2 * (10 - 6) + 6) / 2 + ((t(f0_a) + 1) / 2 * (10 - 6) + 6) / 2
    hz32 = (2 ** f32).masked_fill((ub / 2 + ua / 2) > 0, 0.0).masked_fill(t(mel2ph) == 0, 0.0)
    assert np.array_equal(pp[:n, 1], rp[:, 1].astype(np.float32))
    assert np.all(hz[:n][rhz == 0] == 0) and np.all(hz[:n][rhz > 0] > 0)
    _check_derived("pitch_post_pitch_pred", pp[:n, 0], f32.numpy(), rp[:, 0])
    _check_derived("pitch_post_f0_denorm", hz[:n], hz32.numpy(), rhz)
    keep = ~R.coarse_band(coord)
    assert keep.mean() >= 0.99
    assert np.array_equal(coarse[:n][keep], rc[keep])
    assert np.all(np.abs(coarse[:n] - rc) <= 1) and coarse[:n].min() == 1 and coarse[:n].max() == 255


# ------------------------------------------------------------------------------------------------
# front end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", [False, True])
def test_spec_magnitude_and_power(power):
    """the mel front end's layout: 513 bins in (re | im) blocks of 544 columns; the 31 padding columns of P are written as exact zeros"""
    rows, nbins, ldp, lds = 5, 513, 544, 1088
    S = _f32(_rng(700), rows, lds, scale=3.0)
    S[2] = 0.0
    S[:, nbins:ldp] = 99.0            # what sits between the two blocks is never read into a bin
    Sd = _d(S)
    P = _sent(rows + 1, ldp)
    fn = L.load().ss_spec_power if power else L.load().ss_spec_magnitude
    L.check(fn(L.ptr(Sd), L.ptr(P), rows, lds, ldp, nbins, ldp, L.stream_ptr()), "spec")
    o = _np(P)
    assert np.all(o[rows] == SENT) and np.all(o[:rows, nbins:] == 0) and np.all(o[2] == 0)
    St = torch.from_numpy(S)
    p32 = St[:, :nbins] * St[:, :nbins] + St[:, ldp:ldp + nbins] * St[:, ldp:ldp + nbins]
    cpu = np.zeros((rows, ldp), np.float32)
    cpu[:, :nbins] = (p32 if power else torch.sqrt(p32)).numpy()
    _check_derived("spec_power" if power else "spec_magnitude", o[:rows], cpu, R.spec_magnitude(S, nbins, ldp, ldp, power=power))


def test_reflect_pad_ragged_items():
    """pad = 512 against items longer than, one more than, equal to and much shorter than the pad (several reflections), a single sample and an
    empty item; Ly exceeds the longest padded item, the excess is zero."""
    pad, Lx = 512, 2000
    lens = np.array([2000, 513, 512, 100, 1, 0], np.int32)
    B, Ly = len(lens), 2000 + 2 * 512 + 40
    x = _f32(_rng(710), B, Lx)
    xd, ld = _d(x), _d(lens)
    y = _sent(B + 1, Ly)
    L.check(L.load().ss_reflect_pad(L.ptr(xd), L.ptr(ld), L.ptr(y), B, Lx, Ly, pad, L.stream_ptr()), "ss_reflect_pad")
    o = _np(y)
    assert np.all(o[B] == SENT)
    assert np.array_equal(o[:B], R.reflect_pad(x, lens, Ly, pad))


def test_log10_floor_clip_round_f16():
    lib = L.load()
    eps = np.float32(1e-10)
    g = _rng(720)
    x = np.concatenate([np.array([0.0, -1.0, 1e-12, np.nextafter(eps, np.float32(0)), eps, np.nextafter(eps, np.float32(1)), 1.0, 1e4], np.float32),
                        np.exp(g.uniform(-30, 10, 500)).astype(np.float32)])
    n = len(x)
    xd = _d(x)
    y = _sent(n + 1)
    L.check(lib.ss_log10_floor(L.ptr(xd), L.ptr(y), n, float(eps), L.stream_ptr()), "ss_log10_floor")
    o = _np(y)
    assert o[n] == SENT and np.all(o[:5] == o[4])             # everything at or below eps gives log10(eps)
    _check_derived("log10_floor", o[:n], torch.log10(torch.clamp(torch.from_numpy(x), min=float(eps))).numpy(), R.log10_floor(x, eps))
    # clip
    lo, hi = np.float32(-6.0), np.float32(1.5)
    c = np.concatenate([np.array([lo, hi, np.nextafter(lo, np.float32(-9)), np.nextafter(hi, np.float32(9)), 0.0, -100.0, 100.0], np.float32), _f32(g, 300, scale=4.0)])
    cd = _d(c)
    y = _sent(len(c) + 1)
    L.check(lib.ss_clip(L.ptr(cd), L.ptr(y), len(c), float(lo), float(hi), L.stream_ptr()), "ss_clip")
    assert np.array_equal(_np(y)[:-1], np.clip(c, lo, hi)) and _np(y)[-1] == SENT
    # round_f16_rows: n_out < n_in, n_in < n_out, n_out > Lx; ldy > Lx; fp16 ties (to even), the largest finite fp16 and what rounds past it
    B, Lx, ldx, ldy = 3, 50, 56, 64
    xr = np.full((B, ldx), 3.3, np.float32)
    xr[:, :Lx] = _f32(g, B, Lx, scale=2.0)
    xr[:, :8] = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 65504.0, 65519.0, 65520.0, -70000.0, 6e-8]
    n_in, n_out = np.array([50, 20, 40], np.int32), np.array([30, 45, 64], np.int32)
    xrd, nid, nod = _d(xr), _d(n_in), _d(n_out)
    y = _sent(B + 1, ldy)
    L.check(lib.ss_round_f16_rows(L.ptr(xrd), ldx, Lx, L.ptr(nid), L.ptr(nod), L.ptr(y), ldy, B, L.stream_ptr()), "ss_round_f16_rows")
    o = _np(y)
    want = R.round_f16_rows(xr[:, :Lx], n_in, n_out, ldy)
    assert np.all(o[B] == SENT) and np.array_equal(o[:B], want)
    assert want[0, 0] == 1.0 and want[0, 1] == 1 + 2.0 ** -9 and np.isinf(want[0, 5]) and want[0, 4] == 65504.0
    y = _sent(B, ldy)
    L.check(lib.ss_round_f16_rows(L.ptr(xrd), ldx, Lx, None, L.ptr(nod), L.ptr(y), ldy, B, L.stream_ptr()), "ss_round_f16_rows")
    assert np.array_equal(_np(y), R.round_f16_rows(xr[:, :Lx], None, n_out, ldy))


def test_normalize_volume():
    """a quiet item (gain > 1), a loud one (gain stays 1: bit-exact copy), an all-zero item, an item with lens = 0 and one with lens < L whose tail is
    louder than its head (the mean is taken over the item's own samples only)."""
    B, Ln = 5, 1000
    g = _rng(730)
    wav = np.zeros((B, Ln), np.float32)
    wav[0] = _f32(g, Ln, scale=1e-3)
    wav[1] = _f32(g, Ln, scale=0.3)
    wav[3] = _f32(g, Ln, scale=1e-3)
    wav[4, :300] = _f32(g, 300, scale=2e-3)
    wav[4, 300:] = _f32(g, 700, scale=0.5)
    lens = np.array([Ln, Ln, Ln, 0, 300], np.int32)
    wd, ld = _d(wav), _d(lens)
    out = _sent(B + 1, Ln)
    L.check(L.load().ss_normalize_volume(L.ptr(wd), L.ptr(ld), L.ptr(out), B, Ln, -30.0, L.stream_ptr()), "ss_normalize_volume")
    o = _np(out)
    gain = R.normalize_volume_gain(wav, lens, -30.0)
    assert gain[0] > 20 and gain[1] == 1 and gain[2] == 1 and gain[3] == 1 and gain[4] > 5
    assert np.all(o[B] == SENT) and np.array_equal(o[1], wav[1]) and np.all(o[2] == 0) and np.array_equal(o[3], wav[3])
    wt = torch.from_numpy(wav)
    cpu = wav.copy()
    for b in (0, 4):
        ms = (wt[b, :int(lens[b])] ** 2).mean()
        cpu[b] = (wt[b] * 10 ** ((-30.0 - 10 * torch.log10(ms)) / 20)).numpy()
    _check_derived("normalize_volume", o[:B], cpu, wav.astype(np.float64) * gain[:, None])
