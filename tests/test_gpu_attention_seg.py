"""GPU unit parity of `ss_attention_seg` (csrc/attention.hip, the SEG instantiation of the flash kernel) through the C-ABI against the float64
definition in tests/style_blend_refs.py (itself checked against stock torch multi-head attention by tests/test_style_blend_refs_cpu.py).

H = 2, D = 128, unit-normal inputs, scale = D ** -0.5; K and V are the two column blocks of ONE [B, R * Ts, 2 * H * D] buffer, the form
model.py::_align_style uses; the output buffer is filled with a sentinel before every call. Tq = 130 with qlens = (130, 97, 1): two query tiles, a
partial wave, a lone row. Tolerance: 1e-5, the bar test_gpu_small_kernels.py holds ss_attention to on this input distribution; the equalities
with ss_attention are bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import style_blend_refs as S  # noqa: E402
from conftest import record_measurement  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.model import resolve_ref_weights  # noqa: E402

H, D = 2, 128
HD = H * D
SENT = 7.0
B, TQ = 3, 130
QLENS = (130, 97, 1)
SCALE = D ** -0.5
TOL = 1e-5

# name -> (Ts, R, seg_lens [B][R], weights [R] or [B][R])
CASES = {
    "r1_ts32": (32, 1, [[32], [1], [0]], [1.0]),                                          # the last item has no key at all
    "r1_ts64": (64, 1, [[64], [33], [1]], [1.0]),
    "r2_empty_first_segment": (64, 2, [[0, 64], [33, 32], [1, 0]], [1.0, 1.0]),           # the first staged tile lies in segment 1
    "r3_zero_weight_middle": (64, 3, [[64, 33, 32], [1, 64, 33], [0, 0, 0]], [0.5, 0.0, 2.0]),   # + an item with every segment empty
    "r2_tiny_weight": (32, 2, [[32, 1], [1, 32], [0, 32]], [1.0, 1e-30]),
    "r3_ts32_per_item_weights": (32, 3, [[0, 0, 32], [32, 0, 1], [1, 1, 1]], [[1.0, 1.0, 1.0], [0.2, 5.0, 0.8], [0.0, 3.0, 1.0]]),
}


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of a case (host, float32) and its float64 reference: computed once, shared, never modified."""
    Ts, R, seg_lens, weights = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    q = torch.randn(B, TQ, HD, generator=g)
    kv = torch.randn(B, R * Ts, 2 * HD, generator=g)
    logw, _ = resolve_ref_weights(weights, B, R)
    ref, written = S.seg_attention(q.double(), kv[..., :HD].double(), kv[..., HD:].double(), H=H, D=D, scale=SCALE, R=R, Ts=Ts, seg_lens=seg_lens,
                                   seg_logw=logw, qlens=QLENS)
    return q, kv, np.asarray(seg_lens, np.int32), logw, ref.numpy(), written.numpy()


def _padded(kv, Ts, seg_lens, value):
    """kv with every row at or past its segment's length set to `value`"""
    out = kv.clone()
    for b in range(seg_lens.shape[0]):
        for r in range(seg_lens.shape[1]):
            out[b, r * Ts + int(seg_lens[b, r]):(r + 1) * Ts] = value
    return out


def _seg(q, kv, Ts, seg_lens, logw, qlens=QLENS):
    """ss_attention_seg on device copies of q [B, Tq, HD] and kv [B, R * Ts, 2 HD] -> the sentinel-filled output buffer [B, Tq, HD]"""
    qd, kvd = _d(q.numpy()), _d(kv.numpy())
    R = seg_lens.shape[1]
    out = torch.full((q.shape[0], q.shape[1], HD), SENT, device=dev())
    L.attention_seg(qd, kvd[:, :, :HD], kvd[:, :, HD:], out, B=q.shape[0], H=H, D=D, Tq=q.shape[1], R=R, Ts=Ts, ldq=HD, ldk=2 * HD, ldv=2 * HD,
                    ldo=HD, q_bs=q.shape[1] * HD, k_bs=R * Ts * 2 * HD, v_bs=R * Ts * 2 * HD, o_bs=q.shape[1] * HD,
                    qlens=None if qlens is None else _d(np.asarray(qlens, np.int32)), seg_lens=_d(seg_lens), seg_logw=_d(logw), scale=SCALE)
    torch.cuda.synchronize()
    return out


def _plain(q, kv, Tk, k_rows, klens, qlens=QLENS):
    """ss_attention on the first Tk key rows of every item of kv [B, k_rows, 2 HD]"""
    qd, kvd = _d(q.numpy()), _d(kv.numpy())
    out = torch.full((q.shape[0], q.shape[1], HD), SENT, device=dev())
    L.attention(qd, kvd[:, :, :HD], kvd[:, :, HD:], out, B=q.shape[0], H=H, D=D, Tq=q.shape[1], Tk=Tk, ldq=HD, ldk=2 * HD, ldv=2 * HD, ldo=HD,
                q_bs=q.shape[1] * HD, k_bs=k_rows * 2 * HD, v_bs=k_rows * 2 * HD, o_bs=q.shape[1] * HD, qlens=_d(np.asarray(qlens, np.int32)),
                klens=_d(np.asarray(klens, np.int32)), scale=SCALE)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_accuracy_sentinel_rows_and_padding(name):
    """Against the float64 definition: max |err| < 1e-5; rows >= qlen keep the sentinel; an item without a key is exactly 0; and the result is bit
    for bit the same whether the K/V rows past each segment's length hold zeros or NaN (they are never read)."""
    Ts, R = CASES[name][:2]
    q, kv, seg_lens, logw, ref, written = _case(name)
    out0 = _seg(q, _padded(kv, Ts, seg_lens, 0.0), Ts, seg_lens, logw)
    o = out0.cpu().numpy()
    assert np.all(o[~written] == SENT), "a row >= qlen was written"
    assert np.isfinite(o[written]).all()
    err = float(np.abs(o[written].astype(np.float64) - ref[written]).max())
    record_measurement("attention_seg_" + name, kernel_err=err, bound=TOL, ratio=err / TOL, Ts=Ts, R=R)
    print(f"[attention_seg {name}] max |err| {err:.3e}")
    assert err < TOL, err
    live = (seg_lens > 0) & np.isfinite(logw)
    for b in np.nonzero(~live.any(axis=1))[0]:
        assert np.all(o[b, :QLENS[b]] == 0.0), f"item {b} has no key: exact zeros"
    out_nan = _seg(q, _padded(kv, Ts, seg_lens, float("nan")), Ts, seg_lens, logw)
    assert torch.equal(out0, out_nan), "rows past a segment's length were read"


def test_an_item_without_keys_is_covered():
    assert any(not ((np.asarray(c[2]) > 0) & np.isfinite(resolve_ref_weights(c[3], B, c[1])[0])).any(axis=1).all() for c in CASES.values())


@pytest.mark.parametrize("name", ["r1_ts32", "r1_ts64"])
def test_one_segment_with_weight_one_is_ss_attention_bit_for_bit(name):
    Ts = CASES[name][0]
    q, kv, seg_lens, logw, _, _ = _case(name)
    assert (logw == 0.0).all()
    assert torch.equal(_seg(q, kv, Ts, seg_lens, logw), _plain(q, kv, Ts, Ts, seg_lens[:, 0]))


@pytest.mark.parametrize("Ts", [32, 64])
def test_weights_one_zero_are_ss_attention_on_the_first_segment_bit_for_bit(Ts):
    g = torch.Generator().manual_seed(77 + Ts)
    q, kv = torch.randn(B, TQ, HD, generator=g), torch.randn(B, 2 * Ts, 2 * HD, generator=g)
    seg_lens = np.asarray([[Ts, Ts], [Ts - 31, 1], [1, Ts]], np.int32)
    logw, _ = resolve_ref_weights([1.0, 0.0], B, 2)
    assert (logw[:, 0] == 0.0).all() and np.isneginf(logw[:, 1]).all()
    got = _seg(q, _padded(kv, Ts, np.asarray([[Ts, 0]] * B), float("nan")), Ts, seg_lens, logw)      # segment 1 is never read either
    assert torch.equal(got, _plain(q, kv, Ts, 2 * Ts, seg_lens[:, 0]))


@pytest.mark.parametrize("Ts", [32, 64])
def test_the_same_clip_in_both_segments_is_that_clip_once(Ts):
    """w = (0.3, 0.7) on two copies of one clip is mathematically the single clip's distribution: within the same 1e-5 of it."""
    g = torch.Generator().manual_seed(91 + Ts)
    q, clip = torch.randn(B, TQ, HD, generator=g), torch.randn(B, Ts, 2 * HD, generator=g)
    n = np.asarray([[Ts], [Ts - 31], [1]], np.int32)
    logw2, _ = resolve_ref_weights([0.3, 0.7], B, 2)
    two = _seg(q, torch.cat([clip, clip], 1), Ts, np.concatenate([n, n], 1), logw2)
    one = _seg(q, clip, Ts, n, resolve_ref_weights([1.0], B, 1)[0])
    ref, written = S.seg_attention(q.double(), clip[..., :HD].double(), clip[..., HD:].double(), H=H, D=D, scale=SCALE, R=1, Ts=Ts, seg_lens=n,
                                   seg_logw=np.zeros((B, 1)), qlens=QLENS)
    w = written.numpy()
    d = float((two - one).abs().cpu().numpy()[w].max())
    e = float(np.abs(two.cpu().numpy()[w].astype(np.float64) - ref.numpy()[w]).max())
    record_measurement(f"attention_seg_same_clip_twice_ts{Ts}", vs_single_segment=d, vs_float64=e, bound=TOL)
    assert d < TOL and e < TOL, (d, e)
    assert torch.equal(two.cpu()[~written], one.cpu()[~written])


def _raw(R, Ts, seg_lens_ptr, logw_ptr, out, q, kv):
    lib = L.load()
    rc = lib.ss_attention_seg(L.ptr(q), L.ptr(kv), L.ptr(kv) + 4 * HD, L.ptr(out), B, H, D, TQ, R, Ts, HD, 2 * HD, 2 * HD, HD, TQ * HD, 64 * 2 * HD,
                              64 * 2 * HD, TQ * HD, None, seg_lens_ptr, logw_ptr, SCALE, L.stream_ptr())
    torch.cuda.synchronize()
    return rc, lib.ss_last_error().decode()


def test_refusals_launch_nothing():
    q, kv = torch.randn(B, TQ, HD, device=dev()), torch.randn(B, 64, 2 * HD, device=dev())
    out = torch.full((B, TQ, HD), SENT, device=dev())
    sl, lw = torch.full((B, 2), 16, dtype=torch.int32, device=dev()), torch.zeros(B, 2, device=dev())
    for what, args in (("Ts", (1, 48, L.ptr(sl), L.ptr(lw))), ("Ts", (1, 0, L.ptr(sl), L.ptr(lw))), ("R = 0", (0, 32, L.ptr(sl), L.ptr(lw))),
                       ("seg_lens", (2, 32, None, L.ptr(lw))), ("seg_logw", (2, 32, L.ptr(sl), None))):
        rc, msg = _raw(*args, out, q, kv)
        assert rc < 0 and "ss_attention_seg" in msg and what in msg, (what, rc, msg)
        assert (out == SENT).all(), what
    lib = L.load()
    rc = lib.ss_attention_seg(L.ptr(q), L.ptr(kv), L.ptr(kv) + 4 * HD, L.ptr(out), B, H, 64, TQ, 2, 32, HD, 2 * HD, 2 * HD, HD, TQ * HD, 64 * 2 * HD,
                              64 * 2 * HD, TQ * HD, None, L.ptr(sl), L.ptr(lw), SCALE, L.stream_ptr())
    assert rc < 0 and "head dim" in lib.ss_last_error().decode()
    rc = lib.ss_attention_seg(L.ptr(q), L.ptr(kv), L.ptr(kv) + 4 * HD, L.ptr(out), B, H, D, TQ, 2, 32, HD, 2 * HD + 2, 2 * HD, HD, TQ * HD,
                              64 * 2 * HD, 64 * 2 * HD, TQ * HD, None, L.ptr(sl), L.ptr(lw), SCALE, L.stream_ptr())
    assert rc < 0 and "strides" in lib.ss_last_error().decode()
    torch.cuda.synchronize()
    assert (out == SENT).all()
    rc, _ = _raw(2, 32, L.ptr(sl), L.ptr(lw), out, q, kv)      # the same call with nothing wrong runs
    assert rc == 0 and not (out == SENT).any() and math.isfinite(out.sum().item())
