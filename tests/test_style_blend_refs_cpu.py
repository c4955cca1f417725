"""CPU checks of the reference blend (no GPU): the float64 definition of the segmented attention against stock torch multi-head attention, the host
normalisation of the weights (`model.resolve_ref_weights`), the embedding blend (`model.blend_embeds`) and the host-side refusals of the entry
points."""
import math

import numpy as np
import pytest
import torch

import style_blend_refs as S
from stylesinger_amd.model import StyleSingerHIP, blend_embeds, resolve_ref_weights

H, D = 2, 128


@pytest.mark.parametrize("R,Ts,seg_lens,weights", [
    (1, 32, [[32], [7]], [[1.0], [1.0]]),
    (2, 32, [[32, 5], [0, 17]], [[0.7, 0.3], [1.0, 1.0]]),
    (3, 64, [[64, 33, 1], [40, 64, 9]], [[0.5, 0.0, 2.0], [1.0, 1e-30, 3.0]]),
])
def test_definition_equals_stock_multi_head_attention_in_float64(R, Ts, seg_lens, weights):
    g = torch.Generator().manual_seed(7 + R)
    B, Tq = 2, 11
    q, k, v = (torch.randn(B, n, H * D, generator=g, dtype=torch.float64) for n in (Tq, R * Ts, R * Ts))
    logw, _ = resolve_ref_weights(weights, B, R)
    k_nan, v_nan = k.clone(), v.clone()   # the definition never reads a row outside the segments' lengths, nor one of a zero-weight segment
    valid, _ = S.key_layout(R, Ts, seg_lens, logw)
    k_nan[~valid], v_nan[~valid] = float("nan"), float("nan")
    got, written = S.seg_attention(k=k_nan, v=v_nan, q=q, H=H, D=D, scale=D ** -0.5, R=R, Ts=Ts, seg_lens=seg_lens, seg_logw=logw)
    want = S.stock_mha(q, k, v, H=H, D=D, R=R, Ts=Ts, seg_lens=seg_lens, seg_logw=logw)
    assert written.all() and torch.isfinite(got).all()
    assert (got - want).abs().max().item() <= 1e-12


def test_definition_edges():
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, n, H * D, generator=g, dtype=torch.float64) for n in (5, 64, 64))
    kw = dict(H=H, D=D, scale=D ** -0.5, R=2, Ts=32)
    # no key at all: zeros; rows past qlens are reported as not written
    out, written = S.seg_attention(q, k, v, seg_lens=[[0, 0], [3, 0]], seg_logw=[[0.0, 0.0], [-math.inf, 0.0]], qlens=[5, 2], **kw)
    assert (out == 0).all() and written.tolist() == [[True] * 5, [True, True, False, False, False]]
    # equal weights = the clips concatenated; (1, 0) = the first clip alone; the same clip twice with any weights = that clip once
    cat, _ = S.seg_attention(q, k, v, seg_lens=[[32, 32]] * 2, seg_logw=[[math.log(0.5)] * 2] * 2, **kw)
    one, _ = S.seg_attention(q, k, v, seg_lens=[[64]] * 2, seg_logw=[[0.0]] * 2, H=H, D=D, scale=D ** -0.5, R=1, Ts=64)
    assert (cat - one).abs().max().item() <= 1e-12
    first, _ = S.seg_attention(q, k, v, seg_lens=[[20, 32]] * 2, seg_logw=resolve_ref_weights([1, 0], 2, 2)[0], **kw)
    alone, _ = S.seg_attention(q, k[:, :32], v[:, :32], seg_lens=[[20]] * 2, seg_logw=[[0.0]] * 2, H=H, D=D, scale=D ** -0.5, R=1, Ts=32)
    assert torch.equal(first, alone)
    kk, vv = torch.cat([k[:, :32]] * 2, 1), torch.cat([v[:, :32]] * 2, 1)
    twice, _ = S.seg_attention(q, kk, vv, seg_lens=[[20, 20]] * 2, seg_logw=resolve_ref_weights([0.3, 0.7], 2, 2)[0], **kw)
    assert (twice - alone).abs().max().item() <= 1e-12


def test_resolve_ref_weights():
    logw, p = resolve_ref_weights([1.0], 1, 1)
    assert logw.dtype == np.float32 and logw.shape == (1, 1) and logw[0, 0] == 0.0 and not np.signbit(logw[0, 0]) and p[0, 0] == 1.0
    assert resolve_ref_weights([123.5], 3, 1)[0].tolist() == [[0.0]] * 3
    logw, p = resolve_ref_weights(None, 2, 4)
    assert p.tolist() == [[0.25] * 4] * 2 and np.array_equal(logw, np.full((2, 4), np.log(0.25), np.float32))
    logw, p = resolve_ref_weights([2.0, 0.0, 6.0], 2, 3)          # a length-R sequence serves every item
    assert logw.shape == (2, 3) and np.isneginf(logw[:, 1]).all() and p[0].tolist() == [0.25, 0.0, 0.75]
    assert np.array_equal(logw[:, [0, 2]], np.log(np.array([[0.25, 0.75]] * 2)).astype(np.float32))
    # scale invariance: only the ratios count (a power of two scales exactly; any other factor to the rounding of the float64 quotient)
    a = resolve_ref_weights([[0.3, 0.7], [5.0, 1.0]], 2, 2)
    b = resolve_ref_weights([[0.3 * 1024, 0.7 * 1024], [5.0 / 64, 1.0 / 64]], 2, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = resolve_ref_weights([[0.3 * 17.3, 0.7 * 17.3], [5.0e-20, 1.0e-20]], 2, 2)
    assert np.abs(c[1] - a[1]).max() <= 4 * np.finfo(np.float64).eps and np.abs(c[0] - a[0]).max() <= 2 * np.spacing(np.float32(np.abs(a[0]).max()))
    logw, p = resolve_ref_weights([1.0, 1e-30], 1, 2)
    assert np.isfinite(logw).all() and logw[0, 0] == 0.0 and abs(logw[0, 1] - math.log(1e-30)) < 1e-5
    assert resolve_ref_weights(torch.tensor([[1.0, 3.0]]), 1, 2)[1].tolist() == [[0.25, 0.75]]
    for bad, match in (([1.0, -0.5], ">= 0"), ([1.0, float("nan")], "finite"), ([float("inf"), 1.0], "finite"), ([0.0, 0.0], "all be zero"),
                       ([[1.0, 1.0], [0.0, 0.0]], "all be zero"), ([1.0, 2.0, 3.0], "shape"), ([[1.0, 2.0]] * 3, "shape"), (1.0, "shape"),
                       ([1e308, 1e308], "normalise")):
        with pytest.raises(ValueError, match=match):
            resolve_ref_weights(bad, 2, 2)
    with pytest.raises(ValueError, match="at least one"):
        resolve_ref_weights(None, 1, 0)


def test_blend_embeds():
    g = torch.Generator().manual_seed(5)
    e = torch.nn.functional.normalize(torch.randn(3, 4, 256, generator=g), dim=-1)
    _, p = resolve_ref_weights([[1, 2, 3, 4], [1, 0, 0, 0], [0.5, 0.5, 0, 0]], 3, 4)
    out = blend_embeds(e, p)
    assert out.shape == (3, 256) and out.dtype == torch.float32
    assert (out.norm(dim=1) - 1.0).abs().max().item() <= 2e-7 * 4
    want = (e.double() * torch.from_numpy(p)[:, :, None]).sum(1)
    want = want / want.norm(dim=1, keepdim=True)
    assert (out.double() - want).abs().max().item() <= 1e-6
    # R = 1 is the identity up to the division by the embedding's own norm (1 to fp32 rounding)
    one = blend_embeds(e[:, :1], resolve_ref_weights([1.0], 3, 1)[1])
    assert torch.equal(one, e[:, 0] / e[:, 0].norm(dim=1, keepdim=True).clamp_min(1e-12)) and (one - e[:, 0]).abs().max().item() <= 2e-7
    # opposite embeddings cancel: the guard divides by 1e-12 instead of 0 and the result is finite (zero)
    z = blend_embeds(torch.stack([e[0, 0], -e[0, 0]])[None], [[0.5, 0.5]])
    assert torch.isfinite(z).all() and (z == 0).all()
    with pytest.raises(ValueError, match="blend_embeds"):
        blend_embeds(e, p[:, :3])


def test_forward_refuses_bad_pools_before_the_device():
    """The checks of forward(ref_weights=) and encode_style_blend run before anything is packed or launched (no GPU here)."""
    m = StyleSingerHIP(None)
    txt = torch.zeros(1, 4, dtype=torch.long)
    mel4, f03 = torch.zeros(1, 2, 8, 80), torch.zeros(1, 2, 8)
    with pytest.raises(ValueError, match="ref_f0 must then be"):
        m.forward(txt, ref_mels=mel4, ref_f0=f03[:, 0], infer=True)
    with pytest.raises(ValueError, match="pool of references"):
        m.forward(txt, ref_mels=mel4[:, 0], ref_f0=f03[:, 0], infer=True, ref_weights=[1, 1])
    with pytest.raises(ValueError, match=">= 0"):
        m.forward(txt, ref_mels=mel4, ref_f0=f03, infer=True, ref_weights=[1, -1])
    with pytest.raises(ValueError, match="shape"):
        m.forward(txt, ref_mels=mel4, ref_f0=f03, infer=True, ref_weights=[1, 1, 1])
    with pytest.raises(ValueError, match="style_cache"):
        m.forward(txt, ref_mels=mel4, ref_f0=f03, infer=True, ref_weights=[1, 1], style_cache={})
    with pytest.raises(ValueError, match="encode_style_blend"):
        m.encode_style_blend(mel4[:, 0], f03[:, 0])
    with pytest.raises(ValueError, match="all be zero"):
        m.encode_style_blend(mel4, f03, [0, 0])


def test_entry_points_refuse_bad_reference_lists_on_the_host():
    from stylesinger_amd.infer import StyleSingerInfer
    ins = StyleSingerInfer.__new__(StyleSingerInfer)     # the producers' host checks need no device
    ins.hparams = dict(audio_sample_rate=48000, hop_size=256)
    wav = np.zeros(4800, np.float32)
    with pytest.raises(ValueError, match="infer_once"):
        ins.preprocess_input(dict(ref_audios=[wav, wav]))
    with pytest.raises(ValueError, match="not both"):
        ins._device_batch(dict(ref_audio=wav, ref_audios=[wav]))
    with pytest.raises(ValueError, match="non-empty list"):
        ins._device_batch(dict(ref_audios=[]))
    with pytest.raises(ValueError, match="ref_srs"):
        ins._device_batch(dict(ref_audios=[wav, wav], ref_srs=[48000]))
    with pytest.raises(ValueError, match=">= 0"):
        ins._device_batch(dict(ref_audios=[wav, wav], ref_weights=[1, -2]))
    with pytest.raises(ValueError, match="shape"):
        ins._device_batch(dict(ref_audios=[wav, wav], ref_weights=[1, 2, 3]))
    with pytest.raises(ValueError, match="belong to inp\\['ref_audios'\\]"):
        ins._device_batch(dict(ref_audio=wav, ref_weights=[1]))


def test_cli_reference_blend_flags():
    from stylesinger_amd import infer
    base = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "p"]
    for extra in (["--ref-weight", "2"], ["--ref-blend", "b.wav", "-1"], ["--ref-blend", "b.wav", "0", "--ref-weight", "0"], ["--ref-blend", "b.wav", "abc"]):
        with pytest.raises(SystemExit):
            infer.main(base + extra)
