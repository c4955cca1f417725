"""The FFT decoder blocks (model.py::_fft_blocks) with their first FFN conv (k = 9, 256 -> 1024, GELU) as grouped Winograd F(4,3)
(ss_wino43_conv, what the decoder runs in fp32 mode) and in direct form, on synthetic weights at B = 2, T = 300, ragged lens.

Both forms are held against the float64 restatement of the blocks (oracle.restatement.fft_blocks) within 4 x the larger error the fp32 CPU
restatement has against it on the same input - in its plain form and with the k = 9 convs routed through the CPU emulation of the grouped
F(4,3) arithmetic (oracle.wino_vocoder_numerics.conv1d_wino43) - and at least 2 fp32 ulp at the output's scale.

The reference is taken per item, on the item's own frames (as tests/vocoder_shape_cases.py does for the vocoder): the device reads every row
behind lens[b] as 0 in the FFN conv, which is what the blocks compute for that utterance alone. (Run on the PADDED batch, the restatement -
like the reference - lets the conv see layer_norm2's bias on the padding rows of a shorter item, and differs from the per-item result by
2.7e-2 on the item's last four frames at these weights; that is a property of the decoder's padding rule in both launch forms, not of the
kernel under test.)"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from conftest import record_measurement  # noqa: E402
from oracle import restatement as R  # noqa: E402
from oracle.wino_vocoder_numerics import conv1d_wino43  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd.model import StyleSingerHIP  # noqa: E402

DEV = "cuda:0"
B, T, LENS = 2, 300, (300, 141)


class _WinoFFN:
    """F.conv1d calls with a 9-tap weight and 'same' padding go through conv1d_wino43 (the FFN convs of the blocks; nothing else there has 9 taps)."""
    def __enter__(self):
        self.orig = orig = F.conv1d

        def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
            if w.shape[-1] == 9 and stride == 1 and groups == 1 and dilation == 1 and padding == 4:
                return conv1d_wino43(x, w, b, 1)
            return orig(x, w, b, stride, padding, dilation, groups)
        F.conv1d = conv1d
        return self

    def __exit__(self, *exc):
        F.conv1d = self.orig


def _hp():
    return config.make_hparams(dict(timesteps=2, K_step=2, f0_timesteps=2))


@functools.lru_cache(maxsize=None)
def _case():
    hp = _hp()
    sd = synth.synth_acoustic_state_dict(hp, 909)
    g = torch.Generator().manual_seed(910)
    x = torch.randn(B, T, hp["hidden_size"], generator=g)
    for b, n in enumerate(LENS):
        x[b, n:] = 0
    nl, nh = hp["dec_layers"], hp["num_heads"]
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("decoder.")}
    ref64 = torch.zeros(B, T, hp["hidden_size"], dtype=torch.float64)
    e_direct = e_wino = 0.0
    with torch.no_grad():
        for b, n in enumerate(LENS):
            xi, pad = x[b:b + 1, :n], torch.zeros(1, n, dtype=torch.bool)
            r = R.fft_blocks(sd64, "decoder", xi.double(), pad, nl, nh, False)
            ref64[b, :n] = r[0]
            e_direct = max(e_direct, (R.fft_blocks(sd, "decoder", xi, pad, nl, nh, False).double() - r).abs().max().item())
            with _WinoFFN():
                e_wino = max(e_wino, (R.fft_blocks(sd, "decoder", xi, pad, nl, nh, False).double() - r).abs().max().item())
    floor = 2.0 * 2.0 ** -23 * ref64.abs().max().item()
    return hp, sd, x, ref64, e_direct, e_wino, max(4.0 * max(e_direct, e_wino), floor)


@functools.lru_cache(maxsize=None)
def _model():
    hp, sd = _case()[:2]
    m = StyleSingerHIP(None, hparams=hp)
    m.load_state_dict(sd)
    m.eval().to(DEV)
    m._ensure_packed()
    return m


@pytest.mark.parametrize("form", ["wino", "direct"])
def test_decoder_blocks_match_float64_in_both_ffn_forms(form):
    hp, sd, x, ref64, e_direct, e_wino, bound = _case()
    m = _model()
    assert m.use_wino and all(ly["ffn1"].W43 is not None for ly in m._pk["dec"]["layers"]), "fp32 mode packs the Winograd copy of ffn1"
    assert all(ly["ffn1"].W43 is None for ly in m._pk["enc"]["layers"]), "the phoneme-level encoder keeps the direct kernel"
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        got = m._fft_blocks(m._pk["dec"], x.to(DEV).clone(), B, T, lens, ffn_wino=(form == "wino"))
    torch.cuda.synchronize()
    err = (got.cpu().double() - ref64).abs().max().item()
    print(f"decoder blocks, ffn1 {form}: err {err:.3e} vs float64 (CPU fp32: direct {e_direct:.3e}, F(4,3) {e_wino:.3e}), bound {bound:.3e}")
    record_measurement(f"decoder_ffn_{form}", err=err, cpu_direct=e_direct, cpu_wino=e_wino, bound=bound)
    for b, n in enumerate(LENS):
        assert bool((got[b, n:] == 0).all())
    assert err <= bound, (form, err, bound)


def test_the_two_ffn_forms_are_different_launches():
    """The Winograd and the direct launch round differently: equal outputs would mean the switch did nothing."""
    hp, sd, x = _case()[:3]
    m = _model()
    lens = torch.tensor(LENS, dtype=torch.int32, device=DEV)
    outs = []
    for wino in (True, False):
        with torch.no_grad():
            outs.append(m._fft_blocks(m._pk["dec"], x.to(DEV).clone(), B, T, lens, ffn_wino=wino).clone())
    assert not torch.equal(outs[0], outs[1])
