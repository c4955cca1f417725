"""The vocoder at every generator shape the checkpoint loader accepts (cases: tests/vocoder_shape_cases.py).

Every other GPU test of the vocoder runs DEFAULT_VOCODER. The hand-written kernels of hifigan.hip (noise_conv_kernel, conv_post_kernel,
stage_lens_kernel, the four-kernel phase scan) index by the hop, the stage widths, the upsampling rates and the ResBlock set, and are reached
only through ss_hifigan_forward / ss_hifigan_source - which these tests call directly, so that they own the buffers (sentinel tails).
`wav` is judged against the float64 generator on the fp32 harmonic source, within 4 x the error the fp32 CPU restatement itself has against
that reference on the very same case (the larger of its direct and its grouped-F(4,3) form); `har` against the project's 2e-6 / 2e-5 bars."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vocoder_shape_cases as V  # noqa: E402
from conftest import record_measurement  # noqa: E402
from oracle import philox as P  # noqa: E402
from stylesinger_amd import lib as L  # noqa: E402
from stylesinger_amd.vocoder import HifiGanGeneratorHIP  # noqa: E402

DEV = "cuda:0"
TAIL = 1024                  # sentinel elements behind every buffer the library writes
SENT = -77.25


def _packed(name, monkeypatch, wino):
    """A fresh generator of case `name`, packed with the grouped Winograd ResBlock convs (default) or the direct form (SS_VOC_WINO=0)."""
    if wino:
        monkeypatch.delenv("SS_VOC_WINO", raising=False)
    else:
        monkeypatch.setenv("SS_VOC_WINO", "0")
    monkeypatch.delenv("SS_PRECISION", raising=False)
    cfg, vsd = V.generator(name)
    gen = HifiGanGeneratorHIP(cfg)
    gen.load_state_dict(vsd, strict=True)
    gen.eval().to(DEV)
    gen.pack()
    assert gen._pk["hg"].wino == (1 if wino else 0)
    return gen


def _buf(n):
    return torch.full((n + TAIL,), SENT, device=DEV, dtype=torch.float32)


def _workspace(gen, B, T):
    nbytes = L.load().ss_hifigan_workspace_bytes(ctypes.addressof(gen._pk["hg"]), B, T)
    assert nbytes > 0
    return torch.full((nbytes + TAIL,), 0xA5, device=DEV, dtype=torch.uint8), nbytes


def _tails_untouched(ws, nbytes, *bufs):
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace was written past ss_hifigan_workspace_bytes"
    for b in bufs:
        assert bool((b[-TAIL:] == SENT).all()), "an output buffer was written past its end"


def _forward(gen, mel, f0, lens, noise):
    """ss_hifigan_forward on buffers of this test: wav [B, T*hop], har [B, T*hop] (cpu), sentinel tails checked."""
    lib = L.load()
    hg = gen._pk["hg"]
    B, T, _ = mel.shape
    n = B * T * gen.hop
    wav, har = _buf(n), _buf(n)
    ws, nbytes = _workspace(gen, B, T)
    mel_d, f0_d = mel.to(DEV).contiguous(), f0.to(DEV).contiguous()
    lens_d = torch.tensor(lens, dtype=torch.int32, device=DEV)
    ri, sn = noise["rand_ini"].to(DEV).contiguous(), noise["sine_noise"].to(DEV).contiguous()
    L.check(lib.ss_hifigan_forward(ctypes.addressof(hg), L.ptr(mel_d), L.ptr(f0_d), L.ptr(lens_d), B, T, L.ptr(ri), L.ptr(sn), 0,
                                   L.ptr(wav), L.ptr(har), L.ptr(ws), nbytes, L.stream_ptr()), "ss_hifigan_forward")
    torch.cuda.synchronize()
    _tails_untouched(ws, nbytes, wav, har)
    return wav[:n].view(B, -1).cpu(), har[:n].view(B, -1).cpu()


def _source(gen, f0, noise, seed=0):
    """ss_hifigan_source alone -> har [B, T*hop] (cpu). noise = None: the device draws (Philox, key = seed)."""
    lib = L.load()
    B, T = f0.shape
    n = B * T * gen.hop
    har = _buf(n)
    ws, nbytes = _workspace(gen, B, T)
    f0_d = f0.to(DEV).contiguous()
    ri = sn = None
    if noise is not None:
        ri, sn = noise["rand_ini"].to(DEV).float().contiguous(), noise["sine_noise"].to(DEV).float().contiguous()
    L.check(lib.ss_hifigan_source(ctypes.addressof(gen._pk["hg"]), L.ptr(f0_d), B, T, L.ptr(ri), L.ptr(sn), seed, L.ptr(har), L.ptr(ws), nbytes,
                                  L.stream_ptr()), "ss_hifigan_source")
    torch.cuda.synchronize()
    _tails_untouched(ws, nbytes, har)
    return har[:n].view(B, -1).cpu()


def _wino_switches(cfg):
    """True when some ResBlock conv of some stage qualifies for the grouped Winograd kernel: SS_VOC_WINO then changes the arithmetic."""
    lib = L.load()
    for i in range(len(cfg["upsample_rates"])):
        c = cfg["upsample_initial_channel"] >> (i + 1)
        for k, ds in zip(cfg["resblock_kernel_sizes"], cfg["resblock_dilation_sizes"]):
            if any(lib.ss_wino43_conv_ok(c, k, d) for d in list(ds) + [1]):
                return True
    return False


@pytest.mark.parametrize("batch", list(V.BATCHES))
@pytest.mark.parametrize("name", list(V.GENERATOR_CASES))
def test_generator_matches_float64_at_this_shape(name, batch, monkeypatch):
    """Both conv forms of one generator case on one batch. Measured on an MI355X (wav error / CPU yardstick, har error): DESIGN.md §4,
    'The vocoder at other generator shapes'."""
    cfg, _ = V.generator(name)
    hop = V.hop_of(cfg)
    B, T, lens = V.BATCHES[batch]
    mel, f0, noise = V.generator_inputs(name, batch)
    ref = V.generator_reference(name, batch)
    wavs = {}
    for form, wino in (("wino", True), ("direct", False)):
        wav, har = _forward(_packed(name, monkeypatch, wino), mel, f0, lens, noise)
        wavs[form] = wav
        e_w = e_h = ratio = 0.0
        for b, r in enumerate(ref):
            n = r["n"] * hop
            assert bool((wav[b, n:] == 0).all()), f"{name} {form}: wav of item {b} is not exactly 0 behind its {r['n']} frames"
            eh = (har[b, :n] - r["har"]).abs().max().item()
            ew = (wav[b, :n].double() - r["wav64"]).abs().max().item()
            print(f"{name} {batch} {form} item {b} (T={r['n']}): har err {eh:.3e}; wav err {ew:.3e}, CPU fp32 yardstick {r['yardstick']:.3e} "
                  f"(direct {r['e_direct']:.3e}, F(4,3) {r['e_wino']:.3e}), bound {r['bound']:.3e}")
            e_h, e_w, ratio = max(e_h, eh), max(e_w, ew), max(ratio, ew / r["yardstick"])
        record_measurement(f"vocshape_{name}_{form}_{batch}", wav_err=e_w, yardstick=max(r["yardstick"] for r in ref), ratio=ratio, har_err=e_h)
        for b, r in enumerate(ref):
            n = r["n"] * hop
            assert (har[b, :n] - r["har"]).abs().max().item() <= V.HAR_TOL
            assert (wav[b, :n].double() - r["wav64"]).abs().max().item() <= r["bound"], (name, batch, form, b)
    if _wino_switches(cfg):
        assert not torch.equal(wavs["wino"], wavs["direct"]), "SS_VOC_WINO=0 must have switched kernels (the two forms round differently)"


_SOURCE_GEN = {}


def _source_gen(name, monkeypatch):
    if name not in _SOURCE_GEN:
        _SOURCE_GEN[name] = _packed(name, monkeypatch, True)
    return _SOURCE_GEN[name]


@pytest.mark.parametrize("name", list(V.SOURCE_CASES))
def test_source_matches_restatement_at_this_contour(name, monkeypatch):
    """ss_hifigan_source alone against R.nsf_source with the same recorded rand_ini / sine_noise: the chunk carry of src_base_kernel and
    src_scan_kernel (T = SCAN_CHUNK + 1, 2 SCAN_CHUNK + 1), the voiced / unvoiced edges, wraps on frame boundaries, increments past 1."""
    gen = _source_gen(V.SOURCE_CASES[name][0], monkeypatch)
    f0, noise = V.source_inputs(name)
    ref = V.source_reference(name)
    har = _source(gen, f0, noise)
    err = (har - ref).abs().max().item()
    bound = V.source_bound(ref.shape[1])
    print(f"source {name}: {ref.shape[1]} samples, hop {gen.hop}: har max err {err:.3e} (bound {bound:.0e})")
    record_measurement(f"vocshape_source_{name}", har_err=err, samples=ref.shape[1], hop=gen.hop)
    assert har.shape == ref.shape and err <= bound, err


@pytest.mark.parametrize("name", list(V.PHILOX_CASES))
def test_source_philox_equals_its_restatement_as_a_tape(name, monkeypatch):
    """rand_ini = sine_noise = NULL (device Philox) at hop 64 and hop 1024, judged like test_gpu_noise.py judges the default hop: against the
    same call fed oracle.philox.vocoder_noise as tapes, the additive noise may differ by amp * (z_dev - z_host); and the tape run against
    R.nsf_source."""
    gname, T, seed = V.PHILOX_CASES[name]
    cfg, vsd = V.generator(gname)
    gen = _source_gen(gname, monkeypatch)
    hop = gen.hop
    f0 = torch.full((2, T), 220.0)
    f0[1] = 140.0 + 3.0 * torch.arange(T)
    f0[1, T // 4:T // 2] = 0.0
    noise = {k: v.float() for k, v in P.vocoder_noise(seed, 2, T * hop).items()}
    har_p = _source(gen, f0, None, seed=seed)
    har_t = _source(gen, f0, noise)
    r = P.sine_noise(2, T * hop, seed, want_radius=True)[1]
    lw = vsd["m_source.l_linear.weight"].reshape(-1).double().abs().numpy()
    amp = np.where(np.repeat(f0.numpy(), hop, axis=1) > 0, 0.003, 0.1 / 3.0)[..., None]
    bound = (amp * P.normal_bound(r) * lw).sum(-1) + 2.0 ** -21        # tanh is 1-Lipschitz; a few ulp of the O(1) sum
    ratio = float(((har_p - har_t).abs().double().numpy() / bound).max())
    with torch.no_grad():
        from oracle import restatement as R
        e_t = (har_t - R.nsf_source(vsd, cfg, f0, V.BatchTape(noise))).abs().max().item()
    print(f"source {name}: Philox vs restated tape {ratio:.3f} x bound; tape run vs the restatement {e_t:.3e}")
    record_measurement(f"vocshape_source_{name}", har_over_bound=ratio, har_err=e_t, hop=hop)
    assert ratio <= 1.0 and e_t <= V.HAR_TOL
    assert float((_source(gen, f0, dict(noise, sine_noise=noise["sine_noise"].roll(1, dims=1))) - har_p).abs().max()) > 1e-3
