"""The vocoder output denoise on the device (`ss_wav_denoise`, csrc/denoise.hip; hparams['vocoder_denoise_c']): the kernel against the float64
restatement (tests/denoise_ref.py) within the project's fp32 waveform bar, identity, silence, determinism and batch independence, graph capture,
the vocoder plugin and the batched path. Parity with librosa is UNPINNED (the package is un-vendored); the definition is
stylesinger_amd/denoise.py's."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import record_measurement  # noqa: E402
from denoise_ref import denoise_ref, sine_noise, zero_envelope  # noqa: E402
from oracle import harness  # noqa: E402
from stylesinger_amd import config, synth  # noqa: E402
from stylesinger_amd import denoise as DN  # noqa: E402
from stylesinger_amd.vocoder import HifiGAN  # noqa: E402

WAV_TOL = 1e-5   # the project's standing fp32 waveform bar (tests/test_gpu_parity.py)
GEOMETRIES = [(1024, 256), (512, 128), (2048, 512), (1024, 512), (256, 256)]
PAD = 37         # row stride = row width + PAD
V = 0.1
# the issue's case: ragged lengths of 1, 5 and 12 hops in rows 13 hops wide. "long": lengths that are no multiple of the hop, in rows wide enough
# for several workgroups per item at every geometry (a run is 4 N outputs, 3 N at N = 2048, N with hop == N), the second item ending inside a run
CASES = {"ragged": (13, lambda H: [H, 5 * H, 12 * H]), "long": (41, lambda H: [40 * H + 3, 17 * H + H - 1])}


@functools.lru_cache(maxsize=None)
def _case(N, H, which, v):
    """(lengths, the items' own samples, their restated output) of a geometry - computed once, never modified"""
    width, lens = CASES[which]
    lens = lens(H)
    xs = [sine_noise(n, 1000 * N + H + b, f=(440.0, 311.1, 97.0)[b]) for b, n in enumerate(lens)]
    return width * H, lens, xs, [denoise_ref(x, N, H, v) for x in xs]


def _device_input(xs, lens, width, fill="random"):
    """rows strided (ldx > width); what lies at or beyond an item's length is random (the generator writes garbage there) or NaN"""
    g = torch.Generator().manual_seed(5)
    buf = torch.rand(len(xs), width + PAD, generator=g) * 2 - 1 if fill == "random" else torch.full((len(xs), width + PAD), float("nan"))
    for b, x in enumerate(xs):
        buf[b, :lens[b]] = torch.from_numpy(x)
    return buf.cuda()[:, :width]


PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "denoise_parity.json")


def _write_profile(geometry, which, worst, bound):
    """profiles/denoise_parity.json: the measured maximum per geometry (fft_size x hop_size) and case, as the last run on a device saw it"""
    try:
        with open(PROFILE) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        doc = {}
    doc.setdefault("what", "ss_wav_denoise against the float64 restatement (tests/denoise_ref.py), v = 0.1: worst max-abs error per geometry "
                           "(fft_size x hop_size) and case of tests/test_gpu_denoise.py, written by the test; parity with librosa is unpinned")
    doc["pinned"] = False
    doc.setdefault("worst_abs_err", {}).setdefault(geometry, {})[which] = dict(worst_abs_err=worst, bound=bound)
    with open(PROFILE, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)


@pytest.mark.parametrize("which", ["ragged", "long"])
@pytest.mark.parametrize("N,H", GEOMETRIES + [(256, 64)])
def test_kernel_matches_the_float64_restatement(N, H, which):
    """max-abs <= 1e-5 against the float64 restatement at v = 0.1, n_out exact, exact zeros beyond n_out; the rows hold random values beyond
    each item's length. Measured on an MI355X (profiles/denoise_parity.json): 1.5e-7 ... 3.5e-7 at the fp32 geometries; 1.5e-6 at (256, 256),
    which runs in float64 - there the restated output reaches |y| = 50 next to the frame edges (the envelope w^2 falls to 0), and the figure is
    the fp32 rounding of the stored result (half an ulp of 50 = 1.9e-6). An fp32 transform lies 1e-4 ... 6e-4 away there
    (tests/test_denoise_cpu.py holds the host emulation). Every case rewrites its entry of profiles/denoise_parity.json."""
    width, lens, xs, refs = _case(N, H, which, V)
    xd = _device_input(xs, lens, width)
    assert xd.stride(0) == width + PAD
    y, n_out = DN.denoise_batch(xd, lens, N, H, N, V)
    torch.cuda.synchronize()
    assert y.shape == (len(lens), width) and n_out.dtype == torch.int32
    assert n_out.cpu().tolist() == [n // H * H for n in lens]
    y = y.cpu().numpy()
    worst = 0.0
    for b, (n, r) in enumerate(zip(lens, refs)):
        err = np.abs(y[b, :len(r)] - r).max()
        worst = max(worst, err)
        print(f"N {N} H {H} {which} item {b} (n {n}): max |y| {np.abs(r).max():.3f}, max abs err {err:.3e}")
        assert np.isfinite(y[b]).all()
        assert (y[b, len(r):] == 0.0).all(), "exact zeros beyond n_out"
    record_measurement(f"denoise_device_vs_float64_restatement_n{N}_h{H}_{which}", pinned=False, worst_abs_err=float(worst), bound=WAV_TOL)
    _write_profile(f"{N}x{H}", which, float(worst), WAV_TOL)
    assert worst <= WAV_TOL, worst


@pytest.mark.parametrize("N,H", GEOMETRIES)
def test_v_zero_is_the_identity(N, H):
    """v = 0 returns the input within the same bar, the first and last N/2 samples of every item and the 1-hop item included. At (256, 256) the
    samples whose envelope is zero (w[0] = 0: one per frame) come out as exactly 0."""
    width, lens, xs, _ = _case(N, H, "ragged", 0.0)
    y, _ = DN.denoise_batch(_device_input(xs, lens, width, fill="nan"), lens, N, H, N, 0.0)
    y = y.cpu().numpy()
    for b, (n, x) in enumerate(zip(lens, xs)):
        dead = zero_envelope(n, N, H)
        assert dead.sum() == (n // N if H == N else 0)
        err = np.abs(y[b, :n] - x)[~dead]
        print(f"N {N} H {H} item {b}: identity max abs err {err.max():.3e} (head {err[:N // 2].max():.3e}, tail {err[-(N // 2):].max():.3e})")
        assert err.max() <= WAV_TOL
        assert (y[b, :n][dead] == 0.0).all() and (y[b, n:] == 0.0).all()


@pytest.mark.parametrize("N,H", [(1024, 256), (256, 256)])
def test_silence(N, H):
    """a v above every bin's magnitude gives exactly 0.0 everywhere; a row of zeros gives zeros, not NaN (m = 0)"""
    width, lens, xs, _ = _case(N, H, "ragged", V)
    y, n_out = DN.denoise_batch(_device_input(xs, lens, width), lens, N, H, N, 1e6)
    assert (y == 0.0).all() and n_out.cpu().tolist() == lens
    for v in (0.0, V):
        y, _ = DN.denoise_batch(torch.zeros(2, width, device="cuda"), [width, 5 * H], N, H, N, v)
        assert (y == 0.0).all(), v


@pytest.mark.parametrize("which", ["ragged", "long"])
@pytest.mark.parametrize("N,H", [(1024, 256), (256, 256), (2048, 2048)])
def test_denoise_is_deterministic_and_independent_of_the_batch(N, H, which):
    """two runs are bit-equal; every row of the batch (the B = 3 rows of 1, 5 and 12 hops - alone, the 1-hop item's frame pairs end differently -
    and the rows that span several runs) is bit-equal to its own B = 1 call"""
    width, lens, xs, _ = _case(N, H, which, V)
    xd = _device_input(xs, lens, width)
    ya, na = DN.denoise_batch(xd, lens, N, H, N, V)
    yb, nb = DN.denoise_batch(xd, lens, N, H, N, V)
    assert torch.equal(ya, yb) and torch.equal(na, nb)
    for b, (n, x) in enumerate(zip(lens, xs)):     # alone: another B, another width, another stride, zeros instead of garbage behind the item
        one = torch.zeros(1, n + 5)
        one[0, :n] = torch.from_numpy(x)
        y1, n1 = DN.denoise_batch(one.cuda(), [n], N, H, N, V)
        k = n // H * H
        assert int(n1[0]) == k and torch.equal(y1[0, :k], ya[b, :k]), b


@pytest.mark.parametrize("which", ["ragged", "long"])
def test_float64_kernel_at_the_largest_frame(which):
    """hop_size == fft_size = 2048: the float64 instantiation at its largest LDS footprint (48 KB) and four butterflies per thread and step.
    There the restated output reaches |y| of several hundred next to the frame edges (1 / w[1] = 4.3e5), so the flat 1e-5 bar is below the fp32
    spacing of the stored values themselves. The bound is per sample: the result is a float64 value stored once as fp32, |err| <= 2^-24 |y|, plus
    the float64 transform's own error divided by w (4 log2(N) 2^-52 / w[1] = 4e-9) - 1e-8 covers it. The kernel takes v as fp32 (the C ABI), and
    1 / w amplifies the 1.5e-9 between fl32(0.1) and 0.1 into the 1e-5 range here, so the restatement is run at the value the kernel receives.
    v = 0 is the identity within the flat 1e-5 bar, exact zeros where the envelope is zero."""
    N = H = 2048
    v32 = float(np.float32(V))
    width, lens, xs, _ = _case(N, H, which, 0.0)
    xd = _device_input(xs, lens, width)
    y, n_out = DN.denoise_batch(xd, lens, N, H, N, V)
    y0, _ = DN.denoise_batch(xd, lens, N, H, N, 0.0)
    assert n_out.cpu().tolist() == [n // H * H for n in lens]
    y, y0 = y.cpu().numpy(), y0.cpu().numpy()
    worst = 0.0
    for b, (n, x) in enumerate(zip(lens, xs)):
        r = denoise_ref(x, N, H, v32)
        err = np.abs(y[b, :len(r)] - r)
        k = int(err.argmax())
        worst = max(worst, float(err.max()))
        print(f"N {N} H {H} {which} item {b} (n {n}): max |y| {np.abs(r).max():.1f}, max abs err {err.max():.3e} at |y| = {abs(r[k]):.1f} "
              f"(2^-24 |y| = {2.0 ** -24 * abs(r[k]):.3e})")
        assert (err <= 2.0 ** -24 * np.abs(r) + 1e-8).all(), (b, err.max())
        assert (y[b, len(r):] == 0.0).all() and np.isfinite(y[b]).all()
        dead = zero_envelope(n, N, H)
        k0 = n // H * H
        assert np.abs(y0[b, :k0] - x[:k0])[~dead].max() <= WAV_TOL and (y0[b, :k0][dead] == 0.0).all()
    _write_profile(f"{N}x{H}", which, worst, "2^-24 |y| + 1e-8 per sample")


def test_denoise_batch_is_graph_capturable_and_takes_device_lengths():
    N, H = 1024, 256
    width, lens, xs, _ = _case(N, H, "ragged", V)
    xd = _device_input(xs, lens, width)
    n_dev = torch.tensor(lens, dtype=torch.int32).cuda()
    eager, ne = DN.denoise_batch(xd, n_dev, N, H, N, V)     # (also uploads the table once)
    by_host, _ = DN.denoise_batch(xd, lens, N, H, N, V)
    assert torch.equal(eager, by_host)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, no = DN.denoise_batch(xd, n_dev, N, H, N, V)
    out.fill_(float("nan"))
    no.fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(no, ne)


# ---- plumbing -------------------------------------------------------------------------------------------------------------------------------
def test_plugin_spec2wav_denoises_with_the_hparam():
    """HifiGAN.spec2wav on the golden vocoder_t12 (weights, mel, f0 and noise as tests/test_gpu_parity.py loads them): with
    vocoder_denoise_c = 0.1 it returns the restatement applied to what the same call returns with 0.0 (<= 1e-5), and that differs from the
    undenoised waveform by more than 1e-4 somewhere - before the key was honoured it was ignored and the two calls were equal."""
    case = harness.load_case("vocoder_t12")
    meta = case["meta"]
    cfg, vsd = harness.vocoder_case_setup(meta)
    mel, f0 = case["inp"]["mel"][0].numpy(), case["inp"]["f0"][0].numpy()
    outs = {}
    for c in (0.0, 0.1):
        voc = HifiGAN(cfg, vsd, device="cuda:0", hparams=dict(vocoder_denoise_c=c))
        noise = synth.draw_vocoder_noise(synth.NoiseTape(meta["tape_seed"]), 1, meta["T"] * voc.model.hop)
        outs[c] = voc.spec2wav(mel, f0=f0, noise=noise)
    assert abs(outs[0.0] - case["out"]["wav"][0].numpy()).max() <= WAV_TOL, "off: the golden waveform, as before"
    want = denoise_ref(outs[0.0], 1024, 256, 0.1)
    err, moved = np.abs(outs[0.1] - want).max(), np.abs(outs[0.1] - outs[0.0]).max()
    print(f"spec2wav with vocoder_denoise_c = 0.1: max abs err {err:.3e} against the restatement; moved the waveform by up to {moved:.3e}")
    assert outs[0.1].shape == outs[0.0].shape == (meta["T"] * 256,) and outs[0.1].dtype == np.float32
    assert err <= WAV_TOL
    assert moved > 1e-4
    # another hop_size than the generator's: the reference's denoise() takes the hparams' geometry, length hop_size * (len // hop_size)
    voc = HifiGAN(cfg, vsd, device="cuda:0", hparams=dict(vocoder_denoise_c=0.1, fft_size=2048, win_size=2048, hop_size=512))
    noise = synth.draw_vocoder_noise(synth.NoiseTape(meta["tape_seed"]), 1, meta["T"] * voc.model.hop)
    w = voc.spec2wav(mel, f0=f0, noise=noise)
    assert np.abs(w - denoise_ref(outs[0.0], 2048, 512, 0.1)).max() <= WAV_TOL


@pytest.fixture(scope="module")
def tiny():
    """the smallest acoustic golden's model (acoustic_tiny_s4: B = 1, T = 48, 4 + 4 steps) with the key set, and two batches: the golden's own
    and a ragged one of 80 frames (long enough for a loudness reading)"""
    from stylesinger_amd.infer import StyleSingerInfer
    meta = harness.load_case("acoustic_tiny_s4")["meta"]
    hp, sd, batch = harness.case_setup(meta)
    hp = dict(hp, vocoder_denoise_c=V)
    inf = StyleSingerInfer(hp, device=torch.device("cuda:0"), model_state=sd, vocoder_state=synth.synth_vocoder_state_dict(None, 5))
    second = synth.synth_batch(2, 80, 8, 12, inf.hparams, 5)
    return inf, [{k: v.cuda() for k, v in b.items()} for b in (batch, second)]


def _undenoised(inf, res, seed):
    """what the generator wrote for a result of `infer_batch(seed=seed)`: the vocode call without the plugin's last step"""
    mel = res["mel"].clamp(float(inf.hparams["mel_vmin"]), float(inf.hparams["mel_vmax"]))
    return inf.vocoder.model(mel, res["f0"], lens=res["lens"], seed=seed + 101)


def test_batched_path_denoises_every_item_before_the_loudness_target(tiny):
    from stylesinger_amd import loudness as LD
    inf, batches = tiny
    hop = inf.vocoder.model.hop
    assert inf.vocoder._denoise_v == V and hop == 256
    for i, batch in enumerate(batches):
        res = inf.infer_batch(batch, seed=3)
        raw = _undenoised(inf, res, 3)
        assert res["wav"].shape == raw.shape
        for b, frames in enumerate(res["lens"].cpu().tolist()):
            n = frames * hop
            want = denoise_ref(raw[b, :n].cpu().numpy(), 1024, 256, V)
            err = np.abs(res["wav"][b, :n].cpu().numpy() - want).max()
            moved = (res["wav"][b, :n] - raw[b, :n]).abs().max().item()
            print(f"batch {i} item {b} ({frames} frames): max abs err {err:.3e} against the restatement of the undenoised item; moved by {moved:.3e}")
            assert err <= WAV_TOL and moved > 1e-4
            assert (res["wav"][b, n:] == 0.0).all()
    # the loudness target sees the denoised rows
    res = inf.infer_batch(batches[1], seed=3)
    lens = [int(v) * hop for v in res["lens"].cpu()]
    assert min(lens) >= 0.4 * 48000
    loud = inf.infer_batch(batches[1], seed=3, out_lufs=-16.0)
    want, m = LD.normalize_batch(res["wav"], lens, 48000, target=-16.0, short="skip")
    assert torch.equal(loud["wav"], want) and torch.equal(loud["lufs"], m["lufs"])
    assert not torch.equal(loud["wav"], res["wav"])


def test_batches_in_flight_denoise_like_single_batches(tiny):
    inf, batches = tiny
    got = list(inf.infer_batches(batches, in_flight=2, seed=40))
    torch.cuda.synchronize()
    assert len(got) == 2
    for i, b in enumerate(batches):
        want = inf.infer_batch(b, seed=40 + i)
        assert torch.equal(got[i]["wav"], want["wav"]), i
        assert not torch.equal(want["wav"], _undenoised(inf, want, 40 + i))
