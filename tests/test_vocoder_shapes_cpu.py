"""CPU side of the vocoder shape tests: the input conditions of tests/test_gpu_vocoder_shapes.py from the reference side alone, and the
refusals of vocoder.check_config. (The restatement at these shapes is pinned to the REAL reference by the vocoder_hop512_t6 /
vocoder_hop64_b2_t9 fixtures of test_oracle_golden.py.)"""
import copy

import numpy as np
import pytest
import torch

import vocoder_shape_cases as V
from oracle import harness
from stylesinger_amd import config
from stylesinger_amd.lib import StyleSingerHipError
from stylesinger_amd.vocoder import check_config


@pytest.mark.parametrize("batch", list(V.BATCHES))
@pytest.mark.parametrize("name", list(V.GENERATOR_CASES))
def test_wav_bound_of_every_generator_case_is_within_the_projects_bar(name, batch):
    """(a) 4 x the fp32 CPU yardstick (floored at 2 ulp) never exceeds WAV_TOL = 1e-5: the new device tests are never looser than the existing ones.
    The yardstick itself must be a real fp32 error: nonzero, and far below the signal."""
    ref = V.generator_reference(name, batch)
    assert [r["n"] for r in ref] == list(V.BATCHES[batch][2]) and min(r["n"] for r in ref) >= 1
    for r in ref:
        print(f"{name} {batch} T={r['n']}: direct {r['e_direct']:.3e} F(4,3) {r['e_wino']:.3e} -> bound {r['bound']:.3e}; |wav| max {r['wav64'].abs().max().item():.3f}")
        assert 0.0 < r["yardstick"] and V.WAV_FLOOR <= r["bound"] <= V.WAV_TOL
        assert r["wav64"].abs().max().item() > 1e3 * r["bound"], "a waveform this small would pass with any kernel"
        assert r["har"].dtype == torch.float32 and r["wav64"].dtype == torch.float64


def test_generator_cases_reach_the_paths_they_are_chosen_for():
    cfgs = {n: V.generator(n)[0] for n in V.GENERATOR_CASES}
    for cfg in cfgs.values():
        check_config(cfg)          # every case is a supported shape
    assert {n: V.hop_of(c) for n, c in cfgs.items()} == dict(hop512_5ups=512, hop64_2ups=64, hop1024=1024, wide1024=256, default=256)
    assert cfgs["hop512_5ups"]["upsample_initial_channel"] >> 5 == 16
    assert cfgs["wide1024"]["upsample_initial_channel"] >> 1 == 512
    assert len(cfgs["hop64_2ups"]["resblock_kernel_sizes"]) == 2 and (9 * 64) % 256 != 0
    assert cfgs["hop1024"]["upsample_rates"][2:] == [4, 4]
    assert cfgs["default"] == config.make_vocoder_config()


@pytest.mark.parametrize("name", list(V.SOURCE_CASES))
def test_source_contours_are_off_the_wrap_knife_edge(name):
    """(b) A second, per-frame closed-form float64 statement of the source (vocoder_shape_cases.nsf_source_closed_form) agrees with
    R.nsf_source to a quarter of the bound the device is held to. A contour for which the two disagree has a wrap decided by the last bit of
    a running sum: no implementation can be held to either answer there, and the contour is to be replaced, not the bound widened."""
    gen, kind, T = V.SOURCE_CASES[name]
    cfg, vsd = V.generator(gen)
    f0, noise = V.source_inputs(name)
    ref = V.source_reference(name)
    assert f0.shape == (2, T) and (kind == "all_unvoiced" or not torch.equal(f0[0], f0[1]))
    cf = V.nsf_source_closed_form(vsd, cfg, f0, noise)
    err = float(np.abs(cf - ref.double().numpy()).max())
    bound = V.source_bound(ref.shape[1])
    print(f"{name}: {ref.shape[1]} samples: closed form vs restatement {err:.3e} (bound / 4 = {bound / 4:.1e})")
    assert ref.shape == (2, T * V.hop_of(cfg)) and err <= bound / 4


def test_source_cases_cover_the_edges_they_name():
    sr, hop = 16000, 64
    f = {n: V.source_inputs(n)[0] for n in V.SOURCE_CASES}
    assert V.SOURCE_CASES["carry_2chunks"][2] == V.SCAN_CHUNK + 1 and V.SOURCE_CASES["carry_3chunks"][2] == 2 * V.SCAN_CHUNK + 1
    assert V.source_bound(V.SOURCE_CASES["carry_2chunks"][2] * hop) == V.HAR_TOL_LONG and V.source_bound(1024 * 40) == V.HAR_TOL
    assert bool((f["first_unvoiced"][:, 0] == 0).all()) and bool((f["first_unvoiced"][:, 1:] > 0).all())
    assert bool((f["all_unvoiced"] == 0).all())
    assert bool((f["constant"] == f["constant"][:, :1]).all()) and bool((f["constant"] > 0).all())
    a = f["alternating"] > 0
    assert bool((a[:, 1:] != a[:, :-1]).all()) and bool(a[0, 1]) and bool(a[1, 0])
    adv = f["integer_advance"].double() * hop / sr
    assert bool((adv == adv.round()).all()) and bool((adv >= 1).all())
    assert float(f["high_4000hz_sr16000"].max()) == 4000.0 and 4000.0 * 9 / sr >= 1


REFUSED = [
    ("resblock", "2"),
    ("harmonic_num", 7),
    ("use_pitch_embed", False),
    ("audio_sample_rate", 0),
    ("upsample_rates", [8, 8, 2, 2, 2, 2, 2]),                  # 7 stages
    ("upsample_rates", [8, 8, 2, 1]),                           # hop 128, odd rate
    ("upsample_kernel_sizes", [16, 16, 4, 8]),                  # k != 2u
    ("upsample_kernel_sizes", [16, 16, 4]),
    ("upsample_initial_channel", 24),                           # does not halve four times
    ("upsample_initial_channel", 32),                           # leaves 2 channels: no multiple of 4
    ("upsample_initial_channel", 4096),                         # leaves 256 channels for conv_post
    ("resblock_kernel_sizes", [3, 7, 11, 13, 15]),              # 5 kernels
    ("resblock_kernel_sizes", [3, 7, 17]),                      # more taps than a conv launch takes
    ("resblock_kernel_sizes", [3, 4, 11]),                      # even kernel
    ("resblock_dilation_sizes", [[1, 3, 5], [1, 3, 5]]),        # one list short
    ("resblock_dilation_sizes", [[1, 3], [1, 3, 5], [1, 3, 5]]),
    ("resblock_dilation_sizes", [[1, 3, 5, 7], [1, 3, 5], [1, 3, 5]]),
    ("resblock_dilation_sizes", [[0, 3, 5], [1, 3, 5], [1, 3, 5]]),
]


@pytest.mark.parametrize("key,value", REFUSED, ids=[f"{k}-{i}" for i, (k, _) in enumerate(REFUSED)])
def test_check_config_refuses_and_names_the_key(key, value):
    cfg = config.make_vocoder_config()
    cfg[key] = value
    with pytest.raises(StyleSingerHipError, match=key):
        check_config(cfg)


def test_check_config_refuses_hops_the_source_kernels_cannot_run():
    for rates in ([8, 2, 2], [4, 4, 2], [8, 8, 8, 4], [2, 2, 2, 2, 2, 2]):      # hop 32, 32, 2048, 64 (the last one is fine)
        cfg = config.make_vocoder_config(dict(upsample_rates=rates, upsample_kernel_sizes=[2 * u for u in rates]))
        hop = int(np.prod(rates))
        if hop % 64 == 0 and hop <= 1024:
            assert check_config(cfg) is cfg
        else:
            with pytest.raises(StyleSingerHipError, match="upsample_rates"):
                check_config(cfg)


def test_check_config_is_pure_and_pack_calls_it_first():
    cfg = config.make_vocoder_config()
    before = copy.deepcopy(cfg)
    assert check_config(cfg) is cfg and cfg == before
    import inspect
    from stylesinger_amd.vocoder import HifiGanGeneratorHIP
    first = [ln.strip() for ln in inspect.getsource(HifiGanGeneratorHIP.pack).splitlines()[1:] if ln.strip()][0]
    assert "check_config(self.h)" in first


def test_vocoder_case_setup_reads_the_config_override_of_a_fixture():
    over = dict(upsample_rates=[8, 8], upsample_kernel_sizes=[16, 16], upsample_initial_channel=128)
    cfg, vsd = harness.vocoder_case_setup(dict(seed=3, cfg_over=over))
    assert cfg["upsample_rates"] == [8, 8] and vsd["conv_pre.bias"].shape == (128,)
    cfg0, _ = harness.vocoder_case_setup(dict(seed=3))
    assert cfg0 == config.make_vocoder_config()
