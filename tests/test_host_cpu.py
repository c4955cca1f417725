"""CPU-side checks (no GPU): the C-ABI library loads and exports every declared symbol, the ctypes mirror
matches the C structs, the parameter/hparams contract matches the reference dump, synthetic data is
deterministic, and the product refuses to run without a GPU instead of falling back."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from stylesinger_amd import abi, config, lib, spec, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_at_abi_20_and_exports_header_symbols():
    l = lib.load()
    names = lib.declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(l, n), n
    assert l.ss_abi_version() == lib.ABI_VERSION == 20
    assert l.ss_last_error() is not None


def test_ctypes_struct_mirror_matches_c():
    import ctypes
    l = lib.load()
    sizes = (ctypes.c_int64 * 6)()
    assert l.ss_struct_sizes(sizes, 6) == 0
    assert tuple(sizes) == tuple(ctypes.sizeof(c) for c in (lib.ConvGemmArgs, lib.WaveNet, lib.HifiGan, lib.GemmBf16Args, lib.F0TrackParams, lib.Layer512Args))
    assert tuple(sizes) == (400, 3616, 3888, 264, 104, 136)


STRUCT_FIELDS = {"ss_conv_gemm_args": 56, "ss_wavenet": 89, "ss_gemm_bf16_args": 43, "ss_layer512_args": 22, "ss_hifigan": 27, "ss_f0track_params": 17}


def test_every_struct_field_has_the_c_compilers_offset_and_size(tmp_path):
    """abi.STRUCTS (read from the header) against the host C compiler: a C99 program generated from the parsed field NAMES prints sizeof of every
    struct and offsetof / sizeof of every member of include/stylesinger_hip.h; the ctypes classes must agree on all of them, which two swapped
    fields of one width or an array nested the wrong way round would not."""
    import ctypes
    assert set(abi.STRUCTS) >= set(STRUCT_FIELDS)
    assert {n: len(abi.STRUCTS[n]) for n in STRUCT_FIELDS} == STRUCT_FIELDS
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stylesinger_hip.h"', 'int main(void) {']
    for name, fields in abi.STRUCTS.items():
        lines.append(f'  printf("{name} - %zu 0\\n", sizeof({name}));')
        lines += [f'  printf("{name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in fields]
    src, exe = tmp_path / "abi_layout.c", str(tmp_path / "abi_layout")
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    r = subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0
    c_side = [tuple(ln.split()[:2]) + tuple(int(v) for v in ln.split()[2:]) for ln in r.stdout.splitlines()]
    py_side = []
    for name, fields in abi.STRUCTS.items():
        cls = abi.STRUCTURES[name]
        py_side.append((name, "-", ctypes.sizeof(cls), 0))
        py_side += [(name, f, getattr(cls, f).offset, getattr(cls, f).size) for f, _ in fields]
    assert len(py_side) == len(abi.STRUCTS) + sum(len(f) for f in abi.STRUCTS.values()) >= 6 + 254
    assert py_side == c_side, [(p, c) for p, c in zip(py_side, c_side) if p != c][:5]


def test_parsed_array_shapes_and_constants():
    import ctypes
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert dict(lib.WaveNet._fields_)["w_dil"] is vp * 32
    assert dict(lib.HifiGan._fields_)["rb_d"] is (i32 * 3) * 4
    hg = lib.HifiGan()
    assert (len(hg.w_rb1), len(hg.w_rb1[0]), len(hg.w_rb1[0][0])) == (6, 4, 3) and dict(lib.HifiGan._fields_)["w_rb1"] is ((vp * 3) * 4) * 6
    hg.w_rb1[5][3][2] = 7      # the last element: the three-level indexing stylesinger_amd/vocoder.py uses
    assert ctypes.cast(ctypes.byref(hg, lib.HifiGan.w_rb1.offset), ctypes.POINTER(vp))[6 * 4 * 3 - 1] == 7
    assert len(lib.ConvGemmArgs().tap_off) == 16 and len(lib.GemmBf16Args().tap_off) == 4
    assert (lib.SS_MAX_TAPS, lib.SS_MAX_LAYERS, lib.SS_HG_MAX_UPS, lib.SS_HG_MAX_KERNELS) == (16, 32, 6, 4)
    assert lib.ABI_VERSION == 20 == abi.DEFINES["SS_ABI_VERSION"]
    assert (lib.EPI_STORE, lib.EPI_GATE, lib.EPI_RESSKIP, lib.EPI_DDPM) == (0, 1, 2, 3)
    assert (lib.ACT_NONE, lib.ACT_RELU, lib.ACT_GELU, lib.ACT_MISH, lib.ACT_TANH, lib.ACT_LRELU) == (0, 1, 2, 3, 4, 5)
    assert (lib.HEPI_STORE, lib.HEPI_GATE, lib.HEPI_RESX) == (0, 1, 2)
    assert [abi.ENUMS[n] for n in ("SS_TILE_AUTO", "SS_TILE_128x128", "SS_TILE_64x128", "SS_TILE_64x64", "SS_TILE_128x64", "SS_TILE_128x32")] == [0, 1, 2, 3, 4, 5]
    assert lib.declarations is abi.declarations and lib.declared_symbols is abi.declared_symbols


@pytest.mark.parametrize("what,snippet,offending", [
    ("unknown base type", "typedef struct s { int32_t a; unsigned b; } s;", "unsigned b"),
    ("unknown base type", "typedef struct s { uint16_t h; } s;", "uint16_t h"),          # uint16_t and void only behind a pointer
    ("bit-field", "typedef struct s { int32_t a : 3; } s;", "int32_t a : 3"),
    ("nested struct", "typedef struct s { struct { int32_t a; } in; int32_t b; } s;", "struct { int32_t a"),
    ("nested union", "typedef struct s { int32_t t; union { float f; int32_t i; } u; } s;", "union { float f"),
    ("preprocessor line", "typedef struct s {\n  int32_t a;\n#ifdef SS_WIDE\n  int64_t b;\n#endif\n} s;", "#ifdef SS_WIDE"),
    ("dimension", "typedef struct s { float w[SS_NOT_DEFINED]; } s;", "float w[SS_NOT_DEFINED]"),
    ("dimension", "typedef struct s { float w[SS_N + 1]; } s;", "float w[SS_N + 1]"),
    ("mixed pointer list", "typedef struct s { const float* a, b; } s;", "const float* a, b"),
    ("mixed pointer list", "typedef struct s { float a, *b; } s;", "float a, *b"),
    ("four dimensions", "typedef struct s { float w[2][2][2][2]; } s;", "float w[2][2][2][2]"),
])
def test_struct_parser_refuses_what_it_cannot_read(what, snippet, offending):
    with pytest.raises(abi.HeaderError) as e:
        abi.parse_structs(snippet, {"SS_N": 4})
    assert offending in str(e.value), (what, str(e.value))


def test_struct_parser_reads_the_accepted_grammar_and_requires_enum_values():
    import ctypes
    got = abi.parse_structs("typedef struct s {\n  const float* p, *q[2];\n  int32_t a, b[SS_N], c[2][3];\n  double d;\n  void* v;\n} s;", {"SS_N": 4})
    vp = ctypes.c_void_p
    assert got == {"s": [("p", vp), ("q", vp * 2), ("a", ctypes.c_int32), ("b", ctypes.c_int32 * 4), ("c", (ctypes.c_int32 * 3) * 2), ("d", ctypes.c_double), ("v", vp)]}
    assert abi.parse_enums("enum { A = 0, B = 5 };") == {"A": 0, "B": 5}
    with pytest.raises(abi.HeaderError) as e:
        abi.parse_enums("enum { A = 0, B };")
    assert "'B'" in str(e.value)


def test_abi_module_imports_without_torch():
    r = subprocess.run([sys.executable, "-c", "import sys; import stylesinger_amd.abi as a; assert len(a.STRUCTURES) >= 6; print('torch' in sys.modules)"],
                       capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == "False", r.stdout + r.stderr[-2000:]


def test_argument_errors_are_reported_not_crashed():
    l = lib.load()
    assert l.ss_conv_gemm(None, None) != 0
    assert b"null args" in l.ss_last_error()
    assert l.ss_layernorm(None, None, None, None, 1, 1, 8, 8, 8, 8, 8, 1e-5, None, 0, None) != 0
    # round-5 entry points: the input producers refuse bad arguments before touching a device
    assert l.ss_f0track(None, 0, None, None, None, 1, 1, None, None, None, None, 1, 0, None, 0, None) != 0 and b"ss_f0track" in l.ss_last_error()
    assert l.ss_f0track_workspace_bytes(2, 143, 899) > 2 * 143 * 900 * 8 and l.ss_f0track_workspace_bytes(0, 1, 1) == 0
    assert l.ss_vad_trim(None, 0, None, None, 0, 1, 1, 480, 8, 6, None, 0, None, None, None) != 0 and b"ss_vad_trim" in l.ss_last_error()
    assert l.ss_normalize_volume(None, None, None, 1, 1, -30.0, None) != 0
    assert l.ss_round_f16_rows(None, 0, 0, None, None, None, 0, 1, None) != 0
    assert not hasattr(l, "ss_fused_gate_res")   # the dataflow-launch experiment of round 5 was never part of the library
    assert l.ss_set_tuning(b"q4_force", 1) == 0 and l.ss_get_tuning(b"q4_force") == 1 and l.ss_set_tuning(b"q4_force", 0) == 0
    assert l.ss_set_tuning(b"tile128", 1) != 0 and l.ss_set_tuning(b"skip_deep", 1) != 0      # removed in round 5
    # round-6 entry points
    import ctypes
    assert l.ss_layer512(None, None) != 0 and b"ss_layer512" in l.ss_last_error()
    a = lib.Layer512Args()
    assert l.ss_layer512(ctypes.byref(a), None) != 0 and b"null Hin" in l.ss_last_error()
    assert l.ss_layer512_entry(None, 256, 0, None, None, None, None, 1, 1, None) != 0 and l.ss_layer512_tile_addend(None, 512, 0, None, 1, 1, None) != 0
    assert l.ss_layer512_pack_gate(None, None, 2, None) != 0 and l.ss_layer512_pack_res(None, None, 2, None) != 0
    assert l.ss_debug_null_launch(0, 64, None) != 0 and l.ss_set_q4_guard(None) == 0


def test_param_spec_matches_reference_dump(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "param_spec.json")))
    mine = spec.acoustic_spec(config.make_hparams())
    assert [[k, list(s)] for k, s in mine] == ref["acoustic"]
    minev = spec.vocoder_spec(config.make_vocoder_config())
    assert [[k, list(s)] for k, s in minev] == ref["vocoder"]


def test_prodiff_and_emotion_specs_match_reference_dump(golden_dir):
    """hparams['decoder'] = 'prodiff' (stylesinger.py:111-117) and the emotion encoder (data_gen/tts/emotion/model.py)."""
    ref = json.load(open(os.path.join(golden_dir, "param_spec.json")))
    hp = config.make_hparams(dict(decoder="prodiff", timesteps=8, K_step=8, f0_timesteps=2, schedule_type="vpsde"))
    assert [[k, list(s)] for k, s in spec.acoustic_spec(hp)] == ref["acoustic_prodiff"]
    assert [[k, list(s)] for k, s in spec.emotion_spec()] == ref["emotion"]
    sd = synth.synth_acoustic_state_dict(hp, 3)
    assert set(sd) == {k for k, _ in ref["acoustic_prodiff"]} and sd["diff_decoder.betas"].shape == (9,)


def test_emotion_partial_slices_match_reference(golden_dir):
    """emotion.compute_partial_slices vs the reference's (inference.py:56-108) for several utterance lengths."""
    from stylesinger_amd import emotion
    case = torch.load(os.path.join(golden_dir, "emotion_p5.pt"), weights_only=False)
    assert case["meta"]["partial_slices"]
    for n, (wav_ref, mel_ref) in case["meta"]["partial_slices"].items():
        wav, mel = emotion.compute_partial_slices(n)
        assert [(s.start, s.stop) for s in wav] == [tuple(x) for x in wav_ref], n
        assert [(s.start, s.stop) for s in mel] == [tuple(x) for x in mel_ref], n


def test_plan_cache_is_lru_bounded_by_bytes():
    """The plan / hipGraph cache of StyleSingerHIP (host logic only): frames are bucketed, plans evicted least-recently-used."""
    from stylesinger_amd.model import StyleSingerHIP, _pad_frames
    hp = config.make_hparams(dict(timesteps=2, K_step=2, f0_timesteps=2))
    m = StyleSingerHIP(None, hparams=hp)
    assert m.t_bucket == 64 and [m.bucket_frames(t) for t in (1, 64, 65, 1500)] == [64, 64, 128, 1536]
    x = torch.arange(6.0).reshape(1, 2, 3)
    assert _pad_frames(x, 5).shape == (1, 2, 5) and _pad_frames(x, 4, dim=1).shape == (1, 4, 3)
    assert torch.equal(_pad_frames(x, 5)[..., :3], x) and _pad_frames(x, 5)[..., 3:].abs().sum() == 0

    class FakePlan:
        def __init__(self, b):
            self.bytes, self.uses = b, 0
    import stylesinger_amd.plans as M
    orig = M._DiffPlan
    M._DiffPlan = lambda model, B, T, dev: FakePlan(B * T)
    try:
        m.plan_bytes = 1000
        dev = torch.device("cuda", 0)
        a = m._plan(1, 400, dev); b = m._plan(1, 500, dev)
        assert list(m._plans) == [(1, 400, 0), (1, 500, 0)]
        assert m._plan(1, 400, dev) is a                       # hit: moves to the recent end
        m._plan(1, 300, dev)                                   # 400 + 500 + 300 > 1000 -> evicts the LRU one (500)
        assert list(m._plans) == [(1, 400, 0), (1, 300, 0)]
        m.use_graphs = "auto"
        a.uses = 1
        assert not m._want_graphs(a)
        a.uses = 2
        assert m._want_graphs(a)                               # captured on the second use of a shape
    finally:
        M._DiffPlan = orig


def test_hparams_match_reference_dump(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "hparams.json")))
    hp = config.make_hparams()
    for k, v in ref.items():
        assert hp[k] == v, k


def test_synthetic_weights_and_inputs_are_deterministic():
    hp = config.make_hparams(dict(timesteps=4, K_step=4, f0_timesteps=4))
    a = synth.synth_acoustic_state_dict(hp, 7)
    b = synth.synth_acoustic_state_dict(hp, 7)
    assert set(a) == {n for n, _ in spec.acoustic_spec(hp)}
    for k in ("mel_out.weight", "postdiff.denoise_fn.residual_layers.3.dilated_conv.weight", "postdiff.betas"):
        assert torch.equal(a[k], b[k])
    assert a["gm_diffnet.mlp.0.weight"] is a["f0_gen._denoise_fn.mlp.0.weight"]
    x = synth.synth_batch(2, 20, 4, 16, hp, 3)
    y = synth.synth_batch(2, 20, 4, 16, hp, 3)
    assert all(torch.equal(x[k], y[k]) for k in x)
    assert (x["mel2ph"] > 0).all() and x["mel2ph"].max() == 4


def test_model_state_dict_contract_and_no_cpu_fallback():
    from stylesinger_amd.model import StyleSingerHIP
    hp = config.make_hparams(dict(timesteps=2, K_step=2, f0_timesteps=2))
    m = StyleSingerHIP(None, hparams=hp)
    sd = synth.synth_acoustic_state_dict(hp, 1)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.state_dict()["ln_proj.weight"], sd["ln_proj.weight"])
    with pytest.raises(RuntimeError):
        m.load_state_dict({"bogus": torch.zeros(1)}, strict=True)
    m.eval()
    with pytest.raises(RuntimeError):
        m.train()
    if not torch.cuda.is_available():
        b = synth.synth_batch(1, 8, 2, 8, hp, 1)
        with pytest.raises(lib.StyleSingerHipError):
            m(b["txt_tokens"], mel2ph=b["mel2ph"], spk_embed=b["spk_embed"], emo_embed=b["emo_embed"], ref_mels=b["ref_mels"],
              ref_f0=b["ref_f0"], infer=True, global_steps=320000, note=b["note"], note_dur=b["note_dur"], note_type=b["note_type"])


def test_vocoder_registry_surface():
    from stylesinger_amd import vocoder
    assert vocoder.get_vocoder_cls({"vocoder": "HifiGAN_NSF"}) is vocoder.HifiGAN
    g = vocoder.HifiGanGeneratorHIP()
    vsd = synth.synth_vocoder_state_dict()
    g.load_state_dict(vsd, strict=True)
    assert g.hop == 256


def test_sweep_plan_covers_every_pair_exactly_once():
    """BASELINE config 5 sharding: references rank::world (tasks/tts/tts_base.py:132), one target x `batch` refs per batch."""
    from stylesinger_amd.sweep import bucket_frames, sweep_plan
    n_refs, n_tgt, world, batch = 13, 5, 4, 3
    seen = set()
    for rank in range(world):
        for t, refs in sweep_plan(n_refs, n_tgt, rank, world, batch):
            assert 1 <= len(refs) <= batch
            for r in refs:
                assert r % world == rank
                assert (r, t) not in seen
                seen.add((r, t))
    assert len(seen) == n_refs * n_tgt
    # the BASELINE sizes: 256 x 256 over 8 GPUs -> 8192 pairs per GPU
    assert sum(len(r) for _, r in sweep_plan(256, 256, 3, 8, 8)) == 8192
    assert bucket_frames(1500, 64) == 1536 and bucket_frames(1536, 64) == 1536 and bucket_frames(7, 1) == 7


def test_wav_writer_emits_pcm16_riff(tmp_path):
    """write_wav_pcm16 must be readable as what scipy.io.wavfile.write produces for int16 (utils/audio.py:12-17)."""
    import numpy as np
    from scipy.io import wavfile
    from stylesinger_amd.writer import write_wav_pcm16
    rng = np.random.default_rng(0)
    pcm = rng.integers(-32768, 32767, size=4801, dtype=np.int16)
    p = tmp_path / "a.wav"
    write_wav_pcm16(str(p), pcm, 48000)
    sr, back = wavfile.read(str(p))
    assert sr == 48000 and back.dtype == np.int16 and np.array_equal(back, pcm)
    q = tmp_path / "b.wav"
    wavfile.write(str(q), 48000, pcm)
    assert p.read_bytes() == q.read_bytes()


def test_checkpoint_intake_reads_both_reference_layouts(tmp_path):
    """ckpt.load_ckpt follows utils/commons/ckpt_utils.py:26-67: newest step wins, flat and nested state_dict layouts,
    strict=False drops shape mismatches; the vocoder loader follows hifigan_nsf.py:24-61 (yaml and json flavours)."""
    import yaml
    from stylesinger_amd import ckpt
    from stylesinger_amd.model import StyleSingerHIP
    from stylesinger_amd.vocoder import HifiGanGeneratorHIP
    hp = config.make_hparams(dict(timesteps=4, K_step=4, f0_timesteps=4))
    sd = synth.synth_acoustic_state_dict(hp, 3)
    exp = tmp_path / "exp"
    exp.mkdir()
    old = {k: torch.zeros_like(v) for k, v in sd.items()}
    torch.save({"state_dict": {"model": old}, "optimizer_states": [1, 2, 3]}, exp / "model_ckpt_steps_1000.ckpt")
    torch.save({"state_dict": {"model." + k: v for k, v in sd.items()}, "global_step": 2000}, exp / "model_ckpt_steps_2000.ckpt")
    assert [os.path.basename(p) for p in ckpt.get_all_ckpts(str(exp))] == ["model_ckpt_steps_2000.ckpt", "model_ckpt_steps_1000.ckpt"]
    m = StyleSingerHIP(None, hparams=hp)
    path = ckpt.load_ckpt(m, str(exp), "model", strict=True)
    assert path.endswith("2000.ckpt")
    got = m.state_dict()
    assert all(torch.equal(got[k], sd[k]) for k in sd)
    # nested layout + explicit file + strict=False with one mismatched shape
    bad = dict(sd)
    bad["mel_out.bias"] = torch.zeros(7)
    torch.save({"state_dict": {"model": bad}}, exp / "other.ckpt")
    m2 = StyleSingerHIP(None, hparams=hp)
    ckpt.load_ckpt(m2, str(exp / "other.ckpt"), "model", strict=False)
    assert torch.equal(m2.state_dict()["encoder.embed_tokens.weight"], sd["encoder.embed_tokens.weight"])
    assert ckpt.load_ckpt(m2, str(tmp_path / "nothing"), force=False) is None
    with pytest.raises(FileNotFoundError):
        ckpt.load_ckpt(m2, str(tmp_path / "nothing"))
    n = ckpt.strip(str(exp), str(tmp_path / "infer.pt"))
    assert n == len(sd) and set(torch.load(tmp_path / "infer.pt")["state_dict"]["model"]) == set(sd)
    # vocoder: yaml flavour and json flavour
    cfg = config.make_vocoder_config()
    vsd = synth.synth_vocoder_state_dict(cfg, 3)
    vy = tmp_path / "voc_yaml"
    vy.mkdir()
    yaml.safe_dump(cfg, open(vy / "config.yaml", "w"))
    torch.save({"state_dict": {"model_gen": vsd}}, vy / "model_ckpt_steps_5.ckpt")
    vj = tmp_path / "voc_json"
    vj.mkdir()
    json.dump(cfg, open(vj / "config.json", "w"))
    torch.save({"generator": vsd}, vj / "generator_v1")
    for d in (vy, vj):
        st, c = ckpt.load_vocoder_ckpt(str(d))
        g = HifiGanGeneratorHIP(c)
        g.load_state_dict(st, strict=True)
        assert c["upsample_rates"] == cfg["upsample_rates"]


def test_frontend_host_tables_match_the_oracle():
    """The host-built tables of the GPU mel front end (Slaney filterbank) against oracle/frontend.py, itself pinned by
    librosa's documented known answers; pure numpy, no GPU."""
    import numpy as np
    from oracle import frontend as F
    from stylesinger_amd.frontend import mel_filterbank
    for sr, n_fft, n_mels, fmin, fmax in ((48000, 1024, 80, 20, 24000), (22050, 2048, 128, 0.0, 11025.0), (22050, 1024, 80, 80, 7600)):
        a = mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
        b = F.mel_basis(sr, n_fft, n_mels, fmin, fmax)
        assert a.shape == b.shape == (n_mels, 1 + n_fft // 2)
        assert np.abs(a - b).max() <= 1e-7


def test_sampler_schedules_and_mode_flags():
    from stylesinger_amd.model import StyleSingerHIP
    m = StyleSingerHIP(None, hparams=config.make_hparams(dict(timesteps=100, K_step=100, f0_timesteps=100)))
    ts = m.ddim_timesteps(50)
    assert ts[0] == 99 and ts[-1] == 0 and len(ts) == 50 and all(a > b for a, b in zip(ts, ts[1:]))
    assert m.ddim_timesteps(1000) == list(range(99, -1, -1)) and m.ddim_timesteps(1) == [0]
    assert not m.bf16 and m.use_wino and m.wino_m == 4 and m.defer_skip and m.fold_skip
    mb = StyleSingerHIP(None, hparams=config.make_hparams(dict(mfma_precision="bf16")))
    assert mb.bf16 and not mb.use_wino and mb.defer_skip and not mb.fold_skip


def test_winograd_form_is_selected_by_the_environment(monkeypatch):
    from stylesinger_amd.model import StyleSingerHIP
    hp = config.make_hparams({})
    monkeypatch.setenv("SS_WINO_M", "2")
    assert StyleSingerHIP(None, hparams=hp).wino_m == 2
    monkeypatch.setenv("SS_WINO_M", "3")
    with pytest.raises(AssertionError):
        StyleSingerHIP(None, hparams=hp)
    monkeypatch.delenv("SS_WINO_M")
    monkeypatch.setenv("SS_WINO", "0")
    assert not StyleSingerHIP(None, hparams=hp).use_wino


def test_f43_transform_matrices_reproduce_the_three_tap_conv():
    """The F(4,3) constants written in csrc/wino43_gate.hip (input rows, weight transform, output combination), restated with numpy:
    four outputs of a 3-tap correlation from six products, for random inputs, to fp64 rounding."""
    rng = np.random.default_rng(0)
    BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], float)
    G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], float)
    for _ in range(20):
        r, w = rng.standard_normal(6), rng.standard_normal(3)
        m = (BT @ r) * (G @ w)
        z = np.array([m[0] + m[1] + m[2] + m[3] + m[4], (m[1] - m[2]) + 2 * (m[3] - m[4]), (m[1] + m[2]) + 4 * (m[3] + m[4]),
                      (m[1] - m[2]) + 8 * (m[3] - m[4]) + m[5]])
        ref = np.array([w @ r[o:o + 3] for o in range(4)])
        assert np.abs(z - ref).max() < 1e-12
    # dstep enters component j with the sum of its coefficients over the valid rows; for interior quads: (0, -6, 0, 0, 0, 0)
    assert np.allclose(BT.sum(1), [0, -6, 0, 0, 0, 0])


def test_norm_interp_f0_matches_the_reference_function(golden_dir):
    """pitch.norm_interp_f0 vs the REAL utils/pitch_utils.py:47-62 on float64 / float32 contours with leading, trailing and
    interior unvoiced runs, all-voiced, all-unvoiced and single-voiced-frame inputs: bit-exact (same numpy arithmetic)."""
    from stylesinger_amd import pitch
    g = torch.load(os.path.join(golden_dir, "norm_interp_f0.pt"), weights_only=False)
    hp = config.make_hparams()
    assert hp["pitch_norm"] == g["meta"]["pitch_norm"] and hp["use_uv"] == g["meta"]["use_uv"]
    for key, c in g["cases"].items():
        f0, uv = pitch.norm_interp_f0(c["hz"].numpy(), hp)
        assert f0.dtype == torch.float32 and uv.dtype == torch.float32
        assert torch.equal(uv, c["uv"]), key
        assert torch.equal(f0, c["f0"]), (key, (f0 - c["f0"]).abs().max().item())
        f0t, uvt = pitch.norm_interp_f0(c["hz"], hp)   # torch input, as the reference also accepts
        assert torch.equal(f0t, c["f0"]) and torch.equal(uvt, c["uv"]), key


def test_lds_swizzles_are_conflict_free_in_the_bank_model():
    """tools/lds_sim.py (lane groups / bank functions of MI355X_MICROARCH.md): the fragment reads and staging writes of the 16x16 kernels
    (128-byte fp32 rows with swz16, 64-byte bf16 rows with swz64) cost the conflict-free number of LDS cycles; the unswizzled reads do not
    (the model is not vacuous). On the GPU the fp32 form reads SQ_LDS_BANK_CONFLICT = 0 (profiles/r03_pmc_gate.json)."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lds_sim", os.path.join(root, "tools", "lds_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    assert sim.main() == 0
    c, ideal = sim.cycles("ds_read_b128", lambda lane: (lane & 15) * 128 + ((2 * (lane >> 4)) << 4))
    assert c > ideal


def test_forward_signature_equals_the_reference_operator_surface():
    """The drop-in boundary: StyleSingerHIP.forward has the parameters of the REAL StyleSinger.forward
    (/root/reference/modules/StyleSinger/stylesinger.py:119-121) - same names, order, defaults, **kwargs - and the vocoder plugin /
    entry-point surface keeps the reference's method names. Imports the unmodified reference (skipped where it is not mounted)."""
    import inspect
    from oracle import refimport
    if not refimport.available():
        pytest.skip("/root/reference is not mounted on this box")
    from stylesinger_amd.model import StyleSingerHIP
    from stylesinger_amd.vocoder import HifiGAN, REGISTERED_VOCODERS
    ref = refimport.load()["StyleSinger"]
    want, got = inspect.signature(ref.forward), inspect.signature(StyleSingerHIP.forward)
    assert [(p.name, p.kind, p.default) for p in want.parameters.values()] == [(p.name, p.kind, p.default) for p in got.parameters.values()]
    assert "HifiGAN_NSF" in REGISTERED_VOCODERS and REGISTERED_VOCODERS["HifiGAN_NSF"] is HifiGAN
    assert list(inspect.signature(HifiGAN.spec2wav).parameters)[:2] == ["self", "mel"]
    # every output the goldens recorded from the reference's returned dict is a key the HIP forward documents it returns (the GPU tests compare
    # the values: tests/test_gpu_parity.py::test_acoustic_hip_matches_reference_golden)
    import torch
    gold = torch.load(os.path.join(os.path.dirname(__file__), "golden", "acoustic_tiny_s4.pt"), weights_only=False)["out"]
    src = inspect.getsource(StyleSingerHIP.forward) + inspect.getsource(StyleSingerHIP)
    ALIAS = {"encoder_out": "encoder_out_text"}   # the reference overwrites ret['encoder_out'] later in forward; the stage value is kept under this name
    for k in gold:
        assert f'ret["{ALIAS.get(k, k)}"]' in src or f"'{ALIAS.get(k, k)}'" in src, k


def test_tuning_knob_table_keeps_its_keys_and_refuses_the_removed_ones():
    """ss_set_tuning / ss_get_tuning without a device: the surviving knobs round-trip, bad values and the keys removed with ABI 20 are refused."""
    l = lib.load()
    # knob table: every documented key round-trips, bad values are refused with a message
    for key, val in ((b"gate16_ks", 0), (b"mel_tail", 0), (b"gate16", 3), (b"skip_dense", 0), (b"voc_wino_max_mb", 7), (b"layer512_tail", 2)):
        before = l.ss_get_tuning(key)
        assert before >= 0
        assert l.ss_set_tuning(key, val) == 0 and l.ss_get_tuning(key) == val
        assert l.ss_set_tuning(key, before) == 0
    assert l.ss_set_tuning(b"gate16", 4) != 0 and b"gate16" in l.ss_last_error()
    # A/B switches removed with ABI 20: refused, and unknown to ss_get_tuning
    for key in (b"wave_prio", b"htile", b"wino_tn", b"wino_v1", b"res_tile", b"skip_tile", b"res16", b"skip16", b"e16"):
        assert l.ss_set_tuning(key, 0) != 0 and l.ss_set_tuning(key, 1) != 0 and l.ss_get_tuning(key) < 0
    assert l.ss_get_tuning(b"nope") < 0


def test_launch_planners_of_the_library_run_without_a_gpu():
    """The host-side launch planners of the C-ABI (no kernel launch): tiling picks, split-K slice count, size of the addend re-layout, the layer512
    size rule. Without a device the CU count falls back to MI355X's 256, so the BASELINE shapes give their documented answers."""
    l = lib.load()
    # fp32 F(4,3) gate tiling: C2 mel / f0 pair, one 4 s utterance (16-quad tiles), the C4 shape (32x32x2 kernel)
    assert l.ss_wino43_gate16_pick(8, 1500, 512, 2) == 2 and l.ss_wino43_gate16_pick(16, 1500, 384, 1) == 3
    assert l.ss_wino43_gate16_pick(1, 750, 512, 4) == 1 and l.ss_wino43_gate16_pick(32, 5625, 512, 4) == 0
    # addend in fetch order: [q tiles][n tiles][MT * 4096 floats]; C2 mel at d = 2: 375 quads -> 376 (groups of d) -> 12 tiles of 32 quads per item
    assert l.ss_gate16_tiled_floats(8, 1500, 512, 2, 2) == 8 * 12 * 8 * 2 * 4096
    assert l.ss_gate16_tiled_floats(8, 1500, 512, 2, 0) == -1 and l.ss_gate16_tiled_floats(8, 1500, 500, 2, 2) == -1
    # split-K of the skip GEMM: only for launches that leave CUs idle
    assert l.ss_gemm16_ksplit_pick(1, 750, 256, 5120) == 5 and l.ss_gemm16_ksplit_pick(8, 1500, 256, 5120) == 1 and l.ss_gemm16_ksplit_pick(1, 750, 256, 256) == 1
    # residual-projection row tile: 96 rows at C2 (16 row tiles per 8 s item), 32 rows for one short utterance
    assert l.ss_gemm16_pick(8, 1500, 256) == 6 and l.ss_gemm16_pick(1, 750, 256) == 2
    # round 6: the fused residual layer of the fp16x2 mel stack. Size rule = four rounds of 128-row tiles per CU (256 CUs without a device): the
    # BASELINE configs[3] shape qualifies (32 x 44 = 1408 tiles), C2's does not; the knob value 2 lifts the size rule (parity tests), never the shape rules
    assert l.ss_get_tuning(b"layer512") == 1 and l.ss_get_tuning(b"layer512_tail") == 1
    assert l.ss_layer512_ok(32, 5625, 256, 8, 20 * 256 * 2) == 1 and l.ss_layer512_ok(8, 1500, 256, 8, 20 * 256 * 2) == 0
    assert l.ss_layer512_ok(32, 5625, 192, 8, 20 * 192 * 2) == 0 and l.ss_layer512_ok(32, 5625, 256, 16, 20 * 256 * 2) == 0
    assert l.ss_set_tuning(b"layer512", 2) == 0 and l.ss_layer512_ok(1, 100, 256, 8, 512) == 1 and l.ss_layer512_ok(1, 100, 192, 8, 512) == 0
    assert l.ss_set_tuning(b"layer512", 1) == 0 and l.ss_set_tuning(b"layer512", 3) != 0
    # buffer sizes: 44 tiles per 30 s item; addend 128 x 512 floats, stream 128 x 256 fp32, H 128 x 256 fp16 per tile
    assert l.ss_layer512_addend_floats(32, 5625) == 1408 * 128 * 512 and l.ss_layer512_stream_bytes(32, 5625) == 1408 * 128 * 256 * 2
    assert l.ss_layer512_h_elems(32, 5625) == 1408 * 128 * 256 and l.ss_layer512_h_elems(1, 1) == 128 * 256


def _ws_net(mode, C_=256, L_=20, groups=1):
    """An ss_wavenet descriptor of one precision mode for the size query: placeholder non-null pointers (never dereferenced there)."""
    D = 0x1000
    n = lib.WaveNet()
    n.C, n.L, n.cond_dim, n.dil_cycle, n.in_dim, n.out_dim, n.steps, n.n_groups = C_, L_, 256, 4, 80, 80, 100, groups
    n.w_skipall, n.skipall_folded = D, 1
    if mode in ("fp32", "bf16x3"):
        n.wino_m, n.mfma_x3 = 4, int(mode == "bf16x3")
        for i in range(L_):
            n.w_dil_wino[i] = n.w_dil_wino16[i] = D
        return n
    n.mfma_bf16, n.w_skipall_h, n.w_cond_h = 1, D, D
    for i in range(L_):
        n.w_dil_h[i] = n.w_out_h[i] = D
    if mode != "bf16":
        n.mfma_split, n.mfma_products = 1 if mode == "bf16x2" else 2, 1 if mode == "fp16sd" else 2
    if mode in ("fp16x2", "fp16sd"):
        for i in range(L_):
            n.w_dil_f[i] = n.w_out_f[i] = D
    if mode == "fp16sd":
        n.n_wsets, n.n_esets, n.w_skipall_c = 32, 8, D
    if mode == "fp16q4":
        n.q_scale_gate = 1.0
        for i in range(L_):
            n.w_dil_q[i] = D
    return n


def test_workspace_bytes_of_every_stack_form_are_pinned():
    """ss_wavenet_workspace_bytes without a device (256 CUs) for every precision mode at a launch-bound, a mid and the fused-form shape, the f0
    pair, and every knob that changes the stack's form: the resolved form and the workspace layout stay what they were (integers recorded from
    the library before the form was resolved in one place)."""
    import ctypes
    l = lib.load()

    def ws(n, B, T):
        return l.ss_wavenet_workspace_bytes(ctypes.byref(n), B, T)
    want = {"fp32": (84946944, 1296236544, 11629494272), "bf16x3": (53489664, 792920064, 11629494272), "bf16": (42479616, 679673856, 9968549888),
            "bf16x2": (50343936, 805502976, 11814043648), "fp16x2": (50343936, 805502976, 17627348992), "fp16q4": (50343936, 805502976, 11814043648),
            "fp16sd": (50343936, 805502976, 39773274112)}
    for mode, sizes in want.items():
        assert tuple(ws(_ws_net(mode), B, T) for B, T in ((1, 768), (8, 1536), (32, 5632))) == sizes, mode
    assert ws(_ws_net("fp32", 192, 10, 2), 16, 1536) == 1000734720
    assert ws(_ws_net("fp32"), 0, 768) == -1

    def with_knob(key, val, n, B, T):
        before = l.ss_get_tuning(key)
        assert l.ss_set_tuning(key, val) == 0
        try:
            return ws(n, B, T)
        finally:
            assert l.ss_set_tuning(key, before) == 0
    assert with_knob(b"gate16", 0, _ws_net("fp32"), 8, 1536) == 792920064 and with_knob(b"gate16", 3, _ws_net("fp32"), 8, 1536) == 1296236544
    assert with_knob(b"gate16_ks", 0, _ws_net("fp32"), 1, 768) == 84946944
    assert with_knob(b"layer512", 0, _ws_net("fp16x2"), 32, 5632) == 11814043648 and with_knob(b"layer512", 0, _ws_net("fp16sd"), 32, 5632) == 11814043648
    assert with_knob(b"gate256", 0, _ws_net("fp16sd"), 32, 5632) == 41618767872
    no_esets = _ws_net("fp16sd")
    no_esets.n_esets = 0
    assert ws(no_esets, 32, 5632) == 17627348992
    assert with_knob(b"layer512", 2, _ws_net("fp16x2"), 1, 768) == 82980864 and with_knob(b"layer512", 2, _ws_net("fp16sd"), 1, 768) == 177352704


def test_every_sampler_entry_refuses_a_bad_net_or_workspace_before_any_launch():
    """What the six sampler entry points refuse of a net and a workspace, one table: a null workspace, too many layers, a channel count off the
    entry's own multiple (32 for the mel pair, 64 for the f0 pair; the DDIM and PLMS entries have no such row), a grouped net where the entry
    takes none (the f0 entries take a pair over an even item count only) and a workspace one byte short. Every pointer is a placeholder or a host
    array: each call returns before anything is launched."""
    import ctypes
    l = lib.load()
    P, B, T = 0x1000, 2, 8
    ts = np.array([3, 1, 0], np.int32)
    betas = np.linspace(1e-4, 0.06, 100)

    def mel_net(C_=256, groups=1):
        return _ws_net("fp32", C_, 20, groups)

    def f0_net(C_=256, groups=1):
        n = _ws_net("fp32", C_, 20, groups)
        n.in_dim, n.out_dim = 1, 3
        return n
    entries = {   # name: (net maker, call(net, B, ws, ws_bytes), C off the entry's multiple or None)
        "ss_meldiff_sample": (mel_net, lambda n, b, ws, nb: l.ss_meldiff_sample(n, P, P, None, b, T, None, 17, None, 0, 4, 1, ws, nb, None), 48),
        "ss_prodiff_sample": (mel_net, lambda n, b, ws, nb: l.ss_prodiff_sample(n, P, P, None, b, T, None, 17, None, 4, P, P, P, 1, ws, nb, None), 48),
        "ss_meldiff_sample_ddim": (mel_net, lambda n, b, ws, nb: l.ss_meldiff_sample_ddim(n, P, P, None, b, T, lib.hptr(ts), 3, P, 1.0, None, 17, None, 1, ws,
                                                                                         nb, None), None),
        "ss_meldiff_sample_plms": (mel_net, lambda n, b, ws, nb: l.ss_meldiff_sample_plms(n, P, P, None, b, T, 4, 1, P, 1, P, ws, nb, None), None),
        "ss_f0diff_sample": (f0_net, lambda n, b, ws, nb: l.ss_f0diff_sample(n, P, P, P, P, P, None, b, T, None, None, 17, None, 0, 4, 1, ws, nb, None), 96),
        "ss_f0diff_sample_strided": (f0_net, lambda n, b, ws, nb: l.ss_f0diff_sample_strided(n, P, P, P, P, P, None, b, T, lib.hptr(ts), 3, 0, 3, lib.hptr(betas),
                                                                                             1.0, None, None, 17, None, 1, ws, nb, None), 96),
    }
    for name, (make, call, bad_c) in entries.items():
        deep = make()
        deep.L = lib.SS_MAX_LAYERS + 1
        rows = {"null ws": (make(), B, None, 1 << 40), "too many layers": (deep, B, P, 1 << 40)}
        if bad_c is not None:
            rows["C=%d" % bad_c] = (make(C_=bad_c), B, P, 1 << 40)
        if make is mel_net:
            rows["grouped net"] = (make(groups=2), B, P, 1 << 40)
        else:
            rows["three groups"] = (make(groups=3), 3, P, 1 << 40)
            rows["pair over an odd item count"] = (make(groups=2), 3, P, 1 << 40)
        n = make()
        need = l.ss_wavenet_workspace_bytes(ctypes.byref(n), B, T)
        assert need > 0
        rows["workspace one byte short"] = (n, B, P, need - 1)
        for what, (net, b, ws, nb) in rows.items():
            rc = call(ctypes.byref(net), b, ws, nb)
            assert rc != 0 and l.ss_last_error().startswith(name.encode() + b": "), (name, what, rc, l.ss_last_error())


def test_gate128_index_math_against_a_tagged_lds_image(tmp_path):
    """gate128_kernel (the fp16x2 gate on 256 x 128 tiles, two workgroups per CU) takes all of its DMA / fragment / epilogue addresses from
    stylesinger_amd/csrc/gate128_layout.h; tools/layout_check_gate128.cpp compiles the SAME header on the host, replays every LDS-DMA piece
    into a tagged image and looks every access of the kernel up in it (coverage, right element, no bank conflicts, right output channel)."""
    exe = str(tmp_path / "layout_check_gate128")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "stylesinger_amd", "csrc"), os.path.join(ROOT, "tools", "layout_check_gate128.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-2000:]


def test_fp16q4_weight_pack_round_trips_through_the_kernel_side_decoder():
    """lib.pack_gate_q4 (the operand of ss_gemm_bf16_gate128q: hi plane fp16 of w * 2^8, lo plane as block-scaled fp4 in the kernel's lane
    order) against lib.unpack_gate_q4, which reads the pack the way the kernel addresses it (weight line of the pair's odd step, slots 4 + h
    and 6): every term lands where the kernel looks for it, the fp4 image is within half a grid step of lo, even lines carry nothing."""
    g = torch.Generator().manual_seed(5)
    Wp = torch.randn(64, 768, generator=g) * 0.05
    Wp[3] = 0.0                                   # an all-zero row: scale byte must not produce NaN / inf
    pack, lo_q = lib.pack_gate_q4(Wp, shift=8)
    assert pack.dtype == torch.float16 and pack.shape == (64, 1536)
    hi, lo_dec = lib.unpack_gate_q4(pack)
    ws = Wp * 256.0
    assert torch.equal(hi, ws.half().float())
    assert torch.equal(lo_dec, lo_q), "the decoder (kernel's view) and the packer's own dequantised values agree exactly"
    lo = ws - ws.half().float()
    blocks = lib.gate128q_kindex()
    for p in (0, 5, 11):
        for h in (0, 1):
            idx = blocks[p, h]
            amax = lo[:, idx].abs().amax(dim=1)
            err = (lo_q[:, idx] - lo[:, idx]).abs().amax(dim=1)
            assert bool((err <= 0.26 * amax + 1e-30).all())   # half the grid's largest step (4 -> 6) relative to a block maximum in [4, 8)
    wb = pack.view(torch.uint8).view(64, 24, 128)
    even_lines = [(S % 3) * 8 + S // 3 for S in range(0, 24, 2)]
    assert int(wb[:, even_lines, 64:].max()) == 0
    assert torch.isfinite(lo_dec).all() and float(lo_dec[3].abs().max()) == 0.0


def test_fp16q4_skip_weight_pack_round_trips_through_the_kernel_side_decoder():
    """lib.pack_skip_q4 (operand of ss_gemm_bf16_tile256q: pairs of consecutive 32-channel chunks) against lib.unpack_skip_q4, the kernel's view."""
    g = torch.Generator().manual_seed(6)
    Wp = torch.randn(32, 512, generator=g) * 0.03
    pack, lo_q = lib.pack_skip_q4(Wp, shift=8)
    hi, lo_dec = lib.unpack_skip_q4(pack)
    ws = Wp * 256.0
    assert torch.equal(hi, ws.half().float()) and torch.equal(lo_dec, lo_q)
    lo = ws - ws.half().float()
    tab = lib.tile256q_kindex(8)
    assert sorted(tab.reshape(-1).tolist()) == list(range(512))
    for p in (0, 7):
        for h in (0, 1):
            idx = tab[p, h]
            assert bool(((lo_q[:, idx] - lo[:, idx]).abs().amax(dim=1) <= 0.26 * lo[:, idx].abs().amax(dim=1) + 1e-30).all())
    wb = pack.view(torch.uint8).view(32, 16, 128)
    assert int(wb[:, 0::2, 64:].max()) == 0     # even chunks carry nothing in their second half


def test_speaker_encoder_partial_slicing_known_answers():
    """stylesinger_amd.speaker.compute_partial_slices = resemblyzer.VoiceEncoder.compute_partial_slices (un-vendored dependency of the reference,
    inference/StyleSinger.py:100-104): rate 1.3 partials per second -> one every round(16000 / 1.3 / 160) = 77 frames; hand-computed cases."""
    from stylesinger_amd import speaker
    w, m = speaker.compute_partial_slices(48000)                 # 3 s: n_frames 301, steps 219 -> starts 0, 77, 154; last coverage 0.9125
    assert [(s.start, s.stop) for s in m] == [(0, 160), (77, 237), (154, 314)]
    assert (w[-1].start, w[-1].stop) == (24640, 50240)
    _, m = speaker.compute_partial_slices(16000)                 # 1 s: a single (padded) partial
    assert [(s.start, s.stop) for s in m] == [(0, 160)]
    _, m = speaker.compute_partial_slices(16000 * 2 + 1000)      # n_frames 207, steps 125 -> starts 0, 77; last coverage (33000 - 12320) / 25600 = 0.81
    assert [(s.start, s.stop) for s in m] == [(0, 160), (77, 237)]
    _, m = speaker.compute_partial_slices(16000 * 2 - 2000)      # n_frames 188, steps 106 -> starts 0, 77; last coverage (30000 - 12320) / 25600 = 0.69 < 0.75: dropped
    assert [(s.start, s.stop) for s in m] == [(0, 160)]
    _, m = speaker.compute_partial_slices(16000 * 2 - 2000, min_coverage=0.5)
    assert len(m) == 2


def test_token_text_encoder_equals_the_reference_class(golden_dir, tmp_path):
    """`build_token_encoder(phone_set.json)` / `TokenTextEncoder` (utils/text/text_encoder.py:107-147,257-259; used at inference/StyleSinger.py:28,96
    and as the model's dictionary) - bit-exact against what the REAL class returned in the build container (tests/golden/token_encoder.json,
    `python -m oracle.gen_golden --round6`): example_run's phoneme list with ZH_checkpoint_phone_set.json, out-of-vocabulary and reserved
    tokens, whitespace, decode with padding / EOS stripping, the reversed form. Where /root/reference is mounted the two classes are also run
    side by side on random token strings."""
    import json
    import random
    from stylesinger_amd.text_encoder import TokenTextEncoder, build_token_encoder
    gold = json.load(open(os.path.join(golden_dir, "token_encoder.json")))
    pf = tmp_path / "phone_set.json"
    pf.write_text(json.dumps(gold["phone_set"]))
    enc = build_token_encoder(str(pf))
    assert len(enc) == enc.vocab_size == gold["vocab_size"] == 61
    assert (enc.pad(), enc.eos(), enc.unk(), enc.seg()) == (gold["pad"], gold["eos"], gold["unk"], gold["seg"])
    assert [enc.id_to_token[i] for i in range(len(enc))] == gold["id_to_token"]
    for case in gold["encode"]:
        assert enc.encode(case["s"]) == case["ids"], case["s"]
    assert enc.encode(" ".join(gold["example"]["ph"])) == gold["encode"][0]["ids"]       # what preprocess_input computes (inference/StyleSinger.py:96)
    d = gold["decode"]
    assert enc.decode(d[0]["ids"]) == d[0]["s"] and enc.decode(d[1]["ids"], strip_padding=True) == d[1]["s"]
    assert enc.decode(d[2]["ids"], strip_eos=True) == d[2]["s"] and enc.decode(d[3]["ids"]) == d[3]["s"]
    assert enc.sil_phonemes() == gold["sil"]
    rev = TokenTextEncoder(None, vocab_list=gold["phone_set"] + ["|"], replace_oov=None, reverse=True)
    r = gold["reverse"]
    assert (len(rev), rev.seg(), rev.encode("zh i uan"), rev.decode(rev.encode("zh i uan"))) == (r["vocab_size"], r["seg"], r["ids"], r["s"])
    with pytest.raises(KeyError):
        rev.encode("notaphone")
    vf = tmp_path / "vocab.txt"
    enc.store_to_file(str(vf))
    again = TokenTextEncoder(str(vf))
    assert again.token_to_id == enc.token_to_id
    from oracle import refimport
    if refimport.available():
        refimport.load()
        from utils.text.text_encoder import build_token_encoder as ref_build
        ref = ref_build(os.path.join(refimport.REF, "ZH_checkpoint_phone_set.json"))
        rng = random.Random(7)
        pool = gold["phone_set"] + ["<pad>", "<EOS>", "<UNK>", "|", "xx", "a1"]
        for _ in range(200):
            s_ = " ".join(rng.choice(pool) for _ in range(rng.randrange(0, 40)))
            ids = ref.encode(s_)
            assert enc.encode(s_) == ids
            assert enc.decode(ids) == ref.decode(ids)


def test_entry_point_host_logic_without_a_gpu(tmp_path, golden_dir):
    """Host-side contracts of the reference-shaped entry point (inference/StyleSinger.py:94-137,175-331) that need no device: the explicit opt-out
    of `trim_long_silences` (the reference always trims, audio.py:36-38), `loud_norm` refused instead of ignored (utils/audios/__init__.py:55-59
    is pyloudnorm), bytes paths, the example score shipped with the package, `save_wav` = utils/audio.py:12-17."""
    import json
    import wave
    import warnings
    import numpy as np
    from stylesinger_amd import audiofile, vadtrim, writer
    from stylesinger_amd.infer import StyleSingerInfer
    inf = StyleSingerInfer.__new__(StyleSingerInfer)       # no device: only the host helpers are exercised
    if not vadtrim.have_webrtcvad():
        with pytest.raises(ImportError, match="vad_flags=False"):
            inf._resolve_vad(None)
    else:
        assert inf._resolve_vad(None) == "webrtc"
    StyleSingerInfer._warned_untrimmed = False
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert inf._resolve_vad(False) is None and inf._resolve_vad(False) is None
    assert len([x for x in w if "trim_long_silences skipped" in str(x.message)]) == 1, "warns once"
    f = inf._resolve_vad([1, 0, 1])
    assert f.shape == (1, 3)
    with pytest.raises(NotImplementedError, match="loud_norm"):
        StyleSingerInfer(dict(loud_norm=True), device="cuda")      # refused before anything touches a device
    # a bytes path reaches wave.open as a path, not as "b'...'"
    p = tmp_path / "a.wav"
    pcm = (np.arange(-500, 500) * 30).astype("<i2")
    with wave.open(str(p), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(48000)
        wf.writeframes(pcm.tobytes())
    a = audiofile.load_pcm16(str(p), 48000)
    b = audiofile.load_pcm16(os.fsencode(str(p)), 48000)
    assert np.array_equal(a, b) and np.array_equal(a, pcm.astype(np.float32) / 32768.0)
    with pytest.raises(ValueError, match="16-bit PCM at 44100"):
        audiofile.load_pcm16(str(p), 44100)
    # the example score = the reference's example_run input (fixture generated from the reference by oracle/gen_golden.py --round6)
    gold = json.load(open(os.path.join(golden_dir, "token_encoder.json")))
    ex = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stylesinger_amd", "example_input.json")))
    for k in ("name", "ph", "note", "note_dur", "note_type"):
        assert ex[k] == gold["example"][k], k
    # save_wav: wav * 32767 truncated toward zero, as numpy's astype(int16) does in the reference
    x = np.array([0.0, 0.5, -0.5, 0.99999, -1.0, 1e-5], dtype=np.float32)
    writer.save_wav(x, str(tmp_path / "o.wav"), 48000)
    with wave.open(str(tmp_path / "o.wav"), "rb") as wf:
        got = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2")
    assert np.array_equal(got, (x * 32767).astype(np.int16)) and x[1] == 0.5, "input not modified"


def test_as_waveform_is_the_one_audio_argument_rule(tmp_path):
    """`audiofile.as_waveform`: what `inp['ref_audio']` / `inp['pitch_audio']` may be - a path (str / bytes / PathLike), a `(waveform, sample_rate)`
    pair, or (where the key has a default rate) a bare array. Anything that is not a path or a well-formed pair takes the bare-array branch, as
    the intake always did: a 2-D array comes back as it is, a pair with a non-scalar rate is what numpy makes of it (a ragged-array ValueError)."""
    import pathlib
    import wave
    from stylesinger_amd import audiofile
    p = tmp_path / "a.wav"
    pcm = (np.arange(-500, 500) * 30).astype("<i2")
    with wave.open(str(p), "wb") as wf:
        wf.setnchannels(1)
        wf.setsampwidth(2)
        wf.setframerate(48000)
        wf.writeframes(pcm.tobytes())
    want = pcm.astype(np.float32) / 32768.0
    for what, default_sr in (("ref_audio", 44100), ("pitch_audio", None)):
        for arg in (str(p), os.fsencode(str(p)), pathlib.Path(p)):
            wav, sr, path = audiofile.as_waveform(arg, default_sr, what)
            assert wav.dtype == np.float32 and np.array_equal(wav, want) and sr == 48000 and path == str(p), (what, type(arg))
        for pair in ((want.astype(np.float64), 44100), [want, np.int64(44100)]):
            wav, sr, path = audiofile.as_waveform(pair, default_sr, what)
            assert wav.dtype == np.float32 and np.array_equal(wav, want) and sr == 44100 and type(sr) is int and path is None
    wav, sr, path = audiofile.as_waveform(want.tolist(), 32000, "ref_audio")
    assert wav.dtype == np.float32 and np.array_equal(wav, want) and sr == 32000 and path is None
    two_d = np.stack([want, want])
    wav, sr, path = audiofile.as_waveform(two_d, 32000, "ref_audio")
    assert wav.shape == (2, 1000) and sr == 32000 and path is None
    with pytest.raises(ValueError, match="inhomogeneous|sequence"):
        audiofile.as_waveform((want, [44100]), 32000, "ref_audio")
    with pytest.raises(ValueError, match="inhomogeneous|sequence"):
        audiofile.as_waveform((two_d, 44100), 32000, "ref_audio")
    for bad in (want, two_d, (want, [44100]), (two_d, 44100)):
        with pytest.raises(ValueError, match=r"preprocess_input: inp\['pitch_audio'\] must be a WAV path or a \(waveform, sample_rate\) pair"):
            audiofile.as_waveform(bad, None, "pitch_audio")


def test_from_checkpoints_forwards_the_constructor_keywords(monkeypatch):
    """`from_checkpoints(hparams, exp_dir, vocoder_dir, **ctor)`: the form `example_run`'s docstring advertises (`emotion_state`, `speaker_state`,
    `phone_set` next to the two directories) reaches the constructor; a missing model checkpoint is still the reference's FileNotFoundError."""
    from stylesinger_amd import ckpt
    from stylesinger_amd.infer import StyleSingerInfer
    model, voc, vcfg, emo, spk = (object() for _ in range(5))
    asked = []
    monkeypatch.setattr(ckpt, "read_state", lambda d, name: (asked.append((d, name)), (model if d == "exp" else None, None))[1])
    monkeypatch.setattr(ckpt, "load_vocoder_ckpt", lambda d: (asked.append(d), (voc, vcfg))[1])

    class Recorder(StyleSingerInfer):
        def __init__(self, hparams=None, **kw):
            self.seen = dict(kw, hparams=hparams)
    hp = dict(seed=3)
    ins = Recorder.from_checkpoints(hp, "exp", "voc", emotion_state=emo, speaker_state=spk, phone_set="ps.json", loudness="bs1770", device="cuda:1")
    assert type(ins) is Recorder and asked == [("exp", "model"), "voc"]
    assert ins.seen == dict(hparams=hp, model_state=model, vocoder_state=voc, vocoder_config=vcfg, emotion_state=emo, speaker_state=spk,
                            phone_set="ps.json", loudness="bs1770", device="cuda:1")
    for k, v in dict(model_state=model, vocoder_state=voc, vocoder_config=vcfg, emotion_state=emo, speaker_state=spk).items():
        assert ins.seen[k] is v, k
    with pytest.raises(FileNotFoundError, match=r"\| ckpt not found in nowhere\."):
        Recorder.from_checkpoints(hp, "nowhere", "voc")
