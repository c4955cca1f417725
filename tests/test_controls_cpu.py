"""Every render control of `controls.CONTROLS` at every layer that has to carry it: its flag in the command line's parser, its input-dict key through
`_pitch_inputs` and `plan_song` into the batch form, its batch key from `infer_batch` to the model, and its field in `controls.resolve` (from the
keyword and from its hparams default). A control added to the table without a sample below, or not carried by a layer, fails here. No device."""
import argparse
import dataclasses
import types

import numpy as np
import pytest
import torch

from stylesinger_amd import config, controls, infer, producers, song

HP = config.make_hparams(dict(timesteps=8, K_step=8, f0_timesteps=4))
BASE = ["--exp-dir", "e", "--vocoder-dir", "v", "--emotion-ckpt", "x", "--speaker-ckpt", "y", "--phone-set", "z"]
HZ = (torch.full((1, 8), 220.0), [8])
POOL = dict(ref_mels=torch.zeros(1, 2, 8, 80), ref_f0=torch.zeros(1, 2, 8))
# forward kwarg -> (the other arguments the call needs, a value, where `resolve` puts it, what stands there)
FIELDS = dict(
    pitch_hz=({}, HZ, lambda c: c.pitch_hz, HZ), pitch_shift=(dict(pitch_hz=HZ), 2.0, lambda c: c.pitch_shift, 2.0),
    pitch_align=(dict(pitch_hz=HZ), "dtw", lambda c: c.align, "dtw"), pitch_align_band=(dict(pitch_hz=HZ, pitch_align="dtw"), 4, lambda c: c.align_band, 4),
    pitch_timing=(dict(pitch_hz=HZ), "guide", lambda c: c.timing, "guide"),
    pitch_correct=({}, 0.5, lambda c: c.edit["alpha"], 0.5), vibrato_scale=({}, 2.0, lambda c: c.edit["kappa"], 2.0),
    vibrato_add=({}, (5.5, 30.0), lambda c: c.edit["vibrato"][:2], (5.5, 30.0)), pitch_smooth_ms=(dict(pitch_correct=0.5), 100.0, lambda c: c.edit["W"], 9),
    f0_steps=({}, 2, lambda c: c.f0_ts, [1, 0]), f0_eta=({}, 0.25, lambda c: c.f0_eta, 0.25),
    sampler=(dict(mel_steps=4), "ddim", lambda c: c.mel.name, "ddim"), mel_steps=(dict(sampler="dpmpp"), 5, lambda c: c.mel.steps, 5),
    ddim_steps=(dict(sampler="ddim"), 3, lambda c: c.mel.steps, 3), mel_order=(dict(sampler="dpmpp", mel_steps=4), 1, lambda c: c.mel.order, 1),
    mel_spacing=(dict(sampler="ddim", mel_steps=4), "logsnr", lambda c: c.mel.spacing, "logsnr"),
    eta=(dict(sampler="ddim", mel_steps=4), 0.5, lambda c: c.mel.eta, 0.5), plms_interval=(dict(sampler="plms"), 3, lambda c: c.mel.interval, 3),
    ref_weights=({}, [1.0, 3.0], lambda c: c.ref_weights, [1.0, 3.0]), style_cache=({}, {"sty": 0}, lambda c: c.style_cache, {"sty": 0}),
    plan_slot=({}, 2, lambda c: c.plan_slot, 2), noise=({}, {"mel": 0}, lambda c: c.noise, {"mel": 0}), seed=({}, 77, lambda c: c.seed, 77))
# input-dict key -> a value `_pitch_inputs` and `plan_song` accept, and the other keys it needs
INPUTS = dict(pitch_hz=(np.full(100, 220.0), ()), pitch_shift=(1.0, ()), pitch_align=("dtw", ()), pitch_align_band_s=(0.5, ("pitch_align",)), pitch_timing=("guide", ()),
              pitch_correct=(0.8, ()), vibrato_scale=(0.5, ()), vibrato_add=((5.5, 30.0), ()), pitch_smooth_ms=(250.0, ("pitch_correct",)))
KEYED = [c for c in controls.CONTROLS if c.key]
ids = lambda cs: [c.flag or c.key for c in cs]


def _resolve(kw, hp=HP, **tensors):
    return controls.resolve(kw, hp, lambda n: list(range(n))[::-1], **tensors)


def test_the_key_lists_come_from_the_table():
    assert controls.CONTOUR_KEYS == ("pitch_hz", "pitch_audio", "pitch_shift", "pitch_align", "pitch_align_band_s", "pitch_timing")
    assert controls.EDIT_KEYS == ("pitch_correct", "vibrato_scale", "vibrato_add", "pitch_smooth_ms")
    assert not set(controls.EDIT_KEYS) & set(controls.CONTOUR_KEYS)
    assert set(controls.BATCH_KEYS) == {c.key for c in KEYED if c.group in ("contour", "edit")} | {"ref_weights", "style_cache"}
    assert {c.key for c in KEYED} == set(FIELDS), "a control without a sample in this file (or a sample without a control)"
    assert {c.inp for c in controls.CONTROLS if c.inp and c.group != "call"} == set(INPUTS) | {"pitch_audio"}
    for c in controls.CONTROLS:   # an hparams default is a key of the defaults; the edit group's are its own names
        if c.hp or (c.group == "edit" and c.key):
            assert (c.hp or c.key) in config.DEFAULT_HPARAMS, c


@pytest.fixture(scope="module")
def parser():
    class Parsed(Exception):
        pass

    def stop(self, argv=None):
        raise Parsed(self)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(argparse.ArgumentParser, "parse_args", stop)
        with pytest.raises(Parsed) as e:
            infer.main([])
    return e.value.args[0]


def _argv(c):
    """The flag with a value it accepts, after the flags it needs: its owner, a contour for the contour group."""
    a = c.arg
    val = [str(a["choices"][0])] if a.get("choices") else ["5.5", "30"] if a.get("nargs") == 2 else ["c.npy"] if "type" not in a else ["3"] if a["type"] is int else ["0.5"]
    need = []
    if c.group == "contour" and c.inp not in ("pitch_hz", "pitch_audio"):
        need += ["--pitch-npy", "c.npy"] + (["--pitch-align", "dtw"] if c.inp == "pitch_align_band_s" else [])
    if c.owner:
        need += [c.owner[0]] + ([c.owner[1][0]] if c.owner[1] else ["5.5", "30"] if c.owner[0] == "--vibrato-add" else ["3"])
    if c.flag != "--mel-steps" and (c.owner or (None, None))[1] and c.owner[1][0] in ("ddim", "dpmpp"):
        need += ["--mel-steps", "4"]
    return need + [c.flag] + val


@pytest.mark.parametrize("c", [c for c in controls.CONTROLS if c.flag], ids=ids([c for c in controls.CONTROLS if c.flag]))
def test_the_parser_has_the_flag_and_it_lands_under_its_key(parser, c):
    assert c.flag in {s for act in parser._actions for s in act.option_strings}
    a = parser.parse_args(BASE + _argv(c))
    got = getattr(a, c.flag[2:].replace("-", "_"))
    assert got is not None
    pitch, hp = controls.from_flags(a, config.DEFAULT_HPARAMS)
    if c.inp:
        assert pitch[c.inp] == (tuple(got) + (None, None) if c.inp == "vibrato_add" else got) and c.hp is None
    elif c.hp:
        assert hp[c.hp] == got
    else:   # the two times of --vibrato-add travel inside its tuple
        assert got in pitch["vibrato_add"][2:]
    for k in pitch:
        assert k in controls.CONTOUR_KEYS + controls.EDIT_KEYS
    for k in hp:
        assert k in config.DEFAULT_HPARAMS


@pytest.mark.parametrize("c", [c for c in controls.CONTROLS if c.inp in INPUTS], ids=ids([c for c in controls.CONTROLS if c.inp in INPUTS]))
def test_the_input_key_reaches_the_batch_form(c):
    """(`pitch_audio` is tracked on the device into the same `pitch_hz`: tests/test_gpu_pitch_given.py.)"""
    inp = {k: INPUTS[k][0] for k in (c.inp, *INPUTS[c.inp][1])}
    if c.group == "contour":
        inp.setdefault("pitch_hz", INPUTS["pitch_hz"][0])
    me = types.SimpleNamespace(hparams=HP, device=torch.device("cpu"))
    assert c.key in producers.ReferenceProducers._pitch_inputs(me, dict(inp))
    n = 8
    score = dict(ph_token=list(range(1, n + 1)), note=[60, 62, 0, 64, 65, 0, 67, 69], note_dur=[0.3] * n, note_type=[2, 2, 1, 2, 2, 1, 2, 2], ph_dur=[0.3] * n)
    plan = song.plan_song(dict(score, **inp), sr=48000, hop=256, max_seconds=1.0, segment_batch=2)
    assert len(plan.batches) >= 2 and all(c.key in b for b in plan.batches)
    assert c.key in controls.BATCH_KEYS


def test_infer_batch_hands_every_batch_key_to_the_model():
    seen = {}

    def model(txt, **kw):
        seen.update(kw)
        return dict(mel_out=0, f0_denorm=0, lens=0)
    me = types.SimpleNamespace(hparams=HP, model=model)
    batch = dict(txt_tokens=0, spk_embed=0, emo_embed=0, ref_mels=0, ref_f0=0, note=0, note_dur=0, note_type=0, **{k: object() for k in controls.BATCH_KEYS})
    noise = {"mel": 0}
    infer.StyleSingerInfer.infer_batch(me, batch, noise=noise, seed=5, vocode=False, plan_slot=2)
    for k in controls.BATCH_KEYS:
        assert seen[k] is batch[k], k
    assert seen["noise"] is noise and seen["seed"] == 5 and seen["plan_slot"] == 2
    seen.clear()
    infer.StyleSingerInfer.infer_batch(me, {k: v for k, v in batch.items() if k not in controls.BATCH_KEYS}, vocode=False)
    assert not set(controls.BATCH_KEYS) & set(seen) and seen["seed"] == HP["seed"]      # an absent control is not passed on at all


@pytest.mark.parametrize("c", KEYED, ids=ids(KEYED))
def test_resolve_places_the_control_in_its_field(c):
    ctx, val, field, want = FIELDS[c.key]
    tensors = POOL if c.key == "ref_weights" else {}
    ctl = _resolve(dict(ctx, **{c.key: val}), **tensors)
    assert field(ctl) == want
    with pytest.raises(dataclasses.FrozenInstanceError):
        ctl.seed = 0
    hp_key = c.hp or (c.key if c.group == "edit" else None)
    if hp_key:   # the same value as an hparams default lands in the same field, and an explicit keyword wins over it
        assert field(_resolve(dict(ctx), dict(HP, **{hp_key: val}))) == want
        other = dict(HP, **{hp_key: {"sampler": "dpmpp", "mel_spacing": "uniform", "vibrato_add": (4.0, 10.0)}.get(c.key, 1)})
        assert field(_resolve(dict(ctx, **{c.key: val}), other)) == want
