"""The render controls of `StyleSingerHIP.forward` in one place: their names at every layer (forward kwarg, input-dict key, hparams default,
command-line flag), their dependency and value rules, and "explicit > hparams > neutral". Host only: no device, no tensor data, no `lib`.

`resolve` is what forward reads (an immutable namespace, `c.ctl` in the stages), `from_input` maps the reference's input dict to the batch form
`infer_batch` takes (`_pitch_inputs`, `plan_song`), `add_flags` / `from_flags` are the command line's. A new control is one row of CONTROLS, its
rule in `check_contour` or a resolver, and its field in `resolve`; tests/test_controls_cpu.py fails where a layer does not carry it."""
import collections
import dataclasses
import math
import types

from .abi import DEFINES

Control = collections.namedtuple("Control", "group key inp hp flag owner arg")


def _c(group, key=None, inp=None, hp=None, flag=None, owner=None, **arg):
    """One control: forward kwarg, input-dict key, hparams default, flag (+ argparse keywords), owner = (the flag it belongs to, its values | None)."""
    return Control(group, key, inp, hp, flag, owner, arg)


_STRIDED = ("ddim", "dpmpp")
CONTROLS = (
    _c("contour", "pitch_hz", "pitch_hz", flag="--pitch-npy", help="sing on this contour: a .npy file holding a 1-D array of Hz at the mel hop, 0 = unvoiced"),
    _c("contour", "pitch_hz", "pitch_audio", flag="--pitch-audio",
       help="sing on the pitch of this guide vocal (a WAV file, tracked on the device, 80-800 Hz) instead of the predicted f0"),
    _c("contour", "pitch_shift", "pitch_shift", flag="--pitch-shift", type=float, help="transpose the given contour by this many semitones"),
    _c("contour", "pitch_align", "pitch_align", flag="--pitch-align", choices=["dtw"], help="warp the given contour onto the score's notes by dynamic "
       "time warping (a guide vocal with a timing of its own) instead of scaling it linearly"),
    _c("contour", "pitch_align_band", "pitch_align_band_s", flag="--pitch-align-band-s", type=float,
       help="--pitch-align: half-width of the band around the linear fit, seconds (default 2.0; 0 = full)"),
    _c("contour", "pitch_timing", "pitch_timing", flag="--pitch-timing", choices=["guide"], help="sing in the given contour's timing instead of the "
       "score's: note onsets where the guide has them, as many frames as the contour has (pitch-only alignment: no timing information inside a held or "
       "repeated note)"),
    _c("edit", "pitch_correct", "pitch_correct", flag="--pitch-correct", type=float, metavar="A", help="pull the pitch trend toward the score's notes: "
       "0 = as sung ... 1 = on the notes (with or without a given contour; this project's own trend / vibrato split, rendered quality unassessed)"),
    _c("edit", "vibrato_scale", "vibrato_scale", flag="--vibrato-scale", type=float, metavar="K",
       help="scale what rides on the pitch trend: 0 = flat, 1 = as sung, 2 = twice the vibrato"),
    _c("edit", "vibrato_add", "vibrato_add", flag="--vibrato-add", type=float, nargs=2, metavar=("RATE_HZ", "DEPTH_CENTS"),
       help="put a synthetic vibrato on held notes"),
    _c("edit", flag="--vibrato-delay-ms", owner=("--vibrato-add", None), type=float, metavar="MS",
       help="--vibrato-add: onset after the start of a held note (default 250)"),
    _c("edit", flag="--vibrato-fade-ms", owner=("--vibrato-add", None), type=float, metavar="MS", help="--vibrato-add: fade in and out (default 150)"),
    _c("edit", "pitch_smooth_ms", "pitch_smooth_ms", flag="--pitch-smooth-ms", type=float, metavar="MS",
       help="length of the window that defines the pitch trend (default 333)"),
    _c("f0", "f0_steps", hp="f0_sample_steps", flag="--f0-steps", type=int, help="sample the two f0 / uv diffusions at this many of their f0_timesteps "
       "network times (hparams['f0_sample_steps']; default: every one, the reference's loop)"),
    _c("f0", "f0_eta", hp="f0_sample_eta", flag="--f0-eta", owner=("--f0-steps", None), type=float,
       help="--f0-steps: 0 = deterministic Gaussian half ... 1 = ancestral (hparams['f0_sample_eta'], default 1)"),
    _c("mel", "sampler", hp="mel_sampler", flag="--mel-sampler", choices=["ddpm", "ddim", "plms", "dpmpp"], help="how the shallow mel diffusion is "
       "sampled (hparams['mel_sampler']): ddpm = the reference's ancestral loop, plms = its PLMS sampler (stride: hparams['pndm_speedup']), ddim / "
       "dpmpp = --mel-steps network times, first order / DPM-Solver++ multistep (default: the checkpoint's own choice)"),
    _c("mel", "mel_steps", hp="mel_sample_steps", flag="--mel-steps", owner=("--mel-sampler", _STRIDED), type=int,
       help="--mel-sampler ddim | dpmpp: at most this many network times (hparams['mel_sample_steps'])"),
    _c("mel", "ddim_steps"),
    _c("mel", "mel_order", hp="mel_sample_order", flag="--mel-order", owner=("--mel-sampler", ("dpmpp",)), type=int, choices=[1, 2],
       help="--mel-sampler dpmpp: 2 = the 2M multistep update (default), 1 = first order"),
    _c("mel", "mel_spacing", hp="mel_sample_spacing", flag="--mel-spacing", owner=("--mel-sampler", _STRIDED), choices=["uniform", "logsnr"],
       help="--mel-steps: the times uniform in t or in the log-SNR (hparams['mel_sample_spacing']; default: uniform for ddim, logsnr for dpmpp)"),
    _c("mel", "eta", hp="mel_sample_eta", flag="--mel-eta", owner=("--mel-sampler", ("ddim",)), type=float,
       help="--mel-sampler ddim: 0 = deterministic (default) ... 1 = ancestral (hparams['mel_sample_eta'])"),
    _c("mel", "plms_interval", hp="pndm_speedup"),
    _c("call", "ref_weights", "ref_weights"), _c("call", "style_cache"), _c("call", "plan_slot"), _c("call", "noise"), _c("call", "seed", hp="seed"),
)
CONTOUR_KEYS = tuple(c.inp for c in CONTROLS if c.group == "contour")                   # the input-dict form: what needs ph_dur in a song
EDIT_KEYS = tuple(c.key for c in CONTROLS if c.group == "edit" and c.key)               # the same at every layer; no contour, no ph_dur
BATCH_KEYS = tuple(dict.fromkeys(c.key for c in CONTROLS if c.group in ("contour", "edit") and c.key)) + ("ref_weights", "style_cache")   # infer_batch -> forward

ALIGN_BAND_S = 2.0   # default half-width of the pitch_align band, seconds around the linear fit
EDIT_SMOOTH_MS = 333.0   # default pitch_smooth_ms: at 187.5 frames/s (W = 31) the window passes 1 Hz and drops 5-7 Hz
EDIT_MAX_W = DEFINES["SS_PITCH_EDIT_MAX_W"]   # the widest half-window the kernel's LDS halo holds
VIBRATO_DELAY_MS, VIBRATO_FADE_MS = 250.0, 150.0
MEL_SAMPLERS = ("ddpm", "ddim", "plms", "dpmpp")
MEL_SPACINGS = ("uniform", "logsnr")
MEL_SPACING_DEFAULT = {"ddim": "uniform", "dpmpp": "logsnr"}   # each strided sampler's own default


def given(**kw):
    """The keywords that have a value: an absent control is not passed on at all."""
    return {k: v for k, v in kw.items() if v is not None}


def pick(kwargs, hp, key, hp_key=None, neutral=None):
    """Explicit > hparams > neutral, for every group: kwargs[key] where given (not None), else hp[hp_key or key], else `neutral`."""
    v = kwargs.get(key)
    if v is None:
        v = hp.get(hp_key or key)
    return neutral if v is None else v


# ---- the contour rules, once; a layer supplies the spelling -----------------------------------------------------------------------------------
# prefix; how a key / a name after "needs" is spelled; the contour; its frames; what needs one needs; the "needs" sentence; key and value; the band's key, unit; two sources
Layer = collections.namedtuple("Layer", "prefix key bare contour frames need needs eq band_key band_unit both")
FORWARD = Layer("forward: ", str, str, "the pitch_hz contour", "the pitch_hz contour's frames", "pitch_hz", "{k} {what}; it needs {need}", "{}={}",
                "pitch_align_band", "guide frames >= 0 (0 or None = the full matrix)",
                "give either pitch_hz (a contour in Hz to fit) or f0 / uv (the normalised contour), not both")
INPUT = FORWARD._replace(prefix="preprocess_input: ", key="inp['{}']".format, contour="inp['pitch_hz'] / inp['pitch_audio']",
                         frames="the frames of inp['pitch_hz'] / inp['pitch_audio']", need="one of them", eq="{} = {}", band_key="pitch_align_band_s",
                         band_unit="seconds >= 0 (0 = the full matrix)", both="give inp['pitch_hz'] or inp['pitch_audio'], not both")
PLAN = INPUT._replace(prefix="plan_song: ")
_flag = lambda k: "--" + k.replace("_", "-")
FLAGS = INPUT._replace(prefix="", key=_flag, bare=_flag, need="--pitch-audio or --pitch-npy", needs="{k} needs {need}", eq="{}={}",
                       band_unit="seconds >= 0 (0 = full)", both="--pitch-audio and --pitch-npy exclude each other")


def check_contour(v, has, both, shift, align, band, timing, note=""):
    """The dependency and value rules of the contour group in layer `v`'s words. has: a contour that can be fitted is given; both: two contour
    sources are; band: already a number (int frames in forward, float seconds elsewhere). ValueError on the first rule broken."""
    def needs(k, what, need=v.need, note=note):
        return ValueError(v.prefix + v.needs.format(k=v.key(k), what=what, need=need) + note)
    if both:
        raise ValueError(v.prefix + v.both)
    if shift is not None and not has:
        raise needs("pitch_shift", "transposes " + v.contour, note="")
    if align is not None and align != "dtw":
        raise ValueError(v.prefix + v.eq.format(v.key("pitch_align"), repr(align)) + ": None (the linear fit) or 'dtw'")
    if align is not None and not has:
        raise needs("pitch_align", f"warps {v.contour} onto the score")
    if band is not None and align is None and timing is None:   # pitch_timing aligns too
        raise needs(v.band_key, "is the band of " + v.eq.format(v.key("pitch_align"), "'dtw'"), v.bare("pitch_align"), "")
    if band is not None and not band >= 0:
        raise ValueError(v.prefix + v.eq.format(v.key(v.band_key), band) + ": " + v.band_unit)
    if timing is not None and timing != "guide":
        raise ValueError(v.prefix + v.eq.format(v.key("pitch_timing"), repr(timing)) + ": None (the score's timing) or 'guide'")
    if timing is not None and not has:
        raise needs("pitch_timing", "lays the score out on " + v.frames)


# ---- the resolvers: explicit > hparams > neutral, checked; no device ---------------------------------------------------------------------------
def edit_fps(hparams):
    return float(hparams["audio_sample_rate"]) / float(hparams["hop_size"])


def edit_window_frames(smooth_ms, hparams):
    """Half-width W of the trend window in frames: max(1, round(smooth_ms * 1e-3 * fps / 2)), fps = audio_sample_rate / hop_size."""
    smooth_ms = float(smooth_ms)
    if not smooth_ms >= 0 or not math.isfinite(smooth_ms):
        raise ValueError(f"pitch_smooth_ms={smooth_ms}: milliseconds >= 0")
    return max(1, int(round(smooth_ms * 1e-3 * edit_fps(hparams) / 2)))


def resolve_pitch_edit(kwargs, hparams):
    """The pitch edit a call asks for: kwargs['pitch_correct' | 'vibrato_scale' | 'vibrato_add' | 'pitch_smooth_ms'] where given (not None), else the
    same keys of hparams, else neutral. vibrato_add = (rate_hz, depth_cents[, delay_ms = 250[, fade_ms = 150]]).
    -> None for a neutral edit (pitch_correct 0, vibrato_scale 1, no vibrato_add or depth 0), else dict(W, alpha, kappa, vibrato = None |
    (rate_hz, depth_cents, delay_frames, fade_frames), fps). ValueError on pitch_correct outside [0, 1], vibrato_scale < 0, a rate outside
    (0, fps / 4], a depth outside [0, 1200], negative times, a window beyond EDIT_MAX_W."""
    alpha, kappa = float(pick(kwargs, hparams, "pitch_correct", neutral=0.0)), float(pick(kwargs, hparams, "vibrato_scale", neutral=1.0))
    vib, ms = pick(kwargs, hparams, "vibrato_add"), pick(kwargs, hparams, "pitch_smooth_ms")
    fps = edit_fps(hparams)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"pitch_correct={alpha}: inside [0, 1] (0 = as sung, 1 = the score's notes)")
    if not (kappa >= 0.0 and math.isfinite(kappa)):
        raise ValueError(f"vibrato_scale={kappa}: >= 0 (0 = flat, 1 = as sung)")
    W = edit_window_frames(EDIT_SMOOTH_MS if ms is None else ms, hparams)
    if W > EDIT_MAX_W:
        raise ValueError(f"pitch_smooth_ms={ms}: a half-window of {W} frames exceeds the kernel's cap of {EDIT_MAX_W} (refused, never truncated)")
    vibrato = None
    if vib is not None:
        if not isinstance(vib, (tuple, list)) or not 2 <= len(vib) <= 4:
            raise ValueError(f"vibrato_add={vib!r}: (rate_hz, depth_cents[, delay_ms[, fade_ms]])")
        rate, depth = float(vib[0]), float(vib[1])
        delay_ms = VIBRATO_DELAY_MS if len(vib) < 3 or vib[2] is None else float(vib[2])
        fade_ms = VIBRATO_FADE_MS if len(vib) < 4 or vib[3] is None else float(vib[3])
        if not 0.0 < rate <= fps / 4:
            raise ValueError(f"vibrato_add: rate {rate} Hz outside (0, fps / 4 = {fps / 4:g}]")
        if not 0.0 <= depth <= 1200.0:
            raise ValueError(f"vibrato_add: depth {depth} cents outside [0, 1200]")
        if not (delay_ms >= 0.0 and fade_ms >= 0.0 and math.isfinite(delay_ms) and math.isfinite(fade_ms)):
            raise ValueError(f"vibrato_add: delay {delay_ms} ms / fade {fade_ms} ms: times >= 0")
        if depth > 0.0:
            vibrato = (rate, depth, int(round(delay_ms * 1e-3 * fps)), max(1, int(round(fade_ms * 1e-3 * fps))))
    if alpha == 0.0 and kappa == 1.0 and vibrato is None:
        return None
    return dict(W=W, alpha=alpha, kappa=kappa, vibrato=vibrato, fps=fps)


def f0_sampler(kwargs, hp, contour_given, times):
    """(network times or None, eta) of the f0 pair loop: forward(f0_steps=, f0_eta=), else hparams['f0_sample_steps'] / ['f0_sample_eta'];
    None = the reference's full ancestral loop (ss_f0diff_sample). times(n): the n network times (`Plans.f0_strided_timesteps`)."""
    if kwargs.get("f0_steps") is not None and contour_given:
        raise ValueError("forward: f0_steps chooses how the f0 / uv diffusions are sampled; with a given contour (f0 / uv or pitch_hz) they do not run")
    if contour_given:   # the hparams defaults are simply unused
        return None, 1.0
    steps, eta = pick(kwargs, hp, "f0_steps", "f0_sample_steps"), float(pick(kwargs, hp, "f0_eta", "f0_sample_eta", 1.0))
    if steps is not None and int(steps) < 1:
        raise ValueError(f"forward: f0_steps={steps}: at least 1 (more than f0_timesteps = {hp['f0_timesteps']} means all of them)")
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"forward: f0_eta={eta}: 0 (deterministic Gaussian half) ... 1 (ancestral)")
    return (None if steps is None else times(int(steps))), eta


def mel_sampler(kwargs, hparams, use_hparams=True):
    """How the mel loop is sampled: forward(sampler=, mel_steps= / ddim_steps=, mel_order=, mel_spacing=, eta=, plms_interval=), else
    hparams['mel_sampler'] / ['mel_sample_steps'] / ['mel_sample_order'] / ['mel_sample_spacing'] / ['mel_sample_eta'], else the reference's
    own choice: PLMS under hparams['pndm_speedup'], otherwise its ancestral loop ("ddpm"). Returns a namespace (name, steps, order, spacing,
    eta, interval); `mel_timesteps` turns steps and spacing into network times once the schedule is packed.
    `use_hparams=False` (mel_stage, whose `sampler` argument always has a value) reads the arguments alone."""
    hp = hparams if use_hparams else {}
    pndm = hp.get("pndm_speedup")
    name = kwargs.get("sampler")
    if name is None:
        name = hp.get("mel_sampler")
        if name is not None and name != "plms" and pndm:
            raise ValueError(f"hparams: mel_sampler={name!r} together with pndm_speedup={pndm} (the reference's PLMS sampler): set one of them")
    if name is None:
        name = "plms" if pndm else "ddpm"
    if name not in MEL_SAMPLERS:
        raise ValueError(f"mel sampler {name!r}: one of {', '.join(MEL_SAMPLERS)}")
    spacing, order = pick(kwargs, hp, "mel_spacing", "mel_sample_spacing"), pick(kwargs, hp, "mel_order", "mel_sample_order", 2)
    if spacing is not None and spacing not in MEL_SPACINGS:
        raise ValueError(f"mel_spacing={spacing!r}: one of {', '.join(MEL_SPACINGS)} (None = the sampler's own default)")
    if order not in (1, 2):
        raise ValueError(f"mel_order={order!r}: 1 (first order: DDIM with eta = 0) or 2 (DPM-Solver++ 2M)")
    eta = float(pick(kwargs, hp, "eta", "mel_sample_eta", 0.0))
    steps = interval = None
    if name in MEL_SPACING_DEFAULT:   # the strided samplers
        own = kwargs if kwargs.get("mel_steps") is not None or name != "ddim" else dict(mel_steps=kwargs.get("ddim_steps"))
        steps = pick(own, hp, "mel_steps", "mel_sample_steps")
        if steps is None:
            raise ValueError(f"mel sampler {name!r} needs a number of network times: mel_steps" + (" / ddim_steps" if name == "ddim" else "")
                             + " or hparams['mel_sample_steps']")
        if int(steps) < 1:
            raise ValueError(f"mel_steps={steps}: at least 1 (more than K_step = {hparams['K_step']} means all of them)")
        steps, spacing = int(steps), spacing or MEL_SPACING_DEFAULT[name]
    elif name == "plms":
        interval = pick(kwargs, hp, "plms_interval", "pndm_speedup")
        if not interval:
            raise ValueError("mel sampler 'plms' needs its stride: plms_interval or hparams['pndm_speedup']")
        interval = int(interval)
    return types.SimpleNamespace(name=name, steps=steps, order=int(order), spacing=spacing, eta=eta, interval=interval)


Resolved = dataclasses.make_dataclass("Resolved", ("pitch_hz", "pitch_shift", "align", "align_band", "timing", "f0_ts", "f0_eta", "mel", "edit", "ref_weights",
                                                   "style_cache", "plan_slot", "noise", "seed"), frozen=True)


def resolve(kwargs, hp, f0_times, f0=None, uv=None, ref_mels=None, ref_f0=None):
    """What a forward call asks for, checked: forward's **kwargs (unknown keys are ignored) and the tensor arguments the rules read (shapes only)
    -> Resolved: pitch_hz, pitch_shift, align, align_band, timing (the contour group), f0_ts, f0_eta (`f0_sampler`), mel (`mel_sampler`), edit
    (`resolve_pitch_edit`; None = neutral), ref_weights, style_cache, plan_slot, noise, seed. ValueError on the first rule broken."""
    g = kwargs.get
    pitch_hz, band = g("pitch_hz"), g("pitch_align_band")
    if (f0 is None) != (uv is None):
        raise ValueError(f"forward: f0 and uv go together (got {'f0' if uv is None else 'uv'} without {'uv' if uv is None else 'f0'})")
    check_contour(FORWARD, pitch_hz is not None, pitch_hz is not None and f0 is not None, g("pitch_shift"), g("pitch_align"),
                  None if band is None else int(band), g("pitch_timing"), " (f0 / uv are taken as they are)" if f0 is not None else "")
    if pitch_hz is not None and not (isinstance(pitch_hz, (tuple, list)) and len(pitch_hz) == 2):
        raise ValueError("forward: pitch_hz = (contour_hz [B, Lc], lens_c)")
    if g("pitch_timing") is not None and g("f0_steps") is not None:
        raise ValueError("forward: f0_steps chooses how the f0 / uv diffusions are sampled; with pitch_timing (a pitch_hz contour) they do not run")
    f0_ts, f0_eta = f0_sampler(kwargs, hp, f0 is not None or pitch_hz is not None, f0_times)
    mel, edit = mel_sampler(kwargs, hp), resolve_pitch_edit(kwargs, hp)
    pooled = ref_mels is not None and ref_mels.dim() == 4
    if pooled and (ref_f0 is None or ref_f0.dim() != 3):
        raise ValueError(f"forward: ref_mels {tuple(ref_mels.shape)} is a pool of references per item; ref_f0 must then be [B, R, Tr]")
    if g("ref_weights") is not None and g("style_cache") is not None:
        raise ValueError("forward: ref_weights are part of the style_cache (encode_style_blend(..., ref_weights)); give them there")
    if g("ref_weights") is not None and not pooled:
        raise ValueError("forward: ref_weights weigh a pool of references: ref_mels [B, R, Tr, 80] and ref_f0 [B, R, Tr]")
    return Resolved(pitch_hz, g("pitch_shift"), g("pitch_align"), band, g("pitch_timing"), f0_ts, f0_eta, mel, edit, g("ref_weights"), g("style_cache"),
                    int(g("plan_slot", 0)), g("noise"), int(pick(kwargs, hp, "seed")))


def from_input(inp, hp, has_contour, layer=INPUT):
    """The input-dict form of the contour and edit controls -> the batch form (`infer_batch`, forward), checked in `layer`'s words: pitch_shift,
    pitch_align / pitch_timing with pitch_align_band = round(inp['pitch_align_band_s'] (default ALIGN_BAND_S) * sr / hop) guide frames (0 = full),
    and the edit keys as they are. hp: hparams, or (sr, hop). has_contour: inp gave a contour (the caller turns it into `pitch_hz`). {} without any."""
    hp = hp if isinstance(hp, dict) else dict(audio_sample_rate=hp[0], hop_size=hp[1])
    shift, align, band_s, timing = (inp.get(k) for k in ("pitch_shift", "pitch_align", "pitch_align_band_s", "pitch_timing"))
    band_s = None if band_s is None else float(band_s)
    check_contour(layer, has_contour, inp.get("pitch_hz") is not None and inp.get("pitch_audio") is not None, shift, align, band_s, timing)
    out = given(pitch_shift=None if shift is None else float(shift), pitch_align=align, pitch_timing=timing)
    if align is not None or timing is not None:
        out["pitch_align_band"] = int(round((ALIGN_BAND_S if band_s is None else band_s) * edit_fps(hp)))
    edit = {k: (tuple(inp[k]) if k == "vibrato_add" else float(inp[k])) for k in EDIT_KEYS if inp.get(k) is not None}
    if edit:
        resolve_pitch_edit(edit, hp)
    return {**out, **edit}


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def add_flags(ap):
    for c in CONTROLS:
        if c.flag:
            ap.add_argument(c.flag, **c.arg)


def from_flags(a, hparams):
    """The parsed flags -> (pitch: the input-dict entries, --pitch-npy still a path; hp: the hparams entries), checked by the rules above against
    `hparams` (the defaults: the instance checks again with the checkpoint's own). ValueError on the first rule broken."""
    val = lambda flag: getattr(a, flag[2:].replace("-", "_"))
    for c in CONTROLS:
        if c.owner and val(c.flag) is not None and (val(c.owner[0]) is None or (c.owner[1] and val(c.owner[0]) not in c.owner[1])):
            raise ValueError(f"{c.flag} belongs to {c.owner[0]}" + (" " + " or ".join(c.owner[1]) if c.owner[1] else ""))
    pitch = given(**{c.inp: val(c.flag) for c in CONTROLS if c.flag and c.inp})
    hp = given(**{c.hp: val(c.flag) for c in CONTROLS if c.flag and c.hp})
    check_contour(FLAGS, a.pitch_audio is not None or a.pitch_npy is not None, a.pitch_audio is not None and a.pitch_npy is not None,
                  a.pitch_shift, a.pitch_align, a.pitch_align_band_s, a.pitch_timing)
    if "vibrato_add" in pitch:
        pitch["vibrato_add"] = (*pitch["vibrato_add"], a.vibrato_delay_ms, a.vibrato_fade_ms)
    resolve_pitch_edit(pitch, hparams)
    f0_sampler({}, {**hparams, **hp}, False, int)
    if a.mel_eta is not None and not 0.0 <= a.mel_eta <= 1.0:
        raise ValueError("--mel-eta: inside [0, 1]")
    if a.mel_sampler != "plms":   # (its stride is hparams['pndm_speedup'], which has no flag: forward checks it)
        mel_sampler({}, {**hparams, **hp})
    return pitch, hp
