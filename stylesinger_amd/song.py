"""A score of any length: split into phrases at its rests, rendered as ordinary batches, stitched into one timeline on the device.

The reference was trained on segments of at most `max_frames: 3000` (16 s) and its self-attention and style aligner run over the whole frame
axis, so a song cannot go through `forward` as one item. `plan_song` (host, pure: no device is touched) cuts the reference's `inp` dict into
segments and batches; `sing_score` below (what `StyleSingerInfer.sing_score` runs) renders the plan's batches and puts the results on one timeline
with the two kernels of csrc/song.hip (`song_offsets`, `song_place` below). DESIGN.md §3.4h.

Policy
  * A phone is a REST when note_type == 1 or note == 0. A MINIMAL PHRASE ends at phone i when i is a rest and i + 1 is not, or i is the last phone:
    rests close a phrase (as in the example score); leading rests do not end a phrase that holds no note yet, they open the first one; a score
    without rests is one phrase. A minimal phrase is never cut.
  * Seconds of a phone range: with inp['ph_dur'] (seconds per phone) the exact sum; without, an ESTIMATE from the notes: the sum of note_dur[i]
    over the phones i that start the range or whose (note, note_dur, note_type) differs from phone i - 1 - consecutive phones that share a note
    count once. Immediately repeated EQUAL notes (same pitch, same length, same type) are indistinguishable from one note held over several phones
    and are therefore under-counted; give ph_dur where that matters.
  * Minimal phrases are merged greedily, left to right, while the merged range stays <= max_seconds (default 12 s: below the 16 s training limit,
    because without ph_dur the durations are the model's own). A minimal phrase that is longer on its own stays whole, with one warning.
  * With ph_dur the frame grid is global: b_i = floor(cumsum_f64(ph_dur)[i] * sr / hop + 0.5), phone i owns the frames [b_i, b_{i+1}) (possibly
    none), and a segment's explicit mel2ph is cut from that grid: the segments' frame counts sum to the song's and every segment starts on its score
    time. Without ph_dur, mel2ph is left to the duration predictor and the frame counts are known only after rendering.
  * Song-level pitch control (pitch_hz | pitch_audio, pitch_shift) needs ph_dur: the contour is fitted ONCE to the song's frame count
    (`pitch.contour_fit`, float64) and sliced per segment; every slice has its segment's length, so `ss_contour_fit` copies it bit for bit.
    With pitch_align = "dtw" (+ pitch_align_band_s) every segment then warps ITS slice onto its own notes (`ss_contour_align`), the slice's two ends
    pinned to the segment's: the planner's cut of the contour stays linear, the warp only moves notes inside a segment.
    With pitch_timing = "guide" every segment lays ITS phones out on its slice's frames instead (`ss_retime_mel2ph`, forward(pitch_timing=)): a
    slice has its segment's frame count, so notes move only inside a segment - segment starts and the song's length are those of the plan.
  * Batches: segments ordered by frame count (phone count when frames are unknown), descending, ties in song order; `segment_batch` per batch.
"""
import dataclasses
import warnings

import numpy as np
import torch

from . import lib as L
from .controls import CONTOUR_KEYS, EDIT_KEYS, PLAN, from_input
from .producers import has_features, row

NO_PH_DUR = ("song-level pitch control ({keys}) needs inp['ph_dur'] (seconds per phone): without it the durations are the model's own, so the "
             "segment frame counts are not known before rendering and the contour cannot be cut into per-segment slices")


def is_rest(note, note_type):
    return (np.asarray(note_type) == 1) | (np.asarray(note) == 0)


def minimal_phrases(note, note_type):
    """-> [(first, last)] phone ranges (last exclusive) that tile [0, P) in order."""
    rest = is_rest(note, note_type)
    P = len(rest)
    out, first = [], 0
    for i in range(P):
        # a rest followed by a note closes the phrase - unless the phrase holds nothing but rests so far: leading rests open the first phrase
        if i == P - 1 or (rest[i] and not rest[i + 1] and not rest[first:i + 1].all()):
            out.append((first, i + 1))
            first = i + 1
    return out


def range_seconds(first, last, note, note_dur, note_type, ph_dur=None):
    """Seconds of the phones [first, last): exact with ph_dur, else the estimate of the module docstring."""
    if ph_dur is not None:
        return float(np.sum(np.asarray(ph_dur, dtype=np.float64)[first:last]))
    s = 0.0
    for i in range(first, last):
        if i == first or (note[i], note_dur[i], note_type[i]) != (note[i - 1], note_dur[i - 1], note_type[i - 1]):
            s += float(note_dur[i])
    return s


def merge_phrases(phrases, seconds_of, max_seconds):
    """Greedy left-to-right merge of minimal phrases while seconds_of(first, last) <= max_seconds. -> [(first, last)]"""
    out = []
    for first, last in phrases:
        if out and seconds_of(out[-1][0], last) <= max_seconds:
            out[-1] = (out[-1][0], last)
            continue
        own = seconds_of(first, last)
        if own > max_seconds:
            warnings.warn(f"plan_song: the phrase of phones [{first}, {last}) takes {own:.2f} s on its own, more than max_seconds={max_seconds:g}: "
                          "it has no rest to cut at and is rendered whole")
        out.append((first, last))
    return out


def frame_bounds(ph_dur, sr, hop):
    """b_i = floor(cumsum_f64(ph_dur)[i] * sr / hop + 0.5) for i = 0 .. P: int64 [P + 1], b_0 = 0."""
    d = np.asarray(ph_dur, dtype=np.float64)
    if d.ndim != 1 or not np.isfinite(d).all() or (d < 0).any():
        raise ValueError("plan_song: inp['ph_dur'] must be finite, non-negative seconds per phone")
    t = np.concatenate([[0.0], np.cumsum(d, dtype=np.float64)])
    return np.floor(t * float(sr) / float(hop) + 0.5).astype(np.int64)


def fade_window(fade):
    """win[j] = 0.5 - 0.5 cos(pi (j + 0.5) / fade), j < fade: float64 rounded to fp32 (the table of ss_song_place)."""
    j = np.arange(int(fade), dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (j + 0.5) / max(int(fade), 1))).astype(np.float32)


@dataclasses.dataclass
class SongPlan:
    """What `plan_song` returns, and what the renderer and the tests consume.
    segments[s] (song order): dict(index, first, last (exclusive), seconds, n_frames | None, start_frame | None, batch, row);
    batches[i]: dict of host tensors as `infer_batch` takes them (txt_tokens, note, note_dur, note_type [nb, Tp] zero padded; with ph_dur mel2ph
        [nb, T]; with a contour pitch_hz = ([nb, T] fp32, [n_frames]), pitch_shift, pitch_align / pitch_timing + pitch_align_band) - `sing_score` replaces each by its device form, with the
        reference's features and style encoding added, so `infer_batch(plan.batches[i], seed=seed + i)` is what was rendered;
    rows[i][r] = song index of row r of batch i; n_frames = the song's frame count (None without ph_dur)."""
    segments: list
    batches: list
    rows: list
    n_frames: object
    sr: int
    hop: int
    max_seconds: float
    segment_batch: int
    pitch_hz: object = None    # the contour fitted to n_frames (fp32), before any pitch_shift


def check_pitch_keys(inp):
    """Song-level pitch keys without ph_dur are refused, with the reason (before anything is loaded or rendered)."""
    keys = [k for k in CONTOUR_KEYS if inp.get(k) is not None]
    if keys and inp.get("ph_dur") is None:
        raise ValueError("plan_song: " + NO_PH_DUR.format(keys=", ".join(keys)))
    return keys


def plan_song(inp, sr=48000, hop=256, max_seconds=12.0, segment_batch=8, ph_encoder=None):
    """inp: the reference's input dict at any length - `ph` (or `ph_token`), `note`, `note_dur`, `note_type`, optionally `ph_dur`, `pitch_hz`
    (a 1-D contour in Hz over the whole song, any length), `pitch_shift`, `pitch_align` ("dtw": each segment warps its slice of the contour onto its
    own notes; the cut between segments stays linear) with `pitch_align_band_s`, `pitch_timing` ("guide": each segment is sung in the timing of
    its slice). `pitch_correct`, `vibrato_scale`, `vibrato_add`, `pitch_smooth_ms` (controls.EDIT_KEYS: the pitch expression controls of forward) apply per
    segment, are copied into every batch and need neither a contour nor ph_dur. -> SongPlan."""
    keys = check_pitch_keys(inp)
    if "pitch_audio" in keys:
        raise ValueError("plan_song: the planner runs on the host; track inp['pitch_audio'] first and give its contour as inp['pitch_hz'] "
                         "(StyleSingerInfer.sing_score does)")
    ctl = from_input(inp, (sr, hop), "pitch_hz" in keys, PLAN)   # the batch form, checked: the edit keys (every segment gets them), with a contour the rest
    edit = {k: ctl.pop(k) for k in EDIT_KEYS if k in ctl}
    if inp.get("ph_token") is not None:
        tokens = np.asarray(inp["ph_token"], dtype=np.int64)
    elif ph_encoder is not None and inp.get("ph") is not None:
        tokens = np.asarray(ph_encoder.encode(" ".join(inp["ph"])), dtype=np.int64)
    else:
        raise ValueError("plan_song: give inp['ph_token'], or inp['ph'] and a phone encoder (StyleSingerInfer(..., phone_set=<phone_set.json>))")
    note = np.asarray(inp["note"], dtype=np.int64)
    note_dur = np.asarray(inp["note_dur"], dtype=np.float64)
    note_type = np.asarray(inp["note_type"], dtype=np.int64)
    P = len(tokens)
    if P == 0 or not (len(note) == len(note_dur) == len(note_type) == P):
        raise ValueError(f"plan_song: {P} phones, {len(note)} note, {len(note_dur)} note_dur, {len(note_type)} note_type entries")
    ph_dur = inp.get("ph_dur")
    if ph_dur is not None and len(ph_dur) != P:
        raise ValueError(f"plan_song: {len(ph_dur)} ph_dur entries for {P} phones")
    if int(segment_batch) < 1 or not float(max_seconds) > 0:
        raise ValueError(f"plan_song: segment_batch={segment_batch}, max_seconds={max_seconds}")
    nl, dl, tl = note.tolist(), note_dur.tolist(), note_type.tolist()
    ranges = merge_phrases(minimal_phrases(note, note_type), lambda a, b: range_seconds(a, b, nl, dl, tl, ph_dur), float(max_seconds))
    bounds = frame_bounds(ph_dur, sr, hop) if ph_dur is not None else None
    segments = []
    for s, (first, last) in enumerate(ranges):
        seg = dict(index=s, first=first, last=last, seconds=range_seconds(first, last, nl, dl, tl, ph_dur), n_frames=None, start_frame=None)
        if bounds is not None:
            seg["n_frames"], seg["start_frame"] = int(bounds[last] - bounds[first]), int(bounds[first])
            if seg["n_frames"] == 0:
                raise ValueError(f"plan_song: the segment of phones [{first}, {last}) has no frame on the {hop / sr * 1000:.2f} ms grid (ph_dur sums to "
                                 f"{seg['seconds']:.4f} s)")
        segments.append(seg)
    F = int(bounds[-1]) if bounds is not None else None
    contour = None
    if inp.get("pitch_hz") is not None:
        from .pitch import contour_fit
        hz = np.asarray(inp["pitch_hz"], dtype=np.float64)
        if hz.ndim != 1 or hz.size == 0:
            raise ValueError(f"plan_song: inp['pitch_hz'] must be a non-empty 1-D contour in Hz (got shape {hz.shape})")
        contour = contour_fit(hz, F).astype(np.float32)
    order = sorted(range(len(segments)), key=lambda s: -(segments[s]["n_frames"] if bounds is not None else segments[s]["last"] - segments[s]["first"]))
    batches, rows = [], []
    for i in range(0, len(order), int(segment_batch)):
        idx = order[i:i + int(segment_batch)]
        Tp = max(segments[s]["last"] - segments[s]["first"] for s in idx)
        b = dict(txt_tokens=torch.zeros(len(idx), Tp, dtype=torch.long), note=torch.zeros(len(idx), Tp, dtype=torch.long),
                 note_dur=torch.zeros(len(idx), Tp, dtype=torch.float32), note_type=torch.zeros(len(idx), Tp, dtype=torch.long), **edit)
        if bounds is not None:
            T = max(segments[s]["n_frames"] for s in idx)
            b["mel2ph"] = torch.zeros(len(idx), T, dtype=torch.long)
            if contour is not None:
                b["pitch_hz"] = (torch.zeros(len(idx), T, dtype=torch.float32), [segments[s]["n_frames"] for s in idx])
                b.update(ctl)
        for r, s in enumerate(idx):
            first, last = segments[s]["first"], segments[s]["last"]
            segments[s]["batch"], segments[s]["row"] = len(batches), r
            n = last - first
            b["txt_tokens"][r, :n] = torch.from_numpy(tokens[first:last])
            b["note"][r, :n] = torch.from_numpy(note[first:last])
            b["note_dur"][r, :n] = torch.from_numpy(note_dur[first:last].astype(np.float32))
            b["note_type"][r, :n] = torch.from_numpy(note_type[first:last])
            if bounds is not None:
                f0, nf = segments[s]["start_frame"], segments[s]["n_frames"]
                b["mel2ph"][r, :nf] = torch.from_numpy(np.repeat(np.arange(1, n + 1, dtype=np.int64), np.diff(bounds[first:last + 1])))
                if contour is not None:
                    b["pitch_hz"][0][r, :nf] = torch.from_numpy(contour[f0:f0 + nf])
        batches.append(b)
        rows.append(idx)
    return SongPlan(segments=segments, batches=batches, rows=rows, n_frames=F, sr=int(sr), hop=int(hop), max_seconds=float(max_seconds),
                    segment_batch=int(segment_batch), pitch_hz=contour)


# ---- the two kernels (csrc/song.hip): argument marshalling only ---------------------------------------------------------------------------
FLAG_READ, FLAG_WRITE, FLAG_INDEX = (L.abi.DEFINES["SS_SONG_FLAG_" + n] for n in ("READ", "WRITE", "INDEX"))


@torch.no_grad()
def song_offsets(lens, out=None):
    """lens int32 [S] on the device (frames, song order) -> offsets int64 [S + 1] (exclusive scan; no host sync)."""
    lens = lens.to(torch.int32).contiguous()
    S = lens.numel()
    out = torch.empty(S + 1, device=lens.device, dtype=torch.int64) if out is None else out
    L.ops.ss_song_offsets(lens, S, out)
    return out


@torch.no_grad()
def song_place(src, seg, lens, offsets, unit, out, win=None, flags=None, cap=None):
    """src fp32 [B, ...] contiguous rows on the device, seg int32 [B] (song index per row, < 0 = skip), lens int32 [S], offsets int64 [S + 1],
    unit floats per frame, out fp32 (flat), win fp32 [fade] or None, flags int32 [1] or None. `cap`: floats of `out` that may be written (all)."""
    B = src.shape[0]
    assert src.is_contiguous() and src.dtype == torch.float32 and out.dtype == torch.float32 and out.is_contiguous()
    assert seg.dtype == torch.int32 and lens.dtype == torch.int32 and offsets.dtype == torch.int64 and seg.numel() == B
    lds = src.numel() // B
    L.ops.ss_song_place(src, lds, seg, B, lens, offsets, lens.numel(), int(unit), win, 0 if win is None else win.numel(), out,
                        out.numel() if cap is None else int(cap), flags)
    return out


# ---- the renderer: `StyleSingerInfer.sing_score` ----------------------------------------------------------------------------------------------
def _song_reference(ins, inp, vad_flags):
    """The reference of a song, processed ONCE: (ref_mels [1, Tr, 80], ref_f0 [1, Tr], spk_embed [1, 256], emo_embed [1, 256], None) on the device,
    from the features in `inp` (`mel`, `spk_embed`, `emo_embed`, `f0`: as `infer_once` accepts them) or from inp['ref_audio'] through the
    producers of `_device_batch`. A pool of references (inp['ref_audios'], + 'ref_srs', 'ref_weights'): ref_mels [1, R, Tr, 80], ref_f0 [1, R, Tr], the
    two embeddings blended, and the normalised weights as a fifth entry (None for one reference)."""
    d = ins.device
    if inp.get("ref_audios") is not None:
        if has_features(inp):
            raise ValueError("sing_score: give inp['ref_audios'] (a pool of references) or the features of one reference (mel / spk_embed / emo_embed / f0), not both")
        one = {k: inp[k] for k in ("ref_audios", "ref_audio", "ref_sr", "ref_srs", "ref_weights", "ph", "ph_token", "note", "note_dur", "note_type") if k in inp}
        b = ins._device_batch(one, vad_flags)
        inp.setdefault("ph_token", one["ph_token"])
        return b["ref_mels"], b["ref_f0"], b["spk_embed"], b["emo_embed"], b["ref_weights"]
    if has_features(inp):
        from .pitch import norm_interp_f0
        f0, _uv = norm_interp_f0(np.asarray(inp["f0"]), ins.hparams)
        return (row(inp["mel"], torch.float32).to(d), f0[None].to(d), row(inp["spk_embed"], torch.float32).to(d),
                row(inp["emo_embed"], torch.float32).to(d), None)
    if inp.get("ref_audio") is None:
        raise ValueError("sing_score: give inp['ref_audio'] (the reference voice), or its features mel / spk_embed / emo_embed / f0")
    one = {k: inp[k] for k in ("ref_audio", "ref_sr", "ph", "ph_token", "note", "note_dur", "note_type") if k in inp}
    b = ins._device_batch(one, vad_flags)
    inp.setdefault("ph_token", one["ph_token"])
    return b["ref_mels"], b["ref_f0"], b["spk_embed"], b["emo_embed"], None


@torch.no_grad()
def sing_score(ins, inp, max_seconds=12.0, segment_batch=8, fade_ms=5.0, in_flight=3, seed=None, out_lufs=None, vad_flags=None,
               out_true_peak_db=None):
    """The body of `StyleSingerInfer.sing_score` (arguments and result: its docstring); `ins` = the infer object. The flow is the module docstring's:
    reference once, plan, batches through `infer_batches`, stitch on the device, loudness over the whole song."""
    hp, d = ins.hparams, ins.device
    sr, hop = int(hp["audio_sample_rate"]), int(ins.vocoder.model.hop)
    inp = dict(inp)
    check_pitch_keys(inp)   # pitch control without ph_dur is refused before a device is touched
    seed = hp["seed"] if seed is None else seed
    ref_mels, ref_f0, spk, emo, ref_w = _song_reference(ins, inp, vad_flags)
    if inp.get("pitch_audio") is not None:   # the guide vocal is tracked on the device; the planner takes its contour
        hz, _n = ins._pitch_inputs({"pitch_audio": inp.pop("pitch_audio")})["pitch_hz"]
        inp["pitch_hz"] = hz[0].cpu().numpy()
    plan = plan_song(inp, sr=sr, hop=hop, max_seconds=max_seconds, segment_batch=segment_batch, ph_encoder=ins.ph_encoder)
    S = len(plan.segments)
    # one encode for the whole song; a pool of references is encoded once too, as one blend cache (every tensor of it leads with the batch)
    style = ins.model.encode_style(ref_mels, ref_f0) if ref_mels.dim() == 3 else ins.model.encode_style_blend(ref_mels, ref_f0, ref_w)
    fade = max(0, int(round(float(fade_ms) * sr / 1000.0))) if S > 1 else 0
    win = torch.from_numpy(fade_window(fade)).to(d) if fade else None
    segs_dev, rows_dev = [], []
    for i, hb in enumerate(plan.batches):   # everything the stitch needs from the host goes up before the first batch runs
        nb = len(plan.rows[i])
        b = {k: ((v[0].to(d), v[1]) if k == "pitch_hz" else v.to(d) if torch.is_tensor(v) else v) for k, v in hb.items()}
        rep = lambda x: x.expand(nb, *x.shape[1:]).contiguous()
        b.update(spk_embed=rep(spk), emo_embed=rep(emo), ref_mels=ref_mels.expand(nb, *ref_mels.shape[1:]), ref_f0=ref_f0.expand(nb, *ref_f0.shape[1:]),
                 style_cache={k: rep(v) for k, v in style.items()})
        plan.batches[i] = b
        rows_dev.append(torch.tensor(plan.rows[i], dtype=torch.long).to(d))
        segs_dev.append(rows_dev[-1].to(torch.int32))
    results = list(ins.infer_batches(plan.batches, in_flight=in_flight, seed=seed))
    lens = torch.zeros(S, device=d, dtype=torch.int32)
    for rows, res in zip(rows_dev, results):
        lens.index_copy_(0, rows, res["lens"].to(torch.int32))
    offsets = song_offsets(lens)
    cap = sum(int(res["mel"].shape[0]) * int(res["mel"].shape[1]) for res in results)   # frames: no segment is longer than its batch
    wav, mel, f0 = (torch.empty(cap * u, device=d, dtype=torch.float32) for u in (hop, 80, 1))
    flags = torch.zeros(1, device=d, dtype=torch.int32)
    for seg, res in zip(segs_dev, results):
        song_place(res["wav"].contiguous(), seg, lens, offsets, hop, wav, win=win, flags=flags)
        song_place(res["mel"].contiguous(), seg, lens, offsets, 80, mel, flags=flags)
        song_place(res["f0"].contiguous(), seg, lens, offsets, 1, f0, flags=flags)
    unaligned = [res["model_out"]["pitch_align_status"].to(torch.int64) for res in results if "pitch_align_status" in res["model_out"]]
    loose = [res["model_out"]["pitch_retime_status"].to(torch.int64) for res in results if "pitch_retime_status" in res["model_out"]]
    n_st, n_rt = sum(u.numel() for u in unaligned), sum(u.numel() for u in loose)
    *starts, flagged = (int(v) for v in torch.cat([*unaligned, *loose, offsets, flags.to(torch.int64)]).cpu())   # the one host sync of the stitch
    st, rt, starts = starts[:n_st], starts[n_st:n_st + n_rt], starts[n_st + n_rt:]
    rows_flat = [s for rows in plan.rows for s in rows]   # (batch order) rows -> song indices
    retime_status = {rows_flat[k]: v for k, v in enumerate(rt)}
    if any(rt):
        warnings.warn(f"sing_score: pitch_timing left segment(s) {sorted(s for s, v in retime_status.items() if v)} to the linear stretch (not aligned, "
                      "or fewer guide frames than the segment has pitch changes)")
    if any(st):
        warnings.warn(f"sing_score: pitch_align left segment(s) {sorted(rows_flat[k] for k, v in enumerate(st) if v)} to the linear fit (more guide "
                      "frames per score frame than the band allows); widen pitch_align_band_s")
    if flagged != 0:
        raise L.StyleSingerHipError(f"sing_score: ss_song_place clamped or refused a segment (flags {flagged}): the plan and the rendered "
                                    "batches disagree")
    F = starts[-1]
    out = dict(wav=wav[:F * hop], mel=mel[:F * 80].view(F, 80), f0=f0[:F], plan=plan, segments=[])
    if any("pitch_edit" in res for res in results):   # the pitch edit's statistics per segment, song order, on the device
        out["pitch_edit"] = torch.zeros(S, 6, device=d, dtype=torch.float64)
        for rows, res in zip(rows_dev, results):
            out["pitch_edit"].index_copy_(0, rows, res["pitch_edit"])
    for s, g in enumerate(plan.segments):
        g["start_frame"], g["n_frames"] = starts[s], starts[s + 1] - starts[s]
        out["segments"].append({k: g[k] for k in ("first", "last", "start_frame", "n_frames", "batch", "row")})
        if retime_status:
            out["segments"][-1]["pitch_retime_status"] = retime_status[s]
    long_ = [s for s, g in enumerate(plan.segments) if g["n_frames"] > 3000]
    if long_:
        warnings.warn(f"sing_score: {len(long_)} segment(s) came out longer than the 3000 frames the model was trained on (first: phones "
                      f"[{plan.segments[long_[0]]['first']}, {plan.segments[long_[0]]['last']}), {plan.segments[long_[0]]['n_frames']} frames); lower "
                      "max_seconds or add rests")
    target = out_lufs if out_lufs is not None else hp.get("out_loudness_lufs")
    ceiling = out_true_peak_db if out_true_peak_db is not None else hp.get("out_true_peak_db")
    if target is not None or ceiling is not None:   # the WHOLE song, once, after the stitch
        y, info = ins._finish_wav(out["wav"][None], [F * hop], target, ceiling)
        out["wav"] = y[0]
        if target is not None:
            out["lufs"] = float(info["lufs"][0])
        if ceiling is not None:
            out["limiter"] = info["limiter"]
    return out
