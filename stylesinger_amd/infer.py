"""Inference entrypoint of the HIP path: mirror of `inference/StyleSinger.py::StyleSingerInfer`.

`StyleSingerInfer(hparams).forward_model(inp)` keeps the reference's single-utterance contract
(inference/StyleSinger.py:41-63: run the model, drop all-zero frames, clip the mel to
[mel_vmin, mel_vmax], vocode with the predicted f0).  `infer_batch` is the batched, device-resident
form the benchmark and the data-parallel driver use.  The feature extractors of `preprocess_input`
(:94-137) run on the device (`producers.py`, the `ReferenceProducers` mixin of the class): `preprocess_batch` computes the reference mel, the emotion embedding, the speaker
embedding (resemblyzer's published algorithm on the emotion encoder's kernels, `speaker.py`; parity unpinned: un-vendored package),
the f0 contour (Praat's autocorrelation method, `f0track.py`; parity unpinned: parselmouth is un-vendored) and its normalisation.
`trim_long_silences` runs on the device AROUND webrtcvad's per-window decisions (a fixed-point GMM whose tables are not in the reference tree):
they are computed on the host when the package is importable, or given by the caller; skipping the trim is an explicit opt-out
(`vad_flags=False`), never a silent default. `vad_flags="lrt"` / `StyleSingerInfer(vad="lrt")` / `--vad lrt` opt into this project's own
decision on the device instead (`vadtrim.lrt_statistic`, `ss_vad_lrt`: a likelihood-ratio test, NOT webrtcvad's; the audio then never leaves the device).
`infer_once(inp)` = the reference's entry point (inference/StyleSinger.py:175-179) with the features kept on the device between the producers and
the model; `python -m stylesinger_amd.infer` = `example_run` (:181-331).
`sing_score(inp)` (`--score song.json`) sings a score of any length: split at its rests, rendered as batches, stitched on the device (`song.py`: planner and renderer).
"""
import json
import os
import warnings

import numpy as np
import torch

from . import controls
from . import lib as L
from .config import DEFAULT_HPARAMS, make_hparams, make_vocoder_config
from .model import StyleSingerHIP
from .producers import ReferenceProducers, has_features, row
from .vocoder import get_vocoder_cls


def _write_wav(ins, wav, out_path):
    """The tail of both runs: `wav` (host, fp32) to `out_path` as 16-bit PCM (utils/audio.py:12-17), reported as the reference does."""
    from .writer import save_wav
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    save_wav(wav, out_path, int(ins.hparams["audio_sample_rate"]), norm=bool(ins.hparams.get("out_wav_norm", False)))
    print(f"Save at {out_path}.")


def _instance(cls, hparams, ctor):
    """`ctor` of `example_run` / `_score_run`: `exp_dir` + `vocoder_dir` go through `from_checkpoints`, anything else is the constructor's."""
    if "exp_dir" in ctor:
        return cls.from_checkpoints(hparams, ctor.pop("exp_dir"), ctor.pop("vocoder_dir"), **ctor)
    return cls(hparams, **ctor)


class StyleSingerInfer(ReferenceProducers):
    def __init__(self, hparams=None, device=None, model_state=None, vocoder_state=None, vocoder_config=None, dictionary=None,
                 emotion_state=None, speaker_state=None, phone_set=None, loudness=None, vad=None):
        """`loudness`: "bs1770" = honour hparams['loud_norm'] with this project's BS.1770 meter (`loudness.py`; parity with pyloudnorm UNPINNED, so
        the bare flag stays refused: `loudness.resolve_loudness`).
        `vad`: what `vad_flags=None` resolves to in `preprocess_input` / `infer_once` / `sing_score` (`_resolve_vad`): None = the reference's
        webrtcvad decision on the host (ImportError where the package is missing), "webrtc" = the same, asked for by name, "lrt" = this
        project's own likelihood-ratio decision on the device (`vadtrim.py`; NOT webrtcvad's, constants unassessed on recordings).
        `emotion_state`: state_dict of the reference's emotion encoder checkpoint (`EmotionEncoder.load_model`,
        inference/StyleSinger.py:101) - enables the emotion branch of `preprocess_batch`.
        `speaker_state`: `model_state` of resemblyzer's `pretrained.pt` (`VoiceEncoder()`, inference/StyleSinger.py:100) - enables the
        speaker branch."""
        if vad not in (None, "webrtc", "lrt"):
            raise ValueError(f"vad={vad!r}: expected None, 'webrtc' or 'lrt'")
        self.vad = vad
        self.hparams = make_hparams(hparams)
        self._front_hparams = hparams
        # inference/StyleSinger.py:27-28: ph_encoder = build_token_encoder(f"{processed_data_dir}/phone_set.json"); `phone_set` overrides the path
        # (the released checkpoint ships it as ZH_checkpoint_phone_set.json). Without one the caller passes inp['ph_token'] or sets self.ph_encoder.
        self.ph_encoder = None
        if phone_set is None and hparams and hparams.get("processed_data_dir"):
            cand = os.path.join(str(hparams["processed_data_dir"]), "phone_set.json")
            phone_set = cand if os.path.exists(cand) else None
        if phone_set is not None:
            from .text_encoder import build_token_encoder
            self.ph_encoder = build_token_encoder(phone_set)
            if dictionary is None:
                dictionary = self.ph_encoder
        from .loudness import resolve_loudness
        self._loud_norm = resolve_loudness(hparams, loudness)   # refuses the bare flag, before a device is touched
        from .denoise import resolve_denoise
        resolve_denoise(self.hparams)   # hparams['vocoder_denoise_c'] > 0: a geometry the kernel does not compute is refused here (the vocoder plugin applies it)
        if self.hparams.get("out_loudness_lufs") is not None and (self.hparams.get("out_wav_norm") or (hparams or {}).get("out_wav_norm")):
            raise ValueError("hparams: out_loudness_lufs and out_wav_norm exclude each other (a loudness target or peak normalisation, not both)")
        if self.hparams.get("out_true_peak_db") is not None:
            if self.hparams.get("out_wav_norm") or (hparams or {}).get("out_wav_norm"):
                raise ValueError("hparams: out_true_peak_db and out_wav_norm exclude each other (a true-peak ceiling or peak normalisation, not both)")
            from .limiter import ceiling_f32, window_samples   # a ceiling above 0 dBFS or a window beyond LIMIT_MAX_W: refused before a device is touched
            ceiling_f32(self.hparams["out_true_peak_db"])
            window_samples(self.hparams["audio_sample_rate"], self.hparams["out_limiter_lookahead_ms"])
        if device is None:
            if not torch.cuda.is_available():
                raise L.StyleSingerHipError("StyleSingerInfer (HIP) needs a GPU: there is no CPU path")
            device = "cuda"
        self.device = torch.device(device)
        self.model = self.build_model(dictionary, model_state)
        self.model.eval()
        self.model.to(self.device)
        vcfg = make_vocoder_config(vocoder_config)
        if not (vocoder_config and "mfma_precision" in vocoder_config):
            vcfg["mfma_precision"] = self.hparams.get("mfma_precision", "fp32")
        self.vocoder = get_vocoder_cls(self.hparams)(config=vcfg, state_dict=vocoder_state,
                                                     device=self.device, hparams=self.hparams)
        self._mel_frontend = None
        self._emo_frontend = None
        self.emotion_encoder = None
        if emotion_state is not None:
            from .emotion import EmotionEncoderHIP
            self.emotion_encoder = EmotionEncoderHIP(emotion_state, device=self.device)
        self.speaker_encoder = None
        if speaker_state is not None:
            from .speaker import SpeakerEncoderHIP
            self.speaker_encoder = SpeakerEncoderHIP(speaker_state, device=self.device)

    @classmethod
    def from_checkpoints(cls, hparams, exp_dir, vocoder_dir, **ctor):
        """Build from the reference's on-disk checkpoints (inference/StyleSinger.py:34-39 + hifigan_nsf.py:46-61):
        `exp_dir` = checkpoints/<exp_name> (newest model_ckpt_steps_*.ckpt), `vocoder_dir` = hparams['vocoder_ckpt']; `ctor` = the constructor's other keywords."""
        from . import ckpt
        state, _ = ckpt.read_state(exp_dir, "model")
        if state is None:
            raise FileNotFoundError(f"| ckpt not found in {exp_dir}.")
        vstate, vcfg = ckpt.load_vocoder_ckpt(vocoder_dir)
        return cls(hparams, model_state=state, vocoder_state=vstate, vocoder_config=vcfg, **ctor)

    def build_model(self, dictionary=None, state=None):
        model = StyleSingerHIP(dictionary, hparams=self.hparams)
        if state is not None:
            model.load_state_dict(state, strict=False)
        return model

    # ---- batched, device resident -------------------------------------------------------------
    @torch.no_grad()
    def infer_batch(self, batch, noise=None, vocoder_noise=None, seed=None, vocode=True, plan_slot=0, out_lufs=None, out_true_peak_db=None):
        """batch: dict of device tensors (txt_tokens, note, note_dur, note_type, spk_embed, emo_embed, ref_mels,
        ref_f0, optional mel2ph).  Returns dict(mel [B,T,80], f0 [B,T], lens int32 [B], wav [B,T*hop]).
        Pitch control (StyleSingerHIP.forward): optional `f0` + `uv` [B, T] (the normalised contour, the reference's use_gt_f0 form), or
        `pitch_hz` = (contour in Hz [B, Lc], lens_c) with optional `pitch_shift` (semitones); without them the f0 is predicted. With
        `pitch_align` = "dtw" (+ `pitch_align_band`, guide frames; 0 / None = full) the contour is warped onto the score's notes instead of
        being scaled linearly; items the aligner left to the linear fit (`model_out['pitch_align_status']` != 0) are named in a warning where
        this method reads the lengths on the host anyway (`out_lufs`), never through a sync of its own. With `pitch_timing` = "guide" the score is
        sung in the contour's timing (forward(pitch_timing=): the contour on the mel hop grid; as many frames come out as the contour has); items
        left to the linear stretch (`model_out['pitch_retime_status']` != 0) are named in the same place.
        Pitch expression controls, with or without a contour: `pitch_correct`, `vibrato_scale`, `vibrato_add`, `pitch_smooth_ms` as forward takes
        them; res['pitch_edit'] then carries the statistics [B, 6] (float64, on the device).
        `out_lufs`: bring every item of `wav` to this BS.1770 integrated loudness (`_to_lufs`; adds res['lufs'], the loudness before the gain).
        `out_true_peak_db`: hold every item of `wav` under this true-peak ceiling with the look-ahead limiter (`_finish_wav`, `limiter.py`; adds
        res['limiter'] = {min_gain, n_limited} as device tensors); with `out_lufs` too the loudness gain is applied in full (res['loudness_gain'])
        and the limiter takes the place of the peak rule.
        Optional `style_cache`: what `model.encode_style` returned for the batch's references; the style encoder is then skipped.
        A pool of references per item (`_device_batch` with inp['ref_audios']): `ref_mels` [B, R, Tr, 80], `ref_f0` [B, R, Tr] and optional
        `ref_weights` (host values; priors on the style attention, forward(ref_weights=)), or a `style_cache` from `model.encode_style_blend`;
        `spk_embed` / `emo_embed` are then the blended [B, 256] (`model.blend_embeds`)."""
        hp = self.hparams
        seed = hp["seed"] if seed is None else seed
        passed_on = controls.given(**{k: batch.get(k) for k in controls.BATCH_KEYS})   # (style_cache: the references' style, encoded once by the caller)
        out = self.model(batch["txt_tokens"], mel2ph=batch.get("mel2ph"), spk_embed=batch["spk_embed"], emo_embed=batch["emo_embed"],
                         ref_mels=batch["ref_mels"], ref_f0=batch["ref_f0"], f0=batch.get("f0"), uv=batch.get("uv"), global_steps=320000,
                         infer=True, note=batch["note"], note_dur=batch["note_dur"], note_type=batch["note_type"], noise=noise, seed=seed,
                         plan_slot=plan_slot, **passed_on)
        res = dict(mel=out["mel_out"], f0=out["f0_denorm"], lens=out["lens"], model_out=out)
        if "pitch_edit" in out:   # the statistics of the pitch edit, float64 [B, 6] on the device (forward: pitch_correct / vibrato_scale / vibrato_add)
            res["pitch_edit"] = out["pitch_edit"]
        if vocode:
            res["wav"] = self.vocode(out["mel_out"], out["f0_denorm"], out["lens"], noise=vocoder_noise, seed=seed + 101)
            if out_lufs is not None or out_true_peak_db is not None:
                res["wav"], info = self._finish_wav(res["wav"], [int(v) * self.vocoder.model.hop for v in out["lens"].cpu()], out_lufs, out_true_peak_db)
                res.update(info)
                self._warn_unaligned(out)   # (the copy above synchronised)
        return res

    @staticmethod
    def _warn_unaligned(model_out, what="items"):
        """pitch_align: name the items the aligner did not align (status != 0: they got the linear fit). Call only where the host has just waited for
        the forward: this reads a device tensor."""
        st = model_out.get("pitch_align_status")
        bad = [] if st is None else [i for i, v in enumerate(st.cpu().tolist()) if v != 0]
        if bad:
            warnings.warn(f"pitch_align: {what} {bad} not aligned (more guide frames per score frame than the band allows, or empty): they got the "
                          "linear fit; widen pitch_align_band")
        rt = model_out.get("pitch_retime_status")
        loose = [] if rt is None else [i for i, v in enumerate(rt.cpu().tolist()) if v != 0]
        if loose:
            warnings.warn(f"pitch_timing: {what} {loose} not retimed (not aligned, or fewer guide frames than the score has pitch changes): their "
                          "phones are stretched linearly over the guide's frames")
        return bad

    def _to_lufs(self, wav, lens, target):
        """The output loudness target (hparams['out_loudness_lufs'], `infer_batch(out_lufs=)`): wav [B, L] on the device, lens host ints ->
        (every item at `target` LUFS, divided by its peak where that exceeds 1; lufs [B] float64 = the loudness measured before the gain). An
        item shorter than one 0.4 s gating block has no loudness: it is returned untouched (lufs NaN), with one warning per call."""
        from .loudness import normalize_batch
        y, m = normalize_batch(wav, lens, int(self.hparams["audio_sample_rate"]), target=float(target), short="skip")
        if 0 in m["n_blocks"]:
            warnings.warn(f"out_loudness_lufs: {m['n_blocks'].count(0)} item(s) shorter than one 0.4 s gating block left at their own level")
        return y, m["lufs"]

    def _finish_wav(self, wav, lens, out_lufs=None, true_peak_db=None):
        """The end of the output chain for wav [B, L] on the device (lens host ints) -> (wav, what it adds to a result dict). Without a
        ceiling: `_to_lufs` (or nothing). With `true_peak_db` (hparams['out_true_peak_db']): the look-ahead true-peak limiter (`limiter.py`);
        a loudness target then becomes `ss_loudness_measure` + `ss_limit_true_peak(gain=...)` - the gain in full ('loudness_gain', fp32 [B]), no
        division by the peak - and 'limiter' = {min_gain, n_limited} stay on the device."""
        if true_peak_db is None:
            if out_lufs is None:
                return wav, {}
            y, lufs = self._to_lufs(wav, lens, out_lufs)
            return y, dict(lufs=lufs)
        from .limiter import limit_batch
        sr, info, gain = int(self.hparams["audio_sample_rate"]), {}, None
        if out_lufs is not None:
            from .loudness import measure_batch
            m = measure_batch(wav, lens, sr, target=float(out_lufs), short="skip")
            if 0 in m["n_blocks"]:
                warnings.warn(f"out_loudness_lufs: {m['n_blocks'].count(0)} item(s) shorter than one 0.4 s gating block left at their own level")
            gain = m["gain"]
            info.update(lufs=m["lufs"], loudness_gain=gain)
        y, rep = limit_batch(wav, lens, sr, true_peak_db, lookahead_ms=self.hparams["out_limiter_lookahead_ms"], gain=gain)
        info["limiter"] = rep
        return y, info

    @torch.no_grad()
    def infer_batches(self, batches, in_flight=3, seed=None, vocode=True):
        """Throughput form of infer_batch for a sequence of INDEPENDENT batches: batch i runs on HIP stream i % in_flight with
        its own workspace / hipGraph set (`plan_slot`), so up to `in_flight` batches overlap on the device - one batch's
        single-round kernel launches leave ramps and tails that the others' blocks fill (-10 % wall at C2).
        Yields the result dicts in order; each result is complete (its stream has been waited for) when it is yielded."""
        in_flight = max(1, int(in_flight))
        if not hasattr(self, "_flight_streams") or len(self._flight_streams) < in_flight:
            self._flight_streams = [torch.cuda.Stream(device=self.device) for _ in range(in_flight)]
        seed = self.hparams["seed"] if seed is None else seed
        main = torch.cuda.current_stream(self.device)
        pending = []

        def finish(entry):
            res, strm = entry
            main.wait_stream(strm)
            if self.model.f16:   # the fp16 modes' range check, where this path waits for the batch anyway
                strm.synchronize()
                self.model.check_finite(res["model_out"])
            # the results were allocated from the side stream's pool and are handed to the caller's stream: tell the allocator, or
            # the next batch on that side stream could reuse the memory while `main` still reads it
            for v in list(res.values()) + list(res.get("model_out", {}).values()):
                if torch.is_tensor(v) and v.is_cuda:
                    v.record_stream(main)
            return res
        # `batches` may be a lazy producer (a dataset loop placing batches on the GPU): it is consumed one batch at a time, so at most
        # `in_flight` batches are resident. Lazily built shared state is created here, on the caller's stream, not inside a forward on a
        # side stream: a default size up front, and a batch longer than that grows it when the batch is pulled (the tables only grow).
        warm = 2048
        self.model.warm_caches(warm, self.device)
        if getattr(self.vocoder, "_denoise_v", None) is not None:   # the denoise table of this device: uploaded here, not on a side stream
            from .denoise import device_table, geometry
            device_table(geometry(self.vocoder.hparams)[0], self.device)
        for i, batch in enumerate(batches):
            need = max(int(batch["mel2ph"].shape[1]) if batch.get("mel2ph") is not None else 0, int(batch["ref_mels"].shape[-2]) + (31 if batch["ref_mels"].dim() == 4 else 0))   # (a pool's frame axis is padded to the 32-key tile)
            if need > warm:
                warm = need
                self.model.warm_caches(warm, self.device)
            strm = self._flight_streams[i % in_flight]
            strm.wait_stream(main)   # the batch's inputs were produced on the caller's stream
            with torch.cuda.stream(strm):
                res = self.infer_batch(batch, seed=seed + i, vocode=vocode, plan_slot=i % in_flight)
                for v in batch.values():
                    if torch.is_tensor(v):
                        v.record_stream(strm)
            pending.append((res, strm))
            if len(pending) >= in_flight:
                yield finish(pending.pop(0))
        while pending:
            yield finish(pending.pop(0))

    @torch.no_grad()
    def vocode(self, mel, f0, lens, noise=None, seed=1234):
        """Clip the mel and run the vocoder plugin's batched form; with hparams['vocoder_denoise_c'] > 0 that denoises every item on the device right
        after the generator (`HifiGAN.spec2wav_batch`): before `out_lufs`, before the PCM16 writer and, in `sing_score`, per segment before the stitch -
        the song then holds what single `spec2wav` calls would return."""
        hp = self.hparams
        mel_c = torch.empty_like(mel)
        L.ops.ss_clip(mel, mel_c, mel.numel(), float(hp["mel_vmin"]), float(hp["mel_vmax"]))
        return self.vocoder.spec2wav_batch(mel_c, f0, lens=lens, noise=noise, seed=seed)

    @torch.no_grad()
    def infer_batch_to_files(self, batch, names, writer, seed=None):
        """Batched form of the reference's test step + after_infer (tasks/StyleSinger/stylesinger.py:186-275), which
        is limited to batch size 1: run the batch, vocode it, quantise to PCM16 on the device, crop each item to its own
        frame count and queue the files on `writer` (a writer.WavWriter). As there (:180-182), the batch's ground-truth `f0` / `uv` are handed
        to the model only with hparams['use_gt_f0']; otherwise the f0 is predicted, whatever the dataset batch carries."""
        from .writer import wav_to_pcm16
        if not (self.hparams.get("use_gt_f0") and batch.get("f0") is not None and batch.get("uv") is not None):
            batch = {k: v for k, v in batch.items() if k not in ("f0", "uv")}
        res = self.infer_batch(batch, seed=seed, out_lufs=self.hparams.get("out_loudness_lufs"), out_true_peak_db=self.hparams.get("out_true_peak_db"))
        self.model.check_finite(res["model_out"])
        hop = self.vocoder.model.hop
        pcm = wav_to_pcm16(res["wav"], res["lens"], hop, norm=bool(self.hparams.get("out_wav_norm", False)))
        writer.submit_batch(names, pcm, res["lens"], hop)
        return res

    # ---- the reference's single-utterance surface ---------------------------------------------
    def input_to_batch(self, item):
        """inference/StyleSinger.py:139-172: `item['f0']` is the tracker's contour in Hz (0 = unvoiced) and goes through
        `norm_interp_f0` (utils/pitch_utils.py:47-62) exactly as there (:152)."""
        from .pitch import norm_interp_f0
        d = self.device
        f0, _uv = norm_interp_f0(np.asarray(item["f0"]), self.hparams)
        return dict(txt_tokens=row(item["ph_token"], torch.long).to(d), ref_mels=row(item["mel"], torch.float32).to(d),
                    spk_embed=row(item["spk_embed"], torch.float32).to(d), emo_embed=row(item["emo_embed"], torch.float32).to(d),
                    note=row(item["note"], torch.long).to(d), note_dur=row(item["note_dur"], torch.float32).to(d),
                    note_type=row(item["note_type"], torch.long).to(d), ref_f0=f0[None].to(d),
                    **({"mel2ph": row(item["mel2ph"], torch.long).to(d)} if "mel2ph" in item else {}), **self._pitch_inputs(item))

    def _wav_from_result(self, res, vocoder_noise=None):
        """inference/StyleSinger.py:53-63: drop all-zero frames, clip the mel, vocode with the predicted f0 (one item)."""
        mel_pred = res["mel"].cpu().numpy()
        self.model.check_finite(res["model_out"])   # (the copy above synchronised)
        self._warn_unaligned(res["model_out"])
        f0_pred = res["f0"].cpu().numpy()
        mask = np.abs(mel_pred).sum(-1) > 0
        mel_pred = np.clip(mel_pred[mask], self.hparams["mel_vmin"], self.hparams["mel_vmax"])
        f0_pred = f0_pred[mask]
        return self.vocoder.spec2wav(mel_pred, f0=f0_pred, noise=vocoder_noise)

    def forward_model(self, inp, noise=None, vocoder_noise=None):
        sample = self.input_to_batch(inp)
        return self._wav_from_result(self.infer_batch(sample, noise=noise, vocoder_noise=None, vocode=False), vocoder_noise)

    def postprocess_output(self, output):
        return output

    def infer_once(self, inp, vad_flags=None, noise=None, vocoder_noise=None):
        """inference/StyleSinger.py:175-179: preprocess_input -> forward_model -> postprocess_output. The features stay on the device between the
        producers and the model (no numpy detour; `preprocess_input` is the form that returns them). An `inp` that already carries the features
        (`mel`, `spk_embed`, `emo_embed`, `f0`, `ph_token`) skips the producers, as before."""
        if has_features(inp) and "ph_token" in inp:
            return self.postprocess_output(self.forward_model(inp, noise=noise, vocoder_noise=vocoder_noise))
        batch = self._device_batch(inp, vad_flags)
        res = self.infer_batch({k: v for k, v in batch.items() if k not in ("n_mel", "wav_fn", "ref_f0_hz")}, noise=noise, vocode=False)
        return self.postprocess_output(self._wav_from_result(res, vocoder_noise))

    def sing_score(self, inp, max_seconds=12.0, segment_batch=8, fade_ms=5.0, in_flight=3, seed=None, out_lufs=None, vad_flags=None,
                   out_true_peak_db=None):
        """Sing a score of any length in the reference's voice: `inp` = the reference's input dict (`ph` | `ph_token`, `note`, `note_dur`, `note_type`,
        optionally `ph_dur` = seconds per phone, `pitch_hz` | `pitch_audio`, `pitch_shift`, `pitch_align` (+ `pitch_align_band_s`): every segment
        then warps ITS slice of the contour onto its own notes, the slice's ends pinned; the planner's cut of the contour stays linear;
        `ref_audio` or the reference's features, or `ref_audios` (+ `ref_srs`, `ref_weights`) = a weighted pool of references, blended as
        `_device_batch` / `model.encode_style_blend` describe and encoded once for the whole song). The score
        is cut into phrases at its rests (`song.plan_song`: policy and limits there), the reference is processed and its style encoded ONCE, the
        plan's batches run through `infer_batches` (batch i with seed + i), and the segments are put on one timeline on the device
        (`ss_song_offsets` + three `ss_song_place` per batch: the waveform with a raised-cosine fade of `fade_ms` on both sides of every joint, the
        mel and the f0 as they are). Segments never overlap: the song is their concatenation. ONE host sync at the end learns the length. Loudness
        (`out_lufs`, else hparams['out_loudness_lufs']) is applied to the WHOLE song, never per segment: that would flatten its dynamics. So is the
        true-peak limiter (`out_true_peak_db`, else hparams['out_true_peak_db']; `_finish_wav`), once, after the stitch: adds 'limiter' (one entry).
        `pitch_timing` = "guide": every segment is sung in the timing of ITS slice of the contour (forward(pitch_timing=)); notes move only inside
        a segment, segment starts and the song's length stay the plan's; each entry of `segments` then carries `pitch_retime_status`.
        -> dict(wav [N], mel [F, 80], f0 [F] on the device, segments = [{first, last, start_frame, n_frames, batch, row}] (phones [first, last)),
        plan (the SongPlan; its batches in their device form), lufs (float, the loudness before the gain) when a target is set)."""
        from . import song
        return song.sing_score(self, inp, max_seconds=max_seconds, segment_batch=segment_batch, fade_ms=fade_ms, in_flight=in_flight, seed=seed,
                               out_lufs=out_lufs, vad_flags=vad_flags, out_true_peak_db=out_true_peak_db)

    @torch.no_grad()
    def evaluate(self, res, target_wavs, target_lens, target_srs=None, align="dtw", band_s=2.0):
        """Score what `infer_batch` (wav [B, L], lens = frames per item) or `sing_score` (wav [N]: one item) returned against target recordings
        target_wavs [B, Lt] (target_lens valid samples, host ints; at the model's rate or at `target_srs`): `evaluate.score_wavs` on the rendered
        waveform - the F0 frame error, the f0 RMSE in cents, the log-mel cepstral distortion along the DTW path (`align`, `band_s`; this project's
        own definition, not SPTK / WORLD MCD) and, with a speaker encoder loaded, `singer_cos`. Reads `res['lens']` on the host (one sync)."""
        from .evaluate import score_wavs
        if res.get("wav") is None:
            raise ValueError("evaluate: the result carries no 'wav' (infer_batch(vocode=False)?); score mels with evaluate.score_pairs")
        wav = res["wav"]
        if wav.dim() == 1:                               # sing_score: the song is one item
            wav, lens = wav[None], [int(wav.numel())]
        else:
            hop = int(self.vocoder.model.hop)
            lens = [min(int(v) * hop, int(wav.shape[1])) for v in res["lens"].cpu()]
        tw = torch.as_tensor(target_wavs)
        return score_wavs(self, wav, lens, tw[None] if tw.dim() == 1 else tw, target_lens, srs_b=target_srs, align=align, band_s=band_s)

    @classmethod
    def example_run(cls, hparams=None, ref_audio="test/test.wav", out_path="infer_out/test.wav", vad_flags=None, pitch=None, ref_blend=None, **ctor):
        """inference/StyleSinger.py:181-331: the example score (stylesinger_amd/example_input.json = that method's input dict, extracted by
        `python -m oracle.gen_golden --round6`) sung in the style of `ref_audio`, written to `out_path` as 16-bit PCM (utils/audio.py:12-17).
        `ctor`: how to build the instance - `exp_dir` + `vocoder_dir` (the reference's checkpoints, `from_checkpoints`) or explicit
        `model_state` / `vocoder_state` / `emotion_state` / `speaker_state` / `phone_set`. `ref_blend` = (paths, weights): sing in a weighted
        blend of these references instead (inp['ref_audios'] / ['ref_weights']; `ref_audio` is then unused)."""
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "example_input.json")) as fh:
            inp = {k: v for k, v in json.load(fh).items() if k != "source"}
        if ref_blend is not None:
            inp.pop("ref_audio", None)   # (the example dict names the reference's own test clip)
            inp["ref_audios"], inp["ref_weights"] = list(ref_blend[0]), list(ref_blend[1])
        else:
            inp["ref_audio"] = ref_audio
        inp.update(pitch or {})   # the contour and edit controls in their input-dict form (`controls.CONTOUR_KEYS`, `EDIT_KEYS`)
        ins = _instance(cls, hparams, ctor)
        out = ins.infer_once(inp, vad_flags=vad_flags)
        if ins.hparams.get("out_loudness_lufs") is not None or ins.hparams.get("out_true_peak_db") is not None:
            y, _ = ins._finish_wav(torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32))[None].to(ins.device), [len(out)],
                                   ins.hparams.get("out_loudness_lufs"), ins.hparams.get("out_true_peak_db"))
            out = y[0].cpu().numpy()
        _write_wav(ins, out, out_path)
        return out


def _score_run(score, hparams, out_path, segments_out=None, vad_flags=None, max_seconds=12.0, segment_batch=8, fade_ms=5.0, **ctor):
    """`--score`: sing the score dict with `StyleSingerInfer.sing_score`, write the song as 16-bit PCM and, with `segments_out`, the timeline as JSON
    (per segment its phone range, start sample and sample count: for lining the vocal up with an accompaniment)."""
    ins = _instance(StyleSingerInfer, hparams, ctor)
    res = ins.sing_score(score, max_seconds=max_seconds, segment_batch=segment_batch, fade_ms=fade_ms, vad_flags=vad_flags)
    sr, hop = int(ins.hparams["audio_sample_rate"]), int(ins.vocoder.model.hop)
    _write_wav(ins, res["wav"].cpu().numpy(), out_path)
    if segments_out:
        with open(segments_out, "w") as fh:
            json.dump(dict(sample_rate=sr, hop=hop, n_samples=int(res["wav"].numel()),
                           segments=[dict(first_phone=g["first"], last_phone=g["last"], start_sample=g["start_frame"] * hop,
                                          n_samples=g["n_frames"] * hop,
                                          **({"pitch_retime_status": g["pitch_retime_status"]} if "pitch_retime_status" in g else {}))
                                     for g in res["segments"]]), fh, indent=1)
    return res


def main(argv=None):
    """`python -m stylesinger_amd.infer --exp-dir checkpoints/<exp> --vocoder-dir <hifigan dir> --emotion-ckpt <pt> --speaker-ckpt <pt>
    --phone-set ZH_checkpoint_phone_set.json [--ref-audio test/test.wav] [--out infer_out/test.wav] [--no-vad-trim | --vad {webrtc,lrt}]` = the reference's
    `python inference/StyleSinger.py` (StyleSingerInfer.example_run). `--pitch-audio guide.wav | --pitch-npy contour.npy [--pitch-shift semitones]`:
    sing the score on a given pitch contour instead of the predicted one; `--pitch-align dtw [--pitch-align-band-s 2.0]`: the contour is a guide
    with its own timing, warp it onto the score's notes (band in seconds around the linear fit, 0 = full) instead of scaling it linearly; `--pitch-timing guide`: the
    other way round - lay the score out on the guide's frames (note onsets where the guide has them) so that the result is in sync with the take.
    `--pitch-correct A`, `--vibrato-scale K`, `--vibrato-add RATE_HZ DEPTH_CENTS [--vibrato-delay-ms 250] [--vibrato-fade-ms 150]`, `--pitch-smooth-ms 333`:
    the pitch expression controls of forward (pull the pitch toward the notes, scale the vibrato, add one to held notes), with or without a contour. `--loud-norm`: loudness-normalise the reference audio as a model trained with
    hparams['loud_norm'] expects; `--out-lufs X`: write the result at X LUFS; `--out-true-peak DB [--out-lookahead-ms 2]`: hold the result under DB dBFS
    true peak with the look-ahead limiter (with --out-lufs the loudness gain is then applied in full instead of being divided by the peak); `--vocoder-denoise-c V`: the reference's vocoder output denoise (spectral
    subtraction of V, e.g. 0.1) after the generator, before the loudness target and the writer.
    `--ref-blend PATH WEIGHT` (repeatable) [`--ref-weight W`]: sing in a weighted blend of --ref-audio (weight W, default 1) and these references.
    `--score song.json [--max-seconds 12] [--segment-batch 8] [--fade-ms 5] [--segments-out timeline.json]`: sing a score of any length (the keys of
    example_input.json, optionally `ph_dur`; its `ref_audio` unless --ref-audio is given) with `sing_score`; pitch flags then need `ph_dur` in the score."""
    import argparse
    ap = argparse.ArgumentParser(description="StyleSinger example_run on the HIP path")
    ap.add_argument("--exp-dir", required=True)
    ap.add_argument("--vocoder-dir", required=True)
    ap.add_argument("--emotion-ckpt", required=True, help="the reference's emotion encoder checkpoint (hparams['emotion_encoder_path'])")
    ap.add_argument("--speaker-ckpt", required=True, help="resemblyzer's pretrained.pt")
    ap.add_argument("--phone-set", required=True)
    ap.add_argument("--ref-audio", help="the reference voice (default: the score file's ref_audio, else test/test.wav)")
    ap.add_argument("--ref-blend", nargs=2, action="append", metavar=("PATH", "WEIGHT"), help="one more reference voice and its weight (repeatable): "
                    "the style attention then runs over --ref-audio and these together, the weights as priors on it (not a linear mix of outputs), "
                    "and the speaker / emotion embeddings are the weighted, re-normalised means (rendered quality of such blends is unassessed)")
    ap.add_argument("--ref-weight", type=float, metavar="W", help="--ref-blend: the weight of --ref-audio itself (default 1.0)")
    ap.add_argument("--out", default="infer_out/test.wav")
    ap.add_argument("--no-vad-trim", action="store_true", help="explicit opt-out of trim_long_silences (webrtcvad missing)")
    ap.add_argument("--vad", choices=["webrtc", "lrt"], help="the voice-activity decision inside trim_long_silences: webrtc = the reference's (the "
                    "webrtcvad package on the host; the default), lrt = this project's own likelihood-ratio decision on the device (not webrtcvad's; "
                    "constants unassessed on recordings)")
    controls.add_flags(ap)   # the render controls: contour, pitch edit, f0 and mel sampler
    ap.add_argument("--loud-norm", action="store_true", help="hparams['loud_norm'] with loudness='bs1770': bring the reference audio to -22 LUFS first "
                    "(this project's BS.1770 meter; parity with pyloudnorm unpinned)")
    ap.add_argument("--out-lufs", type=float, help="write the result at this BS.1770 integrated loudness (hparams['out_loudness_lufs'])")
    ap.add_argument("--out-true-peak", type=float, metavar="DB", help="hold the result under this true-peak ceiling in dBFS (<= 0, e.g. -1) with the "
                    "look-ahead limiter on the device (hparams['out_true_peak_db']; this project's own 4x peak estimate, not a standard-conformant meter)")
    ap.add_argument("--out-lookahead-ms", type=float, metavar="MS", help="--out-true-peak: look-ahead and release window (hparams['out_limiter_lookahead_ms'], "
                    "default 2)")
    ap.add_argument("--vocoder-denoise-c", type=float, help="spectral subtraction of this magnitude on the vocoder's output "
                    "(hparams['vocoder_denoise_c'], e.g. 0.1; 0 = off)")
    ap.add_argument("--score", help="a score of any length as JSON (the keys of example_input.json, optionally ph_dur = seconds per phone): split at "
                    "its rests, rendered in batches, stitched on the device")
    ap.add_argument("--max-seconds", type=float, default=12.0, help="--score: longest merged segment")
    ap.add_argument("--segment-batch", type=int, default=8, help="--score: segments per batch")
    ap.add_argument("--fade-ms", type=float, default=5.0, help="--score: raised-cosine fade on both sides of every joint")
    ap.add_argument("--segments-out", help="--score: write the timeline (phone ranges and start samples per segment) to this JSON file")
    a = ap.parse_args(argv)
    if a.vad and a.no_vad_trim:
        ap.error("--vad and --no-vad-trim exclude each other")
    try:   # (against the default hparams; the instance checks again with the checkpoint's own)
        pitch, hp = controls.from_flags(a, DEFAULT_HPARAMS)
    except ValueError as e:
        ap.error(str(e).removeprefix("forward: "))
    if "pitch_hz" in pitch:
        pitch["pitch_hz"] = np.load(pitch["pitch_hz"])
    if a.ref_weight is not None and not a.ref_blend:
        ap.error("--ref-weight is the weight of --ref-audio among --ref-blend references; it needs --ref-blend")
    ref_blend = None
    if a.ref_blend:
        from .model import resolve_ref_weights
        try:
            weights = [1.0 if a.ref_weight is None else a.ref_weight] + [float(w) for _, w in a.ref_blend]
            resolve_ref_weights(weights, 1, len(weights))
        except ValueError as e:
            ap.error(f"--ref-blend / --ref-weight: {e}")
    score = None
    if a.score:
        with open(a.score) as fh:
            score = {k: v for k, v in json.load(fh).items() if k != "source"}
        if any(k in pitch for k in controls.CONTOUR_KEYS) and score.get("ph_dur") is None:
            ap.error("--score with a pitch flag needs 'ph_dur' (seconds per phone) in the score: without it the segment frame counts are not known "
                     "before rendering")
        score.update(pitch)   # (the edit keys apply per segment and need no ph_dur)
        from . import song
        try:
            song.check_pitch_keys(score)
        except ValueError as e:
            ap.error(str(e))
        if a.ref_audio or not score.get("ref_audio"):
            score["ref_audio"] = a.ref_audio or "test/test.wav"
        if a.ref_blend:   # the first reference is the one --ref-audio (or the score file) names
            score["ref_audios"], score["ref_weights"] = [score.pop("ref_audio")] + [p for p, _ in a.ref_blend], weights
    elif a.segments_out:
        ap.error("--segments-out needs --score")
    a.ref_audio = a.ref_audio or "test/test.wav"
    if a.ref_blend:
        ref_blend = ([a.ref_audio] + [p for p, _ in a.ref_blend], weights)
    emo = torch.load(a.emotion_ckpt, map_location="cpu", weights_only=False)
    spk = torch.load(a.speaker_ckpt, map_location="cpu", weights_only=False)
    if a.loud_norm:
        hp["loud_norm"] = True
    if a.out_lufs is not None:
        hp["out_loudness_lufs"] = a.out_lufs
    if a.out_lookahead_ms is not None and a.out_true_peak is None:
        ap.error("--out-lookahead-ms belongs to --out-true-peak")
    if a.out_true_peak is not None:
        from .limiter import ceiling_f32
        try:
            ceiling_f32(a.out_true_peak)   # (the window is checked against the model's sample rate by the constructor)
        except ValueError as e:
            ap.error(str(e))
        hp["out_true_peak_db"] = a.out_true_peak
        if a.out_lookahead_ms is not None:
            hp["out_limiter_lookahead_ms"] = a.out_lookahead_ms
    if a.vocoder_denoise_c is not None:
        hp["vocoder_denoise_c"] = a.vocoder_denoise_c
    ctor = dict(exp_dir=a.exp_dir, vocoder_dir=a.vocoder_dir, emotion_state=emo.get("model_state", emo),
                speaker_state=spk.get("model_state", spk), phone_set=a.phone_set, loudness="bs1770" if a.loud_norm else None)
    if score is not None:
        _score_run(score, hp or None, a.out, segments_out=a.segments_out, vad_flags=False if a.no_vad_trim else a.vad, max_seconds=a.max_seconds,
                   segment_batch=a.segment_batch, fade_ms=a.fade_ms, **ctor)
        return
    StyleSingerInfer.example_run(hp or None, a.ref_audio, a.out, vad_flags=False if a.no_vad_trim else a.vad, pitch=pitch, ref_blend=ref_blend, **ctor)


if __name__ == "__main__":
    main()
