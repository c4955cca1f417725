"""The input producers of `StyleSingerInfer` on the device: from reference audio to the dict `infer_batch` takes. `preprocess_batch` is
the batched form; `_device_batch`, `_pitch_inputs` and `preprocess_input` are the single-item forms of the reference's entry point that feed it.

`ReferenceProducers` is a mixin of the infer object (uses `self.hparams`, `self.device`, `self.ph_encoder`, the two encoders, the resolved loudness
switch and the front-end slots of the constructor)."""
import warnings

import numpy as np
import torch

from . import lib as L
from .audiofile import as_waveform
from .controls import from_input
from .resample import out_len, resample_batch


def has_features(inp):
    """`inp` already carries what the producers would make of inp['ref_audio']."""
    return all(k in inp for k in ("mel", "spk_embed", "emo_embed", "f0"))


def row(x, dtype):
    """One item's host values as a [1, ...] host tensor."""
    return torch.as_tensor(np.asarray(x), dtype=dtype)[None]


align_inputs = lambda inp, has_contour, sr, hop: from_input(inp, (sr, hop), has_contour)   # `controls.from_input` with the frame rate spelled out


class ReferenceProducers:
    """Mixin of StyleSingerInfer: the feature producers of `preprocess_input` on the device, batched and single-item."""

    def _mel_front(self):
        if self._mel_frontend is None:
            from .frontend import MelFrontendHIP
            self._mel_frontend = MelFrontendHIP(self._front_hparams, device=self.device)
        return self._mel_frontend

    def _emo_front(self):
        if self._emo_frontend is None:
            from .frontend import EmotionMelFrontendHIP
            self._emo_frontend = EmotionMelFrontendHIP(self.device)
        return self._emo_frontend

    @staticmethod
    def align_f0_to_mel(f0, n_mel, hop_size=256):
        """The tracker-output alignment of preprocess_input (inference/StyleSinger.py:120-136): left pad 2 * pad_size frames, right
        pad to the mel length, repeat the last value / crop when still off (|delta| <= 8 asserted there). numpy in, numpy out."""
        pad_size = {128: 4, 256: 2}[hop_size]
        f0 = np.asarray(f0)
        lpad = pad_size * 2
        rpad = n_mel - len(f0) - lpad
        f0 = np.pad(f0, [[lpad, max(rpad, 0)]], mode="constant") if rpad >= 0 else np.pad(f0, [[lpad, 0]], mode="constant")
        delta = n_mel - len(f0)
        assert abs(delta) <= 8, delta
        if delta > 0:
            f0 = np.concatenate([f0, [f0[-1]] * delta], 0)
        return f0[:n_mel]

    def _partials_batch(self, wavs, lens, slicer):
        """Shared front half of the two utterance encoders: per item zero-pad to the end of its last partial window, 40-mel power
        spectrogram of the whole batch (EmotionMelFrontendHIP: the same librosa.feature.melspectrogram parameters in both packages),
        gather the 160-frame partial windows of ALL items. -> (frames [sum P_b, 160, 40], counts [P_b])"""
        lens = [int(v) for v in lens]
        B = len(lens)
        slices = [slicer(n) for n in lens]
        need = [max(n, ws[-1].stop) for n, (ws, _) in zip(lens, slices)]   # `if max_wave_length >= len(wav): pad` (inference.py:129-131)
        buf = torch.zeros(B, max(need), device=self.device, dtype=torch.float32)
        buf[:, :wavs.shape[1]] = wavs.to(self.device).float()[:, :max(need)]
        mel40, _ = self._emo_front().wav2mel(buf, need)
        idx_b, idx_t = [], []
        counts = []
        for b, (_, ms) in enumerate(slices):
            counts.append(len(ms))
            for sl in ms:
                idx_b.append(torch.full((sl.stop - sl.start,), b, dtype=torch.long))
                idx_t.append(torch.arange(sl.start, sl.stop, dtype=torch.long))
        ib = torch.cat(idx_b).to(self.device)
        it = torch.cat(idx_t).to(self.device)
        frames = mel40[ib, it].reshape(sum(counts), 160, mel40.shape[-1]).contiguous()
        return frames, counts

    def _mean_l2norm_per_item(self, part, counts):
        out = torch.empty(len(counts), part.shape[1], device=self.device, dtype=torch.float32)
        o = 0
        for b, c in enumerate(counts):
            L.ops.ss_mean_l2norm(part[o:o + c], out[b], c, part.shape[1])
            o += c
        return out

    @torch.no_grad()
    def embed_emotion_batch(self, wavs, lens):
        """`Embed_utterance(wav, using_partials=True)` (data_gen/tts/emotion/inference.py:111-151) for a batch of PREPROCESSED
        waveforms (`preprocess_wav` output, zero beyond lens[b]; lens are host ints): per item zero-pad to the last partial's end,
        40-mel power spectrogram (EmotionMelFrontendHIP), the partial windows of ALL items through the LSTM in one pass, mean + L2
        norm per item. -> [B, 256] on the device."""
        from .emotion import compute_partial_slices
        if self.emotion_encoder is None:
            raise L.StyleSingerHipError("embed_emotion_batch: construct StyleSingerInfer(..., emotion_state=<emotion encoder state_dict>)")
        frames, counts = self._partials_batch(wavs, lens, compute_partial_slices)
        return self._mean_l2norm_per_item(self.emotion_encoder.embed_frames_batch(frames), counts)

    @torch.no_grad()
    def embed_speaker_batch(self, wavs, lens, rate=1.3, min_coverage=0.75):
        """`VoiceEncoder().embed_utterance(wav)` (inference/StyleSinger.py:100,104; resemblyzer 0.1.1.dev0, un-vendored: parity UNPINNED,
        `speaker.py`) for a batch of waveforms [B, L] (zero beyond lens[b]): partial windows of 160 frames every round(16000 / rate / 160)
        frames of the 40-mel, VoiceEncoder.forward on all of them in one pass (3 x LSTM, ReLU(Linear), L2 norm per partial), L2-normalised
        mean per item. The reference hands it the 48 kHz samples of `process_audio` rounded to float16 (:87,104) and the package reads
        them as 16 kHz audio - `preprocess_batch` reproduces exactly that. -> [B, 256] on the device."""
        from .speaker import compute_partial_slices as spk_slices
        if self.speaker_encoder is None:
            raise L.StyleSingerHipError("embed_speaker_batch: construct StyleSingerInfer(..., speaker_state=<resemblyzer model_state>)")
        frames, counts = self._partials_batch(wavs, lens, lambda n: spk_slices(n, rate, min_coverage))
        return self._mean_l2norm_per_item(self.speaker_encoder.forward(frames), counts)

    def _resample_refs(self, ref_wavs, ref_lens, ref_srs):
        """`librosa.core.load(..., sr=audio_sample_rate)`'s resampling for a batch with per-item rates: the items are grouped by rate, each group
        of another rate goes through `resample_batch` (one launch), and the results are scattered back in order. -> ([B, max new length] fp32,
        zero beyond each item's length; the new lengths as host ints)."""
        sr = int(self.hparams["audio_sample_rate"])
        srs = [int(r) for r in ref_srs]
        if len(srs) != ref_wavs.shape[0]:
            raise ValueError(f"preprocess_batch: {len(srs)} ref_srs for {ref_wavs.shape[0]} items")
        new_lens = [out_len(n, r, sr) for n, r in zip(ref_lens, srs)]
        out = torch.zeros(ref_wavs.shape[0], max(new_lens), device=ref_wavs.device, dtype=torch.float32)
        for rate in sorted(set(srs)):
            idx = [b for b, r in enumerate(srs) if r == rate]
            lens = [ref_lens[b] for b in idx]
            if rate == sr:
                sub, width = ref_wavs[idx], max(lens)
            else:
                sub, _ = resample_batch(ref_wavs[idx][:, :max(1, max(lens))], lens, rate, sr)
                width = sub.shape[1]
            out[idx, :width] = sub[:, :width]
        for b, n in enumerate(new_lens):   # an item at the model's rate keeps its samples; what the buffer held past them is padding
            if srs[b] == sr:
                out[b, n:] = 0
        return out, new_lens

    def process_audio_wav(self, ref_wavs, frames, valid_lens=None):
        """The waveform `process_audio` returns next to the mel (inference/StyleSinger.py:86-88): the audio zero-padded to
        n_mel * hop samples (utils/audios/__init__.py:76-78) and rounded to float16. -> ([B, max n_mel * hop] fp32 holding
        float16-representable values, zero beyond each item's length; lengths as host ints). `valid_lens`: the items' own sample
        counts - samples of the batch buffer past them are padding whatever they hold (as MelFrontendHIP.wav2mel treats them)."""
        hop = int(self.hparams["hop_size"])
        lens = [int(f) * hop for f in frames]
        x = ref_wavs.to(self.device).float().contiguous()
        out = torch.empty(x.shape[0], max(lens), device=self.device, dtype=torch.float32)
        n_out = torch.tensor(lens, dtype=torch.int32).to(self.device)
        n_in = None if valid_lens is None else torch.tensor([int(v) for v in valid_lens], dtype=torch.int32).to(self.device)
        L.ops.ss_round_f16_rows(x, x.shape[1], x.shape[1], n_in, n_out, out, out.shape[1], x.shape[0])
        for t_ in (n_out, n_in):
            if t_ is not None:
                t_.record_stream(torch.cuda.current_stream(self.device))
        return out, lens

    @torch.no_grad()
    def preprocess_batch(self, ref_wavs, ref_lens, spk_embed, f0_hz, txt_tokens, note, note_dur, note_type, mel2ph=None,
                         emo_embed=None, emo_wavs=None, emo_lens=None, emo_vad_flags=None, ref_srs=None, loud_norm=None):
        """Batched device form of `preprocess_input` + `input_to_batch` (inference/StyleSinger.py:94-172): from reference audio to
        the dict `infer_batch` takes, with no host round trip of the data.
          ref_wavs [B, L] fp32 reference audio (zero beyond ref_lens[b]; ref_lens host ints)          -> ref_mels  (process_audio, :106-118)
                   at the model's sample rate, or at the per-item rates `ref_srs` (host ints): items of another rate are resampled on the
                   device first, as `librosa.core.load(path, sr=audio_sample_rate)` does (utils/audios/__init__.py:52; `resample.py`, parity
                   UNPINNED), one launch per distinct rate; None or all equal to the model's rate = no resampling
          loud_norm None = the instance's resolved switch (hparams['loud_norm'] with `loudness="bs1770"`), or True / False: the audio at the model's
                   rate is brought to -22 LUFS and divided by its peak where that exceeds 1 (utils/audios/__init__.py:56-61; `loudness.py`, parity
                   with pyloudnorm UNPINNED) before the mel, the f0 tracker and the speaker encoder see it - what `process_audio` returns. The
                   default emotion branch keeps the un-normalised audio: `preprocess_wav(ref_audio)` reloads the file (:105)
          f0_hz    [B, Tr] tracker contour in Hz aligned to the mel frames (align_f0_to_mel), 0 = unvoiced -> ref_f0 (norm_interp_f0, :152);
                   None -> tracked on the device from `process_audio`'s waveform as :112-135 does with parselmouth (`f0track.py`: Praat's
                   published autocorrelation method, 80-800 Hz, voicing threshold 0.6; parity UNPINNED - parselmouth is un-vendored)
          emo_wavs [B, Le] `preprocess_wav` output for the emotion encoder (zero beyond emo_lens[b])  -> emo_embed (Embed_utterance, :104)
                   default: the reference audio itself, volume-normalised on the device. `trim_long_silences` (audio.py:58-100) runs on the
                   device AROUND the caller's decisions: pass `emo_vad_flags` [B, nW] = webrtcvad's `is_speech` per 30 ms window of the
                   volume-normalised 16-bit PCM (the decision itself is an un-vendored fixed-point GMM: `vadtrim.py`); without flags the
                   audio goes untrimmed; `emo_vad_flags="webrtc"` computes them on the host with the webrtcvad package from the device-normalised
                   audio (`vadtrim.webrtc_flags`: the reference's own call); `emo_vad_flags="lrt"` computes them on the device with this
                   project's own likelihood-ratio decision (`vadtrim.lrt_flags_device`, `ss_vad_lrt`: opt-in, NOT webrtcvad's decision, constants
                   unassessed on recordings), the audio never leaving the device. Pass `emo_embed` [B, 256] instead to skip this branch.
        The returned dict also carries `ref_f0_hz` [B, Tr] (the tracker's contour on the mel grid, before normalisation) for callers that mirror
        `preprocess_input`'s `inp['f0']`.
          spk_embed [B, 256], or None -> `VoiceEncoder().embed_utterance(wav)` (:100,104) on the device (`embed_speaker_batch`;
                   needs `speaker_state`) from what the reference hands it: `process_audio`'s waveform, i.e. the reference audio
                   zero-padded to n_mel * hop samples and rounded to float16 (:87; utils/audios/__init__.py:76-78)."""
        from .pitch import norm_interp_f0_device
        d, mel_front = self.device, self._mel_front()
        ref_lens_h = [int(v) for v in ref_lens]
        ref_wavs = ref_wavs.to(d).float()
        if ref_srs is not None and any(int(r) != int(self.hparams["audio_sample_rate"]) for r in ref_srs):
            ref_wavs, ref_lens_h = self._resample_refs(ref_wavs, ref_lens_h, ref_srs)
        raw_wavs = ref_wavs
        if self._loud_norm if loud_norm is None else loud_norm:
            from .loudness import normalize_batch
            ref_wavs, _ = normalize_batch(ref_wavs, ref_lens_h, int(self.hparams["audio_sample_rate"]))
        ref_mels, frames = mel_front.wav2mel(ref_wavs, torch.tensor(ref_lens_h, dtype=torch.int64))
        Tr = ref_mels.shape[1]
        hop = int(self.hparams["hop_size"])
        wav16 = None
        if f0_hz is None or spk_embed is None:   # the waveform the reference hands both third-party producers (:87)
            wav16, wav16_lens = self.process_audio_wav(ref_wavs, [n // hop + 1 for n in ref_lens_h], ref_lens_h)   # frames of a centred STFT
        if f0_hz is None:
            from .f0track import track_f0_device
            f0_hz = track_f0_device(wav16, wav16_lens, Tr, sr=int(self.hparams["audio_sample_rate"]), hop_size=hop)
        f0_hz = f0_hz.to(d).float()
        if f0_hz.shape[1] != Tr:
            raise ValueError(f"preprocess_batch: f0_hz has {f0_hz.shape[1]} frames, the reference mel {Tr} (use align_f0_to_mel)")
        ref_f0, _uv = norm_interp_f0_device(f0_hz, frames, self.hparams)
        if emo_embed is None:
            if emo_wavs is None:
                emo_wavs = self._emo_front().normalize_volume(raw_wavs, torch.tensor(ref_lens_h))
                emo_lens = ref_lens_h
                if isinstance(emo_vad_flags, str):
                    if emo_vad_flags not in ("webrtc", "lrt"):
                        raise ValueError(f"emo_vad_flags={emo_vad_flags!r}: expected flags, None, 'webrtc' or 'lrt'")
                    from .vadtrim import lrt_flags_device, webrtc_flags
                    # "lrt": the audio stays on the device between normalize_volume and ss_vad_trim
                    emo_vad_flags = webrtc_flags(emo_wavs, emo_lens) if emo_vad_flags == "webrtc" else lrt_flags_device(emo_wavs, emo_lens)[0]
                if emo_vad_flags is not None:   # preprocess_wav's second step (audio.py:38), around the VAD flags
                    from .vadtrim import trim_long_silences_device
                    emo_wavs, kept = trim_long_silences_device(emo_wavs, emo_lens, emo_vad_flags)
                    emo_lens = [int(v) for v in kept.cpu()]   # the partial slicing below is host arithmetic on the lengths
            emo_embed = self.embed_emotion_batch(emo_wavs, emo_lens)
        if spk_embed is None:
            spk_embed = self.embed_speaker_batch(wav16, wav16_lens)
        batch = dict(txt_tokens=txt_tokens.to(d), note=note.to(d), note_dur=note_dur.to(d).float(), note_type=note_type.to(d),
                     spk_embed=spk_embed.to(d).float(), emo_embed=emo_embed.to(d).float(), ref_mels=ref_mels, ref_f0=ref_f0, ref_f0_hz=f0_hz)
        if mel2ph is not None:
            batch["mel2ph"] = mel2ph.to(d)
        return batch

    _warned_untrimmed = False

    def _resolve_vad(self, vad_flags):
        """`preprocess_wav` ALWAYS trims long silences (data_gen/tts/emotion/audio.py:36-38). None = do as the reference does: webrtcvad's decisions,
        computed on the host - an ImportError where the package is missing (it is un-vendored), never a silent skip. False = explicit opt-out
        (untrimmed audio; warns once: the emotion embedding of a recording with long pauses then differs from the reference's). Otherwise the
        caller's flags [nW], or a decision by name: "webrtc" (as None, asked for explicitly) or "lrt" (this project's own likelihood-ratio decision
        on the device, `vadtrim.lrt_flags_device`: opt-in, not webrtcvad's). None resolves to the instance's `vad` (StyleSingerInfer(vad=...)) when
        that is set."""
        if vad_flags is None:
            vad_flags = getattr(self, "vad", None)   # (an instance made with __new__ has no attribute: the reference's behaviour)
        if vad_flags is None:
            from .vadtrim import have_webrtcvad
            if not have_webrtcvad():
                raise ImportError("preprocess_input: the reference trims long silences with webrtcvad before the emotion encoder, and the package is "
                                  "not importable here. Pass vad_flags=<webrtcvad's is_speech per 30 ms window> or vad_flags=False to skip the trim "
                                  "explicitly (the emotion embedding then differs from the reference's for audio with long pauses), or "
                                  "vad_flags=\"lrt\" for this project's own on-device decision (not webrtcvad's).")
            return "webrtc"
        if isinstance(vad_flags, str):
            if vad_flags not in ("webrtc", "lrt"):
                raise ValueError(f"vad_flags={vad_flags!r}: expected flags, None, False, 'webrtc' or 'lrt'")
            return vad_flags
        if vad_flags is False:
            if not type(self)._warned_untrimmed:   # on the instance's own class: that is where callers reset it
                type(self)._warned_untrimmed = True
                warnings.warn("StyleSingerInfer: trim_long_silences skipped on request (vad_flags=False): emo_embed is computed from untrimmed audio")
            return None
        return np.asarray(vad_flags)[None]

    @torch.no_grad()
    def _device_batch(self, inp, vad_flags=None):
        """`preprocess_input` + `input_to_batch` (inference/StyleSinger.py:94-172) for ONE item with every producer on the device: the dict
        `infer_batch` takes, device tensors only (+ `ref_f0_hz`, `n_mel`, `wav_fn`). ONE pass of the f0 tracker."""
        sr, hop = int(self.hparams["audio_sample_rate"]), int(self.hparams["hop_size"])
        if inp.get("ref_audios") is not None:
            return self._device_batch_pool(inp, vad_flags)
        if inp.get("ref_weights") is not None or inp.get("ref_srs") is not None:
            raise ValueError("preprocess_input: inp['ref_weights'] / inp['ref_srs'] belong to inp['ref_audios'] (a list of references)")
        wav, in_sr, path = as_waveform(inp["ref_audio"], inp.get("ref_sr") or sr, "ref_audio")
        if "ph_token" not in inp:
            if self.ph_encoder is None:
                raise ValueError("preprocess_input: give inp['ph_token'], construct StyleSingerInfer(..., phone_set=<phone_set.json>) or set "
                                 "self.ph_encoder (the reference's build_token_encoder(f'{processed_data_dir}/phone_set.json'))")
            inp["ph_token"] = self.ph_encoder.encode(" ".join(inp["ph"]))
        # librosa.core.load(wav_path, sr=audio_sample_rate) (utils/audios/__init__.py:52): the samples go to the device once and are resampled there
        batch = self.preprocess_batch(torch.from_numpy(np.ascontiguousarray(wav))[None], [len(wav)], None, None, row(inp["ph_token"], torch.long),
                                      row(inp["note"], torch.long), row(inp["note_dur"], torch.float32), row(inp["note_type"], torch.long),
                                      mel2ph=row(inp["mel2ph"], torch.long) if "mel2ph" in inp else None, emo_vad_flags=self._resolve_vad(vad_flags),
                                      ref_srs=[in_sr])
        batch["n_mel"], batch["wav_fn"] = out_len(len(wav), in_sr, sr) // hop + 1, path
        batch.update(self._pitch_inputs(inp))
        return batch

    @torch.no_grad()
    def _device_batch_pool(self, inp, vad_flags=None):
        """`_device_batch` for a POOL of references: inp['ref_audios'] = a list of R entries, each whatever `as_waveform` accepts (a list under
        'ref_audio' could not say this: a (waveform, sample_rate) pair already means one clip there), inp['ref_srs'] = optional rates of bare
        arrays (one per entry, None = the model's), inp['ref_weights'] = optional R weights >= 0 (default equal; `model.resolve_ref_weights`).
        The R clips go through `preprocess_batch` ONCE, as a batch of R. -> the dict `infer_batch` takes with `ref_mels` [1, R, Tr, 80],
        `ref_f0` [1, R, Tr], `ref_weights` (the normalised weights, host float64 [1, R]) and `spk_embed` / `emo_embed` [1, 256] = the
        weighted, re-normalised means of the clips' embeddings (`model.blend_embeds`); `n_mel` / `wav_fn` are lists of R."""
        from .model import blend_embeds, resolve_ref_weights
        sr, hop = int(self.hparams["audio_sample_rate"]), int(self.hparams["hop_size"])
        if inp.get("ref_audio") is not None:
            raise ValueError("preprocess_input: give inp['ref_audio'] (one reference) or inp['ref_audios'] (a list of references), not both")
        if inp.get("ref_sr") is not None:
            raise ValueError("preprocess_input: with inp['ref_audios'] the rates of bare arrays go in inp['ref_srs'] (one per reference), not inp['ref_sr']")
        auds = inp["ref_audios"]
        if not isinstance(auds, (list, tuple)) or len(auds) < 1:
            raise ValueError("preprocess_input: inp['ref_audios'] must be a non-empty list of references (WAV paths, (waveform, sample_rate) pairs or arrays)")
        R = len(auds)
        srs = inp.get("ref_srs")
        if srs is not None and len(srs) != R:
            raise ValueError(f"preprocess_input: {len(srs)} inp['ref_srs'] for {R} inp['ref_audios']")
        _logw, p = resolve_ref_weights(inp.get("ref_weights"), 1, R)   # a bad weight is refused before a file is read or a device touched
        vad = self._resolve_vad(vad_flags)
        if vad is not None and not isinstance(vad, str):
            raise ValueError("preprocess_input: vad_flags as an array describes ONE clip; with inp['ref_audios'] give None, False, 'webrtc' or 'lrt'")
        clips = [as_waveform(a, (srs[i] if srs is not None and srs[i] else sr), f"ref_audios[{i}]") for i, a in enumerate(auds)]
        lens = [len(w) for w, _, _ in clips]
        if min(lens) < 1:
            raise ValueError(f"preprocess_input: inp['ref_audios'][{lens.index(min(lens))}] is empty")
        wavs = np.zeros((R, max(lens)), dtype=np.float32)
        for i, (w, _, _) in enumerate(clips):
            wavs[i, :len(w)] = w
        if "ph_token" not in inp:
            if self.ph_encoder is None:
                raise ValueError("preprocess_input: give inp['ph_token'], construct StyleSingerInfer(..., phone_set=<phone_set.json>) or set "
                                 "self.ph_encoder (the reference's build_token_encoder(f'{processed_data_dir}/phone_set.json'))")
            inp["ph_token"] = self.ph_encoder.encode(" ".join(inp["ph"]))
        in_srs = [r for _, r, _ in clips]
        batch = self.preprocess_batch(torch.from_numpy(wavs), lens, None, None, row(inp["ph_token"], torch.long), row(inp["note"], torch.long),
                                      row(inp["note_dur"], torch.float32), row(inp["note_type"], torch.long),
                                      mel2ph=row(inp["mel2ph"], torch.long) if "mel2ph" in inp else None, emo_vad_flags=vad, ref_srs=in_srs)
        batch["spk_embed"] = blend_embeds(batch["spk_embed"][None], p)
        batch["emo_embed"] = blend_embeds(batch["emo_embed"][None], p)
        batch["ref_mels"], batch["ref_f0"], batch["ref_f0_hz"] = batch["ref_mels"][None], batch["ref_f0"][None], batch["ref_f0_hz"][None]
        batch["ref_weights"] = p
        batch["n_mel"], batch["wav_fn"] = [out_len(n, r, sr) // hop + 1 for n, r in zip(lens, in_srs)], [path for _, _, path in clips]
        batch.update(self._pitch_inputs(inp))
        return batch

    def _pitch_inputs(self, inp):
        """The pitch-control entries of `inp` as `infer_batch` takes them: inp['pitch_hz'] (a 1-D contour in Hz at the mel hop, 0 = unvoiced) or
        inp['pitch_audio'] (a WAV path or a (waveform, sample_rate) pair: a guide vocal, resampled like `ref_audio` and tracked on the device as
        `preprocess_batch` tracks the reference audio, 80-800 Hz), and inp['pitch_shift'] (semitones). inp['pitch_align'] = "dtw" (+
        inp['pitch_align_band_s'], seconds, default controls.ALIGN_BAND_S, 0 = full) asks for the warp of forward(pitch_align=): -> `pitch_align` and
        `pitch_align_band` = round(s * audio_sample_rate / hop_size) guide frames. inp['pitch_timing'] = "guide" asks for forward(pitch_timing=):
        the score sung in the guide's timing (the contour must be on the mel hop grid, as a tracked `pitch_audio` is) -> `pitch_timing` and the
        band. inp['pitch_correct' | 'vibrato_scale' | 'vibrato_add' | 'pitch_smooth_ms'] (the pitch expression controls of forward; they need no
        contour) pass through. The rules and the mapping are `controls.from_input`'s; the tracking and the upload are done here. -> {} when `inp` has none of them."""
        out = from_input(inp, self.hparams, inp.get("pitch_hz") is not None or inp.get("pitch_audio") is not None)   # the rules, before any tracking
        if inp.get("pitch_hz") is not None:
            hz = torch.as_tensor(np.asarray(inp["pitch_hz"], dtype=np.float32))
            if hz.dim() != 1 or hz.numel() == 0:
                raise ValueError(f"preprocess_input: inp['pitch_hz'] must be a non-empty 1-D contour in Hz (got shape {tuple(hz.shape)})")
            out["pitch_hz"] = (hz[None].to(self.device), [hz.numel()])
        elif inp.get("pitch_audio") is not None:
            from .f0track import track_f0_device
            sr, hop = int(self.hparams["audio_sample_rate"]), int(self.hparams["hop_size"])
            wav, in_sr, _path = as_waveform(inp["pitch_audio"], None, "pitch_audio")   # no default rate: a bare array is refused
            gv, n = torch.from_numpy(np.ascontiguousarray(wav))[None].to(self.device), len(wav)
            gv, (n,) = resample_batch(gv, [n], in_sr, sr)   # (equal rates: returned untouched)
            n_mel = n // hop + 1
            wav16, wav16_lens = self.process_audio_wav(gv, [n_mel], [n])
            out["pitch_hz"] = (track_f0_device(wav16, wav16_lens, n_mel, sr=sr, hop_size=hop), [n_mel])
        return out

    @torch.no_grad()
    def preprocess_input(self, inp, vad_flags=None):
        """Mirror of `StyleSingerInfer.preprocess_input` (inference/StyleSinger.py:94-137) with every producer on the device: fills `mel`,
        `spk_embed`, `emo_embed`, `f0` (the tracker's contour in Hz on the mel grid) as numpy arrays, `ph_token`, and `item_name` / `wav_fn` from
        `inp['ref_audio']`: the path of a WAV file (`audiofile.load_audio`: PCM or float, any channel count, any sample rate), a float waveform at
        `inp['ref_sr']` Hz (default: the model's sample rate) or a `(waveform, sample_rate)` pair; audio of another rate is resampled on the device as
        `librosa.core.load(wav_path, sr=audio_sample_rate)` does (`resample.py`; parity with librosa UNPINNED). Needs `emotion_state` and
        `speaker_state` (the two encoders' checkpoints). `vad_flags`: see `_resolve_vad` (None = webrtcvad on the host unless the instance was made with `vad=`,
        False = opt out, "lrt" = this project's own decision on the device).
        Pitch control (`_pitch_inputs`): `inp['pitch_hz']` / `inp['pitch_shift']` pass through; `inp['pitch_audio']` (a guide vocal) is tracked
        on the device and replaced by its contour in `inp['pitch_hz']`.
        One reference only, as in the reference: a pool (`inp['ref_audios']`) has no single `mel` / `f0` to return - use `infer_once`."""
        if inp.get("ref_audios") is not None:
            raise ValueError("preprocess_input mirrors the reference's single-reference dict (mel, f0, spk_embed, emo_embed of ONE clip); "
                             "inp['ref_audios'] (a pool of references) goes through infer_once or sing_score")
        batch = self._device_batch(inp, vad_flags)
        n_mel = batch["n_mel"]
        inp.update(item_name=inp.get("name"), wav_fn=batch["wav_fn"],
                   mel=batch["ref_mels"][0, :n_mel].cpu().numpy(), spk_embed=batch["spk_embed"][0].cpu().numpy(),
                   emo_embed=batch["emo_embed"][0].cpu().numpy(), f0=batch["ref_f0_hz"][0, :n_mel].double().cpu().numpy())
        if inp.get("pitch_audio") is not None:   # tracked once, here: the contour replaces the audio entry
            inp["pitch_hz"] = batch["pitch_hz"][0][0].cpu().numpy()
            del inp["pitch_audio"]
        return inp
