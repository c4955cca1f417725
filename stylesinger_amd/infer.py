"""Inference entrypoint of the HIP path: mirror of `inference/StyleSinger.py::StyleSingerInfer`.

`StyleSingerInfer(hparams).forward_model(inp)` keeps the reference's single-utterance contract
(inference/StyleSinger.py:41-63: run the model, drop all-zero frames, clip the mel to
[mel_vmin, mel_vmax], vocode with the predicted f0).  `infer_batch` is the batched, device-resident
form the benchmark and the data-parallel driver use.  The feature extractors of `preprocess_input`
(:94-137) run on the device: `preprocess_batch` computes the reference mel, the emotion embedding, the speaker
embedding (resemblyzer's published algorithm on the emotion encoder's kernels, `speaker.py`; parity unpinned: un-vendored package),
the f0 contour (Praat's autocorrelation method, `f0track.py`; parity unpinned: parselmouth is un-vendored) and its normalisation.
`trim_long_silences` runs on the device AROUND webrtcvad's per-window decisions (a fixed-point GMM whose tables are not in the reference tree):
they are computed on the host when the package is importable, or given by the caller; skipping the trim is an explicit opt-out
(`vad_flags=False`), never a silent default.
`infer_once(inp)` = the reference's entry point (inference/StyleSinger.py:175-179) with the features kept on the device between the producers and
the model; `python -m stylesinger_amd.infer` = `example_run` (:181-331).
`sing_score(inp)` (`--score song.json`) sings a score of any length: split at its rests (`song.py`), rendered as batches, stitched on the device.
"""
import json
import os
import warnings

import numpy as np
import torch

from . import lib as L
from .config import make_hparams, make_vocoder_config
from .model import StyleSingerHIP
from .vocoder import get_vocoder_cls


class StyleSingerInfer:
    def __init__(self, hparams=None, device=None, model_state=None, vocoder_state=None, vocoder_config=None, dictionary=None,
                 emotion_state=None, speaker_state=None, phone_set=None, loudness=None):
        """`loudness`: "bs1770" = honour hparams['loud_norm'] with this project's BS.1770 meter (`loudness.py`; parity with pyloudnorm UNPINNED, so
        the bare flag stays refused: `loudness.resolve_loudness`).
        `emotion_state`: state_dict of the reference's emotion encoder checkpoint (`EmotionEncoder.load_model`,
        inference/StyleSinger.py:101) - enables the emotion branch of `preprocess_batch`.
        `speaker_state`: `model_state` of resemblyzer's `pretrained.pt` (`VoiceEncoder()`, inference/StyleSinger.py:100) - enables the
        speaker branch."""
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
        if self.hparams.get("out_loudness_lufs") is not None and (self.hparams.get("out_wav_norm") or (hparams or {}).get("out_wav_norm")):
            raise ValueError("hparams: out_loudness_lufs and out_wav_norm exclude each other (a loudness target or peak normalisation, not both)")
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
    def from_checkpoints(cls, hparams, exp_dir, vocoder_dir, device=None, dictionary=None, loudness=None):
        """Build from the reference's on-disk checkpoints (inference/StyleSinger.py:34-39 + hifigan_nsf.py:46-61):
        `exp_dir` = checkpoints/<exp_name> (newest model_ckpt_steps_*.ckpt), `vocoder_dir` = hparams['vocoder_ckpt']."""
        from . import ckpt
        state, _ = ckpt.read_state(exp_dir, "model")
        if state is None:
            raise FileNotFoundError(f"| ckpt not found in {exp_dir}.")
        vstate, vcfg = ckpt.load_vocoder_ckpt(vocoder_dir)
        return cls(hparams, device=device, model_state=state, vocoder_state=vstate, vocoder_config=vcfg, dictionary=dictionary, loudness=loudness)

    def build_model(self, dictionary=None, state=None):
        model = StyleSingerHIP(dictionary, hparams=self.hparams)
        if state is not None:
            model.load_state_dict(state, strict=False)
        return model

    # ---- batched, device resident -------------------------------------------------------------
    @torch.no_grad()
    def infer_batch(self, batch, noise=None, vocoder_noise=None, seed=None, vocode=True, plan_slot=0, out_lufs=None):
        """batch: dict of device tensors (txt_tokens, note, note_dur, note_type, spk_embed, emo_embed, ref_mels,
        ref_f0, optional mel2ph).  Returns dict(mel [B,T,80], f0 [B,T], lens int32 [B], wav [B,T*hop]).
        Pitch control (StyleSingerHIP.forward): optional `f0` + `uv` [B, T] (the normalised contour, the reference's use_gt_f0 form), or
        `pitch_hz` = (contour in Hz [B, Lc], lens_c) with optional `pitch_shift` (semitones); without them the f0 is predicted.
        `out_lufs`: bring every item of `wav` to this BS.1770 integrated loudness (`_to_lufs`; adds res['lufs'], the loudness before the gain).
        Optional `style_cache`: what `model.encode_style` returned for the batch's references; the style encoder is then skipped."""
        hp = self.hparams
        seed = hp["seed"] if seed is None else seed
        pitch = {k: batch[k] for k in ("pitch_hz", "pitch_shift") if batch.get(k) is not None}
        if batch.get("style_cache") is not None:   # the references' style, encoded once by the caller (model.encode_style; `sing_score`)
            pitch["style_cache"] = batch["style_cache"]
        out = self.model(batch["txt_tokens"], mel2ph=batch.get("mel2ph"), spk_embed=batch["spk_embed"], emo_embed=batch["emo_embed"],
                         ref_mels=batch["ref_mels"], ref_f0=batch["ref_f0"], f0=batch.get("f0"), uv=batch.get("uv"), global_steps=320000,
                         infer=True, note=batch["note"], note_dur=batch["note_dur"], note_type=batch["note_type"], noise=noise, seed=seed,
                         plan_slot=plan_slot, **pitch)
        res = dict(mel=out["mel_out"], f0=out["f0_denorm"], lens=out["lens"], model_out=out)
        if vocode:
            res["wav"] = self.vocode(out["mel_out"], out["f0_denorm"], out["lens"], noise=vocoder_noise, seed=seed + 101)
            if out_lufs is not None:
                res["wav"], res["lufs"] = self._to_lufs(res["wav"], [int(v) * self.vocoder.model.hop for v in out["lens"].cpu()], out_lufs)
        return res

    def _to_lufs(self, wav, lens, target):
        """The output loudness target (hparams['out_loudness_lufs'], `infer_batch(out_lufs=)`): wav [B, L] on the device, lens host ints ->
        (every item at `target` LUFS, divided by its peak where that exceeds 1; lufs [B] float64 = the loudness measured before the gain). An
        item shorter than one 0.4 s gating block has no loudness: it is returned untouched (lufs NaN), with one warning per call."""
        from .loudness import normalize_batch
        y, m = normalize_batch(wav, lens, int(self.hparams["audio_sample_rate"]), target=float(target), short="skip")
        if 0 in m["n_blocks"]:
            warnings.warn(f"out_loudness_lufs: {m['n_blocks'].count(0)} item(s) shorter than one 0.4 s gating block left at their own level")
        return y, m["lufs"]

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
        for i, batch in enumerate(batches):
            need = max(int(batch["mel2ph"].shape[1]) if batch.get("mel2ph") is not None else 0, int(batch["ref_mels"].shape[1]))
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
        hp = self.hparams
        mel_c = torch.empty_like(mel)
        L.check(L.load().ss_clip(L.ptr(mel), L.ptr(mel_c), mel.numel(), float(hp["mel_vmin"]), float(hp["mel_vmax"]), L.stream_ptr()), "ss_clip")
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
        res = self.infer_batch(batch, seed=seed, out_lufs=self.hparams.get("out_loudness_lufs"))
        self.model.check_finite(res["model_out"])
        hop = self.vocoder.model.hop
        pcm = wav_to_pcm16(res["wav"], res["lens"], hop, norm=bool(self.hparams.get("out_wav_norm", False)))
        writer.submit_batch(names, pcm, res["lens"], hop)
        return res

    # ---- input producers on the device ------------------------------------------
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
        from .frontend import EmotionMelFrontendHIP
        if self._emo_frontend is None:
            self._emo_frontend = EmotionMelFrontendHIP(self.device)
        lens = [int(v) for v in lens]
        B = len(lens)
        slices = [slicer(n) for n in lens]
        need = [max(n, ws[-1].stop) for n, (ws, _) in zip(lens, slices)]   # `if max_wave_length >= len(wav): pad` (inference.py:129-131)
        buf = torch.zeros(B, max(need), device=self.device, dtype=torch.float32)
        buf[:, :wavs.shape[1]] = wavs.to(self.device).float()[:, :max(need)]
        mel40, _ = self._emo_frontend.wav2mel(buf, need)
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
        lib, o = L.load(), 0
        for b, c in enumerate(counts):
            L.check(lib.ss_mean_l2norm(L.ptr(part[o:o + c]), L.ptr(out[b]), c, part.shape[1], L.stream_ptr()), "ss_mean_l2norm")
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
        from .resample import out_len, resample_batch
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
        L.check(L.load().ss_round_f16_rows(L.ptr(x), x.shape[1], x.shape[1], L.ptr(n_in), L.ptr(n_out), L.ptr(out), out.shape[1], x.shape[0], L.stream_ptr()),
                "ss_round_f16_rows")
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
                   audio (`vadtrim.webrtc_flags`: the reference's own call). Pass `emo_embed` [B, 256] instead to skip this branch.
        The returned dict also carries `ref_f0_hz` [B, Tr] (the tracker's contour on the mel grid, before normalisation) for callers that mirror
        `preprocess_input`'s `inp['f0']`.
          spk_embed [B, 256], or None -> `VoiceEncoder().embed_utterance(wav)` (:100,104) on the device (`embed_speaker_batch`;
                   needs `speaker_state`) from what the reference hands it: `process_audio`'s waveform, i.e. the reference audio
                   zero-padded to n_mel * hop samples and rounded to float16 (:87; utils/audios/__init__.py:76-78)."""
        from .frontend import MelFrontendHIP
        from .pitch import norm_interp_f0_device
        d = self.device
        if self._mel_frontend is None:
            self._mel_frontend = MelFrontendHIP(self._front_hparams, device=d)
        ref_lens_h = [int(v) for v in ref_lens]
        ref_wavs = ref_wavs.to(d).float()
        if ref_srs is not None and any(int(r) != int(self.hparams["audio_sample_rate"]) for r in ref_srs):
            ref_wavs, ref_lens_h = self._resample_refs(ref_wavs, ref_lens_h, ref_srs)
        raw_wavs = ref_wavs
        if self._loud_norm if loud_norm is None else loud_norm:
            from .loudness import normalize_batch
            ref_wavs, _ = normalize_batch(ref_wavs, ref_lens_h, int(self.hparams["audio_sample_rate"]))
        ref_mels, frames = self._mel_frontend.wav2mel(ref_wavs, torch.tensor(ref_lens_h, dtype=torch.int64))
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
                if self._emo_frontend is None:
                    from .frontend import EmotionMelFrontendHIP
                    self._emo_frontend = EmotionMelFrontendHIP(d)
                emo_wavs = self._emo_frontend.normalize_volume(raw_wavs, torch.tensor(ref_lens_h))
                emo_lens = ref_lens_h
                if isinstance(emo_vad_flags, str):
                    if emo_vad_flags != "webrtc":
                        raise ValueError(f"emo_vad_flags={emo_vad_flags!r}: expected flags, None or 'webrtc'")
                    from .vadtrim import webrtc_flags
                    emo_vad_flags = webrtc_flags(emo_wavs, emo_lens)
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

    # ---- the reference's single-utterance surface ---------------------------------------------
    def input_to_batch(self, item):
        """inference/StyleSinger.py:139-172: `item['f0']` is the tracker's contour in Hz (0 = unvoiced) and goes through
        `norm_interp_f0` (utils/pitch_utils.py:47-62) exactly as there (:152)."""
        from .pitch import norm_interp_f0
        d = self.device
        t = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt)[None].to(d)
        f0, _uv = norm_interp_f0(np.asarray(item["f0"]), self.hparams)
        return dict(txt_tokens=t(item["ph_token"], torch.long), ref_mels=t(item["mel"], torch.float32),
                    spk_embed=t(item["spk_embed"], torch.float32), emo_embed=t(item["emo_embed"], torch.float32),
                    note=t(item["note"], torch.long), note_dur=t(item["note_dur"], torch.float32),
                    note_type=t(item["note_type"], torch.long), ref_f0=f0[None].to(d),
                    **({"mel2ph": t(item["mel2ph"], torch.long)} if "mel2ph" in item else {}), **self._pitch_inputs(item))

    def _wav_from_result(self, res, vocoder_noise=None):
        """inference/StyleSinger.py:53-63: drop all-zero frames, clip the mel, vocode with the predicted f0 (one item)."""
        mel_pred = res["mel"].cpu().numpy()
        self.model.check_finite(res["model_out"])   # (the copy above synchronised)
        f0_pred = res["f0"].cpu().numpy()
        mask = np.abs(mel_pred).sum(-1) > 0
        mel_pred = np.clip(mel_pred[mask], self.hparams["mel_vmin"], self.hparams["mel_vmax"])
        f0_pred = f0_pred[mask]
        return self.vocoder.spec2wav(mel_pred, f0=f0_pred, noise=vocoder_noise)

    def forward_model(self, inp, noise=None, vocoder_noise=None):
        sample = self.input_to_batch(inp)
        return self._wav_from_result(self.infer_batch(sample, noise=noise, vocoder_noise=None, vocode=False), vocoder_noise)

    @staticmethod
    def _load_wav(path, want_sr):
        """The strict static loader: a 16-bit PCM WAV at exactly `want_sr` Hz -> float32 mono in [-1, 1); anything else is a ValueError.
        (`preprocess_input` reads files through `audiofile.load_audio` + `resample.resample_batch`, which take other formats and rates.)"""
        import wave
        with wave.open(os.fsdecode(path), "rb") as wf:
            if wf.getsampwidth() != 2 or wf.getframerate() != want_sr:
                raise ValueError(f"{path}: need 16-bit PCM at {want_sr} Hz (got {8 * wf.getsampwidth()} bit, {wf.getframerate()} Hz)")
            pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2").astype(np.float32).reshape(-1, wf.getnchannels())
        return pcm.mean(axis=1) / 32768.0

    _warned_untrimmed = False

    def _resolve_vad(self, vad_flags):
        """`preprocess_wav` ALWAYS trims long silences (data_gen/tts/emotion/audio.py:36-38). None = do as the reference does: webrtcvad's decisions,
        computed on the host - an ImportError where the package is missing (it is un-vendored), never a silent skip. False = explicit opt-out
        (untrimmed audio; warns once: the emotion embedding of a recording with long pauses then differs from the reference's). Otherwise the
        caller's flags [nW]."""
        if vad_flags is None:
            from .vadtrim import have_webrtcvad
            if not have_webrtcvad():
                raise ImportError("preprocess_input: the reference trims long silences with webrtcvad before the emotion encoder, and the package is "
                                  "not importable here. Pass vad_flags=<webrtcvad's is_speech per 30 ms window> or vad_flags=False to skip the trim "
                                  "explicitly (the emotion embedding then differs from the reference's for audio with long pauses).")
            return "webrtc"
        if vad_flags is False:
            if not StyleSingerInfer._warned_untrimmed:
                StyleSingerInfer._warned_untrimmed = True
                warnings.warn("StyleSingerInfer: trim_long_silences skipped on request (vad_flags=False): emo_embed is computed from untrimmed audio")
            return None
        return np.asarray(vad_flags)[None]

    @torch.no_grad()
    def _device_batch(self, inp, vad_flags=None):
        """`preprocess_input` + `input_to_batch` (inference/StyleSinger.py:94-172) for ONE item with every producer on the device: the dict
        `infer_batch` takes, device tensors only (+ `ref_f0_hz`, `n_mel`). ONE pass of the f0 tracker."""
        sr, hop = int(self.hparams["audio_sample_rate"]), int(self.hparams["hop_size"])
        audio, in_sr = inp["ref_audio"], int(inp.get("ref_sr") or sr)
        if isinstance(audio, (str, bytes)) or hasattr(audio, "__fspath__"):
            from .audiofile import load_audio
            wav, in_sr = load_audio(audio)
        elif isinstance(audio, (tuple, list)) and len(audio) == 2 and np.ndim(audio[1]) == 0 and np.ndim(audio[0]) == 1:
            wav, in_sr = np.asarray(audio[0], dtype=np.float32), int(audio[1])       # (waveform, sample_rate)
        else:
            wav = np.asarray(audio, dtype=np.float32)
        ref, n = torch.from_numpy(np.ascontiguousarray(wav))[None], len(wav)
        if in_sr != sr:   # librosa.core.load(wav_path, sr=audio_sample_rate) (utils/audios/__init__.py:52): the samples go to the device once
            from .resample import resample_batch
            ref, (n,) = resample_batch(ref.to(self.device), [n], in_sr, sr)
        if "ph_token" not in inp:
            if self.ph_encoder is None:
                raise ValueError("preprocess_input: give inp['ph_token'], construct StyleSingerInfer(..., phone_set=<phone_set.json>) or set "
                                 "self.ph_encoder (the reference's build_token_encoder(f'{processed_data_dir}/phone_set.json'))")
            inp["ph_token"] = self.ph_encoder.encode(" ".join(inp["ph"]))
        t = lambda x, dt: torch.as_tensor(np.asarray(x), dtype=dt)[None]
        batch = self.preprocess_batch(ref, [n], None, None, t(inp["ph_token"], torch.long), t(inp["note"], torch.long),
                                      t(inp["note_dur"], torch.float32), t(inp["note_type"], torch.long),
                                      mel2ph=t(inp["mel2ph"], torch.long) if "mel2ph" in inp else None, emo_vad_flags=self._resolve_vad(vad_flags))
        batch["n_mel"] = n // hop + 1
        batch.update(self._pitch_inputs(inp))
        return batch

    def _pitch_inputs(self, inp):
        """The pitch-control entries of `inp` as `infer_batch` takes them: inp['pitch_hz'] (a 1-D contour in Hz at the mel hop, 0 = unvoiced) or
        inp['pitch_audio'] (a WAV path or a (waveform, sample_rate) pair: a guide vocal, resampled like `ref_audio` and tracked on the device as
        `preprocess_batch` tracks the reference audio, 80-800 Hz), and inp['pitch_shift'] (semitones). -> {} when `inp` has none of them."""
        if inp.get("pitch_hz") is not None and inp.get("pitch_audio") is not None:
            raise ValueError("preprocess_input: give inp['pitch_hz'] or inp['pitch_audio'], not both")
        out = {}
        if inp.get("pitch_hz") is not None:
            hz = torch.as_tensor(np.asarray(inp["pitch_hz"], dtype=np.float32))
            if hz.dim() != 1 or hz.numel() == 0:
                raise ValueError(f"preprocess_input: inp['pitch_hz'] must be a non-empty 1-D contour in Hz (got shape {tuple(hz.shape)})")
            out["pitch_hz"] = (hz[None].to(self.device), [hz.numel()])
        elif inp.get("pitch_audio") is not None:
            from .f0track import track_f0_device
            sr, hop = int(self.hparams["audio_sample_rate"]), int(self.hparams["hop_size"])
            audio = inp["pitch_audio"]
            if isinstance(audio, (str, bytes)) or hasattr(audio, "__fspath__"):
                from .audiofile import load_audio
                wav, in_sr = load_audio(audio)
            elif isinstance(audio, (tuple, list)) and len(audio) == 2 and np.ndim(audio[1]) == 0 and np.ndim(audio[0]) == 1:
                wav, in_sr = np.asarray(audio[0], dtype=np.float32), int(audio[1])
            else:
                raise ValueError("preprocess_input: inp['pitch_audio'] must be a WAV path or a (waveform, sample_rate) pair")
            gv, n = torch.from_numpy(np.ascontiguousarray(wav))[None].to(self.device), len(wav)
            if in_sr != sr:
                from .resample import resample_batch
                gv, (n,) = resample_batch(gv, [n], in_sr, sr)
            n_mel = n // hop + 1
            wav16, wav16_lens = self.process_audio_wav(gv, [n_mel], [n])
            out["pitch_hz"] = (track_f0_device(wav16, wav16_lens, n_mel, sr=sr, hop_size=hop), [n_mel])
        if inp.get("pitch_shift") is not None:
            if "pitch_hz" not in out:
                raise ValueError("preprocess_input: inp['pitch_shift'] transposes inp['pitch_hz'] / inp['pitch_audio']; it needs one of them")
            out["pitch_shift"] = float(inp["pitch_shift"])
        return out

    @torch.no_grad()
    def preprocess_input(self, inp, vad_flags=None):
        """Mirror of `StyleSingerInfer.preprocess_input` (inference/StyleSinger.py:94-137) with every producer on the device: fills `mel`,
        `spk_embed`, `emo_embed`, `f0` (the tracker's contour in Hz on the mel grid) as numpy arrays, `ph_token`, and `item_name` / `wav_fn` from
        `inp['ref_audio']`: the path of a WAV file (`audiofile.load_audio`: PCM or float, any channel count, any sample rate), a float waveform at
        `inp['ref_sr']` Hz (default: the model's sample rate) or a `(waveform, sample_rate)` pair; audio of another rate is resampled on the device as
        `librosa.core.load(wav_path, sr=audio_sample_rate)` does (`resample.py`; parity with librosa UNPINNED). Needs `emotion_state` and
        `speaker_state` (the two encoders' checkpoints). `vad_flags`: see `_resolve_vad` (None = webrtcvad on the host, False = opt out).
        Pitch control (`_pitch_inputs`): `inp['pitch_hz']` / `inp['pitch_shift']` pass through; `inp['pitch_audio']` (a guide vocal) is tracked
        on the device and replaced by its contour in `inp['pitch_hz']`."""
        batch = self._device_batch(inp, vad_flags)
        n_mel, audio = batch["n_mel"], inp["ref_audio"]
        inp.update(item_name=inp.get("name"), wav_fn=os.fsdecode(audio) if isinstance(audio, (str, bytes)) or hasattr(audio, "__fspath__") else None,
                   mel=batch["ref_mels"][0, :n_mel].cpu().numpy(), spk_embed=batch["spk_embed"][0].cpu().numpy(),
                   emo_embed=batch["emo_embed"][0].cpu().numpy(), f0=batch["ref_f0_hz"][0, :n_mel].double().cpu().numpy())
        if inp.get("pitch_audio") is not None:   # tracked once, here: the contour replaces the audio entry
            inp["pitch_hz"] = batch["pitch_hz"][0][0].cpu().numpy()
            del inp["pitch_audio"]
        return inp

    def postprocess_output(self, output):
        return output

    def infer_once(self, inp, vad_flags=None, noise=None, vocoder_noise=None):
        """inference/StyleSinger.py:175-179: preprocess_input -> forward_model -> postprocess_output. The features stay on the device between the
        producers and the model (no numpy detour; `preprocess_input` is the form that returns them). An `inp` that already carries the features
        (`mel`, `spk_embed`, `emo_embed`, `f0`, `ph_token`) skips the producers, as before."""
        if all(k in inp for k in ("mel", "spk_embed", "emo_embed", "f0", "ph_token")):
            return self.postprocess_output(self.forward_model(inp, noise=noise, vocoder_noise=vocoder_noise))
        batch = self._device_batch(inp, vad_flags)
        res = self.infer_batch({k: v for k, v in batch.items() if k not in ("n_mel", "ref_f0_hz")}, noise=noise, vocode=False)
        return self.postprocess_output(self._wav_from_result(res, vocoder_noise))

    # ---- a whole score -----------------------------------------------------------------------------
    def _song_reference(self, inp, vad_flags):
        """The reference of a song, processed ONCE: (ref_mels [1, Tr, 80], ref_f0 [1, Tr], spk_embed [1, 256], emo_embed [1, 256]) on the device,
        from the features in `inp` (`mel`, `spk_embed`, `emo_embed`, `f0`: as `infer_once` accepts them) or from inp['ref_audio'] through the
        producers of `_device_batch`."""
        d = self.device
        if all(k in inp for k in ("mel", "spk_embed", "emo_embed", "f0")):
            from .pitch import norm_interp_f0
            t = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float32)[None].to(d)
            f0, _uv = norm_interp_f0(np.asarray(inp["f0"]), self.hparams)
            return t(inp["mel"]), f0[None].to(d), t(inp["spk_embed"]), t(inp["emo_embed"])
        if inp.get("ref_audio") is None:
            raise ValueError("sing_score: give inp['ref_audio'] (the reference voice), or its features mel / spk_embed / emo_embed / f0")
        one = {k: inp[k] for k in ("ref_audio", "ref_sr", "ph", "ph_token", "note", "note_dur", "note_type") if k in inp}
        b = self._device_batch(one, vad_flags)
        inp.setdefault("ph_token", one["ph_token"])
        return b["ref_mels"], b["ref_f0"], b["spk_embed"], b["emo_embed"]

    @torch.no_grad()
    def sing_score(self, inp, max_seconds=12.0, segment_batch=8, fade_ms=5.0, in_flight=3, seed=None, out_lufs=None, vad_flags=None):
        """Sing a score of any length in the reference's voice: `inp` = the reference's input dict (`ph` | `ph_token`, `note`, `note_dur`, `note_type`,
        optionally `ph_dur` = seconds per phone, `pitch_hz` | `pitch_audio`, `pitch_shift`; `ref_audio` or the reference's features). The score
        is cut into phrases at its rests (`song.plan_song`: policy and limits there), the reference is processed and its style encoded ONCE, the
        plan's batches run through `infer_batches` (batch i with seed + i), and the segments are put on one timeline on the device
        (`ss_song_offsets` + three `ss_song_place` per batch: the waveform with a raised-cosine fade of `fade_ms` on both sides of every joint, the
        mel and the f0 as they are). Segments never overlap: the song is their concatenation. ONE host sync at the end learns the length. Loudness
        (`out_lufs`, else hparams['out_loudness_lufs']) is applied to the WHOLE song, never per segment: that would flatten its dynamics.
        -> dict(wav [N], mel [F, 80], f0 [F] on the device, segments = [{first, last, start_frame, n_frames, batch, row}] (phones [first, last)),
        plan (the SongPlan; its batches in their device form), lufs (float, the loudness before the gain) when a target is set)."""
        from . import song
        hp, d = self.hparams, self.device
        sr, hop = int(hp["audio_sample_rate"]), int(self.vocoder.model.hop)
        inp = dict(inp)
        song.check_pitch_keys(inp)   # pitch control without ph_dur is refused before a device is touched
        seed = hp["seed"] if seed is None else seed
        ref_mels, ref_f0, spk, emo = self._song_reference(inp, vad_flags)
        if inp.get("pitch_audio") is not None:   # the guide vocal is tracked on the device; the planner takes its contour
            hz, _n = self._pitch_inputs({"pitch_audio": inp.pop("pitch_audio")})["pitch_hz"]
            inp["pitch_hz"] = hz[0].cpu().numpy()
        plan = song.plan_song(inp, sr=sr, hop=hop, max_seconds=max_seconds, segment_batch=segment_batch, ph_encoder=self.ph_encoder)
        S = len(plan.segments)
        style = self.model.encode_style(ref_mels, ref_f0)
        fade = max(0, int(round(float(fade_ms) * sr / 1000.0))) if S > 1 else 0
        win = torch.from_numpy(song.fade_window(fade)).to(d) if fade else None
        segs_dev, rows_dev = [], []
        for i, hb in enumerate(plan.batches):   # everything the stitch needs from the host goes up before the first batch runs
            nb = len(plan.rows[i])
            b = {k: ((v[0].to(d), v[1]) if k == "pitch_hz" else v.to(d) if torch.is_tensor(v) else v) for k, v in hb.items()}
            rep = lambda x: x.expand(nb, *x.shape[1:]).contiguous()
            b.update(spk_embed=rep(spk), emo_embed=rep(emo), ref_mels=ref_mels.expand(nb, -1, -1), ref_f0=ref_f0.expand(nb, -1),
                     style_cache={k: rep(v) for k, v in style.items()})
            plan.batches[i] = b
            rows_dev.append(torch.tensor(plan.rows[i], dtype=torch.long).to(d))
            segs_dev.append(rows_dev[-1].to(torch.int32))
        results = list(self.infer_batches(plan.batches, in_flight=in_flight, seed=seed))
        lens = torch.zeros(S, device=d, dtype=torch.int32)
        for rows, res in zip(rows_dev, results):
            lens.index_copy_(0, rows, res["lens"].to(torch.int32))
        offsets = song.song_offsets(lens)
        cap = sum(int(res["mel"].shape[0]) * int(res["mel"].shape[1]) for res in results)   # frames: no segment is longer than its batch
        wav, mel, f0 = (torch.empty(cap * u, device=d, dtype=torch.float32) for u in (hop, 80, 1))
        flags = torch.zeros(1, device=d, dtype=torch.int32)
        for seg, res in zip(segs_dev, results):
            song.song_place(res["wav"].contiguous(), seg, lens, offsets, hop, wav, win=win, flags=flags)
            song.song_place(res["mel"].contiguous(), seg, lens, offsets, 80, mel, flags=flags)
            song.song_place(res["f0"].contiguous(), seg, lens, offsets, 1, f0, flags=flags)
        *starts, flagged = (int(v) for v in torch.cat([offsets, flags.to(torch.int64)]).cpu())   # the one host sync of the stitch
        if flagged != 0:
            raise L.StyleSingerHipError(f"sing_score: ss_song_place clamped or refused a segment (flags {flagged}): the plan and the rendered "
                                        "batches disagree")
        F = starts[-1]
        out = dict(wav=wav[:F * hop], mel=mel[:F * 80].view(F, 80), f0=f0[:F], plan=plan, segments=[])
        for s, g in enumerate(plan.segments):
            g["start_frame"], g["n_frames"] = starts[s], starts[s + 1] - starts[s]
            out["segments"].append({k: g[k] for k in ("first", "last", "start_frame", "n_frames", "batch", "row")})
        long_ = [s for s, g in enumerate(plan.segments) if g["n_frames"] > 3000]
        if long_:
            warnings.warn(f"sing_score: {len(long_)} segment(s) came out longer than the 3000 frames the model was trained on (first: phones "
                          f"[{plan.segments[long_[0]]['first']}, {plan.segments[long_[0]]['last']}), {plan.segments[long_[0]]['n_frames']} frames); lower "
                          "max_seconds or add rests")
        target = out_lufs if out_lufs is not None else hp.get("out_loudness_lufs")
        if target is not None:
            y, lufs = self._to_lufs(out["wav"][None], [F * hop], target)
            out["wav"], out["lufs"] = y[0], float(lufs[0])
        return out

    @classmethod
    def example_run(cls, hparams=None, ref_audio="test/test.wav", out_path="infer_out/test.wav", vad_flags=None, pitch=None, **ctor):
        """inference/StyleSinger.py:181-331: the example score (stylesinger_amd/example_input.json = that method's input dict, extracted by
        `python -m oracle.gen_golden --round6`) sung in the style of `ref_audio`, written to `out_path` as 16-bit PCM (utils/audio.py:12-17).
        `ctor`: how to build the instance - `exp_dir` + `vocoder_dir` (the reference's checkpoints, `from_checkpoints`) or explicit
        `model_state` / `vocoder_state` / `emotion_state` / `speaker_state` / `phone_set`."""
        from .writer import save_wav
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "example_input.json")) as fh:
            inp = {k: v for k, v in json.load(fh).items() if k != "source"}
        inp["ref_audio"] = ref_audio
        inp.update(pitch or {})   # pitch control: pitch_hz | pitch_audio, pitch_shift (`_pitch_inputs`)
        if "exp_dir" in ctor:
            ins = cls.from_checkpoints(hparams, ctor.pop("exp_dir"), ctor.pop("vocoder_dir"), **ctor)
        else:
            ins = cls(hparams, **ctor)
        out = ins.infer_once(inp, vad_flags=vad_flags)
        if ins.hparams.get("out_loudness_lufs") is not None:
            y, _ = ins._to_lufs(torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32))[None].to(ins.device), [len(out)], ins.hparams["out_loudness_lufs"])
            out = y[0].cpu().numpy()
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        save_wav(out, out_path, int(ins.hparams["audio_sample_rate"]), norm=bool(ins.hparams.get("out_wav_norm", False)))
        print(f"Save at {out_path}.")
        return out


def _score_run(score, hparams, out_path, segments_out=None, vad_flags=None, max_seconds=12.0, segment_batch=8, fade_ms=5.0, **ctor):
    """`--score`: sing the score dict with `StyleSingerInfer.sing_score`, write the song as 16-bit PCM and, with `segments_out`, the timeline as JSON
    (per segment its phone range, start sample and sample count: for lining the vocal up with an accompaniment)."""
    from .writer import save_wav
    ins = StyleSingerInfer(hparams, **ctor)
    res = ins.sing_score(score, max_seconds=max_seconds, segment_batch=segment_batch, fade_ms=fade_ms, vad_flags=vad_flags)
    sr, hop = int(ins.hparams["audio_sample_rate"]), int(ins.vocoder.model.hop)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    save_wav(res["wav"].cpu().numpy(), out_path, sr, norm=bool(ins.hparams.get("out_wav_norm", False)))
    if segments_out:
        with open(segments_out, "w") as fh:
            json.dump(dict(sample_rate=sr, hop=hop, n_samples=int(res["wav"].numel()),
                           segments=[dict(first_phone=g["first"], last_phone=g["last"], start_sample=g["start_frame"] * hop,
                                          n_samples=g["n_frames"] * hop) for g in res["segments"]]), fh, indent=1)
    print(f"Save at {out_path}.")
    return res


def main(argv=None):
    """`python -m stylesinger_amd.infer --exp-dir checkpoints/<exp> --vocoder-dir <hifigan dir> --emotion-ckpt <pt> --speaker-ckpt <pt>
    --phone-set ZH_checkpoint_phone_set.json [--ref-audio test/test.wav] [--out infer_out/test.wav] [--no-vad-trim]` = the reference's
    `python inference/StyleSinger.py` (StyleSingerInfer.example_run). `--pitch-audio guide.wav | --pitch-npy contour.npy [--pitch-shift semitones]`:
    sing the score on a given pitch contour instead of the predicted one. `--loud-norm`: loudness-normalise the reference audio as a model trained with
    hparams['loud_norm'] expects; `--out-lufs X`: write the result at X LUFS.
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
    ap.add_argument("--out", default="infer_out/test.wav")
    ap.add_argument("--no-vad-trim", action="store_true", help="explicit opt-out of trim_long_silences (webrtcvad missing)")
    ap.add_argument("--pitch-audio", help="sing on the pitch of this guide vocal (a WAV file, tracked on the device, 80-800 Hz) instead of the predicted f0")
    ap.add_argument("--pitch-npy", help="sing on this contour: a .npy file holding a 1-D array of Hz at the mel hop, 0 = unvoiced")
    ap.add_argument("--pitch-shift", type=float, help="transpose the given contour by this many semitones")
    ap.add_argument("--loud-norm", action="store_true", help="hparams['loud_norm'] with loudness='bs1770': bring the reference audio to -22 LUFS first "
                    "(this project's BS.1770 meter; parity with pyloudnorm unpinned)")
    ap.add_argument("--out-lufs", type=float, help="write the result at this BS.1770 integrated loudness (hparams['out_loudness_lufs'])")
    ap.add_argument("--score", help="a score of any length as JSON (the keys of example_input.json, optionally ph_dur = seconds per phone): split at "
                    "its rests, rendered in batches, stitched on the device")
    ap.add_argument("--max-seconds", type=float, default=12.0, help="--score: longest merged segment")
    ap.add_argument("--segment-batch", type=int, default=8, help="--score: segments per batch")
    ap.add_argument("--fade-ms", type=float, default=5.0, help="--score: raised-cosine fade on both sides of every joint")
    ap.add_argument("--segments-out", help="--score: write the timeline (phone ranges and start samples per segment) to this JSON file")
    a = ap.parse_args(argv)
    if a.pitch_audio and a.pitch_npy:
        ap.error("--pitch-audio and --pitch-npy exclude each other")
    if a.pitch_shift is not None and not (a.pitch_audio or a.pitch_npy):
        ap.error("--pitch-shift needs --pitch-audio or --pitch-npy")
    pitch = {}
    if a.pitch_audio:
        pitch["pitch_audio"] = a.pitch_audio
    if a.pitch_npy:
        pitch["pitch_hz"] = np.load(a.pitch_npy)
    if a.pitch_shift is not None:
        pitch["pitch_shift"] = a.pitch_shift
    score = None
    if a.score:
        with open(a.score) as fh:
            score = {k: v for k, v in json.load(fh).items() if k != "source"}
        if pitch and score.get("ph_dur") is None:
            ap.error("--score with a pitch flag needs 'ph_dur' (seconds per phone) in the score: without it the segment frame counts are not known "
                     "before rendering")
        score.update(pitch)
        from . import song
        try:
            song.check_pitch_keys(score)
        except ValueError as e:
            ap.error(str(e))
        if a.ref_audio or not score.get("ref_audio"):
            score["ref_audio"] = a.ref_audio or "test/test.wav"
    elif a.segments_out:
        ap.error("--segments-out needs --score")
    a.ref_audio = a.ref_audio or "test/test.wav"
    emo = torch.load(a.emotion_ckpt, map_location="cpu", weights_only=False)
    spk = torch.load(a.speaker_ckpt, map_location="cpu", weights_only=False)
    from . import ckpt
    state, _ = ckpt.read_state(a.exp_dir, "model")
    if state is None:
        raise FileNotFoundError(f"| ckpt not found in {a.exp_dir}.")
    vstate, vcfg = ckpt.load_vocoder_ckpt(a.vocoder_dir)
    hp = {}
    if a.loud_norm:
        hp["loud_norm"] = True
    if a.out_lufs is not None:
        hp["out_loudness_lufs"] = a.out_lufs
    ctor = dict(model_state=state, vocoder_state=vstate, vocoder_config=vcfg, emotion_state=emo.get("model_state", emo),
                speaker_state=spk.get("model_state", spk), phone_set=a.phone_set, loudness="bs1770" if a.loud_norm else None)
    if score is not None:
        _score_run(score, hp or None, a.out, segments_out=a.segments_out, vad_flags=False if a.no_vad_trim else None, max_seconds=a.max_seconds,
                   segment_batch=a.segment_batch, fade_ms=a.fade_ms, **ctor)
        return
    StyleSingerInfer.example_run(hp or None, a.ref_audio, a.out, vad_flags=False if a.no_vad_trim else None, pitch=pitch, **ctor)


if __name__ == "__main__":
    main()
