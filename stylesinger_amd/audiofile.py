"""Reference-audio FILE intake: the decoding and down-mix half of `librosa.core.load(wav_path, sr=...)` (utils/audios/__init__.py:52; the
resampling half is `resample.py`). librosa reads through libsndfile; this is an own RIFF/WAVE chunk walk for the sample formats a singing
recording comes in (Python 3.10's `wave` refuses IEEE-float and WAVE_FORMAT_EXTENSIBLE headers). Scaling as libsndfile's float read does it:
uint8 (v - 128) / 128, int16 / 2^15, int24 / 2^23, int32 / 2^31, float32 as is, float64 rounded to float32; then the channels are averaged in
float32 (`librosa.to_mono`). Compressed containers (flac, mp3, ogg ...) need a decoder library and are refused by name."""
import os
import struct

import numpy as np

WAVE_FORMAT_PCM = 1
WAVE_FORMAT_IEEE_FLOAT = 3
WAVE_FORMAT_EXTENSIBLE = 0xFFFE
# the sub-format GUID of an extensible header = the 16-bit format tag + this fixed tail (KSDATAFORMAT_SUBTYPE_*)
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


def _decode(raw, tag, bits, path):
    if tag == WAVE_FORMAT_PCM:
        if bits == 8:
            return (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
        if bits == 16:
            return np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
        if bits == 24:
            b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            v = v - ((v & 0x800000) << 1)            # sign extension
            return v.astype(np.float32) / 8388608.0
        if bits == 32:
            return (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    elif tag == WAVE_FORMAT_IEEE_FLOAT:
        if bits == 32:
            return np.frombuffer(raw, dtype="<f4").astype(np.float32)
        if bits == 64:
            return np.frombuffer(raw, dtype="<f8").astype(np.float32)
    raise ValueError(f"{path}: unsupported sample format (format tag {tag}, {bits} bits)")


def load_audio(path):
    """-> (float32 mono samples, sample rate) of a RIFF/WAVE file: format tags 1 (PCM: 8 / 16 / 24 / 32 bit), 3 (IEEE float: 32 / 64 bit) and
    0xFFFE (extensible, either sub-format). ValueError for anything else, saying what was found."""
    name = os.fsdecode(path)
    with open(name, "rb") as fh:
        data = fh.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{name}: not a RIFF/WAVE file (starts with {data[:4]!r}): compressed formats such as flac, mp3 or ogg are not decoded here - "
                         "convert the reference audio to WAV")
    pos, fmt, raw = 12, None, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        body = data[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            if size < 16:
                raise ValueError(f"{name}: fmt chunk of {size} bytes")
            tag, channels, rate, _bps, align, bits = struct.unpack_from("<HHIIHH", body)
            if tag == WAVE_FORMAT_EXTENSIBLE:
                if size < 40 or body[26:40] != _GUID_TAIL:
                    raise ValueError(f"{name}: extensible header with an unknown sub-format")
                tag = struct.unpack_from("<H", body, 24)[0]
            fmt = (tag, channels, rate, align, bits)
        elif cid == b"data":
            raw = body                                  # a truncated file gives what is there, as libsndfile does
            break
        pos += 8 + size + (size & 1)                    # chunks are word aligned
    if fmt is None or raw is None:
        raise ValueError(f"{name}: no {'fmt' if fmt is None else 'data'} chunk")
    tag, channels, rate, align, bits = fmt
    if tag not in (WAVE_FORMAT_PCM, WAVE_FORMAT_IEEE_FLOAT):
        raise ValueError(f"{name}: WAVE format tag {tag:#x} is not PCM (1) or IEEE float (3): compressed audio is not decoded here")
    if channels < 1 or rate < 1 or bits % 8 or align != channels * bits // 8:
        raise ValueError(f"{name}: inconsistent fmt chunk ({channels} channels, {rate} Hz, {bits} bits, block align {align})")
    raw = raw[:len(raw) // align * align]
    x = _decode(raw, tag, bits, name).reshape(-1, channels)
    return (x[:, 0].copy() if channels == 1 else x.mean(axis=1, dtype=np.float32)), int(rate)


def as_waveform(audio, default_sr, what):
    """The audio entries of `preprocess_input`'s dict (`what` = the key: "ref_audio", "pitch_audio"): the path of a WAV file (str / bytes /
    PathLike -> `load_audio`), a `(waveform, sample_rate)` pair, or a bare array read at `default_sr` Hz - refused where the key has no rate
    to read it at (`default_sr=None`). -> (float32 mono samples, sample rate, the decoded path or None)."""
    if isinstance(audio, (str, bytes)) or hasattr(audio, "__fspath__"):
        return (*load_audio(audio), os.fsdecode(audio))
    if isinstance(audio, (tuple, list)) and len(audio) == 2 and np.ndim(audio[1]) == 0 and np.ndim(audio[0]) == 1:
        return np.asarray(audio[0], dtype=np.float32), int(audio[1]), None
    if default_sr is None:
        raise ValueError(f"preprocess_input: inp['{what}'] must be a WAV path or a (waveform, sample_rate) pair")
    return np.asarray(audio, dtype=np.float32), int(default_sr), None


def load_pcm16(path, want_sr):
    """The strict static loader: a 16-bit PCM WAV at exactly `want_sr` Hz -> float32 mono in [-1, 1); anything else is a ValueError.
    (`preprocess_input` reads files through `load_audio` + `resample.resample_batch`, which take other formats and rates.)"""
    import wave
    with wave.open(os.fsdecode(path), "rb") as wf:
        if wf.getsampwidth() != 2 or wf.getframerate() != want_sr:
            raise ValueError(f"{path}: need 16-bit PCM at {want_sr} Hz (got {8 * wf.getsampwidth()} bit, {wf.getframerate()} Hz)")
        pcm = np.frombuffer(wf.readframes(wf.getnframes()), dtype="<i2").astype(np.float32).reshape(-1, wf.getnchannels())
    return pcm.mean(axis=1) / 32768.0
