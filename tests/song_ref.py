"""Host restatement (numpy) of the two kernels of csrc/song.hip, written from include/stylesinger_hip.h: the exclusive scan of the segment lengths
and the placement of rendered rows on the song's timeline with joint fades. The gain is one fp32 multiply by a table value, so the device result
must equal this one bit for bit. Nothing here imports the package."""
import numpy as np

FLAG_READ, FLAG_WRITE, FLAG_INDEX = 1, 2, 4


def fade_window(fade):
    """win[j] = 0.5 - 0.5 cos(pi (j + 0.5) / fade) in float64, rounded to fp32."""
    return np.array([0.5 - 0.5 * np.cos(np.pi * (j + 0.5) / fade) for j in range(fade)], dtype=np.float64).astype(np.float32)


def offsets_ref(lens):
    """[S] frames -> [S + 1] int64: offsets[s] = sum of max(lens[i], 0) over i < s."""
    out = np.zeros(len(lens) + 1, dtype=np.int64)
    for s, n in enumerate(lens):
        out[s + 1] = out[s] + max(int(n), 0)
    return out


def gain_index(k, f, fade):
    """table entry of the k-th float from a joint, k < f <= fade (integer division)"""
    return ((2 * k + 1) * fade) // (2 * f)


def place_ref(src, seg, lens, offsets, unit, out, win=None, cap=None):
    """src [B, lds] fp32 rows, seg [B] song index per row (< 0 = skip), lens [S], offsets [S + 1], unit floats per frame, out flat fp32 (written in
    place), win [fade] fp32 or None, cap = floats of `out` that may be written (default all). -> flags"""
    src = np.asarray(src, dtype=np.float32).reshape(len(seg), -1)
    B, lds = src.shape
    S = len(lens)
    fade = 0 if win is None else len(win)
    cap = out.size if cap is None else cap
    flags = 0
    for b in range(B):
        s = int(seg[b])
        if s < 0:
            continue
        if s >= S or int(offsets[s]) < 0:
            flags |= FLAG_INDEX
            continue
        if lens[s] <= 0:
            continue
        n = int(lens[s]) * unit
        dst = int(offsets[s]) * unit
        n_ok = n
        if n_ok > lds:
            n_ok, flags = lds, flags | FLAG_READ
        room = max(cap - dst, 0)
        if n_ok > room:
            n_ok, flags = room, flags | FLAG_WRITE
        row = src[b, :n].copy() if n <= lds else np.concatenate([src[b], np.zeros(n - lds, np.float32)])   # floats past lds are never used
        f = min(fade, n // 2)
        if f > 0:
            g = np.array([win[gain_index(k, f, fade)] for k in range(f)], dtype=np.float32)
            if s > 0:
                row[:f] = row[:f] * g               # float32 * float32 -> one rounding
            if s < S - 1:
                row[n - f:] = row[n - f:] * g[::-1]
        out[dst:dst + n_ok] = row[:n_ok]
    return flags


def stitch_ref(results, rows, S, hop, fade):
    """The song from per-batch results: results[i] = dict(wav [nb, >= T * hop], mel [nb, T, 80], f0 [nb, T], lens [nb]) as numpy, rows[i][r] = song
    index of row r. -> (wav, mel [F, 80], f0, offsets)"""
    lens = np.zeros(S, dtype=np.int64)
    for idx, res in zip(rows, results):
        lens[np.asarray(idx)] = res["lens"]
    off = offsets_ref(lens)
    F = int(off[-1])
    wav, mel, f0 = np.full(F * hop, np.nan, np.float32), np.full(F * 80, np.nan, np.float32), np.full(F, np.nan, np.float32)
    win = fade_window(fade) if fade else None
    for idx, res in zip(rows, results):
        seg = np.asarray(idx, dtype=np.int32)
        assert place_ref(res["wav"], seg, lens, off, hop, wav, win) == 0
        assert place_ref(res["mel"], seg, lens, off, 80, mel) == 0
        assert place_ref(res["f0"], seg, lens, off, 1, f0) == 0
    return wav, mel.reshape(F, 80), f0, off
