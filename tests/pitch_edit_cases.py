"""Inputs of the pitch-edit tests (tests/test_pitch_edit_cpu.py, tests/test_gpu_pitch_edit.py): one batch of B = 6 items on T = 3 TILE + 40 frames,
built once and read only, and the float64 definition's results on it (`reference`, cached per (W, parameter set)).

Signal: the score's note staircase carrying a 6 Hz / 50-cent vibrato, a constant 30-cent offset and a slow drift (0.3 Hz, 20 cents), rounded to fp32
log2 Hz. Edges (TILE = frames per workgroup of ss_pitch_edit, W in WS):
  item 0 (length T)      held runs of 27 and 28 frames (one frame too short for VIB and exactly long enough), a region of one frame, a region of two
                         frames (shorter than W = 3 and 31), held-run boundaries at TILE - 1, TILE, TILE + 1, a region boundary at TILE + 31, midi 128
                         (sung as 127), a held-run boundary at 2 TILE - 31;
  item 1 (length T - 5)  a held run of 600 frames over three tiles (its bounds cannot come from a tile's halo), starting after a rest of 3 frames;
  item 2 (length 780)    one-frame rests that open regions at TILE - 31, TILE - 3, TILE - 1, TILE + 1, TILE + 3, TILE + 31, then held-run boundaries
                         at 2 TILE - 3, 2 TILE - 1, 2 TILE, 2 TILE + 1, 2 TILE + 3, 2 TILE + 31;
  item 3 (length 700)    a rest that ends exactly at TILE (a region opens there), held-run boundaries at TILE - 31, TILE + 3, TILE + 31;
  item 4 (length 0), item 5 (length 500, all rests).
u cycles through 0 / 0.5 / 1 (mostly 0). Rows are zero past an item's length; `poisoned` fills them with values that would show in a result."""
import functools

import numpy as np

from stylesinger_amd import pitch as P

TILE = P.EDIT_TILE
T = 3 * TILE + 40
FPS = 187.5                                   # 48 kHz / 256
WS = (1, 3, 31)
VIB = (5.5, 40.0, 12, 8)                      # rate Hz, depth cents, delay frames, fade frames: a held run needs 12 + 2 * 8 = 28 frames
PARAMS = {"correct": dict(alpha=0.7, kappa=1.0, vibrato=None), "scale": dict(alpha=0.0, kappa=0.5, vibrato=None),
          "all": dict(alpha=0.6, kappa=1.5, vibrato=VIB)}


def _row(spans):
    """[(midi, first frame)] in ascending order -> the notes per frame up to the last entry's frame (its midi is ignored: it only ends the row)"""
    out = []
    for (m, a), (_, e) in zip(spans[:-1], spans[1:]):
        assert e > a
        out += [m] * (e - a)
    return np.asarray(out, dtype=np.int64)


ITEMS = [
    _row([(60, 0), (62, 27), (0, 55), (64, 56), (0, 57), (65, 59), (0, 61), (67, 63), (69, TILE - 1), (71, TILE), (72, TILE + 1), (0, TILE + 31),
          (128, TILE + 33), (60, 2 * TILE - 31), (0, T)]),
    _row([(0, 0), (57, 3), (0, 603), (59, 700), (0, T - 5)]),
    _row([(60, 0), (0, TILE - 32), (61, TILE - 31), (0, TILE - 4), (62, TILE - 3), (0, TILE - 2), (63, TILE - 1), (0, TILE), (64, TILE + 1),
          (0, TILE + 2), (65, TILE + 3), (0, TILE + 30), (66, TILE + 31), (67, 2 * TILE - 3), (68, 2 * TILE - 1), (69, 2 * TILE), (70, 2 * TILE + 1),
          (71, 2 * TILE + 3), (72, 2 * TILE + 31), (0, 780)]),
    _row([(60, 0), (61, TILE - 31), (0, TILE - 6), (62, TILE), (63, TILE + 3), (64, TILE + 31), (0, 700)]),
    np.zeros(0, dtype=np.int64),
    np.zeros(500, dtype=np.int64),
]
B = len(ITEMS)
LENS = [len(m) for m in ITEMS]
assert B <= 6 and LENS[0] == T and max(LENS) == T


@functools.lru_cache(None)
def batch():
    """-> dict(f fp32 [B, T], midi int64 [B, T], u fp32 [B, T], lens [B]); zeros past every item's length. Read only."""
    f, midi, u = np.zeros((B, T), dtype=np.float32), np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.float32)
    t = np.arange(T, dtype=np.float64)
    for b, m in enumerate(ITEMS):
        n = len(m)
        key = np.where(m > 0, np.minimum(m, 127), 69)
        cents = (P.EDIT_K0 + 100.0 * (key - 69) + 30.0 + 50.0 * np.sin(2 * np.pi * 6.0 * t[:n] / FPS + 0.4 * b)
                 + 20.0 * np.sin(2 * np.pi * 0.3 * t[:n] / FPS))
        f[b, :n], midi[b, :n] = (cents / 1200.0).astype(np.float32), m
        u[b, :n] = np.where(t[:n] % 13 == 5, 1.0, np.where(t[:n] % 11 == 3, 0.5, 0.0))
    for a in (f, midi, u):
        a.setflags(write=False)
    return dict(f=f, midi=midi, u=u, lens=list(LENS))


def poisoned(sign=1.0):
    """The batch with what lies past every item's length filled with values that would show in a result: f = +-1000, u = -1, midi = 99."""
    d = batch()
    f, midi, u = d["f"].copy(), d["midi"].copy(), d["u"].copy()
    for b, n in enumerate(LENS):
        f[b, n:], midi[b, n:], u[b, n:] = sign * 1000.0, 99, -1.0
    return dict(f=f, midi=midi, u=u, lens=list(LENS))


@functools.lru_cache(None)
def reference(W, name):
    """The definition on every item of `batch()` -> dict(f [B, T] fp32 (the input's bits past an item's length), stats [B, 6], run_lo, run_hi
    [B, T] int32 (-1 past an item's length)). Read only."""
    d, prm = batch(), PARAMS[name]
    f, stats = d["f"].copy(), np.zeros((B, 6))
    lo, hi = np.full((B, T), -1, dtype=np.int32), np.full((B, T), -1, dtype=np.int32)
    for b, n in enumerate(LENS):
        f[b, :n], stats[b], lo[b, :n], hi[b, :n] = P.pitch_edit(d["f"][b, :n], d["midi"][b, :n], W, prm["alpha"], prm["kappa"], prm["vibrato"],
                                                                u=d["u"][b, :n], fps=FPS)
    for a in (f, stats, lo, hi):
        a.setflags(write=False)
    return dict(f=f, stats=stats, run_lo=lo, run_hi=hi)


def sung_mask():
    d = batch()
    return (d["midi"] > 0) & (np.arange(T)[None, :] < np.asarray(LENS)[:, None])
