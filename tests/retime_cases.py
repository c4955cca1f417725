"""Inputs shared by tests/test_retime_cpu.py and tests/test_gpu_retime.py (no test is collected from this file).

A score is a list of phones (note, score frames): several phones may share a note (the phones inside a note), a note may repeat, a phone may have no
frame at all. A guide is a list of (note | cents, guide frames) sung at exact integer cents, so the cents the device computes from the Hz are the
integers meant here (contour_align_cases.cents_margin is asserted where the kernel runs)."""
import functools

import numpy as np

import contour_align_cases as K
from stylesinger_amd import pitch as P


def score(phones):
    """[(note, frames)] per phone -> (mel2ph [n_t] 1-based, midi [n_t])"""
    notes = np.asarray([n for n, _ in phones], dtype=np.int64)
    frames = [f for _, f in phones]
    return np.repeat(np.arange(1, len(phones) + 1, dtype=np.int64), frames), np.repeat(notes, frames)


def guide(sung):
    """[(note, frames)] -> fp32 Hz [n_c]; note 0 = unvoiced"""
    return np.repeat(K.note_hz([n for n, _ in sung]), [f for _, f in sung]).astype(np.float32)


MELODY = [(60, 4), (60, 3), (0, 3), (62, 5), (62, 4), (64, 2), (64, 4), (65, 4)]   # 8 phones; notes 60, rest, 62 (two phones: a repeat), 64, 65
MELODY_SUNG = [(60, 9), (0, 3), (62, 20), (64, 6), (65, 11)]                        # the same notes with per-note stretches of 1x to 3x
FOUR = [(60, 3), (62, 3), (64, 3), (65, 3)]


@functools.lru_cache(maxsize=None)
def long_items():
    """Two items at T = Lc = 8192, the kernel's caps. Item 0: 4096 frames that change pitch on EVERY frame (4096 anchors: nine chunks of the block
    scans), then notes of 2 .. 9 frames; the guide moves every second boundary of that part by one frame. Item 1: a new pitch on every frame of all
    8192 (m = n_c = 8192: every span one frame, the LDS arrays full). The host definition of the ALIGNMENT builds the whole 8192 x 8192 cost matrix,
    so these two have no entry in `expected`: the GPU test retimes the path ss_contour_align gave (pinned to its definition by its own tests)."""
    rng = np.random.default_rng(8192)
    cyc = np.asarray([60, 62, 64], dtype=np.int64)
    head = cyc[np.arange(4096) % 3]
    lens = []
    while sum(lens) < 4096:
        lens.append(int(rng.integers(2, 10)))
    lens[-1] -= sum(lens) - 4096
    if lens[-1] < 2:
        lens[-2] += lens[-1]
        lens.pop()
    if len(lens) % 2:
        lens[-2] += lens[-1]
        lens.pop()
    tail_notes = np.asarray([67, 69, 71, 72], dtype=np.int64)[np.arange(len(lens)) % 4]
    sung = np.asarray(lens).copy()
    sung[0::2] += 1                                             # every pair of notes: the boundary one frame later, the pair's total unchanged
    sung[1::2] -= 1
    assert (sung >= 1).all() and sung.sum() == 4096
    midi0 = np.concatenate([head, np.repeat(tail_notes, lens)])
    g0 = np.concatenate([K.note_hz(head), np.repeat(K.note_hz(tail_notes), sung)]).astype(np.float32)
    midi1 = cyc[np.arange(8192) % 3]
    return [dict(mel2ph=np.arange(1, 8193, dtype=np.int64), midi=midi0, guide=g0, band=4, shift=0.0),
            dict(mel2ph=np.arange(1, 8193, dtype=np.int64), midi=midi1, guide=K.note_hz(midi1), band=4, shift=0.0)]


def _case(phones, sung, band=None, shift=0.0):
    mel2ph, midi = score(phones)
    return dict(mel2ph=mel2ph, midi=midi, guide=guide(sung), band=band, shift=shift)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: dict(mel2ph, midi, guide, band, shift)}; `expected(name)` adds what the definition gives."""
    c = {
        "single_note": _case([(60, 5), (60, 4)], [(60, 14)]),                                   # m = 1, two phones
        "melody": _case(MELODY, MELODY_SUNG),                                                   # notes, a rest, repeated equal notes
        "melody_banded": _case(MELODY, MELODY_SUNG, band=24),
        "melody_shifted": _case(MELODY, [(n - 2 if n else 0, f) for n, f in MELODY_SUNG], band=24, shift=2.0),
        "guide_skips_a_note": _case(FOUR, [(60, 6), (64, 5), (65, 7)]),                         # 62 is left out: the min-1 passes move its anchor
        "guide_skips_the_last_notes": _case(FOUR, [(60, 9)]),                                   # every later anchor crowds the end: the pinned end holds
        "guide_skips_the_first_notes": _case(FOUR, [(65, 9)]),
        "n_c_equals_m": _case(FOUR, [(60, 1), (62, 1), (64, 1), (65, 1)]),                      # every span one frame
        "n_c_equals_m_minus_1": _case(FOUR, [(60, 1), (62, 1), (65, 1)]),                       # status 1
        "n_t_1": _case([(60, 1)], [(60, 6)]),
        "n_c_1": _case([(60, 3), (62, 3), (64, 3)], [(62, 1)]),                                 # n_c < m: status 1
        "n_c_1_single_note": _case([(60, 4), (60, 3)], [(60, 1)]),                              # n_c == m == 1: status 0
        "no_score_frames": _case([], [(60, 5)]),
        "no_guide_frames": _case(FOUR, []),
        "phones_without_frames": _case([(60, 4), (62, 0), (64, 5), (65, 0), (65, 0), (67, 3)], [(60, 7), (64, 4), (67, 8)]),
        "alignment_refused": _case([(60, 1), (62, 1), (64, 1)], [(60, 20), (62, 15), (64, 15)], band=4),   # 50 > 4 * 3: status_align 1
        "identity": dict(zip(("mel2ph", "midi"), score(MELODY)), guide=K.note_hz(score(MELODY)[1]), band=None, shift=0.0),
    }
    return c


NAMES = list(cases())


@functools.lru_cache(maxsize=None)
def expected(name):
    """The definition chain on one case: contour_align, then retime_to_guide. -> dict(idx, status_align, out, src, status, n_spans); computed once."""
    c = cases()[name]
    _, idx, _, st_a = P.contour_align(c["guide"], c["midi"], band=c["band"], shift=c["shift"])
    out, src, status, n_spans = P.retime_to_guide(c["mel2ph"], c["midi"], idx, st_a, len(c["guide"]))
    for a in (idx, out, src):
        a.setflags(write=False)
    return dict(idx=idx, status_align=st_a, out=out, src=src, status=status, n_spans=n_spans)


WANT_STATUS = {"n_c_equals_m_minus_1": 1, "n_c_1": 1, "no_score_frames": 1, "no_guide_frames": 1, "alignment_refused": 1}   # every other case: 0
WANT_SPANS = {"single_note": 1, "melody": 5, "guide_skips_a_note": 4, "n_c_equals_m": 4, "n_c_equals_m_minus_1": 4, "n_t_1": 1, "n_c_1": 3,
              "no_score_frames": 0, "no_guide_frames": 4, "phones_without_frames": 3, "alignment_refused": 3}
