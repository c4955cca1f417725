"""Inputs shared by tests/test_contour_align_cpu.py and tests/test_gpu_contour_align.py (no test is collected from this file).

The musical case: a score of six notes and one rest, and a guide that sings the same notes at exact pitch with another timing - the frame counts of
the two long notes are swapped, so a linear time scaling puts the guide's notes on the wrong score frames while a warp can put every one right."""
import numpy as np

NOTES = [60, 64, 0, 62, 67, 65, 69]        # MIDI per phone, 0 = the rest; adjacent notes are distinct
SCORE_FRAMES = [4, 16, 3, 4, 5, 6, 4]      # d_k: frames per phone in the score (42)
GUIDE_FRAMES = [4, 5, 3, 4, 16, 6, 4]      # e_k: frames per phone in the guide (42): the two long notes' counts swapped
BAND = 12                                  # >= every |sum e - sum d| prefix difference (the largest is 11, after the second note)


def cents_to_hz(c):
    """Integer cents (6900 = A4 = 440 Hz) -> fp32 Hz. The fp32 rounding of the frequency moves 1200 log2(g / 440) by at most
    1200 * 2^-24 / ln 2 = 1.03e-4 cent, so the kernel's rounding to integer cents gives c back (`cents_margin` asserts the margin)."""
    c = np.asarray(c, dtype=np.float64)
    return (440.0 * np.exp2((c - 6900.0) / 1200.0)).astype(np.float32)


def note_hz(midi):
    """fp32 frequency of MIDI notes, 0 for a rest."""
    m = np.asarray(midi, dtype=np.int64)
    return np.where(m > 0, cents_to_hz(100 * m), np.float32(0)).astype(np.float32)


def note_hz_f64(midi):
    """The exact (float64) frequency of MIDI notes, 0 for a rest."""
    m = np.asarray(midi, dtype=np.float64)
    return np.where(m > 0, 440.0 * np.exp2((m - 69.0) / 12.0), 0.0)


def cents_margin(hz, shift=0.0):
    """Largest distance (cents, float64) of 1200 log2(g / 440) + 100 shift from the nearest integer over the voiced frames: the fp32 evaluation on
    the device (one division, log2f within 1 ulp, one product, one sum: a few ulp of a value below 16384, i.e. < 5e-3 cent) cannot flip the rounding
    while this stays below 0.25."""
    g = np.asarray(hz, dtype=np.float64)
    x = 1200.0 * np.log2(g[g > 0] / 440.0) + 100.0 * float(shift)
    return float(np.max(np.abs(x - np.rint(x)))) if x.size else 0.0


def musical_case():
    """-> dict(midi [n_t] per score frame, guide [n_c] fp32 Hz, want [n_t] fp32 Hz = the score's note frequency per frame, mel2ph [n_t] (1-based))."""
    assert len(NOTES) == len(SCORE_FRAMES) == len(GUIDE_FRAMES)
    assert all(a != b for a, b in zip(NOTES, NOTES[1:])) and sum(n > 0 for n in NOTES) >= 6 and NOTES.count(0) == 1
    assert SCORE_FRAMES != GUIDE_FRAMES
    assert max(abs(int(x)) for x in np.cumsum(GUIDE_FRAMES) - np.cumsum(SCORE_FRAMES)) <= BAND
    midi = np.repeat(np.asarray(NOTES, dtype=np.int64), SCORE_FRAMES)
    guide = np.repeat(note_hz(NOTES), GUIDE_FRAMES)
    mel2ph = np.repeat(np.arange(1, len(NOTES) + 1, dtype=np.int64), SCORE_FRAMES)
    return dict(midi=midi, guide=guide, want=note_hz(midi), mel2ph=mel2ph)


def wrong_note_share(got_hz, want_hz):
    """Share of the score's VOICED frames on which `got_hz` is not the score's note: unvoiced there, or more than 50 cents away."""
    got, want = np.asarray(got_hz, dtype=np.float64), np.asarray(want_hz, dtype=np.float64)
    v = want > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        off = np.abs(1200.0 * np.log2(np.where(got > 0, got, 1.0) / np.where(v, want, 1.0)))
    wrong = v & ((got <= 0) | (off > 50.0))
    return float(wrong.sum()) / float(v.sum())


def tie_rich(rng, n):
    """A contour from a three-note alphabet with unvoiced runs (integer cents through Hz): many equal costs, so the tie order decides the path."""
    c = rng.choice([5700, 5900, 6000], size=n)
    hz = cents_to_hz(c)
    hz[rng.random(n) < 0.25] = 0
    return hz


def tie_rich_midi(rng, n):
    return rng.choice([0, 57, 59, 60], size=n, p=[0.25, 0.25, 0.25, 0.25]).astype(np.int64)


def random_cents(rng, n):
    """Few ties: every frame its own integer cents value within two octaves, some unvoiced."""
    hz = cents_to_hz(rng.integers(4800, 7200, size=n))
    hz[rng.random(n) < 0.1] = 0
    return hz


def random_midi(rng, n):
    m = rng.integers(48, 73, size=n).astype(np.int64)
    m[rng.random(n) < 0.1] = 0
    return m
