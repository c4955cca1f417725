"""The index identity behind the shared A tile of ss_wino44_conv, and the reach of its halo (numpy restatement, no GPU).

frame_of_quad(q) of wino44_conv.hip: quads are formed inside groups of 4 d frames, quad q covers the frames t, t + d, t + 2d, t + 3d with
t = (q // d) * 4 d + q % d. Tap group g of quad q reads the raw rows at frame_of_quad(q) + 4 d g - lo + i d (i = 0..6); the kernel builds
one tile for the quads q0 .. q0 + 63 + (G - 1) d with the group-0 offsets and lets group g read the tile rows g d further, which is the same
frames iff frame_of_quad(q + g d) == frame_of_quad(q) + 4 d g. The furthest frame a tile addresses must stay inside what the guard of
ss_wino44_conv allows for 32-bit byte offsets: (T + 1024) * lda * 4 < 2^31."""
import numpy as np
import pytest

BQ, AR = 64, 80            # quads per tile, rows of an A tile in LDS
GUARD_ROWS = 1024          # ss_wino44_conv: (T + GUARD_ROWS) * lda * 4 < 2^31
SHAPES_T = [7, 37, 256, 259, 531, 768, 12000, 384000]


def frame_of_quad(q, d):
    q = np.asarray(q, dtype=np.int64)
    return (q // d) * (4 * d) + q % d


def q_tiles_per_item(T, d):
    quads = -(-T // (4 * d)) * d
    return -(-quads // BQ)


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [7, 11])
def test_group_shift_is_a_whole_number_of_quads(k, d):
    G = (k + 3) // 4
    H = (G - 1) * d
    assert BQ + H <= AR and H <= 16, "the halo fits the LDS tile and one staging pass"
    for T in SHAPES_T:
        nq = min(q_tiles_per_item(T, d), 40) * BQ          # every quad of the test shapes; the first 40 tiles of the long items
        q = np.arange(nq)
        for g in range(G):
            assert np.array_equal(frame_of_quad(q + g * d, d), frame_of_quad(q, d) + 4 * d * g), (k, d, T, g)
        # the same through the tile: row r of tile q0 holds quad q0 + r; group g reads row r + g d <= 63 + H
        assert (BQ - 1) + (G - 1) * d < BQ + H


@pytest.mark.parametrize("d", [1, 3, 5])
def test_f43_group_stride_is_no_whole_number_of_quads(d):
    """Why wino43_conv.hip keeps one tile per tap group: its groups are 3 d frames apart, and no row shift m of a shared tile gives
    frame_of_quad(q + m) == frame_of_quad(q) + 3 d g for every q (d quads advance 4 d frames), for g = 1, 2 (k <= 9)."""
    q = np.arange(4 * BQ)
    for g in (1, 2):
        for m in range(0, 4 * d * g + 1):
            assert not np.array_equal(frame_of_quad(q + m, d), frame_of_quad(q, d) + 3 * d * g), (d, g, m)


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [7, 11])
def test_furthest_halo_frame_stays_inside_the_offset_guard(k, d):
    G = (k + 3) // 4
    H = (G - 1) * d
    lo = (k - 1) // 2 * d
    for T in SHAPES_T + [2 ** 20 + 3, 2 ** 22 - 1]:
        last_quad = q_tiles_per_item(T, d) * BQ + H - 1     # the last halo row of the item's last tile
        far = int(frame_of_quad(last_quad, d)) - lo + 6 * d  # its raw row 6
        # what the groups of the item's last quad read without the shared tile: the same frame
        assert far == int(frame_of_quad(last_quad - H, d)) + 4 * d * (G - 1) - lo + 6 * d
        # row `far` ends at byte (far + 1) * lda * 4 <= (T + GUARD_ROWS) * lda * 4 < 2^31
        assert far + 1 <= T + GUARD_ROWS, (k, d, T, far)
        # and it is less than 4 BQ + 4 d + 4 d (G - 1) + 6 d frames behind T: the margin of 1024 rows is not tight
        assert far < T + 4 * BQ + 4 * d * G + 6 * d
    # the smallest offset: raw row 0 of quad 0 is lo frames in front of the item: negative, i.e. >= 2^31 as the unsigned offset the
    # buffer range check sees, for every lda the guard admits
    assert int(frame_of_quad(0, d)) - lo < 0
