"""The layout arithmetic of tests/large_util.py, without a GPU: wherever a far row would land if its offset were cut to 32
bits, it lands inside the arena and not where it belongs; and the residue facts that the many-rows shape rests on.  This is
the proof that tests/test_gpu_large.py can fail without a fault: no broken kernel is ever built to show it."""
import numpy as np
import pytest

import large_util as lu

ELEM_SIZES = (2, 4, 8)
ROW_LENGTHS = (20, 46, 260, lu.TAIL)


def test_residue_facts():
    assert 2 ** 16 % lu.PERIOD == 36 != 0 and lu.ROWS % lu.PERIOD == 101 != 0
    assert lu.ROWS > 2 ** 16 and lu.ROWS % 16 and lu.ROWS % 64
    assert all(lu.PERIOD % d for d in range(2, lu.PERIOD))                        # prime
    res = lu.residues()
    # a row index cut to 16 bits meets another residue class in every row past 2^16
    r = np.arange(2 ** 16, lu.ROWS)
    assert (res[r] != res[r & 0xFFFF]).all()
    # and so does a row that a second lap of a grid capped at 65 536 would serve one lap early or late
    assert (res[r] != res[r - 2 ** 16]).all()
    m = lu.shuffled_map()
    assert (res[m] == res).all() and (m != np.arange(lu.ROWS)).sum() > lu.ROWS - 2 * lu.PERIOD


@pytest.mark.parametrize("elem_size", ELEM_SIZES)
@pytest.mark.parametrize("stride", (lu.STRIDE, lu.STRIDE + 1))
def test_every_cut_offset_lands_inside_the_arena_and_elsewhere(elem_size, stride):
    rows = lu.far_rows(elem_size)
    total = lu.arena_bytes(elem_size)
    assert lu.arena_elems(elem_size) >= lu.row_start(rows - 1, stride) + lu.TAIL
    starts = [lu.row_start(r, stride) * elem_size for r in range(rows)]
    # the shape of the issue: row 1 past 2^31 elements and 2^32 bytes from the matrix, the last of three past 2^32 elements
    assert starts[1] - starts[0] > 2 ** 31 * elem_size and starts[1] - starts[0] >= 2 ** 32
    assert rows == 2 or starts[2] - starts[0] > 2 ** 32 * elem_size
    for r in range(1, rows):
        for mode, at in lu.wrapped(r, stride, elem_size).items():
            for n in ROW_LENGTHS:
                assert 0 <= at and at + n * elem_size <= total, (r, mode, n)     # inside: wrong bits, not a fault
            assert at % elem_size == 0
            if (r, mode) == (1, "u32 elements"):
                # the one cut that loses nothing: S < 2^32, so row 1's element offset fits an unsigned word.  Row 2 is there
                # for it; a matrix of two rows (8-byte elements) cannot see this cut, and DESIGN.md says so.
                assert at == starts[1]
                continue
            assert at != starts[r], (r, mode)                                     # not where the row is
            assert at not in starts, (r, mode)                                    # nor exactly on another row
    if rows == 3:
        assert all(lu.wrapped(2, stride, elem_size)[m] != starts[2] for m in lu.MODES)   # row 2 sees every mode
    # row 0 has no offset to cut
    assert set(lu.wrapped(0, stride, elem_size).values()) == {starts[0]}


def test_arena_sizes():
    gib = 2.0 ** 30
    assert 24.0 <= lu.arena_bytes(4) / gib < 24.1
    assert 12.0 <= lu.arena_bytes(2) / gib < 12.1
    assert 32.0 <= lu.arena_bytes(8) / gib < 32.1
    assert lu.STRIDE % 4 == 0 and lu.MARGIN % 4 == 0 and (lu.STRIDE + 1) % 4 == 1


def test_pattern_is_a_number_under_every_view():
    for dt in (np.float32, np.float64):
        v = lu.pattern_word(dt)
        assert np.isfinite(v) and abs(v) >= np.finfo(dt).tiny
    assert lu.pattern_word(np.int16) == -23131 and lu.pattern_word(np.uint8) == lu.PATTERN
