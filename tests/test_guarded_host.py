"""tests/guarded.py bites (CPU only): one element written in each region outside a window makes check() fail and name it; an untouched
buffer passes; NaN DATA inside the window does not trip the check; another NaN written over a canary does."""
import struct

import pytest
import torch

from tests import guarded as G

ROWS, COLS, LD, BEFORE, AFTER, COL0 = 5, 7, 12, 2, 3, 4          # window rows 2 ... 6, columns 4 ... 10 of a 10 x 12 buffer


def _buffer_of(window, dtype):
    """the whole guarded buffer behind a window, as a (rows, ld) tensor"""
    return torch.as_strided(window, (BEFORE + ROWS + AFTER, LD), (LD, 1), 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
def test_an_untouched_buffer_passes_and_holds_the_canary(dtype):
    w, check = G.guarded(ROWS, COLS, LD, before=BEFORE, after=AFTER, col0=COL0, dtype=dtype)
    assert w.shape == (ROWS, COLS) and w.stride() == (LD, 1) and w.dtype == dtype
    assert w.storage_offset() == BEFORE * LD + COL0
    check()
    bits = _buffer_of(w, dtype).view(torch.int32 if dtype == torch.float32 else torch.int16)
    assert (bits == G.CANARY[dtype]).all()                        # the window too: an output element never written stays a canary
    if dtype == torch.float32:
        assert torch.isnan(w).all()
        assert struct.unpack("<I", struct.pack("<f", w[0, 0].item()))[0] & 0x7F800000 == 0x7F800000
    else:
        assert torch.isnan(w.view(torch.bfloat16)).all()          # every bf16 piece of a split3 operand is a NaN


# (buffer row, buffer column, what it is)
REGIONS = [(BEFORE, COL0 - 1, "pad column left of the first row"), (BEFORE, COL0 + COLS, "pad column right of the first row"),
           (BEFORE + 2, LD - 1, "pad column of a middle row"), (BEFORE + 2, 0, "pad column of a middle row, buffer column 0"),
           (BEFORE + ROWS - 1, COL0 + COLS, "pad column of the last row"), (BEFORE + ROWS - 1, COL0 - 1, "pad column left of the last row"),
           (BEFORE - 1, COL0 + 3, "the row before the window"), (0, 0, "the buffer's first element"),
           (BEFORE + ROWS, COL0, "the row after the window"), (BEFORE + ROWS + AFTER - 1, LD - 1, "the buffer's last element")]


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
@pytest.mark.parametrize("row,col,what", REGIONS)
def test_one_written_element_fails_the_check_and_is_named(dtype, row, col, what):
    w, check = G.guarded(ROWS, COLS, LD, before=BEFORE, after=AFTER, col0=COL0, dtype=dtype, fill=1)
    _buffer_of(w, dtype)[row, col] = 3
    with pytest.raises(AssertionError, match=rf"^1 element\(s\) outside .* the first is row {row}, column {col}$"):
        check()


def test_the_count_and_the_first_of_several():
    w, check = G.guarded(ROWS, COLS, LD, before=BEFORE, after=AFTER, col0=COL0)
    buf = _buffer_of(w, torch.float32)
    buf[BEFORE + ROWS, 5] = 0.0
    buf[BEFORE + 1, COL0 + COLS] = 0.0
    buf[BEFORE + 1, 1] = 0.0
    with pytest.raises(AssertionError, match=rf"^3 element\(s\) .* the first is row {BEFORE + 1}, column 1$"):
        check()


def test_nan_data_in_the_window_passes_and_another_nan_over_a_canary_does_not():
    w, check = G.guarded(ROWS, COLS, LD, before=BEFORE, after=AFTER, col0=COL0, fill=float("nan"))
    assert torch.isnan(w).all()
    check()
    w.view(torch.int32).fill_(G.CANARY[torch.float32] ^ 1)         # NaNs one bit away from the canary, still inside the window
    check()
    _buffer_of(w, torch.float32)[BEFORE, COL0 - 1] = float("nan")  # the default NaN (0x7FC00000) over a canary: only integers can tell
    with pytest.raises(AssertionError, match=rf"the first is row {BEFORE}, column {COL0 - 1}$"):
        check()


def test_fill_copies_data_and_leaves_the_pads():
    data = torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS)
    w, check = G.guarded(ROWS, COLS, LD, before=BEFORE, after=AFTER, col0=COL0, fill=data)
    assert torch.equal(w, data)
    check()
    w.zero_()                                                      # a kernel writing all of its window, and only that
    check()


def test_guarded_refuses_a_window_outside_its_rows():
    with pytest.raises(ValueError):
        G.guarded(4, 8, 10, col0=3)
    with pytest.raises(ValueError):
        G.guarded_split3(4, 12)
    with pytest.raises(ValueError):
        G.guarded_blocked(37, 12)


def test_split3_window_is_the_4d_view_of_wider_rows():
    K, ld = 16, 24
    w, check = G.guarded_split3(3, K, ld, before=1, after=1)
    assert w.shape == (3, 2, 3, 8) and w.stride() == (3 * ld, 24, 8, 1) and w.dtype == torch.int16
    check()
    w.fill_(7)
    check()
    buf = torch.as_strided(w, (5, 3 * ld), (3 * ld, 1), 0)
    assert (buf[1:4, :3 * K] == 7).all() and (buf[1:4, 3 * K:] == G.CANARY[torch.int16]).all()
    buf[2, 3 * K] = 0                                              # the first pad chunk of the middle row
    with pytest.raises(AssertionError, match=rf"the first is row 2, column {3 * K}$"):
        check()


@pytest.mark.parametrize("M", [37, 200, 64])
def test_row_blocked_pad_rows_and_guard_blocks(M):
    N, nb = 16, (M + 31) // 32
    t, check = G.guarded_blocked(M, N)
    assert t.shape == (nb, N // 8, 3, 32, 8) and t.is_contiguous() and t.dtype == torch.int16
    check()
    last = M - 32 * (nb - 1)                                       # rows of the last block that exist
    t[:nb - 1] = 1
    t[nb - 1, :, :, :last] = 1                                     # what a kernel writes: every row below M
    check()
    spots = [("guard block in front", lambda: torch.as_strided(t, (1,), (1,), t.storage_offset() - 1), "block 0, chunk 1, piece 2, row 31, element 7"),
             ("guard block behind", lambda: torch.as_strided(t, (1,), (1,), t.storage_offset() + t.numel()), f"block {nb + 1}, chunk 0, piece 0, row 0, element 0")]
    if last < 32:
        spots += [("first pad row", lambda: t[nb - 1, 1, 2, last, 3:4], f"block {nb}, chunk 1, piece 2, row {last}, element 3"),
                  ("last pad row", lambda: t[nb - 1, 0, 0, 31, 0:1], f"block {nb}, chunk 0, piece 0, row 31, element 0")]
    for what, spot, named in spots:
        keep = spot().clone()
        spot().fill_(0)
        with pytest.raises(AssertionError, match=rf"^1 element\(s\) .* the first is {named}$"):
            check()
        spot().copy_(keep)
        check()
