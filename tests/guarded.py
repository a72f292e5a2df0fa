"""Guard bands for operator tests: a tensor handed to a kernel is a WINDOW of a larger buffer whose every other element holds a canary,
and `check()` afterwards proves that nothing outside the window was written.  No HIP here: CPU and CUDA tensors alike.

The canaries are NaNs with a payload (fp32 0x7FA5C3E1; int16 0x7FA5, a bf16 NaN, so every piece of a split3 operand is one): an INPUT pad
that leaks into a product poisons the result, and an output canary cannot be mistaken for data.  They are compared as INTEGERS — a float
comparison calls every NaN different from itself and equal to nothing, so it could neither pass an untouched buffer nor tell another NaN
written over a canary from the canary.

Further element types: int32 (OUTPUTS only: index results, histograms) carries the fp32 pattern as an integer, float64 a NaN with a payload
(0x7FF5A5C3E1B2D4F6) compared as int64.  An integer INPUT (an index table, targets) must not be surrounded by that pattern — a kernel
that consumed it as an index would address memory far outside the test's buffers — so `pad=` puts a chosen in-range value into the guard
elements instead, and check() compares against that value.  `guarded_like` gives a contiguous window of any shape."""
import torch

CANARY = {torch.float32: 0x7FA5C3E1, torch.int16: 0x7FA5, torch.int32: 0x7FA5C3E1, torch.float64: 0x7FF5A5C3E1B2D4F6}
_BITS = {torch.float32: torch.int32, torch.int16: torch.int16, torch.int32: torch.int32, torch.float64: torch.int64}


def _canary_buffer(shape, dtype, device, pad=None):
    if pad is not None:
        return torch.full(shape, pad, dtype=dtype, device=device)
    return torch.full(shape, CANARY[dtype], dtype=_BITS[dtype], device=device).view(dtype)


def holds_canary(t):
    """Boolean tensor: which elements of `t` hold their type's canary, bit for bit (the integer comparison)."""
    return t.view(_BITS[t.dtype]) == CANARY[t.dtype]


def _first_difference(bad, names):
    """(count, "name a, name b ...") of a boolean tensor's True elements: how many, and the first in row-major order."""
    n = int(bad.sum())
    if n == 0:
        return 0, ""
    flat = int(torch.nonzero(bad.reshape(-1))[0])
    idx = []
    for size in reversed(bad.shape):
        idx.append(flat % size)
        flat //= size
    return n, ", ".join(f"{name} {i}" for name, i in zip(names, reversed(idx)))


def guarded(rows, cols, ld=None, *, before=2, after=2, col0=0, dtype=torch.float32, device="cpu", fill=None, pad=None):
    """A (before + rows + after) x ld buffer of canaries and the (rows, cols) window of it that starts at row `before`, column `col0`
    (row stride ld; ld defaults to col0 + cols).  `fill`: a (rows, cols) tensor or a number copied into the window — an input; None leaves
    the window full of canaries, so an output element the kernel forgets is a NaN in the result.
    Returns (window, check).  check() raises AssertionError unless every element outside the window still holds the canary, bit for bit;
    the message names the first differing (row, column) of the BUFFER — window row r is buffer row before + r — and how many differ.
    `pad`: the guard elements hold this value of `dtype` instead of the canary (integer inputs: see the module's docstring), and so does a
    window without `fill`; check() then compares against it."""
    ld = col0 + cols if ld is None else ld
    if rows < 1 or cols < 1 or before < 0 or after < 0 or col0 < 0 or col0 + cols > ld:
        raise ValueError("guarded: the window must lie inside the rows of the buffer")
    buf = _canary_buffer((before + rows + after, ld), dtype, device, pad)
    window = buf[before:before + rows, col0:col0 + cols]
    if fill is not None:
        window.copy_(fill) if torch.is_tensor(fill) else window.fill_(fill)

    def check():
        bad = (buf != pad) if pad is not None else (buf.view(_BITS[dtype]) != CANARY[dtype])      # the integer comparison: see the module's docstring
        bad[before:before + rows, col0:col0 + cols] = False
        n, where = _first_difference(bad, ("row", "column"))
        assert n == 0, (f"{n} element(s) outside the ({rows}, {cols}) window at (row {before}, column {col0}) of the "
                        f"{before + rows + after} x {ld} buffer were written; the first is {where}")

    return window, check


def _prod(shape):
    n = 1
    for d in shape:
        n *= int(d)
    return n


def guard_rows(cols, itemsize, at_least=0, elements=1024, align=64):
    """The smallest number of guard rows of `cols` elements that is >= at_least, holds >= `elements` elements and >= 4 rows, and is a whole
    multiple of `align` bytes — so that a window behind them starts as aligned as the buffer itself."""
    r = max(int(at_least), 4, -(-elements // cols))
    while (r * cols * itemsize) % align:
        r += 1
    return r


def guarded_like(shape, dtype=torch.float32, device="cpu", fill=None, *, before=None, after=None, pad=None, align=64):
    """A CONTIGUOUS window of any shape — 0-dim and 1-D included — for the operators that take plain contiguous buffers: a view of a guarded
    2-D buffer with ld == cols, cols the last dimension (1 row of numel elements for 0-dim and 1-D).  Returns (window, check) like `guarded`;
    check() names (row, column) of that 2-D buffer, window element [..., c] of flattened leading index r at row before + r, column c.
    before / after: guard ROWS of `cols` elements; by default at least 4 rows and 1024 elements each (a ragged workgroup's worth).  `before`
    is rounded UP until the guard in front is a multiple of `align` bytes: the window is then `align`-byte aligned (torch allocations are),
    which covers every alignment the C ABI documents (16 bytes for float4 rows, 8 for float2 rows and float64) — no entry point is handed
    a misaligned pointer here.  fill: a tensor of `shape`, a number, or None (canaries / `pad`: an output)."""
    shape = tuple(int(d) for d in shape)
    n = _prod(shape)
    if n < 1 or any(d < 1 for d in shape):
        raise ValueError("guarded_like: every dimension is at least 1")
    cols = shape[-1] if len(shape) >= 2 else n
    rows = n // cols
    itemsize = torch.empty((), dtype=dtype).element_size()
    before = guard_rows(cols, itemsize, 0 if before is None else before, 1024 if before is None else 0, align)
    after = guard_rows(cols, itemsize, 0, 1024, 1) if after is None else int(after)
    if torch.is_tensor(fill):
        fill = fill.reshape(rows, cols)
    window, check = guarded(rows, cols, before=before, after=after, dtype=dtype, device=device, fill=fill, pad=pad)
    return window.view(shape), check


def guarded_split3(rows, K, ld=None, *, before=2, after=2, device="cpu", fill=None):
    """`guarded` for a row-major split3 operand: int16 (rows, K/8, 3, 8) as a view of rows of 3 * ld int16 (ld in fp32-equivalents, as the
    C ABI counts a split3 row stride; K % 8 == 0, ld % 8 == 0).  check() reports int16 columns: chunk c, piece p, element e is 24 c + 8 p + e."""
    ld = K if ld is None else ld
    if K % 8 or ld % 8:
        raise ValueError("guarded_split3: K and ld are multiples of 8")
    window, check = guarded(rows, 3 * K, 3 * ld, before=before, after=after, dtype=torch.int16, device=device,
                            fill=None if fill is None else fill.reshape(rows, 3 * K))
    return window.unflatten(1, (K // 8, 3, 8)), check


def guarded_blocked(M, N, *, device="cpu"):
    """A ROW-BLOCKED split3 result [ceil(M / 32)][N / 8][3][32][8] (int16) full of canaries, with one whole guard block before and after.
    Returns (tensor, check).  check() raises AssertionError unless the guard blocks AND the pad rows M ... ceil(M / 32) * 32 - 1 of the last
    block — rows no kernel may write — still hold the canary; the message names the first differing (block, chunk, piece, row, element),
    blocks counted from the guard block in front (block 1 is the tensor's first), and how many differ."""
    if M < 1 or N < 8 or N % 8:
        raise ValueError("guarded_blocked: M >= 1, N a positive multiple of 8")
    nb = (M + 31) // 32
    buf = _canary_buffer((nb + 2, N // 8, 3, 32, 8), torch.int16, device)
    tensor = buf[1:nb + 1]

    def check():
        bad = buf != CANARY[torch.int16]                        # int16 against an integer: the integer comparison
        bad[1:nb] = False                                       # whole blocks: data
        bad[nb, :, :, :M - 32 * (nb - 1)] = False               # the rows of the last block that exist
        n, where = _first_difference(bad, ("block", "chunk", "piece", "row", "element"))
        assert n == 0, (f"{n} element(s) of the guard blocks or of pad rows {M} ... {32 * nb - 1} of a row-blocked ({M}, {N}) operand "
                        f"were written; the first is {where}")

    return tensor, check
