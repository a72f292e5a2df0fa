"""Guard bands for operator tests: a tensor handed to a kernel is a WINDOW of a larger buffer whose every other element holds a canary,
and `check()` afterwards proves that nothing outside the window was written.  No HIP here: CPU and CUDA tensors alike.

The canaries are NaNs with a payload (fp32 0x7FA5C3E1; int16 0x7FA5, a bf16 NaN, so every piece of a split3 operand is one): an INPUT pad
that leaks into a product poisons the result, and an output canary cannot be mistaken for data.  They are compared as INTEGERS — a float
comparison calls every NaN different from itself and equal to nothing, so it could neither pass an untouched buffer nor tell another NaN
written over a canary from the canary."""
import torch

CANARY = {torch.float32: 0x7FA5C3E1, torch.int16: 0x7FA5}
_BITS = {torch.float32: torch.int32, torch.int16: torch.int16}


def _canary_buffer(shape, dtype, device):
    return torch.full(shape, CANARY[dtype], dtype=_BITS[dtype], device=device).view(dtype)


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


def guarded(rows, cols, ld=None, *, before=2, after=2, col0=0, dtype=torch.float32, device="cpu", fill=None):
    """A (before + rows + after) x ld buffer of canaries and the (rows, cols) window of it that starts at row `before`, column `col0`
    (row stride ld; ld defaults to col0 + cols).  `fill`: a (rows, cols) tensor or a number copied into the window — an input; None leaves
    the window full of canaries, so an output element the kernel forgets is a NaN in the result.
    Returns (window, check).  check() raises AssertionError unless every element outside the window still holds the canary, bit for bit;
    the message names the first differing (row, column) of the BUFFER — window row r is buffer row before + r — and how many differ."""
    ld = col0 + cols if ld is None else ld
    if rows < 1 or cols < 1 or before < 0 or after < 0 or col0 < 0 or col0 + cols > ld:
        raise ValueError("guarded: the window must lie inside the rows of the buffer")
    buf = _canary_buffer((before + rows + after, ld), dtype, device)
    window = buf[before:before + rows, col0:col0 + cols]
    if fill is not None:
        window.copy_(fill) if torch.is_tensor(fill) else window.fill_(fill)

    def check():
        bad = buf.view(_BITS[dtype]) != CANARY[dtype]           # the integer comparison: see the module's docstring
        bad[before:before + rows, col0:col0 + cols] = False
        n, where = _first_difference(bad, ("row", "column"))
        assert n == 0, (f"{n} element(s) outside the ({rows}, {cols}) window at (row {before}, column {col0}) of the "
                        f"{before + rows + after} x {ld} buffer were written; the first is {where}")

    return window, check


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
