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


# ------------------------------------------------------------------------------------------------ int32, float64, N-D windows, integer pads
@pytest.mark.parametrize("dtype", [torch.int32, torch.float64])
def test_the_int32_and_float64_canaries(dtype):
    w, check = G.guarded(ROWS, COLS, LD, before=BEFORE, after=AFTER, col0=COL0, dtype=dtype)
    check()
    bits = _buffer_of(w, dtype).view(torch.int32 if dtype == torch.int32 else torch.int64)
    assert (bits == G.CANARY[dtype]).all() and bool(G.holds_canary(w).all())
    if dtype == torch.float64:
        assert torch.isnan(w).all() and G.CANARY[dtype] >> 52 == 0x7FF and G.CANARY[dtype] & ((1 << 52) - 1)      # a NaN with a payload
        assert struct.unpack("<Q", struct.pack("<d", w[0, 0].item()))[0] >> 52 == 0x7FF
    else:
        assert G.CANARY[dtype] == G.CANARY[torch.float32] and int(w[0, 0]) == 0x7FA5C3E1      # the fp32 pattern, far outside any index range
    w.fill_(3)
    check()
    assert not bool(G.holds_canary(w).any())
    for row, col, _ in REGIONS:
        keep = _buffer_of(w, dtype)[row, col].clone()
        _buffer_of(w, dtype)[row, col] = 3
        with pytest.raises(AssertionError, match=rf"^1 element\(s\) outside .* the first is row {row}, column {col}$"):
            check()
        _buffer_of(w, dtype)[row, col] = keep
    check()
    if dtype == torch.float64:
        _buffer_of(w, dtype)[0, 0] = float("nan")                      # the default NaN over the canary: only integers can tell
        with pytest.raises(AssertionError, match=r"the first is row 0, column 0$"):
            check()


@pytest.mark.parametrize("shape", [(), (1,), (7,), (5, 3), (3, 44, 4), (2, 3, 5, 8)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.int32, torch.int16])
def test_guarded_like_is_a_contiguous_aligned_window_of_any_shape(shape, dtype):
    w, check = G.guarded_like(shape, dtype)
    n = 1
    for d in shape:
        n *= d
    cols = shape[-1] if len(shape) >= 2 else n
    assert tuple(w.shape) == shape and w.is_contiguous() and w.dtype == dtype and w.numel() == n
    assert w.data_ptr() % 64 == 0 and w.storage_offset() % cols == 0          # whole guard rows in front, 64-byte aligned
    before, total = w.storage_offset() // cols, w.untyped_storage().nbytes() // w.element_size() // cols
    assert before >= 4 and before * cols >= 1024 and (total - before - n // cols) * cols >= 1024
    check()
    assert bool(G.holds_canary(w).all())
    w.fill_(1)
    check()
    flat = torch.as_strided(w, (total * cols,), (1,), 0)
    for at, row, col in ((w.storage_offset() - 1, before - 1, cols - 1), (w.storage_offset() + n, before + n // cols, 0), (0, 0, 0),
                         (total * cols - 1, total - 1, cols - 1)):
        keep = flat[at].clone()
        flat[at] = 1
        with pytest.raises(AssertionError, match=rf"^1 element\(s\) outside .* the first is row {row}, column {col}$"):
            check()
        flat[at] = keep
    check()


def test_guarded_like_fill_before_after_and_alignment():
    data = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    w, check = G.guarded_like((2, 3, 4), fill=data, before=5, after=3)
    assert torch.equal(w, data) and w.storage_offset() == 8 * 4          # 5 rows asked for: rounded up to 8 rows = 128 bytes
    assert w.untyped_storage().nbytes() == (8 + 6 + 3) * 4 * 4
    check()
    w8, _ = G.guarded_like((7,), torch.float64, before=1)
    assert w8.data_ptr() % 64 == 0 and w8.storage_offset() == 8 * 7      # float64 rows of 7: 8 of them are a multiple of 64 bytes
    s, check = G.guarded_like((), fill=2.5)
    assert s.dim() == 0 and s.item() == 2.5
    check()
    with pytest.raises(ValueError):
        G.guarded_like((3, 0))


def test_an_integer_input_is_padded_with_a_chosen_index_never_the_nan_pattern():
    table = torch.tensor([0, 3, 1, 2], dtype=torch.int32)
    w, check = G.guarded_like((4,), torch.int32, fill=table, pad=4)
    total = w.untyped_storage().nbytes() // 4
    flat = torch.as_strided(w, (total,), (1,), 0)
    assert torch.equal(w, table) and int((flat == 4).sum()) == total - 4 and not bool((flat == G.CANARY[torch.int32]).any())
    check()
    flat[w.storage_offset() + 4] = 5
    with pytest.raises(AssertionError, match=rf"^1 element\(s\) outside .* the first is row {w.storage_offset() // 4 + 1}, column 0$"):
        check()
    from tests.guarded_call import In
    with pytest.raises(ValueError, match="pad"):
        In("table", table)


# ------------------------------------------------------------------------------------------------ guarded_call discriminates
# The "operator": y[t] = 2 * x[table[t]] over x (R, C), an int32 table (T), y (T, C).  Mutants reach past a tensor only where its storage
# has room — in a guarded window — and fall back to what a plain tensor's neighbourhood "usually" holds, something finite, elsewhere.
R_, C_, T_ = 6, 5, 4


def _behind(t, n):
    """the n elements behind t in its storage, or None where the storage ends"""
    end = t.storage_offset() + t.numel()
    return torch.as_strided(t, (n,), (1,), end) if (end + n) * t.element_size() <= t.untyped_storage().nbytes() else None


def _op_correct(x, table, y):
    y.copy_(2 * x[table.long()])


def _op_writes_a_row_past_its_output(x, table, y):
    _op_correct(x, table, y)
    past = _behind(y, C_)
    if past is not None:
        past.copy_(2 * x[0])


def _op_skips_its_last_row(x, table, y):
    y[:-1].copy_(2 * x[table[:-1].long()])


def _op_reads_a_row_past_its_input(x, table, y):
    past = _behind(x, C_)
    _op_correct(x, table, y)
    y[-1] += 0 * (past if past is not None else torch.ones(C_))          # multiplied away — but 0 * NaN is NaN


def _op_scales_its_input_in_place(x, table, y):
    x.mul_(2)
    y.copy_(x[table.long()])


def _op_consumes_an_index_past_its_table(x, table, y):
    _op_correct(x, table, y)
    past, rows = _behind(table, 1), _behind(x, C_)
    if past is not None:
        i = int(past[0])
        y[-1] = 2 * (x[i] if i < R_ else rows)                             # the pad is index R: the row behind x


def _call(op):
    from tests.guarded_call import In, Out, guarded_call
    x = torch.arange(R_ * C_, dtype=torch.float32).reshape(R_, C_) + 1
    table = torch.tensor([5, 0, 3, 3], dtype=torch.int32)
    return guarded_call(op, [In("x", x), In("table", table, pad=R_), Out("y", (T_, C_))], tensors=True, label=op.__name__)


def test_guarded_call_passes_a_correct_operator():
    r = _call(_op_correct)
    assert torch.equal(r.guarded["y"], r.plain["y"]) and r.guarded["y"][0, 0] == 2 * 26


@pytest.mark.parametrize("op,message", [
    (_op_writes_a_row_past_its_output, r"output 'y': 5 element\(s\) outside the \(4, 5\) window .* were written; the first is row \d+, column 0"),
    (_op_skips_its_last_row, r"output 'y': 5 element\(s\) were never written \(they still hold the canary\), the first at flat index 15"),
    (_op_reads_a_row_past_its_input, r"output 'y': 5 element\(s\) differ from the same call on plain contiguous tensors, the first at flat index 15"),
    (_op_scales_its_input_in_place, r"input 'x': 30 element\(s\) of the input window were written, the first at flat index 0"),
    (_op_consumes_an_index_past_its_table, r"output 'y': 5 element\(s\) differ from the same call on plain contiguous tensors, the first at flat index 15"),
], ids=lambda v: v.__name__ if callable(v) else "")
def test_guarded_call_trips_on_each_mutant_and_names_the_tensor(op, message):
    with pytest.raises(AssertionError, match=message) as e:
        _call(op)
    assert e.value.args[0].startswith(op.__name__ + ": ")
    only = {"_op_writes_a_row_past_its_output": 1, "_op_skips_its_last_row": 2, "_op_scales_its_input_in_place": 1}
    if op.__name__ in only:                                                 # nothing else trips beside the assertion (and its consequence)
        assert f": {only[op.__name__]} failure(s):" in e.value.args[0], e.value.args[0]


def test_guarded_call_handles_in_place_buffers_workspaces_and_structs():
    """an InOut window is exempt from assertion 3 and compared with the plain in-place call; a workspace's contents are no contract, its
    guard rows are; a spec standing at two positions is ONE window; a non-zero return code fails with the library's text"""
    import ctypes as C
    from tests.guarded_call import In, InOut, Out, Struct, Ws, guarded_call

    def op(x, acc, out, ws):
        ws.copy_(torch.rand(ws.shape))                                      # differs between the two calls
        assert acc.data_ptr() == out.data_ptr()
        out.add_(x)

    acc = InOut("acc == out", torch.ones(3, 4))
    r = guarded_call(op, [In("x", torch.full((3, 4), 2.0)), acc, acc, Ws("ws", 7)], tensors=True)
    assert (r.guarded["acc == out"] == 3).all()

    def spills(x, acc, out, ws):
        op(x, acc, out, ws)
        _behind(ws, 1).fill_(0.0) if _behind(ws, 1) is not None else None
    with pytest.raises(AssertionError, match=r"workspace 'ws': 1 element\(s\) outside"):
        guarded_call(spills, [In("x", torch.full((3, 4), 2.0)), acc, acc, Ws("ws", 7)], tensors=True)

    class Pair(C.Structure):
        _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", C.c_int32)]
    seen = []

    def fake_entry_point(pair, scale):
        p = C.cast(pair, C.POINTER(Pair)).contents
        seen.append((p.src, p.dst, p.n, scale))
        C.memmove(p.dst, p.src, 4 * p.n)
        return 0
    r = guarded_call(fake_entry_point, [Struct(Pair, src=In("src", torch.arange(6.0)), dst=Out("dst", (6,)), n=6), 1.5])
    assert torch.equal(r.guarded["dst"], torch.arange(6.0)) and len(seen) == 2 and seen[0][0] == r.guarded["src"].data_ptr()
    with pytest.raises(AssertionError, match="the guarded call returned -1: bad argument"):
        guarded_call(lambda *a: -1, [In("src", torch.arange(6.0))], error_text=lambda: "bad argument")


# ------------------------------------------------------------------------------------------------ the case table against the header
_DEVICE_OUT_STRUCTS = ("thmr_outputs", "thmr_val_loss_out", "thmr_tokenizer_out", "thmr_jpeg_item")      # structs that carry device output pointers


def device_output_entry_points(text):
    """The entry points of the C text that take a device output pointer, by the header's own conventions: a parameter that is a
    non-const pointer named *_dev or *_or_null ("every pointer named *_dev is a device pointer owned by the caller"), or a pointer to one
    of the structs whose fields are such pointers.  A typed T** of such a name is a host table of device outputs; a void** is a host
    out-parameter that receives an address."""
    import re
    from tokenhmr_amd._cabi import parse_prototypes
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set()
    for name in parse_prototypes(text)[0]:
        params = re.search(rf"\b{name}\s*\(([^()]*)\)\s*;", text).group(1)
        for p in params.split(","):
            p = " ".join(p.split())
            m = re.fullmatch(r"(const )?(\w+)\s*(\*+)\s*(\w+)", p)
            if not m:
                continue
            const, base, stars, pname = m.groups()
            named = not const and pname.endswith(("_dev", "_or_null")) and (stars == "*" or (stars == "**" and base != "void"))
            if named or (stars == "*" and base in _DEVICE_OUT_STRUCTS):
                names.add(name)
    return names


def test_the_device_output_rule_on_a_small_header():
    text = """int thmr_a(const float* x_dev, float* y_dev, int32_t n, void* stream);      /* an output */
              int thmr_b(const float* x_dev, int32_t* idx_or_null, void* stream);         /* an optional output */
              int thmr_c(const float* x_dev, const int32_t* src_or_null, void* stream);   /* inputs only */
              int thmr_d(thmr_engine* e, void** ptr_dev, size_t* bytes);                   /* a host out-parameter */
              int thmr_e(const thmr_outputs* out, int32_t B, void* stream);               /* a struct of output pointers */
              int thmr_f(thmr_png_item* items_host, int32_t n, void* stream);             /* host memory */
              int thmr_g(const uint8_t** rows_host, uint8_t** out_dev, int32_t n);        /* a host table of device outputs */"""
    assert device_output_entry_points(text) == {"thmr_a", "thmr_b", "thmr_e", "thmr_g"}


def test_every_entry_point_with_a_device_output_is_guarded_or_exempt():
    """Coverage bookkeeping, without a GPU (the pattern of test_every_production_id_is_planned): every entry point of
    include/tokenhmr_hip.h that takes a device output pointer has its cases in tests/test_gpu_guard_bands.py::CASES or a stated reason in
    its EXEMPT — exactly one of the two — and neither names anything the header does not declare."""
    from tokenhmr_amd import _cabi
    from tests import test_gpu_guard_bands as GB
    with open(_cabi.HEADER) as f:
        names = device_output_entry_points(f.read())
    table, exempt = set(GB.CASES), set(GB.EXEMPT)
    assert len(names) > 50 and "thmr_op_layernorm" in names and "thmr_val_loss" in names and "thmr_smpl_forward" in names
    assert not table & exempt, sorted(table & exempt)
    assert not names - table - exempt, f"neither guarded nor exempt: {sorted(names - table - exempt)}"
    assert not (table | exempt) - names, f"not an entry point with a device output: {sorted((table | exempt) - names)}"
    assert all(isinstance(r, str) and len(r) > 10 for r in GB.EXEMPT.values())
    for entry, (builder, cases) in GB.CASES.items():
        assert callable(builder) and len(cases) >= 1 and all(isinstance(kw, dict) for kw in cases), entry
    assert len({p.id for p in GB._params()}) == sum(len(c) for _, c in GB.CASES.values())          # every case has an id of its own


def test_every_guarded_entry_point_has_a_statement_or_names_its_parity_tests():
    """Bit-equality with the plain call cannot tell a value that is wrong in both calls: every entry point of CASES has a float64 / exact
    statement of its own in STATEMENTS or names, in COVERED_BY, the parity tests that hold its shapes — exactly one of the two — and a
    named test file exists."""
    import os
    import re
    from tests import test_gpu_guard_bands as GB
    cases, st, cov = set(GB.CASES), set(GB.STATEMENTS), set(GB.COVERED_BY)
    assert not st & cov, sorted(st & cov)
    assert st | cov == cases, (sorted(cases - st - cov), sorted((st | cov) - cases))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for entry, text in GB.COVERED_BY.items():
        files = re.findall(r"tests/\w+\.py", text)
        assert files and all(os.path.exists(os.path.join(root, f)) for f in files), entry
        for f, t in re.findall(r"(tests/\w+\.py)::(test_\w+)", text):
            with open(os.path.join(root, f)) as fh:
                assert f"def {t}(" in fh.read(), (entry, f, t)


def test_the_floors_are_the_parity_files():
    """No tolerance of tests/test_gpu_guard_bands.py is new: the two it restates are the parity files' own."""
    from tests import test_gpu_guard_bands as GB
    from tests import test_gpu_smplh, test_gpu_val_loss, test_smpl_bounds
    assert GB.REL_FLOOR == test_gpu_val_loss.REL_FLOOR
    assert GB.TOL_M == test_smpl_bounds.TOL_M == test_gpu_smplh.FLOOR_M
