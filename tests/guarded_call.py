"""One calling convention for an operator call inside guard bands (tests/guarded.py).  A plain module: no pytest hooks.

`guarded_call(fn, args)` is given an entry point, and its argument list in the entry point's own order, where every BUFFER argument is one
of the specs below and everything else (counts, flags, a handle, a stream) is passed through:

    In(name, data, pad=None)     an input: a guarded window filled with `data`.  Integer inputs name a `pad` (see guarded.py): an in-range
                                 value that changes the result if a kernel consumes it.
    Out(name, shape, dtype)      an output: a guarded window left full of canaries.  nan_ok: the header defines NaN results for this case.
    InOut(name, data)            a buffer the call reads AND writes (a residual summed in place, counts that are accumulated).
    Ws(name, numel)              a caller-supplied workspace of exactly the stated size, full of canaries; its contents are no contract.
    Struct(ctype, **fields)      a C struct passed by reference whose fields are specs, numbers or None.
    None                         a null pointer.

The same spec object may stand at two positions (xout == resid).  The helper makes the call on the guarded windows, synchronises, makes the
SAME call on fresh plain contiguous copies (inputs cloned, outputs and workspaces zero-filled), and asserts, naming the tensor each time:

  1. check() holds for every guarded tensor, inputs included: nothing outside any window was written;
  2. no output element still holds the canary, and every floating-point output is finite (unless nan_ok);
  3. every input window is bit-equal to what was put in;
  4. every output is bit-equal to the plain call's — an over-read consumed a NaN canary or a result-changing integer pad, and the plain
     call is the form the parity tests already hold to float64.  Workspaces are excluded.

What the method cannot see: an over-read whose value is never used (a load past the end that is masked out, or multiplied away before a
NaN could spread — though NaN * 0 is still NaN), and an over-write that lands beyond the guard rows.

`fn` is a ctypes function (buffers are passed as addresses; a non-zero return code fails with `error_text()`), or with tensors=True any
Python callable that takes the tensors themselves — how tests/test_guarded_host.py proves on the CPU that each assertion discriminates."""
import ctypes as C

import torch

from tests import guarded as G


class _Spec:
    kind = "?"

    def __init__(self, name, before=None, after=None):
        self.name, self.before, self.after = name, before, after


class In(_Spec):
    kind, counts = "input", False

    def __init__(self, name, data, pad=None, **kw):
        super().__init__(name, **kw)
        self.data, self.pad = data, pad
        if not data.dtype.is_floating_point and pad is None and not self.counts:
            raise ValueError(f"{name}: an integer input names its pad value (an in-range index that changes the result)")


class InOut(In):
    """An integer buffer of this kind holds counts, not indices, and may keep the canary around it (pad=None)."""
    kind, counts = "input/output", True


class Out(_Spec):
    kind = "output"

    def __init__(self, name, shape, dtype=torch.float32, nan_ok=False, **kw):
        super().__init__(name, **kw)
        self.shape, self.dtype, self.nan_ok = tuple(shape), dtype, nan_ok


class Ws(Out):
    kind = "workspace"

    def __init__(self, name, numel, dtype=torch.float32, **kw):
        super().__init__(name, (int(numel),), dtype, **kw)


class Struct:
    def __init__(self, ctype, **fields):
        self.ctype, self.fields = ctype, fields


class Result:
    """guarded / plain: {name: tensor} of the two calls (the guarded ones are the windows)."""

    def __init__(self, guarded, plain):
        self.guarded, self.plain = guarded, plain


def _specs(args):
    seen, out = set(), []
    for a in args:
        for s in (a.fields.values() if isinstance(a, Struct) else (a,)):
            if isinstance(s, _Spec) and id(s) not in seen:
                seen.add(id(s))
                out.append(s)
    names = [s.name for s in out]
    if len(set(names)) != len(names):
        raise ValueError(f"two specs share a name: {names}")
    return out


def _bits(t):
    return t.contiguous().view(G._BITS[t.dtype]) if t.dtype in G._BITS else t


def _differ(a, b):
    """(count, first flat index) of the elements whose BITS differ"""
    bad = (_bits(a) != _bits(b)).reshape(-1)
    n = int(bad.sum())
    return n, (int(torch.nonzero(bad)[0]) if n else -1)


def _marshal(args, tensors, as_tensors, keep):
    out = []
    for a in args:
        if isinstance(a, Struct):
            st = a.ctype(**{k: (tensors[v.name].data_ptr() if isinstance(v, _Spec) else v) for k, v in a.fields.items()})
            keep.append(st)
            out.append(C.byref(st))
        elif isinstance(a, _Spec):
            out.append(tensors[a.name] if as_tensors else C.c_void_p(tensors[a.name].data_ptr()))
        else:
            out.append(a)
    return out


def guarded_call(fn, args, *, device="cpu", label="", tensors=False, error_text=None):
    specs = _specs(args)
    dev = torch.device(device)
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda *a: None)
    g, checks, plain = {}, {}, {}
    for s in specs:
        if isinstance(s, In):
            data = s.data.to(dev).contiguous()
            g[s.name], checks[s.name] = G.guarded_like(data.shape, data.dtype, dev, fill=data, pad=s.pad, before=s.before, after=s.after)
            plain[s.name] = data.clone()
        else:
            g[s.name], checks[s.name] = G.guarded_like(s.shape, s.dtype, dev, before=s.before, after=s.after)
            plain[s.name] = torch.zeros(s.shape, dtype=s.dtype, device=dev)
    keep = []
    for which in (g, plain):
        rc = fn(*_marshal(args, which, tensors, keep))
        sync()
        assert not rc, f"{label}: the {'guarded' if which is g else 'plain'} call returned {rc}: {error_text() if error_text else ''}"
    fails = []
    for s in specs:
        name, w = s.name, g[s.name]
        try:                                                                      # 1. nothing outside any window was written
            checks[name]()
        except AssertionError as e:
            fails.append(f"{s.kind} '{name}': {e}")
        if isinstance(s, Ws):
            continue
        if isinstance(s, In) and not isinstance(s, InOut):                        # 3. inputs are left as they were
            n, at = _differ(w, s.data.to(dev))
            if n:
                fails.append(f"input '{name}': {n} element(s) of the input window were written, the first at flat index {at}")
            continue
        if w.dtype in G.CANARY and not isinstance(s, InOut):                      # 2. every element written, and finite
            left = G.holds_canary(w).reshape(-1)
            if bool(left.any()):
                fails.append(f"output '{name}': {int(left.sum())} element(s) were never written (they still hold the canary), the first at "
                             f"flat index {int(torch.nonzero(left)[0])}")
        if w.dtype.is_floating_point and not getattr(s, "nan_ok", False):
            bad = ~(torch.isfinite(w) | G.holds_canary(w)).reshape(-1)            # an element never written is reported above, once
            if bool(bad.any()):
                fails.append(f"output '{name}': {int(bad.sum())} element(s) are not finite, the first at flat index {int(torch.nonzero(bad)[0])}")
        n, at = _differ(w, plain[name])                                           # 4. bit-equal to the plain call
        if n:
            fails.append(f"output '{name}': {n} element(s) differ from the same call on plain contiguous tensors, the first at flat index {at} "
                         f"(guarded {w.reshape(-1)[at].item()!r}, plain {plain[name].reshape(-1)[at].item()!r})")
    assert not fails, f"{label}: {len(fails)} failure(s):\n" + "\n".join(fails)
    return Result(g, plain)
