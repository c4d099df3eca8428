"""The device-side half of a "hold X to float64" test: guarded buffers, `hold` and `env`.

Test infrastructure (not a test file; tests/test_harness.py tests it on the CPU).  The kernel tests call
the C ABI on buffers of their own.  A `Buf` is how they find an over-run or an unwritten element without
a sanitizer: the buffer is filled with a value no kernel under test produces, a guard of the same value
lies behind it (and, misaligned, one word in front), and the test asks afterwards whether the guard is
intact and whether every element came out finite.  `hold` then compares every tensor with the float64
reference under the case module's own `rel_err` and `bound` (tests/yardstick.py) and reports all misses
at once.

pytest rewrites `assert` only in test_*.py, so every assertion here carries its values in its message.
"""
import math

import torch

NAN = float("nan")      # the default fill: an element a kernel did not write fails hold's finite check
SENT = -7777.25         # for files whose accumulator cases pre-fill through `fill`; no kernel produces it
ISENT = -7              # for int64 outputs: no label or frame count is negative
GUARD = 64              # the shortest guard, in elements


class Buf:
    """A device buffer of `shape` holding `fill` (or `src`), with a guard of max(GUARD, shape[-1])
    elements of `fill` behind it.  mis (float32 only): the first element is 4 bytes past a multiple of
    16, and the word in front is a guard too.  `.t` is the buffer, `.full` the whole allocation."""

    def __init__(self, dev, shape, src=None, mis=False, fill=NAN, dtype=torch.float32):
        shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (shape,)
        assert not mis or dtype == torch.float32, f"a misaligned Buf is float32, not {dtype}"
        self.fill, self.n, self.off = fill, math.prod(shape), (1 if mis else 0)
        self.full = torch.full((self.off + self.n + max(GUARD, shape[-1]),), fill, dtype=dtype, device=dev)
        self.t = self.full[self.off:self.off + self.n].view(shape)
        assert self.t.data_ptr() % 16 == (4 if mis else 0), \
            f"the buffer starts {self.t.data_ptr() % 16} bytes past a multiple of 16, wanted {4 if mis else 0}"
        if src is not None:
            self.t.copy_(src.reshape(shape))

    def _is_fill(self, x):
        return bool((torch.isnan(x) if self.fill != self.fill else x == self.fill).all())

    def intact(self, what):
        assert self._is_fill(self.full[self.off + self.n:]), f"{what}: the guard behind the buffer was written"
        assert self._is_fill(self.full[:self.off]), f"{what}: the word in front of the buffer was written"

    def untouched(self, what):
        assert self._is_fill(self.full), f"{what}: a refused call wrote its output"


def ptr(o):
    """The address of a Buf's buffer or of a tensor; None stays None (a NULL argument)."""
    return None if o is None else (o.t if isinstance(o, Buf) else o).data_ptr()


def env():
    """-> (the native module, the library, the current stream)."""
    from speech2text_amd import _native as N
    return N, N.lib(), N.stream()


def hold(cases, name, got, *, ref=None, alias=None, partial=False, exact=False):
    """Every tensor of `got` (name -> tensor or list of tensors) finite and within cases.bound(name, key)
    of the float64 reference under cases.rel_err, after a reshape to the reference's shape; all misses are
    reported together.  ref: instead of cases.reference(name).  alias: got key -> the reference key it is
    held to.  partial: `got` may name fewer tensors than the reference.  exact: the reference on the
    exactly representable inputs; a tensor in cases.EXACT_TENSORS must then equal it."""
    if ref is None:
        ref = cases.reference(name, exact) if exact else cases.reference(name)
    alias = alias or {}
    if not partial:
        keys = {alias.get(k, k) for k in got}
        assert keys == set(ref), f"{name}: tensors {sorted(keys)} against the reference's {sorted(ref)}"
    bad = []
    for k, v in got.items():
        rk = alias.get(k, k)
        r = ref[rk]
        if isinstance(r, (list, tuple)):
            v = [w.detach().cpu() for w in v]
        else:
            v = [v.detach().cpu().reshape(r.shape)]
        for w in v:
            assert bool(torch.isfinite(w).all()), f"{name} {k}: not finite"
        if not isinstance(r, (list, tuple)):
            v = v[0]
        if exact and rk in cases.EXACT_TENSORS:
            if not torch.equal(v.double(), r):
                bad.append(f"{name} {k}: differs from the reference on exact inputs at "
                           f"{(v.double() != r).nonzero()[:4].tolist()}")
            continue
        err, tol = cases.rel_err(v, r), cases.bound(name, rk)
        print(f"{name} {k}: err {err:.3e} bound {tol:.3e} ratio {err / tol:.3f}")
        if not err <= tol:
            bad.append(f"{name} {k}: err {err:.3e} > bound {tol:.3e}")
    assert not bad, "; ".join(bad)
