"""The rule every "hold X to float64" test follows, stated once.

Test infrastructure (not a test file).  A kernel family is held to a float64 restatement (its
`*_f64.py`) on seeded cases (its `*_cases.py`).  What float32 costs the RESTATEMENT on a case, evaluated
on the CPU against float64, is recorded per tensor in the case module's table; a device tensor is then
allowed

    bound_of(figure) = max(FLOOR, MARGIN * figure)

of rel_err, so a bound is never anything a kernel produced.  The case modules keep their own
`bound(name, ...)`: the lookup into their table and any derived exception stay where they are
documented, and each ends in bound_of.  They re-export FLOOR, MARGIN, UNIT and rel_err under these
names.  tests/optim_cases.py, tests/loss_cases.py and tests/loss_types_cases.py follow other rules
and say so.

Also here: the few helpers the `test_*_f64.py` files shared by copy.  tests/guarded.py holds the
device-side half (guarded buffers and `hold`).
"""
import numpy as np
import torch

FLOOR = 2e-5            # test_gpu_conformer_layer.py's bound on LayerNorm / attention gradients
MARGIN = 8.0            # 2 x the loss suite's 4: the kernels' sigmoid / tanh / exp use the hardware
#                         exponential and reciprocal, each about an ulp looser than torch's CPU ones
UNIT = 2.0 ** -24       # one float32 rounding: a recorded figure below it says nothing a host would repeat

F64 = torch.float64
TOL = dict(atol=1e-12, rtol=1e-12)      # a restatement against autograd or a second form of itself


def rel_err(got, ref):
    """max |got - ref| relative to max |ref|, the error measure of every bound; of lists: the largest
    over the items, each relative to its own reference.  Shapes must agree: nothing broadcasts."""
    if isinstance(ref, (list, tuple)):
        return max(rel_err(a, b) for a, b in zip(got, ref))
    ref = ref.detach().double().cpu()
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, f"rel_err: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    return float((got - ref).abs().max() / (ref.abs().max() + 1e-300))


def bound_of(figure):
    """Allowed rel_err of a device tensor whose restatement costs `figure` in float32."""
    return max(FLOOR, MARGIN * figure)


# ------------------------------------------------------------------ shared by the case modules
def clamp(n, T):
    return max(0, min(int(n), T))


# ------------------------------------------------------------------ shared by the test_*_f64.py files
def _rn(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g, dtype=F64)


def _same(a, b, what=""):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), err_msg=what, **TOL)


def _grads(out, g, *leaves):
    for v in leaves:
        v.grad = None
    (out * g).sum().backward(retain_graph=True)
    return [v.grad.clone() for v in leaves]


def _leaf(v, dt, grad=True):
    return None if v is None else v.to(dt).clone().requires_grad_(grad)


class _Ids:
    """A tokenizer that hands the ids back (the decoders only call decode)."""

    def decode(self, t):
        return [int(x) for x in t]
