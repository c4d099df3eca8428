"""Seeded inputs of the smoothed simple loss, shared by tests/test_lattice_smoothed_f64.py (CPU)
and tests/test_gpu_loss_smoothed.py (GPU).

Test infrastructure (not a test file), in the manner of tests/loss_cases.py: what fp32 costs the
REFERENCE (oracle.k2_rnnt.rnnt_loss_smoothed in fp32 against tests/lattice_smoothed_f64.py) is
measured on exactly the inputs the kernels are later held to, and FP32_COST -- the measured figures,
asserted by the CPU file -- is what the GPU file's bounds are derived from.

The fp32 side of that measurement is RECORDED: tests/golden/loss_smoothed_fp32.npz holds what
oracle.k2_rnnt.rnnt_loss_smoothed returned in fp32 on every case on the host the table was measured
on (`python tests/loss_smoothed_cases.py` rewrites it).  An fp32 evaluation's largest deviation
from float64 on one small case is a single draw, and it follows the host: the same oracle on two x86
hosts (another libm, another blocking of the fp32 product) gave 4.14e-6 and 4.67e-6 for one px_grad
figure and 1.65e-6 and 1.47e-6 for one d_lm figure, so a live measurement cannot be asserted against
two recorded digits everywhere.  The live oracle is held to the recording loosely instead.
The float64 side is evaluated live; it moves by parts in 1e15 between hosts.
"""
import functools
import os
import sys

import numpy as np
import torch

import lattice_f64 as L
import lattice_smoothed_f64 as LS
import loss_cases as LC

# the slabs of rows of the two C-vector reductions of csrc/rnnt_smooth.hip
# (S2T_RNNT_SMOOTH_LM_SLAB rows of lm for u, S2T_RNNT_SMOOTH_AM_SLAB rows of am for dlogu)
LM_SLAB, AM_SLAB = 64, 32


def lengths(B, S, T):
    """Ragged (S_b, T_b): a full utterance, an empty transcript, a single frame, then a mix."""
    tl = [S, 0, (S + 1) // 2, max(S - 1, 0)] + [(3 * i) % (S + 1) for i in range(4, B)]
    el = [T, max(T - 3, 1), 1, max(T - 1, 1)] + [1 + (5 * i) % T for i in range(4, B)]
    return torch.tensor(tl[:B]), torch.tensor(el[:B])


# name -> (seed, B, T, S, C, blank, lm_only_scale, am_only_scale)
CASES = {
    # the four scale settings on one ragged batch with an S_b = 0 and a T_b = 1 utterance
    "lam": (1, 4, 20, 7, 33, 0, 0.25, 0.0),
    "mu": (1, 4, 20, 7, 33, 0, 0.0, 0.3),
    "both": (1, 4, 20, 7, 33, 0, 0.25, 0.1),
    "heavy": (1, 4, 20, 7, 33, 0, 0.5, 0.4),
    # class widths at the lane-stride edges of a wave-per-row kernel, and the C3 joiner's
    "C63": (63, 3, 12, 5, 63, 0, 0.25, 0.1),
    "C64": (64, 3, 12, 5, 64, 0, 0.25, 0.1),
    "C65": (65, 3, 12, 5, 65, 0, 0.25, 0.1),
    "C129": (129, 3, 12, 5, 129, 0, 0.25, 0.1),
    "C500": (500, 3, 12, 5, 500, 0, 0.25, 0.1),
    "blank_first": (2, 4, 20, 7, 33, 0, 0.25, 0.1),
    "blank_middle": (2, 4, 20, 7, 33, 16, 0.25, 0.1),
    "blank_last": (2, 4, 20, 7, 33, 32, 0.25, 0.1),
    # one step over the 256-frame tile of the px/py pass
    "T257": (257, 2, 257, 3, 16, 0, 0.25, 0.1),
    # B (S+1) lm rows | B T am rows around the slabs of the two column reductions (64 | 32)
    "rows_lm63_am33": (3, 3, 11, 20, 19, 1, 0.25, 0.1),
    "rows_lm64_am32": (4, 4, 8, 15, 19, 1, 0.25, 0.1),
    "rows_lm65_am35": (5, 5, 7, 12, 19, 1, 0.25, 0.1),
    "rows_lm6_am31": (6, 1, 31, 5, 19, 1, 0.25, 0.1),
    "rows_lm130_am64": (7, 2, 32, 64, 19, 1, 0.25, 0.1),
}
assert 3 * 21 == LM_SLAB - 1 and 3 * 11 == AM_SLAB + 1 and 4 * 16 == LM_SLAB and 4 * 8 == AM_SLAB
assert 5 * 13 == LM_SLAB + 1 and 1 * 31 == AM_SLAB - 1 and 2 * 65 == 2 * LM_SLAB + 2


def case(name):
    seed, B, T, S, C, blank, lam, mu = CASES[name]
    g = torch.Generator().manual_seed(9000 + seed)
    am = torch.randn(B, T, C, generator=g) * 2
    lm = torch.randn(B, S + 1, C, generator=g) * 2
    sym = LC.draw_symbols(g, B, S, C, blank)
    tl, el = lengths(B, S, T)
    return dict(am=am, lm=lm, sym=sym, tl=tl, el=el, blank=blank, lam=lam, mu=mu, w=LC.weights(B),
                B=B, T=T, S=S, C=C)


def reference_of(am, lm, sym, tl, el, blank, lam, mu, w):
    """float64, whole batch (u couples the utterances): per-utterance loss, the gradients of
    sum_b w[b] loss[b], and the occupation counts."""
    a = am.detach().double().requires_grad_(True)
    l = lm.detach().double().requires_grad_(True)
    bnd = L.make_boundary(tl, el)
    neg = LS.smoothed_neg(a, l, sym, bnd, blank, lam, mu)
    d_am, d_lm = torch.autograd.grad((w * neg).sum(), (a, l))
    gx, gy = LS.occupation(a, l, sym, bnd, blank, lam, mu)
    return dict(neg=neg.detach(), d_am=d_am, d_lm=d_lm, gx=gx, gy=gy)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once per process and shared; callers must not modify it."""
    c = case(name)
    return reference_of(c["am"], c["lm"], c["sym"], c["tl"], c["el"], c["blank"], c["lam"],
                        c["mu"], c["w"])


def oracle(c, dtype):
    """oracle.k2_rnnt.rnnt_loss_smoothed in `dtype`: per-utterance loss, gradients of
    sum_b w[b] loss[b], occupation counts."""
    from oracle import k2_rnnt as K
    am = c["am"].to(dtype).requires_grad_(True)
    lm = c["lm"].to(dtype).requires_grad_(True)
    bnd = L.make_boundary(c["tl"], c["el"])
    loss, (gx, gy) = K.rnnt_loss_smoothed(lm, am, c["sym"], c["blank"], bnd, c["lam"], c["mu"],
                                          reduction="none", return_grad=True)
    d_am, d_lm = torch.autograd.grad((c["w"].to(dtype) * loss).sum(), (am, lm))
    return dict(neg=loss.detach(), d_am=d_am, d_lm=d_lm, gx=gx, gy=gy)


QUANTITIES = ("neg", "d_am", "d_lm", "gx", "gy")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_smoothed_fp32.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def recorded_fp32(name):
    """The fp32 oracle's recorded output on a case, as float32 tensors."""
    return {k: torch.from_numpy(_golden()[f"{name}.{k}"]) for k in QUANTITIES}


# ------------------------------------------------------------------ measured cost of fp32
# Deviation of oracle.k2_rnnt.rnnt_loss_smoothed in fp32 (as recorded, see above) from the float64
# restatement on the cases above, under the weights LC.weights(B): per-utterance loss (relative), d_am,
# d_lm, px_grad, py_grad (absolute).  Measured and asserted by tests/test_lattice_smoothed_f64.py; the
# value is the measurement rounded up to two digits, the raw figures are in the comment above each entry.
FP32_COST = {
    # 1.394e-07 5.146e-06 4.565e-05 1.039e-05 1.502e-05
    "lam": dict(loss_rel=1.4e-7, d_am_abs=5.2e-6, d_lm_abs=4.6e-5, gx_abs=1.1e-5, gy_abs=1.6e-5),
    # 6.871e-08 4.130e-06 1.253e-05 5.740e-06 7.629e-06
    "mu": dict(loss_rel=6.9e-8, d_am_abs=4.2e-6, d_lm_abs=1.3e-5, gx_abs=5.8e-6, gy_abs=7.7e-6),
    # 7.718e-08 4.606e-06 1.430e-05 3.131e-06 1.133e-05
    "both": dict(loss_rel=7.8e-8, d_am_abs=4.7e-6, d_lm_abs=1.5e-5, gx_abs=3.2e-6, gy_abs=1.2e-5),
    # 1.307e-07 2.962e-06 3.707e-05 6.280e-06 1.042e-05
    "heavy": dict(loss_rel=1.4e-7, d_am_abs=3.0e-6, d_lm_abs=3.8e-5, gx_abs=6.3e-6, gy_abs=1.1e-5),
    # 7.094e-08 1.332e-06 4.723e-06 2.034e-06 4.145e-06
    "C63": dict(loss_rel=7.1e-8, d_am_abs=1.4e-6, d_lm_abs=4.8e-6, gx_abs=2.1e-6, gy_abs=4.2e-6),
    # 5.792e-08 1.005e-06 2.841e-06 2.727e-06 9.537e-06
    "C64": dict(loss_rel=5.8e-8, d_am_abs=1.1e-6, d_lm_abs=2.9e-6, gx_abs=2.8e-6, gy_abs=9.6e-6),
    # 1.750e-07 2.855e-06 1.992e-05 3.669e-06 6.615e-06
    "C65": dict(loss_rel=1.8e-7, d_am_abs=2.9e-6, d_lm_abs=2.0e-5, gx_abs=3.7e-6, gy_abs=6.7e-6),
    # 2.512e-08 8.933e-07 2.375e-06 2.092e-06 2.171e-06
    "C129": dict(loss_rel=2.6e-8, d_am_abs=9.0e-7, d_lm_abs=2.4e-6, gx_abs=2.1e-6, gy_abs=2.2e-6),
    # 8.397e-08 3.377e-06 1.344e-05 4.499e-06 7.629e-06
    "C500": dict(loss_rel=8.4e-8, d_am_abs=3.4e-6, d_lm_abs=1.4e-5, gx_abs=4.5e-6, gy_abs=7.7e-6),
    # 1.022e-07 5.717e-06 8.618e-05 6.298e-06 1.419e-05
    "blank_first": dict(loss_rel=1.1e-7, d_am_abs=5.8e-6, d_lm_abs=8.7e-5, gx_abs=6.3e-6,
                        gy_abs=1.5e-5),
    # 6.910e-08 5.792e-06 1.508e-05 9.384e-06 1.308e-05
    "blank_middle": dict(loss_rel=7.0e-8, d_am_abs=5.8e-6, d_lm_abs=1.6e-5, gx_abs=9.4e-6,
                         gy_abs=1.4e-5),
    # 7.329e-08 3.107e-06 2.276e-05 4.993e-06 1.049e-05
    "blank_last": dict(loss_rel=7.4e-8, d_am_abs=3.2e-6, d_lm_abs=2.3e-5, gx_abs=5.0e-6,
                       gy_abs=1.1e-5),
    # 2.045e-07 5.528e-05 6.629e-03 9.084e-05 3.961e-04
    "T257": dict(loss_rel=2.1e-7, d_am_abs=5.6e-5, d_lm_abs=6.7e-3, gx_abs=9.1e-5, gy_abs=4.0e-4),
    # 1.161e-07 5.277e-06 8.911e-06 8.359e-06 8.402e-06
    "rows_lm63_am33": dict(loss_rel=1.2e-7, d_am_abs=5.3e-6, d_lm_abs=9.0e-6, gx_abs=8.4e-6,
                           gy_abs=8.5e-6),
    # 4.132e-08 2.492e-06 3.675e-06 1.072e-05 7.007e-06
    "rows_lm64_am32": dict(loss_rel=4.2e-8, d_am_abs=2.5e-6, d_lm_abs=3.7e-6, gx_abs=1.1e-5,
                           gy_abs=7.1e-6),
    # 9.196e-08 1.236e-06 1.646e-06 4.136e-06 3.815e-06
    "rows_lm65_am35": dict(loss_rel=9.2e-8, d_am_abs=1.3e-6, d_lm_abs=1.7e-6, gx_abs=4.2e-6,
                           gy_abs=3.9e-6),
    # 7.604e-08 8.788e-06 1.332e-04 7.776e-06 9.279e-06
    "rows_lm6_am31": dict(loss_rel=7.7e-8, d_am_abs=8.8e-6, d_lm_abs=1.4e-4, gx_abs=7.8e-6,
                          gy_abs=9.3e-6),
    # 5.586e-08 6.858e-05 6.336e-05 5.849e-05 3.136e-05
    "rows_lm130_am64": dict(loss_rel=5.6e-8, d_am_abs=6.9e-5, d_lm_abs=6.4e-5, gx_abs=5.9e-5,
                            gy_abs=3.2e-5),
}


def bounds(name, loss_rtol, grad_atol, occ_atol):
    """The GPU file's bounds for a case: 4x what fp32 costs the reference there, never tighter
    than the floors (tests/test_gpu_loss_lattices.py's bounds for the same quantities)."""
    rec = FP32_COST[name]
    return dict(loss=LC.bound(rec["loss_rel"], loss_rtol), d_am=LC.bound(rec["d_am_abs"], grad_atol),
                d_lm=LC.bound(rec["d_lm_abs"], grad_atol), gx=LC.bound(rec["gx_abs"], occ_atol),
                gy=LC.bound(rec["gy_abs"], occ_atol))


if __name__ == "__main__":                      # re-record the fp32 side (then re-measure FP32_COST)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    torch.set_num_threads(1)
    out = {}
    for case_name in CASES:
        for key, val in oracle(case(case_name), torch.float32).items():
            out[f"{case_name}.{key}"] = val.detach().numpy().astype(np.float32)
    np.savez(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
