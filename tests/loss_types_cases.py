"""Seeded inputs of the typed pruned RNN-T loss (rnnt_type / delay_penalty), shared by
tests/test_lattice_types_f64.py (CPU) and tests/test_gpu_loss_types.py (GPU).

Test infrastructure (not a test file), in the manner of tests/loss_cases.py.  The yardstick is
tests/lattice_types_f64.py in float64.  For the tall lattices (64 rows and more) the GPU bounds are
4x what fp32 costs that restatement on the same inputs: FP32_COST holds the figures, measured as the
restatement in fp32 against itself in float64 and rounded up to two digits.  The fp32 side is
RECORDED in tests/golden/loss_types_fp32.npz (`python tests/loss_types_cases.py` rewrites it): a live
fp32 figure moves between hosts.  The arrays are large but almost all zero (with T = rows + 4 a
path stays within five frames of the diagonal), so the compressed file is small.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lattice_types_f64 as LT          # noqa: E402
from loss_cases import ROW_EDGES, draw_symbols, weights   # noqa: E402

TYPES = LT.TYPES
PENALTIES = (0.0, 0.05)

# ------------------------------------------------------------------ direct cases (both loss paths)
# name -> (S, R, ranges given); B = 4, T = 20, C = 19.  "none" hands ranges=None to the loss.
SHAPES = {"R5": (7, 5, True), "R2": (7, 2, True), "full": (7, 8, True), "none": (7, 8, False)}
DIRECT_B, DIRECT_T, DIRECT_C = 4, 20, 19
# full length, T_b = S_b, empty transcript on one frame, a short one
DIRECT_TL, DIRECT_EL = (7, 5, 0, 3), (20, 5, 1, 12)


def direct_case(shape, blank=0, seed=0, scale=2.0, tl=DIRECT_TL, el=DIRECT_EL):
    """am / lm for the fused joiner and logits (B,T,R,C) for the materialised path, over the
    diagonal band lattice_types_f64.band_ranges: a band every type has a path through."""
    S, R, given = SHAPES[shape]
    B, T, C = len(tl), DIRECT_T, DIRECT_C
    g = torch.Generator().manual_seed(4000 + 17 * seed + R)
    am = torch.randn(B, T, C, generator=g) * scale
    lm = torch.randn(B, S + 1, C, generator=g) * scale
    logits = torch.randn(B, T, R, C, generator=g) * scale
    sym = draw_symbols(g, B, S, C, blank)
    tl, el = torch.tensor(tl), torch.tensor(el)
    ranges = LT.band_ranges(tl, el, S, T, R) if given else None
    return dict(am=am, lm=lm, logits=logits, sym=sym, tl=tl, el=el, ranges=ranges, blank=blank,
                w=weights(B), S=S, T=T, R=R, C=C, B=B)


def direct_reference(c, rnnt_type, pen, path, act="relu"):
    """float64: per-utterance loss and the gradients of sum_b w[b] loss[b] over the utterances
    whose loss is finite (an infeasible one has loss +inf and zero gradients)."""
    bnd = LT.make_boundary(c["tl"], c["el"])
    if path == "fused":
        leaves = [c["am"].double().requires_grad_(True), c["lm"].double().requires_grad_(True)]
        neg = LT.pruned_neg(leaves[0], leaves[1], c["ranges"], c["sym"], bnd, c["blank"], act,
                            rnnt_type, pen)
    else:
        leaves = [c["logits"].double().requires_grad_(True)]
        neg = LT.lattice_neg(leaves[0], c["ranges"], c["sym"], bnd, c["blank"], rnnt_type, pen)
    ok = torch.isfinite(neg)
    grads = torch.autograd.grad((c["w"] * torch.where(ok, neg, torch.zeros((), dtype=neg.dtype))).sum(),
                                leaves)
    return neg.detach(), [g.detach() for g in grads]


# ------------------------------------------------------------------ modified recursion, tall lattices
def mod_rows_case(rows):
    """S+1 = rows lattice rows over T = rows + 4 frames (a path needs T_b >= S_b): raw operands of
    the modified recursion, ragged, with T_b = S_b (one path), a short and an empty utterance."""
    S, T = rows - 1, rows + 4
    g = torch.Generator().manual_seed(7000 + rows)
    px = torch.randn(4, S, T, generator=g) - 2.0
    py = torch.randn(4, S + 1, T, generator=g) - 2.0
    return dict(px=px, py=py, bnd=LT.make_boundary([S, S - 1, 1, 0], [T, S - 1, 9, 1]))


@functools.lru_cache(maxsize=None)
def mod_rows_reference(rows):
    c = mod_rows_case(rows)
    sc, gx, gy = LT.mutual_information(c["px"], c["py"], c["bnd"])
    return dict(sc=sc, gx=gx, gy=gy)


def mod_rows_fp32(rows):
    c = mod_rows_case(rows)
    sc, gx, gy = LT.mutual_information(c["px"], c["py"], c["bnd"], torch.float32)
    return dict(sc=sc, gx=gx, gy=gy)


QUANTITIES = ("sc", "gx", "gy")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss_types_fp32.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def recorded_fp32(rows):
    """The fp32 restatement's recorded output on a rows case, as float32 tensors."""
    return {k: torch.from_numpy(_golden()[f"rows{rows}.{k}"]) for k in QUANTITIES}


def fp32_cost(rows, fp32=None):
    """(score rel, px_grad abs, py_grad abs): fp32 (recorded by default) against live float64."""
    ref = mod_rows_reference(rows)
    got = recorded_fp32(rows) if fp32 is None else fp32
    rel = float(((got["sc"].double() - ref["sc"]).abs() / ref["sc"].abs()).max())
    return (rel, float((got["gx"].double() - ref["gx"]).abs().max()),
            float((got["gy"].double() - ref["gy"]).abs().max()))


# the restatement in fp32 against itself in float64; measured value, rounded up to two digits
FP32_COST = {
    64: dict(mi_rel=9.5e-8, mi_gx_abs=3.3e-6, mi_gy_abs=1.3e-6),        # 9.426e-08 3.202e-06 1.221e-06
    65: dict(mi_rel=1.7e-7, mi_gx_abs=3.8e-6, mi_gy_abs=1.9e-6),        # 1.628e-07 3.700e-06 1.865e-06
    128: dict(mi_rel=2.5e-7, mi_gx_abs=3.6e-6, mi_gy_abs=1.9e-6),       # 2.487e-07 3.599e-06 1.801e-06
    129: dict(mi_rel=1.2e-7, mi_gx_abs=7.9e-6, mi_gy_abs=7.5e-6),       # 1.188e-07 7.844e-06 7.407e-06
    1024: dict(mi_rel=5.5e-7, mi_gx_abs=1.4e-4, mi_gy_abs=1.1e-4),      # 5.414e-07 1.342e-04 1.010e-04
}


def bound(measured, floor):
    """4x what fp32 costs the restatement, never tighter than the small-case bound (the rule of
    tests/loss_cases.py, not the one of tests/yardstick.py)."""
    return max(4.0 * measured, floor)


if __name__ == "__main__":
    out = {}
    for rows in ROW_EDGES:
        got = mod_rows_fp32(rows)
        for k in QUANTITIES:
            out[f"rows{rows}.{k}"] = got[k].numpy()
        print(rows, " ".join(f"{v:.3e}" for v in fp32_cost(rows, got)))
    np.savez_compressed(GOLDEN, **out)
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
