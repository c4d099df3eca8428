"""Seeded inputs shared by tests/test_lattice_f64.py (CPU) and tests/test_gpu_loss_lattices.py (GPU).

Test infrastructure (not a test file).  The large cases live here so that what fp32 costs the
reference is measured (CPU file) on exactly the inputs the kernels are later held to (GPU file),
and FP32_COST -- the measured figures, asserted by the CPU file -- is what the GPU file's bounds
are derived from.
"""
import numpy as np
import torch

import lattice_f64 as L


def draw_symbols(gen, B, S, C, blank):
    """(B,S) int64 labels uniform over the C-1 classes that are not `blank`."""
    r = torch.randint(0, C - 1, (B, S), generator=gen)
    return r + (r >= blank).long()


# ------------------------------------------------------------------ CTC at the dispatch edges
# name -> (U, V, blank); T follows from U.  2U+1 = 255/257 straddles <2>|<4>, 511/513 <4>|<8>,
# 1023/1025 <8>|<16>; U = 1023 is the kernel's limit (2047 states, 16 per thread).
CTC_EDGES = {"U127": (127, 11, 0), "U128": (128, 11, 10), "U255": (255, 12, 5),
             "U256": (256, 12, 0), "U511": (511, 9, 8), "U512": (512, 9, 3),
             "U1023": (1023, 10, 0)}
CTC_LARGE = {k: v for k, v in CTC_EDGES.items() if v[0] >= 255}


def ctc_case(name):
    """B = 4 ragged utterances: the full U over all T frames, an empty target, a long repeat run
    (which needs a blank between every pair), a short one.  Returns float32 logits (B,T,V), int64
    targets (B,U) drawn to exclude the blank, in_len, tgt_len, blank."""
    U, V, blank = CTC_EDGES[name]
    rng = np.random.default_rng(1000 + U)
    B, T = 4, U + U // 4 + 64
    tg = rng.integers(0, V - 1, size=(B, U))
    tg = tg + (tg >= blank)
    tl = np.array([U, 0, U - U // 8, max(1, U // 3)])
    tg[2, 5:5 + 24] = tg[2, 5]                                        # long repeat run
    il = np.zeros(B, dtype=np.int64)
    for b in range(B):
        need = int(tl[b] + (tg[b, 1:tl[b]] == tg[b, :max(tl[b] - 1, 0)]).sum())
        assert need + 8 <= T, (name, b, need, T)                      # feasible by construction
        il[b] = T if b == 0 else rng.integers(need + 8, T + 1)
    logits = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
    return logits, tg.astype(np.int64), il, tl.astype(np.int64), blank


# ------------------------------------------------------------------ C3 bench geometry of the loss
BENCH_B = 64          # the bench's own batch: the float64 side takes a few seconds on 16 CPUs


def bench_case():
    T, S, C, R, B = 248, 50, 500, 5, BENCH_B
    g = torch.Generator().manual_seed(2024)
    am = torch.randn(B, T, C, generator=g) * 2
    lm = torch.randn(B, S + 1, C, generator=g) * 2
    sym = draw_symbols(g, B, S, C, 0)
    tl = torch.randint(5, S + 1, (B,), generator=g); tl[0] = S; tl[1] = 0; tl[2] = 1
    el = torch.randint(S + 1, T + 1, (B,), generator=g); el[0] = T; el[3] = 199
    return dict(am=am, lm=lm, sym=sym, tl=tl, el=el, R=R, B=B, T=T, S=S, C=C)


def bench_reference(c, ranges, chunk=16):
    """float64 per-utterance simple and pruned losses and the gradients of
    0.5 mean(simple) + 0.5 mean(pruned) with the given ranges; utterances are independent, so the
    (B,T,R,C) float64 lattice is built `chunk` utterances at a time."""
    B = c["B"]
    out = dict(simple=[], pruned=[], d_am=[], d_lm=[])
    for i in range(0, B, chunk):
        sl = slice(i, i + chunk)
        am = c["am"][sl].detach().double().requires_grad_(True)
        lm = c["lm"][sl].detach().double().requires_grad_(True)
        bnd = L.make_boundary(c["tl"][sl], c["el"][sl])
        s = L.simple_neg(am, lm, c["sym"][sl], bnd)
        p = L.pruned_neg(am, lm, ranges[sl], c["sym"][sl], bnd)
        ((0.5 * s.sum() + 0.5 * p.sum()) / B).backward()
        out["simple"].append(s.detach()); out["pruned"].append(p.detach())
        out["d_am"].append(am.grad); out["d_lm"].append(lm.grad)
    return {k: torch.cat(v) for k, v in out.items()}


# ------------------------------------------------------------------ lattice rows at thread edges
ROW_EDGES = (64, 65, 128, 129, 1024)


def weights(B):
    """Distinct per-utterance weights with a zero and a negative one, about one in total
    magnitude (the size class of a mean over the batch)."""
    base = torch.tensor([1.3, 0.0, -0.7, 2.1, 0.4, 0.9, 1.7, -1.1])
    return (base.repeat((B + 7) // 8)[:B] * (1.0 + 0.01 * torch.arange(B)) / B).double()


def rows_case(rows):
    """S+1 = rows lattice rows over T = 20 frames: raw recursion operands (px with its -inf
    entries in place, py) and a simple-loss case with blank 2, both ragged with S_b = 0 and
    T_b = 1 utterances."""
    S, T, C = rows - 1, 20, 19
    g = torch.Generator().manual_seed(rows)
    mi_bnd = L.make_boundary([S, S - 1, 1, 0], [T, 9, T, 1])
    px = L._fix_for_boundary(torch.randn(4, S, T + 1, generator=g) - 2.0, mi_bnd)
    px[:, :, T] = L.NEG_INF
    py = torch.randn(4, S + 1, T, generator=g) - 2.0
    am = torch.randn(3, T, C, generator=g) * 2
    lm = torch.randn(3, S + 1, C, generator=g) * 2
    return dict(px=px, py=py, mi_bnd=mi_bnd, am=am, lm=lm, sym=draw_symbols(g, 3, S, C, 2),
                tl=torch.tensor([S, S // 2, 0]), el=torch.tensor([T, 13, 1]), blank=2,
                w=weights(3))


def rows_reference(c):
    """float64: raw recursion (scores, px_grad, py_grad) and the weighted simple loss."""
    sc, gx, gy = L.mutual_information(c["px"], c["py"], c["mi_bnd"])
    a = c["am"].detach().double().requires_grad_(True)
    l = c["lm"].detach().double().requires_grad_(True)
    neg = L.simple_neg(a, l, c["sym"], L.make_boundary(c["tl"], c["el"]), c["blank"])
    (c["w"] * neg).sum().backward()
    return dict(sc=sc, gx=gx, gy=gy, simple=neg.detach(), d_am=a.grad, d_lm=l.grad)


# ------------------------------------------------------------------ measured cost of fp32
# Deviation of the fp32 REFERENCE from float64 on the inputs above (tests/test_lattice_f64.py
# measures and asserts them).  CTC: torch.nn.functional.ctc_loss on an fp32 log_softmax vs
# oracle.ctc, reduction 'sum' (per-utterance loss, relative; gradient, absolute).  RNN-T:
# oracle.k2_rnnt in fp32 vs lattice_f64.
FP32_COST = {                      # measured value, rounded up to two digits
    "U255": dict(loss_rel=7.7e-7, grad_abs=1.3e-3),       # 7.664e-07  1.269e-03
    "U256": dict(loss_rel=2.0e-7, grad_abs=6.9e-4),       # 1.972e-07  6.874e-04
    "U511": dict(loss_rel=7.6e-7, grad_abs=2.3e-3),       # 7.596e-07  2.292e-03
    "U512": dict(loss_rel=3.3e-7, grad_abs=1.3e-3),       # 3.275e-07  1.298e-03
    "U1023": dict(loss_rel=4.1e-7, grad_abs=4.5e-3),      # 4.023e-07  4.459e-03
    # simple 4.372e-07, pruned 6.473e-07, d_am 6.972e-06, d_lm 8.034e-04
    "rnnt_bench": dict(simple_rel=4.4e-7, pruned_rel=6.5e-7, d_am_abs=7.0e-6, d_lm_abs=8.1e-4),
    # rows: raw recursion (score rel, px_grad abs, py_grad abs), weighted simple loss (rel, d_am, d_lm)
    # 1.619e-07 2.515e-05 1.484e-05 2.597e-07 1.213e-04 1.660e-04
    "rows64": dict(mi_rel=1.7e-7, mi_gx_abs=2.6e-5, mi_gy_abs=1.5e-5, simple_rel=2.6e-7,
                   d_am_abs=1.3e-4, d_lm_abs=1.7e-4),
    # 2.610e-07 2.298e-05 2.108e-05 8.643e-08 1.249e-05 1.677e-05
    "rows65": dict(mi_rel=2.7e-7, mi_gx_abs=2.3e-5, mi_gy_abs=2.2e-5, simple_rel=8.7e-8,
                   d_am_abs=1.3e-5, d_lm_abs=1.7e-5),
    # 1.382e-07 3.344e-05 2.006e-05 2.006e-07 3.031e-04 1.462e-04
    "rows128": dict(mi_rel=1.4e-7, mi_gx_abs=3.4e-5, mi_gy_abs=2.1e-5, simple_rel=2.1e-7,
                    d_am_abs=3.1e-4, d_lm_abs=1.5e-4),
    # 2.845e-07 5.876e-05 4.534e-05 2.436e-07 4.126e-04 1.487e-04
    "rows129": dict(mi_rel=2.9e-7, mi_gx_abs=5.9e-5, mi_gy_abs=4.6e-5, simple_rel=2.5e-7,
                    d_am_abs=4.2e-4, d_lm_abs=1.5e-4),
    # 5.724e-07 1.446e-03 6.789e-04 4.696e-07 5.301e-02 1.267e-03
    "rows1024": dict(mi_rel=5.8e-7, mi_gx_abs=1.5e-3, mi_gy_abs=6.8e-4, simple_rel=4.7e-7,
                     d_am_abs=5.4e-2, d_lm_abs=1.3e-3),
}


# ------------------------------------------------------------------ shared by the loss kernels' GPU files
def _kern():
    from speech2text_amd import kernels
    return kernels


def _np(t):
    return t.detach().cpu().double().numpy()


G_ATOL, G_RTOL = 3e-5, 2e-3            # gradients under weights that sum to about one


def _assert_grad(got, ref, atol=G_ATOL, rtol=G_RTOL, what=""):
    got, ref = _np(got), _np(ref)
    print(f"{what}: max abs dev {np.abs(got - ref).max():.3e} (atol {atol:.1e})")
    np.testing.assert_allclose(got, ref, atol=atol, rtol=rtol)


def bound(measured, floor):
    """4x what fp32 costs the reference, never tighter than the small-case bound (the loss suite's own
    rule, with a floor per quantity: not the one of tests/yardstick.py)."""
    return max(4.0 * measured, floor)
