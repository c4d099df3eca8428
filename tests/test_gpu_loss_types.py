"""GPU: the typed pruned RNN-T loss (rnnt_type regular / modified / constrained, delay_penalty) of
csrc/rnnt.hip against float64.

Every kernel is reached through speech2text_amd.kernels (the parity test through the C ABI itself)
and compared with tests/lattice_types_f64.py, which tests/test_lattice_types_f64.py pins by path
enumeration.  Inputs are seeded (tests/loss_types_cases.py); every case that is not marked
infeasible has a finite float64 score, asserted here and on the CPU.

Bounds are those of tests/test_gpu_loss_lattices.py: loss rtol 1e-4; gradients atol 3e-5, rtol 2e-3
under per-utterance weights that sum to about one (a zero and a negative one included); raw
occupation gradients atol 2e-4.  The modified recursion on lattices of 64 rows and more takes 4x
what fp32 costs the restatement on the same inputs (loss_types_cases.FP32_COST), never tighter than
the small-case bound:

  rows   fp32 restatement vs float64 (score rel, px_grad, py_grad)   bounds used
  64     9.5e-8   3.3e-6   1.3e-6                                    2e-5, 2e-4, 2e-4 (floors)
  65     1.7e-7   3.8e-6   1.9e-6                                    floors
  128    2.5e-7   3.6e-6   1.9e-6                                    floors
  129    1.2e-7   7.9e-6   7.5e-6                                    floors
  1024   5.5e-7   1.4e-4   1.1e-4                                    2e-5, 5.6e-4, 4.4e-4

Padded frames are checked for the two new types.  The regular instantiation is the parent's code,
bit for bit, and keeps the parent's behaviour there (its backward multiplies a zero occupation by
the padded values).
"""
import numpy as np
import pytest
import torch

import lattice_f64 as L
import lattice_types_f64 as LT
import loss_cases as LC
import loss_types_cases as TC
from loss_cases import _assert_grad, _kern, _np

pytestmark = pytest.mark.gpu

RNNT_RTOL = 1e-4                       # losses
MI_ATOL = 2e-4                         # raw occupation gradients
NEW_TYPES = ("modified", "constrained")


def _assert_loss(got, ref, what=""):
    got, ref = _np(got), _np(ref)
    fin = np.isfinite(ref)
    print(f"{what}: loss max rel dev {np.abs(got[fin] / ref[fin] - 1).max() if fin.any() else 0:.3e}")
    assert np.array_equal(got[~fin], ref[~fin])            # +inf where there is no path
    np.testing.assert_allclose(got[fin], ref[fin], rtol=RNNT_RTOL)


def _run_device(dev, c, rnnt_type, pen, path, act="relu", am=None, lm=None, logits=None):
    """Loss (B,) and the gradients of sum_b w[b] loss[b] on the device; the weights go in as the
    gradient of the per-utterance losses, so an infinite loss does not spoil the sum."""
    k = _kern()
    bnd = k.make_boundary(c["tl"], c["el"], dev)
    rg = c["ranges"]
    if path == "fused":
        leaves = [(c["am"] if am is None else am).to(dev).requires_grad_(True),
                  (c["lm"] if lm is None else lm).to(dev).requires_grad_(True)]
        per = k.rnnt_pruned_joiner_loss(leaves[0], leaves[1], None if rg is None else rg.to(dev),
                                        c["sym"].to(dev), bnd, c["blank"], act, rnnt_type, pen)
    else:
        leaves = [(c["logits"] if logits is None else logits).to(dev).requires_grad_(True)]
        per = k.rnnt_lattice_loss(leaves[0], None if rg is None else rg.to(dev), c["sym"].to(dev),
                                  bnd, c["blank"], rnnt_type, pen)
    assert per.shape == (c["B"],)
    grads = torch.autograd.grad(per, leaves, grad_outputs=c["w"].float().to(dev))
    return per, grads


def _check(dev, c, rnnt_type, pen, path, act="relu", infeasible=()):
    ref, ref_grads = TC.direct_reference(c, rnnt_type, pen, path, act)
    for b in range(c["B"]):
        assert bool(torch.isfinite(ref[b])) == (b not in infeasible), (b, ref)
    per, grads = _run_device(dev, c, rnnt_type, pen, path, act)
    _assert_loss(per, ref, f"{rnnt_type} {pen} {path}")
    for g, r, name in zip(grads, ref_grads, ("d_am", "d_lm") if path == "fused" else ("d_logits",)):
        assert torch.isfinite(g).all()
        _assert_grad(g, r, what=name)
        for b in infeasible:
            assert (g[b] == 0).all()
    return per, grads


# ------------------------------------------------------------------ types x penalty x paths
@pytest.mark.parametrize("path,act", [("fused", "relu"), ("fused", "tanh"), ("logits", "relu")])
@pytest.mark.parametrize("pen", TC.PENALTIES)
@pytest.mark.parametrize("rnnt_type", TC.TYPES)
@pytest.mark.parametrize("shape", list(TC.SHAPES))
def test_types_and_penalty_on_both_paths(dev, shape, rnnt_type, pen, path, act):
    """B=4, T=20, S=7, C=19 with R=5, R=2, R=S+1 and ranges=None: pruned_{fwd,dam,dlm}_kernel and
    lattice_{fwd,bwd}_kernel in every TYPE instantiation, the recursion of either topology."""
    _check(dev, TC.direct_case(shape), rnnt_type, pen, path, act)


@pytest.mark.parametrize("rnnt_type", NEW_TYPES)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_blank_position(dev, where, rnnt_type):
    blank = {"first": 0, "middle": 9, "last": TC.DIRECT_C - 1}[where]
    c = TC.direct_case("R5", blank=blank, seed=1)
    assert (c["sym"] != blank).all()
    _check(dev, c, rnnt_type, 0.05, "fused")
    _check(dev, c, rnnt_type, 0.05, "logits")


# ------------------------------------------------------------------ the raw modified recursion
def _check_raw_mod(dev, px, py, bnd, sc_rtol=2e-5, gx_atol=MI_ATOL, gy_atol=MI_ATOL, ref=None):
    k = _kern()
    if ref is None:
        sc, rgx, rgy = LT.mutual_information(px, py, bnd)
    else:
        sc, rgx, rgy = ref["sc"], ref["gx"], ref["gy"]
    assert torch.isfinite(sc).all()
    ans, p, gx, gy = k.mutual_information(px.to(dev).contiguous(), py.to(dev).contiguous(), bnd.to(dev))
    assert gx.shape == px.shape and gy.shape == py.shape and p.shape == (px.shape[0], px.shape[1] + 1, px.shape[2] + 1)
    np.testing.assert_allclose(_np(ans), _np(sc), rtol=sc_rtol, atol=1e-4)
    _assert_grad(gx, rgx, atol=gx_atol, rtol=1e-7, what="px_grad")
    _assert_grad(gy, rgy, atol=gy_atol, rtol=1e-7, what="py_grad")


@pytest.mark.parametrize("rows", LC.ROW_EDGES)
def test_modified_recursion_rows_at_the_thread_count_edges(dev, rows):
    """S+1 lattice rows = threads of mi_mod_*_kernel's workgroup, rounded up to whole waves (64 | 65
    -> 64 | 128 threads, 128 | 129 -> 128 | 192, 1024 = the limit), T = rows + 4, with T_b = S_b."""
    c = TC.mod_rows_case(rows)
    cost = TC.FP32_COST[rows]
    _check_raw_mod(dev, c["px"], c["py"], c["bnd"], TC.bound(cost["mi_rel"], 2e-5),
                   TC.bound(cost["mi_gx_abs"], MI_ATOL), TC.bound(cost["mi_gy_abs"], MI_ATOL),
                   ref=TC.mod_rows_reference(rows))


def test_modified_recursion_frame_counts_around_the_look_ahead(dev):
    """T_b in {1, 7, 8, 9, 16, 17} at S = 3 (groups of 8 frames are requested ahead), S_b = 0 and
    S_b = T_b among them; -inf entries in px and py."""
    S, T = 3, 17
    tbs = [1, 7, 8, 9, 16, 17, 3, 12]
    sbs = [1, 3, 0, 3, 2, 3, 3, 0]
    g = torch.Generator().manual_seed(77)
    px = torch.randn(len(tbs), S, T, generator=g) - 2.0
    py = torch.randn(len(tbs), S + 1, T, generator=g) - 2.0
    px[1, 1, 2] = LT.NEG_INF; py[3, 0, 0] = LT.NEG_INF; py[5, 3, 16] = LT.NEG_INF
    _check_raw_mod(dev, px, py, LT.make_boundary(sbs, tbs))


def test_modified_recursion_rows_above_the_limit_are_refused(dev):
    k = _kern()
    S, T = 1024, 4
    px = torch.zeros(1, S, T, device=dev); py = torch.zeros(1, S + 1, T, device=dev)
    with pytest.raises(ValueError, match="1024"):
        k.mutual_information(px, py, k.make_boundary(torch.tensor([S]), torch.tensor([T]), dev))


# ------------------------------------------------------------------ fused joiner widths
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("C", [128, 129, 256, 257, 512, 513, 1024])
def test_fused_constrained_joiner_at_every_width(dev, C, act):
    """pruned_{fwd,dam,dlm}_kernel<2|4|8|16, constrained>; the blank moves with the width."""
    B, T, S, R = 3, 30, 10, 4
    blank = {0: 0, 1: C // 2, 2: C - 1}[C % 3]
    g = torch.Generator().manual_seed(C)
    scale = 0.8 if act == "tanh" else 2.0
    tl, el = torch.tensor([S, 6, 2]), torch.tensor([T, 22, 13])
    c = dict(am=torch.randn(B, T, C, generator=g) * scale, lm=torch.randn(B, S + 1, C, generator=g) * scale,
             sym=LC.draw_symbols(g, B, S, C, blank), tl=tl, el=el, blank=blank, w=LC.weights(B),
             ranges=LT.band_ranges(tl, el, S, T, R), S=S, T=T, R=R, C=C, B=B)
    _check(dev, c, "constrained", 0.05, "fused", act)


# ------------------------------------------------------------------ padded frames
@pytest.mark.parametrize("rnnt_type", NEW_TYPES)
def test_padded_frames_and_rows_are_not_read(dev, rnnt_type):
    """Frames past T_b and rows past S_b hold NaN in am / lm / logits: no NaN in the losses or in
    the valid part of a gradient, the padded gradient rows are exactly zero; the float64 side sees
    zeros there."""
    c = TC.direct_case("R5", seed=2)
    nan = float("nan")
    valid_t = torch.arange(c["T"]).reshape(1, -1) < c["el"].reshape(-1, 1)            # (B,T)
    valid_s = torch.arange(c["S"] + 1).reshape(1, -1) <= c["tl"].reshape(-1, 1)       # (B,S+1)
    valid_n = valid_t.unsqueeze(2) & (c["ranges"] <= c["tl"].reshape(-1, 1, 1))       # (B,T,R)
    zero = dict(c, am=c["am"] * valid_t.unsqueeze(2), lm=c["lm"] * valid_s.unsqueeze(2),
                logits=c["logits"] * valid_n.unsqueeze(3))
    am = torch.where(valid_t.unsqueeze(2), c["am"], torch.tensor(nan))
    lm = torch.where(valid_s.unsqueeze(2), c["lm"], torch.tensor(nan))
    logits = torch.where(valid_n.unsqueeze(3), c["logits"], torch.tensor(nan))
    for path in ("fused", "logits"):
        ref, ref_grads = TC.direct_reference(zero, rnnt_type, 0.05, path)
        assert torch.isfinite(ref).all()
        per, grads = _run_device(dev, c, rnnt_type, 0.05, path, am=am, lm=lm, logits=logits)
        _assert_loss(per, ref, f"{rnnt_type} {path} padded")
        masks = (valid_t, valid_s) if path == "fused" else (valid_n,)
        for g, r, m in zip(grads, ref_grads, masks):
            assert torch.isfinite(g).all()
            assert (g.cpu()[~m] == 0).all()
            assert (r[~m] == 0).all()
            _assert_grad(g, r, what=f"{path} padded")


# ------------------------------------------------------------------ an utterance without a path
@pytest.mark.parametrize("rnnt_type", NEW_TYPES)
def test_infeasible_utterance_inside_a_feasible_batch(dev, rnnt_type):
    """S_b = 6 > T_b = 4: loss +inf, gradient rows finite zeros, the others at tolerance."""
    c = TC.direct_case("R5", seed=3, tl=(7, 5, 6, 3), el=(20, 5, 4, 12))
    for path in ("fused", "logits"):
        per, _ = _check(dev, c, rnnt_type, 0.05, path, infeasible=(2,))
        assert float(per[2].detach()) == float("inf")


# ------------------------------------------------------------------ the defaults through the C ABI
def test_default_wrappers_equal_the_entry_points_at_regular_without_penalty(dev):
    """rnnt_pruned_joiner_loss / rnnt_lattice_loss under their defaults against a direct call of
    s2t_rnnt_{pruned,lattice}_{fwd,bwd} with (S2T_RNNT_REGULAR, 0.0) at the C3 bench geometry (the
    materialised lattice on its first 8 utterances): same bits in the loss, d_am, d_lm and d_logits,
    which pins the place of the type and the penalty among the arguments the binding passes through
    the header-parsed ABI.  Then what the library itself refuses before it launches anything."""
    from speech2text_amd import _native as N
    k = _kern()
    c = LC.bench_case()
    B, T, S, C, R = c["B"], c["T"], c["S"], c["C"], c["R"]
    am, lm, sym = c["am"].to(dev), c["lm"].to(dev), c["sym"].to(dev)
    bnd = k.make_boundary(c["tl"], c["el"], dev)
    _, gx, gy = k.rnnt_simple_loss(lm, am, sym, bnd, 0)
    rg = k.rnnt_prune_ranges(gx, gy, bnd, R)
    lib, st, REG = N.lib(), N.stream(), k.RNNT_TYPES["regular"]
    w = LC.weights(B).float().to(dev)
    gscale = -w

    def new(*shape):
        return torch.full(shape, 7.0, device=dev)

    def wrapped(fn, leaves, *rest):
        leaves = [x.clone().requires_grad_(True) for x in leaves]
        per = fn(*leaves, *rest)
        return (per.detach(),) + torch.autograd.grad(per, leaves, grad_outputs=w[:per.shape[0]])

    px, py, lse = new(B, S, T + 1), new(B, S + 1, T), new(B, T, R)
    N.check(lib.s2t_rnnt_pruned_fwd(N.fp(am), N.fp(lm), N.lp(rg), N.lp(sym), N.lp(bnd), B, S, T, C, R, 0, 0,
                                    REG, 0.0, N.fp(px), N.fp(py), N.fp(lse), st), "fwd")
    ans, _, dx, dy = k.mutual_information(px, py, bnd)
    d_am, d_lm = new(B, T, C), new(B, S + 1, C)
    N.check(lib.s2t_rnnt_pruned_bwd(N.fp(am), N.fp(lm), N.lp(rg), N.lp(sym), N.fp(lse), N.fp(dx), N.fp(dy),
                                    N.fp(gscale), B, S, T, C, R, 0, 0, REG, N.fp(d_am), N.fp(d_lm), 0, st), "bwd")
    for a, b in zip(wrapped(k.rnnt_pruned_joiner_loss, (am, lm), rg, sym, bnd), (-ans, d_am, d_lm)):
        assert torch.equal(a, b)

    Bs = 8
    from speech2text_amd.model.joiner.joiner import PrunedLattice
    logits = PrunedLattice(am[:Bs], lm[:Bs], rg[:Bs].contiguous(), "relu").materialize().contiguous()
    rgs, syms, bnds = rg[:Bs].contiguous(), sym[:Bs].contiguous(), bnd[:Bs].contiguous()
    px, py, lse = new(Bs, S, T + 1), new(Bs, S + 1, T), new(Bs, T, R)
    N.check(lib.s2t_rnnt_lattice_fwd(N.fp(logits), N.lp(rgs), N.lp(syms), N.lp(bnds), Bs, S, T, C, R, 0, REG, 0.0,
                                     N.fp(px), N.fp(py), N.fp(lse), st), "fwd")
    ans, _, dx, dy = k.mutual_information(px, py, bnds)
    d = new(Bs, T, R, C)
    N.check(lib.s2t_rnnt_lattice_bwd(N.fp(logits), N.lp(rgs), N.lp(syms), N.fp(lse), N.fp(dx), N.fp(dy),
                                     N.fp(gscale), Bs, S, T, C, R, 0, REG, N.fp(d), st), "bwd")
    for a, b in zip(wrapped(k.rnnt_lattice_loss, (logits,), rgs, syms, bnds), (-ans, d)):
        assert torch.equal(a, b)

    # an unknown type on all six entry points, a negative or NaN penalty on the two forwards: -1 from the
    # library itself, and every output buffer still holds what it held
    B, S, T, C, R = 1, 2, 3, 8, 2
    am, lm, logits, gscale = new(B, T, C), new(B, S + 1, C), new(B, T, R, C), new(B)
    rg = torch.zeros(B, T, R, dtype=torch.int64, device=dev)
    sym = torch.ones(B, S, dtype=torch.int64, device=dev)
    bnd = k.make_boundary(torch.tensor([S]), torch.tensor([T]), dev)
    px, py, lse, p, ans = new(B, S, T + 1), new(B, S + 1, T), new(B, T, R), new(B, S + 1, T + 1), new(B)
    dx, dy, d_am, d_lm, d = new(B, S, T + 1), new(B, S + 1, T), new(B, T, C), new(B, S + 1, C), new(B, T, R, C)
    forwards = (
        lambda ty, pen: lib.s2t_rnnt_pruned_fwd(N.fp(am), N.fp(lm), N.lp(rg), N.lp(sym), N.lp(bnd), B, S, T, C, R,
                                                0, 0, ty, pen, N.fp(px), N.fp(py), N.fp(lse), st),
        lambda ty, pen: lib.s2t_rnnt_lattice_fwd(N.fp(logits), N.lp(rg), N.lp(sym), N.lp(bnd), B, S, T, C, R, 0,
                                                 ty, pen, N.fp(px), N.fp(py), N.fp(lse), st))
    typed_only = (
        lambda ty: lib.s2t_rnnt_pruned_bwd(N.fp(am), N.fp(lm), N.lp(rg), N.lp(sym), N.fp(lse), N.fp(px), N.fp(py),
                                           N.fp(gscale), B, S, T, C, R, 0, 0, ty, N.fp(d_am), N.fp(d_lm), 0, st),
        lambda ty: lib.s2t_rnnt_lattice_bwd(N.fp(logits), N.lp(rg), N.lp(sym), N.fp(lse), N.fp(px), N.fp(py),
                                            N.fp(gscale), B, S, T, C, R, 0, ty, N.fp(d), st),
        lambda ty: lib.s2t_mutual_info_fwd(N.fp(px), N.fp(py), N.lp(bnd), B, S, T, ty, N.fp(p), N.fp(ans), st),
        lambda ty: lib.s2t_mutual_info_bwd(N.fp(px), N.fp(py), N.lp(bnd), N.fp(p), None, B, S, T, ty, N.fp(dx),
                                           N.fp(dy), st))
    for ty in (3, -1):
        for call in forwards:
            assert call(ty, 0.0) == -1
        for call in typed_only:
            assert call(ty) == -1
    for pen in (-0.5, float("nan")):
        for call in forwards:
            assert call(REG, pen) == -1
    for out in (px, py, lse, p, ans, dx, dy, d_am, d_lm, d):
        assert (out == 7.0).all()


# ------------------------------------------------------------------ the chain
@pytest.mark.parametrize("use_out_project", [False, True])
def test_joiner_to_typed_loss_chain(dev, use_out_project):
    """Joiner.forward -> Loss(Pruned_Rnnt, modified, penalty) -> backward against the float64 chain
    0.5 * simple + pruned on the ranges the device chose; am / lm drawn at scale 0.3, where those
    ranges keep a one-symbol-per-frame path (asserted)."""
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.loss.loss import Loss
    B, T, S, C, R = 4, 24, 6, 21, 5
    g = torch.Generator().manual_seed(31)
    am = torch.randn(B, T, C, generator=g) * 0.3
    lm = torch.randn(B, S + 1, C, generator=g) * 0.3
    sym = LC.draw_symbols(g, B, S, C, 0)
    tl, el = torch.tensor([S, 4, 0, 5]), torch.tensor([T, 15, 3, 9])
    torch.manual_seed(5)
    j = Joiner(JoinerConfig(input_dim=C, output_dim=C, inner_dim=16, activation="tanh", prune_range=R,
                            use_out_project=use_out_project))
    j._enc_proj = torch.nn.Identity(); j._pre_proj = torch.nn.Identity()      # am / lm themselves
    j = j.to(dev)
    loss = Loss({"model": "Pruned_Rnnt", "config": {"termination_symbol": 0, "rnnt_type": "modified",
                                                    "delay_penalty": 0.05, "reduction": "mean"}})
    am_g = am.to(dev).requires_grad_(True); lm_g = lm.to(dev).requires_grad_(True)
    logits, bnd_g, rg, simple = j(am_g, el.to(dev), lm_g, tl.to(dev), sym.to(dev))
    pruned = loss({"logits": logits, "targets": sym.to(dev), "logits_length": el.to(dev),
                   "targets_length": tl.to(dev), "boundary": bnd_g, "ranges": rg})
    (0.5 * simple + pruned).backward()

    a = am.double().requires_grad_(True); l = lm.double().requires_grad_(True)
    bnd = LT.make_boundary(tl, el)
    s_ref = L.simple_neg(a, l, sym, bnd, 0)
    lat = LT.joiner_logits(a, l, rg.cpu(), "tanh")
    if use_out_project:
        w = [p.detach().cpu().double() for p in j._out_projection.parameters()]
        lat = torch.nn.functional.linear(torch.nn.functional.linear(lat, w[0], w[1]), w[2], w[3])
    p_ref = LT.lattice_neg(lat, rg.cpu(), sym, bnd, 0, "modified", 0.05)
    assert torch.isfinite(p_ref).all() and torch.isfinite(s_ref).all()
    (0.5 * s_ref.mean() + p_ref.mean()).backward()
    np.testing.assert_allclose(_np(simple), _np(s_ref.mean()), rtol=RNNT_RTOL)
    np.testing.assert_allclose(_np(pruned), _np(p_ref.mean()), rtol=RNNT_RTOL)
    _assert_grad(am_g.grad, a.grad, what="chain d_am")
    _assert_grad(lm_g.grad, l.grad, what="chain d_lm")
