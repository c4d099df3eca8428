"""CPU tests of tests/lattice_f64.py, the float64 yardstick of tests/test_gpu_loss_lattices.py.

The restatement is pinned three ways before any kernel is compared with it: brute-force path
enumeration, oracle/k2_rnnt.py run in float64 where the oracle keeps the input's type (mutual
information, simple loss, pruned log-probs) and in its own fp32 elsewhere (full lattice), at the
shapes of tests/test_gpu_frontend_losses.py, at blank in {0, C-1} and with tanh.

The last part measures what fp32 costs the REFERENCE at the large cases (the table in
test_gpu_loss_lattices.py): the figures recorded in loss_cases.FP32_COST are asserted here, so the
GPU file's bounds (4x the figure, never tighter than the small-case bounds) cannot drift.
"""
import itertools

import numpy as np
import pytest
import torch

import lattice_f64 as L
import loss_cases as LC
from oracle import ctc as octc
from oracle import k2_rnnt as K


def _case(seed, B, T, S, C, blank=0, scale=2.0):
    g = torch.Generator().manual_seed(seed)
    am = torch.randn(B, T, C, generator=g) * scale
    lm = torch.randn(B, S + 1, C, generator=g) * scale
    sym = LC.draw_symbols(g, B, S, C, blank)
    tl = torch.randint(max(1, S // 2), S + 1, (B,), generator=g); tl[0] = S
    el = torch.randint(max(S + 1, T // 2), T + 1, (B,), generator=g); el[0] = T
    return am, lm, sym, tl, el


def _brute(px, py, S, T):
    tot = -np.inf
    for pos in itertools.combinations(range(S + T), S):
        s = t = 0
        lp = 0.0
        for i in range(S + T):
            if i in pos:
                lp += px[s, t]; s += 1
            else:
                lp += py[s, t]; t += 1
        tot = np.logaddexp(tot, lp)
    return tot


def test_recursion_vs_brute_force_and_occupation_counts():
    rng = np.random.default_rng(0)
    B, S, T = 4, 3, 4
    px = torch.from_numpy(rng.standard_normal((B, S, T + 1)))
    py = torch.from_numpy(rng.standard_normal((B, S + 1, T)))
    bnd = L.make_boundary([3, 2, 3, 0], [4, 4, 1, 3])
    px = L._fix_for_boundary(px, bnd)
    sc, gx, gy = L.mutual_information(px, py, bnd)
    for b in range(B):
        Sb, Tb = int(bnd[b, 2]), int(bnd[b, 3])
        assert abs(sc[b].item() - _brute(px[b].numpy(), py[b].numpy(), Sb, Tb)) < 1e-12
        # every path takes exactly S_b symbol arcs and T_b blank arcs
        assert abs(gx[b].sum().item() - Sb) < 1e-12 and abs(gy[b].sum().item() - Tb) < 1e-12
        assert (gx[b, Sb:] == 0).all() and (gx[b, :, Tb:] == 0).all()
        assert (gy[b, Sb + 1:] == 0).all() and (gy[b, :, Tb:] == 0).all()


@pytest.mark.parametrize("B,T,S,C", [(3, 12, 5, 9), (4, 70, 30, 33), (2, 130, 90, 17)])
def test_mutual_information_vs_oracle_f64(B, T, S, C):
    am, lm, sym, tl, el = _case(3, B, T, S, C)
    bnd = L.make_boundary(tl, el)
    px, py = K.get_rnnt_logprobs_smoothed(lm.double(), am.double(), sym, 0, bnd)
    _, ans, gx, gy = K.mutual_information_np(px.numpy(), py.numpy(), bnd.numpy())
    sc, gx2, gy2 = L.mutual_information(px, py, bnd)
    np.testing.assert_allclose(sc.numpy(), ans, rtol=1e-12)
    np.testing.assert_allclose(gx2.numpy(), gx, atol=1e-11)
    np.testing.assert_allclose(gy2.numpy(), gy, atol=1e-11)


@pytest.mark.parametrize("blank", ["first", "last"])
@pytest.mark.parametrize("B,T,S,C,R", [(3, 12, 5, 9, 3), (4, 70, 30, 33, 5), (2, 40, 12, 500, 5)])
def test_simple_and_pruned_vs_oracle_f64(B, T, S, C, R, blank):
    blank = 0 if blank == "first" else C - 1
    am, lm, sym, tl, el = _case(4, B, T, S, C, blank)
    bnd = L.make_boundary(tl, el)
    w = torch.linspace(-1.0, 2.0, B, dtype=torch.float64)
    # the oracle in float64 (it keeps the input's type on these two paths)
    a1 = am.double().requires_grad_(True); l1 = lm.double().requires_grad_(True)
    s_ref, (gx, gy) = K.rnnt_loss_smoothed(l1, a1, sym, blank, bnd, reduction="none")
    ranges = K.get_rnnt_prune_ranges(gx, gy, bnd, R)
    for act in ["relu", "tanh"]:
        a1.grad = l1.grad = None
        am_p, lm_p = K.do_rnnt_pruning(a1, l1, ranges)
        logits = (torch.relu if act == "relu" else torch.tanh)(am_p + lm_p)
        p_ref = K.rnnt_loss_pruned(logits, sym, ranges, blank, bnd, reduction="none")
        ((w * s_ref).sum() + (w * p_ref).sum()).backward(retain_graph=True)
        a2 = am.double().requires_grad_(True); l2 = lm.double().requires_grad_(True)
        s_new = L.simple_neg(a2, l2, sym, bnd, blank)
        p_new = L.pruned_neg(a2, l2, ranges, sym, bnd, blank, act)
        ((w * s_new).sum() + (w * p_new).sum()).backward()
        np.testing.assert_allclose(s_new.detach().numpy(), s_ref.detach().numpy(), rtol=1e-12)
        np.testing.assert_allclose(p_new.detach().numpy(), p_ref.detach().numpy(), rtol=1e-12)
        np.testing.assert_allclose(a2.grad.numpy(), a1.grad.numpy(), atol=1e-10)
        np.testing.assert_allclose(l2.grad.numpy(), l1.grad.numpy(), atol=1e-10)
        # the materialised-lattice entry of the restatement is the same function of the logits
        lg = logits.detach().clone().requires_grad_(True)
        m_new = L.lattice_neg(lg, ranges, sym, bnd, blank)
        np.testing.assert_allclose(m_new.detach().numpy(), p_ref.detach().numpy(), rtol=1e-12)


@pytest.mark.parametrize("blank", [0, 30])
def test_full_lattice_vs_oracle_fp32(blank):
    """oracle.rnnt_loss_full is fp32 throughout: held at the GPU file's small-case bounds."""
    torch.manual_seed(5)
    B, T, U, V = 3, 25, 9, 31
    logits = torch.randn(B, T, U + 1, V) * 2
    g = torch.Generator().manual_seed(1)
    tg = LC.draw_symbols(g, B, U, V, blank)
    tl = torch.tensor([U, 4, 1]); el = torch.tensor([T, 20, 11])
    lc = logits.clone().requires_grad_(True)
    ref = K.rnnt_loss_full(lc, tg, el, tl, blank=blank, reduction="none")
    ref.sum().backward()
    l2 = logits.double().requires_grad_(True)
    new = L.lattice_neg(l2, None, tg, L.make_boundary(tl, el), blank)
    new.sum().backward()
    np.testing.assert_allclose(ref.detach().numpy(), new.detach().numpy(), rtol=1e-5)
    np.testing.assert_allclose(lc.grad.numpy(), l2.grad.numpy(), atol=2e-5, rtol=2e-3)


def test_simple_equals_full_on_additive_logits_and_pruned_equals_full_when_range_covers():
    am, lm, sym, tl, el = _case(7, 3, 14, 6, 11, blank=4)
    am, lm = am.double(), lm.double()
    bnd = L.make_boundary(tl, el)
    full = L.lattice_neg(am.unsqueeze(2) + lm.unsqueeze(1), None, sym, bnd, 4)
    np.testing.assert_allclose(L.simple_neg(am, lm, sym, bnd, 4).numpy(), full.numpy(), rtol=1e-12)
    ranges = torch.arange(7).reshape(1, 1, 7).expand(3, 14, 7)
    full_t = L.lattice_neg(torch.tanh(am.unsqueeze(2) + lm.unsqueeze(1)), None, sym, bnd, 4)
    np.testing.assert_allclose(L.pruned_neg(am, lm, ranges, sym, bnd, 4, "tanh").numpy(),
                               full_t.numpy(), rtol=1e-12)


# ------------------------------------------------------------------ what fp32 costs the reference
@pytest.mark.parametrize("name", sorted(LC.CTC_LARGE))
def test_fp32_cost_of_the_ctc_reference(name):
    """torch.nn.functional.ctc_loss on an fp32 log_softmax (the reference's own call) against
    oracle.ctc in float64, reduction='sum' on the same inputs."""
    logits, tg, il, tl, blank = LC.ctc_case(name)
    _, rg, per = octc.ctc_loss(logits, tg, il, tl, blank=blank, reduction="sum")
    x = torch.from_numpy(logits).requires_grad_(True)
    lp = torch.log_softmax(x, dim=-1).transpose(0, 1)
    each = torch.nn.functional.ctc_loss(lp, torch.from_numpy(tg), torch.from_numpy(il),
                                        torch.from_numpy(tl), blank=blank, reduction="none",
                                        zero_infinity=True)
    each.sum().backward()
    loss_rel = float(np.max(np.abs(each.detach().numpy() - per) / np.abs(per)))
    grad_abs = float(np.abs(x.grad.numpy() - rg).max())
    print(f"fp32 cost {name}: loss_rel={loss_rel:.3e} grad_abs={grad_abs:.3e}")
    rec = LC.FP32_COST[name]
    assert loss_rel <= rec["loss_rel"] and grad_abs <= rec["grad_abs"]


def test_fp32_cost_of_the_rnnt_reference_at_bench_geometry():
    """oracle.k2_rnnt in fp32 (simple -> ranges -> pruned, 0.5/0.5, mean over the batch) against
    lattice_f64 on the same inputs and the same ranges."""
    c = LC.bench_case()
    am = c["am"].clone().requires_grad_(True); lm = c["lm"].clone().requires_grad_(True)
    bnd = L.make_boundary(c["tl"], c["el"])
    s32, (gx, gy) = K.rnnt_loss_smoothed(lm, am, c["sym"], 0, bnd, reduction="none")
    ranges = K.get_rnnt_prune_ranges(gx, gy, bnd, c["R"])
    am_p, lm_p = K.do_rnnt_pruning(am, lm, ranges)
    p32 = K.rnnt_loss_pruned(torch.relu(am_p + lm_p), c["sym"], ranges, 0, bnd, reduction="none")
    (0.5 * s32.mean() + 0.5 * p32.mean()).backward()
    ref = LC.bench_reference(c, ranges)
    fig = {
        "simple_rel": float((s32.detach().double() - ref["simple"]).abs().div(ref["simple"].abs()).max()),
        "pruned_rel": float((p32.detach().double() - ref["pruned"]).abs().div(ref["pruned"].abs()).max()),
        "d_am_abs": float((am.grad.double() - ref["d_am"]).abs().max()),
        "d_lm_abs": float((lm.grad.double() - ref["d_lm"]).abs().max()),
    }
    print("fp32 cost bench geometry: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    rec = LC.FP32_COST["rnnt_bench"]
    for k, v in fig.items():
        assert v <= rec[k], (k, v, rec[k])


@pytest.mark.parametrize("rows", LC.ROW_EDGES)
def test_fp32_cost_of_the_rnnt_reference_at_the_row_edges(rows):
    """oracle.k2_rnnt in fp32 (raw recursion and weighted simple loss) against lattice_f64."""
    c = LC.rows_case(rows)
    ref = LC.rows_reference(c)
    _, ans, gx, gy = K.mutual_information_any(c["px"].numpy(), c["py"].numpy(), c["mi_bnd"].numpy())
    am = c["am"].clone().requires_grad_(True); lm = c["lm"].clone().requires_grad_(True)
    s32 = K.rnnt_loss_smoothed(lm, am, c["sym"], c["blank"], L.make_boundary(c["tl"], c["el"]),
                               reduction="none", return_grad=False)
    (c["w"].float() * s32).sum().backward()
    fig = {
        "mi_rel": float(np.max(np.abs(ans - ref["sc"].numpy()) / np.abs(ref["sc"].numpy()))),
        "mi_gx_abs": float(np.abs(gx - ref["gx"].numpy()).max()),
        "mi_gy_abs": float(np.abs(gy - ref["gy"].numpy()).max()),
        "simple_rel": float((s32.detach().double() - ref["simple"]).abs().div(ref["simple"].abs()).max()),
        "d_am_abs": float((am.grad.double() - ref["d_am"]).abs().max()),
        "d_lm_abs": float((lm.grad.double() - ref["d_lm"]).abs().max()),
    }
    print(f"fp32 cost rows {rows}: " + " ".join(f"{k}={v:.3e}" for k, v in fig.items()))
    rec = LC.FP32_COST[f"rows{rows}"]
    for k, v in fig.items():
        assert v <= rec[k], (k, v, rec[k])
