"""CPU: the float64 restatement of the optimizers (tests/optim_f64.py) against the reference's own
outputs and torch.optim, what fp32 costs it on the cases of tests/optim_cases.py, the margins of
every discrete decision those cases take, and the project's host forms (ScaledAdam._step_torch, the
host path of FlatAdam / FlatAdamW) against it at the bounds the device is held to in
tests/test_gpu_optim_kernels.py."""
import os

import numpy as np
import pytest
import torch

import optim_cases as OC
import optim_f64 as OF
from speech2text_amd.optimizer.scaled_adam import ScaledAdam

EPS32 = 2.0 ** -24


# ------------------------------------------------------------------ the reference's own outputs
def _eden(it):
    """Eden (lr_batches 10, warmup_batches 4, warmup_start 0.5) on base lr 0.045 at batch `it`."""
    warm = 1.0 if it >= 4 else 0.5 + 0.5 * it / 4
    return 0.045 * ((it * it + 100.0) / 100.0) ** -0.5 * warm


def _golden_run(g, lo, hi, ref):
    for it in range(lo, hi):
        ref.groups[0]["h"]["lr"] = _eden(it)
        ref.step([torch.from_numpy(g[f"grad{it}_{i}"]) for i in range(5)])


def _golden_ref(g):
    return OF.ScaledAdamRef([torch.from_numpy(g[f"init{i}"].copy()) for i in range(5)],
                            [dict(idx=range(5), lr=0.045, clipping_scale=2.0, clipping_update_period=6)])


def test_restatement_follows_reference_trajectory(golden_dir):
    """The reference's 30-step golden (computed in fp32) at the bounds of tests/test_optimizer.py."""
    g = np.load(os.path.join(golden_dir, "scaledadam_ref.npz"))
    np.testing.assert_allclose([_eden(it) for it in range(1, 31)], g["lrs"], rtol=1e-12)
    ref = _golden_ref(g)
    lo = 0
    for it in (0, 9, 29):
        _golden_run(g, lo, it + 1, ref)
        lo = it + 1
        for i in range(5):
            np.testing.assert_allclose(ref.p[i].numpy(), g[f"p{it}_{i}"], atol=2e-6, rtol=1e-5)


def test_restatement_follows_reference_state(golden_dir):
    """Every entry of the reference's state after 15 steps (per batch of same-shaped tensors, kept
    under the batch's first parameter; optimizer/scaled_adam.py:30-109)."""
    g = np.load(os.path.join(golden_dir, "scaledadam_ref.npz"))
    r = np.load(os.path.join(golden_dir, "scaledadam_state_ref.npz"))
    ref = _golden_ref(g)
    _golden_run(g, 0, 15, ref)
    G = ref.groups[0]
    for i in range(5):
        np.testing.assert_allclose(ref.p[i].numpy(), r[f"p14_{i}"], atol=3e-6, rtol=2e-5)
    seen = 0
    for key in r["keys"].tolist():
        idx, k = key.split(":")
        want = r[f"state{idx}_{k}"]
        batch = [i for i in range(5) if ref.p[i].shape == ref.p[int(idx)].shape]
        ones = (1,) * ref.p[int(idx)].dim()
        if k == "step":
            got = np.asarray(G["step"])
        elif k in ("delta", "exp_avg_sq"):
            got = torch.stack([getattr(ref, k)[i] for i in batch]).numpy()
        elif k in ("param_rms", "scale_exp_avg_sq"):
            got = G[k][batch].reshape((len(batch),) + ones).numpy()
        elif k == "scale_grads":
            got = G[k][:, batch].reshape((4, len(batch)) + ones).numpy()
        elif k == "model_norms":
            got = G[k].numpy()
        elif k == "model_norm_threshold":
            got = np.asarray(float(G["threshold"]))
        else:
            assert k == "num_clipped", key
            got = np.asarray(G[k])
        assert got.shape == want.shape, key
        np.testing.assert_allclose(got, want, atol=3e-6, rtol=2e-5, err_msg=key)
        seen += 1
    assert seen == 24


@pytest.mark.parametrize("case", [c for c, v in OC.ADAM_CASES.items() if v["fused"]])
def test_adam_restatement_equals_torch_optim(case):
    """AdamRef in float64 against torch.optim.Adam / AdamW + clip_grad_norm_ in float64 on the same
    gradients (no dropped step: torch has none), to 1e-12 relative."""
    c = OC.ADAM_CASES[case]
    groups = OC.s2_groups(case)
    ref = OF.AdamRef(OC.s2_init(), groups, c["name"] == "AdamW", pre_clip=c["pre_clip"])
    ps = [torch.nn.Parameter(t.double()) for t in OC.s2_init()]
    topt = getattr(torch.optim, c["name"])(
        [dict(params=[ps[i] for i in g["idx"]], lr=g["lr"], betas=g["betas"], eps=g["eps"],
              weight_decay=g["weight_decay"]) for g in groups])
    for it in range(c["steps"]):
        grads = OC.s2_grads(case, it)
        ref.step(grads)
        for p, gr in zip(ps, grads):
            p.grad = gr.double()
        if c["pre_clip"]:
            torch.nn.utils.clip_grad_norm_(ps, c["pre_clip"])
        topt.step()
    for i, p in enumerate(ps):
        assert OC.rel_err(ref.p[i], p) <= 1e-12, i
        if i < OC.S2_GROUPED:
            assert OC.rel_err(ref.exp_avg[i], topt.state[p]["exp_avg"]) <= 1e-12, i
            assert OC.rel_err(ref.exp_avg_sq[i], topt.state[p]["exp_avg_sq"]) <= 1e-12, i
            assert float(topt.state[p]["step"]) == ref.step_count
        else:
            assert torch.equal(ref.p[i], OC.s2_init()[i].double())        # in no group: never updated


# ------------------------------------------------------------------ what fp32 costs the restatement
def _hold_figures(case, measured):
    """Recorded and re-measured figure within a factor 4 of each other (the convention of
    tests/lstm_cases.py).  A figure is a maximum over a tensor and moves with the order in which the
    host sums; under one fp32 ulp it is rounding luck, so both sides are floored there."""
    rec = OC.FP32_COST[case]
    assert set(rec) == set(measured), case
    print(case, " ".join(f"{q}={v:.3e}" for q, v in measured.items()))
    for q, m in measured.items():
        assert (m == 0.0) == (rec[q] == 0.0), (case, q, m, rec[q])
        assert m <= 4.0 * max(rec[q], EPS32) and rec[q] <= 4.0 * max(m, EPS32), (case, q, m, rec[q])


@pytest.mark.parametrize("run", list(OC.RUNS))
def test_scaled_adam_fp32_figures(run):
    _hold_figures(run, OC.sa_fp32_figures(run))


@pytest.mark.parametrize("case", list(OC.ADAM_CASES))
def test_adam_fp32_figures(case):
    _hold_figures(case, OC.adam_fp32_figures(case))


@pytest.mark.parametrize("name", [c for c in OC.COEF_CASES if c != "most_nan"])
def test_coef_fp32_figures(name):
    _hold_figures("coef_" + name, OC.coef_fp32_figures(name))


def test_direct_sum_fp32_figures():
    r64, mag = OC.seg_stats_ref(torch.float64)
    r32, _ = OC.seg_stats_ref(torch.float32)
    m = float(((r32.double() - r64).abs() / mag).max())
    rec = OC.FP32_COST["seg_stats"]
    assert m <= 4.0 * max(rec, EPS32) and rec <= 4.0 * max(m, EPS32), m
    m = max(OC.rel_each(OC.clip_coef_ref(n, torch.float32), OC.clip_coef_ref(n, torch.float64))
            for n in OC.CLIP_NCHUNKS)
    rec = OC.FP32_COST["clip_coef"]
    assert m <= 4.0 * max(rec, EPS32) and rec <= 4.0 * max(m, EPS32), m


# ------------------------------------------------------------------ no case sits on a branch point
def _hold_margins(case, margins):
    """Every decision the float64 run takes is at least 100 x the fp32 figure of the quantity it
    compares away from flipping; a tied median is the same value whichever tied entry is picked
    (optim_f64.median_of measures the gap to the nearest OTHER value)."""
    assert margins, case
    kinds = set()
    for m in margins:
        fig = EPS32 if m["q"] == "eps32" else OC.FP32_COST[case][m["q"]]
        assert m["margin"] >= 100.0 * fig, (case, m, fig)
        kinds.add(m["kind"])
    return kinds


# which decisions a run has to take both ways (`taken` counted over the run) for its branches to be
# exercised at all
def _taken(margins, kind):
    return sum(int(m.get("taken", 0)) for m in margins if m["kind"] == kind)


@pytest.mark.parametrize("run", list(OC.RUNS))
def test_scaled_adam_decisions_have_margin(run):
    _, margins = OC.sa_reference(run)
    kinds = _hold_margins(run, margins)
    assert {"bc2<0.99", "scalar clamp"} <= kinds
    r = OC.RUNS[run]
    if r["steps"] > r["P"]:
        assert _taken(margins, "rms<min") and _taken(margins, "max_rms cap")
        caps = [m["taken"] for m in margins if m["kind"] == "max_rms cap"]
        assert max(caps) == 2            # both the tensor under and the one over param_max_rms
    if r["steps"] >= 12:
        assert _taken(margins, "scalar clamp") >= 2
    if r["cs"] is not None and r["steps"] > r["period"]:
        assert "median" in kinds and "ans<1" in kinds
    if r["spike"] is not None:
        assert _taken(margins, "ans<1")
    if run == "beta2_0.9":
        took = [m["taken"] for m in margins if m["kind"] == "bc2<0.99"]
        assert True in took and False in took
    if run == "p25_s4":                  # the dropped steps repeat norms: the windows hold exact ties
        assert any(m["kind"] == "median" for m in margins)


@pytest.mark.parametrize("name", list(OC.COEF_CASES))
def test_coef_decisions_have_margin(name):
    ref, margins = OC.coef_ref(name, torch.float64)
    if name == "most_nan":
        assert isinstance(ref, RuntimeError) and "not finite" in str(ref)
        return
    _hold_margins("coef_" + name, margins)
    if name in ("all_equal", "tie_pairs"):
        med = [m for m in margins if m["kind"] == "median"]
        assert len(med) == 1 and med[0]["tied"]
        t = OC.coef_case(name)
        want = 17.25 if name == "all_equal" else 4.0
        assert float(ref["threshold"]) == t["cs"] * want
    if name == "one_nan":
        assert bool(torch.isfinite(ref["threshold"]).all()) and bool(torch.isnan(ref["model_norms"]).any())


# ------------------------------------------------------------------ the host forms
@pytest.mark.parametrize("run", list(OC.RUNS))
def test_host_scaled_adam_follows_restatement(run):
    """ScaledAdam on CPU tensors (_step_torch and the host form of the dropped step) on the runs and
    at the bounds of the device.  Covers question 1 (`none_nan`, `nan_step0`: a NaN norm under the
    trainer's clip leaves the factor at 1) and the dropped step's state."""
    r = OC.RUNS[run]
    ref, _ = OC.sa_reference(run)
    ps, st, opt = OC.sa_build(run, "cpu")
    worst = 0.0
    for it in range(r["steps"]):
        OC.take_step(ps, opt, OC.s1_grads(run, it), it in r["skips"])
        assert float(st.flat_g.abs().sum()) == 0.0, it
        if it in r["ckpt"]:
            worst = max(worst, OC.sa_hold(run, OC.sa_project_snapshot(st, opt), ref[it], f"step {it}"))
    print(f"{run}: worst error / bound {worst:.3f}")
    if r["nan"] is not None and r["nan"] < 3:
        p = ref[r["ckpt"][-1]]["p"]
        assert int(torch.isnan(p).sum()) == 1          # the NaN stayed in its own element


@pytest.mark.parametrize("case", list(OC.ADAM_CASES))
def test_host_adam_follows_restatement(case):
    """The host path of FlatAdam / FlatAdamW (CPU tensors) at the device's bounds.  Covers question 2:
    a dropped step advances the count on this path too."""
    c = OC.ADAM_CASES[case]
    ref = OC.adam_reference(case)
    ps, st, opt = OC.adam_build(case, "cpu")
    worst = 0.0
    for it in range(c["steps"]):
        OC.take_step(ps, opt, OC.s2_grads(case, it), it in c["skips"])
        assert opt._flat is False
        assert float(st.flat_g.abs().sum()) == 0.0, it
        if it in c["ckpt"]:
            worst = max(worst, OC.adam_hold(case, OC.adam_project_snapshot(st, opt, ps), ref[it],
                                            f"step {it}"))
    print(f"{case}: worst error / bound {worst:.3f}")


def test_host_adam_keeps_a_nan_norm_out_of_the_finite_elements():
    """Question 1 on the Adam path: one NaN gradient element with the trainer's clip on."""
    case = "adamw_g2"
    ps, st, opt = OC.adam_build(case, "cpu")
    ref = OF.AdamRef(OC.s2_init(), OC.s2_groups(case), True, pre_clip=5.0)
    grads = OC.s2_grads(case, 0)
    grads[1][7] = float("nan")
    ref.step(grads)
    OC.take_step(ps, opt, grads, False)
    got, want = OC.adam_project_snapshot(st, opt, ps), OC.adam_snapshot(ref)
    assert int(torch.isnan(want["p"]).sum()) == 1
    OC.adam_hold(case, got, want)


@pytest.mark.parametrize("period", [0, -3, 1025, 4096, 6.0])
def test_clipping_update_period_outside_the_kernel_limit_is_refused(period):
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match="1..1024"):
        ScaledAdam([p], clipping_scale=2.0, clipping_update_period=period)
    with pytest.raises(ValueError, match="1..1024"):
        ScaledAdam([{"params": [p], "clipping_update_period": period}])


def test_clipping_update_period_limits_are_accepted():
    for period in (1, 1024):
        ScaledAdam([torch.nn.Parameter(torch.zeros(3))], clipping_update_period=period)


def test_non_finite_median_raises_in_both_forms():
    """More than half of the window NaN: the restatement and the host form raise the reference's
    error on the same step (period 4: NaN gradients on steps 2, 3, 4, threshold step 4)."""
    from speech2text_amd.flat import FlatStore
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(6, 5, generator=g), torch.randn(9, generator=g), torch.randn(1, generator=g)]
    ref = OF.ScaledAdamRef(init, [dict(idx=range(3), clipping_scale=2.0, clipping_update_period=4)])
    ps = [torch.nn.Parameter(t.clone()) for t in init]
    FlatStore(ps)
    opt = ScaledAdam(ps, clipping_scale=2.0, clipping_update_period=4)
    for it in range(5):
        grads = [torch.randn(t.shape, generator=g) for t in init]
        if it >= 2:
            grads[1][it] = float("nan")
        for p, gr in zip(ps, grads):
            p.grad.copy_(gr)
        if it < 4:
            ref.step(grads)
            opt.step()
            continue
        with pytest.raises(RuntimeError, match="Too many grads were not finite"):
            ref.step(grads)
        with pytest.raises(RuntimeError, match="Too many grads were not finite"):
            opt.step()
    assert ref.groups[0]["step"] == opt._gstate[0]["step"] == 4
