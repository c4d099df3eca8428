"""GPU: every kernel of csrc/optim.hip against the independent float64 restatement of
tests/optim_f64.py, on the cases of tests/optim_cases.py: through ScaledAdam / FlatAdam / FlatAdamW
on a FlatStore (parameters AND every state buffer at every checkpoint, integer state exactly, pad
lanes and cleared gradients exactly 0) and through the C ABI for the crafted cases.  Bounds: 4 x
what fp32 costs the restatement on the same inputs (measured by tests/test_optim_f64.py), never
tighter than atol 2e-6 + rtol 3e-5."""
import pytest
import torch

import optim_cases as OC
import optim_f64 as OF

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _pads_are_zero(st, *bufs):
    for b in bufs:
        assert int(_bits(OC.pad_lanes(st, b)).abs().sum()) == 0


# ------------------------------------------------------------------ through the optimizers
def _run_scaled_adam(run, dev):
    r = OC.RUNS[run]
    ref, _ = OC.sa_reference(run)
    ps, st, opt = OC.sa_build(run, dev)
    worst = 0.0
    for it in range(r["steps"]):
        OC.take_step(ps, opt, OC.s1_grads(run, it), it in r["skips"])
        assert int(_bits(st.flat_g).abs().sum()) == 0, f"step {it}: gradients not cleared"
        if it in r["ckpt"]:
            worst = max(worst, OC.sa_hold(run, OC.sa_project_snapshot(st, opt), ref[it], f"step {it}"))
            _pads_are_zero(st, st.flat_p, opt._delta, opt._eas)
    return worst, st, opt


@pytest.mark.parametrize("run", list(OC.RUNS))
def test_scaled_adam_kernels_follow_float64(dev, run):
    worst, st, opt = _run_scaled_adam(run, dev)
    print(f"{run}: worst error / bound {worst:.3f}")
    # the tensor no group lists never moved
    i = OC._NAME["free"]
    assert torch.equal(st.params[i].detach().cpu(), OC.s1_init()[i])
    r = OC.RUNS[run]
    if r["nan"] is not None and r["nan"] < 3:
        # question 1: a NaN norm under the trainer's clip, no threshold yet: one element is lost
        assert int(torch.isnan(st.flat_p).sum()) == 1


def _run_adam(case, dev):
    c = OC.ADAM_CASES[case]
    ref = OC.adam_reference(case)
    ps, st, opt = OC.adam_build(case, dev)
    worst = 0.0
    for it in range(c["steps"]):
        OC.take_step(ps, opt, OC.s2_grads(case, it), it in c["skips"])
        if c["fused"]:
            assert opt._flat not in (None, False), "the fused path did not run"
        else:
            assert opt._flat is False, "more groups than the kernel takes: the host path runs"
        assert int(_bits(st.flat_g).abs().sum()) == 0, f"step {it}: gradients not cleared"
        if it in c["ckpt"]:
            worst = max(worst, OC.adam_hold(case, OC.adam_project_snapshot(st, opt, ps), ref[it],
                                            f"step {it}"))
            if c["fused"]:
                _pads_are_zero(st, st.flat_p, opt._flat["m"], opt._flat["v"])
    return worst, st, opt


@pytest.mark.parametrize("case", list(OC.ADAM_CASES))
def test_adam_kernels_follow_float64(dev, case):
    from speech2text_amd import _native as N
    assert N.const("S2T_ADAM_MAX_GROUPS") == OC.ADAM_MAX_GROUPS and N.lib().s2t_optim_chunk_elems() == 8192
    worst, st, opt = _run_adam(case, dev)
    print(f"{case}: worst error / bound {worst:.3f}")
    assert torch.equal(st.params[-1].detach().cpu(), OC.s2_init()[-1])      # in no group: never moved


def test_adam_keeps_a_nan_norm_out_of_the_finite_elements(dev):
    """Question 1 on the Adam path: one NaN gradient element with the trainer's clip on: the factor
    is 1, every other element takes its step."""
    case = "adamw_g2"
    ps, st, opt = OC.adam_build(case, dev)
    ref = OF.AdamRef(OC.s2_init(), OC.s2_groups(case), True, pre_clip=5.0)
    grads = OC.s2_grads(case, 0)
    grads[1][7] = float("nan")
    ref.step(grads)
    OC.take_step(ps, opt, grads, False)
    want = OC.adam_snapshot(ref)
    assert int(torch.isnan(want["p"]).sum()) == 1
    OC.adam_hold(case, OC.adam_project_snapshot(st, opt, ps), want)


# ------------------------------------------------------------------ determinism
def test_scaled_adam_is_bit_reproducible(dev):
    """The kernels sum in a fixed order (data-parallel replicas rely on it): the same run built
    twice in one process ends in identical bits, parameters and all state."""
    run = "p6_s4"
    _, st1, o1 = _run_scaled_adam(run, dev)
    _, st2, o2 = _run_scaled_adam(run, dev)
    assert _same_bits(st1.flat_p, st2.flat_p)
    assert _same_bits(o1._delta, o2._delta) and _same_bits(o1._eas, o2._eas)
    assert _same_bits(o1._segc, o2._segc)
    for a, b in zip(o1._gstate, o2._gstate):
        for k in ("param_rms", "scale_exp_avg_sq", "scale_grads", "model_norms", "fstate"):
            assert _same_bits(a[k], b[k]), k
        assert torch.equal(a["istate"], b["istate"]) and a["step"] == b["step"]


@pytest.mark.parametrize("case", ["adamw_g8", "adam_g2"])
def test_adam_is_bit_reproducible(dev, case):
    _, st1, o1 = _run_adam(case, dev)
    _, st2, o2 = _run_adam(case, dev)
    assert _same_bits(st1.flat_p, st2.flat_p)
    assert _same_bits(o1._flat["m"], o2._flat["m"]) and _same_bits(o1._flat["v"], o2._flat["v"])
    assert _same_bits(o1._flat["coef"], o2._flat["coef"])


# ------------------------------------------------------------------ the dropped step
def test_dropped_step_of_scaled_adam_moves_only_what_it_says(dev):
    """Flag as a device tensor, after 9 live steps (k = 9): bitwise nothing moves but the count, the
    (p . g) sample of the step (0) and the window slot (the previous norm); gradients cleared."""
    run = "p6_s4"
    ps, st, opt = OC.sa_build(run, dev)
    for it in range(9):
        OC.take_step(ps, opt, OC.s1_grads(run, it), False)
    keep = dict(p=st.flat_p.clone(), delta=opt._delta.clone(), eas=opt._eas.clone())
    gkeep = [{k: g[k].clone() for k in ("param_rms", "scale_exp_avg_sq", "scale_grads", "model_norms",
                                         "fstate", "istate")} for g in opt._gstate]
    assert opt.skip_flag.is_cuda
    OC.take_step(ps, opt, OC.s1_grads(run, 9), True)
    assert int(_bits(st.flat_g).abs().sum()) == 0
    assert _same_bits(st.flat_p, keep["p"]) and _same_bits(opt._delta, keep["delta"])
    assert _same_bits(opt._eas, keep["eas"])
    for g, k in zip(opt._gstate, gkeep):
        assert g["step"] == 10
        for q in ("param_rms", "scale_exp_avg_sq", "fstate"):
            assert _same_bits(g[q], k[q]), q
        assert torch.equal(g["istate"], k["istate"])
        want = k["scale_grads"].clone()
        want[9 % 4] = 0.0
        assert _same_bits(g["scale_grads"], want)
        want = k["model_norms"].clone()
        want[9 % 6] = want[8 % 6]
        assert _same_bits(g["model_norms"], want)


@pytest.mark.parametrize("case", ["adamw_g2", "adam_g8", "adamw_g9_host"])
def test_dropped_step_of_adam_moves_only_the_count(dev, case):
    """Question 2: on the fused and on the host path the count advances and nothing else moves."""
    ps, st, opt = OC.adam_build(case, dev)
    for it in range(3):
        OC.take_step(ps, opt, OC.s2_grads(case, it), False)
    before = OC.adam_project_snapshot(st, opt, ps)
    assert opt.skip_flag.is_cuda
    OC.take_step(ps, opt, OC.s2_grads(case, 3), True)
    after = OC.adam_project_snapshot(st, opt, ps)
    assert int(_bits(st.flat_g).abs().sum()) == 0
    assert after["step"] == before["step"] + 1 == 4
    for q in OC.ADAM_QUANTITIES:
        assert _same_bits(after[q], before[q]), q


# ------------------------------------------------------------------ the non-finite median
def test_non_finite_median_raises_and_leaves_the_large_state(dev):
    """Question 3.  Four of group 0's six window entries are made NaN before threshold step k = 6.
    The RuntimeError comes before the update: parameters, delta, exp_avg_sq, the gradients and every
    group's count are as before the call.  The coefficient kernels have run: both groups' window
    slot and (p . g) sample of the step are written, group 1 (finite window) has its new threshold,
    group 0 a NaN one and istate[2] set, which stays: the same call raises again."""
    run = "p6_s4"
    ps, st, opt = OC.sa_build(run, dev)
    for it in range(6):
        OC.take_step(ps, opt, OC.s1_grads(run, it), False)
    g0, g1 = opt._gstate
    g0["model_norms"][1:5] = float("nan")
    keep = dict(p=st.flat_p.clone(), delta=opt._delta.clone(), eas=opt._eas.clone())
    gkeep = [{k: g[k].clone() for k in ("param_rms", "scale_exp_avg_sq", "scale_grads", "model_norms",
                                         "fstate", "istate")} for g in opt._gstate]
    grads = OC.s1_grads(run, 6)
    for p, g in zip(ps, grads):
        p.grad.copy_(g)
    gbits = st.flat_g.clone()
    opt.skip_flag.zero_()
    for attempt in range(2):
        with pytest.raises(RuntimeError, match="Too many grads were not finite"):
            opt.step()
        assert _same_bits(st.flat_p, keep["p"]) and _same_bits(opt._delta, keep["delta"])
        assert _same_bits(opt._eas, keep["eas"]) and _same_bits(st.flat_g, gbits)
        assert g0["step"] == g1["step"] == 6
        for g, k in zip(opt._gstate, gkeep):
            assert _same_bits(g["param_rms"], k["param_rms"])                 # 6 % 4 != 3
            assert _same_bits(g["scale_exp_avg_sq"], k["scale_exp_avg_sq"])
            assert not _same_bits(g["scale_grads"][6 % 4], k["scale_grads"][6 % 4])
            assert _same_bits(g["scale_grads"][[0, 1, 3]], k["scale_grads"][[0, 1, 3]])
            assert _same_bits(g["model_norms"][1:], k["model_norms"][1:])
            assert bool(torch.isfinite(g["model_norms"][0])) and float(g["model_norms"][0]) > 0.0
        # (a NaN threshold gives the factor 0, which counts as a clipped step)
        assert g0["istate"].tolist() == [1, 1, 1] and bool(torch.isnan(g0["fstate"][0]))
        assert g1["istate"].tolist() == [1, 0, 0] and bool(torch.isfinite(g1["fstate"][0]))


# ------------------------------------------------------------------ through the C ABI
def _i32(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _floor_bound(fig, ref, mag):
    return torch.maximum(OC.MARGIN * fig * mag, OC.FLOOR_ATOL + OC.FLOOR_RTOL * ref.abs())


def test_seg_stats_chunk_lengths(dev):
    """One workgroup per chunk of 4, 8188 and 8192 elements against float64 sums."""
    from speech2text_amd import _native as N
    p, g, off, ln = OC.seg_stats_case()
    p, g = p.to(dev), g.to(dev)
    partial = torch.full((3, 3), -1.0, device=dev)
    off, ln = _i32(off, dev), _i32(ln, dev)
    N.check(N.lib().s2t_seg_stats(N.fp(p), N.fp(g), N.ip(off), N.ip(ln), 3, N.fp(partial), N.stream()),
            "s2t_seg_stats")
    ref, mag = OC.seg_stats_ref(torch.float64)
    err = (partial.double().cpu() - ref).abs()
    r = float((err / _floor_bound(OC.FP32_COST["seg_stats"], ref, mag)).max())
    print(f"seg_stats: worst error / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("n", OC.CLIP_NCHUNKS)
def test_clip_coef_chunk_counts(dev, n):
    from speech2text_amd import _native as N
    part, clip = OC.clip_coef_case(n)
    d = part.to(dev).contiguous()
    out = torch.zeros(2, device=dev)
    L = N.lib()
    N.check(L.s2t_clip_coef(N.fp(d), n, clip, N.fp(out), N.stream()), "s2t_clip_coef")
    ref = OC.clip_coef_ref(n, torch.float64)
    assert 0.45 < float(ref[0]) < 0.55                                       # the clip binds
    r = float(((out.double().cpu() - ref).abs() / _floor_bound(OC.FP32_COST["clip_coef"], ref, ref.abs())).max())
    assert r <= 1.0, r
    N.check(L.s2t_clip_coef(N.fp(d), n, 0.0, N.fp(out), N.stream()), "s2t_clip_coef")
    assert float(out[0]) == 1.0                                              # clip off
    d[n // 2, 0] = float("nan")
    N.check(L.s2t_clip_coef(N.fp(d), n, clip, N.fp(out), N.stream()), "s2t_clip_coef")
    assert float(out[0]) == 1.0 and bool(torch.isnan(out[1]))                # question 1: NaN norm


@pytest.mark.parametrize("name", list(OC.COEF_CASES))
def test_scaled_adam_coef_on_crafted_state(dev, name):
    """s2t_scaled_adam_coef alone: window periods 1 and 1024, ties and NaN in the window, 256 / 257
    / 600 tensors in the group, one foreign tensor of the store on either side of it."""
    from speech2text_amd import _native as N
    t = OC.coef_case(name)
    ng, nseg, P, period, k = t["ng"], t["nseg"], t["P"], t["period"], t["k"]
    h = OF.SA_DEFAULTS
    beta1, beta2 = h["betas"]
    f = lambda x: x.to(dev).float().contiguous()                             # noqa: E731
    partial, rms, seas, sg, mn = (f(t[q]) for q in ("partial", "param_rms", "scale_exp_avg_sq",
                                                     "scale_grads", "model_norms"))
    fstate = torch.tensor([t["threshold"], 0.0, 0.0], device=dev)
    istate = _i32([1, t["num_clipped"], 0], dev)
    segstat = torch.zeros(nseg, 3, device=dev)
    segc = torch.zeros(nseg, 12, device=dev)
    beta2c = beta2 ** P
    begin, lens = _i32(list(range(nseg + 1)), dev), t["lens"].to(dev).int()      # one chunk per tensor
    N.check(N.lib().s2t_scaled_adam_coef(
        N.fp(partial), N.ip(begin), N.ip(lens), nseg, 1,
        1 + ng, t["lr"], beta1, beta2, h["eps"], h["scalar_lr_scale"], h["param_min_rms"],
        h["param_max_rms"], h["scalar_max"], t["clip_val"], t["cs"], k, P, period,
        1 - beta2 ** (k + 1), 1 - beta2c ** ((k + 1) // P), beta2c, N.fp(rms), N.fp(seas), N.fp(sg),
        N.fp(mn), N.fp(fstate), N.ip(istate), N.fp(segstat), N.fp(segc), None, N.stream()),
        "s2t_scaled_adam_coef")
    ref, _ = OC.coef_ref(name, torch.float64)
    assert int(_bits(segc[0]).abs().sum()) == 0 and int(_bits(segc[-1]).abs().sum()) == 0
    if name == "most_nan":
        assert isinstance(ref, RuntimeError)
        assert istate.tolist() == [1, 1, 1] and bool(torch.isnan(fstate[0]))     # factor 0: "clipped"
        assert int(torch.isnan(mn).sum()) == 7 and bool(torch.isfinite(mn[k % period]))
        return
    case = "coef_" + name
    got = dict(param_rms=OC.mask_scalars(rms, t["lens"][1:1 + ng]), scale_exp_avg_sq=seas,
               scale_grads=sg, scale_step=segc[1:1 + ng, 1], model_norms=mn, threshold=fstate[:1],
               factor=fstate[2:3], coef=segc[1:1 + ng, 2])
    worst = 0.0
    for q in OC.COEF_QUANTITIES:
        r = OC.ratio(case, q, got[q], ref[q])
        assert r <= 1.0, f"{case}: {q} at {r:.3g} x its bound"
        worst = max(worst, r)
    print(f"{case}: worst error / bound {worst:.3f}")
    threshold_step = k % period == 0
    clipped = int(float(ref["factor"]) < float(OF.clip_factor(t["partial"][:, 0].double().sum(),
                                                                t["clip_val"])))
    assert istate.tolist() == [1, (0 if threshold_step else t["num_clipped"]) + clipped, 0]
    assert ref["num_clipped"] == istate[1].item()
    rows = segc[1:1 + ng].cpu()
    assert torch.equal(rows[:, 3], ref["bc"].float()) and torch.equal(rows[:, 4], ref["lim"].float())
    assert torch.equal(rows[:, 8], torch.ones(ng)) and torch.equal(rows[:, 9], torch.ones(ng))


def test_coef_refuses_a_window_beyond_its_sort_buffer(dev):
    """Question 4: the C ABI answers -1 beyond 1024 and the optimizer never gets there: it refuses
    the period when it is built (tests/test_optim_f64.py)."""
    from speech2text_amd.optimizer.scaled_adam import ScaledAdam
    with pytest.raises(ValueError, match="1..1024"):
        ScaledAdam([torch.nn.Parameter(torch.zeros(3, device=dev))], clipping_scale=2.0,
                   clipping_update_period=1025)
