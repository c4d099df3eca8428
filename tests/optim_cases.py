"""Seeded optimizer cases shared by tests/test_optim_f64.py (CPU) and
tests/test_gpu_optim_kernels.py (GPU), with what fp32 costs the restatement on each of them.

Test infrastructure (not a test file).  The shapes are the smallest at which each branch of
csrc/optim.hip can still go wrong: a chunk is 8192 elements, a workgroup 256 threads, every
per-tensor loop of the coefficient kernel strides by 256, tensors are padded to 4 elements.

FP32_COST[case][quantity] is the worst error over the case's checkpoints of tests/optim_f64.py run
in float32 against the same code in float64 (the REFERENCE's own cost, never the kernel's), scaled
by the quantity's largest magnitude (`rel_err`); param_rms is measured per entry (`rel_each`), each
tensor's rms being a quantity of its own.  The CPU file re-measures every figure and holds it to a
factor 4 both ways; the device and the host forms are held to `allowed`: 4 x the figure, never
tighter than atol 2e-6 + rtol 3e-5 (the bounds of tests/test_gpu_optimizer.py).  This is a rule of its own,
with its own measure and MARGIN = 4: not the one of tests/yardstick.py.
"""
import functools

import torch

import optim_f64 as OF

MARGIN = 4.0
FLOOR_ATOL, FLOOR_RTOL = 2e-6, 3e-5


# ------------------------------------------------------------------ error measures
def _d(x):
    return x.detach().double().cpu().reshape(-1)


def rel_err(got, ref):
    """max |got - ref| over the finite entries of ref, relative to max |ref| there; inf unless
    NaN / +-inf sit at the same places in both."""
    got, ref = _d(got), _d(ref)
    fin = torch.isfinite(ref)
    same = torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.equal(got[~fin & ~torch.isnan(ref)],
                                                                         ref[~fin & ~torch.isnan(ref)])
    if not same:
        return float("inf")
    if not bool(fin.any()):
        return 0.0
    return float((got[fin] - ref[fin]).abs().max() / max(float(ref[fin].abs().max()), 1e-300))


def rel_each(got, ref):
    """max over entries of |got - ref| / |ref| (for positive per-tensor quantities)."""
    got, ref = _d(got), _d(ref)
    fin = torch.isfinite(ref)
    if not torch.equal(torch.isnan(got), torch.isnan(ref)):
        return float("inf")
    if not bool(fin.any()):
        return 0.0
    return float(((got[fin] - ref[fin]).abs() / ref[fin].abs().clamp(min=1e-300)).max())


def measure(q):
    return rel_each if q == "param_rms" else rel_err


def allowed(case, q, ref):
    """Elementwise bound on |got - ref| for quantity q of `case` (see the module docstring)."""
    ref = _d(ref)
    fin = torch.isfinite(ref)
    a = torch.nan_to_num(ref.abs(), nan=0.0, posinf=0.0, neginf=0.0)
    scale = a if q == "param_rms" else torch.full_like(a, float(a[fin].max()) if bool(fin.any()) else 0.0)
    return torch.maximum(MARGIN * FP32_COST[case][q] * scale, FLOOR_ATOL + FLOOR_RTOL * a)


def ratio(case, q, got, ref):
    """Worst |got - ref| / allowed (inf if the non-finite entries differ): <= 1 passes."""
    if measure(q)(got, ref) == float("inf"):
        return float("inf")
    got, ref = _d(got), _d(ref)
    fin = torch.isfinite(ref)
    if not bool(fin.any()):
        return 0.0
    return float(((got - ref).abs()[fin] / allowed(case, q, ref)[fin]).max())


# ------------------------------------------------------------------ ScaledAdam store S1
_A = [("w33x17", (33, 17)),                 # 561 elements: the store pads it to 564
      ("one_chunk", (8192,)),               # exactly one chunk
      ("two_chunks", (8193,)),              # second chunk of length 4 with one live lane
      ("four_chunks", (3 * 8192 + 5,)),
      ("s1", (1,)), ("s0", ()),             # scalars
      ("conv", (64, 3, 3)),
      ("tiny", (40,)),                      # rms 3e-6 < param_min_rms
      ("near_max", (50,)),                  # rms 2.95, gradients push the scale up: the cap binds
      ("over_max", (50,)),                  # rms 3.2: the cap is negative
      ("s_pos", (1,)), ("s_neg", ())]       # 9.99 / -9.99 driven outward past scalar_max
_FREE = [("free", (7,))]                    # trainable, in no group: between the two groups
_B = [("b%d" % i, (3 + i % 3,)) for i in range(300)]    # > 256 tensors in one group
S1 = _A + _FREE + _B
S1_IDX_A = list(range(len(_A)))
S1_IDX_B = list(range(len(_A) + 1, len(S1)))
_NAME = {n: i for i, (n, _) in enumerate(S1)}


@functools.lru_cache(maxsize=None)
def _s1_init():
    g = torch.Generator().manual_seed(11)
    out = []
    for name, shp in S1:
        t = torch.randn(shp, generator=g) * 0.3
        if name == "tiny":
            t = t / (t ** 2).mean().sqrt() * 3e-6
        elif name in ("near_max", "over_max"):
            t = t / (t ** 2).mean().sqrt() * (2.95 if name == "near_max" else 3.2)
        elif name in ("s_pos", "s_neg"):
            t = torch.full(shp, 9.99 if name == "s_pos" else -9.99)
        out.append(t)
    return tuple(out)


def s1_init():
    return [t.clone() for t in _s1_init()]


def _run(seed, period, P, steps, ckpt, cs=2.0, pre_clip=None, spike=None, skips=(), inf=None,
         nan=None, betas=(0.9, 0.98)):
    return dict(seed=seed, period=period, P=P, steps=steps, ckpt=tuple(ckpt), cs=cs,
                pre_clip=pre_clip, spike=spike, skips=tuple(skips), inf=inf, nan=nan, betas=betas)


# gradient norm over the store is about 210 (43.5 k elements of unit variance): 50 binds, 1e4 does
# not, not even on the 10 x spike
RUNS = {
    "p1_s1": _run(1, 1, 1, 12, (0, 1, 5, 11), pre_clip=50.0),
    # the trainer's clip does not bind, so that the spike meets ScaledAdam's own threshold
    "p6_s4": _run(2, 6, 4, 30, (0, 3, 6, 7, 12, 17, 18, 29), pre_clip=1e4, spike=17),
    # irregular step 10; an inf and a NaN element once clipping is live
    "p12_s3": _run(13, 12, 3, 45, (2, 10, 12, 24, 31, 32, 35, 36, 44), pre_clip=50.0, inf=31, nan=35),
    # irregular steps 10, 20; dropped: k = 0, k % P == P - 1 (k = 7), the irregular threshold step
    # 20, the regular threshold step 25 and the two after a threshold step together (26, 27)
    "p25_s4": _run(4, 25, 4, 50, (0, 1, 7, 8, 20, 21, 25, 26, 27, 28, 49), pre_clip=50.0,
                   skips=(0, 7, 20, 25, 26, 27)),
    "p50_s4": _run(5, 50, 4, 50, (9, 10, 11, 20, 33, 34, 40, 43, 49), spike=33),      # irregular 10, 20, 40
    "none": _run(6, 100, 4, 12, (0, 3, 4, 11), cs=None, pre_clip=50.0),
    # question 1: a NaN gradient element while no threshold exists.  The trainer's factor is 1, the
    # finite elements step, the NaN stays in its own element (3 steps: at k = 3 the tensor's rms
    # turns NaN, from where fminf / fmaxf on the device and torch.minimum / clamp part ways)
    "none_nan": _run(7, 100, 4, 3, (0, 1, 2), cs=None, pre_clip=50.0, nan=1),
    "nan_step0": _run(8, 6, 4, 3, (0, 1, 2), pre_clip=50.0, nan=0),
    # beta2 = 0.9: 1 - beta2^(k+1) passes 0.99 at k = 43
    "beta2_0.9": _run(9, 25, 4, 50, (3, 25, 42, 43, 44, 49), pre_clip=50.0, betas=(0.9, 0.9)),
}


def s1_groups(run):
    r = RUNS[run]
    common = dict(clipping_scale=r["cs"], clipping_update_period=r["period"],
                  size_update_period=r["P"], betas=r["betas"])
    return [dict(idx=S1_IDX_A, lr=0.1, **common), dict(idx=S1_IDX_B, lr=0.02, **common)]


def s1_grads(run, it):
    """The float32 gradients of step `it`, one per tensor of S1 (a function of the run and the step
    alone, never of the parameters: every implementation sees the same inputs)."""
    r = RUNS[run]
    g = torch.Generator().manual_seed(7000 + 131 * r["seed"] + it)
    init = _s1_init()
    out = []
    for (name, shp), p0 in zip(S1, init):
        t = torch.randn(shp, generator=g)
        if name in ("near_max", "over_max"):
            t = 0.3 * t - p0 / (p0 ** 2).mean().sqrt()
        elif name in ("s_pos", "s_neg"):
            t = -torch.sign(p0) * (1.0 + 0.3 * t.abs())
        if it == r["spike"]:
            t = t * 10.0
        out.append(t)
    if it == r["inf"]:
        out[_NAME["w33x17"]].view(-1)[5] = float("inf")
    if it == r["nan"]:
        out[_NAME["two_chunks"]].view(-1)[8192] = float("nan")      # the live lane of the short chunk
    return out


SA_FLAT = ("p", "delta", "exp_avg_sq")
SA_GROUP = ("param_rms", "scale_exp_avg_sq", "scale_grads", "scale_step", "model_norms", "threshold")
SA_INT = ("has_threshold", "num_clipped", "step")
SA_QUANTITIES = SA_FLAT + SA_GROUP


def _cat(ts, like):
    return torch.cat([(torch.zeros_like(l) if t is None else t).reshape(-1) for t, l in zip(ts, like)])


def mask_scalars(rms, lens):
    """param_rms with the entries of one-element tensors set to 0: there it is |p|, which the
    parameters themselves cover and which, passing through 0, has no relative error to speak of."""
    return torch.where(lens.to(rms.device) > 1, rms, torch.zeros_like(rms))


def sa_snapshot(ref):
    s = dict(p=_cat(ref.p, ref.p), delta=_cat(ref.delta, ref.p),
             exp_avg_sq=_cat(ref.exp_avg_sq, ref.p), grad=_cat(ref.grad, ref.p), groups=[])
    for G in ref.groups:
        thr = G["threshold"]
        s["groups"].append(dict(
            param_rms=mask_scalars(G["param_rms"], G["lens"]), scale_exp_avg_sq=G["scale_exp_avg_sq"].clone(),
            scale_grads=G["scale_grads"].clone(), scale_step=G["scale_step"].clone(),
            model_norms=G["model_norms"].clone(),
            threshold=torch.zeros(1, dtype=ref.dtype) if thr is None else thr.reshape(1).clone(),
            has_threshold=int(thr is not None), num_clipped=G["num_clipped"], step=G["step"]))
    return s


def sa_evaluate(run, dtype):
    """-> ({step: snapshot after that step}, margins) of the restatement in `dtype`."""
    r = RUNS[run]
    ref = OF.ScaledAdamRef(s1_init(), s1_groups(run), dtype, pre_clip=r["pre_clip"])
    snaps = {}
    for it in range(r["steps"]):
        ref.step(s1_grads(run, it), skip=it in r["skips"])
        if it in r["ckpt"]:
            snaps[it] = sa_snapshot(ref)
    return snaps, ref.margins


@functools.lru_cache(maxsize=None)
def sa_reference(run):
    """float64 snapshots and margins of a run, computed once per process (do not modify)."""
    return sa_evaluate(run, torch.float64)


def sa_compare(fn, got, ref):
    """{quantity: worst fn(quantity, got, ref)} over flat and per-group state of two snapshots."""
    out = {q: fn(q, got[q], ref[q]) for q in SA_FLAT}
    for q in SA_GROUP:
        out[q] = max(fn(q, a[q], b[q]) for a, b in zip(got["groups"], ref["groups"]))
    return out


def sa_fp32_figures(run):
    ref, _ = sa_reference(run)
    f32, _ = sa_evaluate(run, torch.float32)
    worst = {q: 0.0 for q in SA_QUANTITIES}
    for it in ref:
        for q, v in sa_compare(lambda q, a, b: measure(q)(a, b), f32[it], ref[it]).items():
            worst[q] = max(worst[q], v)
    return worst


# ------------------------------------------------------------------ Adam / AdamW store S2
# The five tensors of the issue, four small ones more (S2T_ADAM_MAX_GROUPS + 1 = 9 groups need nine
# grouped tensors) and one trainable tensor in no group, which has to come last: the fused path
# wants the groups to tile the store from its first tensor on.
S2 = [(300, 17), (33,), (64, 8, 3), (5,), (2 * 8192 + 7,), (6,), (2, 2), (11,), (7,), (9,)]
S2_GROUPED = 9
ADAM_MAX_GROUPS = 8
_SPLITS = {1: [9], 2: [2, 7], 8: [1, 1, 1, 1, 2, 1, 1, 1], 9: [1] * 9}


def _adam(name, ngroups, wd, pre_clip, skips=(), steps=12):
    return dict(name=name, ngroups=ngroups, wd=wd, pre_clip=pre_clip, skips=tuple(skips), steps=steps,
                ckpt=(0, 1, 5, 6, 11), fused=ngroups <= ADAM_MAX_GROUPS)


# gradient norm over the store is about 0.3 * sqrt(23.1 k) = 46 (4 x on steps 2, 7): 5 binds
ADAM_CASES = {
    "adamw_g1_wd0": _adam("AdamW", 1, (0.0,), None),
    "adam_g1_wd0.1": _adam("Adam", 1, (0.1,), 5.0),
    "adamw_g2": _adam("AdamW", 2, (0.0, 0.1), 5.0, skips=(0, 6)),     # dropped: step 1 and mid-run
    "adam_g2": _adam("Adam", 2, (0.1, 0.0), None, skips=(0, 6)),
    "adamw_g8": _adam("AdamW", 8, (0.1, 0.0), 5.0),
    "adam_g8": _adam("Adam", 8, (0.0, 0.1), 5.0, skips=(5,)),
    "adamw_g9_host": _adam("AdamW", 9, (0.1, 0.0), 5.0, skips=(0, 6)),
    "adam_g9_host": _adam("Adam", 9, (0.0, 0.1), 5.0, skips=(5,)),
}


def s2_init():
    g = torch.Generator().manual_seed(21)
    return [torch.randn(s, generator=g) for s in S2]


def s2_groups(case):
    c = ADAM_CASES[case]
    out, lo = [], 0
    for q, n in enumerate(_SPLITS[c["ngroups"]]):
        out.append(dict(idx=list(range(lo, lo + n)), lr=3e-3 if q % 2 == 0 else 1e-3,
                        betas=(0.9, 0.98), eps=1e-8, weight_decay=c["wd"][q % len(c["wd"])]))
        lo += n
    assert lo == S2_GROUPED
    return out


def s2_grads(case, it):
    g = torch.Generator().manual_seed(9000 + 17 * sorted(ADAM_CASES).index(case) + it)
    return [torch.randn(s, generator=g) * (1.2 if it % 5 == 2 else 0.3) for s in S2]


ADAM_QUANTITIES = ("p", "exp_avg", "exp_avg_sq")


def adam_snapshot(ref):
    return dict(p=_cat(ref.p, ref.p), exp_avg=_cat(ref.exp_avg, ref.p),
                exp_avg_sq=_cat(ref.exp_avg_sq, ref.p), grad=_cat(ref.grad, ref.p),
                step=ref.step_count)


def adam_evaluate(case, dtype):
    c = ADAM_CASES[case]
    ref = OF.AdamRef(s2_init(), s2_groups(case), c["name"] == "AdamW", dtype, pre_clip=c["pre_clip"])
    snaps = {}
    for it in range(c["steps"]):
        ref.step(s2_grads(case, it), skip=it in c["skips"])
        if it in c["ckpt"]:
            snaps[it] = adam_snapshot(ref)
    return snaps


@functools.lru_cache(maxsize=None)
def adam_reference(case):
    return adam_evaluate(case, torch.float64)


def adam_fp32_figures(case):
    ref, f32 = adam_reference(case), adam_evaluate(case, torch.float32)
    return {q: max(rel_err(f32[it][q], ref[it][q]) for it in ref) for q in ADAM_QUANTITIES}


# ------------------------------------------------------------------ direct C-ABI cases
CHUNK_LENS = (4, 8188, 8192)                # s2t_seg_stats: one workgroup per chunk


def seg_stats_case():
    """-> p, g (float32, the three chunks back to back), chunk_off, chunk_len."""
    g = torch.Generator().manual_seed(31)
    n = sum(CHUNK_LENS)
    off = [0, CHUNK_LENS[0], CHUNK_LENS[0] + CHUNK_LENS[1]]
    return torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.7, off, list(CHUNK_LENS)


def seg_stats_ref(dtype):
    """[3 chunks][sum g^2, sum p g, sum p^2] in dtype, and per entry the sum of the terms'
    magnitudes (the scale an error of a cancelling sum is measured on)."""
    p, g, off, ln = seg_stats_case()
    p, g = p.to(dtype), g.to(dtype)
    rows, mags = [], []
    for o, n in zip(off, ln):
        a, b = p[o:o + n], g[o:o + n]
        rows.append(torch.stack([(b * b).sum(), (a * b).sum(), (a * a).sum()]))
        mags.append(torch.stack([(b * b).sum(), (a * b).abs().sum(), (a * a).sum()]))
    return torch.stack(rows), torch.stack(mags).double()


CLIP_NCHUNKS = (1, 255, 256, 257, 1000)     # s2t_clip_coef: 256 threads stride over the chunks


def clip_coef_case(n):
    g = torch.Generator().manual_seed(40 + n)
    part = torch.rand(n, 3, generator=g) * 50.0
    return part, 0.5 * float(part[:, 0].double().sum().sqrt())     # binds: factor about 0.5


def clip_coef_ref(n, dtype):
    part, clip = clip_coef_case(n)
    s = part[:, 0].to(dtype).sum()
    return torch.stack([OF.clip_factor(s, clip), s.sqrt()])


def _coef(seed, ng, period, k, P=4, norms="random", cs=2.0):
    return dict(seed=seed, ng=ng, period=period, k=k, P=P, norms=norms, cs=cs)


# s2t_scaled_adam_coef on crafted partial sums / model_norms.  Every k is a threshold step
# (k % period == 0) and, but for "p1024" at P = 4, a size-update step is among them.
COEF_CASES = {
    "p1": _coef(1, 256, 1, 7),                               # k % 4 == 3: size update too
    "p1024": _coef(2, 257, 1024, 1024, P=5),                 # 1024 % 5 == 4: size update too
    "all_equal": _coef(3, 256, 12, 12, norms="all_equal"),
    "tie_pairs": _coef(4, 257, 12, 24, norms="tie_pairs"),
    "one_nan": _coef(5, 256, 12, 36, norms="one_nan"),
    "most_nan": _coef(6, 257, 12, 12, norms="most_nan"),     # median NaN: istate[2], the host raises
    "wide": _coef(7, 600, 6, 11, P=3),                       # 11 % 3 == 2; not a threshold step
    "wide_thr": _coef(8, 600, 6, 12),
}
COEF_QUANTITIES = ("param_rms", "scale_exp_avg_sq", "scale_grads", "scale_step", "model_norms",
                   "threshold", "factor", "coef")


def coef_case(name):
    """One tensor of the store in front of the group and one behind it (seg_lo = 1), every tensor one
    chunk.  -> dict of float32 / int inputs and state."""
    c = COEF_CASES[name]
    g = torch.Generator().manual_seed(500 + c["seed"])
    ng, nseg, period, P = c["ng"], c["ng"] + 2, c["period"], c["P"]
    lens = torch.randint(2, 8193, (nseg,), generator=g)
    lens[1 + torch.randperm(ng, generator=g)[:ng // 8]] = 1                # scalars among them
    rms = torch.rand(nseg, generator=g) * 0.5 + 0.05
    rms[3], rms[4], rms[5] = 3e-6, 2.999, 3.3                              # the three limits
    pp = rms * rms * lens
    gg = (torch.rand(nseg, generator=g) + 0.5) * lens
    pg = torch.randn(nseg, generator=g) * (pp * gg).sqrt() * 0.1
    pg[4] = -pg[4].abs() - 1.0
    partial = torch.stack([gg, pg, pp], dim=1).contiguous()
    if c["norms"] == "random":
        mn = torch.rand(period, generator=g) * 40 + 5
    elif c["norms"] == "all_equal":
        mn = torch.full((period,), 17.25)
    elif c["norms"] == "tie_pairs":            # slot 0 is rewritten; sorted: 1 2 2 3 3 4 [4] 5 5 6 6 T
        mn = torch.tensor([1.0, 4, 2, 6, 3, 5, 5, 3, 6, 2, 4, 1])
    else:
        mn = torch.rand(period, generator=g) * 40 + 5
        nn = 1 if c["norms"] == "one_nan" else 7
        mn[1 + torch.randperm(period - 1, generator=g)[:nn]] = float("nan")
    return dict(partial=partial, lens=lens, ng=ng, nseg=nseg, period=period, P=P, k=c["k"],
                cs=c["cs"], model_norms=mn, param_rms=rms[1:1 + ng] * 1.01,
                scale_exp_avg_sq=torch.rand(ng, generator=g) * 4 + 0.1,
                scale_grads=torch.randn(P, ng, generator=g), threshold=30.0, num_clipped=3,
                clip_val=40.0, lr=0.05)


def coef_ref(name, dtype):
    """-> (state dict after OF.group_coef in dtype, or the RuntimeError it raised; margins)."""
    t = coef_case(name)
    ng = t["ng"]
    part = t["partial"].to(dtype)
    h = dict(OF.SA_DEFAULTS, lr=t["lr"], clipping_scale=t["cs"], size_update_period=t["P"],
             clipping_update_period=t["period"])
    G = dict(h=h, param_rms=t["param_rms"].to(dtype), scale_exp_avg_sq=t["scale_exp_avg_sq"].to(dtype),
             scale_grads=t["scale_grads"].to(dtype), model_norms=t["model_norms"].to(dtype),
             threshold=torch.tensor(t["threshold"], dtype=dtype), num_clipped=t["num_clipped"])
    c = OF.clip_factor(part[:, 0].sum(), t["clip_val"])
    margins = []
    grp = part[1:1 + ng]
    try:
        gm, sanitize, sstep, coef, bc, lim = OF.group_coef(G, t["k"], c, grp[:, 0], grp[:, 1], grp[:, 2],
                                                           t["lens"][1:1 + ng], margins)
    except RuntimeError as e:
        return e, margins
    out = {q: G[q] for q in ("scale_exp_avg_sq", "scale_grads", "scale_step", "model_norms")}
    out["param_rms"] = mask_scalars(G["param_rms"], t["lens"][1:1 + ng])
    out.update(threshold=G["threshold"].reshape(1), factor=gm.reshape(1), coef=coef, bc=bc, lim=lim,
               sanitize=sanitize, num_clipped=G["num_clipped"])
    return out, margins


def coef_fp32_figures(name):
    ref, _ = coef_ref(name, torch.float64)
    f32, _ = coef_ref(name, torch.float32)
    return {q: measure(q)(f32[q], ref[q]) for q in COEF_QUANTITIES}


# ------------------------------------------------------------------ the project's optimizers
def sa_build(run, device):
    """The project's ScaledAdam on a FlatStore of S1 on `device` -> (params, store, optimizer)."""
    from speech2text_amd.flat import FlatStore
    from speech2text_amd.optimizer.scaled_adam import ScaledAdam
    r = RUNS[run]
    ps = [torch.nn.Parameter(t.to(device)) for t in s1_init()]
    st = FlatStore(ps)
    opt = ScaledAdam([{"params": [ps[i] for i in g["idx"]], "lr": g["lr"]} for g in s1_groups(run)],
                     clipping_scale=r["cs"], betas=r["betas"], size_update_period=r["P"],
                     clipping_update_period=r["period"])
    opt.pre_clip, opt.zero_grad_in_step = r["pre_clip"], True
    opt.skip_flag = torch.zeros(1, device=device)          # a device tensor, as the trainer sets it
    return ps, st, opt


def adam_build(case, device):
    from speech2text_amd.flat import FlatStore
    from speech2text_amd.optimizer.flat_adam import FlatAdam, FlatAdamW
    c = ADAM_CASES[case]
    ps = [torch.nn.Parameter(t.to(device)) for t in s2_init()]
    st = FlatStore(ps)
    groups = [{"params": [ps[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]}
              for g in s2_groups(case)]
    opt = (FlatAdamW if c["name"] == "AdamW" else FlatAdam)(groups, betas=(0.9, 0.98), eps=1e-8)
    opt.pre_clip, opt.zero_grad_in_step = c["pre_clip"], True
    opt.skip_flag = torch.zeros(1, device=device)
    return ps, st, opt


def take_step(ps, opt, grads, skip):
    for p, g in zip(ps, grads):
        p.grad.copy_(g)
    opt.skip_flag.fill_(1.0 if skip else 0.0)
    opt.step()


def gather(st, buf):
    """The tensors' own elements of a flat buffer of the store, back to back (no pad lanes)."""
    return torch.cat([buf[o:o + n] for o, n in zip(st.offsets, st.lengths)])


def pad_lanes(st, buf):
    """The elements of a flat buffer that belong to no tensor."""
    m = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    for o, n in zip(st.offsets, st.lengths):
        m[o:o + n] = False
    return buf[m]


def sa_project_snapshot(st, opt):
    """The state of the project's ScaledAdam in sa_snapshot's layout (scale_step is read from the
    coefficient kernel's hand-over buffer, which only the device path has)."""
    s = dict(p=gather(st, st.flat_p), delta=gather(st, opt._delta), exp_avg_sq=gather(st, opt._eas),
             grad=st.flat_g.clone(), groups=[])
    for g in opt._gstate:
        lens = st.seg_lengths[g["lo"]:g["hi"]]
        d = dict(param_rms=mask_scalars(g["param_rms"], lens), scale_exp_avg_sq=g["scale_exp_avg_sq"].clone(),
                 scale_grads=g["scale_grads"].clone(), model_norms=g["model_norms"].clone(),
                 threshold=g["fstate"][:1].clone(), has_threshold=int(g["istate"][0]),
                 num_clipped=int(g["istate"][1]), step=g["step"])
        if opt._segc is not None:
            d["scale_step"] = opt._segc.view(-1, 12)[g["lo"]:g["hi"], 1].clone()
        s["groups"].append(d)
    return s


def sa_hold(case, got, ref, where=""):
    """Assert a project snapshot against a float64 one at the case's bounds -> worst ratio."""
    worst = 0.0
    for q in SA_FLAT:
        r = ratio(case, q, got[q], ref[q])
        assert r <= 1.0, f"{case} {where}: {q} at {r:.3g} x its bound"
        worst = max(worst, r)
    for gi, (a, b) in enumerate(zip(got["groups"], ref["groups"])):
        for q in SA_INT:
            assert a[q] == b[q], f"{case} {where}: group {gi} {q} {a[q]} != {b[q]}"
        for q in SA_GROUP:
            if q not in a or (q == "threshold" and not b["has_threshold"]):
                continue
            r = ratio(case, q, a[q], b[q])
            assert r <= 1.0, f"{case} {where}: group {gi} {q} at {r:.3g} x its bound"
            worst = max(worst, r)
    return worst


def adam_project_snapshot(st, opt, ps):
    """State of FlatAdam / FlatAdamW in adam_snapshot's layout, from torch's own per-parameter state
    (views of the flat moments on the fused path).  `step` is the one count every state shares."""
    zeros = lambda p: torch.zeros(p.numel(), device=p.device)                   # noqa: E731
    steps = {float(opt.state[p]["step"]) for p in ps if p in opt.state and len(opt.state[p])}
    assert len(steps) <= 1, steps
    get = lambda k: torch.cat([opt.state[p][k].reshape(-1) if p in opt.state and len(opt.state[p])  # noqa
                               else zeros(p) for p in ps])
    return dict(p=gather(st, st.flat_p), exp_avg=get("exp_avg"), exp_avg_sq=get("exp_avg_sq"),
                grad=st.flat_g.clone(), step=int(steps.pop()) if steps else 0)


def adam_hold(case, got, ref, where=""):
    assert got["step"] == ref["step"], f"{case} {where}: step {got['step']} != {ref['step']}"
    worst = 0.0
    for q in ADAM_QUANTITIES:
        r = ratio(case, q, got[q], ref[q])
        assert r <= 1.0, f"{case} {where}: {q} at {r:.3g} x its bound"
        worst = max(worst, r)
    return worst


# ------------------------------------------------------------------ measured cost of fp32
# Per case: the figures of sa_fp32_figures / adam_fp32_figures / coef_fp32_figures rounded up to two
# digits, the measured values on the line behind.  A figure of 0 is exact: the quantity is never
# written in that case, or is a copy of another.  "seg_stats" is relative to the sum of the terms'
# magnitudes, "clip_coef" the worst of the five chunk counts.
FP32_COST = {
    "p1_s1": dict(p=9.1e-08, delta=6.8e-07, exp_avg_sq=2.0e-07, param_rms=2.2e-07,
                  scale_exp_avg_sq=3.7e-07, scale_grads=1.3e-07, scale_step=7.6e-07,
                  model_norms=7.4e-08, threshold=7.4e-08),
    # 9.057e-08 6.763e-07 1.974e-07 2.186e-07 3.698e-07 1.297e-07 7.563e-07 7.376e-08 7.376e-08
    "p6_s4": dict(p=1.5e-07, delta=4.8e-07, exp_avg_sq=2.5e-07, param_rms=3.6e-07,
                  scale_exp_avg_sq=1.4e-07, scale_grads=1.6e-07, scale_step=3.6e-07,
                  model_norms=9.2e-08, threshold=6.5e-08),
    # 1.438e-07 4.713e-07 2.481e-07 3.502e-07 1.389e-07 1.555e-07 3.525e-07 9.149e-08 6.424e-08
    "p12_s3": dict(p=1.9e-07, delta=7.9e-07, exp_avg_sq=5.1e-07, param_rms=4.2e-07,
                   scale_exp_avg_sq=3.6e-07, scale_grads=3.5e-07, scale_step=1.2e-06,
                   model_norms=2.6e-07, threshold=2.6e-07),
    # 1.810e-07 7.887e-07 5.029e-07 4.190e-07 3.573e-07 3.418e-07 1.162e-06 2.527e-07 2.527e-07
    "p25_s4": dict(p=1.8e-07, delta=4.6e-07, exp_avg_sq=4.1e-07, param_rms=3.6e-07,
                   scale_exp_avg_sq=3.0e-07, scale_grads=3.1e-07, scale_step=2.1e-07,
                   model_norms=2.4e-07, threshold=1.5e-07),
    # 1.790e-07 4.528e-07 4.050e-07 3.537e-07 2.969e-07 3.006e-07 2.038e-07 2.343e-07 1.448e-07
    "p50_s4": dict(p=1.9e-07, delta=6.8e-07, exp_avg_sq=3.5e-07, param_rms=5.0e-07,
                   scale_exp_avg_sq=4.6e-07, scale_grads=2.3e-07, scale_step=3.0e-07,
                   model_norms=1.1e-07, threshold=7.2e-08),
    # 1.829e-07 6.763e-07 3.484e-07 4.963e-07 4.515e-07 2.231e-07 2.968e-07 1.074e-07 7.191e-08
    "none": dict(p=1.2e-07, delta=4.7e-07, exp_avg_sq=2.3e-07, param_rms=2.5e-07,
                 scale_exp_avg_sq=3.3e-07, scale_grads=1.9e-07, scale_step=5.3e-07,
                 model_norms=0.0, threshold=0.0),
    # 1.185e-07 4.660e-07 2.288e-07 2.408e-07 3.252e-07 1.853e-07 5.233e-07 0.000e+00 0.000e+00
    "none_nan": dict(p=8.7e-08, delta=1.7e-07, exp_avg_sq=5.3e-07, param_rms=8.7e-08,
                     scale_exp_avg_sq=0.0, scale_grads=3.1e-07, scale_step=0.0, model_norms=0.0,
                     threshold=0.0),
    # 8.648e-08 1.637e-07 5.222e-07 8.655e-08 0.000e+00 3.097e-07 0.000e+00 0.000e+00 0.000e+00
    "nan_step0": dict(p=7.1e-08, delta=1.6e-07, exp_avg_sq=1.1e-07, param_rms=8.7e-08,
                      scale_exp_avg_sq=0.0, scale_grads=1.5e-07, scale_step=0.0,
                      model_norms=7.7e-08, threshold=0.0),
    # 7.073e-08 1.569e-07 1.008e-07 8.655e-08 0.000e+00 1.496e-07 0.000e+00 7.624e-08 0.000e+00
    "beta2_0.9": dict(p=1.6e-07, delta=6.5e-07, exp_avg_sq=3.3e-07, param_rms=4.0e-07,
                      scale_exp_avg_sq=3.6e-07, scale_grads=2.9e-07, scale_step=4.7e-07,
                      model_norms=2.1e-07, threshold=1.5e-07),
    # 1.590e-07 6.463e-07 3.246e-07 3.965e-07 3.534e-07 2.817e-07 4.611e-07 2.022e-07 1.483e-07
    "adamw_g1_wd0": dict(p=1.7e-07, exp_avg=1.4e-07, exp_avg_sq=2.0e-07),
    # 1.676e-07 1.371e-07 1.963e-07
    "adam_g1_wd0.1": dict(p=2.6e-07, exp_avg=1.4e-07, exp_avg_sq=2.1e-07),
    # 2.556e-07 1.342e-07 2.042e-07
    "adamw_g2": dict(p=3.6e-07, exp_avg=1.4e-07, exp_avg_sq=2.2e-07),
    # 3.511e-07 1.366e-07 2.123e-07
    "adam_g2": dict(p=1.6e-07, exp_avg=1.3e-07, exp_avg_sq=2.2e-07),
    # 1.557e-07 1.255e-07 2.188e-07
    "adamw_g8": dict(p=3.2e-07, exp_avg=1.3e-07, exp_avg_sq=2.8e-07),
    # 3.171e-07 1.223e-07 2.796e-07
    "adam_g8": dict(p=1.7e-07, exp_avg=1.3e-07, exp_avg_sq=1.9e-07),
    # 1.655e-07 1.207e-07 1.818e-07
    "adamw_g9_host": dict(p=2.9e-07, exp_avg=1.5e-07, exp_avg_sq=3.1e-07),
    # 2.827e-07 1.487e-07 3.073e-07
    "adam_g9_host": dict(p=1.8e-07, exp_avg=1.3e-07, exp_avg_sq=1.7e-07),
    # 1.776e-07 1.227e-07 1.652e-07
    "coef_p1": dict(param_rms=5.4e-08, scale_exp_avg_sq=6.1e-08, scale_grads=4.7e-08,
                    scale_step=1.4e-07, model_norms=1.4e-08, threshold=1.4e-08, factor=2.1e-08,
                    coef=1.4e-08),
    # 5.349e-08 6.068e-08 4.630e-08 1.340e-07 1.349e-08 1.349e-08 2.043e-08 1.333e-08
    "coef_p1024": dict(param_rms=5.7e-08, scale_exp_avg_sq=8.9e-08, scale_grads=2.1e-08,
                       scale_step=2.2e-07, model_norms=6.4e-09, threshold=0.0, factor=2.8e-08,
                       coef=3.0e-08),
    # 5.696e-08 8.875e-08 2.014e-08 2.141e-07 6.334e-09 0.000e+00 2.747e-08 2.941e-08
    "coef_all_equal": dict(param_rms=0.0, scale_exp_avg_sq=0.0, scale_grads=2.4e-08,
                           scale_step=0.0, model_norms=1.1e-07, threshold=0.0, factor=1.3e-08,
                           coef=6.8e-08),
    # 0.000e+00 0.000e+00 2.342e-08 0.000e+00 1.022e-07 0.000e+00 1.220e-08 6.706e-08
    "coef_tie_pairs": dict(param_rms=0.0, scale_exp_avg_sq=0.0, scale_grads=8.8e-08,
                           scale_step=0.0, model_norms=4.0e-08, threshold=0.0, factor=5.9e-08,
                           coef=6.8e-08),
    # 0.000e+00 0.000e+00 8.714e-08 0.000e+00 3.923e-08 0.000e+00 5.888e-08 6.706e-08
    "coef_one_nan": dict(param_rms=0.0, scale_exp_avg_sq=0.0, scale_grads=6.5e-08, scale_step=0.0,
                         model_norms=7.0e-09, threshold=0.0, factor=5.8e-08, coef=6.8e-08),
    # 0.000e+00 0.000e+00 6.407e-08 0.000e+00 6.935e-09 0.000e+00 5.789e-08 6.706e-08
    "coef_wide": dict(param_rms=7.6e-08, scale_exp_avg_sq=7.8e-08, scale_grads=2.1e-08,
                      scale_step=2.0e-07, model_norms=3.8e-09, threshold=0.0, factor=5.5e-09,
                      coef=2.8e-08),
    # 7.508e-08 7.770e-08 2.015e-08 1.967e-07 3.761e-09 0.000e+00 5.410e-09 2.767e-08
    "coef_wide_thr": dict(param_rms=0.0, scale_exp_avg_sq=0.0, scale_grads=3.0e-08, scale_step=0.0,
                          model_norms=4.3e-08, threshold=0.0, factor=5.2e-08, coef=6.8e-08),
    # 0.000e+00 0.000e+00 2.986e-08 0.000e+00 4.210e-08 0.000e+00 5.178e-08 6.706e-08
    "seg_stats": 6.2e-08,      # 6.102e-08
    "clip_coef": 4.4e-08,      # 1.237e-08 1.263e-08 3.730e-08 2.493e-08 4.388e-08
}
