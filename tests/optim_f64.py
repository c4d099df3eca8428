"""Independent restatement of the optimizers of csrc/optim.hip, per tensor, in plain torch.

Test infrastructure (not a test file).  Written from the reference's optimizer/scaled_adam.py
(_get_clipping_scale :408-527, _step_one_batch / _size_update / _step / _step_scalar :563-736) and
from torch's documented Adam / AdamW + clip_grad_norm_; it uses neither FlatStore nor
ScaledAdam._step_torch.  The arithmetic dtype is an argument: float64 is the reference the device
and the host forms are held to, float32 measures what fp32 costs that reference on the same inputs
(tests/optim_cases.py FP32_COST).

On top of the reference's rules it states the project's additions, as the code comments give them:
  * the trainer's clip: every gradient of the store is scaled by min(1, clip / (norm + 1e-6)), norm
    over EVERY tensor of the store; a NaN norm leaves the factor at 1 (the device's fminf; torch's
    clamp would keep the NaN);
  * once a clipping threshold exists, non-finite scaled gradients are set to 0 (the reference zeroes
    all gradients when its factor is 0, which is the only way they arise);
  * a trainable tensor that no group lists is never updated, its gradient is only cleared;
  * a dropped step: the count advances, parameters and moments stay, the (p . g) sample of the step
    is 0, model_norms[k % period] repeats model_norms[(k - 1) % period] for k > 0, gradients are
    cleared.
Per-tensor state the reference keeps only for tensors of more than one element (param_rms,
scale_exp_avg_sq, scale_grads) is kept for one-element tensors too, as the device does; it never
reaches their parameters.

Every discrete decision is reported with its margin (`margins`), in the units the fp32 figures of
optim_cases.py use, so that a case can be shown not to sit on a branch point.
"""
import torch

IRREGULAR = (10, 20, 40)
SA_DEFAULTS = dict(lr=3e-2, clipping_scale=None, betas=(0.9, 0.98), scalar_lr_scale=0.1, eps=1e-8,
                   param_min_rms=1e-5, param_max_rms=3.0, scalar_max=10.0, size_update_period=4,
                   clipping_update_period=100)


def _finite_max(x):
    x = x[torch.isfinite(x)].abs()
    return float(x.max()) if x.numel() else 0.0


def clip_factor(sumsq, clip):
    """The trainer's clip factor from the store's total sum of squared gradients (0-d tensor)."""
    if not clip:
        return torch.ones((), dtype=sumsq.dtype)
    r = clip / (sumsq.sqrt() + 1.0e-6)
    if bool(r != r):
        return torch.ones((), dtype=sumsq.dtype)
    return torch.clamp(r, max=1.0)


def median_of(model_norms, k, period):
    """The reference's threshold statistic (:449-458): sorted ascending with NaN last, the last k
    entries on an irregular step, element min(num - 1, (num // 4) * 2).
    -> (median, gap, tied): gap is the distance from the median to the nearest entry of the sorted
    window with another value (inf if there is none), tied says whether a sorted neighbour has
    exactly the median's value (then either may be picked: the value is the same)."""
    srt = torch.sort(model_norms)[0]
    if k in IRREGULAR and k < period:
        srt = srt[-k:]
    num = srt.numel()
    mi = min(num - 1, (num // 4) * 2)
    med = srt[mi]
    tied = any(0 <= j < num and bool(srt[j] == med) for j in (mi - 1, mi + 1))
    other = srt[torch.isfinite(srt) & (srt != med)]
    gap = float((other - med).abs().min()) if other.numel() and bool(torch.isfinite(med)) \
        else float("inf")
    return med, gap, tied


def group_coef(G, k, c, gg, pg, pp, lens, margins):
    """One group's per-step decisions from its per-tensor sums gg = sum g^2, pg = sum p g,
    pp = sum p^2 of the UNCLIPPED gradients (1-D, one entry per tensor) and the trainer's factor c.
    Updates the group state G in place and returns (gm, sanitize, scale_step, coef, bc, lim): the
    gradient factor, whether non-finite scaled gradients become 0, and per tensor the learned-scale
    step, the Adam step coefficient, the divisor of exp_avg_sq and the parameter limit."""
    h = G["h"]
    dt = gg.dtype
    lr, slr, eps = h["lr"], h["scalar_lr_scale"], h["eps"]
    beta1, beta2 = h["betas"]
    P, period, cs = h["size_update_period"], h["clipping_update_period"], h["clipping_scale"]
    scalar = lens == 1
    n = lens.numel()
    ans = torch.ones((), dtype=dt)
    sanitize = False
    if cs is not None and k > 0:
        w = torch.where(scalar, torch.full((n,), slr * slr, dtype=dt), G["param_rms"] ** 2)
        tot_norm = ((c * c) * gg * w).sum().sqrt()
        mn = G["model_norms"]
        mn[k % period] = tot_norm
        G["last_norm"] = tot_norm.clone()
        irregular = k in IRREGULAR and k < period
        if k % period == 0 or irregular:
            med, gap, tied = median_of(mn, k, period)
            if not bool(torch.isfinite(med)):
                raise RuntimeError("Too many grads were not finite")
            G["threshold"] = cs * med * (2.0 if irregular else 1.0)
            G["num_clipped"] = 0
            margins.append(dict(kind="median", q="model_norms", step=k, tied=tied,
                                margin=gap / max(_finite_max(mn), 1e-300)))
        if G["threshold"] is not None:
            r = G["threshold"] / (tot_norm + 1.0e-20)
            ans = torch.zeros((), dtype=dt) if bool(r != r) else torch.clamp(r, max=1.0)
            if bool(torch.isfinite(tot_norm)):
                margins.append(dict(kind="ans<1", q="model_norms", step=k, taken=bool(ans < 1.0),
                                    margin=float((G["threshold"] - tot_norm).abs())
                                    / max(_finite_max(mn), 1e-300)))
            if bool(ans < 1.0):
                G["num_clipped"] += 1
            sanitize = True
    gm = c * ans
    G["last_factor"] = gm.clone()
    G["scale_grads"][k % P] = torch.zeros(n, dtype=dt) if (sanitize and bool(gm == 0)) else gm * pg
    sstep = torch.zeros(n, dtype=dt)
    if k % P == P - 1:
        rms = (pp / lens.to(dt)).sqrt()
        G["param_rms"] = rms
        if k > 0:
            sg = G["scale_grads"]
            beta2c = beta2 ** P
            seas = G["scale_exp_avg_sq"] * beta2c + (1 - beta2c) * (sg * sg).mean(dim=0)
            G["scale_exp_avg_sq"] = seas
            bc2_size = 1 - beta2c ** ((k + 1) // P)
            st = -(lr * slr) * (bc2_size ** 0.5) * sg.sum(dim=0) / (seas.sqrt() + eps)
            small = rms < h["param_min_rms"]
            cap = (h["param_max_rms"] - rms) / rms
            many = ~scalar
            if bool(many.any()):
                # relative: every tensor's rms is a quantity of its own (optim_cases.rel_each)
                margins.append(dict(kind="rms<min", q="param_rms", step=k, taken=int(small[many].sum()),
                                    margin=float(((rms - h["param_min_rms"]).abs() / rms)[many].min())))
                live = many & ~small
                st0 = torch.where(small, torch.zeros_like(st), st)
                margins.append(dict(kind="max_rms cap", q="scale_step", step=k,
                                    taken=int((cap < st0)[live].sum()),
                                    margin=float((st0 - cap).abs()[live].min())
                                    / max(_finite_max(torch.minimum(st0, cap)[many]), 1e-300)))
            st = torch.where(small, torch.zeros_like(st), st)
            st = torch.minimum(st, cap)
            sstep = torch.where(scalar, torch.zeros_like(st), st)
    G["scale_step"] = sstep
    coef = torch.where(scalar, torch.full((n,), -lr * slr * (1 - beta1), dtype=dt),
                       -lr * (1 - beta1) * G["param_rms"].clamp(min=h["param_min_rms"]))
    bc2 = 1 - beta2 ** (k + 1)
    # bc2 is host arithmetic in double on both sides; the kernel compares it as a float
    margins.append(dict(kind="bc2<0.99", q="eps32", step=k, taken=bc2 < 0.99, margin=abs(bc2 - 0.99)))
    bc = torch.where(scalar, torch.full((n,), bc2, dtype=dt),
                     torch.full((n,), bc2 if bc2 < 0.99 else 1.0, dtype=dt))
    lim = torch.where(scalar, torch.full((n,), h["scalar_max"], dtype=dt),
                      torch.full((n,), float("inf"), dtype=dt))
    return gm, sanitize, sstep, coef, bc, lim


class ScaledAdamRef:
    """tensors: every trainable tensor of the store, in store order.  groups: list of dicts with
    `idx` (indices into tensors) and any of SA_DEFAULTS.  State is public: p, delta, exp_avg_sq,
    grad (lists over the store's tensors; None for delta / exp_avg_sq of an ungrouped tensor), and
    per group (self.groups[i]) param_rms, scale_exp_avg_sq, scale_grads, scale_step, model_norms,
    threshold, num_clipped, step."""

    def __init__(self, tensors, groups, dtype=torch.float64, pre_clip=None, zero_grad=True):
        self.dtype, self.pre_clip, self.zero_grad = dtype, pre_clip, zero_grad
        self.p = [t.detach().to(dtype).clone() for t in tensors]
        self.delta = [None] * len(tensors)
        self.exp_avg_sq = [None] * len(tensors)
        self.grad = [torch.zeros_like(t) for t in self.p]
        self.margins = []
        self.groups = []
        for g in groups:
            h = dict(SA_DEFAULTS)
            h.update({k: v for k, v in g.items() if k != "idx"})
            idx = list(g["idx"])
            n = len(idx)
            for i in idx:
                self.delta[i] = torch.zeros_like(self.p[i])
                self.exp_avg_sq[i] = torch.zeros_like(self.p[i])
            self.groups.append(dict(
                h=h, idx=idx, step=0, lens=torch.tensor([self.p[i].numel() for i in idx]),
                param_rms=torch.stack([(self.p[i] ** 2).mean().sqrt() for i in idx]),
                scale_exp_avg_sq=torch.zeros(n, dtype=dtype),
                scale_grads=torch.zeros(h["size_update_period"], n, dtype=dtype),
                scale_step=torch.zeros(n, dtype=dtype),
                model_norms=torch.zeros(h["clipping_update_period"], dtype=dtype),
                threshold=None, num_clipped=0, last_norm=None, last_factor=None))

    def step(self, grads, skip=False):
        dt = self.dtype
        g = [x.detach().to(dt).clone() for x in grads]
        if skip:
            for G in self.groups:
                k, h = G["step"], G["h"]
                G["scale_grads"][k % h["size_update_period"]] = 0
                if h["clipping_scale"] is not None and k > 0:
                    period = h["clipping_update_period"]
                    G["model_norms"][k % period] = G["model_norms"][(k - 1) % period]
                G["step"] = k + 1
        else:
            sumsq = torch.stack([(x * x).sum() for x in g]).sum()
            c = clip_factor(sumsq, self.pre_clip)
            for G in self.groups:
                self._group_step(G, g, c)
        self.grad = [torch.zeros_like(x) for x in g] if self.zero_grad else g

    def _group_step(self, G, g, c):
        h, k, idx = G["h"], G["step"], G["idx"]
        beta1, beta2 = h["betas"]
        p = self.p
        gg = torch.stack([(g[i] * g[i]).sum() for i in idx])
        pg = torch.stack([(p[i] * g[i]).sum() for i in idx])
        pp = torch.stack([(p[i] * p[i]).sum() for i in idx])
        gm, sanitize, sstep, coef, bc, lim = group_coef(G, k, c, gg, pg, pp, G["lens"], self.margins)
        clamp_margin, clamped = float("inf"), 0
        for j, i in enumerate(idx):
            gi = g[i] * gm
            if sanitize:
                gi = torch.nan_to_num(gi, nan=0.0, posinf=0.0, neginf=0.0)
            d = self.delta[i] * beta1 + (1 - beta1) * (p[i] * sstep[j])
            e = self.exp_avg_sq[i] * beta2 + (1 - beta2) * (gi * gi)
            d = d + gi / ((e / bc[j]).sqrt() + h["eps"]) * coef[j]
            if p[i].numel() == 1:
                a = float(p[i].abs().max())
                if a == a:
                    clamp_margin = min(clamp_margin, abs(a - h["scalar_max"]))
                    clamped += int(a > h["scalar_max"])
                p[i] = torch.clamp(p[i], min=-h["scalar_max"], max=h["scalar_max"])
            p[i] = p[i] + d
            self.delta[i], self.exp_avg_sq[i], g[i] = d, e, gi
        if clamp_margin < float("inf"):
            pmax = max(_finite_max(x) for x in p)
            self.margins.append(dict(kind="scalar clamp", q="p", step=k, taken=clamped,
                                     margin=clamp_margin / max(pmax, 1e-300)))
        G["step"] = k + 1


class AdamRef:
    """torch.optim.Adam (decoupled=False) / AdamW (decoupled=True) as documented, amsgrad off, plus
    clip_grad_norm_ over every tensor of the store (NaN norm: factor 1), the ungrouped tensor and
    the dropped step (one shared count, which advances; nothing else moves).  groups: dicts with
    `idx`, lr, betas, eps, weight_decay."""

    def __init__(self, tensors, groups, decoupled, dtype=torch.float64, pre_clip=None,
                 zero_grad=True):
        self.dtype, self.pre_clip, self.zero_grad, self.decoupled = dtype, pre_clip, zero_grad, decoupled
        self.p = [t.detach().to(dtype).clone() for t in tensors]
        self.exp_avg = [None] * len(tensors)
        self.exp_avg_sq = [None] * len(tensors)
        self.grad = [torch.zeros_like(t) for t in self.p]
        self.groups = [dict(g) for g in groups]
        self.step_count = 0
        for g in self.groups:
            for i in g["idx"]:
                self.exp_avg[i] = torch.zeros_like(self.p[i])
                self.exp_avg_sq[i] = torch.zeros_like(self.p[i])

    def step(self, grads, skip=False):
        dt = self.dtype
        g = [x.detach().to(dt).clone() for x in grads]
        self.step_count += 1
        k = self.step_count
        if not skip:
            c = clip_factor(torch.stack([(x * x).sum() for x in g]).sum(), self.pre_clip)
            for G in self.groups:
                lr, (b1, b2), eps, wd = G["lr"], G["betas"], G["eps"], G["weight_decay"]
                bc1, bc2 = 1 - b1 ** k, 1 - b2 ** k
                for i in G["idx"]:
                    gi, pi = g[i] * c, self.p[i]
                    if self.decoupled:
                        pi = pi * (1 - lr * wd)
                    else:
                        gi = gi + wd * pi
                    m = self.exp_avg[i] + (1 - b1) * (gi - self.exp_avg[i])
                    v = self.exp_avg_sq[i] * b2 + (1 - b2) * gi * gi
                    denom = v.sqrt() / (bc2 ** 0.5) + eps
                    self.p[i] = pi - (lr / bc1) * m / denom
                    self.exp_avg[i], self.exp_avg_sq[i], g[i] = m, v, g[i] * c
        self.grad = [torch.zeros_like(x) for x in g] if self.zero_grad else g
