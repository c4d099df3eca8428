"""Seeded cases shared by tests/test_lstm_f64.py (CPU) and tests/test_gpu_lstm_kernel.py (GPU).

Test infrastructure (not a test file).  Every case fixes seed, H, B, T, layer norm, initial state
and input scale; FP32_COST holds what float32 costs the REFERENCE (tests/lstm_f64.py evaluated in
float32 on the CPU against float64) on exactly these inputs.  The CPU file measures and checks
the figures; the GPU file derives its bounds from them (max(2e-5, 8 x figure)), so the figures
measure the reference only, never the kernel.

Why each H (csrc/lstm.hip: threads = min(1024, 4H rounded up to 64), Q = ceil(4H / threads) gate
rows per thread, kgs = threads / H k-groups in the forward product, nparts = threads / (H/4) row
groups in the backward product):
    4     64 threads, 16 k-groups of which 12 are empty, 64 row groups
    8     a single step (T = 1), with and without an initial state
    20    128 threads divide neither by 20 nor by 5: idle tail threads both ways
    64    B 33, T 200: error growth along the recurrence, more workgroups than anywhere else
    256   the C4 dims; the last H with Q = 1 and 1024 threads
    260   first Q = 2; kgs = 3 with 244 idle threads; nparts = 15
    512   the width of every reference YAML with an LSTM predictor; Q = 2 exact
    516   first Q = 3            768   Q = 3 exact
    772   first Q = 4            1024  the limit: kgs = 1, nparts = 4
    30, 1028   outside the kernel's rule (H % 4, H > 1024): the wrapper's composed device path
"""
import functools

import torch

import lstm_f64 as LF
from yardstick import FLOOR, MARGIN, bound_of, rel_err  # noqa: F401  (the rule of tests/yardstick.py)

EPS = 1e-3


def _c(seed, H, B, T, ln=True, state=False, scale=1.0, spike=0.0, kernel=True):
    return dict(seed=seed, H=H, B=B, T=T, ln=ln, state=state, scale=scale, spike=spike,
                kernel=kernel)


CASES = {
    "h4": _c(1, 4, 3, 5),
    "h8_t1": _c(2, 8, 2, 1),
    "h8_t1_state": _c(3, 8, 2, 1, state=True),
    "h20": _c(4, 20, 3, 9),
    "h20_noln": _c(5, 20, 3, 9, ln=False),
    "h20_state": _c(6, 20, 3, 9, state=True),
    "h20_b1": _c(7, 20, 1, 9, state=True),      # one workgroup: one atomic per channel (exact sums)
    "h64_long": _c(8, 64, 33, 200),
    "h256": _c(9, 256, 4, 61),
    "h256_noln": _c(10, 256, 4, 61, ln=False),
    "h256_state": _c(11, 256, 4, 61, state=True),
    "h260": _c(12, 260, 2, 7),
    "h260_b1": _c(13, 260, 1, 7),
    "h512": _c(14, 512, 3, 61),
    "h512_noln": _c(15, 512, 3, 61, ln=False),
    "h512_state": _c(16, 512, 3, 61, state=True),
    "h516": _c(17, 516, 2, 5),
    "h768": _c(18, 768, 2, 5),
    "h772": _c(19, 772, 2, 5),
    "h1024": _c(20, 1024, 2, 17),
    "h1024_noln": _c(21, 1024, 2, 17, ln=False),
    # saturated gates: without layer norm gx reaches the sigmoids / tanh directly.  scale 3, and
    # 1 % of the entries at +-60 (inside __expf's range) or +-100 (beyond it: exp overflows to inf,
    # the quotient must still come out as 0 or 1)
    "sat60": _c(22, 64, 4, 12, ln=False, scale=3.0, spike=60.0),
    "sat100": _c(23, 64, 4, 12, ln=False, scale=3.0, spike=100.0),
    # outside the kernel's rule
    "h30": _c(24, 30, 2, 3, kernel=False),
    "h30_noln": _c(25, 30, 2, 3, ln=False, kernel=False),
    "h1028": _c(26, 1028, 2, 3, kernel=False),
    "h1028_noln": _c(27, 1028, 2, 3, ln=False, kernel=False),
}
KERNEL_CASES = [k for k, v in CASES.items() if v["kernel"]]
FALLBACK_CASES = [k for k, v in CASES.items() if not v["kernel"]]

TENSORS_FWD = ("hs", "hT", "cT")
TENSORS_BWD = ("d_gx", "d_wp", "d_gg", "d_gb", "d_cg", "d_cb")


def make(name):
    """-> dict of float32 CPU tensors: gx (T,B,4H), wp (4H,H), gg, gb (4H), cg, cb (H) (None
    without layer norm), h0, c0 (B,H) or None, dhs (T,B,H)."""
    c = CASES[name]
    H, B, T = c["H"], c["B"], c["T"]
    g = torch.Generator().manual_seed(1000 + c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    t = dict(gx=rn(T, B, 4 * H) * c["scale"], wp=rn(4 * H, H) / H ** 0.5, dhs=rn(T, B, H))
    if c["spike"]:
        n = t["gx"].numel()
        idx = torch.randperm(n, generator=g)[:max(2, n // 100)]
        sign = (torch.arange(idx.numel()) % 2).float() * 2 - 1
        t["gx"].view(-1)[idx] = sign * c["spike"]
    if c["ln"]:
        t["gg"], t["gb"] = 1 + 0.2 * rn(4 * H), 0.2 * rn(4 * H)
        t["cg"], t["cb"] = 1 + 0.2 * rn(H), 0.2 * rn(H)
        for w in (t["gg"], t["cg"]):
            w[1] = 0.0                      # a channel the norm switches off
            w[2] = -0.7                     # and one it flips
    else:
        t["gg"] = t["gb"] = t["cg"] = t["cb"] = None
    t["h0"], t["c0"] = (rn(B, H), rn(B, H)) if c["state"] else (None, None)
    return t


def evaluate(t, dtype):
    """lstm_f64.lnlstm_ref forward and backward (loss = sum(hs * dhs)) on the case tensors `t`
    cast to `dtype` -> dict of the tensors named in TENSORS_FWD + TENSORS_BWD (gradients of
    absent parameters are left out)."""
    leaf = {k: (None if v is None else v.to(dtype).requires_grad_(k in ("gx", "wp", "gg", "gb", "cg", "cb")))
            for k, v in t.items()}
    hs, hT, cT = LF.lnlstm_ref(leaf["gx"], leaf["wp"], leaf["gg"], leaf["gb"], leaf["cg"],
                               leaf["cb"], EPS, leaf["h0"], leaf["c0"])
    (hs * leaf["dhs"]).sum().backward()
    out = dict(hs=hs.detach(), hT=hT.detach(), cT=cT.detach())
    for k in ("gx", "wp", "gg", "gb", "cg", "cb"):
        if leaf[k] is not None:
            out["d_" + k] = leaf[k].grad
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(make(name), torch.float64)


def fp32_figures(name):
    """(fwd, bwd): the largest rel_err over TENSORS_FWD / TENSORS_BWD of the float32 CPU
    evaluation of the reference against float64."""
    ref, f32 = reference(name), evaluate(make(name), torch.float32)
    fwd = max(rel_err(f32[k], ref[k]) for k in TENSORS_FWD)
    bwd = max(rel_err(f32[k], ref[k]) for k in TENSORS_BWD if k in ref)
    return fwd, bwd


def bound(name, kind):
    """Allowed rel_err of a device tensor of `kind` ('fwd' / 'bwd') in case `name`."""
    return bound_of(FP32_COST[name][kind])


# ------------------------------------------------------------------ measured cost of fp32
# (fwd, bwd) of fp32_figures(name).  The figure is a maximum over a tensor and moves with the order in
# which the CPU's matmul sums (up to 1.4 x between 1 and 16 threads) and with the host's vector maths
# (up to 2.9 x on another CPU): recorded is the largest value seen with 1, 4, 8 and 16 threads on one
# host, rounded up to two digits, the value itself behind; test_lstm_f64.py checks it to a factor 4.
FP32_COST = {
    "h4": dict(fwd=4.0e-07, bwd=1.1e-06),            # 3.907e-07  1.034e-06
    "h8_t1": dict(fwd=1.3e-07, bwd=2.3e-07),         # 1.231e-07  2.293e-07
    "h8_t1_state": dict(fwd=1.3e-07, bwd=1.7e-07),   # 1.249e-07  1.685e-07
    "h20": dict(fwd=1.8e-07, bwd=5.0e-07),           # 1.708e-07  4.922e-07
    "h20_noln": dict(fwd=1.5e-07, bwd=1.5e-07),      # 1.454e-07  1.469e-07
    "h20_state": dict(fwd=6.3e-07, bwd=3.6e-07),     # 6.284e-07  3.561e-07
    "h20_b1": dict(fwd=1.9e-07, bwd=3.4e-07),        # 1.849e-07  3.380e-07
    "h64_long": dict(fwd=1.6e-06, bwd=1.9e-06),      # 1.528e-06  1.875e-06
    "h256": dict(fwd=4.7e-06, bwd=4.4e-06),          # 4.626e-06  4.347e-06
    "h256_noln": dict(fwd=1.6e-07, bwd=3.3e-07),     # 1.548e-07  3.266e-07
    "h256_state": dict(fwd=2.1e-06, bwd=5.7e-06),    # 2.059e-06  5.649e-06
    "h260": dict(fwd=2.7e-07, bwd=3.5e-07),          # 2.652e-07  3.407e-07
    "h260_b1": dict(fwd=8.4e-07, bwd=3.1e-06),       # 8.355e-07  3.081e-06
    "h512": dict(fwd=1.2e-06, bwd=1.5e-06),          # 1.164e-06  1.448e-06
    "h512_noln": dict(fwd=1.6e-07, bwd=3.0e-07),     # 1.563e-07  2.972e-07
    "h512_state": dict(fwd=2.8e-06, bwd=1.8e-06),    # 2.756e-06  1.732e-06
    "h516": dict(fwd=5.0e-07, bwd=4.3e-07),          # 4.933e-07  4.218e-07
    "h768": dict(fwd=5.7e-07, bwd=4.7e-07),          # 5.694e-07  4.693e-07
    "h772": dict(fwd=5.4e-07, bwd=4.8e-07),          # 5.364e-07  4.707e-07
    "h1024": dict(fwd=1.3e-06, bwd=1.1e-06),         # 1.269e-06  1.041e-06
    "h1024_noln": dict(fwd=1.4e-07, bwd=3.6e-07),    # 1.393e-07  3.503e-07
    "sat60": dict(fwd=2.2e-07, bwd=1.5e-07),         # 2.191e-07  1.460e-07
    "sat100": dict(fwd=1.9e-07, bwd=1.8e-07),        # 1.888e-07  1.785e-07
    "h30": dict(fwd=1.3e-07, bwd=3.0e-07),           # 1.246e-07  2.913e-07
    "h30_noln": dict(fwd=1.2e-07, bwd=1.9e-07),      # 1.164e-07  1.847e-07
    "h1028": dict(fwd=3.4e-07, bwd=3.3e-07),         # 3.390e-07  3.207e-07
    "h1028_noln": dict(fwd=1.5e-07, bwd=2.3e-07),    # 1.415e-07  2.235e-07
}
