"""Seeded cases shared by tests/test_rnn_lm_f64.py (CPU) and tests/test_gpu_lstm_step_kernel.py
(GPU), in the style of tests/lstm_cases.py.

Test infrastructure (not a test file).  Every case fixes seed, H, B, T, initial state and input
scale.  The float64 reference is tests/rnn_lm_f64.lstm_ref; FP32_COST holds what float32 costs the
REFERENCE -- torch.nn.LSTM in float32 on the CPU against that float64 -- on exactly these inputs
(gx enters nn.LSTM through an identity weight_ih and zero biases, which is exact).  The CPU file
measures and checks the figures; the GPU file derives its bounds from them (max(2e-5, 8 x figure),
the rule of tests/yardstick.py), so the figures measure the reference only, never the kernel.

Why each shape (csrc/lstm_step.hip: a workgroup owns HS = 16 hidden units and BT = 16 utterances,
grid = ceil(H / 16) x ceil(B / 16); a wave walks K = H in chunks of 64 = four 16-wide sub-chunks on
four accumulators, a lane's float4 of a sub-chunk is masked when it starts at or beyond K):
    B  1, 15   one partial batch tile           16   one exact tile
       17, 35  a full tile and a partial one (two / three workgroups along the batch)
    H  4       one slice with 12 idle units, K a quarter of ONE sub-chunk
       20      two slices, the second with 4 units; K = 16 + 4: a whole and a partial sub-chunk
       64      four exact slices, exactly one 64-chunk
       260     17 slices, the last with 4 units; K = 4 x 64 + 4
       512     the YAML width: 32 slices, 8 chunks           1024   the limit of the rule
    T  1       a single launch: no previous step on either walk (NULL h / dgates)
       2       one step with and one without a predecessor         9   a chain
    h64_long   T = 200 at B = 33: error growth along the recurrence
    *_state    h0 / c0 given (the forward's first step then has a product, the backward's last
               step a c_{t-1} that is not a cell of the sequence)
    sat60 / sat100   saturated gates: input scale 3 and 1 % of the entries at +-60 (inside
               __expf's range) / +-100 (beyond it: exp overflows to inf and the quotient must
               still come out as 0 or 1)
    thr_at     B = THRESHOLD through the wrapper's own dispatch: the step kernel.  The measured
               threshold is 1 (the step kernel is the faster one at every batch), so no batch lies
               below it;
    seq_kernel the wrapper's small-batch branch with the threshold raised above B = 15: the
               per-utterance kernel of csrc/lstm.hip with NULL norms, which the dispatch keeps
    h30, h1028 outside the rule (H % 4 != 0, H > 1024): the composed device path
"""
import functools

import torch

import rnn_lm_f64 as RF
from yardstick import FLOOR, MARGIN, bound_of, rel_err  # noqa: F401  (the rule of tests/yardstick.py)

THRESHOLD = 1          # conf_kernels.LSTM_STEP_MIN_BATCH the cases were laid out for (the GPU file
#                        asserts that they agree)


def _c(seed, H, B, T, state=False, scale=1.0, spike=0.0, path="step"):
    """path: 'step' = the step kernel with the threshold pinned to 1, 'auto' = the wrapper's own
    dispatch, 'seq' = the threshold raised above B, 'composed' = outside the rule."""
    return dict(seed=seed, H=H, B=B, T=T, state=state, scale=scale, spike=spike, path=path)


CASES = {
    "h4_b1_t1": _c(1, 4, 1, 1),
    "h4_b1_t1_state": _c(2, 4, 1, 1, state=True),
    "h20_b15_t2": _c(3, 20, 15, 2, state=True),
    "h20_b35_t9": _c(4, 20, 35, 9),
    "h64_b16_t9": _c(5, 64, 16, 9),
    "h64_b17_t2": _c(6, 64, 17, 2),
    "h260_b17_t9": _c(7, 260, 17, 9, state=True),
    "h260_b1_t9": _c(8, 260, 1, 9),
    "h512_b35_t9": _c(9, 512, 35, 9),
    "h512_b16_t9_state": _c(10, 512, 16, 9, state=True),
    "h1024_b17_t2": _c(11, 1024, 17, 2),
    "h1024_b15_t9": _c(12, 1024, 15, 9, state=True),
    "h64_long": _c(13, 64, 33, 200),
    "sat60": _c(14, 64, 17, 12, scale=3.0, spike=60.0),
    "sat100": _c(15, 64, 17, 12, scale=3.0, spike=100.0),
    "seq_kernel": _c(16, 64, 15, 5, state=True, path="seq"),
    "thr_at": _c(17, 64, THRESHOLD, 5, state=True, path="auto"),
    "h30": _c(18, 30, 17, 3, path="composed"),
    "h1028": _c(19, 1028, 17, 3, state=True, path="composed"),
}
STEP_CASES = [k for k, v in CASES.items() if v["path"] == "step"]
AUTO_CASES = [k for k, v in CASES.items() if v["path"] == "auto"]
SEQ_CASES = [k for k, v in CASES.items() if v["path"] == "seq"]
COMPOSED_CASES = [k for k, v in CASES.items() if v["path"] == "composed"]

TENSORS_FWD = ("hs", "hT", "cT")
TENSORS_BWD = ("d_gx", "d_whh")


def make(name):
    """-> dict of float32 CPU tensors: gx (T,B,4H), whh (4H,H), h0, c0 (B,H) or None, dhs (T,B,H)."""
    c = CASES[name]
    H, B, T = c["H"], c["B"], c["T"]
    g = torch.Generator().manual_seed(2000 + c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    t = dict(gx=rn(T, B, 4 * H) * c["scale"], whh=rn(4 * H, H) / H ** 0.5, dhs=rn(T, B, H))
    if c["spike"]:
        n = t["gx"].numel()
        idx = torch.randperm(n, generator=g)[:max(2, n // 100)]
        sign = (torch.arange(idx.numel()) % 2).float() * 2 - 1
        t["gx"].view(-1)[idx] = sign * c["spike"]
    t["h0"], t["c0"] = (rn(B, H), rn(B, H)) if c["state"] else (None, None)
    return t


def _pack(hs, hT, cT, gx, whh):
    return dict(hs=hs.detach(), hT=hT.detach(), cT=cT.detach(), d_gx=gx.grad, d_whh=whh.grad)


def evaluate(t, dtype):
    """rnn_lm_f64.lstm_ref forward and backward (loss = sum(hs * dhs)) on the case tensors cast to
    `dtype` -> dict of the tensors named in TENSORS_FWD + TENSORS_BWD."""
    v = {k: (None if x is None else x.to(dtype)) for k, x in t.items()}
    gx, whh = v["gx"].requires_grad_(True), v["whh"].requires_grad_(True)
    hs, hT, cT = RF.lstm_ref(gx, whh, v["h0"], v["c0"])
    (hs * v["dhs"]).sum().backward()
    return _pack(hs, hT, cT, gx, whh)


def evaluate_nn_lstm(t, dtype):
    """The same through torch.nn.LSTM: gx is its input, weight_ih the identity and the biases zero
    (x I + 0 is exact in any float format), weight_hh the case's."""
    H = t["whh"].shape[1]
    m = torch.nn.LSTM(4 * H, H, 1).to(dtype)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(4 * H))
        m.weight_hh_l0.copy_(t["whh"])
        m.bias_ih_l0.zero_()
        m.bias_hh_l0.zero_()
    gx = t["gx"].to(dtype).requires_grad_(True)
    B = gx.shape[1]
    h0 = torch.zeros(B, H) if t["h0"] is None else t["h0"]
    c0 = torch.zeros(B, H) if t["c0"] is None else t["c0"]
    hs, (hT, cT) = m(gx, (h0.to(dtype)[None], c0.to(dtype)[None]))
    (hs * t["dhs"].to(dtype)).sum().backward()
    return _pack(hs, hT[0], cT[0], gx, m.weight_hh_l0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(make(name), torch.float64)


def fp32_figures(name):
    """(fwd, bwd): the largest rel_err over TENSORS_FWD / TENSORS_BWD of torch.nn.LSTM in float32
    on the CPU against the float64 reference."""
    ref, f32 = reference(name), evaluate_nn_lstm(make(name), torch.float32)
    return (max(rel_err(f32[k], ref[k]) for k in TENSORS_FWD),
            max(rel_err(f32[k], ref[k]) for k in TENSORS_BWD))


def bound(name, kind):
    """Allowed rel_err of a device tensor of `kind` ('fwd' / 'bwd') in case `name`."""
    return bound_of(FP32_COST[name][kind])


# ------------------------------------------------------------------ measured cost of fp32
# (fwd, bwd) of fp32_figures(name): the largest value seen with 1, 4 and 16 threads on one host,
# rounded up to two digits, the value itself behind.  The figure is a maximum over a tensor and
# moves with the order in which the CPU's matmul sums and with the host's vector maths (lstm_cases
# saw up to 2.9 x between hosts): test_rnn_lm_f64.py checks it to a factor 4.
FP32_COST = {
    "h4_b1_t1":              dict(fwd=1.4e-07, bwd=9.7e-08),    # 1.340e-07  9.694e-08
    "h4_b1_t1_state":        dict(fwd=4.7e-08, bwd=1.8e-07),    # 4.621e-08  1.785e-07
    "h20_b15_t2":            dict(fwd=1.1e-07, bwd=3.3e-07),    # 1.052e-07  3.261e-07
    "h20_b35_t9":            dict(fwd=1.6e-07, bwd=3.8e-07),    # 1.568e-07  3.740e-07
    "h64_b16_t9":            dict(fwd=1.5e-07, bwd=4.2e-07),    # 1.464e-07  4.156e-07
    "h64_b17_t2":            dict(fwd=1.2e-07, bwd=2.1e-07),    # 1.171e-07  2.062e-07
    "h260_b17_t9":           dict(fwd=4.7e-07, bwd=3.6e-07),    # 4.602e-07  3.534e-07
    "h260_b1_t9":            dict(fwd=4.3e-07, bwd=3.9e-07),    # 4.267e-07  3.883e-07
    "h512_b35_t9":           dict(fwd=2.5e-07, bwd=6.0e-07),    # 2.423e-07  5.942e-07
    "h512_b16_t9_state":     dict(fwd=6.6e-07, bwd=4.7e-07),    # 6.548e-07  4.672e-07
    "h1024_b17_t2":          dict(fwd=1.7e-07, bwd=2.6e-07),    # 1.607e-07  2.558e-07
    "h1024_b15_t9":          dict(fwd=9.0e-07, bwd=5.4e-07),    # 8.951e-07  5.339e-07
    "h64_long":              dict(fwd=1.8e-07, bwd=3.5e-07),    # 1.755e-07  3.461e-07
    "sat60":                 dict(fwd=2.2e-07, bwd=4.8e-07),    # 2.161e-07  4.731e-07
    "sat100":                dict(fwd=2.1e-07, bwd=3.9e-07),    # 2.035e-07  3.827e-07
    "seq_kernel":            dict(fwd=2.0e-07, bwd=2.8e-07),    # 1.986e-07  2.745e-07
    "thr_at":                dict(fwd=3.3e-07, bwd=2.2e-07),    # 3.210e-07  2.120e-07
    "h30":                   dict(fwd=1.6e-07, bwd=2.6e-07),    # 1.547e-07  2.569e-07
    "h1028":                 dict(fwd=8.0e-07, bwd=6.1e-07),    # 7.903e-07  6.074e-07
}
