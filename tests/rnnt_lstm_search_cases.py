"""Seeded cases shared by tests/test_rnnt_lstm_search_f64.py (CPU) and
tests/test_gpu_rnnt_lstm_search.py (GPU): the searches of csrc/decode_lstm.hip.

Test infrastructure (not a test file).  A MODEL fixes the dimensions of an LSTM predictor + joiner
and the scales of its random weights; a case adds seed, batch, frames, lengths and the search's
settings.  Why each shape (the kernels tile 16 rows x 16 outputs, a lane sums k = lane, lane + 64, ...):
    h20      H 20, E 12, D 24, V 63: everything off the tiles and below one 64-chunk; 1 layer
    h20_v11  the same with V 11: a cutoff_top_k above V is taken only where V <= 16
    h48      H 48, E 32 != H, V 65, 2 layers, NO layer norm (x2g bias, identity norms), tanh, no
             out-projection
    h64      H 64, E 48, V 128, inner 256, 3 layers, tanh with out-projection
    h64o     H 64 = E, V 65, inner 24, 2 layers, no layer norm, relu with out-projection
    yaml     the dimensions of the reference's LSTM YAMLs: E = H = 512, 3 layers, D 256, V 128, inner 256
Batches of 1, 17 and 33 cross the 16-row tile; lengths are T, 0, above T (clamped) and ragged.
max_token_step 0, 1 and 10: the forced frame advance is walked in every greedy case (asserted) --
at 10 through frames whose am lifts one symbol far above the rest, which then wins until the limit
moves the frame on (the LSTM's layer norms leave no embedding direction that would make a symbol
re-emit itself, as tests/test_gpu_greedy_decode.py::_weights builds for the stateless predictor).

The margin condition admits no exclusions: every utterance of every case is decided by at least
1e-3 in float64 at every node, and the float32 CPU evaluation of the restatement gives the same
tokens (the seeds and scales were chosen on the CPU for that; tests/test_rnnt_lstm_search_f64.py
asserts both).

PRED_COST / BEAM_COST hold what float32 costs the RESTATEMENT (tests/rnnt_lstm_search_f64.py in
float32 on the CPU against float64) on exactly these inputs, in the sense of yardstick.rel_err; the
CPU file checks the figures to a factor 4 and the GPU file derives its bounds from them by the rule
of tests/yardstick.py: max(2e-5, 8 x figure).
"""
import functools

import torch

import rnnt_lstm_search_f64 as S
from yardstick import FLOOR, MARGIN as COST_MARGIN, bound_of, clamp, rel_err  # noqa: F401  (the rule of tests/yardstick.py)

EPS_IN, EPS_LSTM, EPS_OUT = 1e-5, 1e-3, 1e-5


def _m(V, E, H, D, L, ln, inner, act, scale, oscale=0.0):
    return dict(V=V, E=E, H=H, D=D, L=L, ln=ln, inner=inner, act=act, scale=scale, oscale=oscale)


MODELS = {
    "h20": _m(63, 12, 20, 24, 1, True, 24, "relu", 3.0, 8.0),
    "h20_v11": _m(11, 12, 20, 24, 1, True, 24, "relu", 3.0, 8.0),
    "h48": _m(65, 32, 48, 40, 2, False, 0, "tanh", 0.3),
    "h64": _m(128, 48, 64, 64, 3, True, 256, "tanh", 1.0, 12.0),
    "h64o": _m(65, 64, 64, 32, 2, False, 24, "relu", 3.0, 8.0),
    "yaml": _m(128, 512, 512, 256, 3, True, 256, "relu", 3.0, 8.0),
}


def weights(model, seed):
    """float32 CPU weights of MODELS[model] in the layout of rnnt_lstm_search_f64."""
    m = MODELS[model]
    V, E, H, D = m["V"], m["E"], m["H"], m["D"]
    g = torch.Generator().manual_seed(5000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    w = dict(emb=rn(V, E), in_g=1 + 0.2 * rn(E), in_b=0.2 * rn(E), layers=[],
             eps_in=EPS_IN, eps_lstm=EPS_LSTM, eps_out=EPS_OUT)
    for l in range(m["L"]):
        K = E if l == 0 else H
        p = dict(x2g_w=rn(4 * H, K) / K ** 0.5, wp=rn(4 * H, H) / H ** 0.5)
        if m["ln"]:
            p.update(gg=1 + 0.2 * rn(4 * H), gb=0.2 * rn(4 * H), cg=1 + 0.2 * rn(H), cb=0.2 * rn(H))
        else:
            p["x2g_b"] = 0.3 * rn(4 * H)
        w["layers"].append(p)
    s = m["scale"]
    w.update(lin_w=rn(D, H) / H ** 0.5 * 3.0, lin_b=0.1 * rn(D), out_g=1 + 0.2 * rn(D), out_b=0.2 * rn(D),
             pre_w=s * rn(V, D) / D ** 0.5, pre_b=0.1 * s * rn(V))
    if m["inner"]:
        o = m["oscale"]
        w.update(o1_w=rn(m["inner"], V) / V ** 0.5, o1_b=0.1 * rn(m["inner"]),
                 o2_w=o * rn(V, m["inner"]) / m["inner"] ** 0.5, o2_b=0.1 * o * rn(V))
    return w


def _c(model, seed, B, T, mts=None, beam=None, topk=None, lift=0.0, blank=1.3):
    return dict(model=model, seed=seed, B=B, T=T, mts=mts, beam=beam, topk=topk, lift=lift, blank=blank)


# lift: am of one symbol on one frame per utterance raised by lift x scale (walks max_token_step)
GREEDY_CASES = {
    "g_h20_b1": _c("h20", 3, 1, 9, mts=1),
    "g_h48_b17_mts10": _c("h48", 4, 17, 7, mts=10, lift=8.0),
    "g_h64_b33_mts0": _c("h64", 0, 33, 5, mts=0),
    "g_h64o_b3_t40": _c("h64o", 0, 3, 40, mts=1),
    "g_yaml": _c("yaml", 0, 4, 24, mts=1),
}
BEAM_CASES = {
    "b_h20_beam1_k1": _c("h20", 0, 3, 9, beam=1, topk=1),
    "b_h20v11_beam16_kV": _c("h20_v11", 0, 2, 8, beam=16, topk=20),
    "b_h48_b17_beam4": _c("h48", 6, 17, 3, beam=4, topk=4, blank=0.7),
    "b_h64_beam16_k4": _c("h64", 0, 2, 6, beam=16, topk=4),
    "b_h64o_b33_beam4_k1": _c("h64o", 0, 33, 4, beam=4, topk=1),
    "b_yaml": _c("yaml", 0, 4, 24, beam=4, topk=4),
}
CASES = dict(GREEDY_CASES, **BEAM_CASES)


def make(name):
    """-> (weights, act, am (B,T,V) float32, lengths (B) int64; some 0, some above T)."""
    c = CASES[name]
    m = MODELS[c["model"]]
    w = weights(c["model"], c["seed"])
    B, T, V, s = c["B"], c["T"], m["V"], m["scale"]
    g = torch.Generator().manual_seed(7000 + c["seed"])
    am = s * torch.randn(B, T, V, generator=g)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = T + 3
    spread = (2 * torch.log(torch.tensor(float(V)))) ** 0.5
    if m["inner"]:
        # the blank bias sits behind the out-projection: blank wins about every other node
        w["o2_b"][0] += c["blank"] * spread * m["oscale"] * (0.6 if m["act"] == "tanh" else 0.8 * s)
    else:
        am[:, :, 0] += c["blank"] * spread * s * 0.5
    if c["lift"]:
        for b in range(B):
            am[b, (b + 1) % T, 1 + b % 2] += c["lift"] * s
    return w, m["act"], am, lens


def evaluate(name, dtype):
    """The restatement on a case with the weights in `dtype` -> per utterance, greedy: (tokens,
    margin, forced); beam: (tokens, score, frames, margin)."""
    c = CASES[name]
    w, act, am, lens = make(name)
    w = S.cast(w, dtype)
    out = []
    for b in range(c["B"]):
        a = am[b, :clamp(lens[b], c["T"])]
        if c["beam"] is None:
            out.append(S.greedy(a, w, act, c["mts"]))
        else:
            out.append(S.beam_search(a, w, act, c["beam"], c["topk"]))
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


# ------------------------------------------------------------------ the predictor step on its own
PRED_ROWS = 19                                       # across the 16-row tile
PRED_MODELS = ["h20", "h48", "h64", "yaml"]


def pred_schedule(model):
    """Five chained masked steps on PRED_ROWS rows: [(tokens, emit, parent)] int64 CPU tensors --
    all rows, alternating rows under a non-identity permutation, none under it, the other
    alternation, all under the permutation."""
    R = PRED_ROWS
    g = torch.Generator().manual_seed(9000 + MODELS[model]["H"])
    ident = torch.arange(R)
    perm = torch.roll(ident, 5)
    perm[3] = perm[4]                                # two rows share a parent, as beams do
    alt = (ident % 2 == 0).long()
    masks = [(torch.ones(R, dtype=torch.int64), ident), (alt, perm),
             (torch.zeros(R, dtype=torch.int64), perm), (1 - alt, ident),
             (torch.ones(R, dtype=torch.int64), perm)]
    return [(torch.randint(0, MODELS[model]["V"], (R,), generator=g), e, p) for e, p in masks]


def pred_chain(model, dtype):
    """-> [(lm, [(h, c)])] after each of the five steps, from zero state and zero lm."""
    w = S.cast(weights(model, 100), dtype)
    state = S.zero_state(w, PRED_ROWS)
    lm = w["emb"].new_zeros(PRED_ROWS, MODELS[model]["V"])
    out = []
    with torch.no_grad():
        for tokens, emit, parent in pred_schedule(model):
            lm, state = S.masked_step(w, tokens, emit, parent, state, lm)
            out.append((lm, state))
    return out


def pred_tensors(step):
    lm, state = step
    return [lm] + [t for hc in state for t in hc]


def pred_fp32_figure(model):
    ref, f32 = pred_chain(model, torch.float64), pred_chain(model, torch.float32)
    return max(rel_err(a, b) for i in (0, 4) for a, b in zip(pred_tensors(f32[i]), pred_tensors(ref[i])))


def beam_fp32_figure(name):
    ref, f32 = reference(name), evaluate(name, torch.float32)
    return rel_err(torch.tensor([r[1] for r in f32]), torch.tensor([r[1] for r in ref]))


def bound(figure):
    """Allowed rel_err of a device tensor whose float32 cost in the restatement is `figure`."""
    return bound_of(figure)


# ------------------------------------------------------------------ measured cost of fp32
# The largest value seen with 1, 4, 8 and 16 host threads, rounded up to two digits, the value
# itself behind (the rule of tests/yardstick.py).
PRED_COST = {
    "h20": 3.6e-07,                     # 3.550e-07
    "h48": 2.9e-07,                     # 2.821e-07
    "h64": 1.4e-06,                     # 1.392e-06
    "yaml": 3.8e-06,                    # 3.765e-06
}
BEAM_COST = {
    "b_h20_beam1_k1": 3.4e-06,          # 3.340e-06
    "b_h20v11_beam16_kV": 1.1e-05,      # 1.013e-05
    "b_h48_b17_beam4": 8.9e-08,         # 8.838e-08
    "b_h64_beam16_k4": 5.8e-06,         # 5.703e-06
    "b_h64o_b33_beam4_k1": 6.1e-06,     # 6.015e-06
    "b_yaml": 4.2e-06,                  # 4.128e-06
}
