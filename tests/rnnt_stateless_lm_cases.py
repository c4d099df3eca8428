"""Seeded cases shared by tests/test_rnnt_stateless_lm_f64.py (CPU) and
tests/test_gpu_rnnt_stateless_lm.py (GPU): the RNN-T beam search with RNN-LM shallow fusion over the
stateless predictor (csrc/decode_lstm.hip s2t_rnnt_beam_stateless_lm, s2t_stateless_pred_step).

Test infrastructure (not a test file).  The construction is rnnt_lm_fusion_cases.stateless_case's
(generator seed 9000 + seed: the predictor / joiner weights, then am with the blank lifted, then ragged
lengths, then the out-projection when there is one), the language models are that file's LM_MODELS
with lm_weights(model, seed).  Why each shape (the step's row kernel sums the depthwise window over k = 0
.. ctx - 1 per embedding channel, 256 channels per pass; the two products tile 16 rows x 16 outputs, a
lane sums k = lane, lane + 64, ...):
    s_b1_ctx1_beam1_k1       ctx 1 (nothing to shift), B 1, beam 1 / top-k 1: the LM cannot change the path,
                             lm_score must still be right; V 63, E 12, D 20: everything off the tiles
    s_v11_beam16_kV          V 11, beam 16, top-k 20 >= V; ctx 2; D 24
    s_b17_ctx5_e65           B 17 (R 68: five row tiles, the last one partial), T 3, ctx 5, E 65: one lane
                             past the 64-lane stride of the first product
    s_b33_ctx2_v65           B 33 (R 132), T 4, V 65
    s_v128_e130_beam16_start V 128, E 130: two 64-chunks and a tail; D 40; beam 16 / top-k 4; start token 127
    s_inner_v65              the joint through the two out-projection Linears (inner 24), relu
    s_yaml                   the dimensions of zipformer_stateless_pruned_rnnt.yaml and the rnn_lm.yaml LM:
                             V 128, E 512, D 256, ctx 5; B 4, T 12
Lengths are T, 0, above T (clamped) and ragged.

The conditions, with no exclusions (tests/test_rnnt_stateless_lm_f64.py asserts them; the seeds were
chosen on the CPU for them): every utterance of every case is decided by at least 1e-3
(rnnt_lstm_search_f64.MARGIN) at every node in float64; the float32 CPU run of the restatement walks
the same tokens and frames; in every case with beam > 1 the LM changes at least one utterance's tokens
against lm_weight = 0.

STEP_COST / FUSED_COST hold what float32 costs the RESTATEMENT (tests/rnnt_stateless_lm_f64.py in float32
on the CPU against float64) on exactly these inputs, in the sense of yardstick.rel_err; the GPU bounds
are max(2e-5, 8 x figure), the rule of tests/yardstick.py.
"""
import functools

import torch

import rnnt_lm_fusion_cases as L
import rnnt_lstm_search_cases as C
import rnnt_stateless_lm_f64 as SF
from yardstick import rel_err  # noqa: F401  (the rule of tests/yardstick.py)

bound = C.bound
clamp = C.clamp
LM_MODELS = L.LM_MODELS
lm_weights = L.lm_weights


def _s(seed, B, T, V, E, D, ctx, beam, topk, lm, weight=0.5, start=None, inner=0, act="relu", scale=3.0,
       oscale=8.0, blank=1.3):
    return dict(seed=seed, B=B, T=T, V=V, E=E, D=D, ctx=ctx, beam=beam, topk=topk, lm=lm, weight=weight,
                start=start, inner=inner, act=act, scale=scale, oscale=oscale, blank=blank)


CASES = {
    "s_b1_ctx1_beam1_k1": _s(0, 1, 9, 63, 12, 20, 1, 1, 1, "lm20", weight=0.3),
    "s_v11_beam16_kV": _s(0, 3, 8, 11, 12, 24, 2, 16, 20, "lm20_v11"),
    "s_b17_ctx5_e65": _s(1, 17, 3, 63, 65, 20, 5, 4, 4, "lm20"),
    "s_b33_ctx2_v65": _s(0, 33, 4, 65, 12, 20, 2, 4, 4, "lm48"),
    "s_v128_e130_beam16_start": _s(0, 2, 6, 128, 130, 40, 5, 16, 4, "lm64", start=127),
    "s_inner_v65": _s(6, 3, 7, 65, 12, 20, 2, 4, 4, "lm48", inner=24, oscale=4.0, blank=1.0),
    "s_yaml": _s(0, 4, 12, 128, 512, 256, 5, 4, 4, "yaml"),
}
B33 = "s_b33_ctx2_v65"
YAML = "s_yaml"


def make(name, seed=None):
    """-> (predictor / joiner weights in the names of rnnt_stateless_lm_f64, am (B,T,V), lengths (B), LM
    state dict; all float32 CPU tensors).  `seed` overrides the case's (the seed search)."""
    c = CASES[name]
    seed = c["seed"] if seed is None else seed
    V, E, D, ctx, s, B, T = c["V"], c["E"], c["D"], c["ctx"], c["scale"], c["B"], c["T"]
    g = torch.Generator().manual_seed(9000 + seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)                     # noqa: E731
    p = dict(emb=rn(V, E), conv_w=rn(E, ctx) / ctx ** 0.5, lin_w=rn(D, E) / E ** 0.5, lin_b=0.1 * rn(D),
             pre_w=s * rn(V, D) / D ** 0.5, pre_b=0.1 * s * rn(V))
    am = s * rn(B, T, V)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 0
    if B > 2:
        lens[2] = T + 3
    spread = (2 * torch.log(torch.tensor(float(V)))) ** 0.5
    if c["inner"]:
        n, o = c["inner"], c["oscale"]
        p.update(o1_w=rn(n, V) / V ** 0.5, o1_b=0.1 * rn(n), o2_w=o * rn(V, n) / n ** 0.5, o2_b=0.1 * o * rn(V))
        # the blank bias sits behind the out-projection (rnnt_lstm_search_cases.make)
        p["o2_b"][0] += c["blank"] * spread * o * (0.6 if c["act"] == "tanh" else 0.8 * s)
    else:
        am[:, :, 0] += c["blank"] * spread * s * 0.5
    return p, am, lens, lm_weights(c["lm"], seed)


def evaluate(name, dtype, lm_weight=None, seed=None):
    """The restatement on a case with the weights in `dtype` -> per utterance (tokens, score, lm_score,
    frames, margin)."""
    c = CASES[name]
    p, am, lens, sd = make(name, seed)
    p, sd = SF.cast(p, dtype), L.cast(sd, dtype)
    return [SF.beam_search_lm(am[b, :clamp(lens[b], c["T"])], p, c["ctx"], c["act"], c["beam"], c["topk"], sd,
                              c["weight"] if lm_weight is None else lm_weight, c["start"])
            for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


@functools.lru_cache(maxsize=None)
def unfused(name):
    """The same search with lm_weight = 0, float64 (do not modify)."""
    return evaluate(name, torch.float64, lm_weight=0.0)


def fused_fp32_figure(name):
    ref, f32 = reference(name), evaluate(name, torch.float32)
    col = lambda rs, i: torch.tensor([r[i] for r in rs], dtype=torch.float64)    # noqa: E731
    return max(rel_err(col(f32, i), col(ref, i)) for i in (1, 2))


# ------------------------------------------------------------------ the predictor step on its own
STEP_ROWS = C.PRED_ROWS                              # 19: across the 16-row tile
STEP_CASES = ["s_b1_ctx1_beam1_k1", "s_b17_ctx5_e65", "s_v128_e130_beam16_start", "s_yaml"]   # ctx 1, 5, 5, 5; E 12 .. 512
_SCHEDULE = {63: "h20", 128: "h64"}                  # V -> whose rnnt_lstm_search_cases.pred_schedule


def step_schedule(name):
    return C.pred_schedule(_SCHEDULE[CASES[name]["V"]])


def step_chain(name, dtype):
    """-> [(ctx (R,ctx) int64, lm (R,V))] after each of the five masked steps of step_schedule, from ctx
    blanks and zero lm, on the weights of seed 100."""
    c = CASES[name]
    p = SF.cast(make(name, 100)[0], dtype)
    ctx = torch.zeros(STEP_ROWS, c["ctx"], dtype=torch.int64)
    lm = p["emb"].new_zeros(STEP_ROWS, c["V"])
    out = []
    with torch.no_grad():
        for tokens, emit, parent in step_schedule(name):
            ctx, lm = SF.masked_step(p, tokens, emit, parent, ctx, lm)
            out.append((ctx, lm))
    return out


def step_fp32_figure(name):
    ref, f32 = step_chain(name, torch.float64), step_chain(name, torch.float32)
    return max(rel_err(f32[i][1], ref[i][1]) for i in (0, 4))


# ------------------------------------------------------------------ measured cost of fp32
# The largest value seen with 1, 4, 8 and 16 host threads, rounded up to two digits, the value
# itself behind (the rule of tests/yardstick.py).
STEP_COST = {                           # the lm rows after steps 1 and 5
    "s_b1_ctx1_beam1_k1": 1.5e-07,      # 1.471e-07
    "s_b17_ctx5_e65": 2.4e-07,          # 2.369e-07
    "s_v128_e130_beam16_start": 3.3e-07,   # 3.259e-07
    "s_yaml": 6.4e-07,                  # 6.337e-07
}
FUSED_COST = {                          # the larger of score's and lm_score's
    "s_b1_ctx1_beam1_k1": 1.9e-08,      # 1.807e-08
    "s_v11_beam16_kV": 3.2e-07,         # 3.107e-07
    "s_b17_ctx5_e65": 4.8e-07,          # 4.715e-07
    "s_b33_ctx2_v65": 1.1e-07,          # 1.053e-07
    "s_v128_e130_beam16_start": 6.7e-08,   # 6.681e-08
    "s_inner_v65": 6.3e-07,             # 6.247e-07
    "s_yaml": 7.0e-08,                  # 6.995e-08
}
