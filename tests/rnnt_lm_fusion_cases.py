"""Seeded cases shared by tests/test_rnnt_lm_fusion_f64.py (CPU) and tests/test_gpu_rnnt_lm_fusion.py
(GPU): the RNN-T beam search with RNN-LM shallow fusion of csrc/decode_lstm.hip.

Test infrastructure (not a test file).  A case takes am, lengths (0, above T, ragged; batches of 1..33)
and predictor / joiner weights of a beam case of tests/rnnt_lstm_search_cases.py and adds a language
model paired by V, lm_weight, the start token and the search's settings.  LM_MODELS (E = H, as
RnnLm builds it; the step kernels tile 16 rows x 16 outputs, a lane sums k = lane, lane + 64, ...):
    lm20      H 20, 1 layer, V 63: off every tile, below one 64-chunk
    lm20_v11  the same with V 11; its logits layer is scaled by 32, not 4: the RNN-T of b_h20v11 is so
              peaked (a path score of -0.35 over 8 frames) that a milder LM changes nothing
    lm48      H 48, 2 layers, V 65
    lm64      H 64, 3 layers, V 128        lm64_v65  the same with V 65
    yaml      H 512, 3 layers, V 128: the dimensions of rnn_lm.yaml
The weights follow rnnt_lstm_search_cases.weights' style (normal, 1 / sqrt(fan-in)); the logits layer
is scaled by `oscale` so that the LM is peaky enough to change what the search keeps.

The b_h64o_b33 inputs are searched with cutoff_top_k 4 here (their own case has top-1, where a beam
search keeps one hypothesis and no LM can change it); beam = cutoff_top_k = 1 is f_h20_beam1_k1, where
the LM cannot change the path but lm_score must still be right.

The conditions, with no exclusions (tests/test_rnnt_lm_fusion_f64.py asserts them; the seeds were
chosen on the CPU for them): every utterance of every case is decided by at least 1e-3 at every node
in float64 and the float32 CPU run of the restatement returns the same tokens and frames; in every
case with beam > 1 at least one utterance's fused tokens differ from the un-fused search's.

LM_STEP_COST / FUSED_COST hold what float32 costs the RESTATEMENT (tests/rnnt_lm_fusion_f64.py in
float32 on the CPU against float64) on exactly these inputs, in the sense of yardstick.rel_err; the
GPU bounds are max(2e-5, 8 x figure), the rule of tests/yardstick.py.
"""
import functools

import torch

import rnnt_lm_fusion_f64 as F
import rnnt_lstm_search_cases as C
import rnnt_lstm_search_f64 as S
from yardstick import rel_err  # noqa: F401  (the rule of tests/yardstick.py)

bound = C.bound


def _lm(V, H, L, oscale):
    return dict(V=V, H=H, L=L, oscale=oscale)


LM_MODELS = {
    "lm20": _lm(63, 20, 1, 4.0),
    "lm20_v11": _lm(11, 20, 1, 32.0),
    "lm48": _lm(65, 48, 2, 4.0),
    "lm64": _lm(128, 64, 3, 4.0),
    "lm64_v65": _lm(65, 64, 3, 4.0),
    "yaml": _lm(128, 512, 3, 4.0),
}


def lm_weights(model, seed):
    """float32 CPU state dict of LM_MODELS[model] in the names of rnn_lm_f64 / RnnLm.state_dict()."""
    m = LM_MODELS[model]
    V, H = m["V"], m["H"]
    g = torch.Generator().manual_seed(6000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    sd = {"_embedding.weight": rn(V, H)}
    for k in range(m["L"]):
        sd[f"_rnn_layer.weight_ih_l{k}"] = rn(4 * H, H) / H ** 0.5
        sd[f"_rnn_layer.weight_hh_l{k}"] = rn(4 * H, H) / H ** 0.5
        sd[f"_rnn_layer.bias_ih_l{k}"] = 0.3 * rn(4 * H)
        sd[f"_rnn_layer.bias_hh_l{k}"] = 0.1 * rn(4 * H)
    sd["_logits_layer.weight"] = m["oscale"] * rn(V, H) / H ** 0.5
    sd["_logits_layer.bias"] = 0.1 * m["oscale"] * rn(V)
    return sd


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def _f(base, lm, lm_seed, weight, beam, topk, start=None):
    return dict(base=base, lm=lm, lm_seed=lm_seed, weight=weight, beam=beam, topk=topk, start=start)


CASES = {
    "f_h20_beam1_k1": _f("b_h20_beam1_k1", "lm20", 0, 0.3, 1, 1),
    "f_h20v11_beam16_kV": _f("b_h20v11_beam16_kV", "lm20_v11", 1, 0.5, 16, 20),
    "f_h48_b17_beam4": _f("b_h48_b17_beam4", "lm48", 0, 0.5, 4, 4),
    "f_h64_beam16_k4_start": _f("b_h64_beam16_k4", "lm64", 1, 0.3, 16, 4, start=127),
    "f_h64o_b33_beam4": _f("b_h64o_b33_beam4_k1", "lm64_v65", 1, 0.5, 4, 4),
    "f_yaml": _f("b_yaml", "yaml", 1, 0.3, 4, 4),
}
B33 = "f_h64o_b33_beam4"


def make(name):
    """-> (predictor / joiner weights, act, am (B,T,V), lengths (B), LM state dict; all float32)."""
    c = CASES[name]
    w, act, am, lens = C.make(c["base"])
    assert LM_MODELS[c["lm"]]["V"] == am.shape[2]
    return w, act, am, lens, lm_weights(c["lm"], c["lm_seed"])


def evaluate(name, dtype, lm_weight=None):
    """The restatement on a case with the weights in `dtype` -> per utterance (tokens, score,
    lm_score, frames, margin)."""
    c = CASES[name]
    w, act, am, lens, sd = make(name)
    w, sd = S.cast(w, dtype), cast(sd, dtype)
    T = am.shape[1]
    return [F.beam_search_lm(am[b, :C.clamp(lens[b], T)], w, act, c["beam"], c["topk"], sd,
                             c["weight"] if lm_weight is None else lm_weight, c["start"])
            for b in range(am.shape[0])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


@functools.lru_cache(maxsize=None)
def unfused(name):
    """rnnt_lstm_search_f64.beam_search (no LM) at the case's settings, float64 (do not modify)."""
    c = CASES[name]
    if (C.CASES[c["base"]]["beam"], C.CASES[c["base"]]["topk"]) == (c["beam"], c["topk"]):
        return C.reference(c["base"])
    w, act, am, lens, _ = make(name)
    w = S.cast(w, torch.float64)
    return [S.beam_search(am[b, :C.clamp(lens[b], am.shape[1])], w, act, c["beam"], c["topk"])
            for b in range(am.shape[0])]


def fused_fp32_figure(name):
    ref, f32 = reference(name), evaluate(name, torch.float32)
    return max(rel_err(torch.tensor([r[i] for r in f32]), torch.tensor([r[i] for r in ref])) for i in (1, 2))


# ------------------------------------------------------------------ the LM step on its own
STEP_MODELS = {"lm20": "h20", "lm48": "h48", "lm64": "h64", "yaml": "yaml"}   # LM -> whose pred_schedule (same V)


def step_chain(model, dtype):
    """-> [(q (R,V), (h, c) each (L,R,H))] after each of the five masked steps of
    rnnt_lstm_search_cases.pred_schedule, from zero state and zero q."""
    sd = cast(lm_weights(model, 100), dtype)
    R = C.PRED_ROWS
    state = F.lm_zero_state(sd, R)
    q = sd["_embedding.weight"].new_zeros(R, LM_MODELS[model]["V"])
    out = []
    with torch.no_grad():
        for tokens, emit, parent in C.pred_schedule(STEP_MODELS[model]):
            q, state = F.lm_masked_step(sd, tokens, emit, parent, state, q)
            out.append((q, state))
    return out


def step_tensors(step):
    return [step[0], step[1][0], step[1][1]]


def step_fp32_figure(model):
    ref, f32 = step_chain(model, torch.float64), step_chain(model, torch.float32)
    return max(rel_err(a, b) for i in (0, 4) for a, b in zip(step_tensors(f32[i]), step_tensors(ref[i])))


# ------------------------------------------------------------------ the stateless predictor (module loop only)
STATELESS = dict(V=65, E=12, D=20, ctx=2, act="relu", seed=1, B=3, T=7, beam=4, topk=4, lm="lm48", lm_seed=0,
                 weight=0.5, start=None, scale=3.0)


def stateless_case():
    """-> (configuration with the float32 numpy parameters of tests/rnnt_beam_restatement.py's layout,
    am (B,T,V), lengths, LM state dict)."""
    c = dict(STATELESS)
    V, E, D, ctx, s = c["V"], c["E"], c["D"], c["ctx"], c["scale"]
    g = torch.Generator().manual_seed(8000 + c["seed"])
    rn = lambda *sh: torch.randn(*sh, generator=g)                     # noqa: E731
    c.update(emb=rn(V, E), conv_w=rn(E, ctx) / ctx ** 0.5, lin_w=rn(D, E) / E ** 0.5, lin_b=0.1 * rn(D),
             pre_w=s * rn(V, D) / D ** 0.5, pre_b=0.1 * s * rn(V))
    am = s * rn(c["B"], c["T"], V)
    am[:, :, 0] += 1.3 * (2 * torch.log(torch.tensor(float(V)))) ** 0.5 * s * 0.5
    lens = torch.tensor([c["T"], 0, c["T"] + 3])
    for k in ("emb", "conv_w", "lin_w", "lin_b", "pre_w", "pre_b"):
        c[k] = c[k].numpy()
    return c, am, lens, lm_weights(c["lm"], c["lm_seed"])


@functools.lru_cache(maxsize=None)
def stateless_reference():
    """float64: per utterance (tokens, score, lm_score, frames, margin) (do not modify)."""
    c, am, lens, sd = stateless_case()
    p = {k: torch.from_numpy(c[k]).double() for k in ("emb", "conv_w", "lin_w", "lin_b", "pre_w", "pre_b")}
    sd = cast(sd, torch.float64)
    return [F.beam_search_lm_stateless(am[b, :C.clamp(lens[b], c["T"])].double(), p, c["ctx"], c["act"], c["beam"],
                                       c["topk"], sd, c["weight"], c["start"]) for b in range(c["B"])]


# ------------------------------------------------------------------ measured cost of fp32
# The largest value seen with 1, 4, 8 and 16 host threads, rounded up to two digits, the value
# itself behind (the rule of tests/yardstick.py).
LM_STEP_COST = {
    "lm20": 1.5e-07,                    # 1.491e-07
    "lm48": 2.1e-07,                    # 2.049e-07
    "lm64": 2.9e-07,                    # 2.899e-07
    "yaml": 1.5e-06,                    # 1.495e-06
}
FUSED_COST = {                          # the larger of score's and lm_score's
    "f_h20_beam1_k1": 1.6e-07,          # 1.600e-07
    "f_h20v11_beam16_kV": 3.4e-06,      # 3.320e-06
    "f_h48_b17_beam4": 6.4e-08,         # 6.399e-08
    "f_h64_beam16_k4_start": 4.8e-07,   # 4.740e-07
    "f_h64o_b33_beam4": 2.7e-06,        # 2.611e-06
    "f_yaml": 3.8e-07,                  # 3.782e-07
}
