"""Seeded cases shared by tests/test_rnnt_lstm_ngram_f64.py (CPU) and tests/test_gpu_rnnt_lstm_ngram.py (GPU):
the lockstep RNN-T beam search of the LSTM predictor fused with a back-off n-gram (csrc/decode_lstm.hip
s2t_rnnt_beam_lstm_ngram, s2t_rnnt_beam_lstm_ngram_chunk).

Test infrastructure (not a test file).  A case is predictor / joiner weights in the layout of
tests/rnnt_lstm_search_f64.py (drawn as tests/rnnt_lstm_search_cases.weights draws them), an ARPA text
(ctc_ngram_cases.lm_text: sparse tables, every back-off depth) and am (B,T,V): scale x normal, a blank
bias, and a bump of `plant` on a path that spells a training sentence, so that hypotheses walk into deep
contexts while the noise's classes back off from them.  lengths T, 0, above T, ragged.  The smallest
shapes at which these kernels can still go wrong: V 11, 63, 65 around the wave; hidden 20 (off every
tile); 1 and 2 layers; a joiner with and without out-projection; B 1, 3, 17 (across the 16-row tile);
beams 1, 4, 16; cutoff_top_k 1, 3 and above V; orders 2, 3, 5; T <= 40, and LONG, a 90-frame case for the
chunk form.  The cuts are rnnt_lm_stream_cases.PARTITIONS (1, 7, 16, irregular with idle calls).

The conditions, with no exclusions (tests/test_rnnt_lstm_ngram_f64.py asserts them; seeds and scales were
chosen on the CPU so that the restatement alone satisfies them): every utterance of every case is
decided by at least rnnt_lstm_search_f64.MARGIN in float64 and the float32 run of the restatement
returns the same tokens and frames; in LM_CHANGES cases the n-gram changes a hypothesis against
lm_weight = 0; across the cases a look-up backs off 0, 1 and order - 1 times and reaches the dense root.

COST holds what float32 costs the RESTATEMENT (float32 on the CPU against float64) on exactly these
inputs, in the sense of yardstick.rel_err, the larger of score's and lm_score's; the GPU bounds are
max(FLOOR, MARGIN x figure), the rule of tests/yardstick.py.
"""
import functools

import numpy as np
import torch

import ctc_ngram_cases as N
import ctc_ngram_f64 as G
import rnnt_lstm_ngram_f64 as R
import rnnt_lstm_search_cases as LC
from yardstick import FLOOR, bound_of, rel_err  # noqa: F401  (the rule of tests/yardstick.py)
from yardstick import MARGIN as COST_MARGIN  # noqa: F401
from rnnt_lm_stream_cases import PARTITIONS  # noqa: F401
from rnnt_lstm_search_f64 import MARGIN  # noqa: F401  (the decision margin, 1e-3)
from rnnt_lstm_stream_f64 import cuts_of as _cuts

_NP = {torch.float64: np.float64, torch.float32: np.float32}


def _m(V, L, inner, ln=True, act="relu", scale=3.0, oscale=8.0, E=12, H=20, D=24):
    return dict(V=V, E=E, H=H, D=D, L=L, ln=ln, inner=inner, act=act, scale=scale, oscale=oscale)


def _c(m, seed, B, T, beam, topk, order, weight=0.5, n_tokens=300, plant=1.0, blank=0.5):
    return dict(m=m, seed=seed, B=B, T=T, beam=beam, topk=topk, order=order, weight=weight, n_tokens=n_tokens,
                plant=plant, blank=blank)


CASES = {
    "n_v11_l1o_beam16_kV": _c(_m(11, 1, 24), 1, 1, 12, 16, 20, 3, weight=1.0, n_tokens=120),
    "n_v63_l2_b3_beam4_k3": _c(_m(63, 2, 0, ln=False), 23, 3, 40, 4, 3, 5),
    "n_v65_l1o_b17_beam4_k3": _c(_m(65, 1, 24), 0, 17, 9, 4, 3, 2),
    "n_v63_l1_beam1_k1": _c(_m(63, 1, 0), 0, 3, 20, 1, 1, 3, weight=0.3),
    "n_v65_l2_t90": _c(_m(65, 2, 0, scale=4.0), 19, 2, 90, 2, 2, 3),
}
LONG = "n_v65_l2_t90"
LM_CHANGES = ["n_v11_l1o_beam16_kV", "n_v63_l2_b3_beam4_k3", "n_v65_l1o_b17_beam4_k3"]
clamp = LC.clamp


def weights(m, seed):
    """float32 CPU weights of a model dict, drawn as rnnt_lstm_search_cases.weights draws them."""
    V, E, H, D = m["V"], m["E"], m["H"], m["D"]
    g = torch.Generator().manual_seed(5500 + seed)
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    w = dict(emb=rn(V, E), in_g=1 + 0.2 * rn(E), in_b=0.2 * rn(E), layers=[],
             eps_in=LC.EPS_IN, eps_lstm=LC.EPS_LSTM, eps_out=LC.EPS_OUT)
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


def text_of(name):
    c = CASES[name]
    return N.lm_text(c["m"]["V"], c["order"], c["n_tokens"], 0)


@functools.lru_cache(maxsize=None)
def model(name):
    """The NgramLm of a case, read from its text (CPU tables; do not move: copy with from_arpa)."""
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.from_arpa(text_of(name), num_classes=CASES[name]["m"]["V"])


@functools.lru_cache(maxsize=None)
def dict_model(name, dtype):
    return G.DictNgram(text_of(name), CASES[name]["m"]["V"], dtype=_NP[dtype])


@functools.lru_cache(maxsize=None)
def make(name):
    """-> (weights, act, am (B,T,V) float32, lengths (B) int64; some 0, some above T).  Shared: do not modify."""
    c = CASES[name]
    m = c["m"]
    w = weights(m, c["seed"])
    B, T, V, s = c["B"], c["T"], m["V"], m["scale"]
    g = torch.Generator().manual_seed(7500 + c["seed"])
    am = s * torch.randn(B, T, V, generator=g)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 0 if name != LONG else T - 17
    if B > 2:
        lens[2] = T + 3
    spread = (2 * torch.log(torch.tensor(float(V)))) ** 0.5
    if m["inner"]:                                         # (the blank bias sits behind the out-projection)
        w["o2_b"][0] += c["blank"] * spread * m["oscale"] * 0.8 * s
    else:
        am[:, :, 0] += c["blank"] * spread * s * 0.5
    seqs = N.lm_sequences(V, c["n_tokens"], 0)
    for b in range(B):
        sent = seqs[(b + c["seed"]) % len(seqs)]
        for t in range(T):
            am[b, t, sent[(t // 2) % len(sent)] if t % 2 == 0 else 0] += c["plant"] * spread * s * 0.5
    return w, m["act"], am, lens


def lengths(name):
    am, lens = make(name)[2:]
    return [clamp(n, am.shape[1]) for n in lens]


def evaluate(name, dtype, lm_weight=None):
    """The restatement on a case in `dtype` -> per utterance a rnnt_ngram_f64.Result."""
    c = CASES[name]
    w, act, am, _ = make(name)
    wt = c["weight"] if lm_weight is None else lm_weight
    return [R.beam_search(am[b, :n], w, act, c["beam"], c["topk"], dict_model(name, dtype), wt, dtype)
            for b, n in enumerate(lengths(name))]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


@functools.lru_cache(maxsize=None)
def reference32(name):
    return evaluate(name, torch.float32)


@functools.lru_cache(maxsize=None)
def unfused(name):
    """The float64 results of a case at lm_weight = 0 (do not modify)."""
    return evaluate(name, torch.float64, lm_weight=0.0)


def cuts_of(name, b, how):
    """Boundaries of partition `how` ("1", "7", "16", "irregular") of utterance b's frames."""
    return _cuts(lengths(name)[b], how, seed=b)


@functools.lru_cache(maxsize=None)
def chunked(name, b, how):
    """rnnt_lstm_ngram_f64.beam_search_chunked in float64 on utterance b (do not modify)."""
    c = CASES[name]
    w, act, am, _ = make(name)
    return R.beam_search_chunked(am[b, :lengths(name)[b]], cuts_of(name, b, how), w, act, c["beam"], c["topk"],
                                 dict_model(name, torch.float64), c["weight"])


def fp32_figure(name):
    ref, f32 = reference(name), reference32(name)
    col = lambda rs, i: torch.tensor([r[i] for r in rs], dtype=torch.float64)    # noqa: E731
    return max(rel_err(col(f32, i), col(ref, i)) for i in (1, 2))


def bound(name):
    """Allowed rel_err of the device's score and lm_score in case `name`."""
    return bound_of(COST[name])


# ------------------------------------------------------------------ the exhaustive cases
# (V, T, seeds, the model's order, lm_weight), the sizes of rnnt_ngram_cases.BRUTE: beam 16 holds every
# hypothesis, the search is exact
BRUTE = ((2, 4, 100, 2, 0.5), (3, 2, 100, 3, 0.5))
BRUTE_MODEL = dict(E=6, H=8, D=8, L=1, ln=True, inner=0, act="tanh", scale=1.0, oscale=0.0)


def brute_inputs(V, T, n):
    """-> (weights, am (n,T,V))."""
    w = weights(dict(BRUTE_MODEL, V=V), 40 + V)
    g = torch.Generator().manual_seed(9700 + 10 * T + V)
    return w, 2.0 * torch.randn(n, T, V, generator=g)


def brute_text(V, order):
    return N.lm_text(V, order, 60, 1)


@functools.lru_cache(maxsize=None)
def brute_reference(V, T, n, order, weight):
    w, am = brute_inputs(V, T, n)
    ng = G.DictNgram(brute_text(V, order), V)
    return [R.brute_force(am[i], w, BRUTE_MODEL["act"], ng, weight) for i in range(n)]


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figure(name), rounded up to two digits, the value itself behind.
COST = {
    "n_v11_l1o_beam16_kV": 1.8e-07,           # 1.741e-07
    "n_v63_l2_b3_beam4_k3": 1.9e-07,          # 1.810e-07
    "n_v65_l1o_b17_beam4_k3": 4.2e-07,        # 4.126e-07
    "n_v63_l1_beam1_k1": 6.1e-08,             # 6.051e-08
    "n_v65_l2_t90": 3.1e-07,                  # 3.058e-07
}
