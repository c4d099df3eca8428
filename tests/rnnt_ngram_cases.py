"""Seeded cases shared by tests/test_rnnt_ngram_f64.py (CPU), tests/test_gpu_rnnt_ngram.py and
tests/test_gpu_rnnt_ngram_stream.py (GPU): the one-workgroup RNN-T beam search of the stateless predictor
fused with a back-off n-gram (csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_ngram and its chunk-carried
form).

Test infrastructure (not a test file).  A case is an ARPA text, predictor / joiner weights and am.  The
text is tests/ctc_ngram_cases.py's lm_text: an order-`order` model estimated on `n_tokens` seeded tokens
of a sparse first-order source, so that the tables are sparse; the code under test reads it with
NgramLm.from_arpa, the restatement (tests/rnnt_ngram_f64.py) with DictNgram's own parser.  The weights
and am are drawn as tests/rnnt_stateless_lm_cases.py draws them (generator seed 9300 + seed), and am
carries a bump of `plant` on a path that spells a training sentence (token, blank, token, ...), so
that hypotheses walk into deep contexts while the other top-k classes back off from them.  Why each
shape (a wave owns a beam and a lane the classes lane, lane + 64, ...; 64 * kRegs = 512 classes are held
in registers; a thread per candidate runs the look-up; the lm rows [beam][V] sit in LDS while they fit
60 KiB next to 16 (E + D) + 128 ctx bytes; the trace-back stages 64 frames of records at a time):
    g_v63_o5_beam16_k16     V 63, beam 16 / top-k 16: 256 candidates, every look-up thread busy; order 5, ctx 2
    g_v65_o3_b17            V 65, B 17, ctx 5, order 3
    g_v11_o2_kV             V 11, top-k 20 above V, ctx 1, order 2, tanh (at a scale that does not saturate it)
    g_v63_o1_beam1_k1       beam 1 / top-k 1: the LM cannot change the path, lm_score must still be right; order 1
    g_v520_o3               V 520 > 512: the instantiation that re-reads am instead of holding it
    g_v1000_o2_beam16       V 1000, beam 16: 64 000 bytes of lm rows leave the LDS for the workspace / state row
    g_long_o3               T 70: the trace-back crosses its 64-frame blocks, a chunked run its history swap
    g_yaml                  zipformer_stateless_pruned_rnnt.yaml's V 128, E 512, D 256, ctx 5; B 4, T 12
Lengths are T, 0, above T (clamped) and ragged.

The conditions, with no exclusions (tests/test_rnnt_ngram_f64.py asserts them; the seeds were chosen on
the CPU for them): every utterance of every case is decided by at least 1e-3
(rnnt_lstm_search_f64.MARGIN) at every ranking cut in float64; the float32 CPU run of the restatement
walks the same tokens and frames; in every case with beam > 1 the LM changes at least one utterance's
tokens against lm_weight = 0; per order the look-ups of the cases back off 0, 1, ..., order - 1 times.

COST holds what float32 costs the RESTATEMENT (float32 on the CPU against float64) on exactly these
inputs, in the sense of yardstick.rel_err, the larger of score's and lm_score's; the GPU bounds are
max(2e-5, 8 x figure), the rule of tests/yardstick.py.
"""
import functools

import numpy as np
import torch

import ctc_ngram_cases as N
import ctc_ngram_f64 as G
import rnnt_ngram_f64 as R
from yardstick import FLOOR, bound_of, clamp, rel_err  # noqa: F401  (the rule of tests/yardstick.py)
from yardstick import MARGIN as COST_MARGIN  # noqa: F401
from rnnt_lstm_search_f64 import MARGIN  # noqa: F401  (the decision margin, 1e-3)


def _g(seed, B, T, V, E, D, ctx, beam, topk, order, weight=0.5, n_tokens=300, act="relu", scale=3.0, plant=3.0,
       blank=0.5):
    return dict(seed=seed, B=B, T=T, V=V, E=E, D=D, ctx=ctx, beam=beam, topk=topk, order=order, weight=weight,
                n_tokens=n_tokens, act=act, scale=scale, plant=plant, blank=blank)


CASES = {
    "g_v63_o5_beam16_k16": _g(0, 2, 8, 63, 12, 20, 2, 16, 16, 5),
    "g_v65_o3_b17": _g(0, 17, 5, 65, 12, 20, 5, 4, 4, 3),
    "g_v11_o2_kV": _g(2, 3, 9, 11, 12, 24, 1, 4, 20, 2, n_tokens=120, act="tanh", scale=0.4),
    "g_v63_o1_beam1_k1": _g(0, 3, 9, 63, 12, 20, 2, 1, 1, 1, weight=0.3),
    "g_v520_o3": _g(1, 3, 6, 520, 12, 20, 2, 4, 4, 3, n_tokens=400),
    "g_v1000_o2_beam16": _g(0, 2, 5, 1000, 12, 20, 2, 16, 4, 2, n_tokens=400),
    "g_long_o3": _g(1, 1, 70, 11, 12, 24, 2, 2, 2, 3, n_tokens=120, scale=4.0),
    "g_yaml": _g(3, 4, 12, 128, 512, 256, 5, 4, 4, 3, weight=0.3),
}
YAML = "g_yaml"
LONG = "g_long_o3"
LARGE = "g_v1000_o2_beam16"


def text_of(name):
    c = CASES[name]
    return N.lm_text(c["V"], c["order"], c["n_tokens"], 0)


@functools.lru_cache(maxsize=None)
def model(name):
    """The NgramLm of a case, read from its text (CPU tables; do not move: copy with from_arpa)."""
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.from_arpa(text_of(name), num_classes=CASES[name]["V"])


@functools.lru_cache(maxsize=None)
def dict_model(name, dtype):
    return G.DictNgram(text_of(name), CASES[name]["V"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def _make(name, seed):
    c = CASES[name]
    V, E, D, ctx, s, B, T = c["V"], c["E"], c["D"], c["ctx"], c["scale"], c["B"], c["T"]
    g = torch.Generator().manual_seed(9300 + seed)
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
    am[:, :, 0] += c["blank"] * s
    seqs = N.lm_sequences(V, c["n_tokens"], 0)
    for b in range(B):
        sent = seqs[(b + seed) % len(seqs)]
        for t in range(T):
            am[b, t, sent[(t // 2) % len(sent)] if t % 2 == 0 else 0] += c["plant"] * s
    return p, am, lens


def make(name, seed=None):
    """-> (predictor / joiner weights by rnnt_beam_restatement.PARAM_KEYS, am (B,T,V), lengths (B); float32
    CPU tensors, shared: do not modify).  `seed` overrides the case's (the seed search)."""
    return _make(name, CASES[name]["seed"] if seed is None else seed)


def evaluate(name, dtype, lm_weight=None, seed=None):
    """The restatement on a case in `dtype` (np.float64 / np.float32) -> per utterance a Result."""
    c = CASES[name]
    p, am, lens = make(name, seed)
    p = {k: v.numpy() for k, v in p.items()}
    w = c["weight"] if lm_weight is None else lm_weight
    return [R.beam_search(am[b, :clamp(lens[b], c["T"])].numpy(), p, c["ctx"], c["act"], c["beam"], c["topk"],
                          dict_model(name, dtype), w, dtype) for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, np.float64)


@functools.lru_cache(maxsize=None)
def reference32(name):
    """The float32 CPU run of the restatement (do not modify)."""
    return evaluate(name, np.float32)


@functools.lru_cache(maxsize=None)
def unfused(name):
    """The float64 results of a case at lm_weight = 0 (do not modify)."""
    return evaluate(name, np.float64, lm_weight=0.0)


def fp32_figure(name):
    ref, f32 = reference(name), reference32(name)
    col = lambda rs, i: torch.tensor([r[i] for r in rs], dtype=torch.float64)    # noqa: E731
    return max(rel_err(col(f32, i), col(ref, i)) for i in (1, 2))


def bound(name):
    """Allowed rel_err of the device's score and lm_score in case `name`."""
    return bound_of(COST[name])


def cuts_of(name, b, kind):
    """The chunk boundaries of utterance b of a case: kind 1, 4, 7 frames a piece, or "ragged": pieces of
    1 + (b + i) % 5 frames with an idle call (an empty piece) after every second one."""
    c = CASES[name]
    L = clamp(make(name)[2][b], c["T"])
    cuts, i = [0], 0
    while cuts[-1] < L:
        step = kind if kind != "ragged" else 1 + (b + i) % 5
        cuts.append(min(L, cuts[-1] + step))
        if kind == "ragged" and i % 2 == 1:
            cuts.append(cuts[-1])
        i += 1
    return cuts


# ------------------------------------------------------------------ the exhaustive cases
# (V, T, seeds, the model's order, lm_weight): beam 16 and top-k V hold every labelling, the search drops nothing
BRUTE = ((2, 4, 100, 2, 0.5), (3, 2, 100, 3, 0.5))
BRUTE_DIMS = dict(E=6, D=8, ctx=2)


def brute_inputs(V, T, n):
    """n seeded (weights, am [T][V]) at the exhaustive shapes, float64 numpy."""
    g = torch.Generator().manual_seed(9400 + 10 * T + V)
    E, D, ctx = BRUTE_DIMS["E"], BRUTE_DIMS["D"], BRUTE_DIMS["ctx"]
    rn = lambda *sh: torch.randn(*sh, generator=g, dtype=torch.float64).numpy()   # noqa: E731
    out = []
    for _ in range(n):
        p = dict(emb=rn(V, E), conv_w=rn(E, ctx) / ctx ** 0.5, lin_w=rn(D, E) / E ** 0.5, lin_b=0.1 * rn(D),
                 pre_w=2.0 * rn(V, D) / D ** 0.5, pre_b=0.2 * rn(V))
        out.append((p, 2.0 * rn(T, V)))
    return out


def brute_text(V, order):
    return N.lm_text(V, order, 60, 1)


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figure(name), rounded up to two digits, the value itself behind.
# (numpy sums here, no threaded matmul: the figures are the same with 1, 4 and 16 host threads)
COST = {
    "g_v63_o5_beam16_k16": 8.2e-08,     # 8.191e-08
    "g_v65_o3_b17": 2.2e-07,            # 2.146e-07
    "g_v11_o2_kV": 1.5e-07,             # 1.401e-07
    "g_v63_o1_beam1_k1": 1.1e-07,       # 1.068e-07
    "g_v520_o3": 9.6e-08,               # 9.526e-08
    "g_v1000_o2_beam16": 6.2e-08,       # 6.102e-08
    "g_long_o3": 1.7e-07,               # 1.699e-07
    "g_yaml": 1.2e-07,                  # 1.123e-07
}


# ------------------------------------------------------------------ the project's modules on a case's weights
class Ids:
    """A tokenizer that spells token ids."""

    def decode(self, t):
        return " ".join(str(int(x)) for x in t)


def build_modules(dev, V, E, D, ctx, act="relu", inner=0):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D, "symbol_embedding_dim": E,
                                                       "context_size": ctx}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=max(inner, 1), activation=act, prune_range=5,
                               use_out_project=inner > 0))
    join._enc_proj = torch.nn.Identity()                   # the searches are handed am itself
    return pred.to(dev).eval().requires_grad_(False), join.to(dev).eval().requires_grad_(False)


def modules(dev, name, dtype=torch.float32):
    """Predictor / Joiner (stateless, no output projection) on `dev` carrying the weights of a case."""
    c = CASES[name]
    p = make(name)[0]
    pred, join = build_modules(dev, c["V"], c["E"], c["D"], c["ctx"], c["act"])
    pred, join = pred.to(dtype), join.to(dtype)
    q = pred.predictor
    with torch.no_grad():
        q._embedding.weight.copy_(p["emb"])
        q._conv.weight.copy_(p["conv_w"].reshape(c["E"], 1, c["ctx"]))
        q._output_linear.weight.copy_(p["lin_w"])
        q._output_linear.bias.copy_(p["lin_b"])
        join._pre_proj.weight.copy_(p["pre_w"])
        join._pre_proj.bias.copy_(p["pre_b"])
    return pred, join


# ------------------------------------------------------------------ the same modules in plain torch, for the host loop on CPU
class PlainPredictor:
    """init_state / streaming_step of the stateless predictor over a case's weights."""

    def __init__(self, p, ctx):
        self.p, self.ctx = p, ctx

    def init_state(self):
        return torch.zeros(1, self.ctx - 1, dtype=torch.int64)

    def streaming_step(self, input, state):
        assert input.shape == (1, 1)
        rows = torch.cat([state, input.long()], dim=1)
        e = (self.p["emb"][rows[0]].t() * self.p["conv_w"]).sum(dim=1)
        return (self.p["lin_w"] @ e + self.p["lin_b"]).reshape(1, 1, -1), rows[:, 1:]


class PlainJoiner:
    """streaming_step of a joiner without output projection whose encoder output IS am."""

    def __init__(self, p, act):
        self.p, self.act = p, act

    def streaming_step(self, encoder_out, predictor_out):
        lm = predictor_out.squeeze(1) @ self.p["pre_w"].t() + self.p["pre_b"]          # (beam, V)
        z = encoder_out.reshape(1, -1) + lm
        return (torch.relu(z) if self.act == "relu" else torch.tanh(z)).log_softmax(dim=-1)


def plain_modules(name, dtype=torch.float64):
    c = CASES[name]
    p = {k: v.to(dtype) for k, v in make(name)[0].items()}
    return PlainPredictor(p, c["ctx"]), PlainJoiner(p, c["act"])
