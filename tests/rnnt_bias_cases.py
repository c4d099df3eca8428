"""Seeded cases shared by tests/test_rnnt_bias_f64.py (CPU), tests/test_gpu_rnnt_bias.py and
tests/test_gpu_rnnt_bias_stream.py (GPU): the one-workgroup RNN-T beam search of the stateless predictor with
hotword biasing, without and with the back-off n-gram (csrc/decode_rnnt.hip s2t_rnnt_beam_stateless_bias,
s2t_rnnt_beam_stateless_ngram_bias and their chunk-carried forms).

Test infrastructure (not a test file).  A case is a phrase list, optionally an ARPA text, predictor / joiner
weights and am.  The code under test compiles the phrases with ContextGraph and reads the text with
NgramLm.from_arpa; the restatement (tests/rnnt_bias_f64.py) keeps the phrases as a list and the text in its own
dicts: they share the inputs, no table.  The weights and am are drawn as tests/rnnt_ngram_cases.py draws them
(generator seed 9300 + seed; the text is its lm_text too), and am carries a bump of `plant` on a path (token,
blank, token, ...) that spells phrases and abandons them part-way: utterance b walks PATHS[(b + seed) % 4] from
step b // 4.
PHRASES (2 to 6 tokens, all below the smallest V) holds [2, 3], a suffix of the prefix [1, 2, 3] of [1, 2, 3, 4],
and lists it twice (it counts once).  Every shape exists without an LM (`order` 0, the entry
s2t_rnnt_beam_stateless_bias) and with the n-gram (`_o<order>`, s2t_rnnt_beam_stateless_ngram_bias).  Why each
shape, the reasons of tests/rnnt_ngram_cases.py (a wave owns a beam and a lane the classes lane, lane + 64, ...;
64 * kRegs = 512 classes are held in registers; a thread per candidate runs the look-ups; the lm rows [beam][V]
sit in LDS while they fit 60 KiB; the trace-back stages 64 frames of records at a time):
    h_v63_beam16_k16   V 63, beam 16 / top-k 16: 256 candidates, every look-up thread busy; ctx 2
    h_v65_b17          V 65, B 17, ctx 5
    h_v11_kV           V 11, top-k 20 above V, ctx 1, tanh (at a scale that does not saturate it)
    h_v63_beam1_k1     beam 1 / top-k 1: the bias cannot change the path, bias_score must still be right
    h_v520             V 520 > 512: the instantiation that re-reads am instead of holding it
    h_v1000_beam16     V 1000, beam 16: 64 000 bytes of lm rows leave the LDS for the workspace / state row
    h_long             T 70: the finalisation reports a beam other than position 0, so the trace-back from a
                       non-zero position crosses its 64-frame blocks, a chunked run its history swap
    h_yaml             zipformer_stateless_pruned_rnnt.yaml's V 128, E 512, D 256, ctx 5; B 4, T 12
Lengths are T, 0, above T (clamped) and ragged.

The conditions, with no exclusions (tests/test_rnnt_bias_f64.py asserts them; the seeds were chosen on the CPU
for them): every utterance of every case is decided by at least MARGIN (1e-3) at every ranking cut and at the
finalisation's pick in float64; the float32 CPU run of the restatement walks the same tokens and frames; in
every case with beam > 1 the bias changes at least one utterance's tokens against bias_weight = 0; each event of
EVENTS occurs in a case of each entry.

COST holds what float32 costs the RESTATEMENT (float32 on the CPU against float64) on exactly these inputs, in
the sense of yardstick.rel_err, the largest of score's, lm_score's and bias_score's; the GPU bounds are
yardstick.bound_of(COST[name]).
"""
import functools

import numpy as np
import torch

import ctc_ngram_cases as N
import ctc_ngram_f64 as G
import rnnt_bias_f64 as R
from yardstick import FLOOR, bound_of, clamp, rel_err  # noqa: F401  (the rule of tests/yardstick.py)
from rnnt_lstm_search_f64 import MARGIN  # noqa: F401  (the decision margin, 1e-3)
from rnnt_ngram_cases import Ids, build_modules, PlainPredictor, PlainJoiner  # noqa: F401

PHRASES = [[1, 2, 3, 4], [2, 3], [2, 3], [5, 6], [7, 8, 9, 10, 1, 2]]
# a step is a token, or (token, rival): the rival gets the same bump, the noise decides between them and the bias
# leans on the one that stays in a phrase
PATHS = ([1, 2, 3, (4, 9), 5, 6, 7, 8, 9, 10, 1],              # phrases completed, [2, 3] nested in [1, 2, 3, 4]
         [1, 2, 3, (9, 4), 5, (7, 6), 8, 1, 2, 3, 4],          # lost after 3 tokens, after 1, after 2 (a fail hop)
         [7, 8, 9, 10, (5, 1), 6, 1, 2, 3, 4, 7],              # the six-token phrase abandoned after 4
         [5, (9, 6), 2, 3, 1, 7, 8, 9, 10, (1, 3), 2])         # lost after 1; the six-token phrase completed


def _h(seed, B, T, V, E, D, ctx, beam, topk, order, weight=0.5, n_tokens=300, act="relu", scale=3.0, plant=3.0,
       blank=0.5, cs=1.0, bias_weight=1.0):
    return dict(seed=seed, B=B, T=T, V=V, E=E, D=D, ctx=ctx, beam=beam, topk=topk, order=order, weight=weight,
                n_tokens=n_tokens, act=act, scale=scale, plant=plant, blank=blank, cs=cs, bias_weight=bias_weight)


# (name, the n-gram twin's order, the settings; seed = (without an LM, with the n-gram))
_SHAPES = (
    ("h_v63_beam16_k16", 5, (1, 11), dict(B=2, T=9, V=63, E=12, D=20, ctx=2, beam=16, topk=16, cs=2.0,
                                         bias_weight=1.5)),
    ("h_v65_b17", 3, (10, 10), dict(B=17, T=5, V=65, E=12, D=20, ctx=5, beam=4, topk=4)),
    ("h_v11_kV", 2, (2, 4), dict(B=3, T=9, V=11, E=12, D=24, ctx=1, beam=4, topk=20, n_tokens=120, act="tanh",
                                 scale=0.4, cs=0.3)),
    ("h_v63_beam1_k1", 1, (3, 3), dict(B=3, T=9, V=63, E=12, D=20, ctx=2, beam=1, topk=1, weight=0.3)),
    ("h_v520", 3, (11, 3), dict(B=3, T=7, V=520, E=12, D=20, ctx=2, beam=4, topk=4, n_tokens=400, cs=2.0,
                                 bias_weight=1.5)),
    ("h_v1000_beam16", 2, (0, 0), dict(B=2, T=5, V=1000, E=12, D=20, ctx=2, beam=16, topk=4, n_tokens=400,
                                         cs=2.0, bias_weight=1.5)),
    ("h_long", 3, (14, 9), dict(B=1, T=70, V=11, E=12, D=24, ctx=2, beam=2, topk=2, n_tokens=120, scale=4.0)),
    ("h_yaml", 3, (4, 4), dict(B=4, T=12, V=128, E=512, D=256, ctx=5, beam=4, topk=4, weight=0.3)),
)
CASES = {}
for _name, _order, _seeds, _kw in _SHAPES:
    CASES[_name] = _h(_seeds[0], order=0, **_kw)
    CASES[f"{_name}_o{_order}"] = _h(_seeds[1], order=_order, **_kw)
PLAIN = [n for n, c in CASES.items() if c["order"] == 0]
NGRAM = [n for n, c in CASES.items() if c["order"] > 0]
YAML, LONG, LARGE = ("h_yaml", "h_yaml_o3"), ("h_long", "h_long_o3"), ("h_v1000_beam16", "h_v1000_beam16_o2")
EVENTS = ("completions", "nested", "lost1", "lost2", "midphrase", "final_pos")


def text_of(name):
    c = CASES[name]
    return N.lm_text(c["V"], c["order"], c["n_tokens"], 0) if c["order"] else None


def graph_of(name, phrases=None):
    """A ContextGraph of the case's phrases (CPU fp32 tables), a new one every call."""
    from speech2text_amd.model.lm.context_graph import ContextGraph
    c = CASES[name]
    return ContextGraph(PHRASES if phrases is None else phrases, c["V"], context_score=c["cs"])


def model_of(name):
    """The NgramLm of an n-gram case (CPU tables), a new one every call; None without an LM."""
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    return NgramLm.from_arpa(text_of(name), num_classes=CASES[name]["V"]) if CASES[name]["order"] else None


@functools.lru_cache(maxsize=None)
def hot_of(name, dtype):
    return R.Hotwords(PHRASES, CASES[name]["cs"], dtype=dtype)


@functools.lru_cache(maxsize=None)
def dict_model(name, dtype):
    return G.DictNgram(text_of(name), CASES[name]["V"], dtype=dtype) if CASES[name]["order"] else None


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
    for b in range(B):
        path = PATHS[(b + seed) % len(PATHS)]
        for t in range(T):
            step = path[(t // 2 + b // 4) % len(path)] if t % 2 == 0 else 0
            for tok in (step if isinstance(step, tuple) else (step,)):
                am[b, t, tok] += c["plant"] * s
    return p, am, lens


def make(name, seed=None):
    """-> (predictor / joiner weights by rnnt_beam_restatement.PARAM_KEYS, am (B,T,V), lengths (B); float32 CPU
    tensors, shared: do not modify).  `seed` overrides the case's (the seed search)."""
    return _make(name, CASES[name]["seed"] if seed is None else seed)


def evaluate(name, dtype, bias_weight=None, seed=None):
    """The restatement on a case in `dtype` (np.float64 / np.float32) -> per utterance a Result."""
    c = CASES[name]
    p, am, lens = make(name, seed)
    p = {k: v.numpy() for k, v in p.items()}
    bw = c["bias_weight"] if bias_weight is None else bias_weight
    return [R.beam_search(am[b, :clamp(lens[b], c["T"])].numpy(), p, c["ctx"], c["act"], c["beam"], c["topk"],
                          hot_of(name, dtype), bw, dict_model(name, dtype), c["weight"], dtype)
            for b in range(c["B"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, np.float64)


@functools.lru_cache(maxsize=None)
def reference32(name):
    """The float32 CPU run of the restatement (do not modify)."""
    return evaluate(name, np.float32)


@functools.lru_cache(maxsize=None)
def unbiased(name):
    """The float64 results of a case at bias_weight = 0 (do not modify)."""
    return evaluate(name, np.float64, bias_weight=0.0)


def occurred(name, event):
    """Whether `event` (one of EVENTS) occurs on a reported hypothesis of the float64 run of the case."""
    return any(getattr(r, event) >= 1 for r in reference(name))


def fp32_figure(name):
    ref, f32 = reference(name), reference32(name)
    col = lambda rs, i: torch.tensor([r[i] for r in rs], dtype=torch.float64)    # noqa: E731
    return max(rel_err(col(f32, i), col(ref, i)) for i in (1, 2, 3))


def bound(name):
    """Allowed rel_err of the device's score, lm_score and bias_score in case `name`."""
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
# (V, T, seeds, the model's order (0: no LM), lm_weight, phrases, bias_weight) at the shapes of
# rnnt_ngram_cases.BRUTE: beam 16 and top-k V hold every labelling, the search drops nothing
BRUTE = ((2, 4, 100, 0, 0.0, ((1, 1), (1,)), 0.7), (2, 4, 100, 2, 0.5, ((1, 1), (1,)), 0.7),
         (3, 2, 100, 0, 0.0, ((1, 2), (2,)), 1.0), (3, 2, 100, 3, 0.5, ((1, 2), (2,)), 1.0))
BRUTE_DIMS = dict(E=6, D=8, ctx=2)


def brute_inputs(V, T, n):
    """n seeded (weights, am [T][V]) at the exhaustive shapes, float64 numpy (rnnt_ngram_cases' draw)."""
    import rnnt_ngram_cases
    return rnnt_ngram_cases.brute_inputs(V, T, n)


def brute_text(V, order):
    return N.lm_text(V, order, 60, 1)


BRUTE_N = 24            # seeds of a configuration the device runs (a launch and a module pair each)


@functools.lru_cache(maxsize=None)
def brute_decided(i):
    """The inputs of BRUTE[i] the device is held to, chosen here on the CPU: of its first BRUTE_N seeds those whose
    best labelling leads the second best by MARGIN and whose float64 restatement decides every cut by MARGIN
    -> [(weights, am, rnnt_bias_f64.brute_force's result, the float64 and the float32 restatement's Result)]."""
    V, T, _, order, weight, phrases, bias_weight = BRUTE[i]
    out = []
    for p, am in brute_inputs(V, T, BRUTE_N):
        runs = []
        for dt in (np.float64, np.float32):
            ng = G.DictNgram(brute_text(V, order), V, dtype=dt) if order else None
            hot = R.Hotwords([list(q) for q in phrases], 1.0, dtype=dt)
            runs.append(R.beam_search(am, p, BRUTE_DIMS["ctx"], "relu", 16, V, hot, bias_weight, ng, weight, dt))
        ng = G.DictNgram(brute_text(V, order), V) if order else None
        best = R.brute_force(am, p, BRUTE_DIMS["ctx"], "relu", R.Hotwords([list(q) for q in phrases], 1.0),
                             bias_weight, ng, weight)
        if best[5] >= MARGIN and runs[0].margin >= MARGIN:
            out.append((p, am, best, runs[0], runs[1]))
    return out


def brute_fp32_figure(i):
    """What float32 costs the restatement on brute_decided(i): the largest rel_err of score, lm_score, bias_score."""
    rows = brute_decided(i)
    col = lambda k, j: torch.tensor([r[k][j] for r in rows], dtype=torch.float64)    # noqa: E731
    return max(rel_err(col(4, j), col(3, j)) for j in (1, 2, 3))


# brute_fp32_figure(i), rounded up to two digits, the value itself behind; the device bound is bound_of of it
BRUTE_COST = (1.4e-07, 1.6e-07, 1.7e-07, 3.0e-07)     # 1.345e-07, 1.575e-07, 1.672e-07, 2.994e-07


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figure(name), rounded up to two digits, the value itself behind.
COST = {
    "h_v63_beam16_k16": 4.3e-07,        # 4.282e-07
    "h_v63_beam16_k16_o5": 1.4e-07,     # 1.384e-07
    "h_v65_b17": 3.6e-07,               # 3.511e-07
    "h_v65_b17_o3": 1.6e-07,            # 1.546e-07
    "h_v11_kV": 4.9e-08,                # 4.894e-08
    "h_v11_kV_o2": 1.3e-07,             # 1.234e-07
    "h_v63_beam1_k1": 5.6e-07,          # 5.587e-07
    "h_v63_beam1_k1_o1": 1.9e-07,       # 1.819e-07
    "h_v520": 3.0e-07,                  # 2.903e-07
    "h_v520_o3": 6.4e-08,               # 6.382e-08
    "h_v1000_beam16": 3.8e-07,          # 3.782e-07
    "h_v1000_beam16_o2": 5.3e-08,       # 5.292e-08
    "h_long": 9.1e-07,                  # 9.006e-07
    "h_long_o3": 1.3e-07,               # 1.268e-07
    "h_yaml": 3.9e-07,                  # 3.807e-07
    "h_yaml_o3": 1.2e-07,               # 1.157e-07
}


# ------------------------------------------------------------------ the project's modules on a case's weights
def modules(dev, name, dtype=torch.float32, inner=0):
    """Predictor / Joiner (stateless; inner > 0: with an output projection of that width, drawn here) on `dev`
    carrying the weights of a case."""
    c = CASES[name]
    p = make(name)[0]
    pred, join = build_modules(dev, c["V"], c["E"], c["D"], c["ctx"], c["act"], inner)
    pred, join = pred.to(dtype), join.to(dtype)
    q = pred.predictor
    with torch.no_grad():
        q._embedding.weight.copy_(p["emb"])
        q._conv.weight.copy_(p["conv_w"].reshape(c["E"], 1, c["ctx"]))
        q._output_linear.weight.copy_(p["lin_w"])
        q._output_linear.bias.copy_(p["lin_b"])
        if not inner:
            join._pre_proj.weight.copy_(p["pre_w"])
            join._pre_proj.bias.copy_(p["pre_b"])
    return pred, join


def plain_modules(name, dtype=torch.float64):
    c = CASES[name]
    p = {k: v.to(dtype) for k, v in make(name)[0].items()}
    return PlainPredictor(p, c["ctx"]), PlainJoiner(p, c["act"])


# ------------------------------------------------------------------ a case on the device
_ON_DEVICE = {}


def device_case(dev, name):
    """(case, predictor, joiner, ContextGraph, NgramLm or None, am and lengths on the device, the float64 results),
    once per case and process (do not modify)."""
    if name not in _ON_DEVICE:
        _, am, lens = make(name)
        pred, join = modules(dev, name)
        lm = model_of(name)
        _ON_DEVICE[name] = (CASES[name], pred, join, graph_of(name).to(dev), None if lm is None else lm.to(dev),
                            am.to(dev), lens.to(dev), reference(name))
    return _ON_DEVICE[name]


def fused(case, am=None, lens=None, graph=None, **kw):
    """rnnt_beam_bias_tokens_from_am on a device_case at the case's settings; kw overrides them."""
    from speech2text_amd.model.rnnt_bias import rnnt_beam_bias_tokens_from_am
    c, p, j, g, lm, am0, lens0, _ = case
    args = dict(bias_weight=c["bias_weight"], lm=lm, lm_weight=c["weight"], beam_size=c["beam"], cutoff_top_k=c["topk"])
    args.update(kw)
    return rnnt_beam_bias_tokens_from_am(am0 if am is None else am, lens0 if lens is None else lens, p, j,
                                         g if graph is None else graph, **args)
