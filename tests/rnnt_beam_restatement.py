"""Functional restatement of the reference's RNN-T beam search (model/decoding.py:295-425,
RnntBeamDecoding) for the stateless predictor and a joiner without output projection, in
float64 numpy.  Test infrastructure: tools/gen_golden.py::gen_rnnt_beam pins it to the reference
class (same tokens on every stored utterance) and tests/test_rnnt_beam.py uses it as the exact
answer for a given `am`.

The predictor state of a beam is its last `ctx` tokens (init state + the blank start token =
`ctx` blanks).  The orders the reference leaves to its library are fixed here: the top-k of a beam
is by (log-prob descending, class ascending); candidates are ranked by (score descending, parent
beam position ascending, rank in the parent's top-k ascending) -- Python's stable
`sorted(..., reverse=True)` over the reference's append order.  Equal hypotheses are not merged.

Besides tokens / score / emission frames the search reports its DECISION MARGIN: the smallest
gap, over all frames, at the three places where a rounding error can change the result -- between
the cutoff_top_k-th and the next class of a live beam, between the beam_size-th and the next
candidate, and between the best and the second beam after the last frame."""
import numpy as np

PARAM_KEYS = ("emb", "conv_w", "lin_w", "lin_b", "pre_w", "pre_b")


def lm_vector(state, p):
    """pre_proj(linear(conv(embed(state)))) of one predictor state (ctx tokens, most recent last)."""
    e = (p["emb"][list(state)].T * p["conv_w"]).sum(axis=1)              # [E]
    return p["pre_w"] @ (p["lin_w"] @ e + p["lin_b"]) + p["pre_b"]       # [V]


def log_softmax(z):
    m = z.max()
    return z - (m + np.log(np.exp(z - m).sum()))


def beam_search(am, params, ctx, act="relu", beam_size=4, cutoff_top_k=4):
    """am [T][V] (= enc_proj(encoder_out), bias included, cut to the utterance's length).
    -> (tokens list, score float, frames list, margin float)."""
    p = {k: np.asarray(params[k], dtype=np.float64) for k in PARAM_KEYS}
    am = np.asarray(am, dtype=np.float64)
    T, V = am.shape
    k = min(int(cutoff_top_k), V)
    fn = (lambda z: np.maximum(z, 0.0)) if act == "relu" else np.tanh
    cache = {}

    def lm(state):
        if state not in cache:
            cache[state] = lm_vector(state, p)
        return cache[state]

    beams = [((), (), 0.0, (0,) * ctx)]                  # (tokens, frames, score, state)
    margin = np.inf
    for t in range(T):
        cands = []
        for tokens, frames, score, state in beams:
            lp = log_softmax(fn(am[t] + lm(state)))
            order = np.argsort(-lp, kind="stable")       # value descending, class ascending
            if k < V:
                margin = min(margin, lp[order[k - 1]] - lp[order[k]])
            for c in order[:k].tolist():
                if c == 0:
                    cands.append((tokens, frames, score + lp[c], state))
                else:
                    cands.append((tokens + (c,), frames + (t,), score + lp[c], state[1:] + (c,)))
        cands.sort(key=lambda x: x[2], reverse=True)     # stable: parent position, then top-k rank
        if len(cands) > beam_size:
            margin = min(margin, cands[beam_size - 1][2] - cands[beam_size][2])
        beams = cands[:beam_size]
    if len(beams) > 1:
        margin = min(margin, beams[0][2] - beams[1][2])
    tokens, frames, score, _ = beams[0]
    return list(tokens), float(score), list(frames), float(margin)


def load_fixture(golden_dir):
    """tests/golden/rnnt_beam_ref*.npz (tools/gen_golden.py::gen_rnnt_beam; the large arrays sit
    in side files) -> list of configurations, each a dict: V D E ctx act Tmax beam topk, the
    parameters (PARAM_KEYS; enc_w / enc_b / enc for all but the C3-dims configuration), am
    [8][Tmax][V] (zero past an utterance's length), lengths, tokens (list of lists: the reference
    class's), frames, score_f64, margin, N."""
    import glob
    import os
    raw = {}
    for f in sorted(glob.glob(os.path.join(golden_dir, "rnnt_beam_ref*.npz"))):
        with np.load(f) as z:
            raw.update({k: z[k] for k in z.files})
    out = []
    for ci in range(int(raw["n_configs"][0])):
        pre = f"c{ci}_"
        c = {k[len(pre):]: v for k, v in raw.items() if k.startswith(pre)}
        V, D, E, ctx, act, Tmax, beam, topk = (int(x) for x in c.pop("dims"))
        c.update(V=V, D=D, E=E, ctx=ctx, act="relu" if act == 0 else "tanh", Tmax=Tmax, beam=beam,
                 topk=topk, N=float(c["N"][0]))
        lens = c["lengths"]
        am = np.zeros((len(lens), Tmax, V), dtype=np.float32)
        off = 0
        for b, n in enumerate(lens.tolist()):
            am[b, :n] = c["am_packed"][off:off + n]
            off += n
        c["am"] = am
        n_tok = c.pop("tok_len").tolist()
        c["frames"] = [c["frames"][b, :n].tolist() for b, n in enumerate(n_tok)]
        c["tokens"] = [c["tokens"][b, :n].tolist() for b, n in enumerate(n_tok)]
        out.append(c)
    return out
