"""The float64 restatement of the RNN-T beam search (tests/rnnt_beam_restatement.py) fed its frames
in chunks: `beam_search_chunk` takes the beam list a previous call returned and the frames of one
chunk, and returns the new list.  Frames are counted from the start of the stream.  The per-frame
body is beam_search's, statement for statement; tests/test_rnnt_stream_host.py pins the two to each
other on every stored utterance for several partitions.  Test infrastructure: the answer the
chunk-carried device search (csrc/decode_rnnt.hip) is held to for `stable_len`."""
import numpy as np

from rnnt_beam_restatement import PARAM_KEYS, lm_vector, log_softmax


def initial_beams(ctx):
    """The empty hypothesis: (tokens, frames, score, predictor state = ctx blanks)."""
    return [((), (), 0.0, (0,) * ctx)]


def beam_search_chunk(beams, t0, am, params, ctx, act="relu", beam_size=4, cutoff_top_k=4, cache=None):
    """beams after frames [0, t0) + am [Tc][V] = frames [t0, t0 + Tc) -> (beams after them, the
    smallest decision gap inside the chunk: top-k cut and beam cut, as beam_search's margin without
    its final best-vs-second term)."""
    p = {k: np.asarray(params[k], dtype=np.float64) for k in PARAM_KEYS}
    am = np.asarray(am, dtype=np.float64)
    Tc, V = am.shape
    k = min(int(cutoff_top_k), V)
    fn = (lambda z: np.maximum(z, 0.0)) if act == "relu" else np.tanh
    cache = {} if cache is None else cache

    def lm(state):
        if state not in cache:
            cache[state] = lm_vector(state, p)
        return cache[state]

    margin = np.inf
    for t in range(Tc):
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
                    cands.append((tokens + (c,), frames + (t0 + t,), score + lp[c], state[1:] + (c,)))
        cands.sort(key=lambda x: x[2], reverse=True)     # stable: parent position, then top-k rank
        if len(cands) > beam_size:
            margin = min(margin, cands[beam_size - 1][2] - cands[beam_size][2])
        beams = cands[:beam_size]
    return beams, float(margin)


def best(beams):
    """-> (tokens list, score float, frames list) of the best beam, and the best-vs-second gap."""
    tokens, frames, score, _ = beams[0]
    gap = beams[0][2] - beams[1][2] if len(beams) > 1 else np.inf
    return list(tokens), float(score), list(frames), float(gap)


def common_prefix_len(beams):
    """Length of the longest common prefix of all live beams' token sequences."""
    seqs = [b[0] for b in beams]
    n = min(len(s) for s in seqs)
    for i in range(n):
        if any(s[i] != seqs[0][i] for s in seqs[1:]):
            return i
    return n


def beam_search_chunked(am, cuts, params, ctx, act="relu", beam_size=4, cutoff_top_k=4):
    """am [T][V] fed as the pieces [cuts[i], cuts[i+1]) (cuts: 0 = c0 <= c1 <= ... = T; an empty
    piece is an idle call).  -> (tokens, score, frames, margin as beam_search's, [common prefix
    length after every piece])."""
    beams, margin, stable, cache = initial_beams(ctx), np.inf, [], {}
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            beams, m = beam_search_chunk(beams, a, am[a:b], params, ctx, act, beam_size, cutoff_top_k, cache)
            margin = min(margin, m)
        stable.append(common_prefix_len(beams))
    tokens, score, frames, gap = best(beams)
    return tokens, score, frames, float(min(margin, gap)), stable
