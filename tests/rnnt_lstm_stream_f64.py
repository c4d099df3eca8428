"""Plain-torch restatement of the chunk-carried RNN-T searches over the LSTM predictor: the
yardstick of `stable_len` in tests/test_gpu_rnnt_lstm_stream.py (csrc/decode_lstm.hip,
s2t_rnnt_*_lstm_chunk).

Test infrastructure (not a test file).  `beam_search_chunk` and `greedy_chunk` are S.beam_search and
S.greedy of tests/rnnt_lstm_search_f64.py statement for statement, with what those keep in local
variables between two frames carried between two calls instead; tests/test_rnnt_lstm_stream_f64.py
holds them to the whole-utterance functions for every case and cut.  They work in the dtype of the
weights, as that module does.
"""
import torch

import rnnt_lstm_search_f64 as S


def beam_start(w):
    """The beams of an empty stream: (tokens, frames, score, state, lm), one beam of score 0."""
    lm, state = S._start(w)
    return [((), (), w["emb"].new_zeros(()), state, lm)]


@torch.no_grad()
def beam_search_chunk(beams, t0, am, w, act="relu", beam_size=4, cutoff_top_k=4):
    """The frames am (Tc,V) of a stream that has seen t0 frames -> (beams, margin of this chunk)."""
    am = am.to(w["emb"].dtype)
    T, V = am.shape
    k = min(int(cutoff_top_k), V)
    margin = float("inf")
    for t in range(T):
        z, _ = S.joint(w, am[t], torch.cat([b[4] for b in beams], 0), act)
        lps = torch.log_softmax(z, dim=-1)
        cands = []
        for (tokens, frames, score, st, lmv), lp in zip(beams, lps):
            vals, order = torch.sort(lp, descending=True, stable=True)   # value desc, class asc
            if k < V:
                margin = min(margin, float(vals[k - 1] - vals[k]))
            for v, c in zip(vals[:k], order[:k].tolist()):
                if c == 0:
                    cands.append((tokens, frames, score + v, st, lmv, 0))
                else:
                    cands.append((tokens + (c,), frames + (t0 + t,), score + v, st, lmv, c))
        cands.sort(key=lambda x: float(x[2]), reverse=True)  # stable: parent position, then rank
        if len(cands) > beam_size:
            margin = min(margin, float(cands[beam_size - 1][2] - cands[beam_size][2]))
        beams = []
        for tokens, frames, score, st, lmv, c in cands[:beam_size]:
            if c != 0:
                lmv, st = S.pred_step(w, torch.tensor([c]), st)
            beams.append((tokens, frames, score, st, lmv))
    return beams, margin


def common_prefix_len(seqs):
    """The length of the longest common prefix of the sequences."""
    n = 0
    for column in zip(*seqs):
        if any(x != column[0] for x in column):
            break
        n += 1
    return n


def beam_search_chunked(am, cuts, w, act="relu", beam_size=4, cutoff_top_k=4, every=None):
    """am (T,V) fed in the pieces [cuts[i], cuts[i+1]) -> (tokens, score, frames, margin, stable):
    the best beam after the last piece as S.beam_search gives it, and the common-prefix length of
    the live beams' token sequences after every piece.  every(beams): called after each piece."""
    beams, margin, stable = beam_start(w), float("inf"), []
    for a, b in zip(cuts[:-1], cuts[1:]):
        beams, m = beam_search_chunk(beams, a, am[a:b], w, act, beam_size, cutoff_top_k)
        margin = min(margin, m)
        stable.append(common_prefix_len([x[0] for x in beams]))
        if every is not None:
            every(beams)
    if len(beams) > 1:
        margin = min(margin, float(beams[0][2] - beams[1][2]))
    tokens, frames, score = beams[0][:3]
    return list(tokens), float(score), list(frames), margin, stable


def greedy_start(w):
    """The carry of an empty stream: (tokens, state, lm)."""
    lm, state = S._start(w)
    return [], state, lm


@torch.no_grad()
def greedy_chunk(carry, am, w, act="relu", max_token_step=10):
    """The frames am (Tc,V) from the carried (tokens, state, lm) -> (carry, margin, forced).  A chunk
    ends right after a frame advance, where the symbols-on-this-frame counter is 0: not carried."""
    am = am.to(w["emb"].dtype)
    out, state, lm = carry
    out = list(out)
    t, nts, margin, forced = 0, 0, float("inf"), 0
    while t < am.shape[0]:
        z, pre = S.joint(w, am[t], lm, act)
        if act == "relu" and "o1_w" not in w and float(pre.max()) < -S.MARGIN:
            tok = 0
        else:
            top = torch.topk(z[0], 2)
            margin = min(margin, float(top.values[0] - top.values[1]))
            tok = int(top.indices[0])
        if tok == 0 or nts > max_token_step:
            forced += tok != 0
            t += 1
            nts = 0
        else:
            nts += 1
            out.append(tok)
            lm, state = S.pred_step(w, torch.tensor([tok]), state)
    return (out, state, lm), margin, forced


def greedy_chunked(am, cuts, w, act="relu", max_token_step=10):
    """-> (tokens, margin, forced, the token count after every piece)."""
    carry, margin, forced, counts = greedy_start(w), float("inf"), 0, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        carry, m, f = greedy_chunk(carry, am[a:b], w, act, max_token_step)
        margin, forced = min(margin, m), forced + f
        counts.append(len(carry[0]))
    return carry[0], margin, forced, counts


def cuts_of(n, how, seed=0):
    """Boundaries [0, ..., n] of the partition `how` of n frames: "1", "7", "16" or "irregular"
    (seeded piece sizes 0..16, empty pieces included)."""
    if how != "irregular":
        return list(range(0, n, int(how))) + [n]
    g = torch.Generator().manual_seed(300 + seed)
    cuts = [0]
    while cuts[-1] < n:
        cuts.append(min(n, cuts[-1] + int(torch.randint(0, 17, (1,), generator=g))))
    return cuts
