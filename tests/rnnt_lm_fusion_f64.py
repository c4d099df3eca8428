"""Plain-torch restatement of the RNN-T beam search with RNN-LM shallow fusion: the yardstick of
tests/test_gpu_rnnt_lm_fusion.py (csrc/decode_lstm.hip s2t_rnnt_beam_lstm_lm, s2t_rnn_lm_step).

Test infrastructure (not a test file).  Built on tests/rnnt_lstm_search_f64.py (pred_step / joint: the
LSTM predictor and the joiner) and tests/rnn_lm_f64.py (score_step_ref: the language model); it works
in the dtype of the weights it is given.  The search is rnnt_lstm_search_f64.beam_search plus one term.
Every beam also carries the LM's state, q = the LM's log-probabilities of the next token given the
beam's tokens, and lm_sum.  At a frame the cutoff_top_k classes of a beam are chosen by the RNN-T
log-probability alone; the candidate of class c scores (score + lp) + (c != blank ? lm_weight * q[c] : 0)
and sums lm_sum + (c != blank ? q[c] : 0); ranking and selection are unchanged; a kept beam that
emitted steps the predictor and the LM, one that took blank keeps everything.  lm_start_token None:
zero LM state, q = 0 (the first token carries no LM term, how rnn_lm_f64.score_ref scores a
sequence); a token: the LM is first stepped on it from zero state.

`sd`: the LM's state dict in the names of rnn_lm_f64 (_embedding.weight, _rnn_layer.weight_ih_l{k} ...,
_logits_layer.weight / .bias).
"""
import torch

import rnn_lm_f64 as R
import rnnt_lstm_search_f64 as S


def lm_zero_state(sd, n):
    L, H = R.num_layers(sd), sd["_rnn_layer.weight_hh_l0"].shape[1]
    z = sd["_embedding.weight"].new_zeros(L, n, H)
    return z, z.clone()


def lm_start(sd, lm_start_token):
    """-> (q (V), LM state) of the empty hypothesis."""
    state = lm_zero_state(sd, 1)
    if lm_start_token is None:
        return sd["_embedding.weight"].new_zeros(sd["_logits_layer.weight"].shape[0]), state
    q, state = R.score_step_ref(sd, torch.tensor([int(lm_start_token)]), state)
    return q[0], state


def search(am, start, step, log_probs, beam_size, cutoff_top_k, sd, lm_weight, lm_start_token=None):
    """The fused search over any predictor: start() -> (lm vector (1,V), state); step(token, state)
    -> the same; log_probs(am_t, lm vectors (n,V)) -> (n,V).  -> (tokens, score, lm_score, frames,
    margin), the margin being beam_search's three-place one taken on the fused scores."""
    T, V = am.shape
    k = min(int(cutoff_top_k), V)
    lm, state = start()
    q, ls = lm_start(sd, lm_start_token)
    zero = am.new_zeros(())
    beams = [((), (), zero, state, lm, ls, q, zero)]  # (tokens, frames, score, state, lm, LM state, q, lm_sum)
    margin = float("inf")
    for t in range(T):
        lps = log_probs(am[t], torch.cat([b[4] for b in beams], 0))
        cands = []
        for (tokens, frames, score, st, lmv, ls, q, lm_sum), lp in zip(beams, lps):
            vals, order = torch.sort(lp, descending=True, stable=True)   # value desc, class asc
            if k < V:
                margin = min(margin, float(vals[k - 1] - vals[k]))
            for v, c in zip(vals[:k], order[:k].tolist()):
                if c == 0:
                    cands.append((tokens, frames, score + v, st, lmv, ls, q, lm_sum, 0))
                else:
                    cands.append((tokens + (c,), frames + (t,), (score + v) + lm_weight * q[c], st, lmv, ls, q,
                                  lm_sum + q[c], c))
        cands.sort(key=lambda x: float(x[2]), reverse=True)  # stable: parent position, then rank
        if len(cands) > beam_size:
            margin = min(margin, float(cands[beam_size - 1][2] - cands[beam_size][2]))
        beams = []
        for tokens, frames, score, st, lmv, ls, q, lm_sum, c in cands[:beam_size]:
            if c != 0:
                lmv, st = step(c, st)
                qq, ls = R.score_step_ref(sd, torch.tensor([c]), ls)
                q = qq[0]
            beams.append((tokens, frames, score, st, lmv, ls, q, lm_sum))
    if len(beams) > 1:
        margin = min(margin, float(beams[0][2] - beams[1][2]))
    tokens, frames, score = beams[0][:3]
    return list(tokens), float(score), float(beams[0][7]), list(frames), margin


@torch.no_grad()
def beam_search_lm(am, w, act, beam_size, cutoff_top_k, sd, lm_weight, lm_start_token=None):
    """am (T,V), cut to the utterance's length; w: the weights of rnnt_lstm_search_f64."""
    am = am.to(w["emb"].dtype)
    return search(am, lambda: S.pred_step(w, torch.zeros(1, dtype=torch.int64), S.zero_state(w, 1)),
                  lambda c, st: S.pred_step(w, torch.tensor([c]), st),
                  lambda am_t, lm: torch.log_softmax(S.joint(w, am_t, lm, act)[0], dim=-1),
                  beam_size, cutoff_top_k, sd, lm_weight, lm_start_token)


@torch.no_grad()
def beam_search_lm_stateless(am, p, ctx, act, beam_size, cutoff_top_k, sd, lm_weight, lm_start_token=None):
    """The same search over the stateless predictor and a projection-free joiner: `p` in the layout
    of tests/rnnt_beam_restatement.py (emb (V,E), conv_w (E,ctx), lin_w (D,E), lin_b, pre_w (V,D),
    pre_b) as tensors; a beam's predictor state is its last ctx tokens (ctx blanks at the start)."""
    am = am.to(p["emb"].dtype)

    def vec(state):                                        # rnnt_beam_restatement.lm_vector
        e = (p["emb"][list(state)].T * p["conv_w"]).sum(dim=1)
        return (p["pre_w"] @ (p["lin_w"] @ e + p["lin_b"]) + p["pre_b"]).unsqueeze(0)

    def log_probs(am_t, lm):
        z = am_t.unsqueeze(0) + lm
        return torch.log_softmax(torch.relu(z) if act == "relu" else torch.tanh(z), dim=-1)

    return search(am, lambda: (vec((0,) * ctx), (0,) * ctx),
                  lambda c, st: (vec(st[1:] + (c,)), st[1:] + (c,)), log_probs,
                  beam_size, cutoff_top_k, sd, lm_weight, lm_start_token)


@torch.no_grad()
def path_score(am, w, act, tokens, frames):
    """The plain RNN-T score of the path that emits tokens[i] at frames[i] and blank at every other
    frame (at most one symbol per frame): what the un-fused search would have summed along it."""
    am = am.to(w["emb"].dtype)
    lm, state = S.pred_step(w, torch.zeros(1, dtype=torch.int64), S.zero_state(w, 1))
    at = dict(zip(frames, tokens))
    score = am.new_zeros(())
    for t in range(am.shape[0]):
        lp = torch.log_softmax(S.joint(w, am[t], lm, act)[0], dim=-1)[0]
        c = at.get(t, 0)
        score = score + lp[c]
        if c != 0:
            lm, state = S.pred_step(w, torch.tensor([c]), state)
    return float(score)


def lm_score_ref(sd, tokens, lm_start_token=None):
    """rnn_lm_f64.score_ref of the hypothesis ([s] + tokens with a start token)."""
    seq = ([] if lm_start_token is None else [int(lm_start_token)]) + list(tokens)
    if len(seq) < 2:
        return 0.0
    t = torch.tensor([seq], dtype=torch.int64)
    return float(R.score_ref(sd, t, torch.tensor([len(seq)]))[0])


def lm_masked_step(sd, tokens, emit, parent, state, q):
    """s2t_rnn_lm_step: row r takes the LM state of row parent[r]; it steps on tokens[r] where emit[r],
    else keeps that state and that q row.  state (h, c) each (L,R,H), q (R,V)."""
    src = (state[0][:, parent], state[1][:, parent])
    q_new, new = R.score_step_ref(sd, tokens, src)
    m = emit.bool()
    return (torch.where(m.unsqueeze(1), q_new, q[parent]),
            (torch.where(m[None, :, None], new[0], src[0]), torch.where(m[None, :, None], new[1], src[1])))


# ------------------------------------------------------------------ stand-in module
class PlainLm:
    """init_states / score_step of the RNN language model over a state dict, in plain torch: what
    RnntBeamDecoding._module_loop_lm calls."""

    def __init__(self, sd):
        self.sd = sd

    def init_states(self, beam_size):
        return lm_zero_state(self.sd, beam_size)

    def score_step(self, tokens, states):
        return R.score_step_ref(self.sd, tokens, states)
