"""Plain-torch restatement of the RNN-T beam search with RNN-LM shallow fusion over the STATELESS
predictor and the joiner with or without output projection: the yardstick of
tests/test_gpu_rnnt_stateless_lm.py (csrc/decode_lstm.hip s2t_rnnt_beam_stateless_lm,
s2t_stateless_pred_step).

Test infrastructure (not a test file).  The search is rnnt_lm_fusion_f64.search (the one
beam_search_lm_stateless runs for inner == 0); what is stated here is the predictor on rows, the joint
with the two out-projection Linears as rnnt_lstm_search_f64.joint states it, the masked step on R rows
(the analogue of lm_masked_step) and the plain RNN-T score of a path.  It works in the dtype of the
weights it is given.

Weights `p`: emb (V,E), conv_w (E,ctx), lin_w (D,E), lin_b (D), pre_w (V,D), pre_b (V), and with an
output projection o1_w (inner,V), o1_b, o2_w (V,inner), o2_b -- the names of rnnt_lstm_search_f64, so that
its joint serves.  A row's predictor state is its last ctx tokens, most recent last; ctx blanks at the
start.
"""
import torch

import rnnt_lm_fusion_f64 as F
import rnnt_lstm_search_f64 as S

KEYS = ("emb", "conv_w", "lin_w", "lin_b", "pre_w", "pre_b", "o1_w", "o1_b", "o2_w", "o2_b")


def cast(p, dtype):
    return {k: v.to(dtype) for k, v in p.items()}


def lm_vectors(p, ctx_rows):
    """ctx_rows (R,ctx) int64 -> lm (R,V) = pre_proj(linear(sum_k conv_w[:,k] * emb[ctx[k]]))."""
    e = (p["emb"][ctx_rows] * p["conv_w"].t().unsqueeze(0)).sum(dim=1)          # (R,ctx,E) -> (R,E)
    return (e @ p["lin_w"].t() + p["lin_b"]) @ p["pre_w"].t() + p["pre_b"]


def shift(ctx_rows, tokens):
    return torch.cat([ctx_rows[:, 1:], tokens.reshape(-1, 1)], dim=1)


def masked_step(p, tokens, emit, parent, ctx_rows, lm):
    """s2t_stateless_pred_step: row r takes the context of row parent[r]; it shifts tokens[r] in where
    emit[r], else keeps that context and that lm row.  ctx_rows (R,ctx) int64, lm (R,V)."""
    src = ctx_rows[parent]
    new = shift(src, tokens)
    m = emit.bool().unsqueeze(1)
    return torch.where(m, new, src), torch.where(m, lm_vectors(p, new), lm[parent])


def log_probs(p, am_t, lm, act):
    return torch.log_softmax(S.joint(p, am_t, lm, act)[0], dim=-1)


@torch.no_grad()
def beam_search_lm(am, p, ctx, act, beam_size, cutoff_top_k, sd, lm_weight, lm_start_token=None):
    """am (T,V), cut to the utterance's length -> (tokens, score, lm_score, frames, margin)."""
    am = am.to(p["emb"].dtype)
    vec = lambda st: lm_vectors(p, torch.tensor([st], dtype=torch.int64))       # noqa: E731
    return F.search(am, lambda: (vec((0,) * ctx), (0,) * ctx),
                    lambda c, st: (vec(st[1:] + (c,)), st[1:] + (c,)),
                    lambda am_t, lm: log_probs(p, am_t, lm, act),
                    beam_size, cutoff_top_k, sd, lm_weight, lm_start_token)


@torch.no_grad()
def path_score(am, p, ctx, act, tokens, frames):
    """The plain RNN-T score of the path that emits tokens[i] at frames[i] and blank elsewhere."""
    am = am.to(p["emb"].dtype)
    st = (0,) * ctx
    at = dict(zip(frames, tokens))
    score = am.new_zeros(())
    for t in range(am.shape[0]):
        lp = log_probs(p, am[t], lm_vectors(p, torch.tensor([st], dtype=torch.int64)), act)[0]
        c = at.get(t, 0)
        score = score + lp[c]
        if c != 0:
            st = st[1:] + (c,)
    return float(score)
