"""Plain-torch restatement of the RNN-T greedy and beam search over the layer-norm LSTM predictor and
the joiner with or without output projection: the yardstick of tests/test_gpu_rnnt_lstm_search.py
(csrc/decode_lstm.hip).

Test infrastructure (not a test file).  Built on tests/lstm_f64.py::lnlstm_ref; it works in the
dtype of the weights it is given (float64 for the reference, float32 to measure what float32 costs
the restatement itself).  The searches are the reference's loops (model/decoding.py:225-271 and
:350-425) with the orders the reference leaves to its library fixed as RnntBeamDecoding's docstring
fixes them; tools/gen_golden.py::gen_rnnt_lstm_search pins them to the reference's own classes.

Weights `w`: emb (S,E), in_g / in_b (E), layers = [dict(x2g_w (4H,K), x2g_b (4H) | None, wp (4H,H),
gg / gb (4H), cg / cb (H) | None)], lin_w (D,H), lin_b, out_g / out_b (D), pre_w (V,D), pre_b, and
with an output projection o1_w (inner,V), o1_b, o2_w (V,inner), o2_b; eps_in, eps_lstm, eps_out.
"""
import torch
import torch.nn.functional as F

import lstm_f64 as LF

MARGIN = 1e-3        # the constant of tests/test_gpu_greedy_decode.py


def cast(w, dtype):
    """The weights with every tensor in `dtype`."""
    def c(v):
        if isinstance(v, torch.Tensor):
            return v.to(dtype)
        if isinstance(v, list):
            return [c(x) for x in v]
        if isinstance(v, dict):
            return {k: c(x) for k, x in v.items()}
        return v
    return c(w)


def zero_state(w, R):
    H = w["layers"][0]["wp"].shape[1]
    z = w["emb"].new_zeros(R, H)
    return [(z.clone(), z.clone()) for _ in w["layers"]]


def pred_step(w, tokens, state):
    """One predictor step of R rows: tokens (R) int64, state = [(h, c)] per layer, each (R,H).
    -> (lm (R,V), new state)."""
    E = w["emb"].shape[1]
    x = F.layer_norm(w["emb"][tokens], (E,), w["in_g"], w["in_b"], w["eps_in"])
    new = []
    for p, (h, c) in zip(w["layers"], state):
        gx = F.linear(x, p["x2g_w"], p.get("x2g_b")).unsqueeze(0)
        _, h, c = LF.lnlstm_ref(gx, p["wp"], p.get("gg"), p.get("gb"), p.get("cg"), p.get("cb"),
                                w["eps_lstm"], h, c)
        new.append((h, c))
        x = h
    D = w["lin_w"].shape[0]
    d = F.layer_norm(F.linear(x, w["lin_w"], w["lin_b"]), (D,), w["out_g"], w["out_b"], w["eps_out"])
    return F.linear(d, w["pre_w"], w["pre_b"]), new


def masked_step(w, tokens, emit, parent, state, lm):
    """s2t_lstm_pred_step: row r takes the state of row parent[r]; it steps on tokens[r] where
    emit[r], else keeps that state and that lm row."""
    src = [(h[parent], c[parent]) for h, c in state]
    lm_new, new = pred_step(w, tokens, src)
    m = emit.bool().unsqueeze(1)
    return (torch.where(m, lm_new, lm[parent]),
            [(torch.where(m, hn, h), torch.where(m, cn, c)) for (hn, cn), (h, c) in zip(new, src)])


def joint(w, am_t, lm, act):
    """am_t (V), lm (n,V) -> the joiner's output before the log-softmax (n,V) and the
    pre-activation (n,V)."""
    pre = am_t.unsqueeze(0) + lm
    z = torch.relu(pre) if act == "relu" else torch.tanh(pre)
    if "o1_w" in w:
        z = F.linear(F.linear(z, w["o1_w"], w["o1_b"]), w["o2_w"], w["o2_b"])
    return z, pre


def _start(w):
    return pred_step(w, torch.zeros(1, dtype=torch.int64), zero_state(w, 1))


@torch.no_grad()
def greedy(am, w, act="relu", max_token_step=10):
    """am (T,V), cut to the utterance's length -> (tokens, the smallest top-1 / runner-up gap over
    the visited nodes, how often max_token_step forced a frame on while a symbol was winning).  A
    relu joiner without output projection whose pre-activations are all below -MARGIN is decided
    (every entry exactly 0: the first index), as in tests/test_gpu_greedy_decode.py."""
    am = am.to(w["emb"].dtype)
    lm, state = _start(w)
    out, t, nts, margin, forced = [], 0, 0, float("inf"), 0
    while t < am.shape[0]:
        z, pre = joint(w, am[t], lm, act)
        if act == "relu" and "o1_w" not in w and float(pre.max()) < -MARGIN:
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
            lm, state = pred_step(w, torch.tensor([tok]), state)
    return out, margin, forced


@torch.no_grad()
def beam_search(am, w, act="relu", beam_size=4, cutoff_top_k=4):
    """am (T,V) -> (tokens, score, frames, margin): rnnt_beam_restatement.beam_search over this
    predictor and joiner, with its three-place decision margin."""
    am = am.to(w["emb"].dtype)
    T, V = am.shape
    k = min(int(cutoff_top_k), V)
    lm, state = _start(w)
    beams = [((), (), am.new_zeros(()), state, lm)]          # (tokens, frames, score, state, lm)
    margin = float("inf")
    for t in range(T):
        z, _ = joint(w, am[t], torch.cat([b[4] for b in beams], 0), act)
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
                    cands.append((tokens + (c,), frames + (t,), score + v, st, lmv, c))
        cands.sort(key=lambda x: float(x[2]), reverse=True)  # stable: parent position, then rank
        if len(cands) > beam_size:
            margin = min(margin, float(cands[beam_size - 1][2] - cands[beam_size][2]))
        beams = []
        for tokens, frames, score, st, lmv, c in cands[:beam_size]:
            if c != 0:
                lmv, st = pred_step(w, torch.tensor([c]), st)
            beams.append((tokens, frames, score, st, lmv))
    if len(beams) > 1:
        margin = min(margin, float(beams[0][2] - beams[1][2]))
    tokens, frames, score = beams[0][:3]
    return list(tokens), float(score), list(frames), margin


# ------------------------------------------------------------------ stand-in modules
class PlainPredictor:
    """init_state / streaming_step of the LSTM predictor over the weights above, in plain torch:
    what the module loops of speech2text_amd.model.decoding (and the reference's classes) call."""

    def __init__(self, w):
        self.w = w

    def init_state(self):
        return []

    def streaming_step(self, input, state):
        assert input.shape == (1, 1)
        d = self._d(input.reshape(1).long(), state if len(state) else zero_state(self.w, 1))
        return d[0].reshape(1, 1, -1), d[1]

    def _d(self, tokens, state):
        w = dict(self.w)                                   # the predictor ends before pre_proj
        D = w["lin_w"].shape[0]
        w["pre_w"], w["pre_b"] = torch.eye(D, dtype=w["emb"].dtype), w["emb"].new_zeros(D)
        return pred_step(w, tokens, state)


class PlainJoiner:
    """streaming_step of the joiner; enc_w / enc_b None: the encoder output IS am."""

    def __init__(self, w, act, enc_w=None, enc_b=None):
        self.w, self.act, self.enc_w, self.enc_b = w, act, enc_w, enc_b

    def streaming_step(self, encoder_out, predictor_out):
        am = encoder_out if self.enc_w is None else F.linear(encoder_out, self.enc_w, self.enc_b)
        lm = F.linear(predictor_out, self.w["pre_w"], self.w["pre_b"])            # (beam,1,V)
        z, _ = joint(self.w, am.reshape(-1), lm.squeeze(1), self.act)
        return z.log_softmax(dim=-1)
