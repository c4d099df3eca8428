"""Plain-torch restatement of the RNN language model and its task: the LSTM cell of
csrc/lstm_step.hip, the stack, the model, `score` / `score_step`, the masked KL loss and the
top-k accuracy.  The yardstick of tests/test_gpu_lstm_step_kernel.py and tests/test_gpu_rnn_lm.py.

Test infrastructure (not a test file).  Written from torch.nn.LSTM's documented recurrence,

    a_t = gx_t + h_{t-1} W_hh^T,   gx_t = x_t W_ih^T + b_ih + b_hh,   i, f, g, o = chunk(a_t, 4)
    c_t = sigmoid(f) c_{t-1} + sigmoid(i) tanh(g),     h_t = sigmoid(o) tanh(c_t)

and from the task's definition (input tokens[:, :-1], labels tokens[:, 1:], KL(smoothed one-hot ||
softmax) averaged over the valid positions).  It works in the dtype of its inputs (float64 for the
reference, float32 to measure what fp32 costs) and leaves the backward to autograd.
tests/test_rnn_lm_f64.py pins it against the reference model's own outputs
(tests/golden/rnn_lm_ref.npz) and against torch.nn.LSTM.
"""
import math

import torch
import torch.nn.functional as F


def lstm_ref(gx, whh, h0=None, c0=None):
    """gx (T,B,4H), whh (4H,H), h0 / c0 (B,H) or None = zeros -> (hs (T,B,H), h_T, c_T)."""
    T, B, G = gx.shape
    H = G // 4
    h = gx.new_zeros(B, H) if h0 is None else h0
    c = gx.new_zeros(B, H) if c0 is None else c0
    outs = []
    for t in range(T):
        i, f, g, o = (gx[t] + h @ whh.t()).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    hs = torch.stack(outs, 0) if outs else gx.new_zeros(0, B, H)
    return hs, h, c


def num_layers(sd, prefix="_rnn_layer."):
    return sum(1 for k in sd if k.startswith(prefix + "weight_hh_l"))


def stack_ref(x, sd, states=None, keep=None, prefix="_rnn_layer."):
    """x (T,B,E) through every layer; states (h, c) each (L,B,H) or None; keep: list of L - 1
    (T,B,H) keep masks already scaled by 1 / (1 - p), applied after every layer but the last.
    -> (hs (T,B,H), (h_T, c_T) each (L,B,H))."""
    L = num_layers(sd, prefix)
    hT, cT = [], []
    for k in range(L):
        gx = F.linear(x, sd[f"{prefix}weight_ih_l{k}"],
                      sd[f"{prefix}bias_ih_l{k}"] + sd[f"{prefix}bias_hh_l{k}"])
        h0, c0 = (None, None) if states is None else (states[0][k], states[1][k])
        x, h, c = lstm_ref(gx, sd[f"{prefix}weight_hh_l{k}"], h0, c0)
        if keep is not None and k + 1 < L:
            x = x * keep[k]
        hT.append(h)
        cT.append(c)
    return x, (torch.stack(hT, 0), torch.stack(cT, 0))


def logits_ref(sd, tokens, states=None, keep=None):
    """tokens (B,T) -> (logits (B,T,V), states)."""
    x = F.embedding(tokens.t(), sd["_embedding.weight"])
    x, states = stack_ref(x, sd, states, keep)
    return F.linear(x, sd["_logits_layer.weight"], sd["_logits_layer.bias"]).permute(1, 0, 2), states


def non_pad_mask(lens, T):
    return torch.arange(T)[None, :] < lens[:, None]


def score_ref(sd, tokens, lens):
    """(B): sum over the valid positions of log p(tokens[:, t + 1] | tokens[:, :t + 1])."""
    logits, _ = logits_ref(sd, tokens)
    lp = F.log_softmax(logits, dim=-1)[:, :-1].gather(2, tokens[:, 1:].unsqueeze(2)).squeeze(2)
    return (lp * non_pad_mask(lens - 1, tokens.shape[1] - 1)).sum(-1)


def score_step_ref(sd, tokens, states):
    """tokens (beam), states (h, c) -> (log_probs (beam,V), states)."""
    logits, states = logits_ref(sd, tokens.unsqueeze(-1), states)
    return F.log_softmax(logits, dim=-1).squeeze(1), states


def masked_kl_ref(logits, labels, lens, label_smoothing, scale=1.0):
    """KL(smoothed one-hot || softmax(scale * logits)) summed over the classes, mean over the
    positions t < lens[b].  logits (B,T,V), labels (B,T)."""
    V = logits.shape[-1]
    lp = F.log_softmax(logits * scale, dim=-1)
    a, b = label_smoothing / (V - 1), 1.0 - label_smoothing
    q = torch.full_like(lp, a).scatter_(-1, labels.unsqueeze(-1), b)
    ent = (V - 1) * (a * math.log(a) if a > 0 else 0.0) + (b * math.log(b) if b > 0 else 0.0)
    row = ent - (q * lp).sum(-1)
    m = non_pad_mask(lens, logits.shape[1]).to(row.dtype)
    return (row * m).sum() / m.sum()


def nnlm_io(text, text_len):
    return text[:, :-1], text[:, 1:], text_len - 1


def nnlm_loss_ref(sd, text, text_len, label_smoothing, keep=None):
    inp, lab, lens = nnlm_io(text, text_len)
    logits, _ = logits_ref(sd, inp, keep=keep)
    return masked_kl_ref(logits, lab, lens, label_smoothing)


def topk_acc_ref(logits, labels, lens, k):
    """share of the valid positions whose label is among the k largest logits (+1e-7 below)."""
    top = logits.topk(k, dim=-1).indices
    m = non_pad_mask(lens, logits.shape[1])
    hit = (top == labels.unsqueeze(-1)).any(-1) & m
    return hit.sum().double() / (m.sum().double() + 1e-7)


def grads_ref(sd, loss_fn):
    """-> (loss, {name: gradient}) of loss_fn(sd with grad-requiring copies)."""
    leaf = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    loss = loss_fn(leaf)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in leaf.items()}
