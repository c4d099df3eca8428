"""Plain-torch restatement of the layer-norm LSTM layer of csrc/lstm.hip, the yardstick of
tests/test_gpu_lstm_kernel.py.

Test infrastructure (not a test file).  Written from the recurrence in the kernel's header:

    g_t = g_norm(gx_t + h_{t-1} Wp^T)            LayerNorm over the 4H gates
    i, f, z, o = chunk(g_t, 4)
    c_t = c_norm(sigmoid(f) c_{t-1} + sigmoid(i) tanh(z))      LayerNorm over H (carried on)
    h_t = sigmoid(o) tanh(c_t)

It works in the dtype of its inputs (float64 for the reference, float32 to measure what fp32 costs
the reference itself) and leaves the backward to autograd.  tests/test_lstm_f64.py pins it against
torch.nn.LSTM, gradcheck and oracle.heads.lstm_predictor.
"""
import torch
import torch.nn.functional as F


def lnlstm_ref(gx, wp, gg=None, gb=None, cg=None, cb=None, eps=1e-3, h0=None, c0=None):
    """gx (T,B,4H) = x2g(x) (+ bias), wp (4H,H) = p2g.weight; gg / gb (4H) and cg / cb (H) the
    affine parameters of g_norm / c_norm, gg None = no layer norm; h0 / c0 (B,H) or None = zeros.
    -> (hs (T,B,H), h_T, c_T)."""
    T, B, G = gx.shape
    H = G // 4
    h = gx.new_zeros(B, H) if h0 is None else h0
    c = gx.new_zeros(B, H) if c0 is None else c0
    outs = []
    for t in range(T):
        g = gx[t] + h @ wp.t()
        if gg is not None:
            g = F.layer_norm(g, (G,), gg, gb, eps)
        i, f, z, o = g.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(z)
        if gg is not None:
            c = F.layer_norm(c, (H,), cg, cb, eps)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    hs = torch.stack(outs, 0) if outs else gx.new_zeros(0, B, H)
    return hs, h, c


def lnlstm_stack_ref(x, layers, keep=None):
    """The predictor's stack: per layer x -> lnlstm_ref(x2g(x)) -> * keep[l].  `layers` is a list
    of dicts with x2g_w (4H,E), x2g_b (4H) or None, wp, gg, gb, cg, cb (None without layer norm)
    and eps; `keep` a list of (T,B,H) keep masks already scaled by 1 / (1 - p) (None = no
    dropout), one per layer: the module applies its dropout after EVERY layer, the last included.
    x (T,B,E) -> (T,B,H)."""
    for l, p in enumerate(layers):
        gx = F.linear(x, p["x2g_w"], p.get("x2g_b"))
        x, _, _ = lnlstm_ref(gx, p["wp"], p.get("gg"), p.get("gb"), p.get("cg"), p.get("cb"),
                             p.get("eps", 1e-3))
        if keep is not None and keep[l] is not None:
            x = x * keep[l]
    return x
