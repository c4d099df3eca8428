"""Plain restatements of the conformer block's element-wise, normalisation and attention operations
(csrc/conf_elem.hip, csrc/conf_attn.hip), the yardstick of tests/test_gpu_conf_kernels.py.

Test infrastructure (not a test file).  Every function is written in torch ops that follow the
dtype of their arguments: in float64 they are the reference, in float32 they measure what float32
costs the reference itself (tests/test_conf_f64.py).  Nothing here is shaped like the kernels: no
tiles, no running maxima, no E[x^2] - mean^2.  Gradients come from autograd over these functions.
"""
import math

import torch


def layernorm_stats(x, eps):
    """-> (mean, rstd) per row: the mean first, then the variance of the centred values."""
    mean = x.mean(-1, keepdim=True)
    xc = x - mean
    var = (xc * xc).mean(-1, keepdim=True)
    return mean.squeeze(-1), (1.0 / torch.sqrt(var + eps)).squeeze(-1)


def layernorm_ref(x, y, alpha, gamma, beta, eps):
    """-> (xsum, out): xsum = x + alpha * y (x itself when y is None), out = LayerNorm(xsum) over
    the last axis with the optional affine gamma / beta."""
    xsum = x if y is None else x + alpha * y
    mean = xsum.mean(-1, keepdim=True)
    xc = xsum - mean
    var = (xc * xc).mean(-1, keepdim=True)
    out = xc / torch.sqrt(var + eps)
    if gamma is not None:
        out = out * gamma
    if beta is not None:
        out = out + beta
    return xsum, out


def silu_ref(x):
    return x * torch.sigmoid(x)


def silu_grad_ref(x):
    """d silu / dx in closed form (autograd over silu_ref gives the same; pinned on the CPU)."""
    s = torch.sigmoid(x)
    return s * (1 + x * (1 - s))


def bn_silu_ref(x, gamma, beta, eps):
    """Training-mode BatchNorm1d + SiLU on channel-last (rows, C) -> (y, mean, biased variance,
    unbiased variance): statistics over the rows, the variance by the two-pass textbook form.
    One row: the unbiased variance is the biased one (torch refuses that batch)."""
    n = x.shape[0]
    mean = x.mean(0)
    xc = x - mean
    var = (xc * xc).mean(0)
    unb = var * n / (n - 1) if n > 1 else var
    y = silu_ref(xc / torch.sqrt(var + eps) * gamma + beta)
    return y, mean, var, unb


def bn_silu_eval_ref(x, mean, var, gamma, beta, eps):
    """Evaluation-mode BatchNorm1d + SiLU with the given (running) statistics."""
    return silu_ref((x - mean) / torch.sqrt(var + eps) * gamma + beta)


def attn_ref(qkv, lens, H, mask=None):
    """nn.MultiheadAttention's core on qkv (T,B,3D) = [q | k | v] -> (T,B,D): per utterance and
    head softmax(q k^T / sqrt(dh)) v, keys at or past lens[b] masked (lens None: all T keys; a
    length above T is T).  All T query rows are computed, padded ones included.  mask: (B,H,T,T)
    keep-scale factors multiplied onto the probabilities (dropout), or None.
    An utterance with lens[b] == 0 has no key to attend to: torch's softmax gives NaN there, the
    kernel documents zeros (output and every gradient), and zeros are what this returns."""
    T, B, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(T, B, H, dh).permute(1, 2, 0, 3) for i in range(3))
    s = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(dh)
    live = None
    if lens is not None:
        lens = lens.to(torch.int64)
        kpm = torch.arange(T).view(1, 1, 1, T) >= lens.view(B, 1, 1, 1)
        live = (lens > 0).view(B, 1, 1, 1)
        s = s.masked_fill(kpm & live, float("-inf"))
    p = s.softmax(-1)
    if live is not None:
        p = p * live.to(p.dtype)
    if mask is not None:
        p = p * mask
    return torch.matmul(p, v).permute(2, 0, 1, 3).reshape(T, B, D)
