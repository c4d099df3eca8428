"""Plain restatements of the zipformer's streaming operations (csrc/zip_elem.hip: Swoosh, BiasNorm,
BiasNorm + bypass, the Balancer's backward; csrc/zip_glue.hip: bypass, SimpleDownsample, upsample +
bypass, the nonlinear attention's gate / out passes, the attention's row constants, the parameter
gradient commit, the add), the yardstick of tests/test_gpu_zip_stream_kernels.py.

Test infrastructure (not a test file).  Every function is written in torch ops that follow the
dtype of their arguments: in float64 they are the reference, in float32 they measure what float32
costs the reference itself (tests/test_zip_f64.py).  Nothing here is shaped like the kernels: no
max(z, 0) + log1p(exp(-|z|)), no E[x^2] sums kept per workgroup, no closed form of the Balancer.
Gradients come from autograd over these functions.
"""
import torch

SWOOSH = {True: (4.0, 0.035), False: (1.0, 0.313261687)}     # is_l -> (offset, constant)


def swoosh_ref(x, is_l):
    off, c = SWOOSH[is_l]
    return torch.logaddexp(torch.zeros((), dtype=x.dtype), x - off) - 0.08 * x - c


def swoosh_grad_ref(x, is_l):
    """d swoosh / dx in closed form (autograd over swoosh_ref gives the same; pinned on the CPU)."""
    return torch.sigmoid(x - SWOOSH[is_l][0]) - 0.08


def biasnorm_ref(x, bias, log_scale):
    """-> (y, scales): scales = mean((x - bias)^2 over the last axis)^-1/2 * exp(log_scale), y = x * scales."""
    d = x - bias
    scales = (d * d).mean(-1) ** -0.5 * log_scale.exp()
    return x * scales.unsqueeze(-1), scales


def biasnorm_tb_ref(x, bias, log_scale):
    """x (B,T,D) batch-major -> (y (T,B,D) time-major, scales (B,T)): the plain one plus a transpose."""
    y, scales = biasnorm_ref(x, bias, log_scale)
    return y.transpose(0, 1), scales


def bypass_ref(orig, src, scale, fm=None):
    """orig + (src - orig) * scale[c], times the feature mask row of every row where fm (same shape
    as orig, or broadcastable to it) is given."""
    out = orig + (src - orig) * scale
    return out if fm is None else out * fm


def bypass_acc_ref(orig, src, scale, acc_in):
    """The bypass whose gradient for orig additionally receives acc_in: acc_in enters as a term whose
    derivative with respect to orig is acc_in (orig * acc_in, acc_in constant)."""
    return bypass_ref(orig, src, scale), (orig * acc_in.detach()).sum()


def norm_bypass_ref(x, bias, log_scale, orig, bscale, fm=None):
    """-> (out, scales): bypass of orig and BiasNorm(x), times the feature mask."""
    y, scales = biasnorm_ref(x, bias, log_scale)
    return bypass_ref(orig, y, bscale, fm), scales


def downsample_ref(src, w, ds, batch_major=False):
    """SimpleDownsample on src (T,B,C) with the weights w (ds,) already normalised: frames padded to
    a multiple of ds by repeating the last one, out[tt] = sum_k w[k] src[tt ds + k]; (dT,B,C), or
    (B,dT,C) with batch_major."""
    T, B, C = src.shape
    dT = (T + ds - 1) // ds
    pad = dT * ds - T
    s = torch.cat((src, src[T - 1:].expand(pad, B, C)), dim=0).reshape(dT, ds, B, C)
    out = (s * w.view(1, ds, 1, 1)).sum(dim=1)
    return out.transpose(0, 1) if batch_major else out


def upsample_bypass_ref(orig, src, scale, up):
    """orig (T,B,C), src (ceil(T / up),B,C): every source frame repeated up times, cut to T frames,
    then the bypass."""
    T = orig.shape[0]
    Ts, B, C = src.shape
    rep = src.unsqueeze(1).expand(Ts, up, B, C).reshape(Ts * up, B, C)[:T]
    return bypass_ref(orig, rep, scale)


def nonlin_gate_ref(u):
    """u (T,B,3C) = [s | x | y] -> xs (B,T,C) = x * tanh(s), batch-major."""
    s, x, _ = u.chunk(3, dim=-1)
    return (x * torch.tanh(s)).transpose(0, 1)


def nonlin_out_ref(z, u):
    """z (B,T,C) batch-major, u (T,B,3C) -> o (T,B,C) = z^T * y."""
    return z.transpose(0, 1) * u.chunk(3, dim=-1)[2]


def attn_delta_pairs_ref(W, dW0, pairs, T, B, H):
    """The softmax-backward row constants: delta[h,b,i] = sum over the pairs (dO, O), each (T,B,H dv),
    of sum_d dO[i,b,h,d] O[i,b,h,d], plus for head 0 sum_j W[0,b,i,j] dW0[b,i,j] where dW0 is given."""
    delta = torch.zeros(H, B, T, dtype=W.dtype)
    for dO, O in pairs:
        dv = O.shape[-1] // H
        delta = delta + (dO * O).reshape(T, B, H, dv).sum(-1).permute(2, 1, 0)
    if dW0 is not None:
        delta = delta + torch.cat(((W[0] * dW0).sum(-1).unsqueeze(0), torch.zeros(H - 1, B, T, dtype=W.dtype)))
    return delta


def commit_ref(x, d, grad, lo, hi, limit):
    """-> (grad + d', zeros): d' is d after limit_param_value's backward (oracle.zipformer._LimitParam:
    the sign flips where the step would push x further outside [lo, hi]) where limit, else d."""
    v = d
    if limit:
        v = v * torch.where(torch.logical_and(v > 0, x < lo), -1.0, 1.0).to(d.dtype)
        v = v * torch.where(torch.logical_and(v < 0, x > hi), -1.0, 1.0).to(d.dtype)
    return grad + v, torch.zeros_like(d)


def add_ref(a, b):
    return a + b


def balancer_bwd_ref(x, g, min_mean, max_mean, min_rms, max_rms, grad_scale, swoosh=None):
    """Balancer backward on x, g (rows, C), channels last, as oracle.zipformer._Balancer.backward
    states it (model/layer/scaling.py:741-789): autograd through the loss inside backward, with the
    clamps -- a clamped statistic has derivative zero -- in the dtype of x (no cast to float32).
    swoosh (True: SwooshL, False: SwooshR): g is the gradient w.r.t. swoosh(x) and is taken through
    the activation's derivative first."""
    if swoosh is not None:
        g = g * swoosh_grad_ref(x, swoosh)
    with torch.enable_grad():
        xd = x.detach().clone().requires_grad_(True)
        uvar = (xd ** 2).mean(dim=0, keepdim=True)
        mean = xd.mean(dim=0, keepdim=True)
        std = (uvar - mean * mean).clamp(min=1.0e-20).sqrt()
        rms = uvar.clamp(min=1.0e-20).sqrt()
        m = mean / std
        loss = (m - m.clamp(min=min_mean, max=max_mean)).abs() + \
            (rms.clamp(min=min_rms, max=max_rms) / rms).log().abs()
        loss.backward(gradient=torch.ones_like(loss))
    lg = xd.grad
    lg_rms = (lg ** 2).mean(dim=0, keepdim=True).sqrt().clamp(min=1.0e-20)
    lg = lg * (grad_scale / lg_rms)
    return g + g.abs() * lg


def balancer_bwd_closed_form(x, g, min_mean, max_mean, min_rms, max_rms, grad_scale, swoosh):
    """reference model/layer/scaling.py:741-789 in closed form (as zk.balancer_backward's torch path), fp64.
    Right on live channels only: where a variance is at the 1e-20 clamp it multiplies by 1 / (std var)
    what autograd sees as a constant.  tests/test_zip_f64.py pins the autograd restatement
    (balancer_bwd_ref above, the yardstick) to it on live channels."""
    x, g = x.double(), g.double()
    if swoosh is not None:
        g = g * (torch.sigmoid(x - (4.0 if swoosh else 1.0)) - 0.08)
    n = x.shape[0]
    mean = x.mean(0, keepdim=True)
    uvar = (x * x).mean(0, keepdim=True)
    var = (uvar - mean * mean).clamp(min=1.0e-20)
    std, rms = var.sqrt(), uvar.clamp(min=1.0e-20).sqrt()
    m = mean / std
    s_m = torch.sign(m - m.clamp(min=min_mean, max=max_mean))
    s_r = -torch.sign((rms.clamp(min=min_rms, max=max_rms) / rms).log())
    a = s_m / n * (1.0 / std + mean * mean / (std * var))
    b = -s_m / n * mean / (std * var) + s_r / n / (rms * rms)
    lg_rms = (a * a + 2 * a * b * mean + b * b * uvar).clamp(min=0).sqrt().clamp(min=1.0e-20)
    return g + g.abs() * (a + b * x) * (grad_scale / lg_rms)
