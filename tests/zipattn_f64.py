"""Plain restatements of what csrc/zip_attn.hip and csrc/whiten.hip compute, in the dtype of their
arguments (float64 for the yardstick, float32 for its cost): the reference of
tests/test_gpu_zip_attn_kernels.py.  Test infrastructure, not a test file; nothing here imports the
package under test.  tests/test_zipattn_f64.py pins every function at 1e-12 against independent
statements (the oracle's composition, index loops, autograd, gradcheck).

Layouts are the kernels': qkp (T,B,H (2 qd + pd)) = [q: H qd | k: H qd | p: H pd], pos (2T-1, H pd),
kpm (B,T) bool (True = padded key), amask (T,T) bool (True = masked), W (H,B,T,T), values (T,B,H dv).
"""
import torch


# ------------------------------------------------------------------ attention weights
def raw_scores(qkp, pos, H, qd, pd):
    """s[h,b,i,j] = q[i,b,h] . k[j,b,h] + p[i,b,h] . pos[(T-1) - i + j, h], before any mask."""
    T, B, _ = qkp.shape
    q = qkp[..., :H * qd].reshape(T, B, H, qd)
    k = qkp[..., H * qd:2 * H * qd].reshape(T, B, H, qd)
    s = torch.einsum("ibhd,jbhd->hbij", q, k)
    if pos is not None and pd > 0:
        p = qkp[..., 2 * H * qd:].reshape(T, B, H, pd)
        rel = torch.einsum("ibhd,rhd->hbir", p, pos.reshape(2 * T - 1, H, pd))       # every offset
        idx = (T - 1) - torch.arange(T).unsqueeze(1) + torch.arange(T).unsqueeze(0)
        s = s + torch.gather(rel, 3, idx.expand(H, B, T, T))
    return s


def attn_weights(qkp, pos, kpm, amask, H, qd, pd):
    """-> (W, raw): raw scores, masked_fill(-1000) by the attention mask and by the padding mask,
    softmax over the keys.  The raw scores are what the penalty flag looks at."""
    raw = raw_scores(qkp, pos, H, qd, pd)
    s = raw
    if amask is not None:
        s = s.masked_fill(amask, -1000.0)
    if kpm is not None:
        s = s.masked_fill(kpm.unsqueeze(1), -1000.0)
    return s.softmax(dim=-1), raw


def attn_grads(qkp, pos, kpm, amask, H, qd, pd, dW):
    """Autograd of attn_weights against a given dW -> (dqkp, dpos or None)."""
    q = qkp.detach().clone().requires_grad_(True)
    p = None if pos is None else pos.detach().clone().requires_grad_(True)
    W, _ = attn_weights(q, p, kpm, amask, H, qd, pd)
    (W * dW).sum().backward()
    dpos = None
    if p is not None:
        dpos = p.grad if p.grad is not None else torch.zeros_like(p)
    return q.grad, dpos


def factored_dw(T, B, H, dW, dW0, pairs):
    """dW[h,b,i,j] (+ dW0[b,i,j] on head 0) + sum_c dO_c[i,b,h,:] . V_c[j,b,h,:], materialised."""
    tot = None
    for dO, V in pairs:
        dv = dO.shape[-1] // H
        t = torch.einsum("ibhd,jbhd->hbij", dO.reshape(T, B, H, dv), V.reshape(T, B, H, dv))
        tot = t if tot is None else tot + t
    if dW is not None:
        tot = dW if tot is None else tot + dW
    if dW0 is not None:
        tot = tot.clone()
        tot[0] = tot[0] + dW0
    return tot


def attn_apply(W, v, H, transpose):
    """transpose False: out[i,b,h] = sum_j W[h,b,i,j] v[j,b,h]; True: out[j,b,h] = sum_i W[h,b,i,j] v[i,b,h]."""
    T, B, _ = v.shape
    vv = v.reshape(T, B, H, -1)
    out = torch.einsum("hbij,ibhd->jbhd" if transpose else "hbij,jbhd->ibhd", W, vv)
    return out.reshape(T, B, -1)


# ------------------------------------------------------------------ Whiten
def _scal(cov, C):
    md = torch.diagonal(cov, dim1=1, dim2=2).sum() / C
    covsq = (cov * cov).sum() / C
    denom = md * md + 1.0e-20
    return torch.stack((md, covsq, denom, covsq / denom))


def whiten_stats(xtx, colsum, n, G, cg):
    """From the metric kernel's own inputs: xtx (C,C) = x^T x, colsum (C), n rows ->
    cov (G,cg,cg) = per-group xtx - mean colsum^T, mean (C), scal = [mean diag, sum cov^2 / C, denom, metric]."""
    C = G * cg
    mean = colsum / n
    full = xtx - mean.unsqueeze(1) * colsum.unsqueeze(0)
    cov = torch.stack([full[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] for g in range(G)])
    return cov, mean, _scal(cov, C)


def whiten_from_x(x, G):
    """The reference's centred form: cov_g = (x_g - mean)^T (x_g - mean) -> cov, mean, scal."""
    n, C = x.shape
    cg = C // G
    mean = x.mean(0)
    xc = (x - mean).reshape(n, G, cg).transpose(0, 1)
    cov = torch.matmul(xc.transpose(1, 2), xc)
    return cov, mean, _scal(cov, C)


def whiten_dcov(cov, mean, scal, G, cg):
    """dcov (C,C), block diagonal = 4 / C (cov / denom - covsq md / denom^2 I), such that the metric's
    gradient with respect to x is (x - mean) dcov = x dcov + bias;  bias = -mean dcov."""
    C = G * cg
    md, covsq, denom = scal[0], scal[1], scal[2]
    eye = torch.eye(cg, dtype=cov.dtype)
    blocks = (4.0 / C) * (cov / denom - (covsq * md / (denom * denom)) * eye)
    dcov = torch.block_diag(*blocks)
    return dcov, -(mean @ dcov)


def whiten_apply(g, pg, grad_scale):
    """-> out = g + pg grad_scale |g| / (|pg| + 1e-20), and (|g|^2, |pg|^2)."""
    sg, sp = (g * g).sum(), (pg * pg).sum()
    scale = grad_scale * (sg.sqrt() / (sp.sqrt() + 1.0e-20))
    return g + pg * scale, torch.stack((sg, sp))


def limit_param_grad(x, g, lo, hi):
    """The sign of g flipped where (g > 0 and x < lo), then where (the result < 0 and x > hi)."""
    g = torch.where((g > 0) & (x < lo), -g, g)
    return torch.where((g < 0) & (x > hi), -g, g)
