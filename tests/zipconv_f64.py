"""Plain restatements of the zipformer's convolution kernels (csrc/zip_conv.hip: the conv module's
gate + padding mask + chunk-causal depthwise conv; csrc/zip_front.hip: the frontend's 1 -> 8 and
8 -> 32 convs, the channel-last depthwise 3x3 / 7x7 conv with its weight gradient, col2im), the
yardstick of tests/test_gpu_zip_conv_kernels.py.

Test infrastructure (not a test file).  Every function is written in torch ops that follow the dtype
of their arguments: in float64 they are the reference, in float32 they measure what float32 costs
the reference itself (tests/test_zipconv_f64.py).  Nothing here is shaped like the kernels: no tiles,
no register windows, no rings; a convolution is a sum of shifted slices.  Gradients come from
autograd over these functions (dwconv2d_wgrad_ref is the one closed form: the tall weight-gradient
case would keep 49 copies of its input alive under autograd; it is pinned against autograd on the CPU).
Swoosh is zip_f64.swoosh_ref.
"""
import torch
import torch.nn.functional as F

from zip_f64 import swoosh_ref  # noqa: F401  (the conv module's activation output)


def conv_module_ref(u, C, gate_off, mask, chunk, K, wc, bc, wk, bk, scale):
    """u (T,B,ld): x = u[..., :C], gate pre-activation u[..., gate_off:gate_off+C] (gate_off < 0:
    none); mask (B,T) bool, True = padded frame, or None; wc (C,(K+1)/2) or None, wk (C,K), bc / bk
    (C) or None, scale (2,C,K) or None  ->  y (T,B,C):
        xg = x * sigmoid(gate), zero on padded frames
        y  = causal_conv(xg) + chunkwise_conv(xg) * (1 + left_edge + right_edge)
    Chunks are `chunk` frames; the chunkwise conv sees zeros outside its chunk.  With wc and scale None
    and chunk >= T this is nn.Conv1d(C, C, K, groups=C, padding=K // 2)."""
    T, B, _ = u.shape
    halo = K // 2
    x = u[..., :C]
    if gate_off >= 0:
        x = x * torch.sigmoid(u[..., gate_off:gate_off + C])
    if mask is not None:
        x = torch.where(mask.t().unsqueeze(-1), torch.zeros((), dtype=x.dtype), x)
    chunk = min(chunk, T)
    nch = (T + chunk - 1) // chunk
    xc = F.pad(x, (0, 0, 0, 0, 0, nch * chunk - T)).reshape(nch, chunk, B, C)
    xc = F.pad(xc, (0, 0, 0, 0, halo, halo))                       # zeros around every chunk
    y = sum(xc[:, j:j + chunk] * wk[:, j] for j in range(K))
    if bk is not None:
        y = y + bk
    if scale is not None:
        le, re = scale[0].t(), scale[1].t()                        # (K,C): position from the edge
        if chunk < K:
            le, re = le[:chunk], re[K - chunk:]
        else:
            z = torch.zeros(chunk - K, C, dtype=scale.dtype)
            le, re = torch.cat((le, z)), torch.cat((z, re))
        y = y * (1.0 + (le + re)).reshape(1, chunk, 1, C)
    y = y.reshape(nch * chunk, B, C)[:T]
    if wc is not None:
        xl = F.pad(x, (0, 0, 0, 0, halo, 0))                       # frames before 0 are zero
        yc = sum(xl[j:j + T] * wc[:, j] for j in range(wc.shape[1]))
        if bc is not None:
            yc = yc + bc
        y = y + yc
    return y


def dwconv2d_ref(x, w, bias=None, flip=False, add=None):
    """Channel-last depthwise conv, zero 'same' padding: x (N,H,W,C), w (C,KH,KW) ->
    y[n,h,w,c] = bias[c] + add[n,h,w,c] + sum_ij w[c,i,j] x[n,h+i-KH/2,w+j-KW/2,c]; flip: the taps
    reversed in both directions (the data gradient of the unflipped conv)."""
    N, H, W, C = x.shape
    KH, KW = w.shape[1:]
    if flip:
        w = w.flip(1, 2)
    xp = F.pad(x, (0, 0, KW // 2, KW // 2, KH // 2, KH // 2))
    y = sum(xp[:, i:i + H, j:j + W] * w[:, i, j] for i in range(KH) for j in range(KW))
    if bias is not None:
        y = y + bias
    return y if add is None else y + add


def dwconv2d_wgrad_ref(x, dy, KH, KW):
    """-> (dw (C,KH,KW), db (C)) of sum(dwconv2d_ref(x, w, b) * dy), in closed form."""
    N, H, W, C = x.shape
    xp = F.pad(x, (0, 0, KW // 2, KW // 2, KH // 2, KH // 2))
    dw = torch.stack([torch.stack([(xp[:, i:i + H, j:j + W] * dy).sum((0, 1, 2)) for j in range(KW)], -1)
                      for i in range(KH)], 1)
    return dw, dy.sum((0, 1, 2))


def conv3x3_c1_ref(x, w, bias, pw):
    """Conv2d(1, CO, 3, padding=(0, pw)) channel-last: x (B,H,W), w (CO,1,3,3) -> (B,H-2,W+2pw-2,CO)."""
    B, H, W = x.shape
    Ho, Wo = H - 2, W + 2 * pw - 2
    xp = F.pad(x, (pw, pw))
    y = sum(xp[:, kh:kh + Ho, kw:kw + Wo].unsqueeze(-1) * w[:, 0, kh, kw] for kh in range(3) for kw in range(3))
    return y if bias is None else y + bias


def conv3x3_s2_ref(x, w, bias):
    """Conv2d(CI, CO, 3, stride 2) channel-last: x (B,H,W,CI), w (CO,CI,3,3) -> (B,Ho,Wo,CO)."""
    B, H, W, CI = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    y = sum(torch.einsum("bhwi,oi->bhwo", x[:, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2], w[:, :, kh, kw])
            for kh in range(3) for kw in range(3))
    return y if bias is None else y + bias


def col2im3x3_ref(dc, H, W, sh, sw):
    """dc (B,Ho,Wo,3,3,C), the gradient of every 3x3 patch entry -> dx (B,H,W,C): each entry added to
    the input position it was taken from, (ho sh + kh, wo sw + kw)."""
    B, Ho, Wo, _, _, C = dc.shape
    dx = torch.zeros(B, H, W, C, dtype=dc.dtype)
    for kh in range(3):
        for kw in range(3):
            dx[:, kh:kh + sh * (Ho - 1) + 1:sh, kw:kw + sw * (Wo - 1) + 1:sw] += dc[:, :, :, kh, kw]
    return dx
