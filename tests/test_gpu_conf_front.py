"""GPU: the conformer Subsampling's first convolution (csrc/conf_front.hip: Conv2d(1, C, 3,
stride 2) + ReLU as a direct stencil kernel, and its one-pass weight / bias gradient with a
recomputed ReLU mask) through conf_kernels.conv1_relu, against
F.relu(F.conv2d(x[:, None].double(), w.double(), b.double(), stride=2)) with autograd.

The thread mapping depends on cg = C / 4 channel quads and npl = 256 / cg position lanes; both
kernels grid-stride once B T1 F1 / npl exceeds their workgroup caps (4096 forward, 1024 weight
gradient); the fold kernel ACCUMULATES into dw / db.

The weight-gradient kernel recomputes the ReLU mask in float32: a pre-activation that float64
puts within rounding of zero may fall on the other side, and a flipped mask changes the sum by a
whole term.  So the incoming gradient d is set to exactly 0 wherever the float64 pre-activation
has |z| < 1e-4 (at most 0.1 % of the positions, asserted; about 0.01 % expected).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, T, F, C)
SHAPES = [
    (1, 3, 3, 4),          # one output position, one channel quad
    (2, 4, 5, 8),
    (2, 5, 80, 16),        # odd T
    (3, 37, 79, 64),       # odd F
    (3, 301, 80, 256),     # C2's width; 17 550 positions at 4 per workgroup: above both caps
    (2, 50, 80, 512),
    (2, 201, 80, 1024),    # one position per workgroup pass; 7 800 positions: above both caps
]
FWD_TOL = 1e-5             # of max |ref|: the project's bound for its 9- to 31-tap direct kernels
GRAD_TOL = 2e-5
NEAR_ZERO = 1e-4


@functools.lru_cache(maxsize=None)
def _case(B, T, Fq, C):
    """Seeded inputs and the float64 results (computed once, shared, not to be modified)."""
    g = torch.Generator().manual_seed(B * 1000003 + T * 1009 + Fq * 31 + C)
    x = torch.randn(B, T, Fq, generator=g) * 2 + 0.3
    w = torch.randn(C, 1, 3, 3, generator=g) / 3
    b = torch.randn(C, generator=g) * 0.2
    T1, F1 = (T - 3) // 2 + 1, (Fq - 3) // 2 + 1
    d = torch.randn(B, C, T1, F1, generator=g)
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    z = F.conv2d(xd[:, None], wd, bd, stride=2)
    near = z.detach().abs() < NEAR_ZERO
    d = d.masked_fill(near, 0.0)
    out = F.relu(z)
    (out * d.double()).sum().backward()
    return dict(x=x, w=w, b=b, d=d, out=out.detach(), dw=wd.grad, db=bd.grad, dx=xd.grad,
                share=near.double().mean().item())


def _err(got, ref):
    ref = ref.double()
    return float((got.detach().double().cpu() - ref).abs().max() / ref.abs().max())


def _conv(c, dev):
    C = c["w"].shape[0]
    conv = torch.nn.Conv2d(1, C, 3, stride=2).to(dev)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
        conv.bias.copy_(c["b"])
    return conv


@pytest.mark.parametrize("B,T,Fq,C", SHAPES)
def test_conv1_relu_forward_and_gradients(dev, B, T, Fq, C):
    from speech2text_amd import conf_kernels as ck
    c = _case(B, T, Fq, C)
    print(f"positions with |z| < {NEAR_ZERO}: {100 * c['share']:.4f} %")
    assert c["share"] <= 1e-3
    conv = _conv(c, dev)
    x = c["x"].to(dev).requires_grad_(True)
    assert ck.conv1_relu_ok(conv, x)
    out = ck.conv1_relu(x, conv)
    assert type(out.grad_fn).__name__ in ("_Conv1ReluBackward", "PermuteBackward0")
    assert out.shape == c["out"].shape
    assert out.permute(0, 2, 3, 1).is_contiguous()            # the kernel's channels-last view
    e = _err(out, c["out"])
    print(f"out err {e:.3e}")
    assert e <= FWD_TOL
    (out * c["d"].to(dev)).sum().backward()
    for k, got in (("dw", conv.weight.grad), ("db", conv.bias.grad), ("dx", x.grad)):
        e = _err(got, c[k])
        print(f"{k} err {e:.3e}")
        assert e <= GRAD_TOL, (k, e)


@pytest.mark.parametrize("store", [False, True], ids=["returned", "slots"])
@pytest.mark.parametrize("B,T,Fq,C", [SHAPES[1], SHAPES[3], SHAPES[4], SHAPES[6]])
def test_conv1_relu_gradients_accumulate(dev, B, T, Fq, C, store):
    """dw / db pre-filled with non-zero values of the gradient's own magnitude: the result is the
    old values plus the gradient, with the parameters in a flat store (the fold kernel adds into
    the slots) and outside one (the gradients are returned and autograd adds)."""
    from speech2text_amd import conf_kernels as ck
    from speech2text_amd import flat
    c = _case(B, T, Fq, C)
    conv = _conv(c, dev)
    if store:
        flat.get_store([conv.weight, conv.bias])
        assert flat.owned(conv.weight) and flat.owned(conv.bias)
    g = torch.Generator().manual_seed(C)
    old_w = (torch.randn(C, 1, 3, 3, generator=g) * 0.5 * c["dw"].abs().max()).float()
    old_b = (torch.randn(C, generator=g) * 0.5 * c["db"].abs().max()).float()
    if store:
        conv.weight.grad.copy_(old_w)
        conv.bias.grad.copy_(old_b)
        slot_w, slot_b = conv.weight.grad.data_ptr(), conv.bias.grad.data_ptr()
    else:
        conv.weight.grad, conv.bias.grad = old_w.to(dev), old_b.to(dev)
    out = ck.conv1_relu(c["x"].to(dev), conv)
    (out * c["d"].to(dev)).sum().backward()
    if store:
        assert conv.weight.grad.data_ptr() == slot_w and conv.bias.grad.data_ptr() == slot_b
    for k, got, old in (("dw", conv.weight.grad, old_w), ("db", conv.bias.grad, old_b)):
        want = old.double() + c[k]
        e = float((got.double().cpu() - want).abs().max() / c[k].abs().max())
        print(f"{k} err {e:.3e}")
        assert e <= GRAD_TOL, (k, e)


@pytest.mark.parametrize("C,bias", [(12, True), (144, True), (2048, True), (16, False)])
def test_subsampling_outside_the_gate_gives_torchs_result(dev, C, bias, arith_bound):
    """C % 4 != 0 / 256 % (C / 4) != 0 / C > 1024 / a conv without bias: conv1_relu_ok is false
    and the conformer Subsampling computes the same function through the library convolution.
    Held to the module composition in float64; the second convolution and the Linear behind it
    are the project's split-bf16 GEMMs, hence arith_bound (2e-5 of max |ref| with the six-product
    arithmetic pinned, the two-piece policy's 10 x otherwise)."""
    from speech2text_amd import conf_kernels as ck
    from speech2text_amd.model.encoder.conformer import Subsampling
    torch.manual_seed(C)
    B, T, Fq = 2, 15, 11
    sub = Subsampling(Fq, C, 4)
    if not bias:
        sub.conv[0] = torch.nn.Conv2d(1, C, 3, 2, bias=False)
    ref = Subsampling(Fq, C, 4).double()
    ref.conv[0] = torch.nn.Conv2d(1, C, 3, 2, bias=bias).double()
    ref.load_state_dict({k: v.double() for k, v in sub.state_dict().items()})
    x = torch.randn(B, T, Fq) * 2 + 0.3
    lens = torch.tensor([T, T - 4])
    y = ref.linear(ref.conv(x.double()[:, None]).permute(0, 2, 1, 3).flatten(2))
    ln = ref.subsampled_length(lens)
    y = y.masked_fill((torch.arange(y.shape[1])[None] >= ln[:, None])[..., None], 0.0)
    sub.to(dev)
    xd = x.to(dev)
    assert not ck.conv1_relu_ok(sub.conv[0], xd)
    out, ol = sub(xd, lens.to(dev))
    assert torch.equal(ol.cpu(), ln)
    e = _err(out, y.detach())
    print(f"C={C} bias={bias}: err {e:.3e}")
    assert e <= 2e-5 * arith_bound
