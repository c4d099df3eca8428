"""Conformer encoder (mirror of the reference's model/encoder/conformer.py).

`Subsampling` (:32-135) is reference-authored; the conformer stack is
torchaudio.models.Conformer (torchaudio 0.13.1, not vendored: the block structure restated here
is the published one -- FFN(0.5) -> MHSA -> conv module -> FFN(0.5) -> LayerNorm, conv module =
LayerNorm -> pointwise(D->2D) -> GLU -> depthwise(k, pad k//2) -> BatchNorm1d|GroupNorm ->
SiLU -> pointwise -> dropout; PARITY UNPINNED).  Parameter names follow torchaudio's so
checkpoints interchange.  Everything runs time-major (T,B,D) on hand-written HIP kernels:
LayerNorm / SiLU / BatchNorm+SiLU (conf_elem.hip), the flash-style MFMA attention core
(conf_attn.hip), GLU + depthwise conv (zip_conv.hip); dense GEMMs are hipBLASLt (forward, data
gradient) and the TN MFMA kernel (weight gradient).  In training a layer is ONE autograd node
(speech2text_amd/conf_layer.py); the module-by-module form below serves evaluation, dropout > 0
and models whose parameters are not in a FlatStore, with the same kernels one op at a time.
"""
import dataclasses
from typing import Tuple


import torch
import torch.nn as nn
import torch.nn.functional as F

from speech2text_amd import conf_kernels as ck
from speech2text_amd import conf_layer
from speech2text_amd import zip_kernels as zk


@dataclasses.dataclass
class ConformerConfig:
    bn_cmvn: bool = False
    feats_dim: int = 80
    subsampling_rate: int = 4
    input_dim: int = 512
    num_heads: int = 8
    ffn_dim: int = 2048
    num_layers: int = 8
    depthwise_conv_kernel_size: int = 31
    dropout: float = 0.0
    use_group_norm: bool = False
    convolution_first: bool = False
    output_dim: int = 45


class Subsampling(nn.Module):
    """Conv2d(1->D,3,2)+ReLU, Conv2d(D->D,k,s)+ReLU[, third], Linear; zeroes padded frames."""

    _SPEC = {4: [(3, 2), (3, 2)], 6: [(3, 2), (5, 3)], 8: [(3, 2), (3, 2), (3, 2)]}

    def __init__(self, idim, odim, subsampling_rate=4):
        super().__init__()
        spec = self._SPEC[subsampling_rate]
        layers, ch, f = [], 1, idim
        for k, s in spec:
            layers += [nn.Conv2d(ch, odim, k, s), nn.ReLU()]
            ch = odim
            f = (f - k) // s + 1
        self.conv = nn.Sequential(*layers)
        lin = nn.Linear(odim * f, odim)
        # the reference wraps the rate-4 Linear in a Sequential (state_dict key linear.0.*)
        self.linear = nn.Sequential(lin) if subsampling_rate == 4 else lin
        self._spec = spec

    def subsampled_length(self, length: torch.Tensor):
        for k, s in self._spec:
            length = torch.div(length - k, s, rounding_mode="floor") + 1
        return length

    def forward(self, x: torch.Tensor, length: torch.Tensor):
        # channel-last all the way: MIOpen's implicit-GEMM kernels are NHWC natively (an NCHW
        # call wraps them in two transposes of the 32 x 256 x 498 x 39 activation), and the
        # Linear consumes the (t, f, c) order through a column-permuted view of its weight
        convs = list(self.conv)
        if ck.conv1_relu_ok(convs[0], x):
            # Conv2d(1, D, 3, 2) + ReLU as one direct stencil kernel (csrc/conf_front.hip): its
            # (B, D, T/2, 39) output is the largest tensor of the step
            x = ck.conv1_relu(x, convs[0])
            convs = convs[2:]
        else:
            x = x.unsqueeze(1).contiguous(memory_format=torch.channels_last)
        for m in convs:
            if isinstance(m, nn.Conv2d):
                plain = (x.is_cuda and tuple(m.kernel_size) == (3, 3) and tuple(m.padding) == (0, 0)
                         and tuple(m.dilation) == (1, 1) and m.groups == 1)
                if plain and zk.conv3x3_s2_map_ok(x.permute(0, 2, 3, 1), m.weight, m.stride):
                    # the pre-split bf16x3 GEMM with implicit operands, forward and data gradient
                    # (zk._Conv3x3S2Map; weight gradient: the implicit-im2col TN kernel): no library
                    # convolution and no patch matrix on the default path
                    y = zk.conv3x3_s2_map(x.permute(0, 2, 3, 1), m.weight, m.bias)
                    x = y.permute(0, 3, 1, 2)
                else:
                    # (the zipformer frontend's implicit-im2col kernel here, round 4, C2: 25.3 ms/step
                    # against 24.4 with the library)
                    x = F.conv2d(x, m.weight.contiguous(memory_format=torch.channels_last), m.bias,
                                 m.stride)
            else:
                x = m(x)
        b, c, t, f = x.size()
        lin = self.linear[0] if isinstance(self.linear, nn.Sequential) else self.linear
        wperm = lin.weight.view(-1, c, f).transpose(1, 2).reshape(-1, f * c)
        out = zk.linear(x.permute(0, 2, 3, 1).reshape(b, t, f * c), wperm, lin.bias)
        length = self.subsampled_length(length)
        mask = torch.arange(t, device=length.device).unsqueeze(0) >= length.unsqueeze(1)
        out = out.masked_fill(mask.unsqueeze(-1), 0.0)
        return out, length




class _FeedForwardModule(nn.Module):
    def __init__(self, input_dim, hidden_dim, dropout):
        super().__init__()
        self.sequential = nn.Sequential(nn.LayerNorm(input_dim), nn.Linear(input_dim, hidden_dim),
                                        nn.SiLU(), ck.Dropout(dropout),
                                        nn.Linear(hidden_dim, input_dim), ck.Dropout(dropout))

    def forward(self, x):
        ln, l1, act, d1, l2, d2 = self.sequential
        h = ck.silu(zk.linear(ck.layer_norm(x, ln), l1.weight, l1.bias))
        return d2(zk.linear(d1(h), l2.weight, l2.bias))


class _ConvolutionModule(nn.Module):
    def __init__(self, input_dim, num_channels, kernel_size, dropout, bias=True,
                 use_group_norm=False):
        super().__init__()
        assert (kernel_size - 1) % 2 == 0
        self.layer_norm = nn.LayerNorm(input_dim)
        self.sequential = nn.Sequential(
            nn.Conv1d(input_dim, 2 * num_channels, 1, bias=bias),
            nn.GLU(dim=1),
            nn.Conv1d(num_channels, num_channels, kernel_size, padding=(kernel_size - 1) // 2,
                      groups=num_channels, bias=bias),
            nn.GroupNorm(1, num_channels) if use_group_norm else nn.BatchNorm1d(num_channels),
            nn.SiLU(),
            nn.Conv1d(num_channels, input_dim, 1, bias=bias),
            ck.Dropout(dropout))

    def forward(self, x):
        """x (T,B,D) time-major -> (T,B,D)."""
        pw1, _, dw, norm, act, pw2, drop = self.sequential
        T, B, D = x.shape
        x = ck.layer_norm(x, self.layer_norm)
        u = zk.linear(x, pw1.weight, pw1.bias)                        # (T,B,2C): [a | gate]
        C = u.shape[-1] // 2
        y = zk.glu_chunk_causal_dwconv(u, C, None, dw, -1)            # GLU + depthwise, fused
        if isinstance(norm, nn.BatchNorm1d):
            y = ck.batchnorm_silu(y, norm)                            # batch statistics over B*T
        else:
            y = ck.silu(norm(y.permute(1, 2, 0)).permute(2, 0, 1).contiguous())
        y = zk.linear(y, pw2.weight, pw2.bias)
        return drop(y)


class ConformerLayer(nn.Module):
    def __init__(self, input_dim, ffn_dim, num_attention_heads, depthwise_conv_kernel_size,
                 dropout=0.0, use_group_norm=False, convolution_first=False):
        super().__init__()
        self.ffn1 = _FeedForwardModule(input_dim, ffn_dim, dropout)
        self.self_attn_layer_norm = nn.LayerNorm(input_dim)
        self.self_attn = nn.MultiheadAttention(input_dim, num_attention_heads, dropout=dropout)
        self.self_attn_dropout = ck.Dropout(dropout)
        self.conv_module = _ConvolutionModule(input_dim, input_dim, depthwise_conv_kernel_size,
                                              dropout, bias=True, use_group_norm=use_group_norm)
        self.ffn2 = _FeedForwardModule(input_dim, ffn_dim, dropout)
        self.final_layer_norm = nn.LayerNorm(input_dim)
        self.convolution_first = convolution_first

    def _mhsa(self, x, lengths):
        """nn.MultiheadAttention (no positional term) on (T,B,D): the in/out projections are
        zk.linear (weight gradients accumulated in place by the TN MFMA GEMM), the
        softmax(QK^T / sqrt(dh))V core is the flash-style MFMA kernel (csrc/conf_attn.hip), which
        reads q / k / v as column blocks of the in-projection's output and masks the keys at
        t >= lengths[b].  `self.self_attn` only holds the parameters, under torchaudio's names."""
        mha = self.self_attn
        qkv = zk.linear(x, mha.in_proj_weight, mha.in_proj_bias)
        p = float(mha.dropout) if self.training else 0.0
        o = ck.mhsa(qkv, lengths, mha.num_heads, p)
        return zk.linear(o, mha.out_proj.weight, mha.out_proj.bias)

    def forward(self, x, lengths):
        """x (T,B,D) time-major; lengths (B,) valid frames (the key padding mask is t >= length)."""
        if conf_layer.eligible(self, x):
            return conf_layer.run(self, x, lengths)
        x = self.ffn1(x) * 0.5 + x
        if self.convolution_first:
            x = x + self.conv_module(x)
        res = x
        x = self._mhsa(ck.layer_norm(x, self.self_attn_layer_norm), lengths)
        x = self.self_attn_dropout(x) + res
        if not self.convolution_first:
            x = x + self.conv_module(x)
        x = self.ffn2(x) * 0.5 + x
        return ck.layer_norm(x, self.final_layer_norm)


class _ConformerStack(nn.Module):
    """torchaudio.models.Conformer: forward(input (B,T,D), lengths) -> ((B,T,D), lengths)."""

    def __init__(self, input_dim, num_heads, ffn_dim, num_layers, depthwise_conv_kernel_size,
                 dropout=0.0, use_group_norm=False, convolution_first=False):
        super().__init__()
        self.conformer_layers = nn.ModuleList([
            ConformerLayer(input_dim, ffn_dim, num_heads, depthwise_conv_kernel_size, dropout,
                           use_group_norm, convolution_first) for _ in range(num_layers)])

    def forward(self, x, lengths):
        x = x.transpose(0, 1).contiguous()
        for layer in self.conformer_layers:
            x = layer(x, lengths)
        return x.transpose(0, 1), lengths


class Conformer(nn.Module):
    def __init__(self, config: ConformerConfig) -> None:
        super().__init__()
        self._bn_cmvn = config.bn_cmvn
        if self._bn_cmvn:
            self._batchnorm = nn.BatchNorm1d(num_features=config.feats_dim)
        self._subsampling_module = Subsampling(config.feats_dim, config.input_dim,
                                               config.subsampling_rate)
        self._conformer_module = _ConformerStack(
            config.input_dim, config.num_heads, config.ffn_dim, config.num_layers,
            config.depthwise_conv_kernel_size, config.dropout, config.use_group_norm,
            config.convolution_first)
        self._output_layer = nn.Conv1d(config.input_dim, config.output_dim, kernel_size=1,
                                       bias=True)

    def forward(self, feats: torch.Tensor, lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._bn_cmvn:
            feats = self._batchnorm(feats.transpose(1, 2)).transpose(1, 2)
        x, lengths = self._subsampling_module(feats, lengths)
        x, lengths = self._conformer_module(x, lengths)
        logits = zk.linear(x, self._output_layer.weight, self._output_layer.bias)
        return logits, lengths
