"""Chunk-by-chunk (streaming) inference of Zipformer2 on the MI355X kernels.

Mirrors the reference's streaming surface (model/encoder/zipformer.py): `get_init_states`
(:529-600), `streaming_step` (:601-663) and the per-module `streaming_forward`s it calls
(:465-527, :1223-1338, :1432-1496, :1616-1650, :2079-2190, :2282-2333, :2485-2541, :2697-2741;
model/layer/scaling.py:683-716; model/layer/subsampling.py:134-178, 321-391).  The state list
keeps the reference's order, shapes and layouts, so states are interchangeable.

Every dense op runs through the kernels the training path uses (no torch fallback): GEMMs,
Swoosh+GEMM, BiasNorm, bypass, down/upsampling and the NHWC convolutions as they are; the two
stateful pieces are mapped onto the existing kernels instead of getting slower special cases:

* attention with a cached left context of L frames is the square relative-position kernel over
  S = L + T positions whose first L query rows are empty (their weights are dropped): key j and
  query i see offset j - i in both formulations, and the table of S positions contains the
  reference's streaming slice -(S-1) .. T-1;
* the chunk-causal depthwise conv with a cached left pad is the fused conv kernel run over
  [zeros | cache | chunk] with chunk length T: the causal half reads back into the cache, the
  chunk-wise half stays inside the last chunk, and only the last chunk's output is kept.
"""
from typing import List, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from speech2text_amd import zip_kernels as zk
from speech2text_amd.model.layer.scaling import convert_num_channels


# ------------------------------------------------------------------ states
def get_init_states(model, batch_size: int = 1, device=torch.device("cpu")) -> List[Tensor]:
    """For layer i, states[6i:6i+6] = (cached_key (L,B,H*qd), cached_nonlin_attn (1,B,L,3D/4),
    cached_val1, cached_val2 (L,B,H*vd), cached_conv1, cached_conv2 (B,D,K//2)); states[-2] the
    ConvNeXt left pad (B,C,3,F'); states[-1] processed_lens (B,) int64."""
    states = []
    left = model.left_context_frames[0]
    for i, stack in enumerate(model.encoders):
        D, H, ds = model.encoder_dim[i], model.num_heads[i], model.downsampling_factor[i]
        L = left // ds
        pad = model.cnn_module_kernel[i] // 2
        for _ in range(stack.num_layers):
            states += [torch.zeros(L, batch_size, H * model.query_head_dim[i], device=device),
                       torch.zeros(1, batch_size, L, 3 * D // 4, device=device),
                       torch.zeros(L, batch_size, H * model.value_head_dim[i], device=device),
                       torch.zeros(L, batch_size, H * model.value_head_dim[i], device=device),
                       torch.zeros(batch_size, D, pad, device=device),
                       torch.zeros(batch_size, D, pad, device=device)]
    emb = model._encoder_embed
    states.append(torch.zeros(batch_size, emb.layer3_channels, emb.convnext.padding[0],
                              emb.out_width, device=device))
    states.append(torch.zeros(batch_size, dtype=torch.int64, device=device))
    return states


# ------------------------------------------------------------------ modules
def _attn_weights(m, x: Tensor, pos_proj: Tensor, cached_key: Tensor, L: int, kpm: Tensor):
    """RelPositionMultiheadAttentionWeights.streaming_forward.  -> (W (H,B,T,L+T), new cache)."""
    H, qd, pd = m.num_heads, m.query_head_dim, m.pos_head_dim
    qkp = m.in_proj(x)
    T, B, W_ = qkp.shape
    full = torch.zeros(L + T, B, W_, dtype=qkp.dtype, device=qkp.device)
    full[L:] = qkp
    full[:L, :, H * qd:2 * H * qd] = cached_key
    new_key = full[T:, :, H * qd:2 * H * qd].contiguous()
    w = zk.relpos_attention_weights(full, pos_proj, H, qd, pd, None, kpm)
    return w[:, :, L:], new_key


def _self_attn(m, x: Tensor, w: Tensor, cached_val: Tensor, L: int):
    """SelfAttention.streaming_forward; the residual add rides in the out_proj GEMM."""
    T, B, _ = x.shape
    H = w.shape[0]
    v = torch.cat([cached_val, m.in_proj(x)], dim=0)
    new_val = v[T:]
    o = torch.matmul(w, v.reshape(L + T, B, H, -1).permute(2, 1, 0, 3))
    o = o.permute(2, 1, 0, 3).reshape(T, B, -1)
    return zk.linear(o, m.out_proj.weight, m.out_proj.bias, residual=x), new_val


def _nonlin_attention(m, x: Tensor, w0: Tensor, cached_x: Tensor, L: int):
    """NonlinAttention.streaming_forward (one head: the weights of head 0)."""
    T, B, _ = x.shape
    s, u, y = m.in_proj(x).chunk(3, dim=2)
    u = (u * torch.tanh(s)).transpose(0, 1).unsqueeze(0)                # (1,B,T,Ch)
    u = torch.cat([cached_x, u], dim=2)
    new_x = u[:, :, T:]
    o = torch.matmul(w0, u)[0].transpose(0, 1) * y                      # (T,B,Ch)
    return zk.linear(o, m.out_proj.weight, m.out_proj.bias, residual=x), new_x


def _conv_module(m, x: Tensor, cache: Tensor, kpm: Tensor):
    """ConvolutionModule.streaming_forward + ChunkCausalDepthwiseConv1d.streaming_forward."""
    T, B, _ = x.shape
    left = cache.shape[-1]
    g, s = m.in_proj(x).chunk(2, dim=2)
    g = g * torch.sigmoid(s)
    if kpm is not None:
        g = g.masked_fill(kpm.t().unsqueeze(-1), 0.0)
    hist = torch.cat([cache.permute(2, 0, 1), g], dim=0)                # (left+T,B,C)
    new_cache = hist[T:].permute(1, 2, 0)
    n = 1 + (left + T - 1) // T                                         # chunks of length T
    seq = F.pad(hist, (0, 0, 0, 0, n * T - (left + T), 0))
    y = zk.glu_chunk_causal_dwconv(seq, None, None, m.depthwise_conv, T)[(n - 1) * T:]
    return m.out_proj(y, residual=x), new_cache


def _layer(layer, src: Tensor, pos_proj_of, st: List[Tensor], L: int, kpm: Tensor):
    """Zipformer2EncoderLayer.streaming_forward."""
    ck, cna, cv1, cv2, cc1, cc2 = st
    orig = src
    w, ck = _attn_weights(layer.self_attn_weights, src, pos_proj_of(layer.self_attn_weights), ck,
                          L, kpm)
    cur = None if kpm is None else kpm[:, L:]
    src = layer.feed_forward1(src, residual=src)
    src, cna = _nonlin_attention(layer.nonlin_attention, src, w[0:1], cna, L)
    src, cv1 = _self_attn(layer.self_attn1, src, w, cv1, L)
    src, cc1 = _conv_module(layer.conv_module1, src, cc1, cur)
    src = layer.feed_forward2(src, residual=src)
    src = layer.bypass_mid(orig, src)
    src, cv2 = _self_attn(layer.self_attn2, src, w, cv2, L)
    src, cc2 = _conv_module(layer.conv_module2, src, cc2, cur)
    src = layer.feed_forward3(src, residual=src)
    src = layer.bypass(orig, layer.norm(src))
    return src, [ck, cna, cv1, cv2, cc1, cc2]


def _stack(enc, src: Tensor, states: List[Tensor], L: int, kpm: Tensor):
    """Zipformer2Encoder.streaming_forward."""
    T = src.shape[0]
    table = enc.encoder_pos.table(L + T, src.device)                    # offsets -(S-1) .. S-1

    def pos_proj_of(attn):
        return attn.linear_pos(table)

    new = []
    for i, layer in enumerate(enc.layers):
        src, st = _layer(layer, src, pos_proj_of, states[6 * i:6 * i + 6], L, kpm)
        new += st
    return src, new


def _embed(emb, x: Tensor, cached_left_pad: Tensor):
    """Conv2dSubsampling.streaming_forward + ConvNeXt.streaming_forward, channel-last.
    x (N,T,F) -> (N,(T-7)//2-3,D); cached_left_pad (N,C,3,F') as in the reference."""
    x = x.unsqueeze(-1)
    for m in emb.conv:
        if isinstance(m, torch.nn.Conv2d):
            x = zk.conv3x3_nhwc(x, m.weight, m.bias, m.stride, pad_w=m.padding[1])
            x = zk.swoosh(x, False)
    cn = emb.convnext
    T = x.shape[1] - cn.padding[0]
    bypass = x[:, :T]
    x = torch.cat([cached_left_pad.permute(0, 2, 3, 1), x], dim=1)
    new_pad = x[:, T:T + cn.padding[0]].permute(0, 3, 1, 2).contiguous()
    # "same"-padded depthwise conv; rows pad .. pad+T are the reference's valid-in-time outputs
    x = zk.dwconv2d_nhwc(x.contiguous(), cn.depthwise_conv.weight, cn.depthwise_conv.bias)
    x = x[:, cn.padding[0]:cn.padding[0] + T]
    x = zk.linear_big_m(x, cn.pointwise_conv1.weight.flatten(1), cn.pointwise_conv1.bias)
    x = zk.swoosh(x, True)
    x = zk.linear_big_m(x, cn.pointwise_conv2.weight.flatten(1), cn.pointwise_conv2.bias)
    x = bypass + x
    b, t, f, c = x.shape
    w = emb.out.weight.view(-1, c, f).permute(0, 2, 1).reshape(-1, f * c)
    x = zk.linear(x.reshape(b, t, f * c), w, emb.out.bias)
    return emb.out_norm(x), new_pad


# ------------------------------------------------------------------ entry points
@torch.no_grad()
def streaming_step(model, x: Tensor, states: List[Tensor]) -> Tuple[Tensor, List[Tensor]]:
    """x (N, 2*chunk+13, F) on the GPU; states from get_init_states / the previous call.
    -> (out (N, chunk//2, max(encoder_dim)), or log-softmax CTC scores when for_ctc; new states)."""
    if model.training:
        raise RuntimeError("streaming_step is an inference path: call model.eval() first")
    if not x.is_cuda:
        raise RuntimeError("streaming_step runs on the HIP kernels: x and states must be on cuda")
    chunk, left = model.chunk_size[0], model.left_context_frames[0]
    if chunk <= 0 or left < 0:
        raise ValueError("streaming needs a causal model with chunk_size > 0 and "
                         "left_context_frames >= 0")
    N = x.size(0)
    T = 2 * chunk + 13                              # 7 + 2*3: subsampling + ConvNeXt right context
    if x.size(1) != T:
        raise ValueError(f"streaming_step expects {T} frames per call, got {x.size(1)}")
    x, new_pad = _embed(model._encoder_embed, x.float(), states[-2])
    assert x.size(1) == chunk, (x.size(1), chunk)

    processed = states[-1]
    pm = (processed.unsqueeze(1) <= torch.arange(left, device=x.device).expand(N, left)).flip(1)
    kpm = torch.cat([pm, torch.zeros(N, chunk, dtype=torch.bool, device=x.device)], dim=1)
    new_processed = processed + chunk

    x = x.permute(1, 0, 2).contiguous()
    outputs, new_states, off = [], [], 0
    for i, stack in enumerate(model.encoders):
        ds, nl = model.downsampling_factor[i], stack.num_layers
        x = convert_num_channels(x, model.encoder_dim[i])
        st = states[6 * off:6 * (off + nl)]
        off += nl
        k_i = kpm[..., ::ds].contiguous()
        if ds == 1:
            x, st = _stack(stack, x, st, left // ds, k_i)
        else:
            orig = x
            y, st = _stack(stack.encoder, stack.downsample(x), st, left // ds, k_i)
            x = zk.bypass_upsampled(orig, y, stack.out_combiner._get_bypass_scale(y.shape[1]),
                                    stack.upsample.upsample)
        outputs.append(x)
        new_states += st
    x = model.downsample_output(model._get_full_dim_output(outputs)).permute(1, 0, 2)
    if model._for_ctc:
        x = F.log_softmax(model._ctc_projection(x), dim=-1)
    return x, new_states + [new_pad, new_processed]


@torch.no_grad()
def simulated_streaming_forward(model, x: Tensor, x_lens: Tensor, chunk_size=(32,),
                                left_context_frames=(128,)):
    """Zipformer2.streaming_forward (reference :391-406): whole-utterance forward with the chunked
    attention mask, 30 frames of log(1e-10) right padding; switches the model to causal chunks."""
    import math
    model.causal = True
    model.chunk_size = tuple(chunk_size)
    model.left_context_frames = tuple(left_context_frames)
    pad_len = 30
    x = F.pad(x, pad=(0, 0, 0, pad_len), value=math.log(1e-10))
    return model.forward(x, x_lens + pad_len)


class StreamingSession:
    """A stream of fixed-shape `streaming_step` calls replayed as ONE hipGraph.

    A chunk step is a few hundred small launches (every tensor is chunk-sized), so eager
    execution is bound by launch latency, not by the GPU.  All shapes are static from one call
    to the next, so the step is captured once -- input, states and output live in fixed buffers,
    the state update is part of the graph -- and each `step()` is a copy-in plus one graph launch.
    The first two steps of a session run eagerly on the capture stream (GEMM plan selection and
    position tables happen there); states then restart from `get_init_states`."""

    def __init__(self, model, batch_size: int = 1, device=None, warmup: int = 2):
        if model.training:
            raise RuntimeError("StreamingSession is an inference path: call model.eval() first")
        device = torch.device("cuda") if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("StreamingSession runs on the HIP kernels: device must be cuda")
        self.model = model
        chunk = model.chunk_size[0]
        self.frames = 2 * chunk + 13
        self.x = torch.zeros(batch_size, self.frames, model._feature_dim, device=device)
        self.states = get_init_states(model, batch_size, device)
        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side):
            st = [s.clone() for s in self.states]
            for _ in range(warmup):
                _, st = streaming_step(model, self.x, st)
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side):
            self.out, new = streaming_step(model, self.x, self.states)
            for dst, src in zip(self.states, new):
                dst.copy_(src)

    def reset(self):
        for s in self.states:
            s.zero_()

    @torch.no_grad()
    def step(self, x: Tensor) -> Tensor:
        """x (B, 2*chunk+13, F) -> out (B, chunk//2, D) (a view of the session's output buffer:
        consume or clone it before the next step)."""
        if tuple(x.shape) != tuple(self.x.shape):
            raise ValueError(f"expected input of shape {tuple(self.x.shape)}, got {tuple(x.shape)}")
        self.x.copy_(x)
        self.graph.replay()
        return self.out


def _state_batch_dim(i: int, n_states: int) -> int:
    """The batch dimension of states[i] (get_init_states): 1 for the four attention caches of a
    layer, 0 for its two conv caches, the ConvNeXt pad and processed_lens."""
    return 1 if i < n_states - 2 and i % 6 < 4 else 0


class StreamingRecognizer:
    """Features in, text out, a chunk at a time: CMVN -> `streaming_step` -> `joiner._enc_proj` -> the
    chunk-carried RNN-T search (model/decoding.py rnnt_streaming_search) -> the encoder-state update,
    captured once and replayed as ONE hipGraph per chunk, in the style of StreamingSession.

    Fixed buffers: the features `x` (B, 2*chunk+13, F), `chunk_len` (B) -- how many of the chunk's
    chunk//2 encoder frames are valid per row; 0 leaves a row's hypothesis as it is --, the encoder
    states, the search state and its outputs.  `step` is a copy-in plus one replay and returns views:
    consume or clone them before the next step.  The search is RnntStreamingSearch for the stateless
    predictor and a joiner without output projection, RnntLstmStreamingSearch (capturable: every
    greedy round enqueued) for the LSTM predictor and a joiner with or without one; any other pair
    is an error: there is no module-loop fallback.  With `lm` (an RnnLm; beam only) the graph captures
    the chunk call fused with the LM (`lm_weight`, `lm_start_token` as RnntBeamDecoding's): the LSTM
    pair through RnntLstmStreamingSearch, the stateless predictor with either joiner through
    RnntStatelessLmStreamingSearch; `search.lm_score` holds the best beams' unweighted LM sums.  With an
    NgramLm (beam only, no `lm_start_token`) the stateless predictor with a projection-free joiner runs
    RnntNgramStreamingSearch, the one-workgroup chunk kernel with the look-up inside its frame body, and
    the LSTM pair RnntLstmNgramStreamingSearch, the lockstep rounds in their n-gram mode.  With `context` (a
    ContextGraph: hotwords; beam only, the stateless predictor with a projection-free joiner, no LM or an NgramLm)
    the graph captures RnntBiasStreamingSearch's chunk call (model/rnnt_bias.py; `context_weight`), and
    `search.bias_score` holds the reported beams' bias sums; anything else with a context is a ValueError."""

    def __init__(self, encoder, predictor, joiner, tokenizer, cmvn=None, batch_size: int = 1,
                 method: str = "greedy", max_token_step: int = 5, beam_size: int = 4,
                 cutoff_top_k: int = 4, max_tokens: int = 1024, device=None, warmup: int = 2,
                 lm=None, lm_weight: float = 0.0, lm_start_token=None, context=None, context_weight: float = 1.0):
        from speech2text_amd.model.decoding import RnntLstmNgramStreamingSearch, _is_lstm_pair, _is_ngram
        from speech2text_amd.model.rnnt_bias import rnnt_bias_streaming_search
        model, device, lm = self._check_model(encoder, (predictor, joiner), tokenizer, batch_size, device, lm)
        if model._for_ctc:
            raise ValueError("StreamingRecognizer searches the encoder output: build the encoder with for_ctc=False")
        self.joiner = joiner
        if context is None and _is_ngram(lm) and method == "beam" and _is_lstm_pair(predictor, joiner):
            if lm_start_token is not None:
                raise ValueError("an NgramLm starts in its own <s> context: lm_start_token must be None")
            self.search = RnntLstmNgramStreamingSearch(predictor, joiner, batch_size, beam_size, cutoff_top_k,
                                                       max_tokens, device, lm=lm, lm_weight=lm_weight)
        else:
            self.search = rnnt_bias_streaming_search(predictor, joiner, batch_size, method, max_token_step,
                                                     beam_size, cutoff_top_k, max_tokens, device, lm=lm,
                                                     lm_weight=lm_weight, lm_start_token=lm_start_token,
                                                     context=context, context_weight=context_weight)
        self._capture(model, cmvn, device, warmup, lambda enc: joiner._enc_proj(enc).float().contiguous())

    def _check_model(self, encoder, heads, tokenizer, batch_size, device, lm):
        """What every recogniser asks of its encoder (eval mode, on the GPU, causal with an even chunk)
        and of the modules behind it (eval mode); sets the model, tokenizer and chunk geometry ->
        (model, device, the LM on that device)."""
        name = type(self).__name__
        model = getattr(encoder, "encoder", encoder)
        if model.training or any(getattr(h, "training", False) for h in heads):
            raise RuntimeError(f"{name} is an inference path: call .eval() first")
        device = torch.device("cuda") if device is None else torch.device(device)
        if device.type != "cuda" or next(model.parameters()).device.type != "cuda":
            raise RuntimeError(f"{name} runs on the HIP kernels: model and device must be cuda")
        chunk = model.chunk_size[0]
        if chunk <= 0 or chunk % 2 or model.left_context_frames[0] < 0:
            raise ValueError("streaming needs a causal model with an even chunk_size > 0 and "
                             "left_context_frames >= 0")
        self.model, self.tokenizer = model, tokenizer
        self.batch_size, self.chunk, self.Tc = batch_size, chunk, chunk // 2
        self.frames = 2 * chunk + 13
        if lm is not None and hasattr(lm, "to"):           # (a frozen LM follows the model to its device)
            lm = lm.to(device)
        return model, device, lm

    def _capture(self, model, cmvn, device, warmup, scores):
        """The fixed buffers, then CMVN -> streaming_step -> `scores` (encoder output -> what the search
        reads) -> self.search.step -> the state update, warmed up and captured as one graph."""
        batch_size = self.batch_size
        self.x = torch.zeros(batch_size, self.frames, model._feature_dim, device=device)
        self.chunk_len = torch.full((batch_size,), self.Tc, dtype=torch.int64, device=device)
        self.states = get_init_states(model, batch_size, device)
        mean = getattr(cmvn, "global_mean", None)
        istd = getattr(cmvn, "global_istd", None)
        self._cmvn = None if mean is None or istd is None else \
            (mean.detach().to(device).float(), istd.detach().to(device).float())

        def chain(states):
            x = self.x if self._cmvn is None else (self.x - self._cmvn[0]) * self._cmvn[1]
            enc, new = streaming_step(model, x, states)
            am = scores(enc)
            return am, self.search.step(am, self.chunk_len), new

        side = torch.cuda.Stream(device)
        side.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(side), torch.no_grad():
            st = [s.clone() for s in self.states]
            for _ in range(warmup):
                _, _, st = chain(st)
            self.search.reset()
        torch.cuda.current_stream(device).wait_stream(side)
        torch.cuda.synchronize(device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=side), torch.no_grad():
            self.am, self.outputs, new = chain(self.states)
            for dst, src in zip(self.states, new):
                dst.copy_(src)

    def reset(self, rows=None):
        """Rows (indices, or None for all) start a new stream: empty hypothesis, zero encoder states."""
        self.search.reset(rows)
        if rows is None:
            for s in self.states:
                s.zero_()
            return
        idx = torch.as_tensor(rows, dtype=torch.int64).to(self.x.device)
        for i, s in enumerate(self.states):
            s.index_fill_(_state_batch_dim(i, len(self.states)), idx, 0)

    @torch.no_grad()
    def step(self, x: Tensor, chunk_len=None):
        """x (B, 2*chunk+13, F); chunk_len (B) valid encoder frames of this chunk per row, 0..chunk//2
        (None: all).  -> greedy (tokens, out_len, am), beam (tokens, frames, out_len, score,
        stable_len, am); am (B, chunk//2, V) is the chunk's joiner input.  (CtcStreamingRecognizer:
        (tokens, out_len, score, stable_len, scores), scores being what its search read.)"""
        if tuple(x.shape) != tuple(self.x.shape):
            raise ValueError(f"expected input of shape {tuple(self.x.shape)}, got {tuple(x.shape)}")
        self.x.copy_(x)
        if chunk_len is None:
            self.chunk_len.fill_(self.Tc)
        else:
            self.chunk_len.copy_(torch.as_tensor(chunk_len, dtype=torch.int64))
        self.graph.replay()
        return (*self.outputs, self.am)

    def _texts(self, lens: Tensor) -> List[str]:
        both = torch.cat([self.search.tokens, lens.unsqueeze(1)], dim=1).cpu()      # one host read
        return [self.tokenizer.decode(both[b, :int(both[b, -1])]) for b in range(both.shape[0])]

    def texts(self) -> List[str]:
        """The current best hypothesis of every row."""
        return self._texts(self.search.out_len)

    def stable_texts(self) -> List[str]:
        """The part of every row's hypothesis that can no longer change (beam: the prefix all live
        beams share; greedy: everything)."""
        return self._texts(self.search.stable_len if self.search.method == "beam" else self.search.out_len)

    def num_output_frames(self, feat_lens: Tensor) -> Tensor:
        """Encoder frames of feat_lens feature frames: the encoder's own arithmetic, (n - 7) // 2
        through the subsampling and (n + 1) // 2 through the output downsampling."""
        n = torch.as_tensor(feat_lens, dtype=torch.int64).cpu()
        return (((n - 7) // 2 + 1) // 2).clamp(min=0)

    def recognize(self, feats: Tensor, feat_lens: Tensor) -> List[str]:
        """Whole utterances (B, T, F) through the stream from a reset: right-padded with log(1e-10)
        (as simulated_streaming_forward pads; the value is the padding's AFTER the CMVN), cut into
        2*chunk-strided windows; row b has clamp(n_out[b] - k * chunk//2, 0, chunk//2) valid frames in
        chunk k, so a row that ended idles while longer ones go on.  -> the texts."""
        import math
        if feats.dim() != 3 or feats.shape[0] != self.batch_size or feats.shape[2] != self.x.shape[2]:
            raise ValueError(f"expected feats of shape ({self.batch_size}, T, {self.x.shape[2]}), "
                             f"got {tuple(feats.shape)}")
        n_out = self.num_output_frames(feat_lens)
        K = max(1, -(-int(n_out.max()) // self.Tc))
        need = 2 * self.chunk * (K - 1) + self.frames
        feats = feats.to(self.x.device).float()
        pad = torch.full((feats.shape[2],), math.log(1e-10), device=feats.device)
        if self._cmvn is not None:
            pad = pad / self._cmvn[1] + self._cmvn[0]
        T = feats.shape[1]
        lens = torch.as_tensor(feat_lens, dtype=torch.int64).to(feats.device).clamp(max=T)
        buf = pad.expand(feats.shape[0], max(need, T), -1).clone()
        valid = torch.arange(T, device=feats.device).unsqueeze(0) < lens.unsqueeze(1)
        buf[:, :T] = torch.where(valid.unsqueeze(-1), feats, buf[:, :T])
        self.reset()
        for k in range(K):
            cl = (n_out - k * self.Tc).clamp(0, self.Tc)
            self.step(buf[:, 2 * self.chunk * k:2 * self.chunk * k + self.frames], cl)
        return self.texts()


class CtcStreamingRecognizer(StreamingRecognizer):
    """StreamingRecognizer for a CTC model: CMVN -> `streaming_step` -> the CTC scores -> the chunk-carried
    prefix beam search (model/decoding.py CtcStreamingSearch) -> the encoder-state update, captured once
    and replayed as ONE hipGraph per chunk.  The encoder is either built with for_ctc=True (its own
    projection; `streaming_step` returns log-softmax scores) or with for_ctc=False and `head`, the CTC
    task's Projector in eval mode, whose raw logits the search normalises itself.

    Same surface: `reset`, `step`, `texts`, `stable_texts`, `num_output_frames`, `recognize`, the fixed
    buffers `x`, `chunk_len`, `states`, and `search` with its outputs.  `step` returns (tokens, out_len,
    score, stable_len, scores), scores (B, chunk//2, V) being what the search read.  method "beam" or
    "greedy" (beam_size = cutoff_top_k = 1); with `lm` (an RnnLm, or an NgramLm, which takes no
    `lm_start_token`; beam only) the chunk call is fused with it (`lm_weight`, `lm_start_token` as
    CtcPrefixBeamDecoding's; model/decoding.py ctc_streaming_search picks the search, through
    model/ctc_bias.py ctc_bias_streaming_search) and `search.lm_score`
    holds the best prefixes' unweighted LM sums.  With `context` (a ContextGraph: hotwords; beam only, no LM
    or an NgramLm) the captured chunk call is CtcBiasStreamingSearch's and `search.bias_score` holds the
    reported prefixes' bias scores.  `max_nodes`: trie nodes per stream (CtcStreamingSearch)."""

    def __init__(self, encoder, tokenizer, head=None, cmvn=None, batch_size: int = 1, method: str = "beam",
                 beam_size: int = 4, cutoff_top_k: int = 4, max_tokens: int = 1024, max_nodes: int = 4096,
                 blank: int = 0, device=None, warmup: int = 2, lm=None, lm_weight: float = 0.0,
                 lm_start_token=None, context=None, context_weight: float = 1.0):
        from speech2text_amd.model.ctc_bias import ctc_bias_streaming_search
        model, device, lm = self._check_model(encoder, (head,), tokenizer, batch_size, device, lm)
        if model._for_ctc == (head is not None):
            raise ValueError("CtcStreamingRecognizer searches CTC scores: build the encoder with for_ctc=True and "
                             "pass no head, or with for_ctc=False and pass the task's Projector as head")
        if head is None:
            num_classes = model._ctc_projection.out_features
            scores = lambda enc: enc.float().contiguous()                                   # noqa: E731
        else:
            num_classes = head._fc.out_features
            scores = lambda enc: head(enc, self.chunk_len)[0].float().contiguous()          # noqa: E731
        self.head = head
        self.search = ctc_bias_streaming_search(num_classes, batch_size, method, beam_size, cutoff_top_k, max_tokens,
                                                max_nodes, blank, device, lm=lm, lm_weight=lm_weight,
                                                lm_start_token=lm_start_token, context=context,
                                                context_weight=context_weight)
        self._capture(model, cmvn, device, warmup, scores)
