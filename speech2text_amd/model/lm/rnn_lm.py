"""RNN language model (reference model/lm/rnn_lm.py:26-100): Embedding -> N-layer LSTM ->
Linear.  Same constructor, state_dict names and method signatures; the LSTM stack is our own
module with torch.nn.LSTM's parameter names and init, each layer one input GEMM for all steps
plus the step-launched recurrence kernel (csrc/lstm_step.hip through conf_kernels.lstm).
Like the reference, the recurrence runs over padded positions (unidirectional; the loss masks
them)."""
import dataclasses
import math
from typing import Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from speech2text_amd import conf_kernels as ck
from speech2text_amd import zip_kernels as zk
from speech2text_amd.model.functions.masking import make_non_pad_mask
from speech2text_amd.model.layer.scaling import Linear


@dataclasses.dataclass
class RnnLmConfig:
    num_symbols: int = 128
    symbol_embedding_dim: int = 512
    num_rnn_layer: int = 3
    dropout: float = 0.0
    bidirectional: bool = False


class LstmStack(nn.Module):
    """torch.nn.LSTM(input_size, hidden_size, num_layers, dropout) restated: parameters
    weight_ih_l{k} (4H,in), weight_hh_l{k} (4H,H), bias_ih_l{k}, bias_hh_l{k} (4H) created and
    initialised in nn.LSTM's order (U(-1/sqrt(H), 1/sqrt(H)) each), gate order i, f, g, o.
    Time-major: x (T,B,in) -> (T,B,H).  Dropout (the hashed-mask kernel) follows every layer but
    the last, in train mode only."""

    def __init__(self, input_size, hidden_size, num_layers, dropout=0.0):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        H = hidden_size
        for k in range(num_layers):
            ins = input_size if k == 0 else H
            self.register_parameter(f"weight_ih_l{k}", nn.Parameter(torch.empty(4 * H, ins)))
            self.register_parameter(f"weight_hh_l{k}", nn.Parameter(torch.empty(4 * H, H)))
            self.register_parameter(f"bias_ih_l{k}", nn.Parameter(torch.empty(4 * H)))
            self.register_parameter(f"bias_hh_l{k}", nn.Parameter(torch.empty(4 * H)))
        self.dropout = ck.Dropout(p=dropout)
        stdv = 1.0 / math.sqrt(H) if H > 0 else 0.0
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def forward(self, x, states=None):
        """states: None or (h0, c0), each (num_layers, B, H) -> (hs (T,B,H), (h_T, c_T))."""
        hT, cT = [], []
        for k in range(self.num_layers):
            bias = getattr(self, f"bias_ih_l{k}") + getattr(self, f"bias_hh_l{k}")
            gx = zk.linear(x, getattr(self, f"weight_ih_l{k}"), bias)
            h0, c0 = (None, None) if states is None else (states[0][k], states[1][k])
            x, h, c = ck.lstm(gx, getattr(self, f"weight_hh_l{k}"), h0, c0)
            if k + 1 < self.num_layers:
                x = self.dropout(x)
            hT.append(h)
            cT.append(c)
        return x, (torch.stack(hT, 0), torch.stack(cT, 0))


class RnnLm(nn.Module):
    def __init__(self, config: RnnLmConfig) -> None:
        super().__init__()
        self._embedding_dim = config.symbol_embedding_dim
        self._num_symbols = config.num_symbols
        self._embedding = nn.Embedding(num_embeddings=self._num_symbols,
                                       embedding_dim=self._embedding_dim)
        self._num_rnn_layer = config.num_rnn_layer
        self._dropout = config.dropout
        self._bidirectional = config.bidirectional
        if self._bidirectional:
            # the reference's own _logits_layer has in_features = embedding_dim and cannot take
            # the 2H output of a bidirectional nn.LSTM: that setting never worked there
            raise ValueError("RnnLm: bidirectional=True is not supported (the reference's logits "
                             "layer cannot take a bidirectional LSTM's output either)")
        self._rnn_layer = LstmStack(self._embedding_dim, self._embedding_dim,
                                    self._num_rnn_layer, self._dropout)
        self._logits_layer = Linear(in_features=self._embedding_dim,
                                    out_features=self._num_symbols)

    def init_states(self, beam_size):
        """(h_0, c_0), each (num_rnn_layer, beam_size, H), on the model's device."""
        dev = self._embedding.weight.device
        shape = (self._num_rnn_layer, beam_size, self._embedding_dim)
        return (torch.zeros(shape, device=dev), torch.zeros(shape, device=dev))

    def _run(self, x, states=None):
        x = self._embedding(x.t())                       # (T,B,E): the kernels are time-major
        x, states = self._rnn_layer(x, states)
        return self._logits_layer(x).permute(1, 0, 2), states

    def forward(self, x: torch.Tensor, x_lens: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """x (B,T) token ids -> (logits (B,T,V), x_lens)."""
        logits, _ = self._run(x)
        return logits, x_lens

    @torch.no_grad()
    def score(self, tokens: torch.Tensor, tokens_length: torch.Tensor):
        """tokens (B,T), tokens_length (B) -> (B) sum of the log-probabilities of tokens[:, 1:]
        over the valid positions."""
        logits, tokens_length = self.forward(tokens, tokens_length)
        log_probs = F.log_softmax(logits, dim=-1)
        tgt = log_probs[:, :-1].gather(2, tokens[:, 1:].long().unsqueeze(2)).squeeze(2)
        mask = make_non_pad_mask(tokens_length - 1)
        return torch.sum(tgt * mask, dim=-1)

    @torch.no_grad()
    def score_step(self, tokens: torch.Tensor, states):
        """tokens (beam), states (h, c) -> (log_probs (beam, V), new states)."""
        logits, states = self._run(tokens.unsqueeze(-1), states)
        return F.log_softmax(logits, dim=-1).squeeze(1), states
