"""Chunked restatement of the CTC prefix beam search over Python token tuples: the yardstick of
tests/test_ctc_stream_f64.py and tests/test_gpu_ctc_stream.py for the chunk-carried entries of
csrc/decode_ctc.hip (s2t_ctc_prefix_beam_chunk, s2t_ctc_prefix_beam_lm_chunk).

Test infrastructure (not a test file).  Written from the contract in include/s2t_mi355.h, not from the
kernel: a `Stream` carries the live prefixes (pb, pnb and with an LM q, state, lm_sum per token tuple)
from one `feed` to the next; a frame is the search ctc_prefix_f64.prefix_beam_search states (the same
candidates, merge by tuple, ranking).  It has no trie: after every cut it reports what the contract
says of one --

    stable  the length of the longest common prefix of the live prefixes,
    kept    the size of the union of the paths from that common prefix to each live prefix, the common
            prefix included: the node count a compaction leaves,
    ever    the number of sequences ever kept (the empty one included): the node count of a trie that
            is never compacted

-- and, given `max_nodes`, the admission rule: a feed of n frames is consumed if and only if kept +
beam_size * n <= max_nodes, else none of it is, `overflow` is set and the stream is inert.
"""
import collections

import numpy as np
import torch

import rnn_lm_f64 as R
import rnnt_lm_fusion_f64 as LF
from ctc_prefix_f64 import _Cand, _lae

Report = collections.namedtuple("Report", "tokens score lm_score stable kept ever overflow")


def common_prefix_len(seqs):
    n = 0
    for col in zip(*seqs):
        if any(c != col[0] for c in col):
            break
        n += 1
    return min([n] + [len(s) for s in seqs])


def kept_nodes(seqs):
    """Nodes on the paths from the common prefix of seqs to each of them, that prefix included."""
    base = common_prefix_len(seqs)
    return len({s[:i] for s in seqs for i in range(base, len(s) + 1)})


class Stream:
    def __init__(self, beam_size, cutoff_top_k, blank=0, sd=None, lm_weight=0.0, lm_start_token=None,
                 dtype=torch.float64, max_nodes=None):
        self.dt = {torch.float64: np.float64, torch.float32: np.float32}[dtype]
        self.dtype, self.beam_size, self.topk, self.blank = dtype, int(beam_size), int(cutoff_top_k), blank
        self.sd, self.w, self.max_nodes = sd, self.dt(lm_weight), max_nodes
        ninf, zero = self.dt(-np.inf), self.dt(0.0)
        self.beam = [((), zero, ninf)]                           # (tokens, pb, pnb) in beam order
        self.lm = None
        if sd is not None:
            q0, st0 = LF.lm_start(sd, lm_start_token)
            self.lm = {(): (q0.numpy().astype(self.dt), st0, zero)}
        self.ever, self.frames, self.overflow = {()}, 0, False

    def _frame(self, row):
        dt, ninf, zero, fused, blank = self.dt, self.dt(-np.inf), self.dt(0.0), self.sd is not None, self.blank
        V = row.shape[0]
        k = min(self.topk, V)
        order = sorted(range(V), key=lambda c: (-float(row[c]), c))
        lp = torch.log_softmax(row, dim=-1).numpy()
        live = {p for p, _, _ in self.beam}
        cand = {}

        def add(tokens, key):
            if tokens not in cand:
                cand[tokens] = _Cand(ninf, key, key[0], tokens in live)
            return cand[tokens]

        for i, (p, pb, pnb) in enumerate(self.beam):
            s = _lae(pb, pnb)
            for r, c in enumerate(order[:k]):
                if c == blank:
                    x = add(p, (i, 0, 0))
                    x.pb = _lae(x.pb, s + lp[c])
                    continue
                if p and c == p[-1]:
                    if pnb + lp[c] != -np.inf:
                        x = add(p, (i, 0, 0))
                        x.pnb = _lae(x.pnb, pnb + lp[c])
                    v = pb + lp[c]
                else:
                    v = s + lp[c]
                if v != -np.inf:
                    x = add(p + (c,), (i, 1, r))
                    x.pnb = _lae(x.pnb, v)
        scored = []
        for tokens, x in cand.items():
            lm_sum = zero
            if fused:
                lm_sum = self.lm[tokens][2] if x.live else \
                    self.lm[tokens[:-1]][2] + self.lm[tokens[:-1]][0][tokens[-1]]
            scored.append((_lae(x.pb, x.pnb) + (self.w * lm_sum if fused else zero), x.key, tokens, x, lm_sum))
        scored.sort(key=lambda e: (-float(e[0]), e[1]))
        kept = scored[:self.beam_size]
        if fused:
            new_lm = {}
            for _, _, tokens, x, lm_sum in kept:
                if x.live:
                    new_lm[tokens] = self.lm[tokens]
                else:
                    q, st = R.score_step_ref(self.sd, torch.tensor([tokens[-1]]), self.lm[tokens[:-1]][1])
                    new_lm[tokens] = (q[0].numpy().astype(dt), st, lm_sum)
            self.lm = new_lm
        self.ever |= {e[2] for e in kept}
        self.beam = [(e[2], e[3].pb, e[3].pnb) for e in kept]

    def kept(self):
        return kept_nodes([p for p, _, _ in self.beam])

    @torch.no_grad()
    def feed(self, logits):
        """logits (n, V) in the stream's dtype: the next n frames -> Report after them."""
        n = logits.shape[0]
        admitted = not self.overflow and n > 0
        if admitted and self.max_nodes is not None and self.kept() + self.beam_size * n > self.max_nodes:
            self.overflow, admitted = True, False
        if admitted:
            for t in range(n):
                self._frame(logits[t].to(self.dtype))
            self.frames += n
        p, pb, pnb = self.beam[0]
        seqs = [b[0] for b in self.beam]
        score = float(_lae(pb, pnb)) if self.frames else 0.0
        lm_score = float(self.lm[p][2]) if self.lm is not None and self.frames else 0.0
        return Report(list(p), score, lm_score, common_prefix_len(seqs), kept_nodes(seqs), len(self.ever),
                      self.overflow)
