"""Chunked restatement of the CTC prefix beam search with back-off n-gram shallow fusion over Python token
tuples: the yardstick of tests/test_ctc_ngram_stream_f64.py and tests/test_gpu_ctc_ngram_stream.py for the
chunk-carried entry of csrc/decode_ctc.hip (s2t_ctc_prefix_beam_ngram_chunk).

Test infrastructure (not a test file).  Written from the contract in include/s2t_mi355.h, not from the
kernel: tests/ctc_stream_f64.Stream's shape (live prefixes carried from one `feed` to the next, no trie,
and after every cut `stable`, `kept`, `ever` and the admission rule as the contract states them of one)
with tests/ctc_ngram_f64.DictNgram as the LM: no shared table, no context id -- an extension p + c that is
not live is scored on p's whole token history from `<s>`, a candidate that is a live prefix keeps its
lm_sum.  `hops` / `root` collect how the look-ups of candidates backed off, `reentered` counts prefixes
that were kept again after they had left the beam.
"""
import numpy as np
import torch

from ctc_prefix_f64 import _Cand, _lae
from ctc_stream_f64 import Report, common_prefix_len, kept_nodes


class Stream:
    def __init__(self, beam_size, cutoff_top_k, ng, lm_weight, blank=0, dtype=torch.float64, max_nodes=None):
        self.dt = {torch.float64: np.float64, torch.float32: np.float32}[dtype]
        assert ng.dt is self.dt
        self.dtype, self.beam_size, self.topk, self.blank = dtype, int(beam_size), int(cutoff_top_k), blank
        self.ng, self.w, self.max_nodes = ng, self.dt(lm_weight), max_nodes
        ninf, zero = self.dt(-np.inf), self.dt(0.0)
        self.beam = [((), zero, ninf)]                           # (tokens, pb, pnb) in beam order
        self.lm = {(): zero}                                     # live prefix -> lm_sum
        self.ever, self.frames, self.overflow = {()}, 0, False
        self.hops, self.root, self.reentered = set(), False, 0

    def _frame(self, row):
        ninf, blank = self.dt(-np.inf), self.blank
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
            if x.live:
                lm_sum = self.lm[tokens]
            else:
                q, n, at_root = self.ng.score(tokens[:-1], tokens[-1])
                self.hops.add(n)
                self.root = self.root or at_root
                lm_sum = self.lm[tokens[:-1]] + q
            scored.append((_lae(x.pb, x.pnb) + self.w * lm_sum, x.key, tokens, x, lm_sum))
        scored.sort(key=lambda e: (-float(e[0]), e[1]))
        kept = scored[:self.beam_size]
        self.reentered += sum(1 for e in kept if not e[3].live and e[2] in self.ever)
        self.ever |= {e[2] for e in kept}
        self.beam = [(e[2], e[3].pb, e[3].pnb) for e in kept]
        self.lm = {e[2]: e[4] for e in kept}

    def kept(self):
        return kept_nodes([p for p, _, _ in self.beam])

    @torch.no_grad()
    def feed(self, logits):
        """logits (n, V) in the stream's dtype: the next n frames -> ctc_stream_f64.Report after them."""
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
        lm_score = float(self.lm[p]) if self.frames else 0.0
        return Report(list(p), score, lm_score, common_prefix_len(seqs), kept_nodes(seqs), len(self.ever),
                      self.overflow)
