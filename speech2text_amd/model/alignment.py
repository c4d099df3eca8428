"""CTC forced alignment and token / word timestamps.

`CtcForcedAligner.align` places a known transcript on the frames of the logits it is scored by: the best
path over the 2U+1 CTC lattice (Viterbi), on the device for the whole batch (csrc/ctc_align.hip,
kernels.ctc_align; the statement is in include/s2t_mi355.h above s2t_ctc_align).  Any hypothesis of any
CTC search here (ctc_greedy_tokens, ctc_prefix_beam_tokens, ctc_prefix_beam_lm_tokens) gets times the same
way, by aligning it against the logits it came from (`align_hypotheses`); no search changes.  CPU tensors
and label widths beyond the kernel's limit run `_module_loop`, the same statement in torch.
"""
import collections
import math
from typing import List, Sequence

import torch

from speech2text_amd import kernels

WORD_MARK = "▁"                                       # sentencepiece's word-initial mark

TokenSpan = collections.namedtuple("TokenSpan", ["token", "begin", "end", "logp", "piece", "begin_s", "end_s"],
                                   defaults=(None, None, None))
WordSpan = collections.namedtuple("WordSpan", ["word", "begin", "end", "logp", "begin_s", "end_s"],
                                  defaults=(None, None))
Alignment = collections.namedtuple("Alignment", ["ok", "score", "tokens", "words"])
# begin inclusive, end exclusive, in frames; begin_s / end_s = frame x frame_seconds where that was given.
# TokenSpan.token is the label id, .piece its text where the aligner has a tokenizer.


def merge_words(pieces: Sequence[str], spans: Sequence) -> List[WordSpan]:
    """Token pieces and their spans (anything with begin, end, logp) -> words.  A piece that starts with
    the sentencepiece word mark opens a word (SubwordTokenizer); the space piece closes the word before it
    and belongs to neither neighbour (CharTokenizer); every other piece continues the word it follows.  A
    word begins where its first token begins, ends where its last token ends, and its logp is the sum of
    its tokens'.  Pure host function."""
    words, cur = [], None
    for piece, sp in zip(pieces, spans):
        if piece == " ":
            if cur is not None:
                words.append(cur)
            cur = None
            continue
        if piece.startswith(WORD_MARK) and cur is not None:
            words.append(cur)
            cur = None
        text = piece[len(WORD_MARK):] if piece.startswith(WORD_MARK) else piece
        if cur is None:
            cur = [text, sp.begin, sp.end, sp.logp]
        else:
            cur = [cur[0] + text, cur[1], sp.end, cur[3] + sp.logp]
    if cur is not None:
        words.append(cur)
    return [WordSpan(*w) for w in words]


class CtcForcedAligner:
    """tokenizer: a CharTokenizer / SubwordTokenizer (anything with `labels` and `encode`) or None: then
    spans carry label ids only and there are no words.  frame_seconds: the duration of one frame of the
    logits (the frontend's shift times the encoder's subsampling), for begin_s / end_s."""

    def __init__(self, tokenizer=None, blank=0, frame_seconds=None) -> None:
        self._tokenizer = tokenizer
        self._blank = int(blank)
        self._frame_seconds = None if frame_seconds is None else float(frame_seconds)
        if self._blank < 0:
            raise ValueError(f"blank must be a class id, got {blank!r}")

    @staticmethod
    def _module_loop(x, targets, blank=0):
        """One utterance on the host's schedule: x (Tb,V) its own frames, targets a list of labels ->
        kernels.CtcAlignment of this utterance (path (Tb), tok_* (U), raw_score, score, ok as tensors /
        Python values of one row).  The statement a frame at a time over all states in torch on x's
        device, in x's dtype (fp32 at least): one maximum and one addition per value, the first maximum in
        the order stay, step, skip; the backtrace runs on the host."""
        x = x.to(torch.promote_types(x.dtype, torch.float32))
        dev, dtype = x.device, x.dtype
        Tb, U = x.shape[0], len(targets)
        S = 2 * U + 1
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)     # noqa: E731
        none = kernels.CtcAlignment(i32([-1] * Tb), i32([-1] * U), i32([-1] * U), torch.zeros(U, dtype=dtype, device=dev),
                                    -math.inf, -math.inf, 0)
        if Tb == 0:
            return none._replace(raw_score=0.0, score=0.0, ok=1) if U == 0 else none
        lab = torch.tensor([targets[s >> 1] if s & 1 else blank for s in range(S)], dtype=torch.int64, device=dev)
        e = x[:, lab]
        skip = torch.zeros(S, dtype=torch.bool, device=dev)
        if U > 1:
            skip[3::2] = lab[3::2] != lab[1:-2:2]
        neg = torch.full((S + 2,), -math.inf, dtype=dtype, device=dev)
        v = torch.cat([e[0, :2], neg[:S - min(S, 2)]])
        back = [torch.zeros(S, dtype=torch.int8, device=dev)]
        for t in range(1, Tb):
            c1 = torch.cat([neg[:1], v[:-1]])
            c2 = torch.where(skip, torch.cat([neg[:2], v[:-2]])[:S], neg[:S])
            step = c1 > v
            m = torch.where(step, c1, v)
            jump = c2 > m
            m = torch.where(jump, c2, m)
            back.append(torch.where(jump, 2, step.to(torch.int8)).to(torch.int8))
            v = m + e[t]
        last = v[-2:].tolist()
        s, raw = S - 1, last[-1]
        if U > 0 and not last[1] > last[0]:
            s, raw = S - 2, last[0]
        if not raw > -math.inf:
            return none._replace(raw_score=raw)
        back = torch.stack(back).cpu()
        path = [s]
        for t in range(Tb - 1, 0, -1):
            s -= int(back[t, s])
            path.append(s)
        path.reverse()
        lse = torch.logsumexp(x, dim=-1)
        begin, end = [-1] * U, [-1] * U
        for t, s in enumerate(path):
            if s & 1:
                if begin[s >> 1] < 0:
                    begin[s >> 1] = t
                end[s >> 1] = t + 1
        path_t = torch.tensor(path, dtype=torch.int64, device=dev)
        on_path = e.gather(1, path_t.unsqueeze(1)).squeeze(1) - lse
        logp = torch.stack([on_path[begin[u]:end[u]].sum() for u in range(U)]) if U else none.tok_logp
        return kernels.CtcAlignment(path_t.to(torch.int32), i32(begin), i32(end), logp, raw, raw - float(lse.sum()), 1)

    def _rows(self, logits, lengths, targets, target_lengths):
        """-> kernels.CtcAlignment over the batch, from the kernel where it applies, else row by row."""
        B, T = logits.shape[0], logits.shape[1]
        U = targets.shape[1] if targets.dim() == 2 else 0
        if logits.is_cuda and U <= kernels.CTC_MAX_LABELS:
            dev = logits.device
            i64 = lambda t: t.to(device=dev, dtype=torch.int64).contiguous()    # noqa: E731
            return kernels.ctc_align(logits.contiguous().float(), i64(lengths), i64(targets.reshape(B, U)),
                                     i64(target_lengths), self._blank)
        dev = logits.device
        out = kernels.CtcAlignment(torch.full((B, T), -1, dtype=torch.int32, device=dev),
                                   torch.full((B, U), -1, dtype=torch.int32, device=dev),
                                   torch.full((B, U), -1, dtype=torch.int32, device=dev),
                                   torch.zeros((B, U), dtype=torch.float32, device=dev),
                                   torch.zeros(B, dtype=torch.float32, device=dev),
                                   torch.zeros(B, dtype=torch.float32, device=dev),
                                   torch.zeros(B, dtype=torch.int32, device=dev))
        lens, tls = lengths.tolist(), target_lengths.tolist()
        for b in range(B):
            n, u = max(0, min(int(lens[b]), T)), max(0, min(int(tls[b]), U))
            r = self._module_loop(logits[b, :n], targets[b, :u].tolist(), self._blank)
            out.raw_score[b], out.score[b], out.ok[b] = r.raw_score, r.score, r.ok
            if r.ok:
                out.path[b, :n], out.tok_begin[b, :u], out.tok_end[b, :u] = r.path, r.tok_begin, r.tok_end
                out.tok_logp[b, :u] = r.tok_logp
        return out

    @torch.no_grad()
    def align(self, logits, lengths, targets, target_lengths) -> List[Alignment]:
        """logits (B,T,V), lengths (B), targets (B,U) label ids, target_lengths (B) -> one Alignment per
        utterance.  An utterance whose transcript does not fit its frames has ok False, score -inf and no
        spans."""
        rows = self._rows(logits, lengths, targets, target_lengths)
        ok, score = rows.ok.tolist(), rows.score.tolist()
        begin, end, logp = rows.tok_begin.tolist(), rows.tok_end.tolist(), rows.tok_logp.tolist()
        ids, tls = targets.tolist(), target_lengths.tolist()
        fs = self._frame_seconds
        labels = self._tokenizer.labels if self._tokenizer is not None else None
        out = []
        for b in range(logits.shape[0]):
            if not ok[b]:
                out.append(Alignment(False, score[b], [], []))
                continue
            toks = []
            for u in range(max(0, min(int(tls[b]), len(begin[b])))):
                piece = labels[ids[b][u]] if labels is not None else None
                toks.append(TokenSpan(ids[b][u], begin[b][u], end[b][u], logp[b][u], piece,
                                      None if fs is None else begin[b][u] * fs, None if fs is None else end[b][u] * fs))
            words = merge_words([t.piece for t in toks], toks) if labels is not None else []
            if fs is not None:
                words = [w._replace(begin_s=w.begin * fs, end_s=w.end * fs) for w in words]
            out.append(Alignment(True, score[b], toks, words))
        return out

    def align_text(self, logits, lengths, texts: Sequence[str]) -> List[Alignment]:
        """The transcripts as text: encoded with the aligner's tokenizer."""
        if self._tokenizer is None:
            raise RuntimeError("align_text needs a tokenizer")
        rows = [self._tokenizer.encode(t).to(torch.int64) for t in texts]
        tl = torch.tensor([r.numel() for r in rows], dtype=torch.int64)
        targets = torch.zeros((len(rows), max([1] + tl.tolist())), dtype=torch.int64)
        for b, r in enumerate(rows):
            targets[b, :r.numel()] = r
        return self.align(logits, lengths, targets.to(logits.device), tl.to(logits.device))

    def align_hypotheses(self, logits, lengths, tokens, out_len) -> List[Alignment]:
        """Times for the hypotheses of a CTC search: the (tokens (B,T), out_len (B)) pair that
        ctc_greedy_tokens, ctc_prefix_beam_tokens and ctc_prefix_beam_lm_tokens return, aligned against the
        logits they were searched in."""
        width = int(out_len.max()) if out_len.numel() else 0
        return self.align(logits, lengths, tokens[:, :width].contiguous(), out_len)
