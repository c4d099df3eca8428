"""CTC and RNN-T forced alignment and token / word timestamps.

`CtcForcedAligner.align` places a known transcript on the frames of the logits it is scored by: the best
path over the 2U+1 CTC lattice (Viterbi), on the device for the whole batch (csrc/ctc_align.hip,
kernels.ctc_align; the statement is in include/s2t_mi355.h above s2t_ctc_align).  Any hypothesis of any
CTC search here (ctc_greedy_tokens, ctc_prefix_beam_tokens, ctc_prefix_beam_lm_tokens) gets times the same
way, by aligning it against the logits it came from (`align_hypotheses`); no search changes.  CPU tensors
and label widths beyond the kernel's limit run `_module_loop`, the same statement in torch.

`RnntForcedAligner.align` does the same for an RNN-T: the best path over the full (S+1) x (T+1) lattice of
a predictor / joiner pair (csrc/rnnt_align.hip, kernels.rnnt_align; the statement is above s2t_rnnt_align),
whose px / py come from the fused joiner builder (a projection-free joiner) or from materialised logits
(an out-projection joiner).  A token is emitted at ONE frame: its span is [frame, frame + 1).
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


def _encode_texts(tokenizer, texts: Sequence[str], device):
    """Transcripts as text -> (targets (B, widest) int64 zero-padded, target_lengths (B)) on `device`."""
    if tokenizer is None:
        raise RuntimeError("align_text needs a tokenizer")
    rows = [tokenizer.encode(t).to(torch.int64) for t in texts]
    tl = torch.tensor([r.numel() for r in rows], dtype=torch.int64)
    targets = torch.zeros((len(rows), max([1] + tl.tolist())), dtype=torch.int64)
    for b, r in enumerate(rows):
        targets[b, :r.numel()] = r
    return targets.to(device), tl.to(device)


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
        return self.align(logits, lengths, *_encode_texts(self._tokenizer, texts, logits.device))

    def align_hypotheses(self, logits, lengths, tokens, out_len) -> List[Alignment]:
        """Times for the hypotheses of a CTC search: the (tokens (B,T), out_len (B)) pair that
        ctc_greedy_tokens, ctc_prefix_beam_tokens and ctc_prefix_beam_lm_tokens return, aligned against the
        logits they were searched in."""
        width = int(out_len.max()) if out_len.numel() else 0
        return self.align(logits, lengths, tokens[:, :width].contiguous(), out_len)


def rnnt_lattice_torch(logits, symbols, boundary, blank=0, rnnt_type="regular"):
    """(px, py) of the full lattice of materialised logits (B,T,S+1,V) in torch, on any device, in the
    logits' dtype (fp32 at least): what kernels.rnnt_logits_lattice computes on the device.  px (B,S,T+1)
    with columns T and T_b at -inf on the regular lattice, (B,S,T) on the two others; 'constrained' adds
    the blank of the row above to the symbol."""
    logits = logits.to(torch.promote_types(logits.dtype, torch.float32))
    B, T, S1, _ = logits.shape
    S = S1 - 1
    lp = torch.log_softmax(logits, dim=-1)
    py = lp[..., blank].transpose(1, 2).contiguous()                       # (B,S+1,T)
    idx = symbols.to(device=logits.device, dtype=torch.int64).reshape(B, 1, S, 1).expand(B, T, S, 1)
    px = lp[:, :, :S, :].gather(3, idx).squeeze(3).transpose(1, 2)         # (B,S,T)
    if rnnt_type == "constrained":
        px = px + py[:, 1:, :]
    if rnnt_type == "regular":
        px = torch.cat([px, px.new_full((B, S, 1), -math.inf)], dim=2)
        tb = boundary[:, 3].to(logits.device).clamp(0, T).reshape(B, 1, 1).expand(B, S, 1)
        px = px.scatter(2, tb, -math.inf)
    return px.contiguous(), py


class RnntForcedAligner:
    """Places a known transcript on the frames of an RNN-T model: the best path over the full (S+1) x
    (T+1) lattice of the predictor / joiner pair (csrc/rnnt_align.hip, kernels.rnnt_align; the statement
    is in include/s2t_mi355.h above s2t_rnnt_align).  An RNN-T token is emitted AT one frame: its span is
    [frame, frame + 1) and its logp the log-probability of that symbol arc.  Any hypothesis of any RNN-T
    search here gets times the same way (`align_hypotheses`); no search changes.

    predictor / joiner: the task's modules (anything called as the training step calls them serves; the
    device kernels take this package's Joiner).  tokenizer, frame_seconds: as CtcForcedAligner.
    rnnt_type: the lattice, 'regular' (several tokens may share a frame) or 'modified' / 'constrained' (at
    most one token per frame)."""

    # the materialised (b,T,S+1,V) fp32 logits of an out-projection joiner are built for as many
    # utterances at a time as fit this many bytes (at least one)
    LOGITS_BUDGET_BYTES = 256 << 20

    def __init__(self, predictor, joiner, tokenizer=None, blank=0, frame_seconds=None, rnnt_type="regular") -> None:
        if rnnt_type not in kernels.RNNT_TYPES:
            raise ValueError(f"rnnt_type {rnnt_type!r} is not one of 'regular', 'modified', 'constrained'")
        self._predictor = predictor
        self._joiner = joiner
        self._tokenizer = tokenizer
        self._blank = int(blank)
        self._frame_seconds = None if frame_seconds is None else float(frame_seconds)
        self._rnnt_type = rnnt_type
        if self._blank < 0:
            raise ValueError(f"blank must be a class id, got {blank!r}")

    @staticmethod
    def _module_loop(px, py, Sb, Tb, rnnt_type="regular"):
        """One utterance on the host's schedule: px (S,T+1 | T), py (S+1,T) its slices of the operands ->
        kernels.RnntAlignment of this utterance (tok_frame (Sb) int32, tok_logp (Sb), score, ok as a
        tensor / Python values of one row).  The statement a step at a time over all rows in torch on px's
        device, in px's dtype (fp32 at least): an anti-diagonal (regular) or a frame per step, one addition
        per candidate, "symbol" exactly when cu > cl; the backtrace runs on the host."""
        px = px.to(torch.promote_types(px.dtype, torch.float32))
        py = py.to(px.dtype)
        dev, dtype = px.device, px.dtype
        reg = rnnt_type == "regular"
        px, py = (px[:Sb, :Tb + 1] if reg else px[:Sb, :Tb]), py[:Sb + 1, :Tb]
        steps = Sb + Tb if reg else Tb
        # the operands of step i per row: the symbol arc (X) and the blank arc (Y) INTO the row's cell of
        # that step, -inf where there is none
        s = torch.arange(Sb + 1, device=dev).unsqueeze(1)
        i = torch.arange(steps + 1, device=dev).unsqueeze(0)
        t = i - s if reg else i + 0 * s
        cell = (t >= 0) & (t <= Tb)
        neg = torch.full((Sb + 1, steps + 1), -math.inf, dtype=dtype, device=dev)
        X, Y = neg, neg
        if Sb and px.shape[1]:
            tx = (t if reg else t - 1).clamp(0, px.shape[1] - 1)
            X = torch.where(cell & (s >= 1) & (t >= (0 if reg else 1)), px[(s - 1).clamp(min=0).expand_as(tx), tx], neg)
        if Tb:
            Y = torch.where(cell & (t >= 1), py[s.expand_as(t), (t - 1).clamp(0, Tb - 1)], neg)
        v = neg[:, 0].clone()
        v[0] = 0.0
        back = []
        for k in range(1, steps + 1):
            cl = v + Y[:, k]
            cu = torch.cat([neg[:1, 0], v[:-1]]) + X[:, k]
            g = cu > cl
            v = torch.where(g, cu, cl)
            back.append(g)
        score = float(v[Sb])
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)     # noqa: E731
        if not score > -math.inf:
            return kernels.RnntAlignment(i32([-1] * Sb), torch.zeros(Sb, dtype=dtype, device=dev), -math.inf, 0)
        back = torch.stack(back).cpu().tolist() if steps else []
        frames = [-1] * Sb
        s, t = Sb, Tb
        while s > 0 or t > 0:
            if back[(s + t if reg else t) - 1][s]:
                frames[s - 1] = t if reg else t - 1
                s, t = (s - 1, t) if reg else (s - 1, t - 1)
            else:
                t -= 1
        f = torch.tensor(frames, dtype=torch.int64, device=dev)
        logp = px.gather(1, f.unsqueeze(1)).squeeze(1) if Sb else torch.zeros(0, dtype=dtype, device=dev)
        return kernels.RnntAlignment(f.to(torch.int32), logp, score, 1)

    def _rows(self, px, py, boundary):
        """-> kernels.RnntAlignment over the batch, from the kernel where it applies, else row by row."""
        B, S = px.shape[0], px.shape[1]
        T = py.shape[2]
        dev = px.device
        if px.is_cuda and S + 1 <= kernels.RNNT_MAX_ROWS and T >= 1:
            return kernels.rnnt_align(px.contiguous().float(), py.contiguous().float(),
                                      boundary.to(device=dev, dtype=torch.int64).contiguous(), self._rnnt_type)
        out = kernels.RnntAlignment(torch.full((B, S), -1, dtype=torch.int32, device=dev),
                                    torch.zeros((B, S), dtype=torch.float32, device=dev),
                                    torch.full((B,), -math.inf, dtype=torch.float32, device=dev),
                                    torch.zeros(B, dtype=torch.int32, device=dev))
        sbs, tbs = boundary[:, 2].tolist(), boundary[:, 3].tolist()
        for b in range(B):
            sb, tb = max(0, min(int(sbs[b]), S)), max(0, min(int(tbs[b]), T))
            r = self._module_loop(px[b], py[b], sb, tb, self._rnnt_type)
            out.score[b], out.ok[b] = r.score, r.ok
            if r.ok:
                out.tok_frame[b, :sb], out.tok_logp[b, :sb] = r.tok_frame, r.tok_logp
        return out

    def _lattice(self, encoder_out, lengths, targets, target_lengths):
        """-> (px, py, boundary) of the full lattice of the batch on encoder_out's device."""
        from speech2text_amd.model.joiner.joiner import Joiner
        dev = encoder_out.device
        B, T = encoder_out.shape[0], encoder_out.shape[1]
        S = targets.shape[1]
        symbols = targets.to(device=dev, dtype=torch.int64).contiguous()
        boundary = kernels.make_boundary(target_lengths, lengths, dev)
        pred = self._predictor(symbols, target_lengths.to(dev), self._predictor.init_state())[0]   # (B,S+1,D)
        j = self._joiner
        ours = isinstance(j, Joiner)
        if not ours:                                       # a foreign joiner: its own forward, all in torch
            logits = j(encoder_out, lengths, pred, target_lengths)[0]
            return (*rnnt_lattice_torch(logits, symbols, boundary, self._blank, self._rnnt_type), boundary)
        am, lm = j._enc_proj(encoder_out).float(), j._pre_proj(pred).float()
        rows_ok = S + 1 <= kernels.RNNT_MAX_ROWS
        if am.is_cuda and rows_ok and T >= 1 and not j._use_out_project and am.shape[2] <= kernels.RNNT_MAX_JOINER_DIM:
            return (*kernels.rnnt_full_lattice(am, lm, symbols, boundary, self._blank, j._act_name,
                                               self._rnnt_type), boundary)
        per = max(1, T * (S + 1) * am.shape[2] * 4)
        nb = max(1, self.LOGITS_BUDGET_BYTES // per)
        pxs, pys = [], []
        for b0 in range(0, B, nb):
            sl = slice(b0, min(B, b0 + nb))
            logits = j._out_projection(j._activation(am[sl].unsqueeze(2) + lm[sl].unsqueeze(1)))
            if am.is_cuda and rows_ok and T >= 1:
                px, py = kernels.rnnt_logits_lattice(logits, symbols[sl], boundary[sl], self._blank, self._rnnt_type)
            else:
                px, py = rnnt_lattice_torch(logits, symbols[sl], boundary[sl], self._blank, self._rnnt_type)
            pxs.append(px)
            pys.append(py)
        return torch.cat(pxs), torch.cat(pys), boundary

    @torch.no_grad()
    def align(self, encoder_out, lengths, targets, target_lengths) -> List[Alignment]:
        """encoder_out (B,T,D): what the joiner's encoder projection takes, lengths (B), targets (B,S)
        label ids, target_lengths (B) -> one Alignment per utterance.  An utterance whose transcript has no
        path (one token per frame and more tokens than frames) has ok False, score -inf and no spans."""
        if targets.dim() != 2:
            targets = targets.reshape(encoder_out.shape[0], -1)
        px, py, boundary = self._lattice(encoder_out, lengths, targets, target_lengths)
        rows = self._rows(px, py, boundary)
        ok, score = rows.ok.tolist(), rows.score.tolist()
        frame, logp = rows.tok_frame.tolist(), rows.tok_logp.tolist()
        ids, tls = targets.tolist(), target_lengths.tolist()
        fs = self._frame_seconds
        labels = self._tokenizer.labels if self._tokenizer is not None else None
        out = []
        for b in range(encoder_out.shape[0]):
            if not ok[b]:
                out.append(Alignment(False, score[b], [], []))
                continue
            toks = []
            for u in range(max(0, min(int(tls[b]), len(frame[b])))):       # in transcript order
                piece = labels[ids[b][u]] if labels is not None else None
                f = frame[b][u]
                toks.append(TokenSpan(ids[b][u], f, f + 1, logp[b][u], piece,
                                      None if fs is None else f * fs, None if fs is None else (f + 1) * fs))
            words = merge_words([t.piece for t in toks], toks) if labels is not None else []
            if fs is not None:
                words = [w._replace(begin_s=w.begin * fs, end_s=w.end * fs) for w in words]
            out.append(Alignment(True, score[b], toks, words))
        return out

    def align_text(self, encoder_out, lengths, texts: Sequence[str]) -> List[Alignment]:
        """The transcripts as text: encoded with the aligner's tokenizer."""
        return self.align(encoder_out, lengths, *_encode_texts(self._tokenizer, texts, encoder_out.device))

    def align_hypotheses(self, encoder_out, lengths, tokens, out_len) -> List[Alignment]:
        """Times for the hypotheses of an RNN-T search: the (tokens (B,N), out_len (B)) pair that the
        greedy and beam searches return (either predictor, with or without an LM), aligned against the
        encoder output they were searched in."""
        width = int(out_len.max()) if out_len.numel() else 0
        return self.align(encoder_out, lengths, tokens[:, :width].contiguous(), out_len)
