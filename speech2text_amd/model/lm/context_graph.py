"""Hotword (contextual) biasing for the CTC prefix beam search: the caller's phrases, as lists of token
ids, compiled to an Aho-Corasick automaton in the n-gram's table form, which the device search reads
(csrc/ngram_lookup.h; s2t_context_score, s2t_ctc_prefix_beam_bias in include/s2t_mi355.h).

THE STATEMENT, on a hypothesis' whole token history h, independent of any table:

    match(h)      the longest suffix of h that is a prefix (proper or whole) of some phrase
    bias_sum(h) = context_score * len(match(h))
                  + sum over k in 1..len(h), over every phrase p that h[:k] ends with, of bonus(p)
    final_bias(h) = bias_sum(h) without the first term

bonus(p) is phrase_scores[p] if given, else context_score * len(p).  The first term is a loan: a partial
match is lent context_score a token and pays it back when the match is lost, or at the end of the
utterance (final_bias).  A phrase listed twice counts once (its first score).  A phrase that is a suffix
of another phrase's prefix pays its bonus when it ends inside the longer match.

The tables, int32 / fp tensors that move with `.to()`; state 0 is the root and is dense:

    ctx_begin [num_ctx + 1]   the arcs of state n are [ctx_begin[n], ctx_begin[n + 1])
    ctx_fail [num_ctx]        the longest proper suffix of the state that is itself a state
    ctx_backoff [num_ctx]     context_score * (depth(fail[n]) - depth(n)): the loan a fail hop pays back
    ctx_final [num_ctx]       -context_score * depth(n): the loan still out at the end
    arc_token, arc_score, arc_next [num_arcs]
                              arc_score: context_score + the bonuses of every phrase ending at the target;
                              a root arc of a class no phrase starts with has score 0 and leads to the root

THE BIAS STATEMENT (include/s2t_mi355.h has it once), bias(state, c) -> (score, next): acc = 0, n = state.
While n != 0: binary-search c among the arcs of n; found: return (acc + arc_score, arc_next); else acc +=
ctx_backoff[n], n = ctx_fail[n].  At the root return (acc + arc_score[c], arc_next[c]).  Adds in the tables'
dtype in exactly this order, at most max_depth + 1 hops.  Then bias_sum(h + c) = bias_sum(h) + score and
the state of h + c is next.

The host loops' protocol is NgramLm's: init_states(n) -> the root, score_step(tokens, states) -> (the rows
(n, V) of the new states, the new states), and final_scores(states) -> ctx_final of them.
"""
import ctypes

import numpy as np
import torch

from speech2text_amd import _native as N


def max_depth_limit():
    return N.const("S2T_CONTEXT_MAX_DEPTH")


class ContextGraph:
    _TABLES = ("ctx_begin", "ctx_fail", "ctx_backoff", "ctx_final", "arc_token", "arc_score", "arc_next")

    def __init__(self, phrases, num_classes, context_score=1.0, phrase_scores=None, dtype=torch.float32):
        """phrases: a list of non-empty lists of token ids in [0, num_classes), none longer than
        S2T_CONTEXT_MAX_DEPTH; the empty list is legal (one state, V zero arcs).  phrase_scores: None, or one
        bonus per phrase."""
        V, cs = int(num_classes), float(context_score)
        if V < 1:
            raise ValueError(f"a context graph needs num_classes >= 1, got {num_classes!r}")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("a context graph's tables are float32 or float64")
        if not np.isfinite(cs):
            raise ValueError(f"context_score must be finite, got {context_score!r}")
        phrases = [tuple(int(t) for t in p) for p in phrases]
        if phrase_scores is not None and len(phrase_scores) != len(phrases):
            raise ValueError("phrase_scores must hold one score per phrase")
        bonus = {}
        for k, p in enumerate(phrases):
            if not p:
                raise ValueError(f"phrase {k} is empty")
            if len(p) > max_depth_limit():
                raise ValueError(f"phrase {k} has {len(p)} tokens, more than S2T_CONTEXT_MAX_DEPTH {max_depth_limit()}")
            if any(not 0 <= t < V for t in p):
                raise ValueError(f"phrase {k} holds a token outside [0, {V})")
            b = cs * len(p) if phrase_scores is None else float(phrase_scores[k])
            if not np.isfinite(b):
                raise ValueError(f"the score of phrase {k} is not finite")
            bonus.setdefault(p, b)                         # (listed twice: once)
        states = {()} | {p[:k] for p in bonus for k in range(1, len(p) + 1)}
        states = sorted(states, key=lambda h: (len(h), h))
        ids = {h: n for n, h in enumerate(states)}

        def longest(h):                                    # the longest suffix of h that is a state
            while h not in ids:
                h = h[1:]
            return ids[h]

        def ending(h):                                     # the bonuses of every phrase h ends with
            return sum(bonus.get(h[k:], 0.0) for k in range(len(h)))

        kids = [[] for _ in states]
        for h in states[1:]:
            kids[ids[h[:-1]]].append(h[-1])
        begin, tok, score, nxt = [0], [], [], []
        for c in range(V):                                 # the dense root
            tok.append(c)
            score.append(cs + ending((c,)) if (c,) in ids else 0.0)
            nxt.append(ids.get((c,), 0))
        begin.append(V)
        for h in states[1:]:
            for c in sorted(kids[ids[h]]):
                tok.append(c)
                score.append(cs + ending(h + (c,)))
                nxt.append(ids[h + (c,)])
            begin.append(len(tok))
        fail = [longest(h[1:]) if h else 0 for h in states]
        depth = [len(h) for h in states]
        i32 = lambda t: torch.tensor(t, dtype=torch.int32)                               # noqa: E731
        flt = lambda t: torch.tensor(t, dtype=torch.float64).to(dtype)                   # noqa: E731
        self.num_classes, self.context_score = V, cs
        self.max_depth = max(depth)
        self.depth = np.asarray(depth, dtype=np.int64)
        self.states = states                               # per state its token tuple, the root first
        self.ctx_begin, self.ctx_fail, self.arc_token, self.arc_next = i32(begin), i32(fail), i32(tok), i32(nxt)
        self.ctx_backoff = flt([cs * (depth[f] - d) for f, d in zip(fail, depth)])
        self.ctx_final = flt([-cs * d for d in depth])
        self.arc_score = flt(score)
        self._cache = {}
        self.validate()

    @classmethod
    def from_texts(cls, texts, tokenizer, num_classes=None, **kw):
        """Phrases as text, encoded with the tokenizer first (as CtcForcedAligner.align_text does)."""
        phrases = [[int(t) for t in tokenizer.encode(text)] for text in texts]
        V = len(tokenizer.labels) if num_classes is None else int(num_classes)
        return cls(phrases, V, **kw)

    # ------------------------------------------------------------------ validation
    def validate(self):
        V = self.num_classes
        b, f, tok, nxt = (t.cpu().numpy().astype(np.int64) for t in (self.ctx_begin, self.ctx_fail, self.arc_token,
                                                                     self.arc_next))
        depth = np.asarray(self.depth, dtype=np.int64)
        nc, na = f.shape[0], tok.shape[0]
        if V < 1 or not 0 <= self.max_depth <= max_depth_limit():
            raise ValueError(f"a context graph needs V >= 1 and a depth in 0..{max_depth_limit()}, got V {V} depth "
                             f"{self.max_depth}")
        if nc < 1 or b.shape != (nc + 1,) or depth.shape != (nc,) or self.ctx_backoff.shape != (nc,) \
                or self.ctx_final.shape != (nc,) or nxt.shape != (na,) or self.arc_score.shape != (na,):
            raise ValueError("the context graph's tables' shapes do not fit each other")
        if b[0] != 0 or b[-1] != na or (np.diff(b) < 0).any() or na < V or b[1] != V:
            raise ValueError("ctx_begin must rise from 0 to num_arcs, with exactly V arcs at the root")
        if not np.array_equal(tok[:V], np.arange(V)):
            raise ValueError("the root is dense: arc c of state 0 must be class c")
        if ((tok < 0) | (tok >= V)).any():
            raise ValueError("an arc's token is outside [0, V)")
        inner = np.ones(na, dtype=bool)                    # arc a and arc a - 1 belong to one state
        inner[b[:-1][b[:-1] < na]] = False
        if (np.diff(tok)[inner[1:]] <= 0).any():
            raise ValueError("the arcs of a state must be sorted by token, without duplicates")
        if ((nxt < 0) | (nxt >= nc)).any():
            raise ValueError("an arc's next state is outside [0, num_ctx)")
        if ((f < 0) | (f >= nc)).any() or f[0] != 0:
            raise ValueError("a fail link is outside [0, num_ctx), or the root's is not the root")
        if depth[0] != 0 or (depth[1:] < 1).any() or depth.max() != self.max_depth:
            raise ValueError("the states' depths do not fit max_depth, or a state beside the root has depth 0")
        if (depth[f][1:] >= depth[1:]).any():
            raise ValueError("a fail link does not go shallower")
        owner = np.repeat(np.arange(nc), np.diff(b))
        if (depth[nxt[V:]] != depth[owner[V:]] + 1).any() or (depth[nxt[:V]] > 1).any():
            raise ValueError("an arc does not lead one token deeper")
        cs = self.context_score
        want_bo = torch.tensor(cs * (depth[f] - depth), dtype=torch.float64).to(self.dtype)
        want_fin = torch.tensor(-cs * depth, dtype=torch.float64).to(self.dtype)
        if not torch.equal(self.ctx_backoff.cpu(), want_bo) or not torch.equal(self.ctx_final.cpu(), want_fin):
            raise ValueError("ctx_backoff / ctx_final are not the loans of the states' depths")
        if not bool(torch.isfinite(self.arc_score).all()):
            raise ValueError("the context graph's tables hold a value that is not finite")

    # ------------------------------------------------------------------ where the tables live
    @property
    def num_ctx(self):
        return self.ctx_fail.shape[0]

    @property
    def num_arcs(self):
        return self.arc_token.shape[0]

    @property
    def device(self):
        return self.arc_score.device

    @property
    def dtype(self):
        return self.arc_score.dtype

    def to(self, device):
        """Moves the tables (in place, like a module) -> self."""
        device = torch.device(device)
        if device != self.device:
            for k in self._TABLES:
                setattr(self, k, getattr(self, k).to(device))
            self._cache = {}
        return self

    def desc(self):
        """-> (S2tContextGraphDesc of the device tables by reference, what it points to: keep it alive while
        the descriptor is in use).  The entries check its limits themselves."""
        if "desc" not in self._cache:
            if self.device.type != "cuda" or self.dtype != torch.float32:
                raise RuntimeError("the device bias entries need fp32 tables on the GPU: ContextGraph.to(device)")
            d = N.struct("S2tContextGraphDesc")()
            d.V, d.max_depth, d.num_ctx, d.num_arcs = self.num_classes, self.max_depth, self.num_ctx, self.num_arcs
            d.ctx_begin, d.ctx_fail, d.arc_token, d.arc_next = (N.ip(getattr(self, k)) for k in (
                "ctx_begin", "ctx_fail", "arc_token", "arc_next"))
            d.ctx_backoff, d.ctx_final, d.arc_score = N.fp(self.ctx_backoff), N.fp(self.ctx_final), N.fp(self.arc_score)
            self._cache["desc"] = d
        return ctypes.byref(self._cache["desc"]), [self._cache["desc"]] + [getattr(self, k) for k in self._TABLES]

    # ------------------------------------------------------------------ the statement on the host
    def _np(self):
        if "np" not in self._cache:
            self._cache["np"] = tuple(getattr(self, k).cpu().numpy() for k in self._TABLES)
        return self._cache["np"]

    def score(self, state, c):
        """The bias statement for one (state, class), in the tables' dtype -> (score, next)."""
        begin, fail, backoff, _, tok, sc, nxt = self._np()
        acc, n, c = sc.dtype.type(0.0), int(state), int(c)
        for _ in range(self.max_depth + 1):
            if n == 0:
                break
            lo, hi = int(begin[n]), int(begin[n + 1])
            a = lo + int(np.searchsorted(tok[lo:hi], c))
            if a < hi and tok[a] == c:
                return acc + sc[a], int(nxt[a])
            acc = acc + backoff[n]
            n = int(fail[n])
        return acc + sc[c], int(nxt[c])

    def _row(self, state):
        """score(state, c) for every class c at once -> (score (V), next (V)) numpy, the same adds."""
        state = int(state)
        hit = self._cache.get("rows", {}).get(state)
        if hit is None:
            begin, fail, backoff, _, tok, sc, nxt = self._np()
            V = self.num_classes
            out, onx, done = np.empty(V, sc.dtype), np.empty(V, np.int32), np.zeros(V, bool)
            acc, n = sc.dtype.type(0.0), state
            for _ in range(self.max_depth + 1):
                if n == 0:
                    break
                lo, hi = int(begin[n]), int(begin[n + 1])
                t = tok[lo:hi]
                new = ~done[t]
                out[t[new]] = acc + sc[lo:hi][new]
                onx[t[new]] = nxt[lo:hi][new]
                done[t[new]] = True
                acc = acc + backoff[n]
                n = int(fail[n])
            rest = ~done
            out[rest] = acc + sc[:V][rest]
            onx[rest] = nxt[:V][rest]
            rows = self._cache.setdefault("rows", {})
            if len(rows) >= 4096:
                rows.clear()
            hit = rows[state] = (out, onx)
        return hit

    def _device_score(self, state, token):
        """s2t_context_score on int32 device rows -> (score fp32, next int32)."""
        d, keep = self.desc()
        R = state.shape[0]
        score = torch.empty((R,), dtype=torch.float32, device=self.device)
        nxt = torch.empty((R,), dtype=torch.int32, device=self.device)
        N.check(N.lib().s2t_context_score(d, R, N.ip(state.contiguous()), N.ip(token.contiguous()), N.fp(score),
                                          N.ip(nxt), N.stream()), "s2t_context_score")
        del keep
        return score, nxt

    # ------------------------------------------------------------------ the host loops' protocol
    def init_states(self, n):
        return torch.zeros((n,), dtype=torch.int64, device=self.device)

    def _rows(self, states):
        V = self.num_classes
        if self.device.type == "cuda" and self.dtype == torch.float32:
            n = states.shape[0]
            st = states.to(torch.int32).repeat_interleave(V)
            tok = torch.arange(V, dtype=torch.int32, device=self.device).repeat(n)
            return self._device_score(st, tok)[0].reshape(n, V)
        return torch.from_numpy(np.stack([self._row(s)[0] for s in states.tolist()])).to(self.device) \
            if len(states) else torch.zeros((0, V), dtype=self.dtype, device=self.device)

    def start_scores(self, states):
        """states (n) -> (n, V): what each class adds to bias_sum from that state."""
        return self._rows(states)

    @torch.no_grad()
    def score_step(self, tokens, states):
        """tokens (n), states (n) graph states -> (the rows (n, V) of the new states, the new states (n))."""
        new = torch.tensor([int(self._row(s)[1][t]) for s, t in zip(states.tolist(), tokens.tolist())],
                           dtype=torch.int64, device=self.device)
        return self._rows(new), new

    def final_scores(self, states):
        """states (n) -> (n): ctx_final of them, what the end of the utterance takes back."""
        return self.ctx_final[states.to(self.device).long()]
