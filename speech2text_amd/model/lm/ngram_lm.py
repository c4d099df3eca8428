"""Back-off n-gram language model over the model's own classes (sentencepiece pieces or characters),
for shallow fusion in the CTC prefix beam search: read from an ARPA file (`NgramLm.from_arpa`) or
estimated from token ids on the spot (`NgramLm.estimate`), held as flat tables that the device search
reads (csrc/ngram_lookup.h; s2t_ngram_score, s2t_ctc_prefix_beam_ngram in include/s2t_mi355.h).

The LM's state is one integer, a context node.  The tables, int32 / fp32 tensors that move with `.to()`:

    ctx_begin [num_ctx + 1]   the arcs of context n are [ctx_begin[n], ctx_begin[n + 1])
    ctx_fail [num_ctx]        the context with its oldest token dropped
    ctx_backoff [num_ctx]     natural log
    arc_token, arc_logp (natural log), arc_next [num_arcs]
                              arc_next: the longest suffix of context + token that is itself a context

Context 0 is the root and is dense: exactly V arcs, arc c is class c (a class without a unigram takes
`missing_logp`, finite on purpose: lm_weight = 0 must never multiply an infinity).  The arcs of every
other context are sorted by token, without duplicates.  Every suffix of a context is a context, so a
fail link shortens by exactly one token.  Construction validates all of this; the kernels trust it.

THE SCORING STATEMENT (include/s2t_mi355.h has it once, this restates it), score(ctx, c) -> (logp, next):
acc = 0, n = ctx.  While n != 0: binary-search c among the arcs of n; found: return (acc + logp, next);
else acc += backoff[n], n = fail[n].  At the root return (acc + arc_logp[c], arc_next[c]).  Adds in the
tables' dtype in exactly this order, at most `order` hops.

`<s>` is the start context when the model has it, else the root; the first token of a hypothesis is
scored from there.  Entries that predict `</s>` are dropped: there is no end-of-sentence term, as in
the RNN-LM path.  The host loops' LM protocol: init_states(n) -> context ids, score_step(tokens, states)
-> (log_probs (n, V), new states), and start_scores(states) -> the rows of the start context.
"""
import ctypes
import math
import os

import numpy as np
import torch

from speech2text_amd import _native as N

BOS = -1                    # `<s>` inside a context tuple: only ever its first element
_LN10 = math.log(10.0)


def max_order():
    return N.const("S2T_NGRAM_MAX_ORDER")


class NgramLm:
    def __init__(self, num_classes, order, ctx_begin, ctx_fail, ctx_backoff, arc_token, arc_logp, arc_next,
                 start_ctx=0, contexts=None, names=None):
        """The tables as above (anything torch.as_tensor takes).  contexts: per context its tuple of token
        ids (BOS for `<s>`), root first, when known (from_arpa / estimate know it; to_arpa needs it);
        names: the V piece strings for to_arpa (None: decimal ids)."""
        i32 = lambda t: torch.as_tensor(t).to(torch.int32).contiguous()              # noqa: E731
        flt = torch.as_tensor(arc_logp)
        dt = flt.dtype if flt.dtype in (torch.float32, torch.float64) else torch.float32
        self.num_classes, self.order, self.start_ctx = int(num_classes), int(order), int(start_ctx)
        self.ctx_begin, self.ctx_fail, self.arc_token, self.arc_next = map(i32, (ctx_begin, ctx_fail, arc_token,
                                                                                 arc_next))
        self.ctx_backoff = torch.as_tensor(ctx_backoff).to(dt).contiguous()
        self.arc_logp = flt.to(dt).contiguous()
        self.contexts = None if contexts is None else [tuple(int(x) for x in c) for c in contexts]
        self.names = None if names is None else list(names)
        self._cache = {}
        self.validate()

    # ------------------------------------------------------------------ validation
    def validate(self):
        V, order = self.num_classes, self.order
        b, f, tok, nxt = (t.cpu().numpy().astype(np.int64) for t in (self.ctx_begin, self.ctx_fail, self.arc_token,
                                                                     self.arc_next))
        if V < 1 or not 1 <= order <= max_order():
            raise ValueError(f"an n-gram LM needs V >= 1 and an order in 1..{max_order()}, got V {V} order {order}")
        nc, na = f.shape[0], tok.shape[0]
        if nc < 1 or b.shape != (nc + 1,) or self.ctx_backoff.shape != (nc,) or nxt.shape != (na,) \
                or self.arc_logp.shape != (na,):
            raise ValueError("the n-gram tables' shapes do not fit each other")
        if b[0] != 0 or b[-1] != na or (np.diff(b) < 0).any() or na < V or b[1] != V:
            raise ValueError("ctx_begin must rise from 0 to num_arcs, with exactly V arcs at the root")
        if not np.array_equal(tok[:V], np.arange(V)):
            raise ValueError("the root is dense: arc c of context 0 must be class c")
        if ((tok < 0) | (tok >= V)).any():
            raise ValueError("an arc's token is outside [0, V)")
        inner = np.ones(na, dtype=bool)                    # arc a and arc a - 1 belong to one context
        inner[b[:-1][b[:-1] < na]] = False
        if (np.diff(tok)[inner[1:]] <= 0).any():
            raise ValueError("the arcs of a context must be sorted by token, without duplicates")
        if ((nxt < 0) | (nxt >= nc)).any():
            raise ValueError("an arc's next context is outside [0, num_ctx)")
        if ((f < 0) | (f >= nc)).any() or f[0] != 0:
            raise ValueError("a fail link is outside [0, num_ctx), or the root's is not the root")
        depth = np.zeros(nc, dtype=np.int64)               # hops to the root; must exist and stay below order
        at = np.arange(nc)
        for _ in range(order - 1):
            depth += at != 0
            at = f[at]
        if (at != 0).any():
            raise ValueError("a fail link does not shorten its context: the root is not reached in order - 1 hops")
        if ((depth[f] >= depth) & (np.arange(nc) != 0)).any():
            raise ValueError("a fail link does not shorten its context")
        if self.contexts is not None:
            if len(self.contexts) != nc or self.contexts[0] != ():
                raise ValueError("contexts must name every context, the root first")
            for n, c in enumerate(self.contexts):
                if n and (len(c) != depth[n] or self.contexts[f[n]] != c[1:]):
                    raise ValueError(f"context {n} {c}: its fail link is not the context with the oldest token dropped")
        if not 0 <= self.start_ctx < nc:
            raise ValueError(f"start_ctx {self.start_ctx} is outside [0, num_ctx)")
        if not bool(torch.isfinite(self.arc_logp).all()) or not bool(torch.isfinite(self.ctx_backoff).all()):
            raise ValueError("the n-gram tables hold a value that is not finite")
        if self.names is not None and len(self.names) != V:
            raise ValueError("names must hold one string per class")

    # ------------------------------------------------------------------ where the tables live
    @property
    def num_ctx(self):
        return self.ctx_fail.shape[0]

    @property
    def num_arcs(self):
        return self.arc_token.shape[0]

    @property
    def device(self):
        return self.arc_logp.device

    @property
    def dtype(self):
        return self.arc_logp.dtype

    _TABLES = ("ctx_begin", "ctx_fail", "ctx_backoff", "arc_token", "arc_logp", "arc_next")

    def to(self, device):
        """Moves the tables (in place, like a module) -> self."""
        device = torch.device(device)
        if device != self.device:
            for k in self._TABLES:
                setattr(self, k, getattr(self, k).to(device))
            self._cache = {}
        return self

    def desc(self):
        """-> (S2tNgramLmDesc of the device tables by reference, what it points to: keep it alive while
        the descriptor is in use).  The entries check its limits themselves."""
        if "desc" not in self._cache:
            if self.device.type != "cuda" or self.dtype != torch.float32:
                raise RuntimeError("the device n-gram entries need fp32 tables on the GPU: NgramLm.to(device)")
            d = N.struct("S2tNgramLmDesc")()
            d.V, d.order, d.num_ctx, d.num_arcs = self.num_classes, self.order, self.num_ctx, self.num_arcs
            d.ctx_begin, d.ctx_fail, d.ctx_backoff = N.ip(self.ctx_begin), N.ip(self.ctx_fail), N.fp(self.ctx_backoff)
            d.arc_token, d.arc_logp, d.arc_next = N.ip(self.arc_token), N.fp(self.arc_logp), N.ip(self.arc_next)
            self._cache["desc"] = d
        return ctypes.byref(self._cache["desc"]), [self._cache["desc"]] + [getattr(self, k) for k in self._TABLES]

    # ------------------------------------------------------------------ the statement on the host
    def _np(self):
        if "np" not in self._cache:
            self._cache["np"] = tuple(getattr(self, k).cpu().numpy() for k in self._TABLES)
        return self._cache["np"]

    def score(self, ctx, c):
        """The scoring statement for one (context, class), in the tables' dtype -> (logp, next)."""
        begin, fail, backoff, tok, logp, nxt = self._np()
        acc, n, c = logp.dtype.type(0.0), int(ctx), int(c)
        for _ in range(self.order):
            if n == 0:
                break
            lo, hi = int(begin[n]), int(begin[n + 1])
            a = lo + int(np.searchsorted(tok[lo:hi], c))
            if a < hi and tok[a] == c:
                return acc + logp[a], int(nxt[a])
            acc = acc + backoff[n]
            n = int(fail[n])
        return acc + logp[c], int(nxt[c])

    def _row(self, ctx):
        """score(ctx, c) for every class c at once -> (logp (V), next (V)) numpy, the same adds."""
        ctx = int(ctx)
        hit = self._cache.get("rows", {}).get(ctx)
        if hit is None:
            begin, fail, backoff, tok, logp, nxt = self._np()
            V = self.num_classes
            out, onx, done = np.empty(V, logp.dtype), np.empty(V, np.int32), np.zeros(V, bool)
            acc, n = logp.dtype.type(0.0), ctx
            for _ in range(self.order):
                if n == 0:
                    break
                lo, hi = int(begin[n]), int(begin[n + 1])
                t = tok[lo:hi]
                new = ~done[t]
                out[t[new]] = acc + logp[lo:hi][new]
                onx[t[new]] = nxt[lo:hi][new]
                done[t[new]] = True
                acc = acc + backoff[n]
                n = int(fail[n])
            rest = ~done
            out[rest] = acc + logp[:V][rest]
            onx[rest] = nxt[:V][rest]
            rows = self._cache.setdefault("rows", {})
            if len(rows) >= 4096:                          # (a host loop revisits few contexts: keep the memory bounded)
                rows.clear()
            hit = rows[ctx] = (out, onx)
        return hit

    def _device_score(self, ctx, token):
        """s2t_ngram_score on int32 device rows -> (logp fp32, next int32)."""
        d, keep = self.desc()
        R = ctx.shape[0]
        logp = torch.empty((R,), dtype=torch.float32, device=self.device)
        nxt = torch.empty((R,), dtype=torch.int32, device=self.device)
        N.check(N.lib().s2t_ngram_score(d, R, N.ip(ctx.contiguous()), N.ip(token.contiguous()), N.fp(logp), N.ip(nxt),
                                        N.stream()), "s2t_ngram_score")
        del keep
        return logp, nxt

    # ------------------------------------------------------------------ the host loops' LM protocol
    def init_states(self, n):
        return torch.full((n,), self.start_ctx, dtype=torch.int64, device=self.device)

    def start_scores(self, states):
        """states (n) context ids -> (n, V): log p(c | state) for every class, the row that scores a
        hypothesis' next token from that state (its first token from init_states)."""
        return self._rows(states)

    def _rows(self, states):
        V = self.num_classes
        if self.device.type == "cuda":
            n = states.shape[0]
            ctx = states.to(torch.int32).repeat_interleave(V)
            tok = torch.arange(V, dtype=torch.int32, device=self.device).repeat(n)
            return self._device_score(ctx, tok)[0].reshape(n, V)
        return torch.from_numpy(np.stack([self._row(s)[0] for s in states.tolist()])) if len(states) else \
            torch.zeros((0, V), dtype=self.dtype)

    @torch.no_grad()
    def score_step(self, tokens, states):
        """tokens (n), states (n) context ids -> (log_probs (n, V) after the token, new states (n)).  On
        the GPU this is s2t_ngram_score, on CPU tables the same statement in numpy."""
        tokens = tokens.to(self.device)
        if self.device.type == "cuda":
            new = self._device_score(states.to(torch.int32), tokens.to(torch.int32))[1].to(torch.int64)
        else:
            new = torch.tensor([int(self._row(s)[1][t]) for s, t in zip(states.tolist(), tokens.tolist())],
                               dtype=torch.int64)
        return self._rows(new), new

    # ------------------------------------------------------------------ building the tables
    @classmethod
    def _build(cls, V, order, probs, backoffs, missing_logp, dtype, names=None):
        """probs: {context + (token,): natural-log probability}, backoffs: {context: natural-log back-off
        weight}, contexts as tuples of token ids with BOS first where the context begins a sentence."""
        ctxs = {g[:-1] for g in probs if len(g) >= 2} | {h for h, b in backoffs.items()
                                                         if 1 <= len(h) < order and b != 0.0}
        for h in list(ctxs):
            while len(h) > 1:                              # every suffix of a context is a context
                h = h[1:]
                ctxs.add(h)
        ctxs.discard(())
        ctxs = [()] + sorted(ctxs, key=lambda h: (len(h), h))
        ids = {h: n for n, h in enumerate(ctxs)}
        arcs = [[] for _ in ctxs]
        for g, lp in probs.items():
            if len(g) >= 2:
                arcs[ids[g[:-1]]].append((g[-1], lp))
        arcs[0] = [(c, probs.get((c,), missing_logp)) for c in range(V)]

        def longest(g):
            g = g[max(0, len(g) - (order - 1)):] if order > 1 else ()
            while g not in ids:
                g = g[1:]
            return ids[g]

        begin, tok, logp, nxt = [0], [], [], []
        for h, row in zip(ctxs, arcs):
            for c, lp in sorted(row):
                tok.append(c)
                logp.append(lp)
                nxt.append(longest(h + (c,)))
            begin.append(len(tok))
        fail = [ids[h[1:]] if h else 0 for h in ctxs]
        backoff = [backoffs.get(h, 0.0) if h else 0.0 for h in ctxs]
        return cls(V, order, begin, fail, torch.tensor(backoff, dtype=torch.float64).to(dtype), tok,
                   torch.tensor(logp, dtype=torch.float64).to(dtype), nxt, start_ctx=ids.get((BOS,), 0),
                   contexts=ctxs, names=names)

    @classmethod
    def from_arpa(cls, path_or_text, tokenizer=None, token_to_id=None, num_classes=None, missing_logp=-30.0,
                  dtype=torch.float32):
        """An ARPA file (a path, or the text itself) whose words are the model's piece strings ->
        NgramLm.  token_to_id ({piece: id}) or tokenizer (its `labels`) name the classes; with neither
        the words are decimal class ids and num_classes is needed.  `<unk>` maps to the unknown id where
        there is one (else its entries are dropped); any other word that is no class is a ValueError,
        as is every malformed line, with its number."""
        text = os.fspath(path_or_text)
        if "\n" not in text and "\\data\\" not in text:
            with open(text, encoding="utf-8") as fh:
                text = fh.read()
        names = None
        if token_to_id is None and tokenizer is not None:
            names = list(tokenizer.labels)
            token_to_id = {p: i for i, p in enumerate(names)}
        elif token_to_id is not None:
            token_to_id = dict(token_to_id)
        if num_classes is None:
            if token_to_id is None:
                raise ValueError("from_arpa needs num_classes, a tokenizer or token_to_id")
            num_classes = len(names) if names is not None else max(token_to_id.values()) + 1
        V = int(num_classes)
        if names is None and token_to_id is not None:
            names = [str(i) for i in range(V)]
            for p, i in token_to_id.items():
                if 0 <= i < V:
                    names[i] = p

        def word(w, no):
            if w == "<s>":
                return BOS
            if w == "</s>":
                return None
            if token_to_id is not None:
                i = token_to_id.get(w)
            else:
                i = int(w) if w.isdigit() else None
            if i is None and w == "<unk>":
                return None
            if i is None or not 0 <= i < V:
                raise ValueError(f"ARPA line {no}: {w!r} is not one of the model's {V} classes")
            return i

        declared, probs, backoffs = {}, {}, {}
        found, state, section, ended = {}, "head", 0, False
        for no, line in enumerate(text.split("\n"), 1):
            line = line.strip()
            if not line:
                continue
            if state == "head":
                if line != "\\data\\":
                    raise ValueError(f"ARPA line {no}: expected \\data\\, got {line!r}")
                state = "counts"
                continue
            if line == "\\end\\":
                ended = True
                state = "end"
                continue
            if state == "end":
                raise ValueError(f"ARPA line {no}: text after \\end\\")
            if line.startswith("\\"):
                if not (line.endswith("-grams:") and line[1:-7].isdigit()):
                    raise ValueError(f"ARPA line {no}: unknown section {line!r}")
                k = int(line[1:-7])
                if k not in declared or k != section + 1:
                    raise ValueError(f"ARPA line {no}: section {line!r} is not declared or out of order")
                section, state = k, "grams"
                found[k] = 0
                continue
            if state == "counts":
                head, _, cnt = line.partition("=")
                if not head.startswith("ngram ") or not head[6:].strip().isdigit() or not cnt.strip().isdigit():
                    raise ValueError(f"ARPA line {no}: expected 'ngram N=count', got {line!r}")
                k = int(head[6:])
                if not 1 <= k <= max_order() or k in declared:
                    raise ValueError(f"ARPA line {no}: order {k} is outside 1..{max_order()} or declared twice")
                declared[k] = int(cnt)
                continue
            parts = line.split()
            if len(parts) not in (section + 1, section + 2):
                raise ValueError(f"ARPA line {no}: a {section}-gram line has {section + 1} or {section + 2} fields, "
                                 f"got {len(parts)}")
            try:
                vals = [float(parts[0])] + ([float(parts[-1])] if len(parts) == section + 2 else [])
            except ValueError:
                raise ValueError(f"ARPA line {no}: not a number in {line!r}") from None
            if not all(math.isfinite(v) for v in vals):
                raise ValueError(f"ARPA line {no}: a value that is not finite in {line!r}")
            found[section] += 1
            g = tuple(word(w, no) for w in parts[1:1 + section])
            if None in g:
                continue                                   # predicts or follows </s>, or an <unk> without an id
            if BOS in g[1:]:
                raise ValueError(f"ARPA line {no}: <s> inside an n-gram")
            if g in probs or (g == (BOS,) and g in backoffs):
                raise ValueError(f"ARPA line {no}: the n-gram is listed twice")
            if len(vals) == 2:
                backoffs[g] = vals[1] * _LN10
            if g[-1] != BOS:
                probs[g] = vals[0] * _LN10
            elif len(vals) == 1:
                backoffs.setdefault(g, 0.0)
        if state == "head":
            raise ValueError("ARPA: no \\data\\ section")
        if not ended:
            raise ValueError("ARPA: no \\end\\ line")
        if not declared or sorted(declared) != list(range(1, len(declared) + 1)):
            raise ValueError(f"ARPA: the declared orders {sorted(declared)} are not 1..N")
        for k, cnt in declared.items():
            if found.get(k) != cnt:
                raise ValueError(f"ARPA: section {k} holds {found.get(k, 0)} n-grams, \\data\\ declares {cnt}")
        return cls._build(V, len(declared), probs, backoffs, float(missing_logp), dtype, names)

    @classmethod
    def estimate(cls, sequences, num_classes, order=3, discount=0.75, dtype=torch.float32):
        """Lists of token ids -> an absolute-discounting back-off model of that order.  Every sentence
        starts at `<s>`; nothing predicts an end.  In a context h with counts c(h w) over n(h) distinct
        followers, p(w | h) = (c(h w) - D) / c(h) for a follower and bo(h) p(w | h without its oldest token)
        otherwise, bo(h) chosen so that the row sums to one (a context that every class follows keeps its
        relative frequencies); the unigrams are discounted onto the uniform distribution."""
        V, order, D = int(num_classes), int(order), float(discount)
        if not 0.0 < D < 1.0 or not 1 <= order <= max_order():
            raise ValueError(f"estimate needs 0 < discount < 1 and an order in 1..{max_order()}")
        counts = {}
        for seq in sequences:
            hist = (BOS,)
            for w in seq:
                w = int(w)
                if not 0 <= w < V:
                    raise ValueError(f"token {w} is outside [0, {V})")
                for k in range(min(order, len(hist) + 1)):
                    h = hist[len(hist) - k:]
                    counts.setdefault(h, {})
                    counts[h][w] = counts[h].get(w, 0) + 1
                hist = (hist + (w,))[-max(order - 1, 1):]
        uni = counts.get((), {})
        total = sum(uni.values())
        p = {(): {w: ((max(uni.get(w, 0) - D, 0.0) + D * len(uni) / V) / total if total else 1.0 / V)
                  for w in range(V)}}
        bo = {}

        def full(h, w):
            return p[h][w] if w in p[h] else bo[h] * full(h[1:], w)

        for h in sorted((h for h in counts if h), key=len):
            c, tot = counts[h], sum(counts[h].values())
            if len(c) == V:
                p[h], bo[h] = {w: n / tot for w, n in c.items()}, 1.0
                continue
            p[h] = {w: (n - D) / tot for w, n in c.items()}
            bo[h] = (D * len(c) / tot) / (1.0 - sum(full(h[1:], w) for w in c))
        probs = {h + (w,): math.log(v) for h, row in p.items() for w, v in row.items()}
        return cls._build(V, order, probs, {h: math.log(v) for h, v in bo.items()}, -30.0, dtype)

    def to_arpa(self):
        """The model as ARPA text that from_arpa (with this model's names and num_classes) reads back to
        equal tables."""
        if self.contexts is None:
            raise ValueError("to_arpa needs the contexts' token tuples")
        begin, _, backoff, tok, logp, _ = self._np()
        names = self.names if self.names is not None else [str(i) for i in range(self.num_classes)]
        ids = {h: n for n, h in enumerate(self.contexts)}
        spell = lambda g: " ".join("<s>" if x == BOS else names[x] for x in g)     # noqa: E731
        rows = {k: [] for k in range(1, self.order + 1)}
        if (BOS,) in ids:
            rows[1].append(f"-99\t<s>\t{float(backoff[ids[(BOS,)]]) / _LN10!r}")
        for n, h in enumerate(self.contexts):
            for a in range(int(begin[n]), int(begin[n + 1])):
                g = h + (int(tok[a]),)
                line = f"{float(logp[a]) / _LN10!r}\t{spell(g)}"
                if g in ids:
                    line += f"\t{float(backoff[ids[g]]) / _LN10!r}"
                rows[len(g)].append(line)
        out = ["\\data\\"] + [f"ngram {k}={len(rows[k])}" for k in rows] + [""]
        for k in rows:
            out += [f"\\{k}-grams:"] + rows[k] + [""]
        return "\n".join(out + ["\\end\\", ""])
