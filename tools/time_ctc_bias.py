"""Time the CTC prefix beam search with hotword biasing (csrc/decode_ctc.hip s2t_ctc_prefix_beam_bias,
s2t_ctc_prefix_beam_ngram_bias and their _chunk partners) next to the entries it extends, and show that
those entries did not pay for it.

    python tools/time_ctc_bias.py [--runs 20] [--loop-runs 1] [--parent-lib PATH] [--label NAME] [--out FILE]

Inputs: tools/bench_ctc_ngram.py's (16 x 250 frames of log-probability rows at V 128, the blank bias bisected
so that the plain search emits about 40 tokens an utterance, beam 4 / top-k 4, the order-3 n-gram of its
seeded token text) and a graph of 100 phrases of 2 to 6 tokens cut from that text.  One process, device
events around warmed calls, the entries of a group alternating call by call; every figure is the median of
its runs with the spread (min .. max) behind.

  1. one_shot     s2t_ctc_prefix_beam, _ngram, _bias, _ngram_bias through their Python wrappers, and the host
                  `_module_loop` with the same n-gram and context (the thing replaced).
  2. chunk        a 16-frame chunk call of the four streaming searches (CtcStreamingSearch,
                  CtcNgramStreamingSearch, CtcBiasStreamingSearch without and with the n-gram), each on a
                  stream of its own that is reset every 32 calls.
  3. vs_parent    (the machinery is tools/vs_parent.py's)
                  with --parent-lib (another build of libs2t_mi355.so, the parent commit's): the twelve search
                  entries (s2t_ctc_prefix_beam, _ngram, _bias, _ngram_bias, _lm and their _chunk partners, each
                  with its matching reset) of this build, of the parent's and of the parent's loaded a second
                  time from a byte copy under another name, through plain ctypes handles on the same inputs
                  (the whole-utterance entries also on the same workspace and outputs, a stream on a state
                  of its own), alternating, the three libraries' order within a figure rotating run by run
                  (no library is always the first after another figure's kernel).  Parent against parent is
                  the noise: `speed_limit_ms` is the larger parent median plus the two parents' difference,
                  `speed_missed` the figures of this build above it.  `bits_equal`: both builds' outputs compared byte for byte on every case of
                  tests/ctc_prefix_cases.PLAIN_CASES, tests/ctc_ngram_cases.CASES and
                  tests/ctc_bias_cases.CASES, every entry on every case, whole utterances and fed in 7-frame
                  chunks, the chunk entries' caller-owned state buffers included after every chunk.

One JSON line, appended to `--out` (default profiles/ctc_bias.jsonl).  Nothing is gated.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from vs_parent import alternate as _alternate, event_ms as _event_ms, same as _same  # noqa: E402
from vs_parent import speed_rule, stats as _stats, three_libraries  # noqa: E402

BEAM, TOPK, CHUNK = 4, 4, 16


class _Tok:
    labels = []

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def phrases_of(text, n, seed):
    """n distinct phrases of 2 to 6 tokens cut from the sentences of `text`."""
    g = torch.Generator().manual_seed(seed)
    out = []
    while len(out) < n:
        s = text[int(torch.randint(0, len(text), (1,), generator=g))]
        k = int(torch.randint(2, 7, (1,), generator=g))
        if len(s) < k:
            continue
        a = int(torch.randint(0, len(s) - k + 1, (1,), generator=g))
        if s[a:a + k] not in out:
            out.append(s[a:a + k])
    return out


class _Kind:
    """What a search runs with, and so which of the six families its entries are: nothing, a back-off n-gram
    (lm, weight), a hotword graph (graph, bias_weight), both, or an RNN-LM (rnn: RnnLm, weight, start token)."""

    def __init__(self, lm=None, weight=0.0, graph=None, bias_weight=1.0, rnn=None, start=-1):
        from speech2text_amd.model.decoding import rnn_lm_desc
        parts = ["lm"] if rnn is not None else ["ngram"] * (lm is not None) + ["bias"] * (graph is not None)
        self.family = "".join(p + "_" for p in parts)        # as in s2t_ctc_<family>stream_reset
        self.suffix = "".join("_" + p for p in parts)        # as in s2t_ctc_prefix_beam<suffix>[_chunk]
        self.rnn, self.lm_scored, self.biased = None, lm is not None or rnn is not None, graph is not None
        # the descriptors in front, then what the whole-utterance, the chunk and the reset entry take of it
        self.descs, self.keep, self.whole, self.chunk, self.reset = (), [], (), (), ()
        if rnn is not None:
            self.rnn, keep = rnn_lm_desc(rnn)
            self.descs, self.whole, self.chunk = (self.rnn,), (weight, start), (weight, start)
            self.keep.append(keep)
        if lm is not None:
            desc, keep = lm.desc()
            ctx = int(lm.start_ctx)
            self.descs, self.whole, self.chunk, self.reset = (desc,), (weight, ctx), (weight,), (ctx,)
            self.keep.append(keep)
        if graph is not None:
            desc, keep = graph.desc()
            self.descs, self.whole, self.chunk = self.descs + (desc,), self.whole + (bias_weight,), \
                self.chunk + (bias_weight,)
            self.keep.append(keep)


class _Raw:
    """The CTC prefix beam search entries of the library at `path` through a ctypes handle of its own."""

    def __init__(self, path, N):
        self.N, lib = N, ctypes.CDLL(path)
        for name, proto in N.parse_header().items():
            if name.startswith("s2t_ctc_"):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = proto
                setattr(self, name[4:], fn)

    def outputs(self, x, k, max_tokens=None):
        """-> (the outputs' tensors, their pointers in the entries' order up to the scores)."""
        B, T, dev, N = x.shape[0], max_tokens or x.shape[1], x.device, self.N
        o = dict(tokens=torch.zeros((B, T), dtype=torch.int64, device=dev),
                 out_len=torch.zeros((B,), dtype=torch.int64, device=dev),
                 score=torch.zeros((B,), device=dev), lm_score=torch.zeros((B,), device=dev),
                 bias_score=torch.zeros((B,), device=dev),
                 stable=torch.zeros((B,), dtype=torch.int64, device=dev),
                 ovf=torch.zeros((B,), dtype=torch.int32, device=dev))
        ptrs = (N.lp(o["tokens"]), N.lp(o["out_len"]), N.fp(o["score"])) + \
            ((N.fp(o["lm_score"]),) if k.lm_scored else ()) + ((N.fp(o["bias_score"]),) if k.biased else ())
        return o, ptrs

    def one_shot(self, x, lens, beam, topk, k, buffers=None):
        """-> (call, outputs, buffers) of the whole-utterance entry of k's family; buffers: another library's,
        so that both work on the same workspace and outputs (a timing; never where outputs are compared)."""
        N, (B, T, V) = self.N, x.shape
        if buffers is None:
            nbytes = self.ctc_prefix_beam_workspace_bytes(B, T, V, beam) if k.rnn is None else \
                self.ctc_prefix_beam_lm_workspace_bytes(k.rnn, B, T, V, beam)
            buffers = self.outputs(x, k) + (torch.empty((nbytes,), dtype=torch.uint8, device=x.device),)
        o, ptrs, ws = buffers
        fn, name = getattr(self, "ctc_prefix_beam" + k.suffix), "s2t_ctc_prefix_beam" + k.suffix
        args = k.descs + (N.fp(x), N.lp(lens), B, T, V, 0, beam, topk) + k.whole + (N.ptr(ws),) + ptrs

        def call():
            N.check(fn(*args, N.stream()), name)
            return ws
        return call, o, buffers

    def stream(self, x, beam, topk, max_tokens, max_nodes, k):
        """-> (reset, chunk(chunk, chunk_len), outputs, state) of the chunk entries of k's family.  The state
        (and the LM family's workspace) starts as one byte pattern, so that what no kernel writes, the
        padding behind every array, is the same in two libraries' buffers."""
        N, (B, _, V) = self.N, x.shape
        o, ptrs = self.outputs(x, k, max_tokens)
        head = () if k.rnn is None else (k.rnn,)
        size = getattr(self, "ctc_" + k.family + "stream_state_bytes")(*head, B, V, beam, max_nodes)
        state = torch.full((size,), 0xA5, dtype=torch.uint8, device=x.device)
        ws = None if k.rnn is None else torch.full((self.ctc_prefix_beam_lm_chunk_workspace_bytes(k.rnn, B, V, beam),),
                                                   0xA5, dtype=torch.uint8, device=x.device)
        reset_fn = getattr(self, "ctc_" + k.family + "stream_reset")
        chunk_fn = getattr(self, f"ctc_prefix_beam{k.suffix}_chunk")
        shape = (N.ptr(state), None, B, V, beam, max_nodes)
        reset_args = shape + k.reset if k.rnn is None else (k.rnn, k.whole[1]) + shape + (N.ptr(ws),)
        mem = (max_tokens, max_nodes, N.ptr(state)) + (() if ws is None else (N.ptr(ws),))
        tail = mem + ptrs + (N.lp(o["stable"]), N.ip(o["ovf"]))

        def reset():
            N.check(reset_fn(*reset_args, N.stream()), f"s2t_ctc_{k.family}stream_reset")

        def chunk(ch, cl):
            rc = chunk_fn(*k.descs, N.fp(ch), N.lp(cl), B, ch.shape[1], V, 0, beam, topk, *k.chunk, *tail, N.stream())
            N.check(rc, f"s2t_ctc_prefix_beam{k.suffix}_chunk")
            return ws
        return reset, chunk, o, state


FAMILIES = ("plain", "ngram", "bias", "ngram_bias", "lm")


def _kinds(V, dev, lm, weight, graph, bias_weight, start=-1):
    """{family: _Kind} on V classes: the n-gram and the graph given, and a seeded RNN-LM of one layer."""
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    torch.manual_seed(1000 + V)
    rnn = RnnLm(config=RnnLmConfig(num_symbols=V, symbol_embedding_dim=16, num_rnn_layer=1)).to(dev).eval()
    return {"plain": _Kind(), "ngram": _Kind(lm=lm, weight=weight), "bias": _Kind(graph=graph, bias_weight=bias_weight),
            "ngram_bias": _Kind(lm=lm, weight=weight, graph=graph, bias_weight=bias_weight),
            "lm": _Kind(rnn=rnn, weight=weight, start=start)}


def _cases(dev):
    """Every plain, n-gram and bias test case as (name, settings, logits, lengths, n-gram, graph): what a case
    does not bring (the plain cases an n-gram and a graph, the n-gram cases a graph, the bias cases without an
    LM an n-gram) is estimated on, or cut from, tests/ctc_ngram_cases.py's seeded token text at the case's V."""
    import ctc_bias_cases as BC
    import ctc_ngram_cases as NC
    import ctc_prefix_cases as PC
    from speech2text_amd.model.lm.context_graph import ContextGraph
    from speech2text_amd.model.lm.ngram_lm import NgramLm

    def stand_in_lm(V):
        return NgramLm.estimate(NC.lm_sequences(V, 120, 1), V, order=2)

    def stand_in_graph(V):
        return ContextGraph(phrases_of(NC.lm_sequences(V, 120, 1), 3, 5), V, context_score=1.0)

    out = []
    for n in PC.PLAIN_CASES:
        c = PC.CASES[n]
        out.append((n, c, *PC.make(n)[:2], stand_in_lm(c["V"]), stand_in_graph(c["V"])))
    for n, c in NC.CASES.items():
        out.append((n, c, *NC.make(n), NgramLm.from_arpa(NC.text_of(n), num_classes=c["V"]), stand_in_graph(c["V"])))
    for n, c in BC.CASES.items():
        out.append((n, c, *BC.make(n), BC.model_of(n) if c["order"] else stand_in_lm(c["V"]), BC.graph_of(n)))
    return [(n, c, x.to(dev), lens.to(dev), lm.to(dev), graph.to(dev)) for n, c, x, lens, lm, graph in out]


def _bits_equal(tree, parent, dev):
    """Both libraries' twelve search entries on every case, whole and in 7-frame chunks, the chunk entries'
    state buffers compared byte for byte after every chunk -> (cases, equal, [what differed])."""
    cases, differ = _cases(dev), []
    for i, (name, c, x, lens, lm, graph) in enumerate(cases):
        T, V = x.shape[1], x.shape[2]
        kinds = _kinds(V, dev, lm, c.get("weight") or 0.5, graph, c.get("bias_weight", 1.0), V - 1 if i % 2 else -1)
        for fam, k in kinds.items():
            whole = [lib.one_shot(x, lens, c["beam"], c["topk"], k) for lib in (tree, parent)]
            for call, _, _ in whole:
                call()
            torch.cuda.synchronize()
            if not _same(whole[0][1].values(), whole[1][1].values()):
                differ.append(f"{name}:{fam}")
            streams = [lib.stream(x, c["beam"], c["topk"], T, 1 + c["beam"] * T, k) for lib in (tree, parent)]
            for reset, _, _, _ in streams:
                reset()
            for t0 in range(0, T, 7):
                ch = x[:, t0:t0 + 7].contiguous()
                cl = (lens.clamp(max=T) - t0).clamp(0, ch.shape[1])
                for _, chunk, _, _ in streams:
                    chunk(ch, cl)
                torch.cuda.synchronize()
                (_, _, oa, sa), (_, _, ob, sb) = streams
                if not _same([sa, *oa.values()], [sb, *ob.values()]):
                    differ.append(f"{name}:{fam}_chunk@{t0}")
                    break
    return len(cases), not differ, differ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--loop-runs", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="another build of libs2t_mi355.so: the parent commit's")
    ap.add_argument("--label", default=None, help="kept in the JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_bias.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ctc_bias.py measures on the GPU; there is none here")
    from bench_ctc_ngram import token_text
    from speech2text_amd import _native as N
    from speech2text_amd.model.ctc_bias import (CtcBiasPrefixBeamDecoding, CtcBiasStreamingSearch,
                                                ctc_prefix_beam_bias_tokens)
    from speech2text_amd.model.decoding import (CtcNgramStreamingSearch, CtcStreamingSearch,
                                                ctc_prefix_beam_ngram_tokens, ctc_prefix_beam_tokens)
    from speech2text_amd.model.lm.context_graph import ContextGraph
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    dev = torch.device("cuda:0")
    V, B, T, lm_w, bias_w = 128, 16, 250, 0.3, 1.0
    text = token_text(V, 20000, 2)
    ngram = NgramLm.estimate(text, V, order=3).to(dev)
    graph = ContextGraph(phrases_of(text, 100, 3), V, context_score=1.0).to(dev)
    raw = 3.0 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)

    def rows(bias):
        x = raw.clone()
        x[:, :, 0] += bias
        return torch.log_softmax(x, dim=-1)

    lo, hi = 0.0, 64.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        n = float(ctc_prefix_beam_tokens(rows(mid), lens, BEAM, TOPK)[1].float().mean())
        lo, hi = (mid, hi) if n > 40 else (lo, mid)
    x = rows(0.5 * (lo + hi))

    # ---- 1. one-shot
    one = {"plain": lambda: ctc_prefix_beam_tokens(x, lens, BEAM, TOPK),
           "ngram": lambda: ctc_prefix_beam_ngram_tokens(x, lens, ngram, lm_w, BEAM, TOPK),
           "bias": lambda: ctc_prefix_beam_bias_tokens(x, lens, graph, bias_w, None, 0.0, BEAM, TOPK),
           "ngram_bias": lambda: ctc_prefix_beam_bias_tokens(x, lens, graph, bias_w, ngram, lm_w, BEAM, TOPK)}
    row = {"tool": "time_ctc_bias", "B": B, "T": T, "V": V, "beam": BEAM, "top_k": TOPK, "lm_weight": lm_w,
           "bias_weight": bias_w, "ngram_contexts": ngram.num_ctx, "ngram_arcs": ngram.num_arcs,
           "graph_phrases": 100, "graph_states": graph.num_ctx, "graph_arcs": graph.num_arcs,
           "gpu": torch.cuda.get_device_name(0)}
    row["one_shot"] = _alternate(one, args.runs)
    outs = {k: fn() for k, fn in one.items()}
    dec = CtcBiasPrefixBeamDecoding(_Tok(), beam_size=BEAM, cutoff_top_k=TOPK, lm=ngram, lm_weight=lm_w, context=graph,
                                    context_weight=bias_w)
    dec.beam_tokens(x[:1, :20], torch.full((1,), 20, dtype=torch.int64, device=dev), fused=False)
    t_loop = []
    for _ in range(args.loop_runs):
        ms, out_loop = _event_ms(lambda: dec.beam_tokens(x, lens, fused=False))
        t_loop.append(ms)
    row["one_shot"]["host_loop_ngram_bias"] = _stats(t_loop)
    med = {k: v["median_ms"] for k, v in row["one_shot"].items()}
    row["tokens_per_utt"] = {k: round(float(o[1].float().mean()), 1) for k, o in outs.items()}
    row["bias_changes_utterances"] = int((outs["plain"][0] != outs["bias"][0]).any(dim=1).sum())
    row["ngram_bias_changes_utterances"] = int((outs["ngram"][0] != outs["ngram_bias"][0]).any(dim=1).sum())
    row["mean_bias_score"] = round(float(outs["ngram_bias"][-1].mean()), 2)
    row["ngram_bias_equals_loop"] = bool(torch.equal(outs["ngram_bias"][0], out_loop[0]))
    row["bias_over_plain"] = round(med["bias"] / med["plain"], 3)
    row["ngram_over_plain"] = round(med["ngram"] / med["plain"], 3)
    row["ngram_bias_over_ngram"] = round(med["ngram_bias"] / med["ngram"], 3)
    row["loop_over_ngram_bias"] = round(med["host_loop_ngram_bias"] / med["ngram_bias"], 1)

    # ---- 2. a 16-frame chunk call
    kw = dict(batch_size=B, beam_size=BEAM, cutoff_top_k=TOPK, max_tokens=1024, max_nodes=4096, device=dev)
    searches = {"plain": CtcStreamingSearch(V, **kw),
                "ngram": CtcNgramStreamingSearch(V, lm=ngram, lm_weight=lm_w, **kw),
                "bias": CtcBiasStreamingSearch(V, context=graph, context_weight=bias_w, **kw),
                "ngram_bias": CtcBiasStreamingSearch(V, lm=ngram, lm_weight=lm_w, context=graph, context_weight=bias_w,
                                                     **kw)}
    pieces = [x[:, t0:t0 + CHUNK].contiguous() for t0 in range(0, T - CHUNK + 1, CHUNK)]
    count = {k: 0 for k in searches}

    def stepper(k):
        def step():
            if count[k] % 32 == 0:
                searches[k].reset()
            searches[k].step(pieces[count[k] % len(pieces)])
            count[k] += 1
        return step
    row["chunk"] = _alternate({k: stepper(k) for k in searches}, 4 * args.runs, warmup=2)
    cm = {k: v["median_ms"] for k, v in row["chunk"].items()}
    row["chunk_frames"] = CHUNK
    row["chunk_bias_over_plain"] = round(cm["bias"] / cm["plain"], 3)
    row["chunk_ngram_bias_over_ngram"] = round(cm["ngram_bias"] / cm["ngram"], 3)

    # ---- 3. every search entry against the parent commit's library, and that library against a copy of itself
    if args.parent_lib:
        libs = three_libraries(N.LIB_PATH, args.parent_lib, lambda path: _Raw(path, N))
        kinds = _kinds(V, dev, ngram, lm_w, graph, bias_w)
        calls, keep = {}, []
        full = torch.full((B,), CHUNK, dtype=torch.int64, device=dev)
        for fam in FAMILIES:
            steps, shared = {}, None
            for who, lib in libs.items():
                calls[f"{fam}_{who}"], o, shared = lib.one_shot(x, lens, BEAM, TOPK, kinds[fam], shared)
                reset, chunk, so, state = lib.stream(x, BEAM, TOPK, 1024, 4096, kinds[fam])
                keep.append((o, so, state))
                n = [0]

                def step(reset=reset, chunk=chunk, n=n):
                    if n[0] % 32 == 0:
                        reset()
                    chunk(pieces[n[0] % len(pieces)], full)
                    n[0] += 1
                steps[f"{fam}_chunk_{who}"] = step
            calls.update(steps)
        row["vs_parent"] = _alternate(calls, 4 * args.runs, group=len(libs))
        # the rule: the tree's median is at most the larger parent median plus the two parents' difference
        speed_rule(row, [f + c for f in FAMILIES for c in ("", "_chunk")])
        row["bits_equal_cases"], row["bits_equal"], row["bits_differ"] = _bits_equal(libs["tree"], libs["parent"], dev)
    if args.label:
        row["label"] = args.label
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
