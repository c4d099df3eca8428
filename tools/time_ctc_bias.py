"""Time the CTC prefix beam search with hotword biasing (csrc/decode_ctc.hip s2t_ctc_prefix_beam_bias,
s2t_ctc_prefix_beam_ngram_bias and their _chunk partners) next to the entries it extends, and show that
those entries did not pay for it.

    python tools/time_ctc_bias.py [--runs 20] [--loop-runs 1] [--parent-lib PATH] [--out FILE]

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
  3. vs_parent    with --parent-lib (another build of libs2t_mi355.so, the parent commit's): s2t_ctc_prefix_beam,
                  _ngram, _chunk and _ngram_chunk of both libraries through plain ctypes handles on the same
                  buffers, alternating, and `bits_equal`: their outputs compared with torch.equal on every
                  case of tests/ctc_prefix_cases.PLAIN_CASES and tests/ctc_ngram_cases.CASES (whole utterances,
                  and fed in 7-frame chunks).

One JSON line, appended to `--out` (default profiles/ctc_bias.jsonl).  Nothing is gated.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BEAM, TOPK, CHUNK = 4, 4, 16


class _Tok:
    labels = []

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def _event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs": len(ms)}


def _alternate(calls, runs, warmup=3):
    """{name: fn} -> {name: stats}, the calls alternating call by call."""
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(runs):
        for k, fn in calls.items():
            times[k].append(_event_ms(fn)[0])
    return {k: _stats(v) for k, v in times.items()}


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


class _Raw:
    """The four existing CTC entries of the library at `path` through a ctypes handle of its own."""

    NAMES = ("s2t_ctc_prefix_beam_workspace_bytes", "s2t_ctc_prefix_beam", "s2t_ctc_prefix_beam_ngram",
             "s2t_ctc_stream_state_bytes", "s2t_ctc_stream_reset", "s2t_ctc_prefix_beam_chunk",
             "s2t_ctc_ngram_stream_state_bytes", "s2t_ctc_ngram_stream_reset", "s2t_ctc_prefix_beam_ngram_chunk")

    def __init__(self, path, N):
        self.N, lib, protos = N, ctypes.CDLL(path), N.parse_header()
        for name in self.NAMES:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = protos[name]
            setattr(self, name[4:], fn)

    def outputs(self, x, max_tokens=None):
        B, T, dev = x.shape[0], max_tokens or x.shape[1], x.device
        return dict(tokens=torch.zeros((B, T), dtype=torch.int64, device=dev),
                    out_len=torch.zeros((B,), dtype=torch.int64, device=dev),
                    score=torch.zeros((B,), device=dev), lm_score=torch.zeros((B,), device=dev),
                    stable=torch.zeros((B,), dtype=torch.int64, device=dev),
                    ovf=torch.zeros((B,), dtype=torch.int32, device=dev))

    def one_shot(self, x, lens, beam, topk, lm=None, weight=0.0):
        """-> (call, outputs): the plain entry, or with lm the n-gram entry."""
        N, (B, T, V) = self.N, x.shape
        o = self.outputs(x)
        ws = torch.empty((self.ctc_prefix_beam_workspace_bytes(B, T, V, beam),), dtype=torch.uint8, device=x.device)
        desc, keep = lm.desc() if lm is not None else (None, None)

        def call():
            if lm is None:
                rc = self.ctc_prefix_beam(N.fp(x), N.lp(lens), B, T, V, 0, beam, topk, N.ptr(ws), N.lp(o["tokens"]),
                                          N.lp(o["out_len"]), N.fp(o["score"]), N.stream())
            else:
                rc = self.ctc_prefix_beam_ngram(desc, N.fp(x), N.lp(lens), B, T, V, 0, beam, topk, weight,
                                                int(lm.start_ctx), N.ptr(ws), N.lp(o["tokens"]), N.lp(o["out_len"]),
                                                N.fp(o["score"]), N.fp(o["lm_score"]), N.stream())
            N.check(rc, "one-shot entry")
            return keep
        return call, o

    def stream(self, x, beam, topk, max_tokens, max_nodes, lm=None, weight=0.0):
        """-> (reset, chunk(chunk, chunk_len), outputs, state) of the plain or n-gram chunk entries."""
        N, (B, _, V) = self.N, x.shape
        o = self.outputs(x, max_tokens)
        size = self.ctc_stream_state_bytes if lm is None else self.ctc_ngram_stream_state_bytes
        state = torch.zeros((size(B, V, beam, max_nodes),), dtype=torch.uint8, device=x.device)
        desc, keep = lm.desc() if lm is not None else (None, None)

        def reset():
            if lm is None:
                rc = self.ctc_stream_reset(N.ptr(state), None, B, V, beam, max_nodes, N.stream())
            else:
                rc = self.ctc_ngram_stream_reset(N.ptr(state), None, B, V, beam, max_nodes, int(lm.start_ctx),
                                                 N.stream())
            N.check(rc, "stream reset")

        def chunk(ch, cl):
            tail = (max_tokens, max_nodes, N.ptr(state), N.lp(o["tokens"]), N.lp(o["out_len"]), N.fp(o["score"]))
            if lm is None:
                rc = self.ctc_prefix_beam_chunk(N.fp(ch), N.lp(cl), B, ch.shape[1], V, 0, beam, topk, *tail,
                                                N.lp(o["stable"]), N.ip(o["ovf"]), N.stream())
            else:
                rc = self.ctc_prefix_beam_ngram_chunk(desc, N.fp(ch), N.lp(cl), B, ch.shape[1], V, 0, beam, topk,
                                                      weight, *tail, N.fp(o["lm_score"]), N.lp(o["stable"]),
                                                      N.ip(o["ovf"]), N.stream())
            N.check(rc, "chunk entry")
            return keep
        return reset, chunk, o, state


def _bits_equal(tree, parent, dev):
    """Both libraries on every plain and n-gram test case, one-shot and in 7-frame chunks -> (cases, equal)."""
    import ctc_ngram_cases as NC
    import ctc_prefix_cases as PC
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    jobs = [(PC.CASES[n], PC.make(n)[:2], None) for n in PC.PLAIN_CASES]
    jobs += [(NC.CASES[n], NC.make(n), NgramLm.from_arpa(NC.text_of(n), num_classes=NC.CASES[n]["V"]).to(dev))
             for n in NC.CASES]
    equal = True
    for c, (x, lens), lm in jobs:
        x, lens = x.to(dev), lens.to(dev)
        T, w = x.shape[1], c.get("weight", 0.0)
        outs = []
        for lib in (tree, parent):
            call, o = lib.one_shot(x, lens, c["beam"], c["topk"], lm, w)
            call()
            reset, chunk, so, state = lib.stream(x, c["beam"], c["topk"], T, 1 + c["beam"] * T, lm, w)
            reset()
            for t0 in range(0, T, 7):
                ch = x[:, t0:t0 + 7].contiguous()
                chunk(ch, (lens.clamp(max=T) - t0).clamp(0, ch.shape[1]))
            torch.cuda.synchronize()
            outs.append(list(o.values()) + list(so.values()) + [state])
        equal = equal and all(torch.equal(a, b) for a, b in zip(*outs))
    return len(jobs), equal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--loop-runs", type=int, default=1)
    ap.add_argument("--parent-lib", default=None, help="another build of libs2t_mi355.so: the parent commit's")
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

    # ---- 3. the existing entries against the parent commit's library
    if args.parent_lib:
        libs = {"tree": _Raw(N.LIB_PATH, N), "parent": _Raw(os.path.abspath(args.parent_lib), N)}
        calls, keep = {}, []
        full = torch.full((B,), CHUNK, dtype=torch.int64, device=dev)
        for who, lib in libs.items():
            for what, lm in (("plain", None), ("ngram", ngram)):
                calls[f"{what}_{who}"], o = lib.one_shot(x, lens, BEAM, TOPK, lm, lm_w)
                reset, chunk, so, state = lib.stream(x, BEAM, TOPK, 1024, 4096, lm, lm_w)
                keep.append((o, so, state))
                n = [0]

                def step(reset=reset, chunk=chunk, n=n):
                    if n[0] % 32 == 0:
                        reset()
                    chunk(pieces[n[0] % len(pieces)], full)
                    n[0] += 1
                calls[f"{what}_chunk_{who}"] = step
        row["vs_parent"] = _alternate(calls, 4 * args.runs)
        pm = {k: v["median_ms"] for k, v in row["vs_parent"].items()}
        row["tree_over_parent"] = {k: round(pm[f"{k}_tree"] / pm[f"{k}_parent"], 4)
                                   for k in ("plain", "ngram", "plain_chunk", "ngram_chunk")}
        row["bits_equal_cases"], row["bits_equal"] = _bits_equal(libs["tree"], libs["parent"], dev)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
