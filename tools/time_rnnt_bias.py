"""Time hotword biasing in the one-launch RNN-T beam search of the stateless predictor (csrc/decode_rnnt.hip:
s2t_rnnt_beam_stateless_bias, s2t_rnnt_beam_stateless_ngram_bias and their _chunk partners) against the entries
it extends, and the host loop once.

    python tools/time_rnnt_bias.py [--runs 20] [--label NAME] [--out FILE]

Inputs: tools/time_rnnt_stateless.py's (16 x 250 frames at the zipformer YAML's V 128, E 512, D 256, ctx 5, the
blank's lift bisected so that the plain beam search emits about 40 tokens an utterance, beam 4 / top-k 4, the
order-3 n-gram of bench_ctc_ngram's seeded token text at lm_weight 0.3, 16-frame chunks) and the graph recipe of
tools/time_ctc_bias.py: 100 phrases of 2 to 6 tokens cut from the n-gram's text, context_score 1, bias_weight 1.
One process, device events around warmed calls of the Python surface (the wrappers' allocations are the same in
an entry and its partner), the four searches of a group alternating call by call (tools/vs_parent.py alternate);
every figure is the median with min and max behind.  A stream is reset every 15 chunk calls (one utterance).

The six EXISTING entries are measured against the parent commit's library by tools/time_rnnt_stateless.py
(--parent-lib, four fresh processes; its `bits_equal` covers outputs and state bytes on 13 cases): this tool adds
no second copy of that comparison.

One JSON line, appended to `--out` (default profiles/rnnt_bias.jsonl).  Nothing is gated.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_ctc_bias import _Tok, phrases_of  # noqa: E402
from time_rnnt_stateless import BEAM, CHUNK, MAX_TOKENS, TOPK, bench_inputs  # noqa: E402
from vs_parent import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--label", default=None, help="kept in the JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_bias.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rnnt_bias.py measures on the GPU; there is none here")
    from bench_ctc_ngram import token_text
    from speech2text_amd.model.decoding import (RnntNgramStreamingSearch, RnntStreamingSearch,
                                                rnnt_beam_ngram_tokens_from_am, rnnt_beam_tokens_from_am)
    from speech2text_amd.model.lm.context_graph import ContextGraph
    from speech2text_amd.model.rnnt_bias import (RnntBiasBeamDecoding, RnntBiasStreamingSearch,
                                                 rnnt_beam_bias_tokens_from_am)
    dev = torch.device("cuda:0")
    lm_w, bias_w = 0.3, 1.0
    pred, join, p, am, lens, ngram = bench_inputs(dev)
    B, T, V = am.shape
    graph = ContextGraph(phrases_of(token_text(V, 20000, 2), 100, 3), V, context_score=1.0).to(dev)

    one_shot = {
        "plain": lambda: rnnt_beam_tokens_from_am(am, lens, pred, join, BEAM, TOPK),
        "bias": lambda: rnnt_beam_bias_tokens_from_am(am, lens, pred, join, graph, bias_w, None, 0.0, BEAM, TOPK),
        "ngram": lambda: rnnt_beam_ngram_tokens_from_am(am, lens, pred, join, ngram, lm_w, BEAM, TOPK),
        "ngram_bias": lambda: rnnt_beam_bias_tokens_from_am(am, lens, pred, join, graph, bias_w, ngram, lm_w, BEAM,
                                                            TOPK)}
    outs = {k: fn() for k, fn in one_shot.items()}
    torch.cuda.synchronize()
    row = {"tool": "time_rnnt_bias", "B": B, "T": T, "V": V, "E": p.E, "D": p.D, "ctx": p.ctx, "beam": BEAM,
           "top_k": TOPK, "lm_weight": lm_w, "bias_weight": bias_w, "ngram_contexts": ngram.num_ctx,
           "ngram_arcs": ngram.num_arcs, "graph_phrases": 100, "graph_states": graph.num_ctx,
           "graph_arcs": graph.num_arcs, "chunk_frames": CHUNK, "gpu": torch.cuda.get_device_name(0),
           "tokens_per_utt": {k: round(float(o[2].float().mean()), 1) for k, o in outs.items()},
           "bias_changes_utts": {k: int((outs[k][0] != outs[q][0]).any(dim=1).sum())
                                 for k, q in (("bias", "plain"), ("ngram_bias", "ngram"))}}
    row["one_shot"] = alternate(one_shot, args.runs, group=len(one_shot))

    pieces = [am[:, t0:t0 + CHUNK].contiguous() for t0 in range(0, T - CHUNK + 1, CHUNK)]
    common = dict(beam_size=BEAM, cutoff_top_k=TOPK, max_tokens=MAX_TOKENS, device=dev)
    streams = {
        "plain": RnntStreamingSearch(pred, join, B, "beam", **common),
        "bias": RnntBiasStreamingSearch(pred, join, B, context=graph, context_weight=bias_w, **common),
        "ngram": RnntNgramStreamingSearch(pred, join, B, lm=ngram, lm_weight=lm_w, **common),
        "ngram_bias": RnntBiasStreamingSearch(pred, join, B, lm=ngram, lm_weight=lm_w, context=graph,
                                              context_weight=bias_w, **common)}
    chunked = {}
    for k, s in streams.items():
        n = [0]

        def step(s=s, n=n):
            if n[0] % len(pieces) == 0:
                s.reset()
            s.step(pieces[n[0] % len(pieces)])
            n[0] += 1
        chunked[k] = step
    row["chunk"] = alternate(chunked, 4 * args.runs, group=len(chunked))
    for part in ("one_shot", "chunk"):
        med = {k: v["median_ms"] for k, v in row[part].items()}
        row[part + "_bias_over_partner"] = {"bias": round(med["bias"] / med["plain"], 3),
                                            "ngram_bias": round(med["ngram_bias"] / med["ngram"], 3)}

    dec = RnntBiasBeamDecoding(_Tok(), pred, join, BEAM, TOPK, ngram, lm_w, None, graph, bias_w)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dec.beam_tokens(am[:1], lens[:1], fused=False)         # the host loop, once, on one utterance
    torch.cuda.synchronize()
    row["host_loop_ngram_bias_one_utt_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
    if args.label:
        row["label"] = args.label
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
