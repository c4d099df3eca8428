"""Time the chunk-carried CTC prefix beam search fused with a back-off n-gram (csrc/decode_ctc.hip
s2t_ctc_prefix_beam_ngram_chunk): what one chunk call costs, next to the plain chunk entry
(s2t_ctc_prefix_beam_chunk), the RNN-LM chunk entry (s2t_ctc_prefix_beam_lm_chunk; the LM at rnn_lm.yaml's
dimensions) and a chunk's share of the one-shot n-gram launch (s2t_ctc_prefix_beam_ngram), on the same
frames and in one process.

    python tools/time_ctc_ngram_stream.py [--chunk 16] [--frames 250] [--batch 16] [--runs 20] [--out FILE]

The inputs and the method are tools/time_ctc_stream.py's: V 128, normal logits x 3, the blank bias bisected
on the device so that the plain search emits about `--tokens` tokens per utterance, beam 4 / top-k 4.  The
n-gram is tools/bench_ctc_ngram.py's: an order-3 model from NgramLm.estimate on 20 000 seeded tokens.  A run
streams the frames in chunks of `--chunk` from a reset through the three searches, alternated chunk by
chunk; device events around every chunk call; run 0 warms up; the figure of a run is the median over its
full chunk calls after the first, the reported one the median over the runs with the spread (min .. max)
behind.  One JSON line, appended to --out when given.  Nothing is gated.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ctc_ngram import _event_ms, _stats, token_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--text-tokens", type=int, default=20000)
    ap.add_argument("--max-nodes", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speech2text_amd.model.decoding import (CtcStreamingSearch, ctc_prefix_beam_ngram_tokens, ctc_prefix_beam_tokens,
                                                ctc_streaming_search)
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    dev = torch.device("cuda:0")
    V, B, T, Tc, w = 128, args.batch, args.frames, args.chunk, args.lm_weight
    torch.manual_seed(0)
    rnn = RnnLm(RnnLmConfig(num_symbols=V, symbol_embedding_dim=512, num_rnn_layer=3)).to(dev).eval().requires_grad_(False)
    with torch.no_grad():
        rnn._logits_layer.weight.mul_(8.0)                 # a peaked LM: decisions, not near-ties
    ngram = NgramLm.estimate(token_text(V, args.text_tokens, 2), V, order=args.order).to(dev)
    raw = 3.0 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)

    def rows(bias):
        x = raw.clone()
        x[:, :, 0] += bias
        return torch.log_softmax(x, dim=-1)

    lo, hi = 0.0, 64.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        n = float(ctc_prefix_beam_tokens(rows(mid), lens, 4, 4)[1].float().mean())
        lo, hi = (mid, hi) if n > args.tokens else (lo, mid)
    x = rows(0.5 * (lo + hi))
    pieces = [x[:, t:t + Tc].contiguous() for t in range(0, T, Tc)]
    full = [i for i, p in enumerate(pieces) if p.shape[1] == Tc and i > 0]
    kw = dict(batch_size=B, beam_size=4, cutoff_top_k=4, max_tokens=T, max_nodes=args.max_nodes, device=dev)
    searches = {"ngram": ctc_streaming_search(V, lm=ngram, lm_weight=w, **kw),
                "plain": CtcStreamingSearch(V, **kw),
                "rnn_lm": CtcStreamingSearch(V, lm=rnn, lm_weight=w, **kw)}
    one_shot = lambda: ctc_prefix_beam_ngram_tokens(x, lens, ngram, w, 4, 4)                               # noqa: E731
    times = {k: [] for k in searches}
    t_one = []
    for run in range(args.runs + 1):                       # (run 0 warms up)
        for s in searches.values():
            s.reset()
        ms = {k: [] for k in searches}
        for p in pieces:                                   # alternated chunk by chunk
            for k, s in searches.items():
                ms[k].append(_event_ms(lambda s=s: s.step(p))[0])
        one_ms, want = _event_ms(one_shot)
        if run:
            for k in searches:
                times[k].append(statistics.median([ms[k][i] for i in full]))
            t_one.append(one_ms)
    s = searches["ngram"]
    n = int(want[1].max())
    same = bool(torch.equal(s.out_len, want[1]) and torch.equal(s.score, want[2]) and torch.equal(s.lm_score, want[3])
                and torch.equal(s.tokens[:, :n], want[0][:, :n]))
    row = {"tool": "time_ctc_ngram_stream", "B": B, "frames": T, "chunk": Tc, "V": V, "beam": 4, "top_k": 4,
           "max_nodes": args.max_nodes, "lm_weight": w, "ngram_order": ngram.order, "ngram_contexts": ngram.num_ctx,
           "ngram_arcs": ngram.num_arcs, "rnn_lm_dims": "H 512 x 3",
           "tokens_per_utt_ngram": round(float(want[1].float().mean()), 1),
           "tokens_per_utt_plain": round(float(searches["plain"].out_len.float().mean()), 1),
           "ngram_chunk_call": _stats(times["ngram"]), "plain_chunk_call": _stats(times["plain"]),
           "rnn_lm_chunk_call": _stats(times["rnn_lm"]), "one_shot_ngram": _stats(t_one),
           "chunked_equals_one_shot": same, "overflow": int(s.overflow.abs().sum())}
    row["one_shot_share_of_a_chunk_ms"] = round(row["one_shot_ngram"]["median_ms"] * Tc / T, 4)
    row["ngram_over_plain"] = round(row["ngram_chunk_call"]["median_ms"] / row["plain_chunk_call"]["median_ms"], 2)
    row["rnn_lm_over_ngram"] = round(row["rnn_lm_chunk_call"]["median_ms"] / row["ngram_chunk_call"]["median_ms"], 1)
    row["chunk_call_over_its_share"] = round(row["ngram_chunk_call"]["median_ms"] / row["one_shot_share_of_a_chunk_ms"], 2)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
