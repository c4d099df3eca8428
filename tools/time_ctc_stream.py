"""Time the chunk-carried CTC prefix beam search (csrc/decode_ctc.hip s2t_ctc_prefix_beam_chunk,
s2t_ctc_prefix_beam_lm_chunk): what one chunk call costs, next to the one-shot entry on the same frames.

    python tools/time_ctc_stream.py [--chunk 16] [--frames 256] [--runs 20] [--lib PATH] [--out FILE]

The blank-biased rows of tools/bench_ctc_prefix_beam.py (V 128, normal logits x 3, the blank bias
bisected on the device so that the plain search emits about `--tokens` tokens per utterance), beam 4 /
top-k 4, B 1 and 16, the LM at the dimensions of rnn_lm.yaml (H 512, 3 layers).  A run streams the
`--frames` frames in chunks of `--chunk` from a reset; device events around every chunk call; the
first stream warms up; the figure of a run is the median over its chunk calls after the first, the
reported one the median over the runs with the spread (min .. max) behind.  Next to it (a) the one-shot
entry on the same frames divided by the number of chunks, timed the same way, and the final tokens'
equality with it.  (b) `--lib PATH` times another build of the library, e.g. one whose compaction is
compiled to a no-op (kept out of the tree): the difference of two runs of this tool is what the
compaction costs per chunk.  Nothing is gated.  One JSON line per batch size, appended to `--out`.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--max-nodes", type=int, default=4096)
    ap.add_argument("--lib", default=None, help="another build of libs2t_mi355.so to time")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speech2text_amd import _native as N
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    from speech2text_amd.model.decoding import CtcStreamingSearch, ctc_prefix_beam_lm_tokens, ctc_prefix_beam_tokens
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    dev = torch.device("cuda:0")
    V, T, Tc = 128, args.frames, args.chunk
    K = -(-T // Tc)
    torch.manual_seed(0)
    lm = RnnLm(RnnLmConfig(num_symbols=V, symbol_embedding_dim=512, num_rnn_layer=3)).to(dev).eval().requires_grad_(False)
    with torch.no_grad():
        lm._logits_layer.weight.mul_(8.0)                  # a peaked LM: decisions, not near-ties
    for B in (1, 16):
        raw = 3.0 * torch.randn(16, T, V, generator=torch.Generator().manual_seed(1))[:B].to(dev)
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
        pieces = [x[:, k * Tc:(k + 1) * Tc].contiguous() for k in range(K)]
        row = {"label": args.label, "B": B, "frames": T, "chunk": Tc, "V": V, "beam": 4, "top_k": 4,
               "max_nodes": args.max_nodes, "lm_dims": "H 512 x 3", "lm_weight": args.lm_weight}
        for kind in ("plain", "lm"):
            kw = dict(lm=lm, lm_weight=args.lm_weight) if kind == "lm" else {}
            search = CtcStreamingSearch(V, B, "beam", 4, 4, max_tokens=T, max_nodes=args.max_nodes, device=dev, **kw)
            one_shot = (lambda: ctc_prefix_beam_lm_tokens(x, lens, lm, args.lm_weight, 4, 4)) if kind == "lm" \
                else (lambda: ctc_prefix_beam_tokens(x, lens, 4, 4))
            t_chunk, t_first, t_one = [], [], []
            for run in range(args.runs + 1):               # (run 0 warms up)
                search.reset()
                ms = [_event_ms(lambda p=p: search.step(p))[0] for p in pieces]
                one_ms, want = _event_ms(one_shot)
                if run:
                    t_chunk.append(statistics.median(ms[1:]))
                    t_first.append(ms[0])
                    t_one.append(one_ms / K)
            n = int(want[1].max())
            same = bool(torch.equal(search.out_len, want[1]) and torch.equal(search.score, want[2])
                        and torch.equal(search.tokens[:, :n], want[0][:, :n]))
            row[kind] = {"chunk_call": _stats(t_chunk), "first_chunk_call": _stats(t_first),
                         "one_shot_per_chunk": _stats(t_one), "equals_one_shot": same,
                         "overflow": int(search.overflow.abs().sum()),
                         "tokens_per_utt": round(float(want[1].float().mean()), 1),
                         "stable_per_utt": round(float(search.stable_len.float().mean()), 1)}
            row[kind]["chunk_over_one_shot"] = round(row[kind]["chunk_call"]["median_ms"]
                                                     / row[kind]["one_shot_per_chunk"]["median_ms"], 2)
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
