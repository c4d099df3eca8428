"""Time the CTC prefix beam search fused with a back-off n-gram (csrc/decode_ctc.hip
s2t_ctc_prefix_beam_ngram, one launch) next to the plain entry (s2t_ctc_prefix_beam, one launch), the
entry with RNN-LM shallow fusion (s2t_ctc_prefix_beam_lm, lockstep rounds; the LM at rnn_lm.yaml's
dimensions) and the n-gram host loop (CtcPrefixBeamDecoding._module_loop), on the same inputs and in one
process.

    python tools/bench_ctc_ngram.py [--frames 250] [--batch 16] [--runs 20] [--loop-runs 2] [--out FILE]

The inputs and the method are tools/bench_ctc_prefix_beam.py's: synthetic log-probability rows at V 128
(normal logits x 3, the blank bias bisected on the device so that the plain search emits about
`--tokens` tokens per utterance), beam 4 / top-k 4; device events around the warmed calls; the device
entries alternate call by call; every figure is the median of its runs with the spread (min .. max)
behind.  The n-gram is an order-3 model from NgramLm.estimate on seeded synthetic token text (a sparse
first-order source over the non-blank classes); its context and arc counts are in the line.  One JSON
line, appended to --out when given.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3),
            "runs": len(ms)}


def token_text(V, n_tokens, seed):
    """Seeded synthetic token text: sentences of 20 tokens over the classes 1..V-1, a class followed by one
    of its four likely successors four times in five."""
    g = torch.Generator().manual_seed(seed)
    succ = torch.randint(1, V, (V, 4), generator=g)
    seqs, cur, tok = [], [], 1
    for _ in range(n_tokens):
        cur.append(tok)
        if len(cur) == 20:
            seqs.append(cur)
            cur, tok = [], int(torch.randint(1, V, (1,), generator=g))
        elif float(torch.rand((), generator=g)) < 0.8:
            tok = int(succ[tok, int(torch.randint(0, 4, (1,), generator=g))])
        else:
            tok = int(torch.randint(1, V, (1,), generator=g))
    return seqs + ([cur] if cur else [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--loop-runs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--text-tokens", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speech2text_amd.model.decoding import (CtcPrefixBeamDecoding, ctc_prefix_beam_lm_tokens,
                                                ctc_prefix_beam_ngram_tokens, ctc_prefix_beam_tokens)
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    dev = torch.device("cuda:0")
    V, B, T = 128, args.batch, args.frames
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

    plain = lambda: ctc_prefix_beam_tokens(x, lens, 4, 4)                                        # noqa: E731
    fused_n = lambda: ctc_prefix_beam_ngram_tokens(x, lens, ngram, args.lm_weight, 4, 4)         # noqa: E731
    fused_r = lambda: ctc_prefix_beam_lm_tokens(x, lens, rnn, args.lm_weight, 4, 4)              # noqa: E731
    dec = CtcPrefixBeamDecoding(_Tok(), beam_size=4, cutoff_top_k=4, lm=ngram, lm_weight=args.lm_weight)
    loop = lambda: dec.beam_tokens(x, lens, fused=False)                                         # noqa: E731
    for _ in range(args.warmup):
        plain(), fused_n(), fused_r()
    t_plain, t_ngram, t_rnn, t_loop = [], [], [], []
    for _ in range(args.runs):                             # alternated call by call
        t_ngram.append(_event_ms(fused_n)[0])
        t_plain.append(_event_ms(plain)[0])
        t_rnn.append(_event_ms(fused_r)[0])
    out_plain, out_ngram, out_rnn = plain(), fused_n(), fused_r()
    short = torch.full((1,), 20, dtype=torch.int64, device=dev)
    dec.beam_tokens(x[:1, :20], short, fused=False)
    for _ in range(args.loop_runs):
        ms, out_loop = _event_ms(loop)
        t_loop.append(ms)
    row = {"tool": "bench_ctc_ngram", "B": B, "T": T, "V": V, "beam": 4, "top_k": 4, "lm_weight": args.lm_weight,
           "ngram_order": ngram.order, "ngram_contexts": ngram.num_ctx, "ngram_arcs": ngram.num_arcs,
           "ngram_text_tokens": args.text_tokens, "rnn_lm_dims": "H 512 x 3",
           "tokens_per_utt_plain": round(float(out_plain[1].float().mean()), 1),
           "tokens_per_utt_ngram": round(float(out_ngram[1].float().mean()), 1),
           "tokens_per_utt_rnn_lm": round(float(out_rnn[1].float().mean()), 1),
           "ngram_changes_utterances": int((out_plain[0] != out_ngram[0]).any(dim=1).sum()),
           "ngram_equals_loop": bool(torch.equal(out_ngram[0], out_loop[0])),
           "ngram": _stats(t_ngram), "plain": _stats(t_plain), "rnn_lm": _stats(t_rnn),
           "host_loop_ngram": _stats(t_loop)}
    row["ngram_over_plain"] = round(row["ngram"]["median_ms"] / row["plain"]["median_ms"], 2)
    row["rnn_lm_over_ngram"] = round(row["rnn_lm"]["median_ms"] / row["ngram"]["median_ms"], 1)
    row["loop_over_ngram"] = round(row["host_loop_ngram"]["median_ms"] / row["ngram"]["median_ms"], 1)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
