"""Time the one-launch RNN-T beam search fused with a back-off n-gram (csrc/decode_rnnt.hip
s2t_rnnt_beam_stateless_ngram) next to the plain one-workgroup entry (s2t_rnnt_beam_stateless, one launch),
the lockstep search with RNN-LM shallow fusion (s2t_rnnt_beam_stateless_lm; the LM at rnn_lm.yaml's
dimensions) and the n-gram host loop (RnntBeamDecoding._module_loop_lm, once), on the same inputs and in one
process; and a chunk call of the chunk-carried form (s2t_rnnt_beam_stateless_ngram_chunk) against its share
of the one-shot launch.

    python tools/bench_rnnt_ngram.py [--frames 250] [--batch 16] [--runs 20] [--chunk 16] [--out FILE]

The inputs and the method are tools/time_rnnt_stateless_lm.py's and tools/bench_ctc_ngram.py's: synthetic
weights at the dimensions of zipformer_stateless_pruned_rnnt.yaml (V 128, embedding 512, output 256, context
5, no out-projection), beam 4 / top-k 4, the blank's lift bisected on the device so that the plain search
emits about `--tokens` tokens per utterance; device events around the warmed calls; the device entries
alternate call by call; every figure is the median of its runs with the spread (min .. max) behind.  The
n-gram is bench_ctc_ngram's: an order-3 model from NgramLm.estimate on 20 000 seeded tokens.  The chunk
figure is the median over the calls of `--runs` passes over the utterance in chunks of `--chunk` frames.
One JSON line, appended to --out when given.  Nothing is gated.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ctc_ngram import _Tok, _event_ms, _stats, token_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--text-tokens", type=int, default=20000)
    ap.add_argument("--no-loop", action="store_true", help="skip the host loop (minutes of small launches)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speech2text_amd.model.decoding import (RnntBeamDecoding, RnntNgramStreamingSearch,
                                                rnnt_beam_ngram_tokens_from_am, rnnt_beam_stateless_lm_tokens_from_am,
                                                rnnt_beam_tokens_from_am)
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    dev = torch.device("cuda:0")
    V, B, T = 128, args.batch, args.frames
    torch.manual_seed(0)
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": 256, "symbol_embedding_dim": 512,
                                                       "context_size": 5}})
    join = Joiner(JoinerConfig(input_dim=256, output_dim=V, activation="relu", prune_range=5, use_out_project=False))
    join._enc_proj = torch.nn.Identity()                   # the searches are handed am itself
    rnn = RnnLm(RnnLmConfig(num_symbols=V, symbol_embedding_dim=512, num_rnn_layer=3))
    pred, join, rnn = (m.to(dev).eval().requires_grad_(False) for m in (pred, join, rnn))
    with torch.no_grad():                                  # spread the logits: decisions, not near-ties
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(3.0)
        rnn._logits_layer.weight.mul_(8.0)
    ngram = NgramLm.estimate(token_text(V, args.text_tokens, 2), V, order=args.order).to(dev)
    am0 = 3.0 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)

    lo, hi = 0.0, 64.0                                     # no out-projection: the blank is lifted in am
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        am = am0.clone()
        am[:, :, 0] += mid
        n = float(rnnt_beam_tokens_from_am(am, lens, pred, join, 4, 4)[2].float().mean())
        lo, hi = (mid, hi) if n > args.tokens else (lo, mid)

    w = args.lm_weight
    plain = lambda: rnnt_beam_tokens_from_am(am, lens, pred, join, 4, 4)                                  # noqa: E731
    fused_n = lambda: rnnt_beam_ngram_tokens_from_am(am, lens, pred, join, ngram, w, 4, 4)                # noqa: E731
    fused_r = lambda: rnnt_beam_stateless_lm_tokens_from_am(am, lens, pred, join, rnn, w, 4, 4)           # noqa: E731
    assert fused_n() is not None and fused_r() is not None, "a fused search refused the shape"
    for _ in range(args.warmup):
        plain(), fused_n(), fused_r()
    t_plain, t_ngram, t_rnn = [], [], []
    for _ in range(args.runs):                             # alternated call by call
        t_ngram.append(_event_ms(fused_n)[0])
        t_plain.append(_event_ms(plain)[0])
        t_rnn.append(_event_ms(fused_r)[0])
    out_plain, out_ngram, out_rnn = plain(), fused_n(), fused_r()

    # the chunk-carried form: `--chunk` frames a call
    Tc = args.chunk
    search = RnntNgramStreamingSearch(pred, join, B, 4, 4, T, dev, lm=ngram, lm_weight=w)
    pieces = [am[:, t:t + Tc].contiguous() for t in range(0, T - T % Tc, Tc)]
    tail = am[:, T - T % Tc:].contiguous() if T % Tc else None
    t_chunk = []
    for rep in range(args.warmup + args.runs):
        search.reset()
        for x in pieces:
            ms = _event_ms(lambda: search.step(x))[0]
            if rep >= args.warmup:
                t_chunk.append(ms)
        if tail is not None:
            search.step(tail)
    torch.cuda.synchronize()
    chunk_equal = all(torch.equal(a, b) for a, b in zip((search.out_len, search.score, search.lm_score), out_ngram[2:]))

    row = {"tool": "bench_rnnt_ngram", "B": B, "T": T, "V": V, "E": 512, "D": 256, "ctx": 5, "beam": 4, "top_k": 4,
           "lm_weight": w, "ngram_order": ngram.order, "ngram_contexts": ngram.num_ctx, "ngram_arcs": ngram.num_arcs,
           "ngram_text_tokens": args.text_tokens, "rnn_lm_dims": "H 512 x 3",
           "tokens_per_utt_plain": round(float(out_plain[2].float().mean()), 1),
           "tokens_per_utt_ngram": round(float(out_ngram[2].float().mean()), 1),
           "tokens_per_utt_rnn_lm": round(float(out_rnn[2].float().mean()), 1),
           "ngram_changes_utterances": int((out_plain[0] != out_ngram[0]).any(dim=1).sum()),
           "ngram": _stats(t_ngram), "plain": _stats(t_plain), "rnn_lm_lockstep": _stats(t_rnn),
           "chunk_frames": Tc, "chunk_call": _stats(t_chunk), "chunked_equals_one_shot": bool(chunk_equal)}
    row["ngram_over_plain"] = round(row["ngram"]["median_ms"] / row["plain"]["median_ms"], 2)
    row["rnn_lm_over_ngram"] = round(row["rnn_lm_lockstep"]["median_ms"] / row["ngram"]["median_ms"], 1)
    row["one_shot_share_of_a_chunk_ms"] = round(row["ngram"]["median_ms"] * Tc / T, 3)
    row["chunk_call_over_its_share"] = round(row["chunk_call"]["median_ms"] / row["one_shot_share_of_a_chunk_ms"], 2)
    if not args.no_loop:
        dec = RnntBeamDecoding(_Tok(), pred, join, beam_size=4, cutoff_top_k=4, lm=ngram, lm_weight=w)
        short = torch.full((1,), 10, dtype=torch.int64, device=dev)
        dec.beam_tokens(am[:1, :10], short, fused=False)   # warm
        ms, out_loop = _event_ms(lambda: dec.beam_tokens(am, lens, fused=False))
        row["host_loop_ngram"] = _stats([ms])
        row["loop_over_ngram"] = round(ms / row["ngram"]["median_ms"], 1)
        row["ngram_equals_loop_tokens"] = bool(torch.equal(out_ngram[0], out_loop[0]))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
