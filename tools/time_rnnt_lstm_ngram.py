"""Time the lockstep RNN-T beam search of the LSTM predictor fused with a back-off n-gram (csrc/decode_lstm.hip
s2t_rnnt_beam_lstm_ngram, s2t_rnnt_beam_lstm_ngram_chunk) next to the plain lockstep entry (s2t_rnnt_beam_lstm),
the RNN-LM entry (s2t_rnnt_beam_lstm_lm; the LM at rnn_lm.yaml's dimensions) and the n-gram host loop
(RnntBeamDecoding._module_loop_lm), on the same inputs and in one process.

    python tools/time_rnnt_lstm_ngram.py [--frames 250] [--batch 16] [--runs 10] [--chunk 16] [--loop-utts 1]
                                         [--out FILE]

The method is tools/bench_rnnt_ngram.py's: synthetic weights at the dimensions of the LSTM-predictor YAML (V 128,
embedding 512, hidden 512 x 3 layers with layer norm, output 256, out-projection 256), beam 4 / top-k 4, the
blank's lift behind the out-projection bisected on the device so that the plain search emits about `--tokens`
tokens per utterance; device events around the warmed calls; the device entries alternate call by call; every
figure is the median of its runs with the spread (min .. max) behind.  The n-gram is bench_ctc_ngram's order-3
model.  The chunk figures are the medians over the full chunk calls of `--runs` passes, the three chunk-carried
searches alternated chunk by chunk.  The host loop walks `--loop-utts` utterances once (it is a loop per
utterance: its cost per batch is that figure x batch / loop-utts).  One JSON line, appended to --out when
given.  Nothing is gated.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_ctc_ngram import _Tok, _event_ms, _stats, token_text  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--order", type=int, default=3)
    ap.add_argument("--text-tokens", type=int, default=20000)
    ap.add_argument("--loop-utts", type=int, default=1, help="utterances the host loop walks (0: skip it)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from speech2text_amd.model.decoding import (RnntBeamDecoding, RnntLstmNgramStreamingSearch, RnntLstmStreamingSearch,
                                                rnnt_beam_lstm_lm_tokens_from_am, rnnt_beam_lstm_ngram_tokens_from_am,
                                                rnnt_beam_lstm_tokens_from_am)
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    dev = torch.device("cuda:0")
    V, B, T, Tc, w = 128, args.batch, args.frames, args.chunk, args.lm_weight
    torch.manual_seed(0)
    pred = Predictor({"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": 256, "symbol_embedding_dim": 512, "num_lstm_layers": 3, "lstm_hidden_dim": 512,
        "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}})
    join = Joiner(JoinerConfig(input_dim=256, output_dim=V, inner_dim=256, activation="relu", use_out_project=True))
    join._enc_proj = torch.nn.Identity()                   # the searches are handed am itself
    rnn = RnnLm(RnnLmConfig(num_symbols=V, symbol_embedding_dim=512, num_rnn_layer=3))
    pred, join, rnn = (m.to(dev).eval().requires_grad_(False) for m in (pred, join, rnn))
    with torch.no_grad():                                  # spread the logits: decisions, not near-ties
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(3.0)
        rnn._logits_layer.weight.mul_(8.0)
    ngram = NgramLm.estimate(token_text(V, args.text_tokens, 2), V, order=args.order).to(dev)
    am = 3.0 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    bias0 = join._out_projection[1].bias[0].clone()
    lo, hi = 0.0, 256.0                                    # the blank is lifted behind the out-projection
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        join._out_projection[1].bias[0] = bias0 + mid
        n = float(rnnt_beam_lstm_tokens_from_am(am, lens, pred, join, 4, 4)[2].float().mean())
        lo, hi = (mid, hi) if n > args.tokens else (lo, mid)

    plain = lambda: rnnt_beam_lstm_tokens_from_am(am, lens, pred, join, 4, 4)                             # noqa: E731
    fused_n = lambda: rnnt_beam_lstm_ngram_tokens_from_am(am, lens, pred, join, ngram, w, 4, 4)           # noqa: E731
    fused_r = lambda: rnnt_beam_lstm_lm_tokens_from_am(am, lens, pred, join, rnn, w, 4, 4)                # noqa: E731
    assert fused_n() is not None and fused_r() is not None, "a fused search refused the shape"
    for _ in range(args.warmup):
        plain(), fused_n(), fused_r()
    t_plain, t_ngram, t_rnn = [], [], []
    for _ in range(args.runs):                             # alternated call by call
        t_ngram.append(_event_ms(fused_n)[0])
        t_plain.append(_event_ms(plain)[0])
        t_rnn.append(_event_ms(fused_r)[0])
    out_plain, out_ngram, out_rnn = plain(), fused_n(), fused_r()

    kw = dict(beam_size=4, cutoff_top_k=4, max_tokens=T, device=dev)
    searches = {"ngram": RnntLstmNgramStreamingSearch(pred, join, B, lm=ngram, lm_weight=w, **kw),
                "plain": RnntLstmStreamingSearch(pred, join, B, "beam", **kw),
                "rnn_lm": RnntLstmStreamingSearch(pred, join, B, "beam", lm=rnn, lm_weight=w, **kw)}
    pieces = [am[:, t:t + Tc].contiguous() for t in range(0, T, Tc)]
    full = [i for i, p in enumerate(pieces) if p.shape[1] == Tc]
    times = {k: [] for k in searches}
    for rep in range(args.warmup + args.runs):
        for s in searches.values():
            s.reset()
        ms = {k: [] for k in searches}
        for p in pieces:                                   # alternated chunk by chunk
            for k, s in searches.items():
                ms[k].append(_event_ms(lambda s=s: s.step(p))[0])
        if rep >= args.warmup:
            for k in searches:
                times[k].append(statistics.median([ms[k][i] for i in full]))
    s = searches["ngram"]
    chunk_equal = all(torch.equal(a, b) for a, b in zip((s.out_len, s.score, s.lm_score), out_ngram[2:]))

    row = {"tool": "time_rnnt_lstm_ngram", "B": B, "T": T, "V": V, "E": 512, "H": 512, "layers": 3, "D": 256,
           "inner": 256, "beam": 4, "top_k": 4, "lm_weight": w, "ngram_order": ngram.order,
           "ngram_contexts": ngram.num_ctx, "ngram_arcs": ngram.num_arcs, "rnn_lm_dims": "H 512 x 3",
           "tokens_per_utt_plain": round(float(out_plain[2].float().mean()), 1),
           "tokens_per_utt_ngram": round(float(out_ngram[2].float().mean()), 1),
           "tokens_per_utt_rnn_lm": round(float(out_rnn[2].float().mean()), 1),
           "ngram_changes_utterances": int((out_plain[0] != out_ngram[0]).any(dim=1).sum()),
           "ngram": _stats(t_ngram), "plain": _stats(t_plain), "rnn_lm": _stats(t_rnn), "chunk_frames": Tc,
           "ngram_chunk_call": _stats(times["ngram"]), "plain_chunk_call": _stats(times["plain"]),
           "rnn_lm_chunk_call": _stats(times["rnn_lm"]), "chunked_equals_one_shot": bool(chunk_equal)}
    row["ngram_over_plain"] = round(row["ngram"]["median_ms"] / row["plain"]["median_ms"], 3)
    row["rnn_lm_over_ngram"] = round(row["rnn_lm"]["median_ms"] / row["ngram"]["median_ms"], 2)
    row["chunk_ngram_over_plain"] = round(row["ngram_chunk_call"]["median_ms"] / row["plain_chunk_call"]["median_ms"], 3)
    row["chunk_rnn_lm_over_ngram"] = round(row["rnn_lm_chunk_call"]["median_ms"] / row["ngram_chunk_call"]["median_ms"], 2)
    if args.loop_utts > 0:
        k = min(args.loop_utts, B)
        dec = RnntBeamDecoding(_Tok(), pred, join, beam_size=4, cutoff_top_k=4, lm=ngram, lm_weight=w)
        short = torch.full((1,), 10, dtype=torch.int64, device=dev)
        dec.beam_tokens(am[:1, :10], short, fused=False)   # warm
        ms, out_loop = _event_ms(lambda: dec.beam_tokens(am[:k], lens[:k], fused=False))
        row["host_loop_ngram"] = dict(_stats([ms]), utterances=k)
        row["host_loop_ms_per_batch"] = round(ms * B / k, 1)
        row["loop_over_ngram"] = round(ms * B / k / row["ngram"]["median_ms"], 1)
        row["ngram_equals_loop_tokens"] = bool(torch.equal(out_ngram[0][:k], out_loop[0]))
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
