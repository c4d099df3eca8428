"""Time the CTC prefix beam search on the device (csrc/decode_ctc.hip): the plain entry
(s2t_ctc_prefix_beam, one launch) and the entry with RNN-LM shallow fusion (s2t_ctc_prefix_beam_lm,
lockstep rounds), each next to s2t_ctc_greedy and to the host loop of the same search
(CtcPrefixBeamDecoding._module_loop), on the same inputs.

    python tools/bench_ctc_prefix_beam.py [--frames 250] [--batch 16] [--runs 20] [--loop-runs 2]

Synthetic log-probability rows at V 128 (normal logits x 3, the blank bias bisected on the device so
that the plain search emits about `--tokens` tokens per utterance), beam 4 / top-k 4, the LM at the
dimensions of rnn_lm.yaml (H 512, 3 layers).  Device events around the warmed calls; the device
entries alternate call by call in one process; every figure is the median of its runs with the spread
(min .. max) behind.  The host loops are warmed on one short utterance.  One JSON line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--loop-runs", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    args = ap.parse_args()
    from speech2text_amd.model.decoding import (CtcPrefixBeamDecoding, ctc_greedy_tokens, ctc_prefix_beam_lm_tokens,
                                                ctc_prefix_beam_tokens)
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    dev = torch.device("cuda:0")
    V, B, T = 128, args.batch, args.frames
    torch.manual_seed(0)
    lm = RnnLm(RnnLmConfig(num_symbols=V, symbol_embedding_dim=512, num_rnn_layer=3)).to(dev).eval().requires_grad_(False)
    with torch.no_grad():
        lm._logits_layer.weight.mul_(8.0)                  # a peaked LM: decisions, not near-ties
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

    plain = lambda: ctc_prefix_beam_tokens(x, lens, 4, 4)                                   # noqa: E731
    fused = lambda: ctc_prefix_beam_lm_tokens(x, lens, lm, args.lm_weight, 4, 4)            # noqa: E731
    greedy = lambda: ctc_greedy_tokens(x, lens)                                             # noqa: E731
    dec = CtcPrefixBeamDecoding(_Tok(), beam_size=4, cutoff_top_k=4)
    dec_lm = CtcPrefixBeamDecoding(_Tok(), beam_size=4, cutoff_top_k=4, lm=lm, lm_weight=args.lm_weight)
    loop = lambda: dec.beam_tokens(x, lens, fused=False)                                    # noqa: E731
    loop_lm = lambda: dec_lm.beam_tokens(x, lens, fused=False)                              # noqa: E731
    for _ in range(args.warmup):
        plain(), fused(), greedy()
    t_plain, t_fused, t_greedy, t_loop, t_loop_lm = [], [], [], [], []
    for _ in range(args.runs):                             # alternated call by call
        t_plain.append(_event_ms(plain)[0])
        t_fused.append(_event_ms(fused)[0])
        t_greedy.append(_event_ms(greedy)[0])
    out_plain, out_fused = plain(), fused()
    short = torch.full((1,), 20, dtype=torch.int64, device=dev)
    dec.beam_tokens(x[:1, :20], short, fused=False), dec_lm.beam_tokens(x[:1, :20], short, fused=False)
    for _ in range(args.loop_runs):
        ms, out_loop = _event_ms(loop)
        t_loop.append(ms)
        ms, out_loop_lm = _event_ms(loop_lm)
        t_loop_lm.append(ms)
    row = {"B": B, "T": T, "V": V, "beam": 4, "top_k": 4, "lm_dims": "H 512 x 3", "lm_weight": args.lm_weight,
           "tokens_per_utt_plain": round(float(out_plain[1].float().mean()), 1),
           "tokens_per_utt_lm": round(float(out_fused[1].float().mean()), 1),
           "plain_equals_loop": bool(torch.equal(out_plain[0], out_loop[0])),
           "lm_equals_loop": bool(torch.equal(out_fused[0], out_loop_lm[0])),
           "plain": _stats(t_plain), "lm": _stats(t_fused), "ctc_greedy": _stats(t_greedy),
           "host_loop": _stats(t_loop), "host_loop_lm": _stats(t_loop_lm)}
    row["loop_over_plain"] = round(row["host_loop"]["median_ms"] / row["plain"]["median_ms"], 1)
    row["loop_lm_over_lm"] = round(row["host_loop_lm"]["median_ms"] / row["lm"]["median_ms"], 1)
    row["plain_over_greedy"] = round(row["plain"]["median_ms"] / row["ctc_greedy"]["median_ms"], 1)
    row["lm_over_plain"] = round(row["lm"]["median_ms"] / row["plain"]["median_ms"], 1)
    print(json.dumps(row), flush=True)
    assert row["plain"]["median_ms"] < row["host_loop"]["median_ms"], "the plain entry is not faster than the host loop"
    assert row["lm"]["median_ms"] < row["host_loop_lm"]["median_ms"], "the LM entry is not faster than the host loop"


if __name__ == "__main__":
    main()
