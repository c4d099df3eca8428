"""Time the RNN-T beam search with RNN-LM shallow fusion over the stateless predictor (csrc/decode_lstm.hip
s2t_rnnt_beam_stateless_lm) against the module loop with the LM (RnntBeamDecoding._module_loop_lm, what
ran for this call before the fused search existed) and against the one-workgroup device search without
an LM (s2t_rnnt_beam_stateless), on the same inputs.

    python tools/time_rnnt_stateless_lm.py [--frames 250] [--batch 16] [--runs 10] [--loop-runs 3]
                                           [--lib PATH] [--label NAME]

Synthetic weights at the dimensions of zipformer_stateless_pruned_rnnt.yaml (V 128, embedding 512, output
256, context 5, no out-projection) and of rnn_lm.yaml (H 512, 3 layers), beam 4 / top-k 4, the blank's
lift bisected on the device so that the search without an LM emits about `--tokens` tokens per utterance.
Device events around the warmed calls; the two device searches alternate call by call in one process;
every figure is the median of its runs with the spread (min .. max) behind.  `--lib PATH` times another
build of the library, `--label` names it in the row.  One JSON line.
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
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--loop-runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--lm-weight", type=float, default=0.3)
    ap.add_argument("--lib", default=None, help="another build of libs2t_mi355.so to time")
    ap.add_argument("--label", default="tree")
    args = ap.parse_args()
    from speech2text_amd import _native as N
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    from speech2text_amd.model.decoding import (RnntBeamDecoding, rnnt_beam_stateless_lm_tokens_from_am,
                                                rnnt_beam_tokens_from_am)
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    dev = torch.device("cuda:0")
    V, B, T = 128, args.batch, args.frames
    torch.manual_seed(0)
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": 256, "symbol_embedding_dim": 512,
                                                       "context_size": 5}})
    join = Joiner(JoinerConfig(input_dim=256, output_dim=V, activation="relu", prune_range=5, use_out_project=False))
    join._enc_proj = torch.nn.Identity()                   # the searches are handed am itself
    lm = RnnLm(RnnLmConfig(num_symbols=V, symbol_embedding_dim=512, num_rnn_layer=3))
    pred, join, lm = (m.to(dev).eval().requires_grad_(False) for m in (pred, join, lm))
    with torch.no_grad():                                  # spread the logits: decisions, not near-ties
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(3.0)
        lm._logits_layer.weight.mul_(8.0)
    am0 = 3.0 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)

    lo, hi = 0.0, 64.0                                     # no out-projection: the blank is lifted in am
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        am = am0.clone()
        am[:, :, 0] += mid
        n = float(rnnt_beam_tokens_from_am(am, lens, pred, join, 4, 4)[2].float().mean())
        lo, hi = (mid, hi) if n > args.tokens else (lo, mid)

    fused = lambda: rnnt_beam_stateless_lm_tokens_from_am(am, lens, pred, join, lm, args.lm_weight, 4, 4)  # noqa: E731
    plain = lambda: rnnt_beam_tokens_from_am(am, lens, pred, join, 4, 4)                                  # noqa: E731
    dec = RnntBeamDecoding(_Tok(), pred, join, beam_size=4, cutoff_top_k=4, lm=lm, lm_weight=args.lm_weight)
    loop = lambda: dec.beam_tokens(am, lens, fused=False)                                                 # noqa: E731
    assert fused() is not None, "the fused search refused the shape"
    for _ in range(args.warmup):
        fused(), plain()
    t_fused, t_plain, t_loop = [], [], []
    for _ in range(args.runs):                             # alternated call by call
        t_fused.append(_event_ms(fused)[0])
        t_plain.append(_event_ms(plain)[0])
    n_fused = float(fused()[2].float().mean())
    loop()
    for _ in range(args.loop_runs):
        t_loop.append(_event_ms(loop)[0])
    row = {"label": args.label, "B": B, "T": T, "beam": 4, "top_k": 4, "lm_weight": args.lm_weight,
           "tokens_per_utt_no_lm": round(n, 1), "tokens_per_utt_fused": round(n_fused, 1),
           "fused_lm": _stats(t_fused), "one_workgroup_no_lm": _stats(t_plain), "module_loop_lm": _stats(t_loop)}
    row["fused_over_no_lm"] = round(row["fused_lm"]["median_ms"] / row["one_workgroup_no_lm"]["median_ms"], 2)
    row["loop_over_fused"] = round(row["module_loop_lm"]["median_ms"] / row["fused_lm"]["median_ms"], 1)
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
