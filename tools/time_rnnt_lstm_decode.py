"""Time the RNN-T search with the LSTM predictor: the lockstep device search (csrc/decode_lstm.hip)
against the module-by-module loop (what every decode ran before the device search existed, and
still runs for shapes the kernels refuse), on the same inputs.

    python tools/time_rnnt_lstm_decode.py [--frames 250] [--runs 10] [--warmup 2] [--lib PATH]
                                          [--label NAME]

Synthetic weights at the dimensions of the bench's C4 configuration (bench.c4_config: the LSTM
predictor and the out-projection joiner), T = 250 frames per utterance, the blank bias calibrated
on the device so that greedy emits about 40 tokens per utterance; B = 1 and B = 16; greedy with
max_token_step 1 and beam 4 / top-k 4.  Every figure is the median of `runs` device-synchronised
runs after `warmup`; one JSON line per (search, B) pair, then a table.  `--lib PATH` times another build of
the library, and `--label` names it in every row.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class _Tok:
    labels = []

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def _median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tokens", type=int, default=40, help="emitted tokens per utterance to calibrate to")
    ap.add_argument("--lib", default=None, help="another build of libs2t_mi355.so to time")
    ap.add_argument("--label", default="tree")
    args = ap.parse_args()
    from speech2text_amd import _native as N
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    import bench
    from speech2text_amd.model.decoding import RnntBeamDecoding, RnntGreedyDecoding
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    dev = torch.device("cuda:0")
    cfg = bench.c4_config()
    torch.manual_seed(0)
    pred = Predictor(cfg["predictor"]).to(dev).eval()
    join = Joiner(JoinerConfig(**cfg["joiner"])).to(dev).eval()
    with torch.no_grad():                                  # spread the logits: decisions, not near-ties
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(3.0)
    T, D = args.frames, cfg["joiner"]["input_dim"]
    hidden = torch.randn(16, T, D, generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((16,), T, dtype=torch.int64, device=dev)
    greedy = RnntGreedyDecoding(_Tok(), pred, join, max_token_step=1)
    beams = RnntBeamDecoding(_Tok(), pred, join, beam_size=4, cutoff_top_k=4)
    assert greedy._lstm_search() and beams._lstm_search()

    # blank bias behind the out-projection: bisect to about `tokens` emissions per utterance
    bias = join._out_projection[1].bias
    base, lo, hi = float(bias.detach()[0]), 0.0, 64.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        with torch.no_grad():
            bias[0] = base + mid
        n = float(greedy.greedy_tokens_lstm(hidden, lens)[1].float().mean())
        lo, hi = (mid, hi) if n > args.tokens else (lo, mid)
    print(f"# blank bias +{mid:.2f}: {n:.1f} greedy tokens per utterance of {T} frames", flush=True)

    rows = []
    for B in (1, 16):
        h, n = hidden[:B], lens[:B]
        pairs = {
            "greedy_mts1": (lambda: greedy.decode_batch(h, n),
                            lambda: [greedy._module_loop(h[b:b + 1]) for b in range(B)]),
            "beam4_top4": (lambda: beams.beam_tokens(h, n),
                           lambda: beams.beam_tokens(h, n, fused=False)),
        }
        for name, (new, old) in pairs.items():
            with torch.no_grad():
                t_new = _median_ms(new, args.runs, args.warmup)
                t_old = _median_ms(old, args.runs, max(1, args.warmup // 2))
            row = {"label": args.label, "search": name, "B": B, "T": T, "device_ms": round(t_new, 3),
                   "module_loop_ms": round(t_old, 3), "ratio": round(t_old / t_new, 2), "runs": args.runs}
            rows.append(row)
            print(json.dumps(row), flush=True)
    print("\nsearch        B   device ms   module loop ms   module / device")
    for r in rows:
        print(f"{r['search']:<12} {r['B']:>2} {r['device_ms']:>11.2f} {r['module_loop_ms']:>16.2f} {r['ratio']:>17.1f}")


if __name__ == "__main__":
    main()
