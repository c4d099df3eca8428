"""Time the chunk-carried RNN-T search with the LSTM predictor at the dimensions of
the reference's LSTM YAMLs: E = H = 512, 3 layers, D 256, V 128, out-projection inner 256, relu;
chunks of Tc = 16 encoder frames (--tc); B in {1, 16}.

    python tools/bench_lstm_stream_search.py [--reps 40] [--chunks 8] [--blank 0] [--tc 16] [--lib PATH]
                                            [--label NAME] [--out FILE] [batch ...]

Per batch size, medians over `reps` chunk calls after a warm-up on random am (streams running on,
reset once per `chunks` calls outside the timed call):
  greedy at max_token_step 1 and 5, capturable (every round enqueued, no host read) and with the
  host poll (blocks of 32 rounds, one read of the live counter each); beam 4 / top-k 4.
Each figure is a host clock around one call that ends in a device synchronise -- what a caller
waits for, the enqueue of the rounds included -- and next to it the device time between two events
around the same call.  Each is set against the whole-utterance call on the same Tc * chunks frames,
divided by chunks.  --blank lifts the blank logit behind the out-projection (fewer emissions: fewer
predictor steps do work).  `--lib PATH` times another build of the library, `--label` names it in the
row.  Prints one JSON line per batch size (and appends it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn, reps, between=None):
    """-> (wall ms, device ms) per call; every call ends in a synchronise."""
    wall, devms = [], []
    for i in range(reps):
        if between is not None:
            between(i)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn(i)
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        devms.append(e0.elapsed_time(e1))
    return wall, devms


def _stats(ms, div=1):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms) / div, 4), "p10_ms": round(q[0] / div, 4),
            "p90_ms": round(q[-1] / div, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--chunks", type=int, default=8)
    ap.add_argument("--blank", type=float, default=0.0)
    ap.add_argument("--tc", type=int, default=16, help="frames per chunk")
    ap.add_argument("--lib", default=None, help="another build of libs2t_mi355.so to time")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("batch", nargs="*", type=int)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    from speech2text_amd import _native as N
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    from speech2text_amd.model.decoding import (RnntLstmStreamingSearch, rnnt_beam_lstm_tokens_from_am,
                                                rnnt_greedy_lstm_tokens_from_am)
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    dev = torch.device("cuda:0")
    V, D, E, H, L, inner, Tc, K = 128, 256, 512, 512, 3, 256, args.tc, args.chunks
    torch.manual_seed(0)
    pred = Predictor({"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": D, "symbol_embedding_dim": E, "num_lstm_layers": L,
        "lstm_hidden_dim": H, "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=inner, activation="relu", use_out_project=True))
    with torch.no_grad():
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(3.0)
        join._out_projection[1].bias[0] += args.blank
    pred.to(dev).eval()
    join.to(dev).eval()
    for B in args.batch or [1, 16]:
        row = {"label": args.label, "B": B, "V": V, "D": D, "E": E, "H": H, "layers": L, "inner": inner,
               "Tc": Tc, "chunks": K, "reps": args.reps, "blank": args.blank}
        g = torch.Generator().manual_seed(B)
        am_all = (torch.randn(B, Tc * K, V, generator=g) * 3.0).to(dev)
        ams = [am_all[:, k * Tc:(k + 1) * Tc].contiguous() for k in range(K)]
        lens = torch.full((B,), Tc * K, dtype=torch.int64, device=dev)
        runs = [("greedy", mts, cap) for mts in (1, 5) for cap in (True, False)] + [("beam", 0, True)]
        with torch.no_grad():
            for method, mts, cap in runs:
                key = "beam" if method == "beam" else f"greedy_mts{mts}_{'capturable' if cap else 'host_poll'}"
                s = RnntLstmStreamingSearch(pred, join, B, method, max_token_step=mts, beam_size=4, cutoff_top_k=4,
                                            max_tokens=Tc * K * (mts + 1), device=dev, capturable=cap)
                for k in range(K):
                    s.step(ams[k])
                wall, devms = _timed(lambda i: s.step(ams[i % K]), args.reps,
                                     between=lambda i: s.reset() if i % K == 0 else None)
                row[key] = {"wall": _stats(wall), "device": _stats(devms)}
                if cap or method == "beam":
                    row[key]["tokens_per_frame"] = round(float(s.out_len.sum()) / (B * Tc * ((args.reps - 1) % K + 1)), 3)
                    row[key]["state_bytes_per_stream"] = s.state.numel() // B
                if cap:                                    # the whole-utterance call on the same frames
                    if method == "beam":
                        whole = lambda i: rnnt_beam_lstm_tokens_from_am(am_all, lens, pred, join, 4, 4)   # noqa: E731
                    else:
                        whole = lambda i, m=mts: rnnt_greedy_lstm_tokens_from_am(am_all, lens, pred, join, m)  # noqa: E731
                    out = whole(0)
                    s.reset()
                    for k in range(K):
                        got = s.step(ams[k])
                    n = out[-2] if method == "beam" else out[1]
                    row[key]["equals_whole_utterance"] = bool(torch.equal(got[-3] if method == "beam" else got[1], n))
                    wall, devms = _timed(whole, max(5, args.reps // K))
                    name = "whole_beam_per_chunk" if method == "beam" else f"whole_greedy_mts{mts}_per_chunk"
                    row[name] = {"wall": _stats(wall, K), "device": _stats(devms, K)}
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
