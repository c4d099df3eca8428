"""Time the chunk-carried RNN-T beam search with RNN-LM shallow fusion at the
dimensions of the reference's YAMLs: the LSTM predictor (E = H = 512, 3 layers, D 256, V 128,
out-projection inner 256, relu) and the stateless predictor (E 512, D 256, ctx 5, V 128, no
out-projection), each with the LM of rnn_lm.yaml (H 512, 3 layers, V 128); chunks of Tc = 16 encoder
frames (--tc), beam 4 / top-k 4, B in {1, 16}.

    python tools/time_rnnt_lm_stream.py [--reps 40] [--chunks 8] [--tc 16] [--lib PATH] [--label NAME] [--out FILE]
                                        [batch ...]

Per family and batch size, medians over `reps` warmed chunk calls on random am (streams running on,
reset once per `chunks` calls outside the timed call), and beside them
  (a) the same family's chunk call without an LM, where one exists (the LSTM family's
      s2t_rnnt_beam_lstm_chunk; the lockstep rounds over the stateless predictor exist with an LM only);
  (b) the one-shot fused call on the same Tc * chunks frames, divided by chunks.
Each figure is a host clock around one call that ends in a device synchronise -- what a caller waits
for, the enqueue of the rounds included -- and next to it the device time between two events around the
same call.  Nothing is asserted: the reading is whether carrying state costs anything over (b).
`--lib PATH` times another build of the library, `--label` names it in the row.
Prints one JSON line per family and batch size (and appends it to --out)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_lstm_stream_search import _stats, _timed  # noqa: E402


def _pairs(dev, V, D):
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    torch.manual_seed(0)
    lstm = Predictor({"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": D, "symbol_embedding_dim": 512, "num_lstm_layers": 3,
        "lstm_hidden_dim": 512, "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}})
    lstm_join = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=256, activation="relu", use_out_project=True))
    stateless = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D,
                                                            "symbol_embedding_dim": 512, "context_size": 5}})
    stateless_join = Joiner(JoinerConfig(input_dim=D, output_dim=V, activation="relu", use_out_project=False))
    out = {}
    for name, (p, j) in (("lstm", (lstm, lstm_join)), ("stateless", (stateless, stateless_join))):
        with torch.no_grad():
            for q in list(p.parameters()) + list(j.parameters()):
                q.mul_(3.0)
        out[name] = (p.to(dev).eval(), j.to(dev).eval())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--chunks", type=int, default=8)
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
    from speech2text_amd.model.decoding import (RnntLstmStreamingSearch, rnnt_beam_lstm_lm_tokens_from_am,
                                                rnnt_beam_stateless_lm_tokens_from_am, rnnt_streaming_search)
    from speech2text_amd.model.lm.rnn_lm import RnnLm, RnnLmConfig
    dev = torch.device("cuda:0")
    V, D, Tc, K, weight = 128, 256, args.tc, args.chunks, 0.3
    pairs = _pairs(dev, V, D)
    torch.manual_seed(1)
    lm = RnnLm(config=RnnLmConfig(num_symbols=V, symbol_embedding_dim=512, num_rnn_layer=3)).to(dev).eval()
    one_shot = {"lstm": rnnt_beam_lstm_lm_tokens_from_am, "stateless": rnnt_beam_stateless_lm_tokens_from_am}
    for family, (pred, join) in pairs.items():
        for B in args.batch or [1, 16]:
            row = {"label": args.label, "family": family, "B": B, "V": V, "D": D, "Tc": Tc, "chunks": K,
                   "beam": 4, "topk": 4, "lm": "H 512 x 3", "lm_weight": weight, "reps": args.reps}
            g = torch.Generator().manual_seed(B)
            am_all = (torch.randn(B, Tc * K, V, generator=g) * 3.0).to(dev)
            ams = [am_all[:, k * Tc:(k + 1) * Tc].contiguous() for k in range(K)]
            lens = torch.full((B,), Tc * K, dtype=torch.int64, device=dev)
            kw = dict(beam_size=4, cutoff_top_k=4, max_tokens=Tc * K, device=dev)
            with torch.no_grad():
                runs = [("lm_chunk", rnnt_streaming_search(pred, join, B, "beam", lm=lm, lm_weight=weight, **kw))]
                if family == "lstm":
                    runs.append(("chunk_without_lm", RnntLstmStreamingSearch(pred, join, B, "beam", **kw)))
                for key, s in runs:
                    for k in range(K):
                        s.step(ams[k])
                    wall, devms = _timed(lambda i: s.step(ams[i % K]), args.reps,
                                         between=lambda i: s.reset() if i % K == 0 else None)
                    row[key] = {"wall": _stats(wall), "device": _stats(devms),
                                "state_bytes_per_stream": s.state.numel() // B}
                whole = lambda i: one_shot[family](am_all, lens, pred, join, lm, weight, 4, 4)   # noqa: E731
                out = whole(0)
                s = runs[0][1]
                s.reset()
                for k in range(K):
                    got = s.step(ams[k])
                row["lm_chunk"]["tokens_per_frame"] = round(float(s.out_len.sum()) / (B * Tc * K), 3)
                row["lm_chunk"]["equals_one_shot"] = bool(torch.equal(got[2], out[2]) and torch.equal(got[3], out[3])
                                                          and torch.equal(s.lm_score, out[4]))
                wall, devms = _timed(whole, max(5, args.reps // K))
                row["one_shot_per_chunk"] = {"wall": _stats(wall, K), "device": _stats(devms, K)}
            line = json.dumps(row)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
