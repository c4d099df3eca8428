"""Time the chunk-carried RNN-T search and the streaming recogniser at the C3 dimensions (DESIGN.md
§3l): V 128, D 256, E 512, ctx 5, relu; encoder of tools/bench_stream.py with chunk 32, so a chunk is
Tc = 16 encoder frames = 0.64 s of audio; B in {1, 16}.

    python tools/bench_stream_search.py [--reps 60] [--out FILE] [batch ...]

Per batch size, medians over `reps` steps after a warm-up, every step bracketed by device events:
  (a) the chunk search launch alone on a random am chunk, greedy (max_token_step 5) and beam 4 / top-k 4,
      streams running on (no reset inside the window; max_tokens 1024, reset once per 64 steps outside it);
  (b) one StreamingRecognizer.step: copy-in + ONE graph replay of CMVN -> streaming_step -> enc_proj ->
      search -> state copy-back;
  (c) the same work issued eagerly: StreamingSession.step (the encoder's own graph), joiner._enc_proj,
      RnntStreamingSearch.step -- three pieces a caller would have to order itself;
(b) and (c) alternate in blocks of 10 steps, so that what else runs on the host touches both alike.
Prints one JSON line per batch size (and appends it to --out)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_stream import CFG  # noqa: E402


def _steps_ms(fn, reps, between=None):
    """Median and spread of fn()'s device time, one event pair per call."""
    ms = []
    for i in range(reps):
        if between is not None:
            between(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def _stats(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": round(statistics.median(ms), 4), "p10_ms": round(q[0], 4), "p90_ms": round(q[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    ap.add_argument("batch", nargs="*", type=int)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    from speech2text_amd.model.decoding import RnntStreamingSearch
    from speech2text_amd.model.encoder.zipformer import Zipformer2, Zipformer2Config
    from speech2text_amd.model.encoder.zipformer_streaming import StreamingRecognizer, StreamingSession
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    dev = torch.device("cuda:0")
    V, D, E, ctx, chunk = 128, 256, 512, 5, 32
    Tc, T = chunk // 2, 2 * chunk + 13
    torch.manual_seed(0)
    enc = Zipformer2(Zipformer2Config(**CFG)).to(dev).eval()
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D,
                                                       "symbol_embedding_dim": E, "context_size": ctx}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, activation="relu", prune_range=5,
                               use_out_project=False))
    with torch.no_grad():
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(4.0)                                    # (tokens on a share of the frames, as trained weights give)
    pred.to(dev).eval()
    join.to(dev).eval()
    for B in args.batch or [1, 16]:
        row = {"B": B, "V": V, "D": D, "E": E, "ctx": ctx, "chunk": chunk, "Tc": Tc, "reps": args.reps}
        xs = [torch.randn(B, T, 80, device=dev) for _ in range(8)]
        ams = [torch.randn(B, Tc, V, device=dev) * 3.0 for _ in range(8)]
        with torch.no_grad():
            for method in ("greedy", "beam"):
                s = RnntStreamingSearch(pred, join, B, method, max_token_step=5, beam_size=4, cutoff_top_k=4,
                                        device=dev)
                it = [0]

                def launch():
                    s.step(ams[it[0] % 8])
                    it[0] += 1

                for _ in range(10):
                    launch()
                ms = _steps_ms(launch, args.reps, between=lambda i: s.reset() if i % 64 == 0 else None)
                row[f"search_{method}"] = _stats(ms)
                row[f"search_{method}_tokens_per_frame"] = round(
                    float(s.out_len.sum()) / (B * Tc * (args.reps - 64 * ((args.reps - 1) // 64))), 3)
                row[f"search_{method}_state_bytes_per_stream"] = s.state.numel() // B
            for method in ("greedy", "beam"):
                kw = dict(max_token_step=5, beam_size=4, cutoff_top_k=4)
                rec = StreamingRecognizer(enc, pred, join, None, batch_size=B, method=method, device=dev, **kw)
                sess = StreamingSession(enc, B, dev)
                eager = RnntStreamingSearch(pred, join, B, method, device=dev, **kw)
                it = [0, 0]

                def replay():
                    rec.step(xs[it[0] % 8])
                    it[0] += 1

                def pieces():
                    out = sess.step(xs[it[1] % 8])
                    eager.step(join._enc_proj(out).float().contiguous())
                    it[1] += 1

                same = True
                for _ in range(10):                         # warm-up, and: the two give the same bits
                    replay()
                    pieces()
                    live = torch.arange(eager.max_tokens, device=dev) < eager.out_len.unsqueeze(1)
                    same = same and torch.equal(rec.search.out_len, eager.out_len) \
                        and torch.equal(rec.search.tokens * live, eager.tokens * live)
                a, b = [], []
                for blk in range(max(1, args.reps // 10)):
                    if blk % 6 == 0:
                        rec.reset()
                        sess.reset()
                        eager.reset()
                    a += _steps_ms(replay, 10)
                    b += _steps_ms(pieces, 10)
                row[f"recognizer_step_{method}"] = _stats(a)
                row[f"eager_pieces_{method}"] = _stats(b)
                row[f"recognizer_equals_eager_{method}"] = bool(same)
        row["audio_s_per_s_recognizer_beam"] = round(B * 0.64 / (row["recognizer_step_beam"]["median_ms"] * 1e-3))
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
