"""Time the RNN-T decoders on one batch at the C3 dimensions (kernel table, row
`s2t_rnnt_beam_stateless`): B = 64 utterances of T = 247 frames, V = 128, D = 256, E = 512,
ctx = 5, relu, random parameters times 4 and random encoder output (the first configuration of
tests/golden/rnnt_beam_ref*.npz is this model).

    python tools/bench_rnnt_decoders.py [--reps 30] [--loop-utts 64]

(a) s2t_rnnt_greedy_stateless at max_token_step = 1, (b) s2t_rnnt_beam_stateless at beam 4 /
top-k 4, both on the same am (device events around `reps` launches after a warm-up), and (c) the
module-by-module loop of RnntBeamDecoding on the same encoder output (host clock around a
synchronised run of `loop-utts` utterances, scaled to the batch).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--loop-utts", type=int, default=64)
    args = ap.parse_args()
    from speech2text_amd.model.decoding import (RnntBeamDecoding, RnntGreedyDecoding,
                                                rnnt_beam_tokens_from_am)
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    dev = torch.device("cuda:0")
    B, T, V, D, E, ctx = 64, 247, 128, 256, 512, 5
    torch.manual_seed(11)
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D,
                                                       "symbol_embedding_dim": E, "context_size": ctx}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, activation="relu", prune_range=5,
                               use_out_project=False))
    with torch.no_grad():
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(4.0)
    pred.to(dev)
    join.to(dev)
    enc = torch.randn(B, T, D).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64)
    greedy = RnntGreedyDecoding(None, pred, join, max_token_step=1)
    beam = RnntBeamDecoding(None, pred, join, beam_size=4, cutoff_top_k=4)
    with torch.no_grad():
        am = join._enc_proj(enc).contiguous().float()

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    from speech2text_amd import _native as N
    q = pred.predictor
    weights = (N.fp(q._embedding.weight), N.fp(q._conv.weight.reshape(E, ctx).contiguous()),
               N.fp(q._output_linear.weight), N.fp(q._output_linear.bias),
               N.fp(join._pre_proj.weight), N.fp(join._pre_proj.bias))
    lens_d = lens.to(dev)
    tok = torch.zeros((B, 2 * T), dtype=torch.int64, device=dev)
    frm = torch.zeros((B, T), dtype=torch.int64, device=dev)
    cnt = torch.zeros((B,), dtype=torch.int64, device=dev)
    sco = torch.zeros((B,), dtype=torch.float32, device=dev)
    ws = torch.empty((N.lib().s2t_rnnt_beam_workspace_bytes(B, T, V, 4),), dtype=torch.uint8, device=dev)

    def run_greedy():                                       # launches only: buffers are reused
        N.check(N.lib().s2t_rnnt_greedy_stateless(N.fp(am), N.lp(lens_d), *weights, B, T, V, E, D, ctx,
                                                  0, 1, 2 * T, 0, N.lp(tok), N.lp(cnt), N.stream()),
                "s2t_rnnt_greedy_stateless")

    def run_beam():
        N.check(N.lib().s2t_rnnt_beam_stateless(N.fp(am), N.lp(lens_d), *weights, B, T, V, E, D, ctx,
                                                0, 0, 4, 4, N.ptr(ws), N.lp(tok), N.lp(frm),
                                                N.lp(cnt), N.fp(sco), N.stream()),
                "s2t_rnnt_beam_stateless")

    with torch.no_grad():
        gemm_ms = timed(lambda: join._enc_proj(enc))
        greedy_ms = timed(run_greedy)
        beam_ms = timed(run_beam)
        greedy_ms2 = timed(run_greedy)                      # alternated: the spread of the method
        beam_ms2 = timed(run_beam)
        g_tok, g_n = greedy.greedy_tokens(enc, lens)
        b_tok, _, b_n, _ = rnnt_beam_tokens_from_am(am, lens, pred, join, 4, 4)
        n = max(1, min(args.loop_utts, B))
        beam.beam_tokens(enc[:1, :8], lens[:1].clamp(max=8), fused=False)        # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        l_tok, _, l_n, _ = beam.beam_tokens(enc[:n], lens[:n], fused=False)
        torch.cuda.synchronize()
        loop_ms = (time.perf_counter() - t0) * 1e3 * B / n
    same = sum(int(l_n[b]) == int(b_n[b]) and torch.equal(l_tok[b, :int(l_n[b])], b_tok[b, :int(b_n[b])])
               for b in range(n))
    print(json.dumps({"B": B, "T": T, "V": V, "D": D, "E": E, "ctx": ctx, "reps": args.reps,
                      "enc_proj_gemm_ms": round(gemm_ms, 4),
                      "greedy_mts1_kernel_ms": round(greedy_ms, 4),
                      "beam4_top4_kernel_ms": round(beam_ms, 4),
                      "greedy_mts1_kernel_ms_again": round(greedy_ms2, 4),
                      "beam4_top4_kernel_ms_again": round(beam_ms2, 4),
                      "module_loop_ms_per_batch": round(loop_ms, 1), "module_loop_utts": n,
                      "greedy_tokens_per_frame": round(float(g_n.sum()) / (B * T), 3),
                      "beam_tokens_per_frame": round(float(b_n.sum()) / (B * T), 3),
                      "loop_equals_fused_utts": same}))


if __name__ == "__main__":
    main()
