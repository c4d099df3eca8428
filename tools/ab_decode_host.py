"""Two versions of speech2text_amd/model/decoding.py in ONE process, their calls alternated: the tree's module
against another file (say `git show <commit>:speech2text_amd/model/decoding.py > /tmp/other.py`) over the same
library.  Separate processes differ among themselves by several per cent on the lockstep greedy figures
(the Python host layer), which hides a host-side difference of microseconds; one process does not.

    python tools/ab_decode_host.py --other /tmp/other.py [--rounds 12] [--out FILE]

(a) the whole-utterance LSTM greedy call at tools/bench_lstm_stream_search.py's shapes (B 1 and 16, 128 frames,
max_token_step 1 and 5), host clock around a synchronised call; (b) the host cost of a chunk step of four
chunk-carried searches at B 1: eight steps enqueued back to back, clocked before the synchronise.  Prints one
JSON line; per figure the median and the minimum of the rounds for `tree` and `other`."""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="another version of model/decoding.py")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    from speech2text_amd.model import decoding as tree
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.predictor.predictor import Predictor
    spec = importlib.util.spec_from_file_location("decoding_other", os.path.abspath(args.other))
    other = importlib.util.module_from_spec(spec)
    sys.modules["decoding_other"] = other
    spec.loader.exec_module(other)
    versions = (("tree", tree), ("other", other))
    dev = torch.device("cuda:0")
    V, D, E, H, L, inner, Tc, K = 128, 256, 512, 512, 3, 256, 16, 8
    torch.manual_seed(0)
    pred = Predictor({"model": "Lstm", "config": {
        "num_symbols": V, "output_dim": D, "symbol_embedding_dim": E, "num_lstm_layers": L,
        "lstm_hidden_dim": H, "lstm_layer_norm": True, "lstm_layer_norm_epsilon": 1e-3, "lstm_dropout": 0.0}})
    join = Joiner(JoinerConfig(input_dim=D, output_dim=V, inner_dim=inner, activation="relu", use_out_project=True))
    with torch.no_grad():
        for p in list(pred.parameters()) + list(join.parameters()):
            p.mul_(3.0)
    pred.to(dev).eval()
    join.to(dev).eval()
    spred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": D, "symbol_embedding_dim": E,
                                                        "context_size": 5}}).to(dev).eval()
    sjoin = Joiner(JoinerConfig(input_dim=D, output_dim=V, activation="relu", use_out_project=False)).to(dev).eval()
    row = {"tool": "ab_decode_host", "rounds": args.rounds, "V": V, "D": D, "E": E, "H": H, "layers": L, "frames": Tc * K}

    def stats(ms, digits):
        return {k: {"median": round(statistics.median(v), digits), "min": round(min(v), digits)} for k, v in ms.items()}

    def order(i):
        return versions if i % 2 == 0 else versions[::-1]

    with torch.no_grad():
        for B in (16, 1):
            am = (torch.randn(B, Tc * K, V, generator=torch.Generator().manual_seed(B)) * 3.0).to(dev)
            lens = torch.full((B,), Tc * K, dtype=torch.int64, device=dev)
            for mts in (1, 5):
                ms = {"tree": [], "other": []}
                for i in range(args.rounds + 3):           # three rounds of warm-up
                    for name, mod in order(i):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got = mod.rnnt_greedy_lstm_tokens_from_am(am, lens, pred, join, mts)
                        torch.cuda.synchronize()
                        if i >= 3:
                            ms[name].append((time.perf_counter() - t0) * 1e3)
                        ms.setdefault("out_" + name, got)
                same = all(torch.equal(x, y) for x, y in zip(ms.pop("out_tree"), ms.pop("out_other")))
                row[f"whole_greedy_lstm_B{B}_mts{mts}"] = dict(stats(ms, 3), unit="ms per call", equal=same)
        searches = (
            ("lstm_beam", lambda m: m.RnntLstmStreamingSearch(pred, join, 1, "beam", max_tokens=256, device=dev)),
            ("stateless_greedy", lambda m: m.RnntStreamingSearch(spred, sjoin, 1, "greedy", max_tokens=256, device=dev)),
            ("stateless_beam", lambda m: m.RnntStreamingSearch(spred, sjoin, 1, "beam", max_tokens=256, device=dev)),
            ("ctc_beam", lambda m: m.CtcStreamingSearch(V, 1, max_tokens=256, device=dev)))
        chunk = (torch.randn(1, Tc, V, generator=torch.Generator().manual_seed(3)) * 3.0).to(dev)
        for key, build in searches:
            built = {name: build(mod) for name, mod in versions}
            us = {"tree": [], "other": []}
            for i in range(args.rounds):
                for name, _ in order(i):
                    s = built[name]
                    s.reset()
                    s.step(chunk)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(8):
                        s.step(chunk)
                    us[name].append((time.perf_counter() - t0) / 8 * 1e6)
                    torch.cuda.synchronize()
            row[f"step_enqueue_{key}_B1"] = dict(stats(us, 1), unit="us of host time per step")
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
