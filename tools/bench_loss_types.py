"""Time the C3 train step (bench.py's zipformer pruned-RNN-T task and synthetic batch) under each
setting of the pruned loss: rnnt_type regular / modified / constrained, delay_penalty 0 / 0.05.

    python tools/bench_loss_types.py [--steps 20] [--warmup 5] [--out FILE] [setting ...]
    python tools/bench_loss_types.py --recursion [--reps 200] [--out FILE]

A setting is TYPE or TYPE:PENALTY (default: regular modified constrained modified:0.05).  The task is
bench.py's c3_config with `loss: config:` overridden, nothing else; bench.py itself is not touched.
Per setting: the step time over `steps` steps after the warm-up (wall clock around a synchronised
loop, as bench.py), then one profiled step whose per-entry-point times of the loss's own launches
(the two recursions, the px / py builders and their backwards) are reported next to it.  The
settings run one after the other in one process, `regular` first and again last, so that a drift of
the box shows.  One JSON line per setting (appended to --out).

A freshly initialised model's prune ranges need not hold a one-symbol-per-frame path for every
utterance; such an utterance costs +inf under the two new types and the reported loss is then inf.
The launches and their sizes are the same either way.

--recursion times the two recursions alone at the C3 lattice (B 64, S 50, T 248, ragged lengths as
tests/loss_cases.bench_case): kernels.mutual_information forward + backward on random operands, px
(B,S,T+1) for the diagonal walk and (B,S,T) for the column walk, medians of device-event times.  Run
it under a kernel trace for the per-kernel split.
"""
import argparse
import copy
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

LOSS_ENTRIES = ("s2t_mutual_info_fwd", "s2t_mutual_info_bwd", "s2t_rnnt_pruned_fwd",
                "s2t_rnnt_pruned_bwd")


def run(setting, args, device):
    from speech2text_amd import _native
    from speech2text_amd.build_task import TaskFactory
    from speech2text_amd.trainer import Trainer
    ty, _, pen = setting.partition(":")
    cfg = copy.deepcopy(bench.c3_config(500))
    cfg["loss"]["config"].update({"rnnt_type": ty, "delay_penalty": float(pen or 0.0)})
    random.seed(1234); np.random.seed(1234); torch.manual_seed(1234)
    task = TaskFactory.get(cfg["task"]["type"])(cfg)
    trainer = Trainer(**cfg["trainer"]).setup(task, device)
    task.train()
    torch.manual_seed(1234)
    batch = bench.make_batch(0, 64, 10.0, 50, 500, device)
    torch.manual_seed(1234)
    for i in range(args.warmup):
        loss = trainer.training_step(batch, i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = trainer.training_step(batch, args.warmup + i)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    _native.profile_begin("*")
    trainer.training_step(batch, args.warmup + args.steps + 1)
    torch.cuda.synchronize()
    prof = _native.profile_end()
    entries = {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 4)}
               for k, v in prof.items() if k in LOSS_ENTRIES}
    return {"setting": setting, "step_ms": round(ms, 3), "steps": args.steps, "loss": float(loss),
            "loss_entries": entries}


def recursion(args, device):
    import statistics
    from speech2text_amd import kernels as K
    B, S, T = 64, 50, 248
    g = torch.Generator().manual_seed(2024)
    tl = torch.randint(5, S + 1, (B,), generator=g); tl[0] = S
    el = torch.randint(S + 1, T + 1, (B,), generator=g); el[0] = T
    bnd = K.make_boundary(tl, el, device)
    py = (torch.randn(B, S + 1, T, generator=g) - 2.0).to(device)
    out = {"setting": "recursion", "B": B, "S": S, "T": T, "reps": args.reps}
    for name, cols in (("diagonal_walk", T + 1), ("column_walk", T)):
        px = (torch.randn(B, S, cols, generator=g) - 2.0).to(device)
        if cols == T + 1:
            px[:, :, T] = float("-inf")
        for _ in range(10):
            K.mutual_information(px, py, bnd)
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            K.mutual_information(px, py, bnd)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        q = statistics.quantiles(ms, n=10)
        out[name] = {"fwd_bwd_median_us": round(1e3 * statistics.median(ms), 2),
                     "p10_us": round(1e3 * q[0], 2), "p90_us": round(1e3 * q[-1], 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recursion", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("setting", nargs="*")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to time")
    device = torch.device("cuda", 0)
    if args.recursion:
        line = json.dumps(recursion(args, device))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")
        return
    settings = args.setting or ["regular", "modified", "constrained", "modified:0.05", "regular"]
    for s in settings:
        line = json.dumps(run(s, args, device))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
