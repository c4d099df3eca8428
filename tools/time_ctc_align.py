"""Time CTC forced alignment (csrc/ctc_align.hip s2t_ctc_align) next to the aligner's host loop and the CTC
loss kernel on the same batch.

    python tools/time_ctc_align.py [--reps 200] [--loop-reps 3] [--lib PATH] [--label NAME] [--out FILE]

Two batches: 16 x 250 frames and the C2 shape 32 x 248, both V 128 and 40 labels per utterance, logits =
2 x normal, full lengths.  Per batch, on the process's own stream, after a warm-up of every call:
  device_entry   kernels.ctc_align into held outputs (the workspace allocation included, as a caller pays
                 it): device events around `--reps` back-to-back calls, divided; 5 such windows, the median
                 with min .. max behind
  loss_yardstick s2t_ctc_loss_fwd_bwd without a gradient on the same batch, timed the same way: the same
                 lattice walked twice with logf / expf
  module_loop    CtcForcedAligner._module_loop over the batch's utterances on the same device tensors:
                 a host clock around the loop, ending in a device synchronise, median of `--loop-reps`
                 (0 leaves the loop out, for a kernel trace of the entry alone)
and whether the device entry's paths equal the host loop's.  `form` is what s2t_ctc_align_form answers for
the shape in the library timed.  `--lib PATH` times another build of the library, e.g. one whose
S2T_CTC_ALIGN_LDS_BYTES is small enough that these shapes take the workspace form (kept out of the tree):
two processes of this tool on the same device give both backpointer forms at one shape.  Nothing is gated.
One JSON line per batch, appended to `--out` (default profiles/ctc_align.jsonl).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return 1000.0 * e0.elapsed_time(e1) / reps


def _stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "windows": len(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--lib", default=None, help="another build of libs2t_mi355.so to time")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_align.jsonl"))
    args = ap.parse_args()
    from speech2text_amd import _native as N
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    from speech2text_amd import kernels
    from speech2text_amd.model.alignment import CtcForcedAligner
    if not torch.cuda.is_available():
        raise SystemExit("time_ctc_align.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    V, U = 128, 40
    lib = N.lib()
    for B, T in ((16, 250), (32, 248)):
        g = torch.Generator().manual_seed(B)
        x = (2.0 * torch.randn(B, T, V, generator=g)).to(dev)
        targets = torch.randint(1, V, (B, U), generator=g).to(dev)
        lens = torch.full((B,), T, dtype=torch.int64, device=dev)
        tl = torch.full((B,), U, dtype=torch.int64, device=dev)
        out = kernels.ctc_align(x, lens, targets, tl)
        ws = torch.empty(lib.s2t_ctc_workspace_floats(B, T, U), dtype=torch.float32, device=dev)
        per = torch.empty(B, dtype=torch.float32, device=dev)

        def entry():
            kernels.ctc_align(x, lens, targets, tl, out=out)

        def loss():
            N.check(lib.s2t_ctc_loss_fwd_bwd(N.fp(x), N.lp(targets), U, N.lp(lens), N.lp(tl), B, T, V, U, 0, 1, None,
                                             N.fp(ws), N.fp(per), None, N.stream()), "s2t_ctc_loss_fwd_bwd")

        def loop():
            return [CtcForcedAligner._module_loop(x[b], targets[b].tolist(), 0) for b in range(B)]

        for fn in (entry, loss):
            _window_us(fn, 20)                             # warm-up
        t_entry, t_loss = [], []
        for _ in range(5):                                 # alternating windows
            t_entry.append(_window_us(entry, args.reps))
            t_loss.append(_window_us(loss, args.reps))
        rows = loop() if args.loop_reps else None          # warm-up of the loop's torch kernels
        t_loop = []
        for _ in range(args.loop_reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = loop()
            torch.cuda.synchronize()
            t_loop.append(1e6 * (time.perf_counter() - t0))
        same = rows and all(bool(r.ok) and torch.equal(r.path, out.path[b]) for b, r in enumerate(rows))
        row = {"label": args.label, "B": B, "T": T, "V": V, "U": U, "form": int(lib.s2t_ctc_align_form(T, U)),
               "reps_per_window": args.reps, "device_entry": _stats(t_entry), "loss_yardstick": _stats(t_loss),
               "module_loop": _stats(t_loop) if t_loop else None, "paths_equal_module_loop": same,
               "all_feasible": bool(out.ok.all())}
        row["entry_over_loss"] = round(row["device_entry"]["median_us"] / row["loss_yardstick"]["median_us"], 2)
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
