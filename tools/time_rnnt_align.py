"""Time RNN-T forced alignment (csrc/rnnt_align.hip s2t_rnnt_align) next to the mutual-information recursion
on the same operands and the aligner's host loop.

    python tools/time_rnnt_align.py [--reps 200] [--loop-reps 3] [--lib PATH] [--label NAME] [--out FILE]

Two batches: 16 x 250 frames and the C3 lattice's 32 x 248, both with 40 labels per utterance at full
lengths; px / py are the full lattice of the fused joiner (kernels.rnnt_full_lattice, 128 classes, am and lm
2 x normal), on the regular and on the modified lattice.  Per batch and type, on the process's own stream,
after a warm-up of every call:
  device_entry   kernels.rnnt_align into held outputs (the workspace allocation included, as a caller pays
                 it): device events around `--reps` back-to-back calls, divided; 5 such windows, the median
                 with min .. max behind
  mi_yardstick   s2t_mutual_info_fwd on the same px / py into held buffers, timed the same way: the same
                 lattice walked once with a log-add per cell and p written out
  module_loop    RnntForcedAligner._module_loop over the batch's utterances on the same device tensors: a
                 host clock around the loop, ending in a device synchronise, median of `--loop-reps` (0
                 leaves the loop out, for a kernel trace of the entry alone)
and whether the device entry's frames equal the host loop's.  `form` is what s2t_rnnt_align_form answers
for the shape in the library timed.  `--lib PATH` times another build of the library, e.g. one whose
S2T_RNNT_ALIGN_LDS_BYTES is small enough that these shapes take the workspace form (kept out of the tree):
two processes of this tool on the same device give both backpointer forms at one shape.  Nothing is gated.
One JSON line per batch and type, appended to `--out` (default profiles/rnnt_align.jsonl).
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_align.jsonl"))
    args = ap.parse_args()
    from speech2text_amd import _native as N
    if args.lib:
        N.LIB_PATH = os.path.abspath(args.lib)
    from speech2text_amd import kernels
    from speech2text_amd.model.alignment import RnntForcedAligner
    if not torch.cuda.is_available():
        raise SystemExit("time_rnnt_align.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    C, S = 128, 40
    lib = N.lib()
    for B, T in ((16, 250), (32, 248)):
        for rnnt_type in ("regular", "modified"):
            ty = kernels.RNNT_TYPES[rnnt_type]
            g = torch.Generator().manual_seed(B)
            am, lm = (2.0 * torch.randn(B, T, C, generator=g)).to(dev), (2.0 * torch.randn(B, S + 1, C, generator=g)).to(dev)
            symbols = torch.randint(1, C, (B, S), generator=g).to(dev)
            boundary = kernels.make_boundary(torch.full((B,), S), torch.full((B,), T), dev)
            px, py = kernels.rnnt_full_lattice(am, lm, symbols, boundary, 0, "relu", rnnt_type)
            out = kernels.rnnt_align(px, py, boundary, rnnt_type)
            p = torch.empty((B, S + 1, T + 1), dtype=torch.float32, device=dev)
            ans = torch.empty((B,), dtype=torch.float32, device=dev)

            def entry():
                kernels.rnnt_align(px, py, boundary, rnnt_type, out=out)

            def recursion():
                N.check(lib.s2t_mutual_info_fwd(N.fp(px), N.fp(py), N.lp(boundary), B, S, T, ty, N.fp(p), N.fp(ans),
                                                N.stream()), "s2t_mutual_info_fwd")

            def loop():
                return [RnntForcedAligner._module_loop(px[b], py[b], S, T, rnnt_type) for b in range(B)]

            for fn in (entry, recursion):
                _window_us(fn, 20)                         # warm-up
            t_entry, t_mi = [], []
            for _ in range(5):                             # alternating windows
                t_entry.append(_window_us(entry, args.reps))
                t_mi.append(_window_us(recursion, args.reps))
            rows = loop() if args.loop_reps else None      # warm-up of the loop's torch kernels
            t_loop = []
            for _ in range(args.loop_reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rows = loop()
                torch.cuda.synchronize()
                t_loop.append(1e6 * (time.perf_counter() - t0))
            same = rows and all(bool(r.ok) and torch.equal(r.tok_frame, out.tok_frame[b]) for b, r in enumerate(rows))
            row = {"label": args.label, "rnnt_type": rnnt_type, "B": B, "T": T, "S": S,
                   "form": int(lib.s2t_rnnt_align_form(S, T, ty)), "reps_per_window": args.reps,
                   "device_entry": _stats(t_entry), "mi_yardstick": _stats(t_mi),
                   "module_loop": _stats(t_loop) if t_loop else None, "frames_equal_module_loop": same,
                   "all_feasible": bool(out.ok.all()), "score_at_most_ans": bool((out.score <= ans + 1e-3 * ans.abs()).all())}
            row["entry_over_mi"] = round(row["device_entry"]["median_us"] / row["mi_yardstick"]["median_us"], 2)
            line = json.dumps(row)
            print(line, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
