"""This build's entries against the parent commit's, in one process: what tools/time_ctc_bias.py and
tools/time_rnnt_stateless.py share.

Three libraries are loaded through plain ctypes handles of their own: this build's, the parent's (another
build of libs2t_mi355.so, `--parent-lib`) and the parent's a second time from a byte copy under another name.
Their calls alternate call by call on the same inputs, the three libraries' order within a figure rotating
run by run (no library is always the first after another figure's kernel).  Parent against parent is the
noise: a figure's limit is the larger parent median plus the two parents' difference, and the figures of this
build above their limit are `speed_missed`.  Outputs and caller-owned state are compared byte for byte.
"""
import os
import shutil
import statistics
import tempfile

import torch

LIBS = ("tree", "parent", "parent_again")


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "runs": len(ms)}


def alternate(calls, runs, warmup=3, group=1):
    """{name: fn} -> {name: stats}, the calls alternating call by call.  group: the calls are groups of that
    many in a row (one figure of several libraries), and run r walks every group from its member r % group
    on, so that each member follows each neighbour equally often."""
    names = list(calls)
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for r in range(runs):
        for g0 in range(0, len(names), group):
            for i in range(group):
                k = names[g0 + (r + i) % group]
                times[k].append(event_ms(calls[k])[0])
    return {k: stats(v) for k, v in times.items()}


def same(xs, ys):
    """Whether the tensors of xs are those of ys byte for byte."""
    return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(xs, ys))


def three_libraries(tree_lib, parent_lib, load):
    """{"tree", "parent", "parent_again"} -> load(path): this build, the parent's, and the parent's again from
    a byte copy under another name (a second mapping of the same code)."""
    with tempfile.TemporaryDirectory() as tmp:
        again = shutil.copy(os.path.abspath(parent_lib), os.path.join(tmp, "libs2t_parent_again.so"))
        return dict(zip(LIBS, (load(tree_lib), load(os.path.abspath(parent_lib)), load(again))))


def speed_rule(row, figures):
    """row["vs_parent"] holds alternate()'s stats of `<figure>_<library>` for every figure: adds
    tree_over_parent, speed_limit_ms (the larger parent median plus the two parents' difference) and
    speed_missed (the figures of this build above their limit) to the row."""
    pm = {k: v["median_ms"] for k, v in row["vs_parent"].items()}
    row["tree_over_parent"] = {k: round(pm[f"{k}_tree"] / pm[f"{k}_parent"], 4) for k in figures}
    row["speed_limit_ms"] = {k: round(max(pm[f"{k}_parent"], pm[f"{k}_parent_again"])
                                      + abs(pm[f"{k}_parent"] - pm[f"{k}_parent_again"]), 4) for k in figures}
    row["speed_missed"] = [k for k in figures if pm[f"{k}_tree"] > row["speed_limit_ms"][k]]
