"""Time the chunk-carried fbank (csrc/fbank_stream.hip s2t_fbank_chunk_f32) next to what it replaces.

    python tools/time_fbank_stream.py [--reps 200] [--parent-lib PATH] [--no-recognizer] [--out FILE]

16 rows.  After a warm-up of every call, device events around `--reps` back-to-back calls, divided; 5
such windows per entry, alternating between the entries; the median with min .. max behind.  A fbank call
of this size is shorter than the host takes to issue it, so every fbank entry is timed twice: `call`, as
a caller pays it from Python, and `device`, 50 calls captured into one hipGraph and the replay divided
by 50 (the chunk entry is capturable by its statement), which leaves the host out:
  chunk_call        one fbank_chunk call of 5 120 new samples per row on a StreamingFbank's fixed buffers
                    (32 frames: one 2*chunk window at chunk 16; both launches, the frame kernel and the
                    state update)
  one_shot_same     fbank_batch on 16 x 5 360 samples: the same 16 x 32 frames in the one-shot kernel
  one_shot_10s      fbank_batch on 16 x 160 000 samples: the one-shot kernel re-run on 10 s heard so far,
                    what a caller without the chunk entry does per cut (16 x 32 workgroups: two to a CU)
  one_shot_60s      the same after a minute of audio (16 x 188 workgroups)
  recognizer_replay one replay of a StreamingRecognizer's graph (the bench's C3 zipformer made causal at
                    chunk 16, left context 64, greedy search, batch 16): what follows the fbank per chunk
  one_shot_tree / one_shot_parent   s2t_fbank_f32 on 16 x 160 000 samples from this tree's library and,
                    with --parent-lib, from another build of it (the parent commit's), through plain
                    ctypes handles in this same process, windows alternating: the shared kernel body
                    must not cost the one-shot kernel anything (and whether the two wrote the same bits)
One JSON line, appended to `--out` (default profiles/fbank_stream.jsonl).  Nothing is gated.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

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


GRAPH_CALLS = 50


def _graphed(fn):
    """`fn` GRAPH_CALLS times in one captured graph -> its replay."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(GRAPH_CALLS):
            fn()
    return graph.replay


def _stats(us):
    return {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
            "windows": len(us)}


def _raw_one_shot(path, N, tab, pcm, lens, out, frames):
    """s2t_fbank_f32 of the library at `path` through a ctypes handle of its own."""
    lib = ctypes.CDLL(path)
    fn = lib.s2t_fbank_f32
    fn.restype, fn.argtypes = N.parse_header()["s2t_fbank_f32"]
    B, mf = out.shape[0], out.shape[1]

    def call():
        N.check(fn(N.fp(pcm), pcm.stride(0), N.lp(lens), B, N.fp(tab.window), N.fp(tab.twiddle), N.ip(tab.mel_off),
                   N.ip(tab.mel_k0), N.fp(tab.mel_w), tab.nnz, tab.num_mel, 1.1920928955078125e-07, 1.0, None, None,
                   N.fp(out), mf, N.lp(frames), N.stream()), "s2t_fbank_f32")
    return call


def _recognizer(dev, B):
    import bench
    from speech2text_amd.build_task import TaskFactory
    cfg = bench.c3_config(500)
    cfg["encoder"]["config"].update({"chunk_size": [16], "left_context_frames": [64]})
    cfg["tokenizer"] = {"type": "char", "config": {"labels": [chr(0x4e00 + i) for i in range(500 - 3)]}}
    cfg["metric"] = {"decode_method": "rnnt_greedy_search", "max_token_step": 5}
    torch.manual_seed(0)
    task = TaskFactory.get("Pruned_Rnnt")(cfg).to(dev)
    task.eval()
    return task.streaming_recognizer(batch_size=B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--parent-lib", default=None, help="another build of libs2t_mi355.so: its one-shot fbank is timed")
    ap.add_argument("--no-recognizer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_stream.jsonl"))
    args = ap.parse_args()
    from speech2text_amd import _native as N
    from speech2text_amd import kernels as K
    from speech2text_amd.dataset.frontend.frontend import KaldiWaveFeature
    if not torch.cuda.is_available():
        raise SystemExit("time_fbank_stream.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    B, CH = 16, 5120
    g = torch.Generator().manual_seed(0)
    front = KaldiWaveFeature(num_mel_bins=80)
    tab = front.tables(dev)
    long_pcm = (0.1 * torch.randn(B, 160000, generator=g)).to(dev)
    long_len = torch.full((B,), 160000, dtype=torch.int64, device=dev)
    min_pcm = (0.1 * torch.randn(B, 960000, generator=g)).to(dev)
    min_len = torch.full((B,), 960000, dtype=torch.int64, device=dev)
    same_pcm, same_len = long_pcm[:, :5360].contiguous(), torch.full((B,), 5360, dtype=torch.int64, device=dev)
    sf = front.streaming(B, CH, device=dev)
    sf.pcm.copy_(long_pcm[:, :CH])
    sf.chunk_samples.fill_(CH)

    calls = {"chunk_call": sf.launch,
             "one_shot_same": lambda: K.fbank_batch(same_pcm, same_len, tab),
             "one_shot_10s": lambda: K.fbank_batch(long_pcm, long_len, tab),
             "one_shot_60s": lambda: K.fbank_batch(min_pcm, min_len, tab)}
    out10 = torch.empty((B, 998, 80), dtype=torch.float32, device=dev)
    fr10 = torch.empty((B,), dtype=torch.int64, device=dev)
    calls["one_shot_tree"] = _raw_one_shot(N.LIB_PATH, N, tab, long_pcm, long_len, out10, fr10)
    if args.parent_lib:
        parent_out = torch.empty_like(out10)
        calls["one_shot_parent"] = _raw_one_shot(os.path.abspath(args.parent_lib), N, tab, long_pcm, long_len,
                                                 parent_out, fr10.clone())
    graphs = {k: _graphed(fn) for k, fn in calls.items()}
    if not args.no_recognizer:
        rec = _recognizer(dev, B)
        calls["recognizer_replay"] = rec.graph.replay
    for fn in list(calls.values()) + list(graphs.values()):
        _window_us(fn, 20)                                 # warm-up
    times = {k: [] for k in calls}
    dtimes = {k: [] for k in graphs}
    for _ in range(5):                                     # alternating windows
        for k, fn in calls.items():
            times[k].append(_window_us(fn, args.reps))
        for k, fn in graphs.items():
            dtimes[k].append(_window_us(fn, max(args.reps // 10, 1)) / GRAPH_CALLS)
    row = {"B": B, "chunk_samples": CH, "frames_per_chunk": 32, "reps_per_window": args.reps,
           "gpu": torch.cuda.get_device_name(0)}
    row["call"] = {k: _stats(v) for k, v in times.items()}
    row["device"] = {k: _stats(v) for k, v in dtimes.items()}
    med = {k: v["median_us"] for k, v in row["device"].items()}
    row["device_chunk_over_one_shot_same"] = round(med["chunk_call"] / med["one_shot_same"], 2)
    row["device_one_shot_10s_over_chunk"] = round(med["one_shot_10s"] / med["chunk_call"], 2)
    row["device_one_shot_60s_over_chunk"] = round(med["one_shot_60s"] / med["chunk_call"], 2)
    if "recognizer_replay" in row["call"]:
        replay = row["call"]["recognizer_replay"]["median_us"]
        row["fbank_share_of_chunk"] = round(med["chunk_call"] / (med["chunk_call"] + replay), 4)
    if "one_shot_parent" in med:
        row["device_one_shot_tree_over_parent"] = round(med["one_shot_tree"] / med["one_shot_parent"], 4)
        torch.cuda.synchronize()                           # and the bits: both wrote the same input's features
        row["one_shot_bits_equal_parent"] = bool(torch.equal(out10, parent_out))
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
