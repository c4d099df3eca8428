"""Time the six one-launch RNN-T search entries of the stateless predictor (csrc/decode_rnnt.hip:
s2t_rnnt_greedy_stateless, s2t_rnnt_beam_stateless, s2t_rnnt_beam_stateless_ngram and their _chunk partners)
of this build against the parent commit's, and compare what they compute byte for byte.

    python tools/time_rnnt_stateless.py --parent-lib PATH [--runs 20] [--label NAME] [--out FILE]

The comparison is tools/vs_parent.py's: this build, the parent's library and the parent's again from a byte
copy, through plain ctypes handles, alternating call by call with the libraries' order rotating; a figure's
`speed_limit_ms` is the larger parent median plus the two parents' difference, `speed_missed` the figures of
this build above it.

Inputs: tools/bench_rnnt_ngram.py's (16 x 250 frames, V 128, E 512, D 256, ctx 5, the blank's lift bisected
so that the plain beam search emits about 40 tokens an utterance, beam 4 / top-k 4, the order-3 n-gram of
bench_ctc_ngram's seeded token text at lm_weight 0.3, 16-frame chunks) and the greedy pair at max_token_step
1 and 5 (tools/bench_rnnt_decoders.py, tools/bench_stream_search.py).  The whole-utterance entries of the
three libraries work on the same workspace and outputs; every stream has a state of its own and is reset
every 32 calls.

`bits_equal`: both builds' six entries on the five configurations of tests/golden/rnnt_beam_ref*.npz and on
every case of tests/rnnt_ngram_cases.CASES, whole and fed in 7-frame chunks, every output compared byte for
byte and, after every chunk, the caller-owned state buffer, which both builds got filled with one byte
pattern before their reset.

One JSON line, appended to `--out` (default profiles/rnnt_stateless.jsonl).  Nothing is gated.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from vs_parent import LIBS, alternate, same, speed_rule, three_libraries  # noqa: E402

BEAM, TOPK, CHUNK, MAX_TOKENS = 4, 4, 16, 1024
KEYS = ("emb", "conv_w", "lin_w", "lin_b", "pre_w", "pre_b")


class _Predictor:
    """The six weight tensors on the device and the dimensions every entry takes behind them."""

    def __init__(self, w, act, dev):
        self.w = [t.to(dev).float().contiguous() for t in w]
        self.V, self.D = self.w[4].shape
        self.E, self.ctx = self.w[1].shape
        self.act = act


class _Raw:
    """The stateless RNN-T entries of the library at `path` through a ctypes handle of its own."""

    def __init__(self, path, N):
        self.N, lib = N, ctypes.CDLL(path)
        for name, proto in N.parse_header().items():
            if name.startswith("s2t_rnnt_") and hasattr(lib, name):   # (the parent's library lacks newer entries)
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = proto
                setattr(self, name[4:], fn)

    def _head(self, p, am, lens):
        N = self.N
        return (N.fp(am), N.lp(lens), *[N.fp(t) for t in p.w], am.shape[0], am.shape[1], p.V, p.E, p.D, p.ctx, p.act)

    def _outputs(self, B, width, dev):
        return dict(tokens=torch.zeros((B, width), dtype=torch.int64, device=dev),
                    frames=torch.zeros((B, width), dtype=torch.int64, device=dev),
                    out_len=torch.zeros((B,), dtype=torch.int64, device=dev), score=torch.zeros((B,), device=dev),
                    lm_score=torch.zeros((B,), device=dev), stable=torch.zeros((B,), dtype=torch.int64, device=dev),
                    ovf=torch.zeros((B,), dtype=torch.int32, device=dev))

    def greedy(self, p, am, lens, mts, o=None):
        """-> (call, outputs) of s2t_rnnt_greedy_stateless; o: another library's outputs (a timing)."""
        N, (B, T, _) = self.N, am.shape
        max_out = T * (mts + 1)
        o = o or self._outputs(B, max_out, am.device)
        args = self._head(p, am, lens) + (mts, max_out, 0, N.lp(o["tokens"]), N.lp(o["out_len"]))
        return (lambda: N.check(self.rnnt_greedy_stateless(*args, N.stream()), "s2t_rnnt_greedy_stateless")), o

    def beam(self, p, am, lens, beam, topk, lm=None, weight=0.0, buffers=None):
        """-> (call, outputs, buffers) of s2t_rnnt_beam_stateless, or of _ngram with lm = (desc, start_ctx);
        buffers: another library's, so that both work on the same workspace and outputs (a timing)."""
        N, (B, T, V) = self.N, am.shape
        if buffers is None:
            size = self.rnnt_beam_workspace_bytes if lm is None else self.rnnt_beam_ngram_workspace_bytes
            buffers = (self._outputs(B, T, am.device),
                       torch.empty((size(B, T, V, beam),), dtype=torch.uint8, device=am.device))
        o, ws = buffers
        outs = (N.ptr(ws), N.lp(o["tokens"]), N.lp(o["frames"]), N.lp(o["out_len"]), N.fp(o["score"]))
        if lm is None:
            fn, name, args = self.rnnt_beam_stateless, "s2t_rnnt_beam_stateless", self._head(p, am, lens) + (0, beam, topk) + outs
        else:
            fn, name = self.rnnt_beam_stateless_ngram, "s2t_rnnt_beam_stateless_ngram"
            args = (lm[0],) + self._head(p, am, lens) + (0, beam, topk, weight, lm[1]) + outs + (N.fp(o["lm_score"]),)
        return (lambda: N.check(fn(*args, N.stream()), name)), o, buffers

    def stream(self, p, B, dev, max_tokens, beam=0, topk=0, mts=0, lm=None, weight=0.0):
        """-> (reset, chunk(chunk, chunk_len), outputs, state) of the chunk entries: greedy at beam 0, the beam
        search, or its n-gram form with lm = (desc, start_ctx).  The state starts as one byte pattern, so that
        what no kernel writes, the padding behind every array, is the same in two libraries' buffers."""
        N = self.N
        o = self._outputs(B, max_tokens, dev)
        size = self.rnnt_stream_state_bytes if lm is None else self.rnnt_ngram_stream_state_bytes
        state = torch.full((size(B, p.V, p.ctx, beam, max_tokens),), 0xA5, dtype=torch.uint8, device=dev)
        shape = (N.ptr(state), None, B, p.V, p.ctx, beam, max_tokens, 0)
        tail = (N.lp(o["stable"]), N.ip(o["ovf"]))
        beam_outs = (N.lp(o["tokens"]), N.lp(o["frames"]), N.lp(o["out_len"]), N.fp(o["score"]))

        def reset():
            if lm is None:
                N.check(self.rnnt_stream_reset(*shape, N.stream()), "s2t_rnnt_stream_reset")
            else:
                N.check(self.rnnt_ngram_stream_reset(*shape, lm[1], N.stream()), "s2t_rnnt_ngram_stream_reset")

        def chunk(ch, cl):
            head = self._head(p, ch, cl)
            if beam == 0:
                rc = self.rnnt_greedy_stateless_chunk(*head, mts, max_tokens, 0, N.ptr(state), N.lp(o["tokens"]),
                                                      N.lp(o["out_len"]), N.ip(o["ovf"]), N.stream())
            elif lm is None:
                rc = self.rnnt_beam_stateless_chunk(*head, 0, beam, topk, max_tokens, N.ptr(state), *beam_outs, *tail,
                                                    N.stream())
            else:
                rc = self.rnnt_beam_stateless_ngram_chunk(lm[0], *head, 0, beam, topk, weight, max_tokens,
                                                          N.ptr(state), *beam_outs, N.fp(o["lm_score"]), *tail,
                                                          N.stream())
            N.check(rc, "a stateless RNN-T chunk entry")
        return reset, chunk, o, state


def _cases(dev):
    """The five golden configurations and every n-gram case as (name, predictor, am, lengths, beam, top-k,
    n-gram, lm_weight); a golden configuration's n-gram is estimated on tests/ctc_ngram_cases.py's seeded
    token text at its V."""
    import ctc_ngram_cases as NC
    import rnnt_beam_restatement as R
    import rnnt_ngram_cases as C
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    out = []
    for i, c in enumerate(R.load_fixture(os.path.join(ROOT, "tests", "golden"))):
        p = _Predictor([torch.from_numpy(c[k]) for k in KEYS], 0 if c["act"] == "relu" else 1, dev)
        lm = NgramLm.estimate(NC.lm_sequences(c["V"], 120, 1), c["V"], order=2)
        out.append((f"golden{i}", p, torch.from_numpy(c["am"]).float(), torch.from_numpy(c["lengths"]).long(),
                    c["beam"], c["topk"], lm, 0.5))
    for n, c in C.CASES.items():
        w, am, lens = C.make(n)
        p = _Predictor([w[k] for k in KEYS], 0 if c["act"] == "relu" else 1, dev)
        out.append((n, p, am, lens, c["beam"], c["topk"], NgramLm.from_arpa(C.text_of(n), num_classes=c["V"]),
                    c["weight"]))
    return [(n, p, am.to(dev).contiguous(), lens.to(dev), beam, topk, lm.to(dev), w)
            for n, p, am, lens, beam, topk, lm, w in out]


def _bits_equal(tree, parent, dev):
    """Both libraries' six entries on every case, whole and in 7-frame chunks, the chunk entries' state buffers
    compared byte for byte after every chunk -> (cases, equal, [what differed])."""
    cases, differ = _cases(dev), []
    for i, (name, p, am, lens, beam, topk, lm, weight) in enumerate(cases):
        B, T, _ = am.shape
        desc, keep = lm.desc()
        ngram, mts = (desc, int(lm.start_ctx)), (1, 5)[i % 2]
        # (call, outputs, ...): the workspaces stay referenced here while their calls run
        whole = {"greedy": [lib.greedy(p, am, lens, mts) for lib in (tree, parent)],
                 "beam": [lib.beam(p, am, lens, beam, topk) for lib in (tree, parent)],
                 "beam_ngram": [lib.beam(p, am, lens, beam, topk, ngram, weight) for lib in (tree, parent)]}
        for what, (a, b) in whole.items():
            a[0](), b[0]()
            torch.cuda.synchronize()
            if not same(a[1].values(), b[1].values()):
                differ.append(f"{name}:{what}:" + ",".join(k for k in a[1] if not same([a[1][k]], [b[1][k]])))
        kinds = {"greedy_chunk": dict(mts=mts), "beam_chunk": dict(beam=beam, topk=topk),
                 "beam_ngram_chunk": dict(beam=beam, topk=topk, lm=ngram, weight=weight)}
        for what, kw in kinds.items():
            streams = [lib.stream(p, B, dev, T * (mts + 1), **kw) for lib in (tree, parent)]
            for reset, _, _, _ in streams:
                reset()
            for t0 in range(0, T, 7):
                ch = am[:, t0:t0 + 7].contiguous()
                cl = (lens.clamp(max=T) - t0).clamp(0, ch.shape[1])
                for _, chunk, _, _ in streams:
                    chunk(ch, cl)
                torch.cuda.synchronize()
                (_, _, oa, sa), (_, _, ob, sb) = streams
                if not same([sa, *oa.values()], [sb, *ob.values()]):
                    differ.append(f"{name}:{what}@{t0}:" + ",".join(
                        k for k in oa if not same([oa[k]], [ob[k]])) + ("" if same([sa], [sb]) else ",state"))
                    break
        del keep
    return len(cases), not differ, differ


def bench_inputs(dev):
    """tools/bench_rnnt_ngram.py's inputs -> (predictor, joiner, their _Predictor, am (16, 250, 128) with the blank's
    lift bisected so that the plain beam search emits about 40 tokens an utterance, lengths, the order-3 NgramLm)."""
    from bench_ctc_ngram import token_text
    from speech2text_amd.model.decoding import _stateless_weights, rnnt_beam_tokens_from_am
    from speech2text_amd.model.joiner.joiner import Joiner, JoinerConfig
    from speech2text_amd.model.lm.ngram_lm import NgramLm
    from speech2text_amd.model.predictor.predictor import Predictor
    V, B, T = 128, 16, 250
    torch.manual_seed(0)
    pred = Predictor({"model": "Stateless", "config": {"num_symbols": V, "output_dim": 256, "symbol_embedding_dim": 512,
                                                       "context_size": 5}})
    join = Joiner(JoinerConfig(input_dim=256, output_dim=V, activation="relu", prune_range=5, use_out_project=False))
    join._enc_proj = torch.nn.Identity()
    pred, join = (m.to(dev).eval().requires_grad_(False) for m in (pred, join))
    with torch.no_grad():
        for q in list(pred.parameters()) + list(join.parameters()):
            q.mul_(3.0)
    ngram = NgramLm.estimate(token_text(V, 20000, 2), V, order=3).to(dev)
    am0 = 3.0 * torch.randn(B, T, V, generator=torch.Generator().manual_seed(1)).to(dev)
    lens = torch.full((B,), T, dtype=torch.int64, device=dev)
    lo, hi = 0.0, 64.0
    for _ in range(12):
        mid = 0.5 * (lo + hi)
        am = am0.clone()
        am[:, :, 0] += mid
        n = float(rnnt_beam_tokens_from_am(am, lens, pred, join, BEAM, TOPK)[2].float().mean())
        lo, hi = (mid, hi) if n > 40 else (lo, mid)
    w, _, _, _, act = _stateless_weights(pred, join)
    return pred, join, _Predictor(w, act, dev), am, lens, ngram


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--parent-lib", required=True, help="another build of libs2t_mi355.so: the parent commit's")
    ap.add_argument("--label", default=None, help="kept in the JSON line")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rnnt_stateless.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rnnt_stateless.py measures on the GPU; there is none here")
    from speech2text_amd import _native as N
    dev = torch.device("cuda:0")
    V, B, T, lm_w = 128, 16, 250, 0.3
    _, _, p, am, lens, ngram = bench_inputs(dev)
    desc, keep = ngram.desc()
    lm = (desc, int(ngram.start_ctx))

    libs = three_libraries(N.LIB_PATH, args.parent_lib, lambda path: _Raw(path, N))
    pieces = [am[:, t0:t0 + CHUNK].contiguous() for t0 in range(0, T - CHUNK + 1, CHUNK)]
    full = torch.full((B,), CHUNK, dtype=torch.int64, device=dev)
    whole = {"greedy_mts1": lambda lib, sh: lib.greedy(p, am, lens, 1, sh and sh[0]) + (None,),
             "greedy_mts5": lambda lib, sh: lib.greedy(p, am, lens, 5, sh and sh[0]) + (None,),
             "beam": lambda lib, sh: lib.beam(p, am, lens, BEAM, TOPK, buffers=sh and sh[1]),
             "beam_ngram": lambda lib, sh: lib.beam(p, am, lens, BEAM, TOPK, lm, lm_w, buffers=sh and sh[1])}
    chunked = {"greedy_mts1_chunk": dict(mts=1), "greedy_mts5_chunk": dict(mts=5),
               "beam_chunk": dict(beam=BEAM, topk=TOPK), "beam_ngram_chunk": dict(beam=BEAM, topk=TOPK, lm=lm, weight=lm_w)}
    calls, hold, tokens = {}, [], {}
    for fig, make in whole.items():
        shared = None
        for who in LIBS:
            calls[f"{fig}_{who}"], o, buffers = make(libs[who], shared)
            shared = shared or (o, buffers)
        hold.append(shared)
        calls[f"{fig}_tree"]()
        tokens[fig] = round(float(shared[0]["out_len"].float().mean()), 1)
    for fig, kw in chunked.items():
        for who in LIBS:
            reset, chunk, so, state = libs[who].stream(p, B, dev, MAX_TOKENS, **kw)
            hold.append((so, state))
            n = [0]

            def step(reset=reset, chunk=chunk, n=n):
                if n[0] % 32 == 0:
                    reset()
                chunk(pieces[n[0] % len(pieces)], full)
                n[0] += 1
            calls[f"{fig}_{who}"] = step
    row = {"tool": "time_rnnt_stateless", "B": B, "T": T, "V": V, "E": p.E, "D": p.D, "ctx": p.ctx, "beam": BEAM,
           "top_k": TOPK, "lm_weight": lm_w, "ngram_contexts": ngram.num_ctx, "ngram_arcs": ngram.num_arcs,
           "chunk_frames": CHUNK, "tokens_per_utt": tokens, "gpu": torch.cuda.get_device_name(0)}
    row["vs_parent"] = alternate(calls, 4 * args.runs, group=len(LIBS))
    speed_rule(row, list(whole) + list(chunked))
    row["bits_equal_cases"], row["bits_equal"], row["bits_differ"] = _bits_equal(libs["tree"], libs["parent"], dev)
    del keep
    if args.label:
        row["label"] = args.label
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
