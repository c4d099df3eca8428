"""Seeded cases shared by tests/test_rnnt_align_f64.py (CPU) and tests/test_gpu_rnnt_align.py (GPU): RNN-T
forced alignment, csrc/rnnt_align.hip.

Test infrastructure (not a test file).  A case is the operand pair of the mutual-information recursion --
px (B,S,T+1) on the regular lattice, (B,S,T) on the two others, py (B,S+1,T) -- and a boundary (B,4).
Values are scale x normal - 1 (multiples of 0.25 where `quant`); on the regular lattice column Tb of px is
-inf, as both lattice builders leave it.  Every cell outside s <= Sb, t <= Tb is NaN: a kernel that read
one could not return the restatement's bits.  The shapes are the smallest that reach each branch:

  S    0, 1; 63 / 64, 127 / 128, 255 / 256, 511 / 512 (S + 1 rows = one thread each: either side of every
       count of waves that changes the launch) and 1023, the recursion's limit;
  T    1 (regular: every token at frame 0; modified with S >= 2: no path);
  rows kinds cycled over the batch (ROW KINDS below): full, random, no symbols, no frames and no symbols,
       no frames but symbols, lengths above the shape and negative ones (both clamped), modified with
       Sb == Tb (a single path) and Sb == Tb + 1 (none); batches of 1, 17 and 33;
  type regular, modified, constrained;
  -inf cells inside the lattice that leave exactly one path (row 0) and none (row 1);
  ties three cases quantised to multiples of 0.25;
  form the backpointers in LDS and through the workspace (S2T_RNNT_ALIGN_LDS_BYTES decides): regular with
       S 5 between T 5114 and 5115 (5120 anti-diagonals fit), S 255 between T 1024 and 1025 (1280 fit),
       S 1023 at T 100 (320 fit: four blocks), S 2 at T 51200 (eleven blocks), S 128 at T 1600 (three waves:
       1706 fit, which is no whole number of the recursion's groups of 8 steps); modified with S 5 between T
       5120 and 5121.  FORMS records what s2t_rnnt_align_form must answer for every case.

The conditions, with no exclusions (tests/test_rnnt_align_f64.py asserts them; seeds and scales were
chosen on the CPU so that the restatement alone satisfies them): the float32 and the float64 run of the
restatement return the same ok and tok_frame on every utterance of every case; every TIES case has at
least one tied decision on its best paths.
"""
import functools
import math

import torch

import rnnt_align_f64 as A

KINDS = ("full", "rand", "s0", "t0s0", "t0", "above", "neg", "eq", "eq1")
NAN = float("nan")


def _c(seed, ty, B, S, T, rows=("full",), scale=2.0, quant=False, special=None):
    return dict(seed=seed, ty=ty, B=B, S=S, T=T, rows=rows, scale=scale, quant=quant, special=special)


RAGGED = ("full", "rand", "s0", "t0s0", "t0", "above", "neg", "eq", "eq1", "rand", "rand")
CASES = {
    "s0_t1_reg": _c(0, "regular", 1, 0, 1),
    "s0_b17_mod_ragged": _c(1, "modified", 17, 0, 5, rows=("full", "t0s0", "rand", "above", "neg")),
    "s1_t1_reg": _c(2, "regular", 3, 1, 1, rows=("full", "s0", "t0")),
    "s1_t1_mod": _c(3, "modified", 3, 1, 1, rows=("full", "s0", "t0")),
    "s3_t1_reg_all_at_frame0": _c(4, "regular", 2, 3, 1),
    "s2_t1_mod_infeasible": _c(5, "modified", 2, 2, 1),
    "s7_b17_reg_ragged": _c(6, "regular", 17, 7, 11, rows=RAGGED),
    "s7_b17_mod_ragged": _c(7, "modified", 17, 7, 11, rows=RAGGED),
    "s12_b33_con_ragged": _c(8, "constrained", 33, 12, 19, rows=RAGGED),
    "s12_b33_reg_ragged": _c(9, "regular", 33, 12, 9, rows=RAGGED),
    "s4_reg_inf_one_and_none": _c(10, "regular", 2, 4, 6, special="inf"),
    "s4_mod_inf_one_and_none": _c(11, "modified", 2, 4, 7, special="inf"),
    "s63_reg": _c(12, "regular", 2, 63, 7, rows=("full", "rand")),
    "s64_reg": _c(13, "regular", 2, 64, 7, rows=("full", "rand")),
    "s63_mod": _c(14, "modified", 2, 63, 66, rows=("full", "eq")),
    "s64_con": _c(15, "constrained", 2, 64, 67, rows=("full", "eq1")),
    "s127_reg": _c(16, "regular", 2, 127, 6, rows=("full", "rand")),
    "s128_mod": _c(17, "modified", 2, 128, 131, rows=("full", "rand")),
    "s255_reg": _c(18, "regular", 1, 255, 5),
    "s256_mod": _c(19, "modified", 2, 256, 258, rows=("full", "eq")),
    "s511_reg": _c(20, "regular", 1, 511, 4),
    "s512_reg": _c(21, "regular", 2, 512, 4, rows=("full", "rand")),
    "s512_mod_infeasible": _c(22, "modified", 1, 512, 6),
    "s1023_reg_t100_ws4": _c(23, "regular", 1, 1023, 100),
    "s5_reg_t5114_lds": _c(24, "regular", 1, 5, 5114),
    "s5_reg_t5115_ws": _c(24, "regular", 2, 5, 5115, rows=("full", "rand")),
    "s255_reg_t1024_lds": _c(25, "regular", 1, 255, 1024),
    "s255_reg_t1025_ws": _c(25, "regular", 1, 255, 1025),
    "s128_reg_t1600_ws": _c(28, "regular", 1, 128, 1600),
    "s5_mod_t5120_lds": _c(26, "modified", 1, 5, 5120),
    "s5_mod_t5121_ws": _c(26, "modified", 2, 5, 5121, rows=("full", "rand")),
    "s2_reg_t51200_ws11": _c(27, "regular", 1, 2, 51200),
    "ties_s4_reg": _c(35, "regular", 3, 4, 6, scale=1.0, quant=True),
    "ties_s6_b17_mod": _c(31, "modified", 17, 6, 9, rows=RAGGED, scale=1.0, quant=True),
    "ties_s64_reg": _c(32, "regular", 2, 64, 9, scale=1.0, quant=True),
}
TIES = [k for k, v in CASES.items() if v["quant"]]
_WS = 256                                                  # S2T_RNNT_ALIGN_FORM_WORKSPACE
FORMS = {                                                  # what s2t_rnnt_align_form(S, T, type) answers
    "s0_t1_reg": 1, "s0_b17_mod_ragged": 1, "s1_t1_reg": 1, "s1_t1_mod": 1, "s3_t1_reg_all_at_frame0": 1,
    "s2_t1_mod_infeasible": 1, "s7_b17_reg_ragged": 1, "s7_b17_mod_ragged": 1, "s12_b33_con_ragged": 1,
    "s12_b33_reg_ragged": 1, "s4_reg_inf_one_and_none": 1, "s4_mod_inf_one_and_none": 1, "s63_reg": 1, "s64_reg": 2,
    "s63_mod": 1, "s64_con": 2, "s127_reg": 2, "s128_mod": 3, "s255_reg": 4, "s256_mod": 5, "s511_reg": 8,
    "s512_reg": 9, "s512_mod_infeasible": 9, "s1023_reg_t100_ws4": 16 + _WS, "s5_reg_t5114_lds": 1,
    "s5_reg_t5115_ws": 1 + _WS, "s255_reg_t1024_lds": 4, "s255_reg_t1025_ws": 4 + _WS, "s128_reg_t1600_ws": 3 + _WS,
    "s5_mod_t5120_lds": 1,
    "s5_mod_t5121_ws": 1 + _WS, "s2_reg_t51200_ws11": 1 + _WS, "ties_s4_reg": 1, "ties_s6_b17_mod": 1,
    "ties_s64_reg": 2,
}


def clamp(n, hi):
    return max(0, min(int(n), hi))


def _one_path(px, py, Sb, Tb, reg, frames):
    """Leave exactly the path that emits symbol s at frames[s]: every other arc of the lattice is -inf."""
    kx, ky = torch.zeros_like(px, dtype=torch.bool), torch.zeros_like(py, dtype=torch.bool)
    t = 0
    for s in range(Sb):
        ky[s, t:frames[s]] = True
        kx[s, frames[s]] = True
        t = frames[s] if reg else frames[s] + 1
    ky[Sb, t:Tb] = True
    px[~kx] = -math.inf
    py[~ky] = -math.inf


@functools.lru_cache(maxsize=None)
def make(name):
    """-> dict(px, py float32 with NaN outside every utterance's cells; boundary (B,4) int64 (entries above
    the shape and negative ones where the row kind says so); sb, tb: the clamped lengths as lists; ty; S; T;
    B).  Computed once per process and shared (do not modify)."""
    c = CASES[name]
    ty, B, S, T = c["ty"], c["B"], c["S"], c["T"]
    reg = ty == "regular"
    g = torch.Generator().manual_seed(9000 + c["seed"])
    px = c["scale"] * torch.randn(B, S, T + 1 if reg else T, generator=g) - 1.0
    py = c["scale"] * torch.randn(B, S + 1, T, generator=g) - 1.0
    if c["quant"]:
        px, py = torch.round(px * 4.0) / 4.0, torch.round(py * 4.0) / 4.0
    boundary = torch.zeros(B, 4, dtype=torch.int64)
    for b in range(B):
        kind = c["rows"][b % len(c["rows"])]
        assert kind in KINDS
        rt = int(torch.randint(1, T + 1, (1,), generator=g))
        rs = int(torch.randint(0, (S if reg else min(S, rt)) + 1, (1,), generator=g))
        e = min(S, T)
        sb, tb = {"full": (S, T), "rand": (rs, rt), "s0": (0, T), "t0s0": (0, 0), "t0": (S, 0), "above": (S + 3, T + 2),
                  "neg": (-1, -2), "eq": (e, e), "eq1": (min(S, e + 1), min(S, e + 1) - 1)}[kind]
        boundary[b, 2], boundary[b, 3] = sb, tb
    sbs = [clamp(boundary[b, 2], S) for b in range(B)]
    tbs = [clamp(boundary[b, 3], T) for b in range(B)]
    if c["special"] == "inf":
        frames = [1, 1, 3, 5] if reg else [0, 2, 3, 5]
        for b in range(2):
            _one_path(px[b], py[b], S, T, reg, frames)
        px[1, 2, frames[2]] = -math.inf                    # row 1: the single path loses an arc
    for b in range(B):
        sb, tb = sbs[b], tbs[b]
        if reg:
            px[b, :, tb] = -math.inf                       # (the builders' column Tb)
            px[b, :, tb + 1:] = NAN
        else:
            px[b, :, tb:] = NAN
        px[b, sb:] = NAN
        py[b, sb + 1:] = NAN
        py[b, :, tb:] = NAN
    return dict(px=px, py=py, boundary=boundary, sb=sbs, tb=tbs, ty=ty, S=S, T=T, B=B)


def evaluate(name, dtype):
    """The restatement on a case in `dtype` -> per utterance a rnnt_align_f64.Result."""
    m = make(name)
    return [A.align(m["px"][b].to(dtype), m["py"][b].to(dtype), m["sb"][b], m["tb"][b], m["ty"])
            for b in range(m["B"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The float32 results of a case: the kernel's outputs bit for bit (do not modify)."""
    return evaluate(name, torch.float32)


def dense(results, S):
    """Per-utterance Results -> the entry's output tensors with its sentinels: (tok_frame (B,S) int32,
    tok_logp (B,S) float64, score (B) float64, ok (B) int32)."""
    B = len(results)
    tf = torch.full((B, S), -1, dtype=torch.int32)
    lp = torch.zeros((B, S), dtype=torch.float64)
    score = torch.tensor([r.score for r in results], dtype=torch.float64)
    ok = torch.tensor([int(r.ok) for r in results], dtype=torch.int32)
    for b, r in enumerate(results):
        if r.ok and r.tok_frame:
            n = len(r.tok_frame)
            tf[b, :n] = torch.tensor(r.tok_frame, dtype=torch.int32)
            lp[b, :n] = torch.tensor(r.tok_logp, dtype=torch.float64)
    return tf, lp, score, ok
