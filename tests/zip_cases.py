"""Seeded cases shared by tests/test_zip_f64.py (CPU) and tests/test_gpu_zip_stream_kernels.py (GPU).

Test infrastructure (not a test file).  Every case fixes a seed and a shape; FP32_COST holds what
float32 costs the REFERENCE (tests/zip_f64.py evaluated in float32 on the CPU against float64) on
exactly these inputs, per output tensor.  The CPU file measures and checks the figures; the GPU file
takes its bounds from them (bound(): max(2e-5, 8 x figure)), so the figures measure the reference
only, never a kernel.  Error measure everywhere: max |got - ref| / max |ref| per tensor.

Why each case is there (csrc/zip_elem.hip, csrc/zip_glue.hip; the launch code names the numbers):

Swoosh (group "sw"; forward and backward; grid = min(4096, ceil(n / 1024)) workgroups of 256, a
  float4 body over n / 4 quads and a scalar tail over the last n % 4 elements, both grid-stride):
    sw_n4         one float4, no tail                 sw_n3        tail only, the body loop is empty
    sw_n1027      256 quads + a tail of 3 (SwooshR)
    sw_overcap    n = 4 (4096 * 256 + 257): a partial second trip past the grid cap (SwooshR)
    sw_sat_l, sw_sat_r       0, -0.0, +-20, +-87, +-88.5, +-100, +-1e4 spliced into N(0, 3): __expf
                  overflows to inf, __fdividef meets a denominator above 2^126, u == 1 in log1p_fast
    sw_sat100_l, sw_sat100_r the same without +-1e4, so that max |ref| = 100 does not hide the rest
    sw_view       (group "swmod") the wrappers on a [1:4097] view at data_ptr % 16 == 4
BiasNorm (group "bn"; forward: one wave per row, 4 rows per workgroup, lanes stride the row by 64;
  backward <CPL> = 1, 2, 4, 8, 16 columns per lane for D <= 64, 128, 256, 512, 1024 on
  min(1024, ceil(rows / 32)) workgroups, a wave takes rows w and w + nwaves per trip (has2), dbias /
  dls by one atomic per column and workgroup; every case pre-fills dbias / dls):
    bn_d8, bn_d64 <1>   bn_d68, bn_d128 <2>   bn_d132, bn_d256 <4>   bn_d260, bn_d512 <8>
    bn_d516, bn_d1024 <16>   at 37 rows: first and last D of each instantiation, partial last
                  column groups (2 workgroups of 4 waves: has2 true and false in one launch)
    bn_r1, bn_r3  one workgroup, idle waves, has2 false     bn_r5   wave 0 has2, the others not
    bn_r9         8 + 1 rows: every wave has2 but wave 0's second trip does not exist
    bn_cap        32 * 1024 + 33 rows at D = 8: 1026 workgroups wanted, 1024 given: 8192 rows per
                  trip, a fifth trip of 33 waves whose second row does not exist
    bn_offset     x = 100 + N(0,1), bias = 100 + 0.3 N(0,1): the subtraction before the square
    bn_zerog      every gradient row exactly zero: the `t != 0` atomics skip (dbias / dls keep their
                  pre-filled values bit for bit, dx is exactly zero)
    bn_d1028      forward only: its row loop takes any D (17 trips of 64 lanes, the last of 4), where the
                  backward refuses D > 1024
    bn_tb_b1t7, bn_tb_b5t1, bn_tb_b3t50   the _tb form (batch-major in, time-major out / g) at
                  (B,T) = (1,7), (5,1), (3,50)
Norm + bypass (group "nb"; forward one wave per row; backward 16-byte form <Q,RT> = <1,4> D <= 256,
  <2,2> D <= 512, <4,1> above on min(512, ceil(rows / (32 or 64 from 8192 rows))) workgroups, a wave
  takes RT rows per trip; scalar form <CPL> when D % 4 != 0 or an operand is off 16 bytes; every
  case pre-fills d_bypass_scale / dbias / dls):
    nb_d4, nb_d256 <1,4>   nb_d260, nb_d512 <2,2>   nb_d516, nb_d1024 <4,1>   at 37 rows, B = 3,
                  alternately with and without fm
    nb_r1, nb_r5  one workgroup with idle waves (B = 1, and B = 3 with fm)
    nb_r17_q1, nb_r9_q2, nb_r5_q4   4 * RT + 1 rows: wave 0 alone makes a second trip
    nb_r8191, nb_r8192   the rows-per-workgroup switch (256 and 128 workgroups), D = 8, B = 7 (7
                  divides neither 1024 nor 512 waves: a wave meets every fm row), with fm
    nb_cap16      64 * 512 + 65 rows at D = 4: 514 workgroups wanted, 512 given, a partial fifth trip
    nb_s6 <1>  nb_s70 <2>  nb_s130 <4>  nb_s258 <8>  nb_s514 <16>   the scalar form by D % 4 != 0
    nb_mis        D = 64 at data_ptr % 16 == 4 of x, orig, g, dx and d_orig: the scalar form
    nb_fmzero     one fm row all zero: out, d_orig and dx of its rows are exactly zero
Balancer (group "bal"; s2t_balancer_bwd, and s2t_balancer_stats + s2t_balancer_apply; tensors `out`
  and `upd` = out - g (* swoosh'), the update alone, which is at most 4 % of out):
  general form: col_stats on (min(256, ceil(rows / 64)), min(16, ceil(C / 64))) workgroups of 64
  columns x 4 row lanes, 8 rows in flight; apply on min(2048, ceil(rows / 16)) workgroups, 4 rows in
  flight, coefficients per workgroup in LDS:
    bal_c1, bal_c63, bal_c64, bal_c65, bal_c100   at 65 rows (two col_stats workgroups, 8-unroll
                  taken by lane 0 and the tail by all; apply 5 workgroups, 4-unroll and tail)
    bal_c1024     gy capped at 16: the c0 loop strides (37 rows)
    bal_r1        one row: every channel has E[x^2] - mean^2 = 0: live_v false everywhere
    bal_r3, bal_r4   fewer rows than row lanes, and exactly one per lane
    bal_r33       8 * 4 + 1 rows: one 8-unroll trip of col_stats and one tail row
    bal_gxcap     64 * 256 + 65 rows at C = 64: past the gx cap of col_stats
    bal_applycap  16 * 2048 + 17 rows at C = 8 with ldx, ldg, ldo = 9, 10, 11: the general form (not
                  contiguous), past the apply cap
    bal_strided   65 x 100 with ldx, ldg, ldo = 108, 104, 112
    bal_c12       contiguous, C no power of two: the general form
    bal_dead_gen  64 x 12: channel 1 constant 0.5 (live_v false), channel 2 all zero (live_r false too)
  small flat form (C in 4, 8, 16, 32 contiguous and aligned; min(2048, ceil(nquads / 2048))
  workgroups, 4 quads in flight in the statistics, 2 in the update):
    bal_s4_q1, bal_s4_q255, bal_s4_q257   nquads 1, 255, 257 at C = 4
    bal_s4_q1025  one past the 4 * step unroll (step = 256)
    bal_s8, bal_s16, bal_s32   260 / 260 / 264 quads: every channel-quad count of the shuffle tree
    bal_s4_huge   2048 * 2048 + 257 quads at C = 4: past the grid cap, a third partial trip (67 MB)
    bal_dead_small   64 x 8 with the two dead channels
  every case has channels on both sides of every clamp (mean / std in -1.2 ... 1.6 around [-0.05,
  0.6], rms from 0.05 to 19 around [0.3, 4]) as far as C reaches;
    bal_offset8   257 x 64, mean / std from -7.99 to 7.99 on channels of std 0.2 ... 5
    bal_sw_l, bal_sw_r, bal_s8_sw_l, bal_s8_sw_r   the Swoosh derivative in front, both offsets, both forms
  parity: bal_c1024 then bal_c64 through s2t_balancer_bwd must leave the other accumulator zero.
Bypass (group "by"; forward: float4 stream on min(4096, ceil(n4 / 256)) workgroups; backward: RB = 64
  rows per workgroup, thread = channel strided by 256, 4 rows in flight (r + 3 < r1) and a tail;
  forward, backward, the _mask forms (B = 3) and _acc; d_scale pre-filled):
    by_r1, by_r3, by_r4, by_r63, by_r64, by_r65   at C = 260 (a second column trip of 4 channels):
                  tail only, 4-unroll only, 15 trips + 3, a full workgroup, a second workgroup of one row
    by_c4, by_c256, by_c1024   at 65 rows          by_c6   C % 4 != 0: the forward refuses, the
                  backward is scalar and must be right
    by_overcap    n4 = 4096 * 256 + 257 (C = 4): the forward grid1 cap, 16388 backward workgroups
Downsample (group "ds"; forward one thread per output element; backward 16-byte form on (frames, row
  slices) <= 512 workgroups when B C % 4 == 0, C % 4 == 0 and aligned, else the _any form; time-major
  and batch-major (_bt) output / gradient; dw pre-filled):
    ds{1,2,4,8}_t{1, ds-1, ds, ds+1, 3 ds+1}   B = 2, C = 8: no padding, all padding but one frame,
                  the last frame collecting 1 ... ds taps
    ds_c6, ds_odd (B C = 15), ds_mis (src, g, d_src at data_ptr % 16 == 4)   the _any form, three ways
    ds_longt      dT = 514 > 512: cap / dT = 0, gy clamped to 1, gx = 512: the frame loop strides
    ds_slices     dT = 300, rowlen / 4 = 300 > 256 * gy (gy = 1): the slice loop
Upsample + bypass (group "up"; forward float4 stream; backward <UP,IU> = <2,4>, <4,2>, <8,1> when C % 4
  == 0, C <= 1024, aligned and up in 2, 4, 8, on min(256, ceil(n / 256)) workgroups rounded UP to a
  multiple of m = C4 / gcd(256, C4); else one workgroup per (source frame, 16 utterances); d_scale
  pre-filled):
    up2_c4, up4_c192, up8_c384, up2_c1024   T % up = 0, 1, up - 1, 1; m = 1, 3, 3, 1 (at C = 192 and
                  384 with n = 432 and 384: two workgroups wanted, three launched, the third idle)
    up4_short, up8_short   T < up: one source frame
    up2_big       n = 65 * 4 * 256 > 256 * 256: past the cap, IU items per lane
    up4_m3_cap    C = 192, n = 70 * 20 * 48 > 256 * 256: 256 workgroups rounded up to 258
    up3           up = 3     up2_c6   C % 4 != 0 (the forward refuses)     up2_c1028   C > 1024
    up2_mis       misaligned operands     up2_b1, up2_b16, up2_b17 (with up = 3)   gridDim.y = 1, 1, 2
Nonlinear attention (group "nl"; gate / out forward and backward on u (T,B,3C) = [s | x | y] with the
  (T,B) <-> (B,T) transposition; grid1 = min(4096, ceil(n / 256))):
    nl_1, nl_735, nl_33x2x64   (T,B,C) = (1,1,1), (7,3,5), (33,2,64)
    nl_overcap    129 x 2 x 4100 > 4096 * 256 elements: a second trip
    nl_sat        |s| up to 20 (tanh = +-1 in float32, 1 - tanh^2 = 0)
  du is written in thirds: [ds | dx] by gate_bwd, [dy] by out_bwd; the third neither writes keeps
  its sentinel.
attn_delta_pairs (group "dp"; one wave per (h,b,i), lane < dv, the dW0 row strided by 64):
    dp_dv4_t1, dp_dv12_t63, dp_dv63_t64, dp_dv64_t65   dv1 = dv2, with dW0
    dp_mixed_t130 dv1 = 12, dv2 = 64, T = 130 (three trips over the dW0 row, the last of 2)
    dp_one_pair   the second pair absent           dp_no_dw0   without dW0
param_grad_commit_n (group "cm"; up to 8 items per launch, grid over the longest):
    cm_n1, cm_n1_nolimit   one item of 257         cm_n8   lengths 1, 255, 257, 5000, 1, 255, 257, 5000
                  with limit on and off alternately; x below lo, above hi and inside, both signs of d
add (group "add"): add_n4, add_n1027 (float4 body + tail of 3), add_overcap (a second trip).
"""
import functools
import math

import torch

import zip_f64 as ZF
from yardstick import FLOOR, MARGIN, UNIT, _leaf, bound_of, rel_err  # noqa: F401  (the rule of tests/yardstick.py)

SAT = (0.0, -0.0, 20.0, -20.0, 87.0, -87.0, 88.5, -88.5, 100.0, -100.0, 1e4, -1e4)
STREAM_CAP = 4096 * 256            # float4 elements one trip of a swoosh / add / bypass stream covers
BAL_CFG = (-0.05, 0.6, 0.3, 4.0, 0.04)     # min_mean, max_mean, min_rms, max_rms, grad_scale
BAL_MU = (-1.2, -0.4, 0.15, 0.35, 1.0, 1.6)
BAL_SD = (0.05, 0.12, 0.6, 1.5, 6.0, 10.0, 0.9)
LO, HI = -0.5, 0.5


def _sw(seed, n, is_l, sat=None):
    return dict(group="sw", seed=seed, n=n, is_l=is_l, sat=sat)


def _bn(seed, rows, D, kind="plain", tb=None):
    return dict(group="bn", seed=seed, rows=rows, D=D, kind=kind, tb=tb)


def _nb(seed, rows, B, D, fm, mis=False, fmzero=False):
    return dict(group="nb", seed=seed, rows=rows, B=B, D=D, fm=fm, mis=mis, fmzero=fmzero)


def _bal(seed, rows, C, ld=None, kind="plain", swoosh=None):
    return dict(group="bal", seed=seed, rows=rows, C=C, ld=ld, kind=kind, swoosh=swoosh)


def _by(seed, rows, C):
    return dict(group="by", seed=seed, rows=rows, C=C, B=3)


def _ds(seed, ds, T, B=2, C=8, mis=False):
    return dict(group="ds", seed=seed, ds=ds, T=T, B=B, C=C, mis=mis)


def _up(seed, up, T, B, C, mis=False):
    return dict(group="up", seed=seed, up=up, T=T, B=B, C=C, mis=mis)


def _dp(seed, T, B, H, dv1, dv2, dw0=True):
    return dict(group="dp", seed=seed, T=T, B=B, H=H, dv1=dv1, dv2=dv2, dw0=dw0)


CASES = {
    # ---------------------------------------------------------------- Swoosh
    "sw_n4": _sw(1, 4, True), "sw_n3": _sw(2, 3, True), "sw_n1027": _sw(3, 1027, False),
    "sw_overcap": _sw(4, 4 * (STREAM_CAP + 257), False),
    "sw_sat_l": _sw(5, 4096, True, SAT), "sw_sat_r": _sw(6, 4096, False, SAT),
    "sw_sat100_l": _sw(7, 4096, True, SAT[:-2]), "sw_sat100_r": _sw(8, 4096, False, SAT[:-2]),
    "sw_view": dict(group="swmod", seed=9, n=4096, is_l=True),
    # ---------------------------------------------------------------- BiasNorm
    **{f"bn_d{D}": _bn(10 + i, 37, D) for i, D in enumerate((8, 64, 68, 128, 132, 256, 260, 512, 516, 1024))},
    "bn_r1": _bn(20, 1, 64), "bn_r3": _bn(21, 3, 64), "bn_r5": _bn(22, 5, 64), "bn_r9": _bn(23, 9, 64),
    "bn_cap": _bn(24, 32 * 1024 + 33, 8),
    "bn_offset": _bn(25, 37, 256, "offset"), "bn_zerog": _bn(26, 5, 64, "zerog"),
    "bn_tb_b1t7": _bn(27, 7, 68, tb=(1, 7)), "bn_tb_b5t1": _bn(28, 5, 68, tb=(5, 1)),
    "bn_tb_b3t50": _bn(29, 150, 68, tb=(3, 50)),
    "bn_d1028": _bn(200, 5, 1028, "fwdonly"),
    # ---------------------------------------------------------------- BiasNorm + bypass
    **{f"nb_d{D}": _nb(30 + i, 37, 3, D, fm=bool(i % 2)) for i, D in enumerate((4, 256, 260, 512, 516, 1024))},
    "nb_r1": _nb(36, 1, 1, 64, False), "nb_r5": _nb(37, 5, 3, 64, True),
    "nb_r17_q1": _nb(38, 17, 3, 64, True), "nb_r9_q2": _nb(39, 9, 3, 260, False),
    "nb_r5_q4": _nb(40, 5, 3, 516, True),
    "nb_r8191": _nb(41, 8191, 7, 8, True), "nb_r8192": _nb(42, 8192, 7, 8, True),
    "nb_cap16": _nb(43, 64 * 512 + 65, 3, 4, False),
    **{f"nb_s{D}": _nb(44 + i, 37, 3, D, fm=bool(i % 2)) for i, D in enumerate((6, 70, 130, 258, 514))},
    "nb_mis": _nb(49, 37, 3, 64, True, mis=True),
    "nb_fmzero": _nb(50, 37, 3, 64, True, fmzero=True),
    # ---------------------------------------------------------------- Balancer
    **{f"bal_c{C}": _bal(60 + i, 65, C) for i, C in enumerate((1, 63, 64, 65, 100))},
    "bal_c1024": _bal(65, 37, 1024),
    "bal_r1": _bal(66, 1, 100), "bal_r3": _bal(67, 3, 100), "bal_r4": _bal(68, 4, 100),
    "bal_r33": _bal(69, 33, 100),
    "bal_gxcap": _bal(70, 64 * 256 + 65, 64),
    "bal_applycap": _bal(71, 16 * 2048 + 17, 8, ld=(9, 10, 11)),
    "bal_strided": _bal(72, 65, 100, ld=(108, 104, 112)),
    "bal_c12": _bal(73, 65, 12),
    "bal_dead_gen": _bal(74, 64, 12, kind="dead"),
    "bal_s4_q1": _bal(75, 1, 4), "bal_s4_q255": _bal(76, 255, 4), "bal_s4_q257": _bal(77, 257, 4),
    "bal_s4_q1025": _bal(78, 1025, 4),
    "bal_s8": _bal(79, 130, 8), "bal_s16": _bal(80, 65, 16), "bal_s32": _bal(81, 33, 32),
    "bal_s4_huge": _bal(82, 2048 * 2048 + 257, 4),
    "bal_dead_small": _bal(83, 64, 8, kind="dead"),
    "bal_offset8": _bal(84, 257, 64, kind="offset8"),
    "bal_sw_l": _bal(85, 65, 100, swoosh=True), "bal_sw_r": _bal(86, 65, 100, swoosh=False),
    "bal_s8_sw_l": _bal(87, 130, 8, swoosh=True), "bal_s8_sw_r": _bal(88, 130, 8, swoosh=False),
    # ---------------------------------------------------------------- bypass
    **{f"by_r{R}": _by(90 + i, R, 260) for i, R in enumerate((1, 3, 4, 63, 64, 65))},
    "by_c4": _by(96, 65, 4), "by_c256": _by(97, 65, 256), "by_c1024": _by(98, 65, 1024),
    "by_c6": _by(99, 65, 6),
    "by_overcap": _by(100, STREAM_CAP + 257, 4),
    # ---------------------------------------------------------------- downsample
    **{f"ds{ds}_t{T}": _ds(110 + 5 * j + i, ds, T)
       for j, ds in enumerate((1, 2, 4, 8))
       for i, T in enumerate(sorted({1, max(1, ds - 1), ds, ds + 1, 3 * ds + 1}))},
    "ds_c6": _ds(131, 4, 9, 2, 6), "ds_odd": _ds(132, 2, 7, 3, 5), "ds_mis": _ds(133, 4, 9, 2, 8, mis=True),
    "ds_longt": _ds(134, 2, 1027, 1, 4), "ds_slices": _ds(135, 2, 600, 5, 240),
    # ---------------------------------------------------------------- upsample + bypass
    "up2_c4": _up(140, 2, 10, 3, 4), "up4_c192": _up(141, 4, 9, 3, 192), "up8_c384": _up(142, 8, 15, 2, 384),
    "up2_c1024": _up(143, 2, 7, 2, 1024),
    "up4_short": _up(144, 4, 3, 3, 64), "up8_short": _up(145, 8, 1, 3, 64),
    "up2_big": _up(146, 2, 130, 4, 1024), "up4_m3_cap": _up(147, 4, 279, 20, 192),
    "up3": _up(148, 3, 10, 3, 64), "up2_c6": _up(149, 2, 9, 3, 6), "up2_c1028": _up(150, 2, 5, 2, 1028),
    "up2_mis": _up(151, 2, 9, 3, 64, mis=True),
    "up2_b1": _up(152, 2, 9, 1, 6), "up2_b16": _up(153, 2, 5, 16, 6), "up3_b17": _up(154, 3, 5, 17, 8),
    # ---------------------------------------------------------------- nonlinear attention glue
    "nl_1": dict(group="nl", seed=160, T=1, B=1, C=1, sat=False),
    "nl_735": dict(group="nl", seed=161, T=7, B=3, C=5, sat=False),
    "nl_33x2x64": dict(group="nl", seed=162, T=33, B=2, C=64, sat=False),
    "nl_overcap": dict(group="nl", seed=163, T=129, B=2, C=4100, sat=False),
    "nl_sat": dict(group="nl", seed=164, T=7, B=3, C=64, sat=True),
    # ---------------------------------------------------------------- attention row constants
    "dp_dv4_t1": _dp(170, 1, 2, 3, 4, 4), "dp_dv12_t63": _dp(171, 63, 2, 2, 12, 12),
    "dp_dv63_t64": _dp(172, 64, 1, 2, 63, 63), "dp_dv64_t65": _dp(173, 65, 2, 3, 64, 64),
    "dp_mixed_t130": _dp(174, 130, 2, 2, 12, 64),
    "dp_one_pair": _dp(175, 65, 2, 3, 12, 0), "dp_no_dw0": _dp(176, 65, 2, 3, 12, 64, dw0=False),
    # ---------------------------------------------------------------- parameter gradient commit
    "cm_n1": dict(group="cm", seed=180, lens=(257,), limit=(1,)),
    "cm_n1_nolimit": dict(group="cm", seed=181, lens=(257,), limit=(0,)),
    "cm_n8": dict(group="cm", seed=182, lens=(1, 255, 257, 5000) * 2, limit=(1, 0) * 4),
    # ---------------------------------------------------------------- add
    "add_n4": dict(group="add", seed=190, n=4), "add_n1027": dict(group="add", seed=191, n=1027),
    "add_overcap": dict(group="add", seed=192, n=4 * (STREAM_CAP + 257)),
}


def names(group):
    return [k for k, v in CASES.items() if v["group"] == group]


# ------------------------------------------------------------------ inputs
def _standardised(z):
    """Columns of z with sample mean 0 and sample std 1 (so that a case's mean / std is what it asks for)."""
    return (z - z.mean(0)) / z.std(0, unbiased=False)


def make(name):
    """-> dict of the case's float32 CPU inputs (and plain settings)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(3000 + c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=g)                        # noqa: E731
    grp = c["group"]
    if grp == "sw":
        n = c["n"]
        t = dict(x=rn(n) * 3, g=rn(n))
        if c["sat"]:
            idx = torch.randperm(n, generator=g)[:4 * len(c["sat"])]
            t["x"][idx] = torch.tensor(c["sat"]).repeat(4)
            t["sat_idx"] = idx
        return t
    if grp == "swmod":
        return dict(buf=rn(c["n"] + 4) * 3, gbuf=rn(c["n"] + 4))
    if grp == "bn":
        R, D = c["rows"], c["D"]
        t = dict(x=rn(R, D) * 2 + 0.5, bias=0.3 * rn(D), ls=torch.tensor([0.3]), g=rn(R, D),
                 db0=rn(D), dl0=rn(1))
        if c["kind"] == "offset":
            t["x"], t["bias"] = 100 + rn(R, D), 100 + 0.3 * rn(D)
        if c["kind"] == "zerog":
            t["g"].zero_()
        if c["tb"]:
            B, T = c["tb"]
            t["x"], t["g"] = t["x"].view(B, T, D), t["g"].view(T, B, D)
        return t
    if grp == "nb":
        R, B, D = c["rows"], c["B"], c["D"]
        t = dict(x=rn(R, D) * 2 + 0.5, bias=0.3 * rn(D), ls=torch.tensor([0.3]), orig=rn(R, D),
                 bscale=0.1 + 0.8 * ru(D), g=rn(R, D), dk0=rn(D), db0=rn(D), dl0=rn(1),
                 fm=(0.5 + ru(B, D)) if c["fm"] else None)
        if c["fmzero"]:
            t["fm"][B - 1] = 0.0
        return t
    if grp == "bal":
        R, C = c["rows"], c["C"]
        if c["kind"] == "offset8":
            sd = torch.exp(torch.linspace(math.log(0.2), math.log(5.0), C))[torch.randperm(C, generator=g)]
            x = (_standardised(rn(R, C)) + torch.linspace(-7.99, 7.99, C)) * sd
        elif R < 3:
            x = rn(R, C) * 1.5
        else:
            mu = torch.tensor([BAL_MU[i % len(BAL_MU)] for i in range(C)])
            sd = torch.tensor([BAL_SD[i % len(BAL_SD)] for i in range(C)])
            x = (_standardised(rn(R, C)) + mu) * sd
        if c["kind"] == "dead":
            x[:, 1] = 0.5           # sums, mean and E[x^2] - mean^2 = 0 are exact in every precision
            x[:, 2] = 0.0
        return dict(x=x, g=rn(R, C))
    if grp == "by":
        R, C, B = c["rows"], c["C"], c["B"]
        return dict(orig=rn(R, C), src=rn(R, C), scale=0.1 + 0.8 * ru(C), g=rn(R, C), fm=0.5 + ru(B, C),
                    acc_in=rn(R, C), dk0=rn(C))
    if grp == "ds":
        ds, T, B, C = c["ds"], c["T"], c["B"], c["C"]
        dT = (T + ds - 1) // ds
        return dict(src=rn(T, B, C), w=rn(ds).softmax(0), g=rn(dT, B, C), dw0=rn(ds))
    if grp == "up":
        up, T, B, C = c["up"], c["T"], c["B"], c["C"]
        return dict(orig=rn(T, B, C), src=rn((T + up - 1) // up, B, C), scale=0.1 + 0.8 * ru(C),
                    g=rn(T, B, C), dk0=rn(C))
    if grp == "nl":
        T, B, C = c["T"], c["B"], c["C"]
        u = rn(T, B, 3 * C)
        if c["sat"]:
            u[..., :C] = (u[..., :C] * 8).clamp(-20, 20)
            u[0, 0, :4] = torch.tensor([20.0, -20.0, 19.5, -19.5])
        return dict(u=u, z=rn(B, T, C), g=rn(T, B, C), dxs=rn(B, T, C))
    if grp == "dp":
        T, B, H = c["T"], c["B"], c["H"]
        t = dict(W=rn(H, B, T, T).softmax(-1), dW0=rn(B, T, T) if c["dw0"] else None, pairs=[])
        for dv in (c["dv1"], c["dv2"]):
            t["pairs"].append((rn(T, B, H * dv), rn(T, B, H * dv)) if dv else None)
        return t
    if grp == "cm":
        return dict(items=[dict(x=rn(n), d=rn(n), grad=rn(n)) for n in c["lens"]])
    if grp == "add":
        return dict(a=rn(c["n"]), b=rn(c["n"]))
    raise KeyError(grp)


def fm_rows(fm, rows):
    """The feature mask (B, D) as the kernels index it: row r takes fm[r % B]."""
    return None if fm is None else fm[torch.arange(rows) % fm.shape[0]]


@functools.lru_cache(maxsize=None)
def bal_kappa(name):
    """1 + max_c (mean_c / std_c)^2 over the live channels of the case's input, in float64: the factor
    by which var = E[x^2] - mean^2 from float32 sums amplifies rounding (zip_elem.hip takes the
    Balancer's variance that way by design).  A channel whose variance is at the 1e-20 clamp has no
    variance term left to amplify.  Computed from the case's input, never from a kernel's output."""
    x = make(name)["x"].double()
    m, v = x.mean(0), (x * x).mean(0) - x.mean(0) ** 2
    live = v > 1.0e-20
    if not bool(live.any()):
        return 1.0
    return 1.0 + float((m[live] ** 2 / v[live]).max())


# ------------------------------------------------------------------ the yardstick on a case
def _eval_sw(c, t, dt):
    x = _leaf(t["x"], dt)
    y = ZF.swoosh_ref(x, c["is_l"])
    (y * t["g"].to(dt)).sum().backward()
    return dict(y=y.detach(), d=x.grad)


def _eval_swmod(c, t, dt):
    n = c["n"]
    x = _leaf(t["buf"][1:n + 1], dt)
    y = ZF.swoosh_ref(x, c["is_l"])
    (y * t["gbuf"][1:n + 1].to(dt)).sum().backward()
    return dict(y=y.detach(), d=x.grad)


def _eval_bn(c, t, dt):
    x, b, ls = _leaf(t["x"], dt), _leaf(t["bias"], dt), _leaf(t["ls"], dt)
    y, scales = (ZF.biasnorm_tb_ref if c["tb"] else ZF.biasnorm_ref)(x, b, ls[0])
    if c["kind"] == "fwdonly":
        return dict(y=y.detach(), scales=scales.detach().reshape(-1))
    (y * t["g"].to(dt)).sum().backward()
    return dict(y=y.detach(), scales=scales.detach().reshape(-1), dx=x.grad,
                dbias=t["db0"].to(dt) + b.grad, dls=t["dl0"].to(dt) + ls.grad)


def _eval_nb(c, t, dt):
    x, b, ls, o, k = (_leaf(t[n], dt) for n in ("x", "bias", "ls", "orig", "bscale"))
    fm = fm_rows(t["fm"], c["rows"])
    out, scales = ZF.norm_bypass_ref(x, b, ls[0], o, k, None if fm is None else fm.to(dt))
    (out * t["g"].to(dt)).sum().backward()
    return dict(out=out.detach(), scales=scales.detach(), dx=x.grad, d_orig=o.grad,
                d_bscale=t["dk0"].to(dt) + k.grad, dbias=t["db0"].to(dt) + b.grad,
                dls=t["dl0"].to(dt) + ls.grad)


def _eval_bal(c, t, dt):
    x, g = t["x"].to(dt), t["g"].to(dt)
    out = ZF.balancer_bwd_ref(x, g, *BAL_CFG, swoosh=c["swoosh"])
    ge = g if c["swoosh"] is None else g * ZF.swoosh_grad_ref(x, c["swoosh"])
    return dict(out=out, upd=out - ge)


def _eval_by(c, t, dt):
    R = c["rows"]
    res = {}
    for sfx, fm in (("", None), ("_m", fm_rows(t["fm"], R).to(dt))):
        o, s, k = (_leaf(t[n], dt) for n in ("orig", "src", "scale"))
        out = ZF.bypass_ref(o, s, k, fm)
        (out * t["g"].to(dt)).sum().backward()
        res.update({"out" + sfx: out.detach(), "d_orig" + sfx: o.grad, "d_src" + sfx: s.grad,
                    "d_scale" + sfx: t["dk0"].to(dt) + k.grad})
    o, s, k = (_leaf(t[n], dt) for n in ("orig", "src", "scale"))
    out, extra = ZF.bypass_acc_ref(o, s, k, t["acc_in"].to(dt))
    ((out * t["g"].to(dt)).sum() + extra).backward()
    res["d_orig_acc"] = o.grad
    return res


def _eval_ds(c, t, dt):
    s, w = _leaf(t["src"], dt), _leaf(t["w"], dt)
    out = ZF.downsample_ref(s, w, c["ds"])
    (out * t["g"].to(dt)).sum().backward()
    return dict(out=out.detach(), out_bt=ZF.downsample_ref(s, w, c["ds"], True).detach(), d_src=s.grad,
                dw=t["dw0"].to(dt) + w.grad)


def _eval_up(c, t, dt):
    o, s, k = (_leaf(t[n], dt) for n in ("orig", "src", "scale"))
    out = ZF.upsample_bypass_ref(o, s, k, c["up"])
    (out * t["g"].to(dt)).sum().backward()
    return dict(out=out.detach(), d_orig=o.grad, d_src=s.grad, d_scale=t["dk0"].to(dt) + k.grad)


def _eval_nl(c, t, dt):
    u, z = _leaf(t["u"], dt), _leaf(t["z"], dt)
    xs, o = ZF.nonlin_gate_ref(u), ZF.nonlin_out_ref(z, u)
    ((xs * t["dxs"].to(dt)).sum() + (o * t["g"].to(dt)).sum()).backward()
    return dict(xs=xs.detach(), o=o.detach(), dz=z.grad, du=u.grad)


def _eval_dp(c, t, dt):
    pairs = [(a.to(dt), b.to(dt)) for a, b in filter(None, t["pairs"])]
    dW0 = None if t["dW0"] is None else t["dW0"].to(dt)
    return dict(delta=ZF.attn_delta_pairs_ref(t["W"].to(dt), dW0, pairs, c["T"], c["B"], c["H"]))


def _eval_cm(c, t, dt):
    return dict(grad=[ZF.commit_ref(it["x"].to(dt), it["d"].to(dt), it["grad"].to(dt), LO, HI, lim)[0]
                      for it, lim in zip(t["items"], c["limit"])])


def _eval_add(c, t, dt):
    return dict(out=ZF.add_ref(t["a"].to(dt), t["b"].to(dt)))


def evaluate(name, dtype, t=None):
    """The yardstick (tests/zip_f64.py), forward and backward, on the case's inputs cast to `dtype`
    -> {tensor name: tensor, or list of tensors (one per item of a commit case)}."""
    c = CASES[name]
    t = make(name) if t is None else t
    return globals()["_eval_" + c["group"]](c, t, dtype)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


def fp32_figures(name):
    """{tensor: rel_err of the float32 CPU evaluation of the yardstick against float64}."""
    ref, f32 = reference(name), evaluate(name, torch.float32)
    return {k: rel_err(f32[k], ref[k]) for k in ref}


def bound(name, tensor):
    """Allowed rel_err of device tensor `tensor` of case `name`: max(2e-5, 8 x the float32 figure of
    the yardstick).  One derived exception: the Balancer's tensors have the figure multiplied by
    kappa = 1 + max_c (mean_c / std_c)^2 of the case's input (bal_kappa), because the kernel takes
    var = E[x^2] - mean^2 from float32 sums by design (stated in csrc/zip_elem.hip), where the
    figure is measured on a reference whose float32 sums are pairwise."""
    fig = FP32_COST[name][tensor]
    if CASES[name]["group"] == "bal":
        fig = fig * bal_kappa(name)
    return bound_of(fig)


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figures(name), rounded up to two digits.  The figure is a maximum over a tensor and moves with
# the host's summation order and vector maths; tests/test_zip_f64.py checks it to a factor 4 both
# ways after raising both to UNIT, as tests/test_conf_f64.py does: a figure below one float32 rounding
# says nothing a host would repeat, and no figure below FLOOR / MARGIN = 2.5e-6 reaches a bound.
FP32_COST = {
    "sw_n4": dict(y=1.7e-8, d=1.3e-7),
    "sw_n3": dict(y=5.9e-8, d=4.0e-7),
    "sw_n1027": dict(y=6.8e-8, d=7.5e-8),
    "sw_overcap": dict(y=9.7e-8, d=1.2e-7),
    "sw_sat_l": dict(y=1.7e-8, d=6.2e-8),
    "sw_sat_r": dict(y=2.4e-8, d=7.7e-8),
    "sw_sat100_l": dict(y=6.3e-8, d=9.5e-8),
    "sw_sat100_r": dict(y=3.5e-8, d=1.1e-7),
    "sw_view": dict(y=5.7e-8, d=7.3e-8),
    "bn_d8": dict(y=1.6e-7, scales=1.3e-7, dx=1.9e-7, dbias=3.0e-7, dls=2.3e-7),
    "bn_d64": dict(y=1.1e-7, scales=1.1e-7, dx=1.3e-7, dbias=7.1e-8, dls=1.1e-7),
    "bn_d68": dict(y=1.6e-7, scales=1.6e-7, dx=1.5e-7, dbias=4.9e-8, dls=2.7e-7),
    "bn_d128": dict(y=9.9e-8, scales=9.9e-8, dx=1.2e-7, dbias=5.8e-8, dls=7.0e-8),
    "bn_d132": dict(y=1.9e-7, scales=1.6e-7, dx=1.4e-7, dbias=6.0e-8, dls=2.1e-8),
    "bn_d256": dict(y=1.4e-7, scales=1.6e-7, dx=2.0e-7, dbias=7.5e-8, dls=2.2e-7),
    "bn_d260": dict(y=1.3e-7, scales=1.6e-7, dx=1.7e-7, dbias=6.2e-8, dls=2.1e-6),
    "bn_d512": dict(y=1.4e-7, scales=1.3e-7, dx=1.3e-7, dbias=4.4e-8, dls=6.9e-8),
    "bn_d516": dict(y=1.4e-7, scales=1.2e-7, dx=1.2e-7, dbias=4.7e-8, dls=5.6e-8),
    "bn_d1024": dict(y=1.4e-7, scales=1.4e-7, dx=1.6e-7, dbias=4.2e-8, dls=9.4e-8),
    "bn_r1": dict(y=2.4e-8, scales=8.8e-9, dx=4.4e-8, dbias=4.8e-8, dls=1.8e-7),
    "bn_r3": dict(y=5.1e-8, scales=2.9e-8, dx=6.0e-8, dbias=6.4e-8, dls=1.9e-7),
    "bn_r5": dict(y=1.6e-7, scales=1.2e-7, dx=1.4e-7, dbias=4.0e-8, dls=1.8e-7),
    "bn_r9": dict(y=1.6e-7, scales=1.4e-7, dx=1.5e-7, dbias=4.4e-8, dls=3.1e-7),
    "bn_cap": dict(y=2.4e-7, scales=1.3e-7, dx=1.4e-7, dbias=3.0e-7, dls=9.4e-8),
    "bn_offset": dict(y=1.7e-7, scales=1.2e-7, dx=1.7e-7, dbias=2.1e-7, dls=6.1e-8),
    "bn_zerog": dict(y=9.2e-8, scales=1.1e-7, dx=0.0, dbias=0.0, dls=0.0),
    "bn_tb_b1t7": dict(y=9.1e-8, scales=1.2e-7, dx=1.7e-7, dbias=4.7e-8, dls=7.4e-8),
    "bn_tb_b5t1": dict(y=1.2e-7, scales=1.5e-7, dx=1.5e-7, dbias=4.1e-8, dls=9.0e-8),
    "bn_tb_b3t50": dict(y=1.3e-7, scales=1.5e-7, dx=1.6e-7, dbias=9.2e-8, dls=6.6e-8),
    "bn_d1028": dict(y=9.1e-8, scales=7.2e-8),
    "nb_d4": dict(out=1.1e-7, scales=1.1e-7, dx=8.9e-8, d_orig=4.7e-8, d_bscale=5.1e-8, dbias=4.9e-8,
                  dls=1.9e-7),
    "nb_d256": dict(out=1.5e-7, scales=1.3e-7, dx=1.9e-7, d_orig=5.0e-8, d_bscale=1.1e-7, dbias=4.0e-8,
                    dls=1.1e-8),
    "nb_d260": dict(out=1.7e-7, scales=2.0e-7, dx=1.3e-7, d_orig=3.7e-8, d_bscale=1.9e-7, dbias=5.0e-8,
                    dls=5.1e-8),
    "nb_d512": dict(out=1.6e-7, scales=1.3e-7, dx=1.2e-7, d_orig=5.9e-8, d_bscale=1.6e-7, dbias=3.3e-8,
                    dls=9.7e-8),
    "nb_d516": dict(out=1.6e-7, scales=1.7e-7, dx=1.8e-7, d_orig=5.2e-8, d_bscale=1.3e-7, dbias=3.2e-8,
                    dls=4.9e-7),
    "nb_d1024": dict(out=1.7e-7, scales=1.4e-7, dx=1.5e-7, d_orig=6.5e-8, d_bscale=2.1e-7, dbias=4.1e-8,
                     dls=1.2e-7),
    "nb_r1": dict(out=4.2e-8, scales=3.4e-8, dx=1.3e-7, d_orig=3.0e-8, d_bscale=5.1e-8, dbias=3.7e-8,
                  dls=1.8e-7),
    "nb_r5": dict(out=1.1e-7, scales=1.2e-7, dx=1.7e-7, d_orig=6.1e-8, d_bscale=1.7e-7, dbias=3.6e-8,
                  dls=1.4e-7),
    "nb_r17_q1": dict(out=1.4e-7, scales=1.2e-7, dx=1.2e-7, d_orig=7.9e-8, d_bscale=1.3e-7, dbias=5.9e-8,
                      dls=6.5e-7),
    "nb_r9_q2": dict(out=1.2e-7, scales=1.6e-7, dx=1.2e-7, d_orig=4.1e-8, d_bscale=8.9e-8, dbias=4.1e-8,
                     dls=2.8e-7),
    "nb_r5_q4": dict(out=8.1e-8, scales=6.6e-8, dx=1.4e-7, d_orig=8.5e-8, d_bscale=1.1e-7, dbias=4.4e-8,
                     dls=5.6e-8),
    "nb_r8191": dict(out=1.8e-7, scales=9.8e-8, dx=1.2e-7, d_orig=5.1e-8, d_bscale=1.6e-7, dbias=1.5e-7,
                     dls=3.6e-8),
    "nb_r8192": dict(out=1.8e-7, scales=9.5e-8, dx=9.6e-8, d_orig=5.6e-8, d_bscale=2.1e-7, dbias=2.4e-7,
                     dls=3.0e-7),
    "nb_cap16": dict(out=1.3e-7, scales=8.5e-8, dx=9.4e-8, d_orig=5.1e-8, d_bscale=5.6e-7, dbias=2.1e-7,
                     dls=1.3e-6),
    "nb_s6": dict(out=1.5e-7, scales=9.3e-8, dx=1.3e-7, d_orig=3.9e-8, d_bscale=2.1e-7, dbias=8.8e-8,
                  dls=4.1e-7),
    "nb_s70": dict(out=1.2e-7, scales=1.4e-7, dx=1.1e-7, d_orig=6.0e-8, d_bscale=1.5e-7, dbias=7.7e-8,
                   dls=1.7e-7),
    "nb_s130": dict(out=2.0e-7, scales=1.3e-7, dx=1.6e-7, d_orig=4.3e-8, d_bscale=8.0e-8, dbias=5.8e-8,
                    dls=4.7e-7),
    "nb_s258": dict(out=2.0e-7, scales=1.6e-7, dx=2.0e-7, d_orig=5.9e-8, d_bscale=1.5e-7, dbias=3.3e-8,
                    dls=1.9e-7),
    "nb_s514": dict(out=1.6e-7, scales=1.2e-7, dx=1.6e-7, d_orig=4.7e-8, d_bscale=1.8e-7, dbias=3.9e-8,
                    dls=2.7e-7),
    "nb_mis": dict(out=1.3e-7, scales=1.5e-7, dx=1.3e-7, d_orig=6.1e-8, d_bscale=2.9e-7, dbias=4.2e-8,
                   dls=2.6e-7),
    "nb_fmzero": dict(out=1.1e-7, scales=1.2e-7, dx=1.1e-7, d_orig=7.8e-8, d_bscale=9.6e-8, dbias=4.0e-8,
                      dls=2.7e-8),
    "bal_c1": dict(out=3.5e-8, upd=6.1e-7),
    "bal_c63": dict(out=3.8e-8, upd=6.3e-7),
    "bal_c64": dict(out=3.6e-8, upd=3.9e-7),
    "bal_c65": dict(out=5.4e-8, upd=6.2e-7),
    "bal_c100": dict(out=5.2e-8, upd=6.0e-7),
    "bal_c1024": dict(out=5.6e-8, upd=7.1e-7),
    "bal_r1": dict(out=3.9e-8, upd=9.9e-7),
    "bal_r3": dict(out=3.9e-8, upd=6.2e-7),
    "bal_r4": dict(out=4.9e-8, upd=9.1e-7),
    "bal_r33": dict(out=3.4e-8, upd=4.7e-7),
    "bal_gxcap": dict(out=4.9e-8, upd=5.2e-7),
    "bal_applycap": dict(out=5.3e-8, upd=6.1e-7),
    "bal_strided": dict(out=3.5e-8, upd=5.4e-7),
    "bal_c12": dict(out=4.2e-8, upd=6.9e-7),
    "bal_dead_gen": dict(out=2.8e-8, upd=4.5e-7),
    "bal_s4_q1": dict(out=2.2e-8, upd=5.7e-7),
    "bal_s4_q255": dict(out=4.3e-8, upd=6.9e-7),
    "bal_s4_q257": dict(out=3.7e-8, upd=7.5e-7),
    "bal_s4_q1025": dict(out=3.2e-8, upd=4.6e-7),
    "bal_s8": dict(out=4.4e-8, upd=4.9e-7),
    "bal_s16": dict(out=3.6e-8, upd=7.0e-7),
    "bal_s32": dict(out=2.9e-8, upd=4.1e-7),
    "bal_s4_huge": dict(out=5.8e-8, upd=4.5e-7),
    "bal_dead_small": dict(out=2.7e-8, upd=5.8e-7),
    "bal_offset8": dict(out=7.6e-8, upd=1.1e-6),
    "bal_sw_l": dict(out=1.1e-7, upd=9.2e-7),
    "bal_sw_r": dict(out=1.2e-7, upd=6.8e-7),
    "bal_s8_sw_l": dict(out=7.8e-8, upd=1.4e-6),
    "bal_s8_sw_r": dict(out=1.1e-7, upd=6.5e-7),
    "by_r1": dict(out=4.9e-8, d_orig=3.6e-8, d_src=3.3e-8, d_scale=6.2e-8, out_m=5.3e-8, d_orig_m=3.5e-8,
                  d_src_m=6.9e-8, d_scale_m=7.1e-8, d_orig_acc=6.7e-8),
    "by_r3": dict(out=5.2e-8, d_orig=4.9e-8, d_src=4.3e-8, d_scale=8.4e-8, out_m=5.4e-8, d_orig_m=5.5e-8,
                  d_src_m=6.9e-8, d_scale_m=9.5e-8, d_orig_acc=1.2e-7),
    "by_r4": dict(out=7.3e-8, d_orig=6.4e-8, d_src=4.8e-8, d_scale=9.1e-8, out_m=6.0e-8, d_orig_m=4.9e-8,
                  d_src_m=3.7e-8, d_scale_m=1.1e-7, d_orig_acc=7.0e-8),
    "by_r63": dict(out=9.7e-8, d_orig=5.1e-8, d_src=3.9e-8, d_scale=1.5e-7, out_m=8.2e-8, d_orig_m=7.6e-8,
                   d_src_m=6.7e-8, d_scale_m=1.3e-7, d_orig_acc=8.0e-8),
    "by_r64": dict(out=8.3e-8, d_orig=5.3e-8, d_src=3.3e-8, d_scale=1.2e-7, out_m=1.2e-7, d_orig_m=7.5e-8,
                   d_src_m=6.8e-8, d_scale_m=1.8e-7, d_orig_acc=8.8e-8),
    "by_r65": dict(out=9.3e-8, d_orig=5.6e-8, d_src=4.2e-8, d_scale=1.2e-7, out_m=8.6e-8, d_orig_m=5.5e-8,
                   d_src_m=6.5e-8, d_scale_m=1.1e-7, d_orig_acc=9.6e-8),
    "by_c4": dict(out=7.1e-8, d_orig=5.9e-8, d_src=4.6e-8, d_scale=4.6e-8, out_m=7.6e-8, d_orig_m=7.3e-8,
                  d_src_m=6.0e-8, d_scale_m=4.8e-8, d_orig_acc=6.6e-8),
    "by_c256": dict(out=7.9e-8, d_orig=4.8e-8, d_src=3.3e-8, d_scale=1.4e-7, out_m=8.3e-8, d_orig_m=4.3e-8,
                    d_src_m=5.3e-8, d_scale_m=1.1e-7, d_orig_acc=8.5e-8),
    "by_c1024": dict(out=1.3e-7, d_orig=4.6e-8, d_src=3.7e-8, d_scale=1.1e-7, out_m=1.3e-7, d_orig_m=6.5e-8,
                     d_src_m=6.7e-8, d_scale_m=1.1e-7, d_orig_acc=7.7e-8),
    "by_c6": dict(out=6.0e-8, d_orig=4.9e-8, d_src=3.4e-8, d_scale=8.5e-8, out_m=7.5e-8, d_orig_m=3.7e-8,
                  d_src_m=3.9e-8, d_scale_m=1.1e-7, d_orig_acc=5.2e-8),
    "by_overcap": dict(out=9.7e-8, d_orig=4.5e-8, d_src=3.6e-8, d_scale=2.9e-7, out_m=9.8e-8,
                       d_orig_m=7.4e-8, d_src_m=6.6e-8, d_scale_m=2.5e-7, d_orig_acc=8.0e-8),
    "ds1_t1": dict(out=0.0, out_bt=0.0, d_src=0.0, dw=1.2e-7),
    "ds1_t2": dict(out=0.0, out_bt=0.0, d_src=0.0, dw=1.1e-7),
    "ds1_t4": dict(out=0.0, out_bt=0.0, d_src=0.0, dw=6.5e-8),
    "ds2_t1": dict(out=3.0e-8, out_bt=3.0e-8, d_src=3.0e-8, dw=1.1e-7),
    "ds2_t2": dict(out=6.8e-8, out_bt=6.8e-8, d_src=3.1e-8, dw=2.3e-8),
    "ds2_t3": dict(out=4.2e-8, out_bt=4.2e-8, d_src=6.4e-8, dw=9.4e-8),
    "ds2_t7": dict(out=4.7e-8, out_bt=4.7e-8, d_src=4.5e-8, dw=2.0e-8),
    "ds4_t1": dict(out=6.0e-8, out_bt=6.0e-8, d_src=5.3e-8, dw=1.6e-8),
    "ds4_t3": dict(out=3.1e-8, out_bt=3.1e-8, d_src=4.0e-8, dw=1.1e-7),
    "ds4_t4": dict(out=5.7e-8, out_bt=5.7e-8, d_src=2.2e-8, dw=6.0e-8),
    "ds4_t5": dict(out=4.5e-8, out_bt=4.5e-8, d_src=4.6e-8, dw=3.5e-8),
    "ds4_t13": dict(out=3.6e-8, out_bt=3.6e-8, d_src=5.5e-8, dw=5.1e-8),
    "ds8_t1": dict(out=4.0e-8, out_bt=4.0e-8, d_src=6.1e-8, dw=1.1e-7),
    "ds8_t7": dict(out=1.6e-7, out_bt=1.6e-7, d_src=2.1e-8, dw=2.2e-7),
    "ds8_t8": dict(out=8.8e-8, out_bt=8.8e-8, d_src=4.1e-8, dw=1.4e-7),
    "ds8_t9": dict(out=5.0e-8, out_bt=5.0e-8, d_src=4.5e-8, dw=9.9e-8),
    "ds8_t25": dict(out=5.2e-8, out_bt=5.2e-8, d_src=5.0e-8, dw=9.4e-8),
    "ds_c6": dict(out=4.0e-8, out_bt=4.0e-8, d_src=7.6e-8, dw=8.9e-8),
    "ds_odd": dict(out=3.1e-8, out_bt=3.1e-8, d_src=2.9e-8, dw=4.2e-7),
    "ds_mis": dict(out=6.6e-8, out_bt=6.6e-8, d_src=7.2e-8, dw=5.5e-8),
    "ds_longt": dict(out=5.8e-8, out_bt=5.8e-8, d_src=3.7e-8, dw=1.1e-6),
    "ds_slices": dict(out=7.4e-8, out_bt=7.4e-8, d_src=3.7e-8, dw=2.4e-7),
    "up2_c4": dict(out=5.6e-8, d_orig=6.2e-8, d_src=5.9e-8, d_scale=1.5e-7),
    "up4_c192": dict(out=8.8e-8, d_orig=4.4e-8, d_src=7.0e-8, d_scale=1.1e-7),
    "up8_c384": dict(out=9.4e-8, d_orig=5.0e-8, d_src=9.6e-8, d_scale=1.3e-7),
    "up2_c1024": dict(out=8.5e-8, d_orig=4.9e-8, d_src=5.2e-8, d_scale=8.1e-8),
    "up4_short": dict(out=8.0e-8, d_orig=3.9e-8, d_src=5.4e-8, d_scale=9.2e-8),
    "up8_short": dict(out=1.4e-7, d_orig=4.5e-8, d_src=3.9e-8, d_scale=4.8e-8),
    "up2_big": dict(out=1.2e-7, d_orig=4.4e-8, d_src=7.9e-8, d_scale=1.5e-7),
    "up4_m3_cap": dict(out=1.3e-7, d_orig=4.8e-8, d_src=1.2e-7, d_scale=1.8e-7),
    "up3": dict(out=7.9e-8, d_orig=5.3e-8, d_src=4.9e-8, d_scale=1.1e-7),
    "up2_c6": dict(out=5.2e-8, d_orig=5.3e-8, d_src=5.0e-8, d_scale=6.1e-8),
    "up2_c1028": dict(out=8.9e-8, d_orig=5.8e-8, d_src=5.5e-8, d_scale=1.1e-7),
    "up2_mis": dict(out=6.5e-8, d_orig=3.8e-8, d_src=6.4e-8, d_scale=8.0e-8),
    "up2_b1": dict(out=4.3e-8, d_orig=4.1e-8, d_src=3.9e-8, d_scale=8.2e-8),
    "up2_b16": dict(out=5.4e-8, d_orig=6.6e-8, d_src=4.1e-8, d_scale=8.5e-8),
    "up3_b17": dict(out=1.2e-7, d_orig=3.8e-8, d_src=5.2e-8, d_scale=1.3e-7),
    "nl_1": dict(xs=3.1e-8, o=2.8e-8, dz=1.3e-8, du=3.5e-8),
    "nl_735": dict(xs=2.3e-8, o=3.2e-8, dz=2.1e-8, du=3.5e-8),
    "nl_33x2x64": dict(xs=5.0e-8, o=4.1e-8, dz=2.7e-8, du=4.9e-8),
    "nl_overcap": dict(xs=5.6e-8, o=3.8e-8, dz=4.1e-8, du=7.6e-8),
    "nl_sat": dict(xs=5.3e-8, o=4.1e-8, dz=3.3e-8, du=7.0e-8),
    "dp_dv4_t1": dict(delta=1.2e-7),
    "dp_dv12_t63": dict(delta=1.2e-7),
    "dp_dv63_t64": dict(delta=8.6e-8),
    "dp_dv64_t65": dict(delta=9.9e-8),
    "dp_mixed_t130": dict(delta=9.1e-8),
    "dp_one_pair": dict(delta=8.0e-8),
    "dp_no_dw0": dict(delta=7.9e-8),
    "cm_n1": dict(grad=2.8e-8),
    "cm_n1_nolimit": dict(grad=5.2e-8),
    "cm_n8": dict(grad=5.8e-8),
    "add_n4": dict(out=0.0),
    "add_n1027": dict(out=5.2e-8),
    "add_overcap": dict(out=3.2e-8),
}
