"""Seeded cases shared by tests/test_conf_f64.py (CPU) and tests/test_gpu_conf_kernels.py (GPU).

Test infrastructure (not a test file).  Every case fixes a seed and a shape; FP32_COST holds what
float32 costs the REFERENCE (tests/conf_f64.py evaluated in float32 on the CPU against float64) on
exactly these inputs, per output tensor.  The CPU file measures and checks the figures; the GPU file
takes its bounds from them (bound(): max(2e-5, 8 x figure)), so the figures measure the reference
only, never a kernel.  Error measure everywhere: max |got - ref| / max |ref| per tensor.

Why each case is there (csrc/conf_elem.hip, csrc/conf_attn.hip):

LayerNorm (group "ln"; forward with and without the fused add, backward with and without resid).
  A lane owns the float4 groups lane + 64 i of a row, nv = C / 4 of them.  The backward is built as
  <NV float4 per lane, NW waves>: <1,16> C <= 256, <2,8> C <= 512, <3,4> C <= 768, <4,4> above, on
  min(256, ceil(rows / NW)) workgroups whose waves stride over the rows.
    ln_c4        one live lane                     ln_c64       plain
    ln_c252      nv = 63, the last lane idle       ln_c256      <1,16> full
    ln_c260      first <2,8>                       ln_c512      <2,8> full
    ln_c516      first <3,4>                       ln_c768      <3,4> full
    ln_c772      first <4,4>                       ln_c1024     the limit
    ln_r1, ln_r1_c772   one row: three idle waves forward, one workgroup with NW - 1 idle waves backward
    ln_r5        fewer rows than one workgroup's waves
    ln_cap16 (4115 x 64), ln_cap8 (2051 x 260), ln_cap4 (1027 x 772)   one row past 256 workgroups
                 x NW waves: the grid-stride row loop makes a second trip in exactly one wave
    ln_offset, ln_offset_c772   x = 100 + N(0,1): the mean-then-centred-variance order
    ln_constrow  one constant row: variance 0, rstd = eps^-1/2, the output is beta
LayerNorm fold (group "fold", C = 64; one s2t_layernorm_param_grad call per case, dgamma / dbeta
  pre-filled with random values so that the fold must ACCUMULATE; LN_MAX_FOLD = 8 items per launch,
  16 thread groups per channel each summing every 16th partial row):
    fold_n1, fold_n8, fold_n9   one launch not full, full, and a second launch of one item
    fold_mixed   rows (5, 272, 4115) in one call: nwg = 1, 17 (one past the 16 groups), 256
  Two items naming the SAME (dgamma, dbeta) pair are not a case: each item is folded by workgroups
  of its own (blockIdx.y) which read-modify-write the destination without atomics, so two items on
  one pair race.  The layer executor never does that (every LayerNorm has its own slots); the
  sub-case is dropped rather than bending the kernel.
SiLU streams (group "silu"; grid = min(2048, ceil(n / 4 / 256)) workgroups, grid-stride):
    silu_n4      one float4                        silu_n77x2048   the FFN's hidden shape, under the cap
    silu_overcap n = 4 (2048 * 256 + 257): a partial second trip past the grid cap
    silu_sat     0, -0.0, +-20, +-87, +-88.5, +-100, +-1e4 spliced into N(0, 3): __expf overflows to
                 inf, __fdividef meets a denominator above 2^126; everything stays finite
    silu_sat100  the same without +-1e4, so that max |ref| = 100 does not hide the rest
    silu_odd     numel % 4 != 0: outside the kernel's rule, the wrapper's device op
Dropout streams (group "drop": dropout_add with and without x, silu_drop_fwd, silu_drop_bwd):
    drop_n4; drop_p{0.1, 0.5, 1e-12, 0.999}_s{0, 2**62 - 1} at n = 77 * 2048 (1e-12: the threshold
    is forced to 1; seed 2**62 - 1: the largest a draw gives); drop_overcap_p0.1, drop_overcap_p0.5:
    element indices past 2^21 on the second trip.  The ABI takes p as a float: at p = 0.999 the
    kernel's 1 / (1 - p) is 1000.013 where the restated mask carries 1000, 1.3e-5 relative -- inside
    the 2e-5 floor, and the reason the mask is compared bit for bit at p = 0.1 and 0.5 only (the
    keep PATTERN is compared at every p).
    dropmod_view  the Dropout module on a [1:4097] view of a 4100-float buffer (address % 16 == 4)
BatchNorm + SiLU (group "bn"; bn_stats thread map cg = C / 4 column groups x rl = 256 / cg row lanes;
  per = ceil(rows / 128) rows per partial, nb = ceil(rows / per) partials, folded in 8 pieces by one
  finalize workgroup per 64 channels; a row lane has work only if per > its index, so the cases that
  are there for a thread map have 128 (rl + 1) + 1 rows, per = rl + 2):
    bn_c4        cg = 1, rl = 256                  bn_c12       cg = 3, rl = 85, one idle thread
    bn_c68       a second finalize block with 4 live channels
    bn_c192      cg = 48, rl = 5, 16 idle          bn_c256      cg = 64, rl = 4, plain
    bn_c516      cg = 129, rl = 1, 127 idle        bn_c1024     cg = 256
    bn_r2        two partials, six empty pieces    bn_r7        fewer than 8 partials, one piece empty
    bn_r127, bn_r128   below and at S2T_BN_PARTIALS
    bn_r129      per = 2, nb = 65                  bn_r257      per = 3, nb = 86
    bn_overcap   2048 * 256 * 4 / 256 + 3 = 8195 rows at C = 256: the apply and backward streams past
                 their grid cap
    bn_mom_none  momentum None over two successive batches (cumulative average)
    bn_no_track  track_running_stats False: batch statistics in evaluation as well
    bn_offset8   per-channel offsets up to |mean| / std = 8 on channels of std 0.2 .. 5
  Every case pre-fills dgamma / dbeta and uses momentum 0.1 unless it says otherwise.
Attention (group "attn"; 128 queries per workgroup, 32 per wave, keys streamed in tiles of 64 as two
  sub-tiles of 32; `break` on kb >= len, prefetch guarded by k0 + 64 < len):
    attn_t{1,31,32,33,63,64,65,127,128,129,200,300}   every tile edge of T at dh = 32; H in {1,3,8}
                 and B in 1..4 spread over them
    attn_dh16_t33, attn_dh16_t129, attn_dh64_t33, attn_dh64_t129   the other two head widths
    attn_len_a [200,32,33,64], attn_len_b [65,128,129,1], attn_len_c [0,200,450,100] at T = 200:
                 len on every tile edge below T; length 0 (exact zeros) and a length above T (clamped)
    attn_peaky   |s| up to 60, the row maximum at key T - 3 (the last tile) for about half of the rows and
                 anywhere for the rest: the running-max rescale across tiles, both ways
    attn_drop_*  dropout p in {0.1, 0.5} x ragged lens x dh in {16,32,64} x T in {33,65,129,200}
    attn_dh36_len0   dh = 36 with a length-0 utterance: outside the kernel's rule, the wrapper's path
  The strided and permuted layout (ld = 3D + 8, blocks ordered v, q, k, ldo = D + 4) reuses attn_t65,
  attn_len_b and attn_drop_dh32_t200 in the GPU file: bit-identical to the packed layout.
Outside the kernels' rules (group "lnmod", through conf_kernels.layer_norm):
    lnmod_c6, lnmod_c1028, lnmod_noaffine, lnmod_nobias, lnmod_strided (row-strided input),
    lnmod_misaligned (data_ptr % 16 == 4)
"""
import functools
import math

import torch

import conf_f64 as CF
from oracle import conformer as OC
from yardstick import FLOOR, MARGIN, UNIT, _leaf, bound_of, rel_err  # noqa: F401  (the rule of tests/yardstick.py)

EPS = 1e-5
SMAX = 2 ** 62 - 1
STREAM_CAP = 2048 * 256            # float4 elements one trip of a streaming kernel covers
SAT = (0.0, -0.0, 20.0, -20.0, 87.0, -87.0, 88.5, -88.5, 100.0, -100.0, 1e4, -1e4)


def _ln(seed, rows, C, kind="plain"):
    return dict(group="ln", seed=seed, rows=rows, C=C, kind=kind)


def _bn(seed, rows, C, momentum=0.1, batches=1, track=True, offset=False):
    return dict(group="bn", seed=seed, rows=rows, C=C, momentum=momentum, batches=batches,
                track=track, offset=offset)


def _at(seed, T, B, H, dh, lens=None, p=0.0, peaky=False, kernel=True):
    return dict(group="attn", seed=seed, T=T, B=B, H=H, dh=dh, lens=lens, p=p, peaky=peaky,
                kernel=kernel)


CASES = {
    # ---------------------------------------------------------------- LayerNorm
    "ln_c4": _ln(1, 37, 4), "ln_c64": _ln(2, 37, 64), "ln_c252": _ln(3, 37, 252),
    "ln_c256": _ln(4, 37, 256), "ln_c260": _ln(5, 37, 260), "ln_c512": _ln(6, 37, 512),
    "ln_c516": _ln(7, 37, 516), "ln_c768": _ln(8, 37, 768), "ln_c772": _ln(9, 37, 772),
    "ln_c1024": _ln(10, 37, 1024),
    "ln_r1": _ln(11, 1, 64), "ln_r1_c772": _ln(12, 1, 772), "ln_r5": _ln(13, 5, 64),
    "ln_cap16": _ln(14, 4115, 64), "ln_cap8": _ln(15, 2051, 260), "ln_cap4": _ln(16, 1027, 772),
    "ln_offset": _ln(17, 37, 256, "offset"), "ln_offset_c772": _ln(18, 37, 772, "offset"),
    "ln_constrow": _ln(19, 37, 64, "constrow"),
    # ---------------------------------------------------------------- LayerNorm fold
    "fold_n1": dict(group="fold", seed=20, C=64, rows=(37,)),
    "fold_n8": dict(group="fold", seed=21, C=64, rows=(37,) * 8),
    "fold_n9": dict(group="fold", seed=22, C=64, rows=(37,) * 9),
    "fold_mixed": dict(group="fold", seed=23, C=64, rows=(5, 272, 4115)),
    # ---------------------------------------------------------------- SiLU
    "silu_n4": dict(group="silu", seed=30, n=4, sat=None, kernel=True),
    "silu_n77x2048": dict(group="silu", seed=31, n=77 * 2048, sat=None, kernel=True),
    "silu_overcap": dict(group="silu", seed=32, n=4 * (STREAM_CAP + 257), sat=None, kernel=True),
    "silu_sat": dict(group="silu", seed=33, n=4096, sat=SAT, kernel=True),
    "silu_sat100": dict(group="silu", seed=34, n=4096, sat=SAT[:-2], kernel=True),
    "silu_odd": dict(group="silu", seed=35, n=3 * 7, sat=None, kernel=False),
    # ---------------------------------------------------------------- dropout streams
    "drop_n4": dict(group="drop", seed=40, n=4, p=0.5, dseed=0),
    **{f"drop_p{p}_s{'0' if s == 0 else 'max'}": dict(group="drop", seed=41 + i, n=77 * 2048, p=p, dseed=s)
       for i, (p, s) in enumerate((p, s) for p in (0.1, 0.5, 1e-12, 0.999) for s in (0, SMAX))},
    "drop_overcap_p0.1": dict(group="drop", seed=49, n=4 * (STREAM_CAP + 257), p=0.1, dseed=SMAX),
    "drop_overcap_p0.5": dict(group="drop", seed=50, n=4 * (STREAM_CAP + 257), p=0.5, dseed=0),
    "dropmod_view": dict(group="dropmod", seed=51, n=4096, p=0.1, dseed=123456789),
    # ---------------------------------------------------------------- BatchNorm + SiLU
    # rows = 128 (rl + 1) + 1 where rl > 1: per = rl + 2 rows per partial, so every row lane of the
    # thread map carries a sum and the first two carry two rows (fewer rows leave the lanes idle)
    "bn_c4": _bn(60, 128 * 257 + 1, 4), "bn_c12": _bn(61, 128 * 86 + 1, 12),
    "bn_c68": _bn(62, 128 * 16 + 1, 68), "bn_c192": _bn(63, 128 * 6 + 1, 192),
    "bn_c256": _bn(64, 128 * 5 + 1, 256), "bn_c516": _bn(65, 257, 516), "bn_c1024": _bn(66, 257, 1024),
    "bn_r257": _bn(76, 257, 256),
    "bn_r2": _bn(67, 2, 256), "bn_r7": _bn(68, 7, 256), "bn_r127": _bn(69, 127, 256),
    "bn_r128": _bn(70, 128, 256), "bn_r129": _bn(71, 129, 256),
    "bn_overcap": _bn(72, STREAM_CAP * 4 // 256 + 3, 256),
    "bn_mom_none": _bn(73, 129, 68, momentum=None, batches=2),
    "bn_no_track": _bn(74, 129, 68, track=False),
    "bn_offset8": _bn(75, 257, 256, offset=True),
    # ---------------------------------------------------------------- attention
    "attn_t1": _at(80, 1, 2, 3, 32), "attn_t31": _at(81, 31, 2, 1, 32),
    "attn_t32": _at(82, 32, 1, 3, 32), "attn_t33": _at(83, 33, 3, 8, 32),
    "attn_t63": _at(84, 63, 2, 3, 32), "attn_t64": _at(85, 64, 2, 1, 32),
    "attn_t65": _at(86, 65, 3, 3, 32, lens=(65, 33, 64)), "attn_t127": _at(87, 127, 2, 3, 32),
    "attn_t128": _at(88, 128, 2, 1, 32), "attn_t129": _at(89, 129, 2, 8, 32),
    "attn_t200": _at(90, 200, 4, 3, 32), "attn_t300": _at(91, 300, 4, 8, 32, lens=(300, 257, 129, 2)),
    "attn_dh16_t33": _at(92, 33, 2, 3, 16), "attn_dh16_t129": _at(93, 129, 2, 3, 16, lens=(129, 70)),
    "attn_dh64_t33": _at(94, 33, 2, 3, 64), "attn_dh64_t129": _at(95, 129, 2, 3, 64, lens=(129, 70)),
    "attn_len_a": _at(96, 200, 4, 2, 32, lens=(200, 32, 33, 64)),
    "attn_len_b": _at(97, 200, 4, 2, 32, lens=(65, 128, 129, 1)),
    "attn_len_c": _at(98, 200, 4, 2, 32, lens=(0, 200, 450, 100)),
    "attn_peaky": _at(99, 200, 2, 2, 32, peaky=True),
    "attn_drop_dh16_t33": _at(100, 33, 3, 2, 16, lens=(33, 20, 1), p=0.1),
    "attn_drop_dh16_t129": _at(101, 129, 3, 2, 16, lens=(129, 64, 33), p=0.5),
    "attn_drop_dh32_t65": _at(102, 65, 3, 3, 32, lens=(65, 64, 31), p=0.5),
    "attn_drop_dh32_t200": _at(103, 200, 3, 2, 32, lens=(200, 129, 65), p=0.1),
    "attn_drop_dh64_t33": _at(104, 33, 3, 1, 64, lens=(33, 32, 5), p=0.5),
    "attn_drop_dh64_t129": _at(105, 129, 3, 2, 64, lens=(129, 128, 70), p=0.1),
    "attn_drop_dh64_t200": _at(106, 200, 3, 2, 64, lens=(200, 0, 97), p=0.5),
    "attn_dh36_len0": _at(107, 9, 3, 2, 36, lens=(9, 0, 5), kernel=False),
    # ---------------------------------------------------------------- LayerNorm outside the rules
    "lnmod_c6": dict(group="lnmod", seed=110, C=6, affine=True, bias=True, how="plain"),
    "lnmod_c1028": dict(group="lnmod", seed=111, C=1028, affine=True, bias=True, how="plain"),
    "lnmod_noaffine": dict(group="lnmod", seed=112, C=64, affine=False, bias=False, how="plain"),
    "lnmod_nobias": dict(group="lnmod", seed=113, C=64, affine=True, bias=False, how="plain"),
    "lnmod_strided": dict(group="lnmod", seed=114, C=64, affine=True, bias=True, how="strided"),
    "lnmod_misaligned": dict(group="lnmod", seed=115, C=64, affine=True, bias=True, how="misaligned"),
}


def names(group, kernel=None):
    return [k for k, v in CASES.items()
            if v["group"] == group and (kernel is None or v.get("kernel", True) == kernel)]


# ------------------------------------------------------------------ inputs
def make(name):
    """-> dict of the case's float32 CPU inputs (and plain settings)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(2000 + c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    grp = c["group"]
    if grp == "ln":
        R, C = c["rows"], c["C"]
        t = dict(x=rn(R, C) * 2 + 0.5, y=rn(R, C), gamma=1 + 0.3 * rn(C), beta=0.3 * rn(C),
                 dy=rn(R, C), resid=rn(R, C))
        if c["kind"] == "offset":
            t["x"] = 100 + rn(R, C)
        if c["kind"] == "constrow":
            t["x"][R // 2] = 1.5
            t["y"][R // 2] = 0.5
        return t
    if grp == "lnmod":
        C = c["C"]
        t = dict(x=rn(5, 7, C) * 2 + 0.5, dy=rn(5, 7, C))
        t["gamma"] = 1 + 0.3 * rn(C) if c["affine"] else None
        t["beta"] = 0.3 * rn(C) if c["bias"] else None
        return t
    if grp == "fold":
        C = c["C"]
        return dict(items=[dict(x=rn(R, C) * 2 + 0.5, gamma=1 + 0.3 * rn(C), beta=0.3 * rn(C),
                                dy=rn(R, C), dg0=rn(C), db0=rn(C)) for R in c["rows"]])
    if grp == "silu":
        n = c["n"]
        t = dict(h=rn(n) * 3, da=rn(n))
        if c["sat"]:
            idx = torch.randperm(n, generator=g)[:4 * len(c["sat"])]
            t["h"][idx] = torch.tensor(c["sat"]).repeat(4)
            t["sat_idx"] = idx
        return t
    if grp == "drop":
        n = c["n"]
        return dict(x=rn(n), y=rn(n), h=rn(n) * 3, da=rn(n))
    if grp == "dropmod":
        return dict(buf=rn(c["n"] + 4), gbuf=rn(c["n"] + 4))
    if grp == "bn":
        R, C = c["rows"], c["C"]
        t = dict(gamma=1 + 0.3 * rn(C), beta=0.3 * rn(C), rm0=rn(C), rv0=torch.rand(C, generator=g) + 0.5,
                 ds=rn(R, C), dg0=rn(C), db0=rn(C), xs=[])
        for _ in range(c["batches"]):
            # standardised per channel first, so that the SAMPLE |mean| / std is the ratio asked for
            # (two rows of plain noise would put it anywhere): at most 8 in every case
            z = rn(R, C)
            z = (z - z.mean(0)) / z.std(0, unbiased=False)
            if c["offset"]:
                std = torch.exp(torch.linspace(math.log(0.2), math.log(5.0), C))[torch.randperm(C, generator=g)]
                x = (z + torch.linspace(-7.99, 7.99, C)) * std
            else:
                x = (z + rn(C).clamp(-2.5, 2.5) * 0.6) * 1.7
            t["xs"].append(x)
        return t
    if grp == "attn":
        T, B, H, dh = c["T"], c["B"], c["H"], c["dh"]
        D = H * dh
        qkv = rn(T, B, 3 * D)
        qkv[..., :D] *= 1.5
        if c["peaky"]:
            q = qkv[..., :D].view(T, B, H, dh)
            k = qkv[..., D:2 * D].view(T, B, H, dh)
            q[..., 0] = q[..., 0].abs() + 4.0
            k[T - 3, :, :, 0] = 5.0
            s = torch.einsum("tbhd,sbhd->bhts", q.double(), k.double()) / math.sqrt(dh)
            q *= 60.0 / float(s.abs().max())
        return dict(qkv=qkv, do=rn(T, B, D),
                    lens=None if c["lens"] is None else torch.tensor(c["lens"], dtype=torch.int64))
    raise KeyError(grp)


def attn_seed(name):
    """The dropout seed of an attention case (spread over the 62 bits a draw can give)."""
    return (CASES[name]["seed"] * 0x9E3779B97F4A7C15) % (2 ** 62)


@functools.lru_cache(maxsize=None)
def bn_kappa(name):
    """1 + max_c (mean_c / std_c)^2 of the case's input (every batch), in float64: the factor by
    which var = E[x^2] - mean^2 from float32 sums amplifies rounding (conf_elem.hip forms the batch
    variance that way by design).  Computed from the case's input, never from a kernel's output."""
    k = 1.0
    for x in make(name)["xs"]:
        x = x.double()
        m, s = x.mean(0), x.std(0, unbiased=False)
        k = max(k, 1.0 + float(((m / s) ** 2).max()))
    return k


def bn_mean_over_std(name):
    return max(float((x.double().mean(0) / x.double().std(0, unbiased=False)).abs().max())
               for x in make(name)["xs"])


# ------------------------------------------------------------------ the yardstick on a case
def _eval_ln(c, t, dt):
    out = {}
    for add in (False, True):
        x, y, g, b = (_leaf(t[k], dt) for k in ("x", "y", "gamma", "beta"))
        xsum, o = CF.layernorm_ref(x, y if add else None, 0.5, g, b, EPS)
        (o * t["dy"].to(dt)).sum().backward()
        sfx = "_add" if add else ""
        out["out" + sfx] = o.detach()
        out["dgamma" + sfx], out["dbeta" + sfx] = g.grad, b.grad
        if add:      # the backward runs on the saved sum and adds the residual branch's gradient
            out["xsum"] = xsum.detach()
            out["dx_add"] = x.grad + t["resid"].to(dt)
        else:
            out["dx"] = x.grad
            out["mean"], out["rstd"] = CF.layernorm_stats(x.detach(), EPS)
    return out


def _eval_lnmod(c, t, dt):
    x, g, b = _leaf(t["x"], dt), _leaf(t["gamma"], dt), _leaf(t["beta"], dt)
    _, o = CF.layernorm_ref(x, None, 0.0, g, b, EPS)
    (o * t["dy"].to(dt)).sum().backward()
    out = dict(out=o.detach(), dx=x.grad)
    if g is not None:
        out["dgamma"] = g.grad
    if b is not None:
        out["dbeta"] = b.grad
    return out


def _eval_fold(c, t, dt):
    dg, db = [], []
    for it in t["items"]:
        x, g, b = _leaf(it["x"], dt, False), _leaf(it["gamma"], dt), _leaf(it["beta"], dt)
        _, o = CF.layernorm_ref(x, None, 0.0, g, b, EPS)
        (o * it["dy"].to(dt)).sum().backward()
        dg.append(it["dg0"].to(dt) + g.grad)
        db.append(it["db0"].to(dt) + b.grad)
    return dict(dgamma=dg, dbeta=db)


def _eval_silu(c, t, dt):
    h = _leaf(t["h"], dt)
    a = CF.silu_ref(h)
    (a * t["da"].to(dt)).sum().backward()
    return dict(a=a.detach(), dh=0.5 * h.grad)


def _eval_drop(c, t, dt):
    m = OC.keep_scale(c["dseed"], (c["n"],), c["p"]).to(dt)
    x, y, da = (t[k].to(dt) for k in ("x", "y", "da"))
    h = _leaf(t["h"], dt)
    a = CF.silu_ref(h) * m
    (a * da).sum().backward()
    return dict(add=x + 0.5 * (y * m), grad=0.5 * (y * m), sd_fwd=a.detach(), sd_bwd=0.5 * h.grad)


def _eval_dropmod(c, t, dt, seed=None):
    n = c["n"]
    m = OC.keep_scale(c["dseed"] if seed is None else seed, (n,), c["p"]).to(dt)
    return dict(out=t["buf"][1:n + 1].to(dt) * m, grad=t["gbuf"][1:n + 1].to(dt) * m)


def _eval_bn(c, t, dt):
    g, b = _leaf(t["gamma"], dt), _leaf(t["beta"], dt)
    rm, rv = t["rm0"].to(dt), t["rv0"].to(dt)
    for i, x0 in enumerate(t["xs"]):
        x = _leaf(x0, dt)
        y, mean, var, unb = CF.bn_silu_ref(x, g, b, EPS)
        mom = 1.0 / (i + 1) if c["momentum"] is None else c["momentum"]
        rm = (1 - mom) * rm + mom * mean.detach()
        rv = (1 - mom) * rv + mom * unb.detach()
    (y * t["ds"].to(dt)).sum().backward()
    out = dict(y=y.detach(), mean=mean.detach(), rstd=(1.0 / torch.sqrt(var + EPS)).detach(),
               dgamma=t["dg0"].to(dt) + g.grad, dbeta=t["db0"].to(dt) + b.grad)
    if c["rows"] == 2:
        # two rows normalise to +-1 whatever they hold, so the true dx is zero up to eps / var and
        # "relative to max |ref|" would measure rounding noise against rounding noise: the tensor
        # held is dx + ds (the sum a residual branch would form), which has a size
        out["dx_plus_ds"] = x.grad + t["ds"].to(dt)
    else:
        out["dx"] = x.grad
    xe = t["ds"].to(dt) * 1.7                      # evaluation runs on another tensor of the shape
    if c["track"]:
        out["running_mean"], out["running_var"] = rm, rv
        out["y_eval"] = CF.bn_silu_eval_ref(xe, rm, rv, g.detach(), b.detach(), EPS)
    else:
        out["y_eval"] = CF.bn_silu_ref(xe, g.detach(), b.detach(), EPS)[0]
    return out


def _eval_attn(c, t, dt, seed=None):
    qkv = _leaf(t["qkv"], dt)
    T, B, H = c["T"], c["B"], c["H"]
    mask = None
    if c["p"] > 0:
        mask = OC.keep_scale(seed, (B, H, T, T), c["p"]).to(dt)
    o = CF.attn_ref(qkv, t["lens"], H, mask)
    (o * t["do"].to(dt)).sum().backward()
    if T == 1:       # one key: the probability is 1 whatever q and k are, dq = dk = 0 exactly and
        return dict(o=o.detach(), dqkv=qkv.grad)        # only the whole gradient tensor has a size
    dq, dk, dv = qkv.grad.chunk(3, dim=-1)
    return dict(o=o.detach(), dq=dq, dk=dk, dv=dv)


def evaluate(name, dtype, t=None):
    """The yardstick (tests/conf_f64.py), forward and backward, on the case's inputs cast to `dtype`
    -> {tensor name: tensor, or list of tensors (one per item of a fold case)}."""
    c = CASES[name]
    t = make(name) if t is None else t
    if c["group"] == "attn":
        return _eval_attn(c, t, dtype, attn_seed(name))
    return globals()["_eval_" + c["group"]](c, t, dtype)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64)


def fp32_figures(name):
    """{tensor: rel_err of the float32 CPU evaluation of the yardstick against float64}."""
    ref, f32 = reference(name), evaluate(name, torch.float32)
    return {k: rel_err(f32[k], ref[k]) for k in ref}


BN_VAR_TENSORS = ("y", "dx", "dx_plus_ds", "dgamma", "rstd", "running_var")


def bound(name, tensor):
    """Allowed rel_err of device tensor `tensor` of case `name`: max(2e-5, 8 x the float32 figure of
    the yardstick).  One derived exception: tensors that depend on BatchNorm's batch variance have
    the figure multiplied by kappa = 1 + max_c (mean_c / std_c)^2 of the case's input (bn_kappa),
    because the kernel takes var = E[x^2] - mean^2 from float32 partial sums by design (stated in
    csrc/conf_elem.hip; test_balancer_backward_vs_fp64_closed_form accepts the same with
    "|mean| / std <= 8 keeps four digits"), where the yardstick's two-pass form does not amplify."""
    fig = FP32_COST[name][tensor]
    if CASES[name]["group"] == "bn" and tensor in BN_VAR_TENSORS:
        fig = fig * bn_kappa(name)
    return bound_of(fig)


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figures(name), rounded up to two digits.  The figure is a maximum over a tensor and moves with
# the host's summation order and vector maths; tests/test_conf_f64.py checks it to a factor 4 both
# ways, the factor tests/test_lstm_f64.py uses, after raising both to UNIT: a figure below one
# float32 rounding (a tensor of one or four elements that happened to round well, or an exact
# product with a mask of 0 / 1 / 2: 0.0) says nothing a host would repeat, and no figure below
# FLOOR / MARGIN = 2.5e-6 reaches a bound.
FP32_COST = {
    "ln_c4": dict(out=1.1e-7, dgamma=9.6e-8, dbeta=5.5e-8, dx=1.7e-7, mean=3.7e-8, rstd=4.2e-8,
                  out_add=2.1e-7, dgamma_add=6.3e-8, dbeta_add=5.5e-8, xsum=3.5e-8, dx_add=2.6e-7),
    "ln_c64": dict(out=1.2e-7, dgamma=1.6e-7, dbeta=5.9e-8, dx=1.4e-7, mean=6.5e-8, rstd=9.4e-8,
                   out_add=9.7e-8, dgamma_add=1.3e-7, dbeta_add=5.9e-8, xsum=5.9e-8, dx_add=9.0e-8),
    "ln_c252": dict(out=1.2e-7, dgamma=1.2e-7, dbeta=1.3e-7, dx=1.4e-7, mean=9.4e-8, rstd=9.7e-8,
                    out_add=1.5e-7, dgamma_add=1.3e-7, dbeta_add=1.3e-7, xsum=3.4e-8,
                    dx_add=8.9e-8),
    "ln_c256": dict(out=1.4e-7, dgamma=1.2e-7, dbeta=1.1e-7, dx=1.3e-7, mean=8.8e-8, rstd=1.1e-7,
                    out_add=1.9e-7, dgamma_add=1.4e-7, dbeta_add=1.1e-7, xsum=3.0e-8,
                    dx_add=9.1e-8),
    "ln_c260": dict(out=1.5e-7, dgamma=9.4e-8, dbeta=1.4e-7, dx=1.4e-7, mean=9.6e-8, rstd=1.1e-7,
                    out_add=1.6e-7, dgamma_add=1.1e-7, dbeta_add=1.4e-7, xsum=3.1e-8,
                    dx_add=7.2e-8),
    "ln_c512": dict(out=1.1e-7, dgamma=1.4e-7, dbeta=6.8e-8, dx=1.5e-7, mean=6.4e-8, rstd=9.2e-8,
                    out_add=1.3e-7, dgamma_add=1.3e-7, dbeta_add=6.8e-8, xsum=3.3e-8,
                    dx_add=9.8e-8),
    "ln_c516": dict(out=1.1e-7, dgamma=1.2e-7, dbeta=1.3e-7, dx=1.6e-7, mean=1.2e-7, rstd=8.1e-8,
                    out_add=1.7e-7, dgamma_add=1.3e-7, dbeta_add=1.3e-7, xsum=2.9e-8,
                    dx_add=9.4e-8),
    "ln_c768": dict(out=1.1e-7, dgamma=1.3e-7, dbeta=1.2e-7, dx=1.8e-7, mean=9.2e-8, rstd=9.7e-8,
                    out_add=1.2e-7, dgamma_add=1.4e-7, dbeta_add=1.2e-7, xsum=4.9e-8,
                    dx_add=1.1e-7),
    "ln_c772": dict(out=1.3e-7, dgamma=1.3e-7, dbeta=1.1e-7, dx=1.9e-7, mean=1.1e-7, rstd=1.2e-7,
                    out_add=1.4e-7, dgamma_add=1.1e-7, dbeta_add=1.1e-7, xsum=5.4e-8,
                    dx_add=1.2e-7),
    "ln_c1024": dict(out=1.1e-7, dgamma=9.9e-8, dbeta=1.2e-7, dx=1.6e-7, mean=9.2e-8, rstd=7.7e-8,
                     out_add=1.4e-7, dgamma_add=1.2e-7, dbeta_add=1.2e-7, xsum=3.0e-8,
                     dx_add=1.2e-7),
    "ln_r1": dict(out=8.9e-8, dgamma=7.3e-8, dbeta=0.0, dx=1.1e-7, mean=5.1e-8, rstd=6.2e-8,
                  out_add=5.3e-8, dgamma_add=7.3e-8, dbeta_add=0.0, xsum=4.9e-8, dx_add=5.9e-8),
    "ln_r1_c772": dict(out=9.9e-8, dgamma=5.7e-8, dbeta=0.0, dx=1.2e-7, mean=1.2e-7, rstd=2.4e-9,
                       out_add=1.4e-7, dgamma_add=1.3e-7, dbeta_add=0.0, xsum=4.0e-8,
                       dx_add=4.9e-8),
    "ln_r5": dict(out=7.5e-8, dgamma=1.1e-7, dbeta=1.5e-7, dx=1.4e-7, mean=4.7e-8, rstd=6.4e-8,
                  out_add=6.9e-8, dgamma_add=8.6e-8, dbeta_add=1.5e-7, xsum=3.5e-8, dx_add=6.6e-8),
    "ln_cap16": dict(out=1.1e-7, dgamma=1.5e-7, dbeta=1.1e-7, dx=1.7e-7, mean=1.1e-7, rstd=9.3e-8,
                     out_add=1.2e-7, dgamma_add=1.5e-7, dbeta_add=1.1e-7, xsum=4.7e-8,
                     dx_add=1.1e-7),
    "ln_cap8": dict(out=1.7e-7, dgamma=2.0e-7, dbeta=1.8e-7, dx=1.7e-7, mean=1.5e-7, rstd=1.3e-7,
                    out_add=1.5e-7, dgamma_add=2.1e-7, dbeta_add=1.8e-7, xsum=4.9e-8,
                    dx_add=1.3e-7),
    "ln_cap4": dict(out=1.6e-7, dgamma=1.6e-7, dbeta=1.5e-7, dx=2.1e-7, mean=1.3e-7, rstd=1.3e-7,
                    out_add=2.4e-7, dgamma_add=1.8e-7, dbeta_add=1.5e-7, xsum=4.5e-8,
                    dx_add=1.2e-7),
    "ln_offset": dict(out=2.8e-6, dgamma=4.0e-6, dbeta=1.2e-7, dx=8.2e-7, mean=9.8e-8, rstd=1.1e-7,
                      out_add=3.4e-6, dgamma_add=5.1e-6, dbeta_add=1.2e-7, xsum=3.7e-8,
                      dx_add=4.0e-7),
    "ln_offset_c772": dict(out=4.8e-6, dgamma=4.8e-6, dbeta=8.6e-8, dx=4.8e-7, mean=1.4e-7,
                           rstd=8.4e-8, out_add=5.4e-6, dgamma_add=5.3e-6, dbeta_add=8.6e-8,
                           xsum=3.7e-8, dx_add=2.6e-7),
    "ln_constrow": dict(out=1.1e-7, dgamma=1.1e-7, dbeta=1.4e-7, dx=4.7e-8, mean=5.1e-8,
                        rstd=5.5e-8, out_add=1.1e-7, dgamma_add=1.7e-7, dbeta_add=1.4e-7,
                        xsum=2.8e-8, dx_add=3.9e-8),
    "fold_n1": dict(dgamma=1.1e-7, dbeta=1.2e-7),
    "fold_n8": dict(dgamma=1.5e-7, dbeta=1.6e-7),
    "fold_n9": dict(dgamma=2.1e-7, dbeta=1.5e-7),
    "fold_mixed": dict(dgamma=1.9e-7, dbeta=1.8e-7),
    "silu_n4": dict(a=9.0e-9, dh=1.2e-7),
    "silu_n77x2048": dict(a=8.2e-8, dh=3.3e-7),
    "silu_overcap": dict(a=8.3e-8, dh=3.5e-7),
    "silu_sat": dict(a=8.5e-11, dh=2.1e-7),
    "silu_sat100": dict(a=1.1e-8, dh=2.5e-7),
    "silu_odd": dict(a=2.9e-8, dh=4.9e-8),
    "drop_n4": dict(add=4.8e-8, grad=0.0, sd_fwd=4.3e-8, sd_bwd=1.1e-8),
    "drop_p0.1_s0": dict(add=5.7e-8, grad=4.3e-8, sd_fwd=1.3e-7, sd_bwd=3.7e-7),
    "drop_p0.1_smax": dict(add=5.4e-8, grad=4.9e-8, sd_fwd=1.2e-7, sd_bwd=3.1e-7),
    "drop_p0.5_s0": dict(add=3.9e-8, grad=0.0, sd_fwd=7.5e-8, sd_bwd=3.8e-7),
    "drop_p0.5_smax": dict(add=4.0e-8, grad=0.0, sd_fwd=7.7e-8, sd_bwd=3.8e-7),
    "drop_p1e-12_s0": dict(add=4.7e-8, grad=0.0, sd_fwd=8.0e-8, sd_bwd=3.5e-7),
    "drop_p1e-12_smax": dict(add=4.6e-8, grad=0.0, sd_fwd=6.7e-8, sd_bwd=4.3e-7),
    "drop_p0.999_s0": dict(add=6.7e-8, grad=2.8e-8, sd_fwd=8.4e-8, sd_bwd=3.2e-7),
    "drop_p0.999_smax": dict(add=6.7e-8, grad=3.6e-8, sd_fwd=6.0e-8, sd_bwd=4.6e-8),
    "drop_overcap_p0.1": dict(add=5.6e-8, grad=4.5e-8, sd_fwd=1.1e-7, sd_bwd=3.2e-7),
    "drop_overcap_p0.5": dict(add=3.3e-8, grad=0.0, sd_fwd=8.6e-8, sd_bwd=4.3e-7),
    "dropmod_view": dict(out=2.9e-8, grad=3.1e-8),
    "bn_c4": dict(y=1.4e-7, mean=5.4e-8, rstd=5.2e-8, dgamma=1.9e-7, dbeta=1.4e-7, dx=1.9e-7,
                  running_mean=3.0e-8, running_var=4.0e-8, y_eval=1.5e-7),
    "bn_c12": dict(y=1.3e-7, mean=4.6e-8, rstd=9.6e-8, dgamma=1.1e-7, dbeta=1.4e-7, dx=2.2e-7,
                   running_mean=5.0e-8, running_var=6.8e-8, y_eval=1.6e-7),
    "bn_c68": dict(y=2.0e-7, mean=6.2e-8, rstd=1.4e-7, dgamma=2.3e-7, dbeta=9.4e-8, dx=2.0e-7,
                   running_mean=7.1e-8, running_var=6.8e-8, y_eval=1.9e-7),
    "bn_c192": dict(y=1.5e-7, mean=1.2e-7, rstd=1.3e-7, dgamma=1.8e-7, dbeta=1.8e-7, dx=2.3e-7,
                    running_mean=5.2e-8, running_var=7.8e-8, y_eval=1.5e-7),
    "bn_c256": dict(y=1.6e-7, mean=8.2e-8, rstd=1.2e-7, dgamma=2.3e-7, dbeta=1.5e-7, dx=1.8e-7,
                    running_mean=7.4e-8, running_var=8.4e-8, y_eval=1.8e-7),
    "bn_c516": dict(y=1.7e-7, mean=1.1e-7, rstd=1.5e-7, dgamma=1.9e-7, dbeta=1.7e-7, dx=2.1e-7,
                    running_mean=9.3e-8, running_var=8.7e-8, y_eval=2.4e-7),
    "bn_c1024": dict(y=1.9e-7, mean=2.3e-7, rstd=1.4e-7, dgamma=2.1e-7, dbeta=1.3e-7, dx=1.9e-7,
                     running_mean=7.5e-8, running_var=1.1e-7, y_eval=1.6e-7),
    "bn_r257": dict(y=1.7e-7, mean=1.5e-7, rstd=1.5e-7, dgamma=1.8e-7, dbeta=1.6e-7, dx=2.0e-7,
                    running_mean=9.3e-8, running_var=9.2e-8, y_eval=1.2e-7),
    "bn_r2": dict(y=1.2e-7, mean=4.7e-8, rstd=7.2e-8, dgamma=9.3e-8, dbeta=6.0e-8,
                  dx_plus_ds=6.9e-8, running_mean=8.0e-8, running_var=1.1e-7, y_eval=7.7e-8),
    "bn_r7": dict(y=1.6e-7, mean=1.1e-7, rstd=1.8e-7, dgamma=1.6e-7, dbeta=9.9e-8, dx=2.0e-7,
                  running_mean=7.1e-8, running_var=7.9e-8, y_eval=1.4e-7),
    "bn_r127": dict(y=2.0e-7, mean=1.4e-7, rstd=1.3e-7, dgamma=1.3e-7, dbeta=1.8e-7, dx=1.9e-7,
                    running_mean=5.4e-8, running_var=8.7e-8, y_eval=1.7e-7),
    "bn_r128": dict(y=1.9e-7, mean=9.8e-8, rstd=1.4e-7, dgamma=1.6e-7, dbeta=1.3e-7, dx=1.5e-7,
                    running_mean=7.3e-8, running_var=9.0e-8, y_eval=1.8e-7),
    "bn_r129": dict(y=1.6e-7, mean=1.1e-7, rstd=1.3e-7, dgamma=2.3e-7, dbeta=1.4e-7, dx=1.6e-7,
                    running_mean=5.4e-8, running_var=8.1e-8, y_eval=1.9e-7),
    "bn_overcap": dict(y=1.8e-7, mean=1.4e-7, rstd=1.5e-7, dgamma=1.8e-7, dbeta=2.1e-7, dx=2.6e-7,
                       running_mean=5.2e-8, running_var=9.9e-8, y_eval=2.1e-7),
    "bn_mom_none": dict(y=2.1e-7, mean=1.4e-7, rstd=9.9e-8, dgamma=1.5e-7, dbeta=8.4e-8, dx=1.8e-7,
                        running_mean=1.1e-7, running_var=1.1e-7, y_eval=1.2e-7),
    "bn_no_track": dict(y=1.1e-7, mean=1.2e-7, rstd=1.2e-7, dgamma=1.1e-7, dbeta=1.6e-7, dx=2.1e-7,
                        y_eval=1.9e-7),
    "bn_offset8": dict(y=3.8e-7, mean=1.1e-7, rstd=1.4e-7, dgamma=8.7e-7, dbeta=4.2e-7, dx=5.9e-7,
                       running_mean=1.1e-7, running_var=1.3e-7, y_eval=1.7e-7),
    "attn_t1": dict(o=0.0, dqkv=0.0),
    "attn_t31": dict(o=3.2e-7, dq=4.0e-7, dk=2.7e-7, dv=3.5e-7),
    "attn_t32": dict(o=3.0e-7, dq=6.1e-7, dk=4.4e-7, dv=5.5e-7),
    "attn_t33": dict(o=3.1e-7, dq=3.1e-7, dk=3.7e-7, dv=4.2e-7),
    "attn_t63": dict(o=3.6e-7, dq=4.4e-7, dk=4.9e-7, dv=3.6e-7),
    "attn_t64": dict(o=3.4e-7, dq=5.3e-7, dk=4.5e-7, dv=2.8e-7),
    "attn_t65": dict(o=3.0e-7, dq=2.8e-7, dk=5.2e-7, dv=3.1e-7),
    "attn_t127": dict(o=4.4e-7, dq=4.3e-7, dk=6.9e-7, dv=5.9e-7),
    "attn_t128": dict(o=8.4e-7, dq=3.9e-7, dk=6.3e-7, dv=6.2e-7),
    "attn_t129": dict(o=6.3e-7, dq=5.3e-7, dk=3.8e-7, dv=5.3e-7),
    "attn_t200": dict(o=9.0e-7, dq=6.6e-7, dk=6.0e-7, dv=6.1e-7),
    "attn_t300": dict(o=5.8e-7, dq=2.6e-7, dk=5.8e-7, dv=5.3e-7),
    "attn_dh16_t33": dict(o=2.6e-7, dq=3.6e-7, dk=2.3e-7, dv=2.5e-7),
    "attn_dh16_t129": dict(o=4.8e-7, dq=4.8e-7, dk=4.3e-7, dv=3.0e-7),
    "attn_dh64_t33": dict(o=2.7e-7, dq=4.2e-7, dk=3.6e-7, dv=3.6e-7),
    "attn_dh64_t129": dict(o=8.2e-7, dq=7.0e-7, dk=5.4e-7, dv=9.8e-7),
    "attn_len_a": dict(o=3.7e-7, dq=3.5e-7, dk=5.1e-7, dv=6.3e-7),
    "attn_len_b": dict(o=4.6e-7, dq=7.0e-7, dk=5.8e-7, dv=3.3e-7),
    "attn_len_c": dict(o=8.3e-7, dq=7.6e-7, dk=5.4e-7, dv=4.1e-7),
    "attn_peaky": dict(o=2.2e-6, dq=2.7e-6, dk=2.1e-6, dv=7.4e-7),
    "attn_drop_dh16_t33": dict(o=2.3e-7, dq=2.1e-7, dk=2.2e-7, dv=1.4e-7),
    "attn_drop_dh16_t129": dict(o=2.2e-7, dq=2.0e-7, dk=3.1e-7, dv=3.6e-7),
    "attn_drop_dh32_t65": dict(o=5.2e-7, dq=3.1e-7, dk=3.4e-7, dv=4.2e-7),
    "attn_drop_dh32_t200": dict(o=5.0e-7, dq=5.6e-7, dk=5.7e-7, dv=8.7e-7),
    "attn_drop_dh64_t33": dict(o=2.4e-7, dq=2.6e-7, dk=2.4e-7, dv=1.5e-7),
    "attn_drop_dh64_t129": dict(o=5.7e-7, dq=6.5e-7, dk=6.3e-7, dv=5.4e-7),
    "attn_drop_dh64_t200": dict(o=7.3e-7, dq=5.6e-7, dk=4.9e-7, dv=7.9e-7),
    "attn_dh36_len0": dict(o=1.8e-7, dq=2.0e-7, dk=1.4e-7, dv=1.8e-7),
    "lnmod_c6": dict(out=1.2e-7, dx=1.3e-7, dgamma=2.2e-7, dbeta=1.3e-7),
    "lnmod_c1028": dict(out=1.1e-7, dx=1.8e-7, dgamma=1.5e-7, dbeta=1.2e-7),
    "lnmod_noaffine": dict(out=9.6e-8, dx=1.8e-7),
    "lnmod_nobias": dict(out=8.8e-8, dx=1.2e-7, dgamma=1.4e-7),
    "lnmod_strided": dict(out=9.2e-8, dx=1.1e-7, dgamma=8.0e-8, dbeta=1.1e-7),
    "lnmod_misaligned": dict(out=1.5e-7, dx=1.1e-7, dgamma=1.4e-7, dbeta=9.1e-8),
}
