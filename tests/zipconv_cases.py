"""The cases of tests/test_gpu_zip_conv_kernels.py (csrc/zip_conv.hip, csrc/zip_front.hip against the
float64 yardstick tests/zipconv_f64.py) and why each is there.  Test infrastructure, not a test file.

Conv module (group "cm"; tile = 64 frames x 64 channels of one utterance, 16 frames per thread):
  ins_k{3,5,7,15,31}_{plain,edge,chunk}   every K the dispatch knows x the lean / one-chunk-with-scale /
        chunked kernel at (T,B,C) = (70,2,68): two frame tiles (6 frames in the second), two channel
        tiles (4 channels in the second).  K = 3 and 5 stage their taps with 64 K < 256 threads.
  fr_t*          K = 15, C = 64, one chunk with scale: T below the halo, below K, around the 16 frames of
        a thread and the 64 of a tile, three tiles.  fr_interior_*: T = 200, tile 1 is no edge tile, its
        edge arrays are not staged and must not be read.
  ch_c*          T = 40, K = 7, chunk 16: C of 1, 3 (scalar stores), 4, 63, 64, 65, 130 (three tiles).
  ck_k*_c*       chunk = 1 .. 64 at (K,T) = (15,100) and (31,96): sub-block forms 0 / 2 / 4 / 8 / 16,
        chunk < K (sliced scale), chunk == K, K < chunk < 2K, chunk = tile; T % chunk zero and not.
        ck_c128_t200: chunk above the tile.  ck_glu_fold: through glu_chunk_causal_dwconv with
        chunk_size > T, folded to one chunk by the wrapper.
  op_*           operand forms at (40,3,64,15), chunk 8: no gate, a wide row, a gate / row off the
        16-byte rule, u and the outputs off 16 bytes, C % 4 != 0 with the gate quad of the very last row
        crossing the buffer end (no mask, so that row is observed), absent biases / scale / causal conv /
        dscale, an utterance that is all padding, no mask.  Unused words of a wide row hold NaN.
  sp_*           s2t_zipconv_bwd against bwd_data + bwd_params: bit-equal but for dscale (atomics).
  ug_*           S2T_CONV_BLOCKS: several utterances per workgroup, a last group of 1 and of 3.
  red_b*         (T,C,K) = (20,8,3): nblk = B partial blocks through the reduce kernel: tail loop only
        (28), lane group 0 alone in the 8-in-flight loop (29), some (31), all (32, 33), two trips (65);
        red_nt3: nblk = nt gy with nt = 3.
  act_*          s2t_zipconv_fwd_act: y on Swoosh's saturation points (zip_cases.SAT without +-1e4), both
        store forms (C = 64: 16-byte, C = 66: scalar).
  op_2gib        T B ld 4 >= 0x7FFFFF00: the plain-load staging of the forward and the tap-gradient
        kernel and the scalar form of bwd_data.  The buffer is allocated and ~40 KB of it written.  The
        dy_buf == false branch of bwd_data needs a 2 GiB gradient and its float64 reference: left out.
Every case that runs forward + backward (via wrapper / direct) runs a second time on exactly representable
inputs, in its own operand layout: integers in [-4,4], taps / biases / scales in quarters up to 2, and -- so
that the gated cases can take part, not only op_nogate and op_nogate_c6_tail -- a gate pre-activation of 100
everywhere, whose sigmoid is 1.0 in float32 and in float64.  Every float32 sum is then exact in any order
and the device must equal the reference bit for bit (y, du, the tap and bias gradients).

Frontend:
  dw7_* / dw3_*  depthwise conv forward, both flips (RWO = 7 columns, RRT = 30 rows, RCT = 128 channels,
        2 thread groups per workgroup for 7x7; TH = 4 rows, WT = 8 columns for 3x3): W / H / C around
        every one of those, an odd number of thread groups (an idle one), no bias, the addend.
  wg_*           weight gradient; `path` is what wgrad_path() gives from the launch arithmetic (asserted
        on the CPU): ring, roll (MODE 2 fallback), generic; the reduce kernel at nblk = 16 .. 113;
        wg_fix_*: C mod 128 in 1 .. 64, where the unfixed kernels wrote a tile past the workspace.
        wg_ring_tall (600,40,7,128) is the one large case (rrt = 40 > 24).
  c1_*           s2t_conv3x3_c1 modes 0 / 1 / 2: H = 3, W = 1 with pw = 1, fewer than 256 positions (1023
        idle workgroups add zeros), and (17,130,243): 524 416 outputs > 2048 x 256, a second trip.
  s2_*           s2t_conv3x3_s2 modes 0 / 2: odd / even H and W (a last row / column no tap reaches is
        exactly zero), npair > 64.
  c2i_*          col2im at strides (1,1), (2,2), (1,2), W C below and above 256.
Frontend forward / data-gradient cases (dw, c1, s2, c2i) also run on the exact inputs.

Bounds: rel_err = max |got - ref| / max |ref| per tensor <= bound() = max(2e-5, 8 x FP32_COST), the
figure measured on the CPU from the yardstick in float32 against float64 (never from a kernel).  There
is no derived exception: no kernel tensor needed one.
"""
import functools

import torch

import zip_cases as ZC
from yardstick import FLOOR, MARGIN, UNIT, bound_of, rel_err  # noqa: F401  (the rule of tests/yardstick.py)
import zipconv_f64 as ZR

SAT10 = tuple(v for v in ZC.SAT if abs(v) < 1e4)
CASES = {}


def _add(name, group, **kw):
    assert name not in CASES
    CASES[name] = dict(group=group, seed=9000 + len(CASES), **kw)


def _cm(name, T, B, C, K, chunk=None, scale=True, causal=True, bias=True, gate=True, mask="rule",
        ld=None, gate_off=None, u_mis=False, out_mis=False, dscale=True, blocks=None, via="wrapper",
        is_l=None):
    """chunk None: one chunk (T).  ld / gate_off: the device layout of u (the reference reads x | gate)."""
    ld = ld if ld is not None else (2 * C if gate else C)
    gate_off = gate_off if gate_off is not None else (C if gate else -1)
    _add(name, "cm", T=T, B=B, C=C, K=K, chunk=chunk, scale=scale, causal=causal, bias=bias, gate=gate,
         mask=mask, ld=ld, gate_off=gate_off, u_mis=u_mis, out_mis=out_mis, dscale=dscale, blocks=blocks,
         via=via, is_l=is_l)


for _k in (3, 5, 7, 15, 31):
    _cm(f"ins_k{_k}_plain", 70, 2, 68, _k, scale=False, causal=False)
    _cm(f"ins_k{_k}_edge", 70, 2, 68, _k)
    _cm(f"ins_k{_k}_chunk", 70, 2, 68, _k, chunk=16)
for _t in (1, 7, 15, 16, 17, 63, 64, 65, 129):
    _cm(f"fr_t{_t}", _t, 2, 64, 15, via="direct")
_cm("fr_interior_k15", 200, 2, 64, 15, via="direct")
_cm("fr_interior_k31", 200, 2, 64, 31, via="direct")
for _c in (1, 3, 4, 63, 64, 65, 130):
    _cm(f"ch_c{_c}", 40, 2, _c, 7, chunk=16)
for _ch in (1, 2, 3, 4, 8, 12, 15, 16, 32, 64):
    _cm(f"ck_k15_c{_ch}", 100, 2, 64, 15, chunk=_ch)
    _cm(f"ck_k31_c{_ch}", 96, 2, 64, 31, chunk=_ch)
_cm("ck_c128_t200", 200, 2, 64, 15, chunk=128)
_cm("ck_glu_fold", 40, 2, 64, 15, chunk=None, via="glu")
_OP = (40, 3, 64, 15)
_cm("op_nogate", *_OP, chunk=8, gate=False)
_cm("op_wide", *_OP, chunk=8, ld=2 * 64 + 12, gate_off=64 + 8)
_cm("op_gate_odd", *_OP, chunk=8, ld=2 * 64 + 2, gate_off=64 + 1)
_cm("op_ld_odd", *_OP, chunk=8, ld=2 * 64 + 1)
_cm("op_u_mis", *_OP, chunk=8, u_mis=True, via="direct")
_cm("op_out_mis", *_OP, chunk=8, out_mis=True, via="direct")
_cm("op_c66_tail", 40, 3, 66, 15, chunk=8, mask="none")
_cm("op_nogate_c6_tail", 40, 3, 6, 15, chunk=8, gate=False, mask="none")
_cm("op_nobias", *_OP, chunk=8, bias=False)
_cm("op_noscale_chunk", *_OP, chunk=8, scale=False)
_cm("op_nocausal_chunk", *_OP, chunk=8, causal=False)
_cm("op_no_dscale", *_OP, chunk=8, dscale=False)
_cm("op_allpad", *_OP, chunk=8, mask="allpad")
_cm("op_nomask", *_OP, chunk=8, mask="none")
_cm("sp_chunk", 70, 3, 68, 15, chunk=16, via="split")
_cm("sp_plain", 70, 3, 68, 15, scale=False, causal=False, via="split")
_cm("ug_b7", 70, 7, 64, 15, chunk=16, blocks=4)
_cm("ug_b17", 40, 17, 64, 7, chunk=16, blocks=1)
_cm("ug_b35", 40, 35, 64, 7, chunk=16, blocks=1)
for _b in (28, 29, 31, 32, 33, 65):
    _cm(f"red_b{_b}", 20, _b, 8, 3, chunk=8, via="direct")
_cm("red_nt3", 130, 11, 8, 3, chunk=8, via="direct")
for _c in (64, 66):
    _cm(f"act_l_c{_c}", 40, 2, _c, 7, chunk=16, via="act", is_l=True)
    _cm(f"act_r_c{_c}", 40, 2, _c, 7, chunk=16, via="act", is_l=False)
_LD_MIN = -(-0x7FFFFF00 // (40 * 2 * 4))
LD_2GIB = (_LD_MIN + 3) // 4 * 4                # smallest multiple of 4 with T B ld 4 >= 0x7FFFFF00
_cm("op_2gib", 40, 2, 64, 15, chunk=8, ld=LD_2GIB, gate_off=64, via="direct")


def _dw(name, N, H, W, C, K=7, bias=True, add=False):
    _add(name, "dw", N=N, H=H, W=W, C=C, K=K, bias=bias, add=add)


for _w in (1, 6, 7, 8, 15, 19):
    _dw(f"dw7_w{_w}", 2, 9, _w, 128)
for _h in (1, 3, 29, 30, 31, 61):
    _dw(f"dw7_h{_h}", 2, _h, 8, 128)
for _c in (1, 64, 127, 128, 129, 192):
    _dw(f"dw7_c{_c}", 2, 9, 8, _c)
_dw("dw7_groups6", 1, 31, 19, 128)
_dw("dw7_idle_group", 1, 9, 19, 128)
_dw("dw7_nobias", 2, 9, 8, 128, bias=False)
_dw("dw7_add", 2, 31, 15, 129, bias=False, add=True)
for _h in (1, 4, 5):
    _dw(f"dw3_h{_h}", 2, _h, 9, 64, K=3)
for _w in (1, 7, 8, 9, 17):
    _dw(f"dw3_w{_w}", 2, 5, _w, 64, K=3)
for _c in (1, 64, 65):
    _dw(f"dw3_c{_c}", 2, 5, 9, _c, K=3)


def wgrad_path(N, H, W, C, K):
    """What s2t_dwconv2d_nhwc_wgrad launches, from its constants (RWO = 7, RRT = 30, RCT = 128, 2 thread
    groups per workgroup, a workspace of (H + 7) / 8 blocks per (n, 64-channel tile))."""
    nparts, nrr, hb = (W + 6) // 7, (H + 29) // 30, (H + 7) // 8
    if K == 7:
        per_row = nparts * N * ((C + 127) // 128)
        nr = max(1, (512 * 2) // per_row)
        rrt = max(24, (H + nr - 1) // nr)
        nrr2 = (H + rrt - 1) // rrt
        gx = (nparts * nrr2 + 1) // 2
        if gx <= hb:
            return dict(path="ring", gx=gx, nblk=gx * N, nrr=nrr2, rrt=rrt)
        gx = (nparts * nrr + 1) // 2
        if gx <= hb:
            return dict(path="roll", gx=gx, nblk=gx * N)
    rpb = (H * N * ((C + 63) // 64) + 1023) // 1024
    rpb = 8 if rpb < 8 else (rpb + 3) // 4 * 4
    gx = (H + rpb - 1) // rpb
    return dict(path="generic", gx=gx, nblk=gx * N, rows_per_blk=rpb)


def _wg(name, N, H, W, C, path, K=7, db=True):
    _add(name, "wg", N=N, H=H, W=W, C=C, K=K, db=db, path=path)


_wg("wg_ring", 3, 37, 19, 128, "ring")
_wg("wg_ring_nrr3", 2, 61, 19, 128, "ring", db=False)
_wg("wg_ring_c129", 2, 31, 15, 129, "ring")
_wg("wg_ring_tall", 600, 40, 7, 128, "ring")
_wg("wg_roll_w35", 2, 30, 35, 128, "roll")
_wg("wg_roll_w29", 2, 30, 29, 128, "roll", db=False)
_wg("wg_fix_roll_c64", 2, 30, 56, 64, "roll")
_wg("wg_gen_w99", 2, 24, 99, 128, "generic", db=False)
_wg("wg_gen_rows12", 70, 130, 3, 64, "generic", K=3)
for _h in (1, 4, 5):
    _wg(f"wg3_h{_h}", 2, _h, 9, 64, "generic", K=3)
for _w in (1, 7, 8, 9, 17):
    _wg(f"wg3_w{_w}", 2, 5, _w, 64, "generic", K=3)
for _c in (1, 64, 65):
    _wg(f"wg3_c{_c}", 2, 5, 9, _c, "generic", K=3)
for _n in (16, 17, 48, 49, 65, 113):
    _wg(f"wg_red_n{_n}", _n, 8, 7, 128, "ring")
_wg("wg_fix_c64", 1, 8, 7, 64, "ring")
_wg("wg_fix_h37_c64", 1, 37, 19, 64, "ring")
_wg("wg_fix_c1", 2, 16, 7, 1, "ring")
_wg("wg_fix_c192", 2, 9, 8, 192, "ring")

for _n, (_b, _h, _w, _pw) in dict(h3=(2, 3, 9, 0), w1_pw1=(2, 5, 1, 1), small_pw1=(2, 6, 11, 1),
                                  small_pw0=(3, 7, 10, 0), cap=(17, 130, 243, 0)).items():
    _add("c1_" + _n, "c1", B=_b, H=_h, W=_w, pw=_pw)
for _h, _w in ((3, 3), (4, 4), (5, 5), (8, 9), (9, 8), (10, 11), (11, 130), (12, 131)):
    _add(f"s2_{_h}x{_w}", "s2", B=2, H=_h, W=_w)
for _n, (_h, _w, _c, _sh, _sw) in dict(s11=(5, 9, 16, 1, 1), s22=(9, 11, 32, 2, 2), s12=(6, 11, 8, 1, 2),
                                       h3=(3, 7, 8, 1, 1), wide=(7, 40, 32, 2, 2)).items():
    _add("c2i_" + _n, "c2i", B=2, H=_h, W=_w, C=_c, sh=_sh, sw=_sw)

C1_CAP = 2048 * 256                # positions one trip of the conv3x3_c1 forward / data-gradient grid covers
CM_REFUSALS = (dict(K=9), dict(K=4), dict(chunk=0), dict(T=0), dict(B=0), dict(C=0))


def names(group, **flt):
    return [n for n, c in CASES.items() if c["group"] == group and all(c.get(k) == v for k, v in flt.items())]


def has_exact(name):
    c = CASES[name]
    return c["group"] in ("dw", "c1", "s2", "c2i") or (c["group"] == "cm" and c["via"] in ("wrapper", "direct"))


# ------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def make(name, exact=False):
    """The float32 inputs of a case (shared, do not modify).  exact: integers in [-4,4] for data and
    gradients, quarters in [-2,2] for taps, biases and scales, 100 for the gate (sigmoid = 1 exactly)."""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"] + (100000 if exact else 0))

    def rn(*s, k=1.0):
        if exact:
            return torch.randint(-4, 5, s, generator=g).float()
        return torch.randn(*s, generator=g) * k

    def rw(*s, k=1.0):
        if exact:
            return torch.randint(-8, 9, s, generator=g).float() / 4
        return torch.randn(*s, generator=g) * k

    grp = c["group"]
    if grp == "cm":
        T, B, C, K = c["T"], c["B"], c["C"], c["K"]
        Kh = (K + 1) // 2
        x = rn(T, B, C)
        gate = (torch.full((T, B, C), 100.0) if exact else rn(T, B, C)) if c["gate"] else None
        t = dict(x=x, gate=gate, dy=rn(T, B, C),
                 wc=rw(C, Kh, k=K ** -0.5) if c["causal"] else None,
                 bc=rw(C, k=0.1) if c["causal"] and c["bias"] else None,
                 wk=rw(C, K, k=K ** -0.5), bk=rw(C, k=0.1) if c["bias"] else None,
                 scale=rw(2, C, K, k=0.3) if c["scale"] else None)
        if c["mask"] == "none":
            t["mask"] = None
        else:
            lens = torch.randint(T // 2, T + 1, (B,), generator=g)
            lens[0] = T
            if c["mask"] == "allpad":
                lens[1] = 0
            t["mask"] = torch.arange(T).unsqueeze(0) >= lens.unsqueeze(1)
        if c["via"] == "act":
            n = len(SAT10)
            t["x"][..., :n] *= 0.01
            t["bk"][:n] = torch.tensor(SAT10)
            t["bc"][:n] = 0.0
        for k, shape in (("dwc", (C, Kh)), ("dbc", (C,)), ("dwk", (C, K)), ("dbk", (C,)), ("dscale", (2, C, K))):
            t["pre_" + k] = torch.randn(*shape, generator=g)
        return t
    if grp == "dw":
        N, H, W, C, K = c["N"], c["H"], c["W"], c["C"], c["K"]
        return dict(x=rn(N, H, W, C), w=rw(C, K, K, k=1.0 / K), bias=rw(C, k=0.1) if c["bias"] else None,
                    add=rn(N, H, W, C) if c["add"] else None)
    if grp == "wg":
        N, H, W, C = c["N"], c["H"], c["W"], c["C"]
        return dict(x=rn(N, H, W, C), dy=rn(N, H, W, C))
    if grp == "c1":
        B, H, W, pw = c["B"], c["H"], c["W"], c["pw"]
        return dict(x=rn(B, H, W), w=rw(8, 1, 3, 3, k=1 / 3), bias=rw(8, k=0.1), g=rn(B, H - 2, W + 2 * pw - 2, 8),
                    pre_dw=torch.randn(72, generator=g), pre_db=torch.randn(8, generator=g))
    if grp == "s2":
        B, H, W = c["B"], c["H"], c["W"]
        return dict(x=rn(B, H, W, 8), w=rw(32, 8, 3, 3, k=72 ** -0.5), bias=rw(32, k=0.1),
                    g=rn(B, (H - 3) // 2 + 1, (W - 3) // 2 + 1, 32))
    if grp == "c2i":
        B, H, W, C, sh, sw = (c[k] for k in ("B", "H", "W", "C", "sh", "sw"))
        return dict(dc=rn(B, (H - 3) // sh + 1, (W - 3) // sw + 1, 3, 3, C))
    raise KeyError(grp)


# ------------------------------------------------------------------ the yardstick on a case
def _leaf(v, dt):
    return None if v is None else v.to(dt).clone().requires_grad_(True)


def _eval_cm(c, t, dt):
    T, C, K = c["T"], c["C"], c["K"]
    u = _leaf(torch.cat((t["x"], t["gate"]), -1) if c["gate"] else t["x"], dt)
    p = {k: _leaf(t[k], dt) for k in ("wc", "bc", "wk", "bk", "scale")}
    y = ZR.conv_module_ref(u, C, C if c["gate"] else -1, t["mask"], c["chunk"] or T, K, p["wc"], p["bc"],
                           p["wk"], p["bk"], p["scale"])
    if c["via"] == "act":
        return dict(y=y.detach(), y_act=ZR.swoosh_ref(y.detach(), c["is_l"]))
    (y * t["dy"].to(dt)).sum().backward()
    out = dict(y=y.detach(), du=u.grad, dwk=p["wk"].grad)
    for k, v in (("dwc", p["wc"]), ("dbc", p["bc"]), ("dbk", p["bk"])):
        if v is not None:
            out[k] = v.grad
    if c["scale"] and c["dscale"]:
        out["dscale"] = p["scale"].grad
    return out


def _eval_dw(c, t, dt):
    x, w = t["x"].to(dt), t["w"].to(dt)
    b, a = (None if t[k] is None else t[k].to(dt) for k in ("bias", "add"))
    return dict(y0=ZR.dwconv2d_ref(x, w, b, False, a), y1=ZR.dwconv2d_ref(x, w, b, True, a))


def _eval_wg(c, t, dt):
    dw, db = ZR.dwconv2d_wgrad_ref(t["x"].to(dt), t["dy"].to(dt), c["K"], c["K"])
    return dict(dw=dw, db=db) if c["db"] else dict(dw=dw)


def _eval_c1(c, t, dt):
    x, w, b = _leaf(t["x"], dt), _leaf(t["w"], dt), _leaf(t["bias"], dt)
    y = ZR.conv3x3_c1_ref(x, w, b, c["pw"])
    (y * t["g"].to(dt)).sum().backward()
    return dict(y=y.detach(), dw=w.grad.reshape(72), db=b.grad, dx=x.grad)


def _eval_s2(c, t, dt):
    x = _leaf(t["x"], dt)
    y = ZR.conv3x3_s2_ref(x, t["w"].to(dt), t["bias"].to(dt))
    (y * t["g"].to(dt)).sum().backward()
    return dict(y=y.detach(), dx=x.grad)


def _eval_c2i(c, t, dt):
    return dict(dx=ZR.col2im3x3_ref(t["dc"].to(dt), c["H"], c["W"], c["sh"], c["sw"]))


def evaluate(name, dtype, exact=False):
    """The yardstick, forward and backward, on the case's inputs cast to `dtype` -> {tensor: value}."""
    c = CASES[name]
    return globals()["_eval_" + c["group"]](c, make(name, exact), dtype)


@functools.lru_cache(maxsize=None)
def reference(name, exact=False):
    """The float64 results of a case, computed once per process and shared (do not modify)."""
    return evaluate(name, torch.float64, exact)


EXACT_TENSORS = ("y", "du", "dwc", "dbc", "dwk", "dbk", "y0", "y1", "dx")     # not dscale, not c1's dw / db
# cases whose float32 and float64 references differ on the exact inputs (test_zipconv_f64.py): none
EXACT_DROPPED = ()


def fp32_figures(name):
    """{tensor: rel_err of the float32 CPU evaluation of the yardstick against float64}."""
    ref, f32 = reference(name), evaluate(name, torch.float32)
    return {k: rel_err(f32[k], ref[k]) for k in ref}


def bound(name, tensor):
    """Allowed rel_err of device tensor `tensor` of case `name`: max(2e-5, 8 x the float32 figure)."""
    return bound_of(FP32_COST[name][tensor])


# ------------------------------------------------------------------ measured cost of fp32
# fp32_figures(name), rounded up to two digits; tests/test_zipconv_f64.py checks them to a factor 4
# both ways after raising both to UNIT (see tests/zip_cases.py).
FP32_COST = {
    "ins_k3_plain": dict(y=1.1e-7, du=9.3e-8, dwk=1.4e-7, dbk=1.2e-7),
    "ins_k3_edge": dict(y=7.7e-8, du=1.4e-7, dwk=1.1e-7, dwc=1.3e-7, dbc=9.1e-8, dbk=1.0e-7, dscale=3.5e-8),
    "ins_k3_chunk": dict(y=1.1e-7, du=1.5e-7, dwk=1.4e-7, dwc=1.8e-7, dbc=9.0e-8, dbk=1.2e-7, dscale=1.1e-7),
    "ins_k5_plain": dict(y=1.4e-7, du=1.6e-7, dwk=1.5e-7, dbk=1.2e-7),
    "ins_k5_edge": dict(y=1.3e-7, du=1.3e-7, dwk=1.2e-7, dwc=1.3e-7, dbc=1.1e-7, dbk=9.1e-8, dscale=6.4e-8),
    "ins_k5_chunk": dict(y=7.8e-8, du=9.8e-8, dwk=1.6e-7, dwc=1.5e-7, dbc=9.2e-8, dbk=1.3e-7, dscale=1.5e-7),
    "ins_k7_plain": dict(y=1.2e-7, du=1.1e-7, dwk=1.4e-7, dbk=1.3e-7),
    "ins_k7_edge": dict(y=1.5e-7, du=1.4e-7, dwk=1.6e-7, dwc=1.6e-7, dbc=9.2e-8, dbk=4.6e-8, dscale=8.0e-8),
    "ins_k7_chunk": dict(y=1.2e-7, du=1.2e-7, dwk=1.6e-7, dwc=8.7e-8, dbc=1.2e-7, dbk=9.5e-8, dscale=1.2e-7),
    "ins_k15_plain": dict(y=1.5e-7, du=1.8e-7, dwk=1.3e-7, dbk=1.2e-7),
    "ins_k15_edge": dict(y=1.4e-7, du=1.6e-7, dwk=1.5e-7, dwc=1.1e-7, dbc=7.6e-8, dbk=9.9e-8, dscale=1.4e-7),
    "ins_k15_chunk": dict(y=2.2e-7, du=1.2e-7, dwk=1.6e-7, dwc=1.4e-7, dbc=1.6e-7, dbk=1.2e-7, dscale=1.4e-7),
    "ins_k31_plain": dict(y=2.1e-7, du=1.7e-7, dwk=1.4e-7, dbk=9.7e-8),
    "ins_k31_edge": dict(y=1.1e-7, du=1.5e-7, dwk=1.3e-7, dwc=1.2e-7, dbc=1.2e-7, dbk=1.1e-7, dscale=1.4e-7),
    "ins_k31_chunk": dict(y=1.8e-7, du=1.3e-7, dwk=1.7e-7, dwc=1.1e-7, dbc=2.4e-7, dbk=1.7e-7, dscale=9.5e-8),
    "fr_t1": dict(y=6.1e-8, du=5.8e-8, dwk=1.6e-7, dwc=4.5e-8, dbc=3.2e-8, dbk=1.1e-7, dscale=7.2e-8),
    "fr_t7": dict(y=1.2e-7, du=9.6e-8, dwk=8.8e-8, dwc=9.1e-8, dbc=6.7e-8, dbk=6.7e-8, dscale=1.2e-7),
    "fr_t15": dict(y=1.3e-7, du=1.2e-7, dwk=1.5e-7, dwc=1.3e-7, dbc=7.5e-8, dbk=8.6e-8, dscale=1.4e-7),
    "fr_t16": dict(y=2.0e-7, du=1.1e-7, dwk=1.2e-7, dwc=1.5e-7, dbc=1.0e-7, dbk=9.5e-8, dscale=1.2e-7),
    "fr_t17": dict(y=1.2e-7, du=1.3e-7, dwk=1.3e-7, dwc=1.3e-7, dbc=5.9e-8, dbk=9.4e-8, dscale=8.8e-8),
    "fr_t63": dict(y=1.1e-7, du=1.2e-7, dwk=1.5e-7, dwc=1.2e-7, dbc=8.5e-8, dbk=9.3e-8, dscale=1.3e-7),
    "fr_t64": dict(y=1.4e-7, du=2.1e-7, dwk=1.3e-7, dwc=1.5e-7, dbc=1.3e-7, dbk=1.1e-7, dscale=1.6e-7),
    "fr_t65": dict(y=1.5e-7, du=1.1e-7, dwk=1.7e-7, dwc=1.5e-7, dbc=8.6e-8, dbk=9.8e-8, dscale=1.6e-7),
    "fr_t129": dict(y=1.7e-7, du=1.4e-7, dwk=2.3e-7, dwc=1.4e-7, dbc=1.1e-7, dbk=1.3e-7, dscale=9.6e-8),
    "fr_interior_k15": dict(y=1.6e-7, du=1.8e-7, dwk=1.1e-7, dwc=1.5e-7, dbc=1.1e-7, dbk=1.2e-7, dscale=8.4e-8),
    "fr_interior_k31": dict(y=2.2e-7, du=1.3e-7, dwk=1.2e-7, dwc=1.1e-7, dbc=1.7e-7, dbk=1.3e-7, dscale=1.4e-7),
    "ch_c1": dict(y=1.3e-7, du=9.3e-8, dwk=1.3e-7, dwc=2.0e-7, dbc=7.9e-8, dbk=1.7e-7, dscale=1.4e-7),
    "ch_c3": dict(y=1.1e-7, du=6.8e-8, dwk=2.1e-7, dwc=2.5e-7, dbc=7.3e-8, dbk=1.2e-7, dscale=6.8e-8),
    "ch_c4": dict(y=7.0e-8, du=1.2e-7, dwk=2.0e-7, dwc=1.7e-7, dbc=9.4e-8, dbk=1.9e-7, dscale=5.9e-8),
    "ch_c63": dict(y=1.1e-7, du=1.3e-7, dwk=7.6e-8, dwc=1.3e-7, dbc=9.0e-8, dbk=1.5e-7, dscale=1.5e-7),
    "ch_c64": dict(y=1.2e-7, du=1.3e-7, dwk=1.1e-7, dwc=1.1e-7, dbc=1.5e-7, dbk=1.1e-7, dscale=1.6e-7),
    "ch_c65": dict(y=1.6e-7, du=1.3e-7, dwk=1.2e-7, dwc=9.8e-8, dbc=8.3e-8, dbk=9.3e-8, dscale=1.0e-7),
    "ch_c130": dict(y=1.5e-7, du=1.7e-7, dwk=1.9e-7, dwc=1.9e-7, dbc=1.1e-7, dbk=1.1e-7, dscale=1.8e-7),
    "ck_k15_c1": dict(y=1.2e-7, du=1.7e-7, dwk=1.8e-7, dwc=1.2e-7, dbc=1.3e-7, dbk=1.6e-7, dscale=1.4e-7),
    "ck_k31_c1": dict(y=1.2e-7, du=1.7e-7, dwk=9.2e-8, dwc=1.3e-7, dbc=1.8e-7, dbk=1.5e-7, dscale=1.3e-7),
    "ck_k15_c2": dict(y=1.5e-7, du=1.8e-7, dwk=8.5e-8, dwc=1.2e-7, dbc=8.8e-8, dbk=1.9e-7, dscale=1.8e-7),
    "ck_k31_c2": dict(y=1.7e-7, du=1.8e-7, dwk=1.2e-7, dwc=1.4e-7, dbc=1.4e-7, dbk=1.2e-7, dscale=2.1e-7),
    "ck_k15_c3": dict(y=1.0e-7, du=1.1e-7, dwk=2.0e-7, dwc=1.3e-7, dbc=7.9e-8, dbk=8.3e-8, dscale=1.7e-7),
    "ck_k31_c3": dict(y=1.5e-7, du=2.1e-7, dwk=2.0e-7, dwc=1.5e-7, dbc=1.1e-7, dbk=1.4e-7, dscale=1.9e-7),
    "ck_k15_c4": dict(y=1.8e-7, du=1.2e-7, dwk=1.6e-7, dwc=2.2e-7, dbc=1.2e-7, dbk=1.4e-7, dscale=1.1e-7),
    "ck_k31_c4": dict(y=1.6e-7, du=1.5e-7, dwk=1.4e-7, dwc=1.7e-7, dbc=9.1e-8, dbk=9.5e-8, dscale=1.1e-7),
    "ck_k15_c8": dict(y=1.1e-7, du=1.3e-7, dwk=1.9e-7, dwc=1.6e-7, dbc=1.4e-7, dbk=1.5e-7, dscale=1.1e-7),
    "ck_k31_c8": dict(y=1.1e-7, du=1.5e-7, dwk=1.9e-7, dwc=1.4e-7, dbc=1.5e-7, dbk=1.2e-7, dscale=7.4e-8),
    "ck_k15_c12": dict(y=1.1e-7, du=1.4e-7, dwk=2.7e-7, dwc=1.4e-7, dbc=1.5e-7, dbk=8.4e-8, dscale=1.4e-7),
    "ck_k31_c12": dict(y=1.7e-7, du=1.5e-7, dwk=2.5e-7, dwc=1.2e-7, dbc=1.1e-7, dbk=1.6e-7, dscale=1.4e-7),
    "ck_k15_c15": dict(y=1.5e-7, du=1.3e-7, dwk=1.0e-7, dwc=1.7e-7, dbc=1.4e-7, dbk=1.9e-7, dscale=1.2e-7),
    "ck_k31_c15": dict(y=1.6e-7, du=1.5e-7, dwk=1.3e-7, dwc=1.5e-7, dbc=1.2e-7, dbk=1.4e-7, dscale=1.6e-7),
    "ck_k15_c16": dict(y=1.6e-7, du=1.4e-7, dwk=1.3e-7, dwc=1.6e-7, dbc=1.4e-7, dbk=1.3e-7, dscale=9.2e-8),
    "ck_k31_c16": dict(y=1.5e-7, du=9.1e-8, dwk=1.3e-7, dwc=1.3e-7, dbc=1.0e-7, dbk=1.5e-7, dscale=1.7e-7),
    "ck_k15_c32": dict(y=1.3e-7, du=1.2e-7, dwk=1.9e-7, dwc=2.0e-7, dbc=8.5e-8, dbk=9.8e-8, dscale=1.3e-7),
    "ck_k31_c32": dict(y=1.6e-7, du=1.7e-7, dwk=1.2e-7, dwc=1.2e-7, dbc=8.3e-8, dbk=6.9e-8, dscale=1.2e-7),
    "ck_k15_c64": dict(y=1.2e-7, du=1.5e-7, dwk=1.8e-7, dwc=1.4e-7, dbc=9.0e-8, dbk=1.1e-7, dscale=2.1e-7),
    "ck_k31_c64": dict(y=2.0e-7, du=2.0e-7, dwk=1.4e-7, dwc=1.3e-7, dbc=9.4e-8, dbk=1.3e-7, dscale=2.1e-7),
    "ck_c128_t200": dict(y=1.4e-7, du=1.5e-7, dwk=1.8e-7, dwc=1.7e-7, dbc=1.1e-7, dbk=1.4e-7, dscale=1.1e-7),
    "ck_glu_fold": dict(y=1.7e-7, du=1.1e-7, dwk=1.4e-7, dwc=1.3e-7, dbc=1.6e-7, dbk=1.4e-7, dscale=1.4e-7),
    "op_nogate": dict(y=1.4e-7, du=1.1e-7, dwk=9.1e-8, dwc=1.5e-7, dbc=1.1e-7, dbk=1.0e-7, dscale=1.2e-7),
    "op_wide": dict(y=9.3e-8, du=2.2e-7, dwk=2.0e-7, dwc=1.8e-7, dbc=8.0e-8, dbk=8.8e-8, dscale=8.5e-8),
    "op_gate_odd": dict(y=1.4e-7, du=1.2e-7, dwk=1.3e-7, dwc=1.3e-7, dbc=7.7e-8, dbk=9.9e-8, dscale=8.5e-8),
    "op_ld_odd": dict(y=2.1e-7, du=1.2e-7, dwk=2.0e-7, dwc=1.4e-7, dbc=1.3e-7, dbk=1.6e-7, dscale=1.9e-7),
    "op_u_mis": dict(y=7.6e-8, du=1.8e-7, dwk=9.9e-8, dwc=1.2e-7, dbc=1.3e-7, dbk=9.4e-8, dscale=1.2e-7),
    "op_out_mis": dict(y=1.2e-7, du=1.1e-7, dwk=1.7e-7, dwc=1.1e-7, dbc=8.6e-8, dbk=1.5e-7, dscale=8.9e-8),
    "op_c66_tail": dict(y=1.1e-7, du=1.6e-7, dwk=9.2e-8, dwc=1.6e-7, dbc=9.1e-8, dbk=6.2e-8, dscale=9.8e-8),
    "op_nogate_c6_tail": dict(y=1.4e-7, du=9.1e-8, dwk=1.3e-7, dwc=7.7e-8, dbc=1.1e-7, dbk=1.5e-7, dscale=8.9e-8),
    "op_nobias": dict(y=1.6e-7, du=1.1e-7, dwk=1.3e-7, dwc=1.5e-7, dscale=1.1e-7),
    "op_noscale_chunk": dict(y=1.6e-7, du=9.8e-8, dwk=1.3e-7, dwc=1.3e-7, dbc=1.7e-7, dbk=1.7e-7),
    "op_nocausal_chunk": dict(y=1.4e-7, du=1.1e-7, dwk=1.2e-7, dbk=8.9e-8, dscale=1.6e-7),
    "op_no_dscale": dict(y=1.2e-7, du=1.1e-7, dwk=1.3e-7, dwc=1.1e-7, dbc=1.6e-7, dbk=9.2e-8),
    "op_allpad": dict(y=1.3e-7, du=1.4e-7, dwk=1.6e-7, dwc=1.5e-7, dbc=9.4e-8, dbk=1.2e-7, dscale=1.1e-7),
    "op_nomask": dict(y=1.5e-7, du=1.2e-7, dwk=1.2e-7, dwc=1.5e-7, dbc=1.2e-7, dbk=1.8e-7, dscale=6.7e-8),
    "sp_chunk": dict(y=1.1e-7, du=1.6e-7, dwk=1.2e-7, dwc=1.4e-7, dbc=1.5e-7, dbk=1.5e-7, dscale=1.4e-7),
    "sp_plain": dict(y=1.7e-7, du=1.2e-7, dwk=1.4e-7, dbk=1.7e-7),
    "ug_b7": dict(y=1.2e-7, du=1.2e-7, dwk=1.8e-7, dwc=2.0e-7, dbc=1.3e-7, dbk=1.1e-7, dscale=1.7e-7),
    "ug_b17": dict(y=1.1e-7, du=1.1e-7, dwk=2.1e-7, dwc=1.4e-7, dbc=1.1e-7, dbk=1.1e-7, dscale=1.4e-7),
    "ug_b35": dict(y=1.3e-7, du=1.3e-7, dwk=2.2e-7, dwc=1.9e-7, dbc=1.2e-7, dbk=9.9e-8, dscale=1.4e-7),
    "red_b28": dict(y=8.4e-8, du=1.1e-7, dwk=1.2e-7, dwc=8.2e-8, dbc=1.4e-7, dbk=2.0e-7, dscale=3.5e-8),
    "red_b29": dict(y=7.6e-8, du=8.0e-8, dwk=1.1e-7, dwc=1.3e-7, dbc=8.5e-8, dbk=1.5e-7, dscale=8.3e-8),
    "red_b31": dict(y=1.1e-7, du=5.9e-8, dwk=1.2e-7, dwc=1.3e-7, dbc=9.7e-8, dbk=1.1e-7, dscale=1.0e-7),
    "red_b32": dict(y=9.9e-8, du=1.3e-7, dwk=1.3e-7, dwc=1.5e-7, dbc=1.3e-7, dbk=1.4e-7, dscale=1.7e-7),
    "red_b33": dict(y=1.1e-7, du=1.2e-7, dwk=1.9e-7, dwc=1.3e-7, dbc=1.6e-7, dbk=8.2e-8, dscale=1.2e-7),
    "red_b65": dict(y=1.1e-7, du=1.2e-7, dwk=1.3e-7, dwc=1.2e-7, dbc=1.2e-7, dbk=1.8e-7, dscale=1.2e-7),
    "red_nt3": dict(y=8.8e-8, du=1.2e-7, dwk=1.9e-7, dwc=1.2e-7, dbc=8.4e-8, dbk=7.8e-8, dscale=1.1e-7),
    "act_l_c64": dict(y=1.1e-7, y_act=1.3e-7),
    "act_r_c64": dict(y=1.3e-7, y_act=1.7e-7),
    "act_l_c66": dict(y=1.1e-7, y_act=1.3e-7),
    "act_r_c66": dict(y=1.7e-7, y_act=1.1e-7),
    "op_2gib": dict(y=1.5e-7, du=7.0e-8, dwk=1.3e-7, dwc=1.2e-7, dbc=8.4e-8, dbk=1.2e-7, dscale=1.1e-7),
    "dw7_w1": dict(y0=1.3e-7, y1=1.1e-7),
    "dw7_w6": dict(y0=1.7e-7, y1=2.1e-7),
    "dw7_w7": dict(y0=2.4e-7, y1=3.9e-7),
    "dw7_w8": dict(y0=2.2e-7, y1=2.8e-7),
    "dw7_w15": dict(y0=1.9e-7, y1=2.2e-7),
    "dw7_w19": dict(y0=2.6e-7, y1=2.8e-7),
    "dw7_h1": dict(y0=1.1e-7, y1=1.6e-7),
    "dw7_h3": dict(y0=1.4e-7, y1=1.2e-7),
    "dw7_h29": dict(y0=3.2e-7, y1=2.7e-7),
    "dw7_h30": dict(y0=2.7e-7, y1=2.7e-7),
    "dw7_h31": dict(y0=2.7e-7, y1=2.3e-7),
    "dw7_h61": dict(y0=2.5e-7, y1=2.7e-7),
    "dw7_c1": dict(y0=9.9e-8, y1=1.4e-7),
    "dw7_c64": dict(y0=2.3e-7, y1=2.3e-7),
    "dw7_c127": dict(y0=2.5e-7, y1=1.8e-7),
    "dw7_c128": dict(y0=2.7e-7, y1=2.8e-7),
    "dw7_c129": dict(y0=2.7e-7, y1=2.5e-7),
    "dw7_c192": dict(y0=2.6e-7, y1=2.3e-7),
    "dw7_groups6": dict(y0=2.9e-7, y1=2.5e-7),
    "dw7_idle_group": dict(y0=2.4e-7, y1=2.0e-7),
    "dw7_nobias": dict(y0=1.9e-7, y1=2.1e-7),
    "dw7_add": dict(y0=1.9e-7, y1=2.3e-7),
    "dw3_h1": dict(y0=7.5e-8, y1=5.5e-8),
    "dw3_h4": dict(y0=8.9e-8, y1=7.6e-8),
    "dw3_h5": dict(y0=1.2e-7, y1=1.1e-7),
    "dw3_w1": dict(y0=6.6e-8, y1=4.9e-8),
    "dw3_w7": dict(y0=8.9e-8, y1=1.1e-7),
    "dw3_w8": dict(y0=1.1e-7, y1=1.3e-7),
    "dw3_w9": dict(y0=1.2e-7, y1=1.3e-7),
    "dw3_w17": dict(y0=1.4e-7, y1=1.1e-7),
    "dw3_c1": dict(y0=8.6e-8, y1=8.0e-8),
    "dw3_c64": dict(y0=1.3e-7, y1=1.7e-7),
    "dw3_c65": dict(y0=1.1e-7, y1=1.3e-7),
    "wg_ring": dict(dw=1.6e-7, db=1.1e-7),
    "wg_ring_nrr3": dict(dw=1.4e-7),
    "wg_ring_c129": dict(dw=1.5e-7, db=1.3e-7),
    "wg_ring_tall": dict(dw=2.4e-7, db=1.9e-7),
    "wg_roll_w35": dict(dw=1.6e-7, db=1.4e-7),
    "wg_roll_w29": dict(dw=1.0e-7),
    "wg_fix_roll_c64": dict(dw=1.9e-7, db=9.8e-8),
    "wg_gen_w99": dict(dw=1.6e-7),
    "wg_gen_rows12": dict(dw=2.0e-7, db=1.3e-7),
    "wg3_h1": dict(dw=8.6e-8, db=8.1e-8),
    "wg3_h4": dict(dw=2.1e-7, db=8.8e-8),
    "wg3_h5": dict(dw=1.4e-7, db=1.6e-7),
    "wg3_w1": dict(dw=7.8e-8, db=4.6e-8),
    "wg3_w7": dict(dw=9.5e-8, db=7.8e-8),
    "wg3_w8": dict(dw=1.6e-7, db=1.1e-7),
    "wg3_w9": dict(dw=9.8e-8, db=5.8e-8),
    "wg3_w17": dict(dw=1.5e-7, db=1.3e-7),
    "wg3_c1": dict(dw=7.1e-8, db=9.5e-8),
    "wg3_c64": dict(dw=9.3e-8, db=9.1e-8),
    "wg3_c65": dict(dw=1.5e-7, db=1.2e-7),
    "wg_red_n16": dict(dw=1.2e-7, db=1.2e-7),
    "wg_red_n17": dict(dw=1.2e-7, db=1.2e-7),
    "wg_red_n48": dict(dw=1.4e-7, db=1.5e-7),
    "wg_red_n49": dict(dw=1.4e-7, db=1.3e-7),
    "wg_red_n65": dict(dw=1.5e-7, db=2.2e-7),
    "wg_red_n113": dict(dw=1.2e-7, db=1.7e-7),
    "wg_fix_c64": dict(dw=1.2e-7, db=9.5e-8),
    "wg_fix_h37_c64": dict(dw=1.5e-7, db=1.3e-7),
    "wg_fix_c1": dict(dw=1.1e-7, db=1.9e-7),
    "wg_fix_c192": dict(dw=1.1e-7, db=9.9e-8),
    "c1_h3": dict(y=1.8e-7, dw=7.6e-8, db=5.4e-8, dx=6.5e-8),
    "c1_w1_pw1": dict(y=5.5e-8, dw=1.4e-7, db=8.0e-8, dx=7.0e-8),
    "c1_small_pw1": dict(y=1.1e-7, dw=7.7e-8, db=1.1e-7, dx=8.4e-8),
    "c1_small_pw0": dict(y=6.6e-8, dw=8.2e-8, db=6.8e-8, dx=8.7e-8),
    "c1_cap": dict(y=2.6e-7, dw=2.5e-7, db=2.7e-7, dx=1.6e-7),
    "s2_3x3": dict(y=9.3e-8, dx=1.3e-7),
    "s2_4x4": dict(y=7.9e-8, dx=1.2e-7),
    "s2_5x5": dict(y=9.7e-8, dx=1.1e-7),
    "s2_8x9": dict(y=1.3e-7, dx=1.5e-7),
    "s2_9x8": dict(y=1.6e-7, dx=1.5e-7),
    "s2_10x11": dict(y=1.1e-7, dx=1.4e-7),
    "s2_11x130": dict(y=1.5e-7, dx=1.6e-7),
    "s2_12x131": dict(y=1.6e-7, dx=2.1e-7),
    "c2i_s11": dict(dx=8.4e-8),
    "c2i_s22": dict(dx=5.4e-8),
    "c2i_s12": dict(dx=9.0e-8),
    "c2i_h3": dict(dx=5.4e-8),
    "c2i_wide": dict(dx=6.8e-8),
}
