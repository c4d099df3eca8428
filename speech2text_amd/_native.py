"""ctypes binding of libs2t_mi355.so (the C ABI declared in include/s2t_mi355.h).

There is no fallback: if the shared library is missing, or a tensor handed to a
kernel is not a contiguous device tensor of the declared dtype, this raises.
"""
import ctypes
import functools
import keyword
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libs2t_mi355.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "s2t_mi355.h")
_lib = None

_CT = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float,
       "double": ctypes.c_double, "void*": ctypes.c_void_p}


def parse_header(path=HEADER_PATH):
    """Returns {name: (restype, [argtypes])} for every prototype in the header."""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    protos = {}
    for m in re.finditer(r"\b(int|long|void\*)\s+(s2t_\w+)\s*\(([^)]*)\)\s*;", txt):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        ats = []
        for a in args.split(","):
            a = a.strip()
            if not a or a == "void":
                continue
            if "*" in a:
                ats.append(ctypes.c_void_p)
            else:
                ats.append(_CT[a.split()[-2] if len(a.split()) > 1 else a])
        protos[name] = (_CT[ret], ats)
    return protos


_FIELD_CT = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float,
             "double": ctypes.c_double, "unsigned": ctypes.c_uint}
_DECL = r"(\**)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?"


def parse_abi(txt):
    """-> ({S2T_NAME: int} for every plain-integer #define, {S2tName: ctypes.Structure class} for every
    `typedef struct { ... } S2tName;`) of a header's text.  Pointers of any pointee are c_void_p, as in
    the prototypes; a field named like a Python keyword gets a trailing underscore.  A field this does
    not understand raises ValueError: a layout is never guessed."""
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    consts = {m.group(1): int(m.group(2))
              for m in re.finditer(r"^[ \t]*#define[ \t]+(S2T_\w+)[ \t]+(\d+)[ \t]*$", txt, re.M)}
    structs = {}
    for m in re.finditer(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", txt):
        sname, fields = m.group(2), []
        for stmt in filter(None, (s.strip() for s in m.group(1).split(";"))):
            first, *rest = stmt.split(",")
            head = re.fullmatch(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\b\s*" + _DECL, first.strip())
            decls = [re.fullmatch(_DECL, r.strip()) for r in rest]
            if head is None or None in decls:
                raise ValueError(f"{sname}: cannot parse the field declaration {stmt!r}")
            base = head.group(1)
            for stars, name, dim in [head.groups()[1:]] + [d.groups() for d in decls]:
                ct = ctypes.c_void_p if stars else _FIELD_CT.get(base) or structs.get(base)
                if ct is None:
                    raise ValueError(f"{sname}: unknown type {base!r} in {stmt!r}")
                if dim is not None:
                    if not dim.isdigit() and dim not in consts:
                        raise ValueError(f"{sname}: undefined array dimension {dim!r} in {stmt!r}")
                    ct = ct * (int(dim) if dim.isdigit() else consts[dim])
                fields.append((name + "_" if keyword.iskeyword(name) else name, ct))
        structs[sname] = type(sname, (ctypes.Structure,), {"_fields_": fields})
    return consts, structs


@functools.lru_cache(maxsize=None)
def _abi():
    return parse_abi(open(HEADER_PATH).read())


def struct(name):
    """The ctypes.Structure class of a struct of include/s2t_mi355.h, laid out from the header."""
    return _abi()[1][name]


def const(name):
    """The value of a plain-integer #define of include/s2t_mi355.h."""
    return _abi()[0][name]


class _Prof:
    target = None        # None | "*" (every entry point) | one C entry-point name
    events = {}          # entry -> [(start, stop)] HIP events on the launch stream
    algo_bytes = {}      # entry -> algorithmic bytes reported by the call sites
    algo_flops = {}
    every = 1            # bracket every n-th launch of the target only (an entry launched hundreds
    count = {}           # of times per step would otherwise pay two event records per launch)


_NO_LAUNCH = ("s2t_side_stream", "s2t_stream_order", "s2t_balancer_next_parity", "s2t_gemm_arith",
              "s2t_gemm_arith_of", "s2t_gemm_class_set", "s2t_gemm_arith_set",
              "s2t_zip_layer_info", "s2t_zip_layer_error", "s2t_zip_layer_plans_missing", "s2t_zl_plan_put",
              "s2t_zl_plan_choose", "s2t_ctc_align_form", "s2t_rnnt_align_form")   # stream plumbing, nothing to time
SELF_NOTING = ("s2t_gemm_x3p",)   # entries whose call site calls profile_note() whenever a profile is active
PROF = [False]   # True while profile_begin() is active: call sites write `N.PROF[0] and
                 # N.profile_note(...)` so that the note's arguments cost nothing on the training path
_EXT = {}


def _launch_stream(args):
    """The torch stream object of the hipStream_t a launch was given (every launching entry point
    takes it as its last argument): events must be recorded on THAT stream -- the weight-gradient
    GEMMs run on the library's side stream, not on torch's current one."""
    cur = torch.cuda.current_stream()
    h = args[-1].value if args and isinstance(args[-1], ctypes.c_void_p) else None
    if not h or h == cur.cuda_stream:
        return cur
    st = _EXT.get(h)
    if st is None:
        st = _EXT[h] = torch.cuda.ExternalStream(h)
    return st


KERNEL_TIMED = ("s2t_gemm_x3p",)   # entries whose launch takes an armed event pair (csrc/streams.hip)
_free_pairs = []


class _Pair:
    """A (start, stop) HIP event pair stamped by the kernel launch itself."""
    __slots__ = ("h",)

    def __init__(self, h):
        self.h = h


def _new_pair(cdll):
    if _free_pairs:
        return _free_pairs.pop()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    check(cdll.s2t_prof_pair_create(ctypes.byref(a), ctypes.byref(b)), "s2t_prof_pair_create")
    return (a, b)


class _LibProxy:
    """Attribute access returns the ctypes function.  While profile_begin() is active the
    functions are wrapped so that launches of the selected entry point(s) are bracketed by HIP
    events on the stream the launch is given; otherwise the raw ctypes function is cached on the instance
    (no per-call indirection on the training path)."""

    def __init__(self, cdll):
        self._cdll = cdll

    def _reset(self):
        for k in [k for k in self.__dict__ if k.startswith("s2t_")]:
            del self.__dict__[k]

    def __getattr__(self, name):
        raw = getattr(self._cdll, name)
        if _Prof.target is None or name.endswith(("_floats", "_elems", "_bytes")) \
                or name in _NO_LAUNCH or (_Prof.target != "*" and _Prof.target != name) \
                or (_Prof.target != "*" and name in KERNEL_TIMED):    # (sampled inside the library)
            fn = raw          # (a single-entry profile leaves every other entry point unwrapped)
        else:
            def fn(*args, _raw=raw, _name=name):
                tgt = _Prof.target
                if tgt is None or (tgt != "*" and tgt != _name):
                    return _raw(*args)
                c = _Prof.count.get(_name, 0)
                _Prof.count[_name] = c + 1
                if c % _Prof.every:
                    return _raw(*args)
                if _name in KERNEL_TIMED:
                    # the kernel's own begin / end times (hipExtLaunchKernelGGL start / stop events:
                    # what rocprof reports) instead of marker packets recorded around the launch
                    pair = _new_pair(self._cdll)
                    self._cdll.s2t_prof_pair_arm(pair[0], pair[1])
                    rc = _raw(*args)
                    if self._cdll.s2t_prof_pair_consumed():
                        _Prof.events.setdefault(_name, []).append(_Pair(pair))
                    else:                        # the call returned before launching (-2, empty problem)
                        _free_pairs.append(pair)
                    return rc
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                st = _launch_stream(args)
                e0.record(st)
                rc = _raw(*args)
                e1.record(st)
                _Prof.events.setdefault(_name, []).append((e0, e1))
                return rc
        self.__dict__[name] = fn
        return fn


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m speech2text_amd.csrc.build` "
                "(there is no CPU or eager fallback for the hot path)")
        l = ctypes.CDLL(LIB_PATH)
        for name, (ret, ats) in parse_header().items():
            fn = getattr(l, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = ret
            fn.argtypes = ats
        _lib = _LibProxy(l)
    return _lib


def profile_begin(entry_point, every=1):
    """entry_point: a C entry-point name declared in include/s2t_mi355.h, or "*" for all.
    every = n: only every n-th launch of it is bracketed by events (and only those launches'
    algorithmic bytes / flops are counted): pick n coprime to the launches per step so that the
    sample walks over all call sites."""
    if entry_point != "*" and entry_point not in parse_header():
        raise ValueError(f"{entry_point!r} is not an entry point of include/s2t_mi355.h")
    _Prof.target = entry_point
    # The call sites' `N.PROF[0] and N.profile_note(...)` costs ~1.5 us of argument arithmetic per
    # launch while the flag is up: ~2 ms of host time per step, which a slow host does not hide
    # behind the GPU.  bench.py brackets ONE entry inside its timed region; when that entry's call
    # site reports by itself (SELF_NOTING: it tests _Prof.target), the global flag stays down.
    PROF[0] = entry_point == "*" or entry_point not in SELF_NOTING
    _Prof.events = {}
    _Prof.algo_bytes = {}
    _Prof.algo_flops = {}
    _Prof.every = max(1, int(every))
    _Prof.count = {}
    if _lib is not None:
        _lib._reset()
    if entry_point in KERNEL_TIMED:
        # a single-entry profile of a kernel-timed entry is taken INSIDE the library (every n-th
        # launch carries its own event pair): launches issued by the native layer executor never
        # pass through this module
        check(lib()._cdll.s2t_x3p_sample_begin(_Prof.every), "s2t_x3p_sample_begin")


def profile_note(entry_point, nbytes=0.0, flops=0.0):
    """Call sites report the ALGORITHMIC bytes/flops of a launch (DESIGN.md formulas)."""
    tgt = _Prof.target
    if tgt is None:
        return
    if (tgt == "*" or tgt == entry_point) and _Prof.count.get(entry_point, 0) % _Prof.every == 0:
        _Prof.algo_bytes[entry_point] = _Prof.algo_bytes.get(entry_point, 0.0) + nbytes
        _Prof.algo_flops[entry_point] = _Prof.algo_flops.get(entry_point, 0.0) + flops


def profile_end():
    """-> {entry: {launches, total_ms, avg_ms, algo_bytes, algo_flops}}"""
    sampled = _Prof.target if (_Prof.target in KERNEL_TIMED) else None
    _Prof.target = None
    PROF[0] = False
    if _lib is not None:
        _lib._reset()
    out = {}
    if _Prof.events:
        torch.cuda.synchronize()
    for name, evs in _Prof.events.items():
        ms = []
        for ev in evs:
            if isinstance(ev, _Pair):
                out_ms = ctypes.c_float()
                check(_lib._cdll.s2t_prof_pair_ms(ev.h[0], ev.h[1], ctypes.byref(out_ms)), "s2t_prof_pair_ms")
                ms.append(float(out_ms.value))
                _free_pairs.append(ev.h)
            else:
                ms.append(ev[0].elapsed_time(ev[1]))
        out[name] = {"launches": len(ms), "total_ms": float(sum(ms)),
                     "avg_ms": float(sum(ms) / len(ms)),
                     "algo_bytes": _Prof.algo_bytes.get(name, 0.0),
                     "algo_flops": _Prof.algo_flops.get(name, 0.0)}
    _Prof.events = {}
    if sampled is not None:
        n, ms, nb, fl = ctypes.c_long(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        check(_lib._cdll.s2t_x3p_sample_end(ctypes.byref(n), ctypes.byref(ms), ctypes.byref(nb),
                                            ctypes.byref(fl)), "s2t_x3p_sample_end")
        nmin = ctypes.c_double()
        check(_lib._cdll.s2t_x3p_sample_min_bytes(ctypes.byref(nmin)), "s2t_x3p_sample_min_bytes")
        if n.value > 0:
            out[sampled] = {"launches": int(n.value), "total_ms": float(ms.value),
                            "avg_ms": float(ms.value) / n.value, "algo_bytes": float(nb.value),
                            "algo_flops": float(fl.value), "algo_bytes_min": float(nmin.value)}
    return out


def stream():
    """hipStream_t torch considers current on the current device (raw handle, no Stream object)."""
    return ctypes.c_void_p(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))


# Pointer helpers return plain ints: every entry point has its argtypes set from the header
# (lib()), so ctypes converts an int to the pointer argument itself -- a ctypes.c_void_p object per
# argument was ~0.4 us of host time, times ~5 000 arguments per training step.
_F32, _I64, _I32 = torch.float32, torch.int64, torch.int32


def ptr(t, dtype=None):
    """Device pointer of a contiguous CUDA(HIP) tensor, or NULL for None."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("s2t kernels need device tensors (no CPU fallback)")
    if not t.is_contiguous():
        raise RuntimeError("s2t kernels need contiguous tensors")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def raw(t, dtype=None):
    """Device pointer of a (possibly row-strided) tensor; the caller passes the strides."""
    if not t.is_cuda:
        raise RuntimeError("s2t kernels need device tensors (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise RuntimeError(f"expected {dtype}, got {t.dtype}")
    return t.data_ptr()


def fp(t):
    if t is None:
        return None
    if t.dtype is not _F32 or not t.is_cuda or not t.is_contiguous():
        return ptr(t, _F32)                      # raises with the specific message
    return t.data_ptr()


def lp(t):
    return ptr(t, _I64)


def ip(t):
    return ptr(t, _I32)


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed with code {rc}")
