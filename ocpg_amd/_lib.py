"""ctypes loader for libocpg_hip.so -- the only way the product reaches its kernels.

There is deliberately NO fallback: if the library is missing or a tensor is not on the GPU the call raises.
"""
import ctypes
import glob
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# OCPG_HIP_LIB: load another build of the SAME library (kernel experiments / A-B timing); never a fallback path
LIB_PATH = os.environ.get("OCPG_HIP_LIB") or os.path.join(_HERE, "lib", "libocpg_hip.so")
_lib = None

# The dtype code of the C ABI (include/ocpg_hip.h, "dtype: 0 = float32, 1 = bfloat16, 2 = float16" at ocpg_bn_act_fwd; the _h16 entry
# points take the 16-bit subset with the same numbering).  The one statement of it on the Python side: the bindings import these.
DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
H16_CODE = {torch.bfloat16: 1, torch.float16: 2}

# ---- the ctypes signatures come from the header: to add an entry point, declare it in include/*.h and export it ----------
_BY_VALUE = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_ulonglong, "float": ctypes.c_float,
             "double": ctypes.c_double}
_RETURNS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "void": None, "const char*": ctypes.c_char_p}
_DECL = re.compile(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)")


def _declarations(text):
    """Header text -> [(return type, symbol, [(parameter type, parameter name)])], types with single blanks and the `*` attached.
    Block comments and preprocessor lines are dropped; anything that is not a plain function declaration raises."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    if "//" in text:
        raise ValueError("a // comment in the header: the signature parser reads block comments only")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    text = re.sub(r"^[ \t]*\}[ \t]*$", "", text, flags=re.M)

    def norm(t):
        return re.sub(r"\s*\*\s*", "*", " ".join(t.split()))
    out = []
    for stmt in text.split(";"):
        if not stmt.strip():
            continue
        m = _DECL.fullmatch(stmt.strip())
        if m is None:
            raise ValueError(f"not a function declaration: {' '.join(stmt.split())!r}")
        params = []
        for p in m.group(3).split(","):
            if p.strip() in ("", "void"):
                continue
            t, pname = re.fullmatch(r"(.*?)(\w*)", p.strip(), flags=re.S).groups()
            params.append((norm(t), pname))
        out.append((norm(m.group(1)), m.group(2), params))
    return out


def parse_header(text):
    """Header text -> {symbol: (restype, [argtypes])}.  A pointer is c_void_p (callers pass data_ptr() integers or None); a by-value
    or return type outside the header's vocabulary raises: there is no default."""
    out = {}
    for ret, name, params in _declarations(text):
        if ret not in _RETURNS:
            raise ValueError(f"{name}: return type {ret!r} is not one of {sorted(_RETURNS)}")
        argtypes = []
        for t, pname in params:
            if "*" not in t and t not in _BY_VALUE:
                raise ValueError(f"{name}: parameter {pname!r} has by-value type {t!r}, not one of {sorted(_BY_VALUE)}")
            argtypes.append(ctypes.c_void_p if "*" in t else _BY_VALUE[t])
        out[name] = (_RETURNS[ret], argtypes)
    return out


_HEADERS = "".join(open(h).read() for h in sorted(glob.glob(os.path.join(os.path.dirname(_HERE), "include", "*.h"))))
_PARSED = parse_header(_HEADERS)
# symbol -> argtypes of every compute entry point the headers declare (tests and tools read it)
SIGNATURES = {name: argtypes for name, (_, argtypes) in _PARSED.items() if name != "ocpg_hip_version"}


# ---- optional live kernel timing (bench.py): HIP events on the launch stream around every library call ----------
_TIMING = {"on": False, "events": []}
# an entry point without a `void* stream` parameter launches nothing (a host-side query or setter): handed out raw, never timed or counted
_UNTIMED = frozenset(name for _, name, params in _declarations(_HEADERS)
                     if name in SIGNATURES and ("void*", "stream") not in params)


def enable_kernel_timing(on=True):
    _TIMING["on"] = on
    _TIMING["events"] = []


def collect_kernel_timing(work=None):
    """-> {symbol: {"ms": total, "n": calls, "work": sum of work(symbol, args) over the calls}}; `work` maps a call's
    arguments (pointers and scalars as passed) to its algorithmic bytes / FLOPs, or None.  (MSDeformAttn is timed by its own
    wrapper, which knows the encoder / decoder shape: ops/functions/ms_deform_attn_func.py.)"""
    torch.cuda.synchronize()
    out = {}
    for name, args, e0, e1 in _TIMING["events"]:
        d = out.setdefault(name, {"ms": 0.0, "n": 0, "work": 0.0, "modelled": 0})
        d["ms"] += e0.elapsed_time(e1)
        d["n"] += 1
        w = work(name, args) if work is not None else None
        if isinstance(w, tuple):            # (FLOPs, low-precision operands): matrix-core symbols
            d["work_lowp"] = d.get("work_lowp", 0.0) + (w[0] if w[1] else 0.0)
            w = w[0]
        if w is not None:
            d["work"] += w
            d["modelled"] += 1
    _TIMING["events"] = []
    _TIMING["on"] = False
    return out


# ---- optional call census (tests: prove WHICH entry points served a module; bench.py: launches per step by symbol) ----
CENSUS = {"on": False, "calls": {}}
# a symbol that is another ROW ORDER of a kernel (same arguments, bit-identical result) is also counted as the symbol it stands in for:
# the census answers "which kernel family served this module", and that answer does not change with the row order
CENSUS_ALSO = {"ocpg_conv3x3_mfma_dgrad_w_s2": "ocpg_conv3x3_mfma_dgrad_w", "ocpg_conv3x3_mfma_dgrad_w_s2_h16": "ocpg_conv3x3_mfma_dgrad_w_h16",
               # the ring form of the 3x3 weight gradient (csrc/conv3x3_wgrad_ring_kernel.h): same arguments, bit-identical partial sums
               "ocpg_conv3x3_mfma_wgrad_ring": "ocpg_conv3x3_mfma_wgrad", "ocpg_conv3x3_mfma_wgrad_ring_h16": "ocpg_conv3x3_mfma_wgrad_h16",
               # the same dropout+add+LayerNorm kernels with more ports (csrc/fused_ln.hip)
               "ocpg_dropout_add_ln_fwd_ex": "ocpg_dropout_add_ln_fwd", "ocpg_dropout_add_ln_bwd_ex": "ocpg_dropout_add_ln_bwd"}


def census(on=True):
    """Start (and clear) / stop counting successful (rc == 0) calls per entry point; read CENSUS['calls']."""
    CENSUS["on"] = on
    if on:
        CENSUS["calls"] = {}
    return CENSUS["calls"]


class _Lib:
    """Attribute proxy over the CDLL: every kernel entry point can be bracketed by events when timing is on."""

    def __init__(self, cdll):
        self._cdll = cdll

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if name not in SIGNATURES or name in _UNTIMED:
            setattr(self, name, fn)
            return fn
        timed = not name.startswith("ocpg_msda_")       # MSDeformAttn is timed by its own wrapper (knows enc / dec shape)

        def call(*a):
            if CENSUS["on"]:
                rc = fn(*a)
                if rc == 0:
                    for k in (name, CENSUS_ALSO.get(name)):
                        if k is not None:
                            CENSUS["calls"][k] = CENSUS["calls"].get(k, 0) + 1
                return rc
            if not (timed and _TIMING["on"]):
                return fn(*a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            _TIMING["events"].append((name, tuple(getattr(x, "value", x) for x in a), e0, e1))
            return rc
        setattr(self, name, call)
        return call


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m ocpg_amd.csrc.build` "
                "(hipcc --offload-arch=gfx950). The HIP extension is mandatory; there is no CPU/PyTorch fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _PARSED.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = _Lib(L)
    return _lib


def check(status, what):
    if status != 0:
        if status <= -1000:
            raise RuntimeError(f"{what}: invalid argument #{-status - 1000}")
        raise RuntimeError(f"{what}: HIP error {-status}")


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu(name, t):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor: Not implemented on the CPU")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} tensor has to be contiguous")
