"""ctypes binding of libposecnn_hip.so: the C-ABI is what the headers under include/ declare, and the ctypes signatures
are derived from their prototypes when the library is first loaded (`BINDINGS`), not repeated here.

This is the Python-side analogue of the reference's ``tf.load_op_library('<op>.so')`` stubs
(lib/hough_voting_gpu_layer/hough_voting_gpu_op.py:4-7 and siblings). The library is built
in-tree by ``__graft_entry__.build()`` / ``make -C posecnn_amd/csrc``. There is NO fallback:
if the shared object is missing or an entry point fails, the call raises.
"""
import ctypes
import glob
import os
import re
from ctypes import (POINTER, c_char_p, c_float, c_int, c_int64, c_long, c_size_t, c_uint32, c_uint64, c_void_p)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libposecnn_hip.so")

PCNN_OK = 0
PCNN_EINVAL = -1
PCNN_EWORKSPACE = -2
PCNN_EHIP = -3
PCNN_ENULL = -4

MAX_ROI = 128
HOUGH_ROWS_CAPACITY = MAX_ROI * 9
VERTEX_CHANNELS = 3
POSE_CHANNELS = 4

INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

# ---- the headers are the one statement of the C-ABI: every `ret pcnn_name(params);` in them is bound from its own text ----
# The grammar is closed: what it does not name raises, nothing falls back to void*.
_RESTYPES = {"int": c_int, "long": c_long, "uint32_t": c_uint32, "const char*": c_char_p}
_SCALARS = {"int": c_int, "long": c_long, "float": c_float, "size_t": c_size_t, "int64_t": c_int64, "uint32_t": c_uint32,
            "uint64_t": c_uint64}
_POINTERS = {"size_t": POINTER(c_size_t), "int": POINTER(c_int), "char": c_char_p}   # every other pointer: void*

BINDINGS = {}   # header basename -> {symbol: (restype, argtypes)} in header order; filled by the first lib() call


def _strip_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _argtype(param, where):
    if "(" in param or "[" in param:
        raise ValueError("%s: array and function-pointer parameters are not part of the C-ABI" % where)
    tokens = [t for t in re.findall(r"\w+|\*", param) if t != "const"]
    stars = tokens.count("*")
    if stars > 1:
        raise ValueError("%s: pointer to pointer" % where)
    if stars:
        base, name = tokens[:tokens.index("*")], tokens[tokens.index("*") + 1:]
        if not base or len(name) > 1:
            raise ValueError("%s: not `type* [name]`" % where)
        return _POINTERS.get(" ".join(base), c_void_p)
    base = " ".join(tokens[:-1] if len(tokens) > 1 else tokens)   # the last word is the parameter's name
    if base not in _SCALARS:
        raise ValueError("%s: scalar type '%s' is not one of %s" % (where, base, sorted(_SCALARS)))
    return _SCALARS[base]


def parse_header(header, text):
    """The prototypes of one header's text -> {symbol: (restype, argtypes)}; ValueError names header, symbol and parameter."""
    text = re.sub(r"^[ \t]*#.*$", "", _strip_comments(text), flags=re.M)
    found = {}
    for m in re.finditer(r"\b(pcnn_\w+)\s*\(", text):
        name, depth, end = m.group(1), 1, m.end()
        while depth and end < len(text):
            depth += {"(": 1, ")": -1}.get(text[end], 0)
            end += 1
        if depth or not re.match(r"\s*;", text[end:]):
            raise ValueError("%s: %s: not a prototype `ret %s(params);`" % (header, name, name))
        ret = re.sub(r"\s*\*\s*", "*", " ".join(re.split(r"[;{}]", text[:m.start()])[-1].split()))
        if ret not in _RESTYPES:
            raise ValueError("%s: %s: return type '%s' is not one of %s" % (header, name, ret, sorted(_RESTYPES)))
        if name in found:
            raise ValueError("%s: %s is declared twice" % (header, name))
        params, depth = [""], 0
        for ch in text[m.end():end - 1]:
            depth += {"(": 1, "[": 1, ")": -1, "]": -1}.get(ch, 0)
            if ch == "," and not depth:
                params.append("")
            else:
                params[-1] += ch
        params = [" ".join(p.split()) for p in params]
        found[name] = (_RESTYPES[ret], [] if params == ["void"] else
                       [_argtype(p, "%s: %s: parameter %d '%s'" % (header, name, i + 1, p)) for i, p in enumerate(params)])
    return found


def parse_headers(texts):
    """[(header basename, text), ...] -> {basename: parse_header(...)} in the given order; a symbol in two headers raises."""
    out, owner = {}, {}
    for header, text in texts:
        out[header] = parse_header(header, text)
        for name in out[header]:
            if name in owner:
                raise ValueError("%s: %s is already declared in %s" % (header, name, owner[name]))
            owner[name] = header
    return out


def header_texts():
    """[(name, text)] of every include/*.h (name: the basename), sorted, then of every include/*/*.h (name: the path under
    include/ with forward slashes, e.g. "posecnn_hip/pose_polish.h"), sorted."""
    top = sorted(glob.glob(os.path.join(INCLUDE_DIR, "*.h")))
    sub = sorted(glob.glob(os.path.join(INCLUDE_DIR, "*", "*.h")))
    return [(os.path.relpath(p, INCLUDE_DIR).replace(os.sep, "/"), open(p).read()) for p in top + sub]


def route_header_texts():
    """[(name, text)] of every include/*/*/*.h (name: the path under include/), sorted: the entries of single routes of
    the network (e.g. "posecnn_hip/trunk/conv2_fused.h"), bound like every other header, listed apart from the public ones."""
    deep = sorted(glob.glob(os.path.join(INCLUDE_DIR, "*", "*", "*.h")))
    return [(os.path.relpath(p, INCLUDE_DIR).replace(os.sep, "/"), open(p).read()) for p in deep]


def header_abi_version(texts=None):
    """PCNN_ABI_VERSION as include/posecnn_hip.h defines it."""
    text = dict(header_texts() if texts is None else texts)["posecnn_hip.h"]
    return int(re.search(r"^[ \t]*#[ \t]*define[ \t]+PCNN_ABI_VERSION[ \t]+(\d+)[ \t]*$", _strip_comments(text), flags=re.M).group(1))


def profile_enable(on=True):
    """Bracket every library kernel launch with HIP events on its launch stream."""
    call("pcnn_profile_enable", 1 if on else 0)


def profile_report(reset=True):
    """-> {kernel_name: {"calls", "total_ms", "avg_us"}} for launches since the last reset."""
    import json
    L = lib()
    n = L.pcnn_profile_report(None, 0)
    buf = ctypes.create_string_buffer(int(n) + 16)
    L.pcnn_profile_report(buf, len(buf))
    if reset:
        L.pcnn_profile_reset()
    rep = json.loads(buf.value.decode())
    # template instances are launched as `(kernel<a, b>)`: drop the macro's parentheses
    return {k.strip("()"): v for k, v in rep.items()}

_lib = None


class PoseCNNHipError(RuntimeError):
    """A libposecnn_hip.so entry point returned a negative pcnn_status."""

    def __init__(self, fn, status, message):
        super().__init__("%s failed: status %d (%s)" % (fn, status, message))
        self.status = status


def lib():
    """Load (once) and return the ctypes handle; raises if the HIP library is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libposecnn_hip.so not found at %s — build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C posecnn_amd/csrc`. There is no CPU/PyTorch fallback." % LIB_PATH)
        # The HIP runtime the process uses must be ONE: torch ships its own libamdhip64 under torch/lib, this library names the
        # system's by soname. Loaded after torch, the soname resolves to torch's already-mapped copy; loaded BEFORE it, the
        # process ends up with two runtimes and every launch on a torch stream fails with "no ROCm-capable device is detected"
        # (round 6: `build()` followed by `smoke()` in one process did exactly that). So torch's goes in first, always.
        import torch  # noqa: F401
        handle = ctypes.CDLL(LIB_PATH)
        texts = header_texts()
        bindings = parse_headers(texts + route_header_texts())
        for table in bindings.values():
            for name, (res, args) in table.items():
                fn = getattr(handle, name)  # AttributeError if the symbol is missing: fail loudly
                fn.restype = res
                fn.argtypes = args
        if handle.pcnn_abi_version() != header_abi_version(texts):
            raise RuntimeError("libposecnn_hip.so ABI version mismatch")
        BINDINGS.update(bindings)
        _lib = handle
    return _lib


def check(fn_name, status):
    if status != PCNN_OK:
        msg = lib().pcnn_last_error_string()
        msg = msg.decode("utf-8", "replace") if msg else ""
        if status in (PCNN_EINVAL, PCNN_ENULL):
            # the reference raises InvalidArgument for the same conditions (OP_REQUIRES)
            raise ValueError("%s: %s" % (fn_name, msg))
        raise PoseCNNHipError(fn_name, status, msg)


def call(name, *args):
    """Call the entry `name` of the library (AttributeError if it has none) and pass its status through `check`."""
    check(name, getattr(lib(), name)(*args))
