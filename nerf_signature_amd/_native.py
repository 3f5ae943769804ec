"""ctypes loader of libnerfsig.so (the C ABI declared in include/nerfsig.h).

The library is the product path; there is no fallback.  If it is missing the import-time error says
how to build it, and every call checks its return code and raises with nsig_last_error().
"""
import ctypes
import os
import re

import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libnerfsig.so")

_c = ctypes
_vp, _u32, _fl, _int, _sz = _c.c_void_p, _c.c_uint32, _c.c_float, _c.c_int, _c.c_size_t


class NativeError(RuntimeError):
    pass


# The header is the one written record of the ABI: argument and return types are read from its declarations, as the compiler reads them for csrc/*.hip.
HEADER_PATH = os.path.join(_PKG, "..", "include", "nerfsig.h")
_PARAM_TYPES = {"nsig_stream_t": _vp, "uint32_t": _u32, "int32_t": _c.c_int32, "uint64_t": _c.c_uint64, "int": _int, "float": _fl, "double": _c.c_double, "size_t": _sz}
_RETURN_TYPES = {"int": _int, "size_t": _sz, "const char *": _c.c_char_p, "void *": _vp}
_DECLARATION = re.compile(r"^(int|size_t|const char \*|void \*)\s*(\w+)\s*\(([^()]*)\)\s*;", re.M)


def parse_header(text):
    """{name: (restype, argtypes)} of every `<ret> name(<params>);` in a header's text.  A parameter with a `*` and nsig_stream_t are pointers, the scalar types map by
    name, `(void)` is no arguments; anything else -- and any other text with a parenthesis in it -- raises NativeError naming the declaration: nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    found = {}
    for ret, name, params in _DECLARATION.findall(text):
        argtypes = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            words = [w for w in p.split() if w != "const"]
            t = _vp if "*" in p else _PARAM_TYPES.get(words[0] if words else "")
            if t is None:
                raise NativeError(f"{name}({' '.join(params.split())}): no ctypes type for the parameter '{p.strip()}'")
            argtypes.append(t)
        found[name] = (_RETURN_TYPES[ret], argtypes)
    stray = [line.strip() for line in _DECLARATION.sub("", text).splitlines() if "(" in line]
    if stray:
        raise NativeError(f"cannot read the declaration '{stray[0]}'")
    return found


def _read_header(path):
    try:
        with open(path) as f:
            return parse_header(f.read())
    except (OSError, NativeError) as e:
        raise NativeError(f"{path}: {e} (the ctypes signatures of libnerfsig.so are derived from this header; there is no second table)") from e


_DECLARED = _read_header(HEADER_PATH)
SIGNATURES = {name: argtypes for name, (_, argtypes) in _DECLARED.items()}      # name -> argtypes
_RESTYPES = {name: restype for name, (restype, _) in _DECLARED.items()}

_lib = None


def load():
    """Load libnerfsig.so; raises if the library is missing (there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("NERFSIG_LIB", LIB_PATH)   # override: instrumented builds of the same sources (tools/dec_timing.py)
    if not os.path.exists(path):
        raise NativeError(f"{path} not found: the HIP extension is required (no fallback). "
                          f"Build it with `python -m nerf_signature_amd.build`.")
    _lib = ctypes.CDLL(path)
    _lib.nsig_last_error.restype = _c.c_char_p
    return _lib


_bound = {}


def fn(name):
    """Bound entry point `name` with the argtypes of include/nerfsig.h; raises if the library lacks it."""
    f = _bound.get(name)
    if f is None:
        lib = load()
        try:
            f = getattr(lib, name)
        except AttributeError as e:
            raise NativeError(f"libnerfsig.so does not export {name}; rebuild with `python -m nerf_signature_amd.build --force`") from e
        f.argtypes = SIGNATURES[name]
        f.restype = _RESTYPES[name]
        _bound[name] = f
    return f


def verify_exports():
    """Every symbol declared in the header must be exported (used by the CPU test-suite and build())."""
    for name in SIGNATURES:
        fn(name)
    return sorted(SIGNATURES)


def call(name, *args):
    """Invoke an int-returning entry point; non-zero return raises with the library's message."""
    rc = fn(name)(*args)
    if rc != 0:
        msg = load().nsig_last_error().decode("utf-8", "replace")
        raise (ValueError if rc == 1 else NativeError)(f"{name} failed (code {rc}): {msg}")


def mlp_precision_name():
    """Human-readable arithmetic of the MLP kernels as currently selected (mlp_get_precision)."""
    return ("fp16 MFMA with f32 accumulate (MLPs)" if fn("mlp_get_precision")() == 1 else "split-bf16 MFMA (3 per product) with f32 accumulate (MLPs)")


def mlp_mfma_per_wave():
    """(MFMAs the forward MLP kernel issues per 32 points, operand dtype key) for the selected arithmetic."""
    return (24, "f16") if fn("mlp_get_precision")() == 1 else (72, "bf16")


def set_mlp_precision(name):
    """'f16' or 'bf16x3' (mlp_set_precision)."""
    call("mlp_set_precision", {"bf16x3": 0, "f16": 1}[name])


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  The tensor must be contiguous and on the GPU."""
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("libnerfsig entry points take device tensors; got a CPU tensor")
    if not t.is_contiguous():
        raise ValueError("libnerfsig entry points take contiguous tensors")
    return t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream():
    """The current torch stream as a hipStream_t, so launches compose with autograd/autocast/RCCL streams.
    (torch's raw-stream query: the eager loops call this ~30 times per step, and torch.cuda.current_stream() builds a Stream object each time.)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def ptr_array(tensors):
    """Host array of device pointers (for the `*_host` pointer-table arguments)."""
    arr = (ctypes.c_void_p * len(tensors))(*[ptr(t) for t in tensors])
    return arr


def check(t, dtype, name, shape_last=None):
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if shape_last is not None and t.shape[-1] != shape_last:
        raise ValueError(f"{name}: expected last dimension {shape_last}, got {tuple(t.shape)}")
    return t
