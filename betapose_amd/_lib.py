"""ctypes binding of libbetapose_hip.so (include/betapose_hip.h).

The library is the product: if it is missing it is built in-tree with hipcc, and
if that is impossible the import of any engine class FAILS LOUDLY -- there is no
CPU or eager-PyTorch fallback on the product path.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# BP_LIB: an alternative build of the same library (tools only: `python -m betapose_amd.build --experimental` makes
# libbetapose_hip_exp.so with the measured-and-rejected kernels and the timing ablations compiled in)
LIB_PATH = os.environ.get("BP_LIB") or os.path.join(_HERE, "libbetapose_hip.so")
HEADER_PATH = os.path.join(_HERE, "csrc", "..", "..", "include", "betapose_hip.h")      # build.py HEADERS
_lock = threading.Lock()
_lib = None

_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long long": C.c_longlong,
            "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}


def _ctype(text, decl, is_return=False):
    """The ctypes type of one parameter (its name, if any, included in ``text``) or of a return type."""
    tok = [t for t in re.findall(r"\w+|\*|\S", text) if t != "const"]
    if any(t != "*" and not re.fullmatch(r"\w+", t) for t in tok):      # ( ) [ ] ... : function pointers, arrays, variadics
        raise ValueError("cannot map '%s' in the declaration: %s" % (text.strip(), decl))
    if "*" in tok:      # char* is a C string, every other pointer (pointer to pointer included) an address
        return C.c_char_p if tok[:tok.index("*")] == ["char"] and tok.count("*") == 1 else C.c_void_p
    if is_return and tok == ["void"]:
        return None
    for name in (tok, tok[:-1] if not is_return else None):                 # without and with the parameter's name
        if name and " ".join(name) in _SCALARS:
            return _SCALARS[" ".join(name)]
    raise ValueError("unknown type '%s' in the declaration: %s" % (text.strip(), decl))


def parse_prototypes(header_text):
    """name -> (restype, argtypes) of every function ``header_text`` declares.  Scalars map by name, ``char*`` to
    c_char_p and every other pointer to c_void_p; a declaration that cannot be mapped raises ValueError naming it."""
    code = re.sub(r"/\*.*?\*/|//[^\n]*", " ", header_text, flags=re.S)
    code = re.sub(r"^[ \t]*#.*$", " ", code, flags=re.M).replace('extern "C" {', " ")
    code = re.sub(r"\{[^{}]*\}", " ", code).replace("}", " ")               # struct bodies; the closing brace of extern "C"
    protos = {}
    for decl in (" ".join(s.split()) for s in code.split(";")):
        if not decl or decl.startswith("typedef "):
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", decl)
        if not m:
            raise ValueError("not a function declaration: %s" % decl)
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        protos[name] = (_ctype(ret, decl, True), [_ctype(p, decl) for p in params])
    return protos


with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_prototypes(_f.read())      # every symbol include/betapose_hip.h declares

RESULT_FLOATS = 316
POSE_DOUBLES = 166          # include/betapose_hip.h BP_POSE_DOUBLES
PNP_MAX_POINTS = 64
MAX_SCENE_CLASSES = 16      # include/betapose_hip.h BP_MAX_SCENE_CLASSES
MAX_CANDIDATES = 8          # include/betapose_hip.h BP_MAX_CANDIDATES
MERGED_FLOATS = 152         # include/betapose_hip.h BP_MERGED_FLOATS


class BetaposeHipError(RuntimeError):
    pass


def lib():
    """Load (building first if needed) the HIP library.  Raises on failure."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        # torch ships its own libamdhip64; load it FIRST so this library binds to the same HIP runtime
        # (loading /opt/rocm's copy first leaves two runtimes in the process and ours then sees no device)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            from .build import build
            build(verbose=False)
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:
            raise BetaposeHipError("cannot load %s: %s (run `python -m betapose_amd.build`)" % (LIB_PATH, e))
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)   # AttributeError if the .so is stale/incomplete
            fn.restype = res
            fn.argtypes = args
        _lib = L
        return L


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().bp_last_error()
        raise BetaposeHipError(msg.decode() if msg else "libbetapose_hip error %d" % rc)


def require_gpu() -> None:
    """Product entry points call this: no GPU / no HIP extension => hard error."""
    import torch
    if not torch.cuda.is_available():
        raise BetaposeHipError("betapose_amd needs an AMD GPU (gfx950): torch.cuda.is_available() is False; "
                               "there is no CPU fallback on the product path")
    if lib().bp_device_count() <= 0:
        raise BetaposeHipError("libbetapose_hip.so sees no HIP device")


def ptr(t) -> int:
    """Device/host pointer of a contiguous torch tensor or numpy array."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        if not t.is_contiguous():
            raise ValueError("tensor must be contiguous")
        return t.data_ptr()
    return t.ctypes.data


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream


_BITS = {"uint16": "int16", "uint32": "int32", "uint64": "int64"}       # torch holds these as the signed type of their size


class Side:
    """Where a host/device pair ``bp_X_host`` / ``bp_X`` runs and where its buffers live: the host (``device=None``,
    numpy arrays) or a torch device (tensors).  A wrapper takes its buffers from ``put`` / ``empty`` / ``zeros``, states
    its argument list once in ``call`` and reads the results back with ``get``."""

    def __init__(self, device=None):
        self.torch = self.dev = None
        if device is not None:
            import torch
            require_gpu()
            self.torch, self.dev = torch, torch.device(device)

    def _dtype(self, dtype):
        name = np.dtype(dtype).name
        return getattr(self.torch, _BITS.get(name, name))

    def put(self, a, dtype=None, copy=False):
        """``a`` (array, tensor or None) on this side: a contiguous numpy array on the host (``copy``: one of its own),
        a tensor on the device.  A tensor that already lives there is taken as it is; an unsigned array goes up as the
        bits of the signed type of its size."""
        if a is None:
            return None
        if self.dev is None:
            if hasattr(a, "data_ptr"):
                a = a.detach().cpu().numpy()
            return np.array(a, dtype, order="C") if copy else np.ascontiguousarray(a, dtype)
        if hasattr(a, "data_ptr"):
            return (a.to(self.dev) if dtype is None else a.to(self.dev, self._dtype(dtype))).contiguous()
        a = np.ascontiguousarray(a, dtype)
        if a.dtype.name in _BITS:
            a = a.view(_BITS[a.dtype.name])
        return self.torch.from_numpy(a if a.flags.writeable else a.copy()).to(self.dev)     # (torch warns on a read-only array)

    def empty(self, shape, dtype=np.float32):
        if self.dev is None:
            return np.empty(shape, dtype)
        return self.torch.empty(shape, dtype=self._dtype(dtype), device=self.dev)

    def zeros(self, shape, dtype=np.float32):
        if self.dev is None:
            return np.zeros(shape, dtype)
        return self.torch.zeros(shape, dtype=self._dtype(dtype), device=self.dev)

    def get(self, a, dtype=None, copy=False):
        """The buffer ``a`` of this side as a numpy array: itself on the host (``copy``: a copy), read back from the
        device.  ``dtype`` names the unsigned type whose bits a device buffer holds."""
        a = (a.copy() if copy else a) if self.dev is None else a.cpu().numpy()
        return a if dtype is None else a.view(dtype)

    def call(self, name, *args):
        """``name + "_host"`` on the host, ``name`` on the device's current stream.  An argument with a ``shape`` (or
        None) becomes its pointer, anything else (scalars, the ``ptr`` of an array that stays on the host in both calls)
        passes through."""
        args = [ptr(a) if (a is None or hasattr(a, "shape")) else a for a in args]
        if self.dev is None:
            check(getattr(lib(), name + "_host")(*args))
        else:
            with self.torch.cuda.device(self.dev):
                check(getattr(lib(), name)(*args, self.torch.cuda.current_stream(self.dev).cuda_stream))
