"""ctypes loader for libivlm_hip.so (the C-ABI of include/ivlm_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch  # (before the library is loaded: libivlm_hip.so must bind to torch's HIP runtime instance)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (IVLM_LIB_PATH: load another build of the same library - kernel experiments; the default is the in-tree build)
LIB_PATH = os.environ.get("IVLM_LIB_PATH") or os.path.join(_HERE, "libivlm_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ivlm_hip.h")

_lib = None

_CTYPES = {
    "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float,
    "ivlm_stream_t": C.c_void_p, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint8_t": C.c_uint8, "double": C.c_double,
}

class IvlmError(RuntimeError):
    pass


_constants = None


def header_constant(name):
    """the value of ``#define <name> <integer>`` in include/ivlm_hip.h: the ABI's numbers are read, not retyped (every such line of the
    header is parsed once)"""
    global _constants
    if _constants is None:
        _constants = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define[ \t]+(IVLM_\w+)[ \t]+(\d+)\b", open(HEADER_PATH).read(), flags=re.M)}
    if name not in _constants:
        raise IvlmError(f"include/ivlm_hip.h does not define {name} as an integer")
    return _constants[name]


FIT_MASK, FIT_CENTROID, FIT_CONTACT = (header_constant(f"IVLM_FIT_{k}") for k in ("MASK", "CENTROID", "CONTACT"))  # bits of terms_on
FIT_POSE, FIT_SCALE = header_constant("IVLM_FIT_POSE"), header_constant("IVLM_FIT_SCALE")                      # bits of optimise


class FitStepArgs(C.Structure):
    """``IvlmFitStepArgs`` of include/ivlm_hip.h, field for field (tests/test_fit_device_cpu.py compares the two)"""
    _fields_ = (
        [(n, C.c_void_p) for n in (
            "obj_verts", "faces", "vert_face_offsets", "vert_face_list", "human_verts", "obj_probs", "human_probs", "target",
            "target_centroid", "centroid_offset", "rotation", "translation", "scale", "m_rotation", "m_translation", "m_scale",
            "v_rotation", "v_translation", "v_scale", "grad_rotation", "grad_translation", "grad_scale", "step", "history",
            "term_history", "workspace")]
        + [("workspace_bytes", C.c_size_t)]
        + [(n, C.c_double) for n in ("lr_rotation", "lr_translation", "lr_scale", "beta1", "beta2", "eps")]
        + [(n, C.c_int32) for n in ("B", "N", "F", "H", "W", "N_h", "p_dtype", "max_iter", "terms_on", "optimise")]
        + [(n, C.c_float) for n in ("fx", "fy", "px", "py", "sigma", "blur_radius", "w_mask", "w_centroid", "w_contact")])


def header_prototypes(path: str = HEADER_PATH):
    """Parse ``include/ivlm_hip.h`` -> {name: (restype_str, [argtype_str, ...])}."""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    txt = re.sub(r"^\s*#.*$", " ", txt, flags=re.M)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w \*]*?)\b(ivlm_\w+)\s*\(([^;{}]*?)\)\s*;", txt, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if "typedef" in ret:
            continue
        argl = [] if args in ("", "void") else [a.strip() for a in args.split(",")]
        protos[name] = (ret, argl)
    return protos


def _to_ctype(decl: str):
    decl = decl.replace("const", " ").strip()
    if "*" in decl:
        base = decl.split("*")[0].strip().split()[0]
        return C.c_char_p if base == "char" else C.c_void_p
    base = decl.split()[0]
    return _CTYPES[base]


def load():
    """Load (once) and type-annotate the library. Raises IvlmError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise IvlmError(
            f"{LIB_PATH} not found: the HIP extension is required (no CPU fallback). "
            "Build it with `python -m interactvlm_amd.build` (hipcc --offload-arch=gfx950).")
    lib = C.CDLL(LIB_PATH)
    for name, (ret, args) in header_prototypes().items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:  # header/library drift is a build error, not a soft failure
            # (an experiment library built from an older tree - tools/experiments, timing only - may lack newer symbols: allowed only
            #  with BOTH an explicit library path and IVLM_ALLOW_MISSING_SYMBOLS=1, and never silently)
            if os.environ.get("IVLM_LIB_PATH") and os.environ.get("IVLM_ALLOW_MISSING_SYMBOLS") == "1":
                import warnings

                warnings.warn(f"{LIB_PATH} does not export {name} (declared in ivlm_hip.h): skipped (IVLM_ALLOW_MISSING_SYMBOLS=1)")
                continue
            raise IvlmError(f"libivlm_hip.so does not export {name} declared in ivlm_hip.h") from e
        fn.restype = _to_ctype(ret) if ret != "void" else None
        fn.argtypes = [_to_ctype(a) for a in args]
    _lib = lib
    return lib


def stream():
    """the handle of torch's current stream, as an ``ivlm_stream_t``"""
    return torch.cuda.current_stream().cuda_stream


def ptr(x):
    """the device address of a tensor, 0 for None (an output or input the call does without)"""
    return 0 if x is None else x.data_ptr()


def require_gpu(named):
    """named: (tensor, name) pairs (or ``_args``' triples), in the order their errors are reported"""
    for t, name, *_ in named:
        if not t.is_cuda:
            raise IvlmError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")


def require(t, dtype, name):
    """-> t, a contiguous GPU tensor of ``dtype`` (None: any); what every wrapper asks of an operand it hands over by address"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise IvlmError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise IvlmError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise IvlmError(f"{name}: tensor must be contiguous")
    return t


def workspace(size_fn, what, device, **sizes):
    """Ask ``size_fn(*sizes.values())`` (an ``ivlm_*_bytes`` query) and -> (uint8 tensor of that size on ``device``, nbytes); sizes the
    library refuses (the query returns 0) raise.  device None: only the check, -> (None, nbytes)."""
    nbytes = size_fn(*sizes.values())
    if nbytes == 0:
        raise IvlmError(f"{what}: sizes {', '.join(f'{k}={v}' for k, v in sizes.items())} are not supported")
    if device is None:
        return None, nbytes
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        lib = load()
        msg = lib.ivlm_error_string(rc)
        detail = lib.ivlm_last_hip_error() if rc == -3 else b""
        raise IvlmError(f"{what or 'ivlm call'} failed: {msg.decode() if msg else rc} ({rc})"
                        + (f" [{detail.decode()}]" if detail else ""))
