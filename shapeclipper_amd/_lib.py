"""ctypes binding of libshapeclipper_hip.so (the C ABI declared in include/shapeclipper_hip.h).

The product path has no CPU fallback: if the shared library is missing or a tensor is not on a
ROCm device, calls raise.  Tensors are passed as raw device pointers (``tensor.data_ptr()``) plus
explicit sizes; kernels are enqueued on torch's *current* stream.
"""
from __future__ import annotations

import ctypes
import os
import re
import threading
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# SHAPECLIPPER_HIP_LIB: load another build of the same C ABI (tuning / A-B experiments, e.g. tools/micro variants)
LIB_PATH = os.environ.get("SHAPECLIPPER_HIP_LIB") or os.path.join(_HERE, "lib", "libshapeclipper_hip.so")

HEADER_PATH = os.path.join(_HERE, os.pardir, "include", "shapeclipper_hip.h")
_CTYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double}


def read_signatures(text):
    """{name: (restype, [argtypes])} of every `sc_*` function the header text declares.  A reader for this one regular header, not a C
    parser: comments, preprocessor lines, the extern "C" braces and the sc_block_args struct body go, the rest is split on `;` and
    every piece must be `(int|long long) sc_name(params)`.  A parameter with a `*` is a c_void_p (device pointers, `void* stream`,
    host pointer arrays, `const sc_block_args*`); anything that is not understood raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    text = re.sub(r"typedef struct sc_block_args \{.*?\} sc_block_args", " ", text, flags=re.S)
    text = re.sub(r'extern "C" \{|\}', " ", text)
    sigs = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        m = re.fullmatch(r"(int|long long) (sc_\w+)\((.*)\)", decl)
        if m is None:
            raise RuntimeError("shapeclipper_amd: include/shapeclipper_hip.h: unrecognised declaration %r" % decl)
        params = [] if m.group(3) == "void" else m.group(3).split(",")
        try:        # `const float* x` -> pointer; `const int n` / `long long n` -> the type without qualifier and name
            args = [ctypes.c_void_p if "*" in p else _CTYPES[" ".join(w for w in p.split()[:-1] if w != "const")] for p in params]
        except KeyError:
            raise RuntimeError("shapeclipper_amd: include/shapeclipper_hip.h: unrecognised parameter type in %r" % decl) from None
        sigs[m.group(2)] = (_CTYPES[m.group(1)], args)
    return sigs


with open(HEADER_PATH) as _f:
    SIGNATURES = read_signatures(_f.read())
# derived from the header: the `int` returners (hipError_t status; wrapped by _Timed unless TIMING_SKIP names them) / the host-only
# `long long` size queries (never wrapped)
SYMBOLS = tuple(n for n, (res, _) in SIGNATURES.items() if res is ctypes.c_int)
SYMBOLS_OTHER = tuple(n for n, (res, _) in SIGNATURES.items() if res is ctypes.c_longlong)

_lib: Optional[ctypes.CDLL] = None

# Optional per-entry-point GPU timing (bench.py): when TIMING is a dict every C-ABI call is bracketed by
# two events on torch's current stream (the stream the kernels are enqueued on).
TIMING = None
TIMING_SKIP = ("sc_sdf_stream_pack", "sc_sdf_stream_pack_bytes", "sc_rgb_composite_backward_fused_parts", "sc_rgb_composite_backward_fused_partial_floats", "sc_latent_bias_forward", "sc_latent_bias_backward", "sc_set_reserved_cus", "sc_grid_cus", "sc_chamfer3d_backward_ordered_chunk","sc_conv3x3_release_tables", "sc_conv3x3_plan","sc_linear_bn_supported", "sc_linear_bn_forward", "sc_linear_bn_backward", "sc_linear_backward_data", "sc_bn_splits", "sc_isosurface_blocks_per_image", "sc_marching_cubes_mesh_vertex_blocks_per_image", "sc_bn_act_forward", "sc_bn_act_backward", "sc_bn_relu_pool_forward", "sc_bn_relu_pool_backward", "sc_gemm_plan",
               # the trunks' convolutions: ~250 calls per step -- two events each cost the step ~1 ms (rocprofv3 covers them: profiles/)
               "sc_conv3x3_forward", "sc_conv3x3_forward_split", "sc_conv3x3_forward_add", "sc_conv3x3_wgrad", "sc_conv3x3_wgrad_split", "sc_conv3x3_pack", "sc_conv3x3_pack_multi", "sc_conv3x3_pack_multi_units",
               "sc_conv_stem_forward", "sc_conv_stem_wgrad", "sc_conv1x1s2_forward", "sc_conv1x1s2_backward_data", "sc_conv1x1s2_wgrad",
               "sc_conv3x3s2_forward", "sc_conv3x3s2_bd_pack", "sc_conv3x3s2_backward_data", "sc_conv3x3s2_wgrad", "sc_conv3x3_tile_channels", "sc_conv3x3_tile_channels_split",
               "sc_basic_block_forward", "sc_basic_block_backward")

class _Timed:
    """Wraps a ctypes function: records (start, end) events around the call when TIMING is enabled."""

    def __init__(self, name, fn):
        self.name, self.fn = name, fn

    def __call__(self, *args):
        if TIMING is None:
            return self.fn(*args)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        code = self.fn(*args)
        e.record()
        TIMING.setdefault(self.name, []).append((s, e, args))
        return code


class _LibProxy:
    """The one table of bound functions: every declared entry point with the header's restype and argtypes, so plain ints, floats,
    None and data_ptr() integers go in as they are and a wrong argument kind raises ctypes.ArgumentError before the call.  Status
    entry points are wrapped by _Timed unless TIMING_SKIP names them; those and the size queries are the ctypes functions themselves
    (no Python frame between the ~270 BatchNorm / block / convolution calls of a step and the library)."""

    def __init__(self, cdll):
        self._cdll = cdll
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(cdll, name)
            fn.restype, fn.argtypes = restype, argtypes
            setattr(self, name, _Timed(name, fn) if restype is ctypes.c_int and name not in TIMING_SKIP else fn)


class HipLibraryMissing(RuntimeError):
    pass


def load():
    """Load the library once.  Raises HipLibraryMissing (never falls back)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryMissing(
                f"{LIB_PATH} not found -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C shapeclipper_amd/csrc`; there is no CPU fallback for the HIP hot path")
        _lib = _LibProxy(ctypes.CDLL(LIB_PATH))
    return _lib


NO_CPU = "shapeclipper_amd: HIP kernels need device tensors (got a CPU tensor); the product path has no CPU fallback"
_tls = threading.local()    # .dev: device index of the tensor ptr() saw last ON THIS THREAD (autograd and side-stream threads have their own)


def ptr(t: Optional[torch.Tensor]):
    """Device pointer of a contiguous CUDA/ROCm tensor (NULL for None)."""
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise RuntimeError(NO_CPU)
    if not t.is_contiguous():
        raise RuntimeError("shapeclipper_amd: tensor must be contiguous")
    _tls.dev = t.get_device()
    return ctypes.c_void_p(t.data_ptr())


def raw_stream(device: Optional[int] = None) -> int:
    """hipStream_t of torch's current stream on the current device as an integer.  (torch.cuda.current_stream() builds a Python Stream
    object per call, ~8 us: at ~280 entry-point calls per training step that was 2.4 ms of host time per step.)

    Device guard: the kernels are launched on the CURRENT device's stream, so a tensor that lives on another device
    (rank != device index, a stray `cuda:0` default in a multi-GPU process) would be dereferenced by the wrong GPU.  `device` = the
    device index of the call's tensors: callers that take raw data_ptr()s (BatchNorm and block paths) pass it explicitly;
    entry points that pass their tensors through ptr() leave it None and the device of the last ptr() of THIS thread is checked.  The
    remembered device is consumed by the check, so a later, unrelated call is never judged by a stale tensor."""
    cur = torch._C._cuda_getDevice()
    want = getattr(_tls, "dev", -1) if device is None else device
    _tls.dev = -1
    if want is not None and want >= 0 and want != cur:
        raise RuntimeError("shapeclipper_amd: tensor on cuda:%d but the current device is cuda:%d -- call torch.cuda.set_device(rank's device) "
                           "(or wrap the call in `with torch.cuda.device(t.device)`); kernels launch on the current device's stream"
                           % (want, cur))
    return torch._C._cuda_getCurrentRawStream(cur)


def stream():
    return ctypes.c_void_p(raw_stream())


def check(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"shapeclipper_amd: {what} failed with hipError_t {code}")
