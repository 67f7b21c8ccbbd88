"""The C-ABI library builds, loads without a GPU and exports every symbol include/*.h declares."""
import ctypes
import os
import re

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "shapeclipper_hip.h")).read()
    return sorted(set(re.findall(r"^(?:int|long long) (sc_\w+)\(", text, flags=re.M)))


def test_library_exports_every_declared_symbol():
    from shapeclipper_amd import _lib
    names = declared_symbols()
    assert len(names) >= 9
    assert os.path.exists(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    cdll = ctypes.CDLL(_lib.LIB_PATH)          # loads without a GPU; no compute calls here
    for n in names:
        assert hasattr(cdll, n), n
    assert sorted(_lib.SYMBOLS + _lib.SYMBOLS_OTHER) == names, (sorted(_lib.SYMBOLS + _lib.SYMBOLS_OTHER), names)


def test_product_fails_loudly_without_device_tensors():
    import pytest
    import torch
    from shapeclipper_amd import ops, packing
    from oracle import reference_ops as R
    W = R.init_sdf_weights(R.Cfg(), 0)
    pack, cb = packing.pack_sdf(W, torch.zeros(1, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sdf_forward(torch.zeros(4, 3), pack, cb, 4)


def test_product_does_not_import_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "shapeclipper_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in re.sub(r"#.*", "", src).replace("oracle/", ""), os.path.join(dirpath, f)
    for f in ("chamfer_3D.py", "train.py", "evaluate.py", "pretrain.py"):
        assert "import oracle" not in open(os.path.join(ROOT, f)).read() and "from oracle" not in open(os.path.join(ROOT, f)).read()


def test_device_guard_raises_when_a_tensor_is_not_on_the_current_device(monkeypatch):
    """Kernels are launched on the CURRENT device's stream (shapeclipper_amd/_lib.py): every entry point passes its tensors through ptr()
    and then asks for the stream, which refuses a tensor of another device (rank != device index in a multi-GPU process).  No GPU here:
    the device queries are replaced, the tensor is a stand-in with the four methods ptr() uses."""
    import torch
    from shapeclipper_amd import _lib

    class FakeCudaTensor:
        is_cuda = True
        def __init__(self, dev): self._dev = dev
        def is_contiguous(self): return True
        def get_device(self): return self._dev
        def data_ptr(self): return 4096

    monkeypatch.setattr(torch._C, "_cuda_getCurrentRawStream", lambda dev: 1234 + dev, raising=False)
    monkeypatch.setattr(torch._C, "_cuda_getDevice", lambda: 1, raising=False)
    assert _lib.ptr(FakeCudaTensor(1)).value == 4096
    assert _lib.raw_stream() == 1235                       # tensor on cuda:1, current device cuda:1: the stream of device 1
    _lib.ptr(FakeCudaTensor(0))
    with pytest.raises(RuntimeError, match="current device is cuda:1"):
        _lib.stream()
    #  the remembered device is consumed by the check: an unrelated later call is not judged by the stale cuda:0 tensor ...
    assert _lib.raw_stream() == 1235
    # ... callers that take raw data_ptr()s name the device themselves (BatchNorm / block / workspace paths) ...
    assert _lib.raw_stream(1) == 1235
    with pytest.raises(RuntimeError, match="tensor on cuda:0"):
        _lib.raw_stream(0)
    # ... and the memory is per thread (autograd and side-stream threads launch concurrently)
    import threading
    _lib.ptr(FakeCudaTensor(0))
    seen = []
    t = threading.Thread(target=lambda: seen.append(_lib.raw_stream()))
    t.start(); t.join()
    assert seen == [1235]
    with pytest.raises(RuntimeError):
        _lib.raw_stream()


def _header_text():
    return open(os.path.join(ROOT, "include", "shapeclipper_hip.h")).read()


def _declarations():
    """{name: (result type, parameter count)} read off the header independently of the product's reader: comments out, then every
    `int|long long sc_name(...)` up to its closing parenthesis (no declaration nests parentheses)."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", _header_text(), flags=re.S)
    out = {}
    for res, name, params in re.findall(r"^(int|long long) (sc_\w+)\(([^)]*)\)\s*;", text, flags=re.M):
        out[name] = (res, 0 if params.strip() == "void" else params.count(",") + 1)
    return out


def test_every_declared_function_is_bound_with_the_headers_signature():
    from shapeclipper_amd import _lib
    lib, decl = _lib.load(), _declarations()
    assert sorted(decl) == declared_symbols() == sorted(_lib.SIGNATURES)        # the reader skipped nothing
    for name, (res, n_params) in decl.items():
        fn = getattr(lib._cdll, name)
        assert fn.restype is {"int": ctypes.c_int, "long long": ctypes.c_longlong}[res], name
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, (name, fn.argtypes, n_params)
        assert getattr(getattr(lib, name), "fn", getattr(lib, name)) is fn, name      # the proxy calls this very function
        assert (name in _lib.SYMBOLS) == (res == "int") and (name in _lib.SYMBOLS_OTHER) == (res == "long long"), name
    # kinds: pointers of every spelling are c_void_p, scalars keep theirs
    vp, ci, cf, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
    assert list(lib._cdll.sc_vis_frames.argtypes) == [vp, ll, ci, ci, cf, cf, vp, vp]
    assert list(lib._cdll.sc_basic_block_forward.argtypes) == [vp, vp]
    assert list(lib._cdll.sc_conv3x3_pack_multi.argtypes) == [vp, ci, vp, ll, vp]
    assert lib._cdll.sc_silhouette_rays.argtypes[5] is ctypes.c_double


def test_header_reader_refuses_what_it_does_not_understand():
    from shapeclipper_amd import _lib
    ok = "int sc_a(const float* x, int n, void* stream);\nlong long sc_b(void);\n"
    sig = _lib.read_signatures(ok)
    assert sig == {"sc_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]), "sc_b": (ctypes.c_longlong, [])}
    for bad in ("float sc_c(int n);", "int sc_d(short n);", "int sc_e(unsigned n);", "struct sc_t { int a; };", "int sc_f(int n)"):
        with pytest.raises(RuntimeError, match="unrecognised"):
            _lib.read_signatures(ok + bad + "\nint sc_z(int n);")


def test_size_queries_return_long_long_and_wrong_argument_kinds_raise():
    from shapeclipper_amd import _lib
    lib = _lib.load()
    assert "sc_sdf_stream_pack_bytes" in _lib.SYMBOLS_OTHER and lib.sc_sdf_stream_pack_bytes.restype is ctypes.c_longlong
    assert lib.sc_sdf_stream_pack_bytes() == 331776            # the header's figure
    n = lib.sc_conv3x3_pack_floats(64, 64, 56)
    assert n > 0 and lib.sc_conv3x3_pack_floats(ctypes.c_int(64), ctypes.c_int(64), ctypes.c_int(56)) == n      # wrapped scalars still pass
    for bad in ("56", 56.0, None):
        with pytest.raises(ctypes.ArgumentError):
            lib.sc_conv3x3_pack_floats(64, 64, bad)
    with pytest.raises((ctypes.ArgumentError, TypeError)):      # the argument count is checked too
        lib.sc_conv3x3_pack_floats(64, 64)


def test_block_args_mirror_the_header_struct():
    from shapeclipper_amd import ops
    body = re.search(r"typedef struct sc_block_args \{(.*?)\} sc_block_args;", _header_text(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/|//[^\n]*", " ", body, flags=re.S)
    fields = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        kind = "float" if stmt.startswith("float ") and "*" not in stmt else "int" if stmt.startswith("int ") and "*" not in stmt else "ptr"
        assert kind != "ptr" or "*" in stmt, stmt
        fields += [(name, kind) for name in re.findall(r"(\w+)\s*(?:,|$)", stmt)]
    assert [k for _, k in fields] == ["ptr"] * 34 + ["int"] * 7 + ["float"] * 4
    ctype = {"ptr": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float}
    assert [(n, t) for n, t in ops.BlockArgs._fields_] == [(n, ctype[k]) for n, k in fields]
    assert ctypes.sizeof(ops.BlockArgs) == 34 * 8 + 7 * 4 + 4 * 4 + 4        # 316 bytes of fields, padded to the pointers' alignment


def test_scratch_cache_is_one_dict_keyed_by_tag_device_and_stream(monkeypatch):
    """ops._scratch without a GPU: the stream and device queries are replaced as in the device-guard test and torch.empty allocates
    on the host."""
    import torch
    from shapeclipper_amd import _lib, ops
    stream, empty = [77], torch.empty
    monkeypatch.setattr(torch._C, "_cuda_getCurrentRawStream", lambda dev: stream[0] + dev, raising=False)
    monkeypatch.setattr(torch._C, "_cuda_getDevice", lambda: 1, raising=False)
    monkeypatch.setattr(torch, "empty", lambda n, device, dtype: empty(n, dtype=dtype))
    monkeypatch.setattr(ops, "_SCRATCH", {})
    dev = torch.device("cuda", 1)
    a = ops._scratch("rowsum", dev, 100)
    assert a.numel() == 100 and a.dtype == torch.float32
    assert ops._scratch("rowsum", dev, 100) is a and ops._scratch("rowsum", dev, 10) is a       # same key: same buffer, never shrinks
    b = ops._scratch("rowsum", dev, 101)                                                          # a larger request grows it
    assert b is not a and b.numel() == 101 and ops._scratch("rowsum", dev, 100) is b
    c = ops._scratch("park", dev, 100)                                                            # another tag
    stream[0] = 99
    d = ops._scratch("rowsum", dev, 100)                                                          # another stream
    e = ops._scratch("rowsum", torch.device("cuda", 0), 100)                                      # another device
    assert len({id(t) for t in (b, c, d, e)}) == 4
    assert sorted(ops._SCRATCH, key=repr) == sorted([("rowsum", 1, 78), ("park", 1, 78), ("rowsum", 1, 100), ("rowsum", 0, 99)], key=repr)
    assert all(v.dtype == torch.float32 for v in ops._SCRATCH.values())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops._scratch("rowsum", torch.device("cpu"), 4)

    class FakeCudaTensor:
        is_cuda = True
        def __init__(self, dev): self._dev = dev
        def is_contiguous(self): return True
        def get_device(self): return self._dev
        def data_ptr(self): return 4096

    # the device ptr() remembers survives a scratch lookup: the launch's own stream() still judges the call's tensors
    _lib.ptr(FakeCudaTensor(0))
    ops._scratch("rowsum", dev, 100)
    with pytest.raises(RuntimeError, match="tensor on cuda:0 but the current device is cuda:1"):
        _lib.stream()
    _lib.ptr(FakeCudaTensor(1))
    ops._scratch("park", dev, 100)
    assert _lib.stream().value == 100


def test_stream_image_lives_and_dies_with_its_pack(monkeypatch):
    """ops._sdf_stream_image without a GPU (library, pointers and stream replaced): one pack launch per (pack, version, stream), packs
    that alternate keep their images, and nothing but the pack's owner keeps the pack alive."""
    import gc
    import weakref
    import torch
    from shapeclipper_amd import _lib, ops

    class FakeLib:
        packs = 0
        def sc_sdf_stream_pack_bytes(self): return 16
        def sc_sdf_stream_pack(self, w, img, stream):
            FakeLib.packs += 1
            return 0

    stream, empty = [5], torch.empty
    monkeypatch.setattr(_lib, "load", lambda: FakeLib())
    monkeypatch.setattr(_lib, "ptr", lambda t: 0)
    monkeypatch.setattr(_lib, "stream", lambda: stream[0])
    monkeypatch.setattr(_lib, "raw_stream", lambda device=None: stream[0])
    monkeypatch.setattr(torch, "empty", lambda n, device, dtype: empty(n, dtype=dtype))
    monkeypatch.setattr(ops, "_stream_imgs", {})
    a, b = torch.zeros(8), torch.zeros(8)
    ia, ib = ops._sdf_stream_image(a), ops._sdf_stream_image(b)
    assert FakeLib.packs == 2 and ia is not ib and ia.dtype == torch.uint8 and ia.numel() == 16
    for _ in range(3):                                     # two packs alternating on one stream: no re-pack
        assert ops._sdf_stream_image(a) is ia and ops._sdf_stream_image(b) is ib
    assert FakeLib.packs == 2
    a.add_(1)                                              # a new version of the pack: packed again
    assert ops._sdf_stream_image(a) is not ia and FakeLib.packs == 3
    stream[0] = 6                                          # another stream: the image was not written on it
    ops._sdf_stream_image(a)
    assert FakeLib.packs == 4 and len(ops._stream_imgs) == 2
    alive = weakref.ref(a)
    del a, ia
    gc.collect()
    assert alive() is None and len(ops._stream_imgs) == 1  # the cache held the pack weakly and dropped its entry with it
    del b
    gc.collect()
    assert not ops._stream_imgs
