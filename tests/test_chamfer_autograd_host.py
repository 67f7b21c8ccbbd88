"""dist_chamfer_3D without a GPU: it imports quietly, refuses CPU tensors and a misspelt BACKWARD, and the ordered backward's three
C-ABI entry points are declared and bound."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("sc_chamfer3d_backward_ordered", "sc_chamfer3d_backward_ordered_workspace_bytes", "sc_chamfer3d_backward_ordered_chunk")


def test_import_is_quiet_and_does_not_pull_the_oracle():
    code = ("import sys; sys.path.insert(0, %r); import dist_chamfer_3D as d; "
            "assert d.BACKWARD == 'ordered'; assert callable(d.chamfer_3DDist) and hasattr(d.chamfer_3DFunction, 'apply'); "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]; assert not bad, bad" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr
    assert r.stdout == "" and r.stderr == ""


def test_source_does_not_name_the_oracle():
    with open(os.path.join(ROOT, "dist_chamfer_3D.py")) as f:
        text = f.read()
    assert "oracle" not in text and "print(" not in text


def test_cpu_tensors_raise():
    import dist_chamfer_3D
    a, b = torch.rand(1, 5, 3), torch.rand(1, 7, 3)
    with pytest.raises(RuntimeError):
        dist_chamfer_3D.chamfer_3DDist()(a, b)
    with pytest.raises(RuntimeError):
        dist_chamfer_3D.chamfer_3DFunction.apply(a.requires_grad_(True), b)


def test_unknown_backward_raises_value_error(monkeypatch):
    import dist_chamfer_3D
    monkeypatch.setattr(dist_chamfer_3D, "BACKWARD", "nonsense")
    with pytest.raises(ValueError):
        dist_chamfer_3D.chamfer_3DDist()(torch.rand(1, 5, 3), torch.rand(1, 7, 3))


def test_new_entry_points_are_declared_and_bound():
    import ctypes
    from shapeclipper_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert _lib.SIGNATURES[NEW[1]][0] is ctypes.c_longlong and len(_lib.SIGNATURES[NEW[0]][1]) == 13


def test_chunk_and_workspace_queries_are_host_only():
    from shapeclipper_amd import _lib
    lib = _lib.load()
    chunk = lib.sc_chamfer3d_backward_ordered_chunk()
    assert chunk >= 64 and chunk % 64 == 0
    size = lib.sc_chamfer3d_backward_ordered_workspace_bytes
    assert size(0, 10, 10) == 0 and size(1, 0, 10) == 0
    assert 0 < size(1, 100, 50) < size(2, 100, 50)
    assert size(1, 100, 50) == size(1, 50, 100)          # both directions are always carved
