"""`--hip.largest_component` without a GPU: the option, the argument checks of ops.level_largest_component, the header's declarations,
and the numpy restatement the GPU tests compare against (tests/level_components_ref.py) on three grids worked out by hand."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import level_components_ref as ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_option_defaults_to_off_and_parses():
    from shapeclipper_amd.utils import options
    assert options.HIP_DEFAULTS["hip"]["largest_component"] is False
    assert options.parse_arguments(["--hip.largest_component"]).hip.largest_component is True
    assert options.parse_arguments(["--hip.largest_component!"]).hip.largest_component is False
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_lc", "--output_root=/tmp/sc_pytest"]),
                      verbose=False)
    assert opt.hip.largest_component is False
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_lc", "--output_root=/tmp/sc_pytest",
                                               "--hip.largest_component"]), verbose=False)
    assert opt.hip.largest_component is True
    from shapeclipper_amd.utils import eval_3D
    assert eval_3D.largest_component_enabled(opt) and not eval_3D.largest_component_enabled(options.edict(hip=options.edict()))


def test_op_refuses_cpu_tensors_and_bad_shapes():
    from shapeclipper_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.level_largest_component(torch.zeros(1, 4, 4, 4))
    for bad in (torch.zeros(1, 4, 4, 5), torch.zeros(1, 4, 5, 4), torch.zeros(4, 4, 4), torch.zeros(1, 1, 4, 4, 4)):
        with pytest.raises(ValueError, match="cubic"):
            ops.level_largest_component(bad)
    for bad in (torch.zeros(1, 4, 4, 4, dtype=torch.float64), torch.zeros(1, 4, 4, 4, dtype=torch.float16), torch.zeros(1, 4, 4, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="fp32"):
            ops.level_largest_component(bad)
    with pytest.raises(ValueError, match="grid side"):
        ops.level_largest_component(torch.zeros(1, 1, 1, 1))
    with pytest.raises(ValueError, match="grid side"):
        ops.level_largest_component(torch.zeros(1, 1025, 1025, 1025, device="meta"))


def test_header_declares_the_entry_point_and_its_definition():
    from shapeclipper_amd import _lib
    text = open(os.path.join(ROOT, "include", "shapeclipper_hip.h")).read()
    assert re.search(r"^long long sc_level_largest_component_scratch_bytes\(int n_images, int n_axis\);", text, flags=re.M)
    assert re.search(r"^int sc_level_largest_component\(const float\* level, int n_images, int n_axis, float iso, float\* level_out,", text, flags=re.M)
    assert "sc_level_largest_component" in _lib.SYMBOLS and "sc_level_largest_component_scratch_bytes" in _lib.SYMBOLS_OTHER
    assert len(_lib.SIGNATURES["sc_level_largest_component"][1]) == 10
    comment = text[text.index("Largest connected component"):text.index("long long sc_level_largest_component_scratch_bytes")]
    for phrase in ("level < iso", "6-connectivity", "share a face", "(x * S + y) * S + z", "smallest label", "iso + (iso - level)", "NaN"):
        assert phrase in comment, phrase
    lib = _lib.load()                                       # host-only query: loads without a GPU
    assert lib.sc_level_largest_component_scratch_bytes(1, 65) >= 8 * 65 ** 3 + 16
    assert lib.sc_level_largest_component_scratch_bytes(3, 1024) >= 3 * 8 * 1024 ** 3
    assert lib.sc_level_largest_component_scratch_bytes(1, 1) == 0 and lib.sc_level_largest_component_scratch_bytes(1, 1025) == 0


def _grid(S, voxels, value=-1.0):
    g = np.full((S, S, S), 1.0, np.float32)
    for i, v in enumerate(voxels):
        g[v] = value - 0.25 * i                             # distinct values: the reflection is checked voxel by voxel
    return g


def test_restatement_two_blobs_of_sizes_3_and_2():
    # blob A: (0,0,1) (0,0,2) (0,1,2), labels 1, 2, 6 -> label 1, size 3;  blob B: (3,3,2) (3,3,3), label 62, size 2
    A, B = [(0, 0, 1), (0, 0, 2), (0, 1, 2)], [(3, 3, 2), (3, 3, 3)]
    g = _grid(4, A + B)
    r = ref.largest_component(g)
    assert r["components"] == [(1, 3), (62, 2)]
    assert (r["n_components"], r["inside_voxels"], r["kept_voxels"], r["kept_label"]) == (2, 5, 3, 1)
    want = g.copy()
    want[3, 3, 2], want[3, 3, 3] = 1.75, 2.0                # -(-1.75), -(-2.0)
    assert np.array_equal(r["out"].view(np.int32), want.view(np.int32))
    # iso = 0.5: the same blobs (the background 1.0 stays outside); B is reflected about 0.5
    r = ref.largest_component(g, 0.5)
    want[3, 3, 2], want[3, 3, 3] = 2.75, 3.0
    assert r["components"] == [(1, 3), (62, 2)] and np.array_equal(r["out"], want)
    # the larger blob second: it is kept although its label is larger
    r = ref.largest_component(_grid(4, [(0, 0, 0), (2, 2, 1), (2, 2, 2), (2, 3, 2)]))
    assert r["components"] == [(0, 1), (41, 3)] and (r["kept_label"], r["kept_voxels"]) == (41, 3)
    assert r["out"][0, 0, 0] == 1.0 and r["out"][2, 2, 1] == -1.25


def test_restatement_tie_keeps_the_smaller_label():
    # (0,2,0) (0,2,1): labels 8, 9 -> label 8;  (1,0,0) (2,0,0): labels 16, 32 -> label 16.  Equal sizes: label 8 stays.
    g = _grid(4, [(1, 0, 0), (2, 0, 0), (0, 2, 0), (0, 2, 1)])
    r = ref.largest_component(g)
    assert r["components"] == [(8, 2), (16, 2)]
    assert (r["n_components"], r["inside_voxels"], r["kept_voxels"], r["kept_label"]) == (2, 4, 2, 8)
    want = g.copy()
    want[1, 0, 0], want[2, 0, 0] = 1.0, 1.25
    assert np.array_equal(r["out"], want)


def test_restatement_edge_contact_does_not_connect():
    # (1,1,1) and (1,2,2) share an edge only; (1,1,1) and (2,2,2) a corner only
    for other, label in (((1, 2, 2), 26), ((2, 2, 2), 42)):
        g = _grid(4, [(1, 1, 1), other])
        r = ref.largest_component(g)
        assert r["components"] == [(21, 1), (label, 1)]
        assert (r["n_components"], r["inside_voxels"], r["kept_voxels"], r["kept_label"]) == (2, 2, 1, 21)
        want = g.copy()
        want[other] = 1.25
        assert np.array_equal(r["out"], want)
    # a shared face does connect
    assert ref.largest_component(_grid(4, [(1, 1, 1), (1, 1, 2)]))["components"] == [(21, 2)]


def test_restatement_special_values_and_the_test_grids():
    g = np.full((3, 3, 3), np.float32(1.0))
    g[0, 0, 0], g[0, 0, 2], g[2, 2, 2], g[1, 1, 1] = -np.inf, np.nan, np.inf, -2.0
    g[2, 0, 0] = -3.0
    g[2, 1, 0] = -4.0
    r = ref.largest_component(g)
    assert r["components"] == [(0, 1), (13, 1), (18, 2)] and r["kept_label"] == 18       # NaN and +Inf are outside, -Inf is inside
    assert r["out"][0, 0, 0] == np.inf and r["out"][1, 1, 1] == 2.0 and np.isnan(r["out"][0, 0, 2]) and r["out"][2, 2, 2] == np.inf
    # the grids of the GPU tests are what their names say
    for S in (2, 5, 8, 9, 17, 33):
        m = ref.serpentine_mask(S)
        r = ref.expected("serpentine", S, 0.0, 0)
        assert (r["n_components"], r["kept_voxels"]) == (1, int(m.sum())) and m.sum() >= S * S * S // 4
        assert ref.expected("checker", S, 0.05, 0)["n_components"] == (S ** 3 + 1) // 2
    S = 33
    m = ref.serpentine_mask(S)
    for axis in range(3):                                                   # the path crosses every face plane of the 8 x 8 x 8 tiling
        for k in (8, 16, 24, 32):
            assert (np.take(m, k - 1, axis) & np.take(m, k, axis)).any(), (axis, k)
    p = np.pad(m, 1).astype(np.int32)
    nb = (p[2:, 1:-1, 1:-1] + p[:-2, 1:-1, 1:-1] + p[1:-1, 2:, 1:-1] + p[1:-1, :-2, 1:-1] + p[1:-1, 1:-1, 2:] + p[1:-1, 1:-1, :-2])[m]
    assert int((nb == 1).sum()) == 2 and int((nb > 2).sum()) == 0           # a simple path: two ends, no branch
    for k in range(3):
        t = ref.expected("tie", 9, 0.05, k)
        assert t["n_components"] == 2 and t["kept_voxels"] * 2 == t["inside_voxels"] and t["kept_label"] == min(l for l, _ in t["components"])
        assert ref.expected("none", 9, 0.0, k)["n_components"] == 0 and ref.expected("all", 9, 0.0, k)["kept_voxels"] == 729
        assert ref.expected("one", 17, 0.0, k)["n_components"] == 1
        assert ref.expected("two_balls", 17, 0.05, k)["n_components"] == 2 and ref.expected("ball_floater", 17, 0.0, k)["n_components"] == 2
    n = ref.image("nonfinite", 17, 0.0, 0)
    assert np.isnan(n).sum() > 50 and np.isposinf(n).sum() > 10 and np.isneginf(n).sum() > 10
    assert {int(b) for b in n.view(np.uint32)[np.isnan(n)]} == set(ref.NAN_PAYLOADS)
    for p, lo, hi in ((25, 0.2, 0.3), (31, 0.26, 0.36), (50, 0.45, 0.55)):
        r = ref.expected("random%d" % p, 33, 0.05, 0)
        assert lo < r["inside_voxels"] / 33 ** 3 < hi and r["n_components"] > 50


def test_component_stats_keep_their_names_inside_var():
    """eval_metrics stores the counts as a dict: var (an EasyDict) turns a tuple into a plain list and would lose the field names."""
    from shapeclipper_amd import ops
    from shapeclipper_amd.model import runner
    from shapeclipper_amd.utils.util import EasyDict as edict
    st = ops.ComponentStats(*(torch.tensor([v, v + 1], dtype=torch.int32) for v in (2, 90, 70)))
    var = edict(idx=torch.tensor([5, 6]))
    var.component_stats = st._asdict()
    assert "component_stats" in var and var.component_stats.n_components.tolist() == [2, 3] and var.component_stats.kept_voxels.tolist() == [70, 71]
    assert [c.tolist() for c in runner._component_counts(var)] == [[2, 3], [90, 91], [70, 71]]
