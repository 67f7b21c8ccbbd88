"""The similarity ICP of the evaluation without a GPU: the numpy restatement (tests/icp_ref.py) recovers the known transform of every
test case, and the `--eval.icp*` options parse as documented."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_ref as ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.mark.parametrize("seed", ref.SEEDS)
def test_the_restatement_recovers_every_case(seed):
    for k in range(len(ref.CASES)):
        c = ref.case(seed, k)
        out = ref.align(c["src"], c["dst"], iters=30, scale=c["scale"])
        T = out["transform"]
        err = max(np.abs(T[:3, :3] - c["s0"] * c["R0"]).max(), np.abs(T[:3, 3] - c["t0"]).max(), abs(out["s"] - c["s0"]))
        print("seed %d case %d: worst |error| of s R, t, s = %.3g, objective %.3g -> %.3g" % (seed, k, err, out["objective"][0], out["objective"][-1]))
        assert np.array_equal(out["idx1"], c["inv"])                    # exact final correspondences, both ways
        assert np.array_equal(c["inv"][out["idx2"]], np.arange(len(c["inv"])))
        assert err <= 5e-9
        assert np.array_equal(T[3], [0, 0, 0, 1])


def test_chair_and_cases_are_as_specified():
    pts = ref.chair(1024, np.random.default_rng(0))
    assert pts.dtype == np.float32 and pts.shape == (1024, 3)
    for (lo, hi), sl in zip(ref.BOXES, (slice(0, 512), slice(512, 768), slice(768, 1024))):
        lo, hi = np.float32(lo), np.float32(hi)
        part = pts[sl]
        assert (part >= lo).all() and (part <= hi).all()
        assert ((part == lo) | (part == hi)).any(axis=1).all()          # every point lies on a face of its box
    c = ref.case(2, 3)
    assert np.array_equal(c["dst"][c["inv"]], (c["s0"] * (c["src"].astype(np.float64) @ c["R0"].T) + c["t0"]).astype(np.float32))
    assert abs(np.linalg.norm(c["t0"]) - 0.08) < 1e-15 and abs(np.linalg.det(c["R0"]) - 1) < 1e-14
    assert abs(np.degrees(np.arccos((np.trace(c["R0"]) - 1) / 2)) - 20.0) < 1e-9
    assert len(ref.all_cases()) == 16


def test_degenerate_fits_keep_the_previous_transform():
    rng = np.random.default_rng(5)
    dst = rng.uniform(-1, 1, (60, 3)).astype(np.float32)
    i1, i2 = rng.integers(0, 60, 50).astype(np.int32), rng.integers(0, 50, 60).astype(np.int32)
    same = np.tile(np.float32([0.3, -0.2, 0.7]), (50, 1))
    line = (np.float32([0.25, -0.5, 0.125]) + np.arange(-25, 25, dtype=np.float32)[:, None] * np.float32([2 ** -9, 2 ** -8, -2 ** -9]))
    nan = rng.uniform(-1, 1, (50, 3)).astype(np.float32)
    nan[7, 1] = np.nan
    prev = (np.diag([2.0, 2.0, 2.0, 1.0]), 2.0)
    for src in (same, line, nan):
        T, s = ref.fit(src, dst, i1, i2)
        assert np.array_equal(T, np.eye(4)) and s == 1.0
        T, s = ref.fit(src, dst, i1, i2, prev=prev)
        assert np.array_equal(T, prev[0]) and s == 2.0
    T, s = ref.fit(rng.uniform(-1, 1, (50, 3)).astype(np.float32), dst, i1, i2)
    assert not np.array_equal(T, np.eye(4))


# ---- options ---------------------------------------------------------------------------------------------------------------------------
def _set(tmp_path, *extra):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_icp_options",
                                                "--output_root=%s" % tmp_path, *extra]), verbose=False)


def test_icp_options_absent_means_off_and_defaults(tmp_path):
    from shapeclipper_amd.utils import options
    o = _set(tmp_path)
    assert options.icp_settings(o) is None
    assert "icp" not in o.eval and "icp_iters" not in o.eval and "icp_scale" not in o.eval        # nothing is written into the tree
    o = _set(tmp_path, "--eval.icp")
    assert options.icp_settings(o) == (30, True)
    o = _set(tmp_path, "--eval.icp", "--eval.icp_iters=7", "--eval.icp_scale!")
    assert options.icp_settings(o) == (7, False)
    assert options.icp_settings(_set(tmp_path, "--eval.icp!", "--eval.icp_iters=100")) is None
    assert options.icp_settings(_set(tmp_path, "--eval.icp", "--eval.icp_iters=1")) == (1, True)
    # an option tree built by hand, without an eval node
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert options.icp_settings(edict()) is None


@pytest.mark.parametrize("switch", [(), ("--eval.icp",)])
@pytest.mark.parametrize("bad", ["--eval.icp_iters=0", "--eval.icp_iters=101", "--eval.icp_iters=true", "--eval.icp_iters=1.5",
                                 "--eval.icp_iters=many", "--eval.icp_scale=2", "--eval.icp_scale=yes please"])
def test_icp_options_refuse_bad_values_whether_or_not_the_switch_is_on(tmp_path, bad, switch):
    with pytest.raises(ValueError, match="eval.icp_"):
        _set(tmp_path, bad, *switch)


def test_icp_is_not_a_hip_switch(tmp_path):
    from shapeclipper_amd.utils import options
    assert not any("icp" in row.key for row in options.HIP_TABLE)
    o = _set(tmp_path, "--eval.icp")
    assert not any("icp" in k for k in o.hip)
