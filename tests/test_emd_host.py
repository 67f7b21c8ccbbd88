"""The Earth Mover's Distance without a GPU: the numpy restatement tests/emd_ref.py of sc_emd3d_match against the exact optimum of scipy's
linear_sum_assignment, options.emd_settings, and the refusals of ops.emd_match that are made before the device is looked at."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emd_ref as ref  # noqa: E402

EPS = 1e-4


def _inputs():
    return {"sphere_cube_64": ref.sphere_cube(64, seed=0), "sphere_cube_256": ref.sphere_cube(256, seed=0),
            "lattice_64": ref.lattice_reverse(), "permuted_192": ref.permuted_noise(192)}


# ---- the restatement against the exact optimum -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere_cube_64", "sphere_cube_256", "lattice_64", "permuted_192"])
def test_restatement_against_the_exact_optimum(name):
    """converged, a permutation, epsilon-complementary slackness in float64 with the DERIVED rounding slack delta = 8 * 2^-24 * (max c +
    max p) -- the five fp32 roundings that form a bid each err by at most 2^-24 of a magnitude at most max c + max p -- and hence
    exact <= emd <= exact + eps + delta.  (Measured: the slackness exceeds eps by at most 9.5e-8, delta is about 1.2e-6, the gap to the
    optimum is at most 1.6e-6.)"""
    a, b = _inputs()[name]
    n = a.shape[0]
    assert a.shape == b.shape == (n, 3) and a.dtype == b.dtype == np.float32
    r = ref.emd_match_one(a, b, eps=EPS)
    assert r.converged == 1 and r.rounds > 0
    assert sorted(r.assignment.tolist()) == list(range(n))
    c = ref.cost_matrix(a, b)
    assert np.array_equal(r.cost, c[np.arange(n), r.assignment])
    delta = ref.slack_delta(c, r.price)
    excess = ref.slackness_excess(a, b, r.assignment, r.price)
    exact, _ = ref.exact_emd(a, b)
    print("%s: rounds %d, slackness %.6e (eps + delta %.6e), emd - optimum %.3e" % (name, r.rounds, excess, EPS + delta, r.emd - exact))
    assert excess <= EPS + delta
    assert exact <= r.emd <= exact + EPS + delta
    assert r.emd == r.cost.astype(np.float64).cumsum()[-1] / n                       # the ascending float64 sum


def test_tie_rules():
    """Two coincident persons midway between two objects: both prefer object 0 (the lowest j among the maxima of w) and bid the same
    b = 0 + ((w1 - w2) + e) = 0.25 for it; the lowest person wins."""
    a = np.zeros((2, 3), np.float32)
    b = np.array([[1, 0, 0], [-1, 0, 0]], np.float32)
    r = ref.emd_match_one(a, b, max_rounds=1)
    assert r.rounds == 1 and r.converged == 0
    assert r.price.tolist() == [0.25, 0.0] and r.assignment.tolist() == [0, 1]        # person 1 takes the unowned object by the fallback
    r = ref.emd_match_one(a, b)
    assert r.converged == 1 and sorted(r.assignment.tolist()) == [0, 1] and r.emd == 1.0
    la, lb = ref.lattice_reverse()
    c = ref.cost_matrix(la, lb)
    assert max((row == row.min()).sum() for row in c) > 1       # the lattice case does meet exact ties in a first bid


def test_eps_list():
    e = ref.eps_list()
    assert e.dtype == np.float32 and len(e) == 7 and e[0] == np.float32(0.25) and e[-1] == np.float32(1e-4)
    assert all(e[k + 1] == e[k] / np.float32(4) for k in range(5)) and e[5] > e[6]
    assert ref.eps_list(0.25, 0.25).tolist() == [0.25]
    from shapeclipper_amd import ops
    for eps, start in ((1e-4, 0.25), (0.25, 0.25), (3e-7, 0.2), (1e-3, 1.0)):
        assert [np.float32(x) for x in ops.emd_eps_list(eps, start)] == list(ref.eps_list(eps, start))


def test_max_rounds_fallback_and_non_finite_input():
    a, b = ref.sphere_cube(64)
    r = ref.emd_match_one(a, b, max_rounds=5)
    assert r.converged == 0 and r.rounds == 5 and sorted(r.assignment.tolist()) == list(range(64))
    full = ref.emd_match_one(a, b)
    assert ref.emd_match_one(a, b, max_rounds=int(full.rounds)).converged == 1           # ending in exactly max_rounds rounds is converged
    assert ref.emd_match_one(a, b, max_rounds=int(full.rounds) - 1).converged == 0
    a = a.copy()
    a[3, 1] = np.nan
    r = ref.emd_match_one(a, b)
    assert r.assignment.tolist() == list(range(64)) and r.rounds == 0 and r.converged == 0 and np.isnan(r.emd)
    assert not r.cost.any() and not r.price.any()


# ---- options.emd_settings --------------------------------------------------------------------------------------------------------------
def _opt(**ev):
    from shapeclipper_amd.utils.util import EasyDict as edict
    return edict(dict(eval=dict(ev)))


def test_emd_settings():
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.utils.util import EasyDict as edict
    assert options.emd_settings(edict()) is None and options.emd_settings(_opt()) is None          # absent means off
    assert options.emd_settings(_opt(emd=False)) is None
    assert options.emd_settings(_opt(emd_points=128, emd_eps=1e-3)) is None                        # settings alone switch nothing on
    assert options.emd_settings(_opt(emd=True)) == (1024, 1e-4)
    assert options.emd_settings(_opt(emd=True, emd_points=2, emd_eps=0.25)) == (2, 0.25)
    assert options.emd_settings(_opt(emd=True, emd_points=2048, emd_eps="1e-3")) == (2048, 1e-3)   # what --eval.emd_eps=1e-3 parses to
    parsed = options.parse_arguments(["--eval.emd", "--eval.emd_points=128", "--eval.emd_eps=1e-3"])
    assert options.emd_settings(parsed) == (128, 1e-3)
    assert options.emd_settings(options.parse_arguments(["--eval.emd!"])) is None
    bad = [dict(emd=1), dict(emd="yes"), dict(emd_points=1), dict(emd_points=2049), dict(emd_points=128.0), dict(emd_points=True),
           dict(emd_points="many"), dict(emd_eps=0), dict(emd_eps=0.0), dict(emd_eps=-1e-4), dict(emd_eps=0.26), dict(emd_eps=True),
           dict(emd_eps="small"), dict(emd_eps=float("nan")), dict(emd_eps=None)]
    for on in (False, True):                                    # a bad value raises with the switch off too
        for b in bad:
            with pytest.raises(ValueError):
                options.emd_settings(_opt(**dict(dict(emd=on), **b)))
    assert "emd" not in options.HIP                             # an evaluation setting, not a hip.* switch


# ---- ops.emd_match: the refusals that need no device -------------------------------------------------------------------------------------
def test_emd_match_refusals():
    from shapeclipper_amd import ops
    x = torch.zeros(2, 8, 3)
    with pytest.raises(ValueError):
        ops.emd_match(x, torch.zeros(2, 9, 3))                  # unequal n
    with pytest.raises(ValueError):
        ops.emd_match(x, torch.zeros(3, 8, 3))                  # unequal B
    with pytest.raises(ValueError):
        ops.emd_match(torch.zeros(8, 3), torch.zeros(8, 3))     # not [B,n,3]
    with pytest.raises(ValueError):
        ops.emd_match(torch.zeros(2, 8, 2), torch.zeros(2, 8, 2))
    with pytest.raises(ValueError):
        ops.emd_match(torch.zeros(1, 1, 3), torch.zeros(1, 1, 3))
    with pytest.raises(ValueError):
        ops.emd_match(torch.zeros(1, 2049, 3), torch.zeros(1, 2049, 3))
    with pytest.raises(ValueError):
        ops.emd_match(x, x, eps=0.5, eps_start=0.25)            # eps > eps_start
    with pytest.raises(ValueError):
        ops.emd_match(x, x, eps=0.0)
    with pytest.raises(ValueError):
        ops.emd_match(x, x, eps=float("nan"))
    with pytest.raises(ValueError):
        ops.emd_match(x, x, eps_start=float("inf"))
    with pytest.raises(ValueError):
        ops.emd_match(x, x, eps=1e-30, eps_start=1e30)          # more phases than the kernel takes
    with pytest.raises(ValueError):
        ops.emd_match(x, x, max_rounds=0)
    with pytest.raises(TypeError):
        ops.emd_match(x.double(), x)
    with pytest.raises(TypeError):
        ops.emd_match(x, x.double())
    with pytest.raises(TypeError):
        ops.emd_match(x.numpy(), x)
    with pytest.raises(TypeError):
        ops.emd_match(x, x, max_rounds=2.5)
    # host tensors that pass every check above: what the ICP entry points raise for them
    from shapeclipper_amd import _lib
    with pytest.raises(RuntimeError, match="no CPU fallback") as e:
        ops.emd_match(x, x)
    assert str(e.value) == _lib.NO_CPU
    with pytest.raises(RuntimeError) as e2:
        ops.icp_apply(x, torch.eye(4, dtype=torch.float64).repeat(2, 1, 1))
    assert str(e2.value) == str(e.value)
    assert ops.EmdResult._fields == ("assignment", "cost", "price", "emd", "rounds", "converged")


def test_header_declares_the_entry_point_and_the_makefile_builds_it_uncontracted():
    from shapeclipper_amd import _lib
    import ctypes
    res, args = _lib.SIGNATURES["sc_emd3d_match"]
    assert res is ctypes.c_int and len(args) == 14 and args[2:4] == [ctypes.c_int, ctypes.c_int] and args[6] is ctypes.c_int
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    mk = open(os.path.join(root, "shapeclipper_amd", "csrc", "Makefile")).read()
    assert "build/emd3d.o: EXTRA := -ffp-contract=off" in mk
    hdr = open(_lib.HEADER_PATH).read()
    from shapeclipper_amd import ops
    assert "#define SC_EMD3D_MAX_POINTS %d\n" % ops.EMD_MAX_POINTS in hdr and "#define SC_EMD3D_MAX_PHASES %d\n" % ops.EMD_MAX_PHASES in hdr
    assert ref.EPS_LIST_MAX == ops.EMD_MAX_PHASES
