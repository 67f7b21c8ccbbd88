"""`--hip.surface_render` without a GPU: the three options, the argument checks of ops.ray_first_crossing / ops.ray_bracket_step, the
header's declarations and their binding, what Renderer.render_surface refuses, and the numpy restatement the GPU tests compare against
(tests/surface_hit_ref.py) on rays worked out by hand."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import surface_hit_ref as ref  # noqa: E402

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32


def _opt(*extra):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_surface", "--output_root=/tmp/sc_pytest",
                                                *extra]), verbose=False)


def test_options_default_parse_and_refuse_out_of_range_values():
    from shapeclipper_amd.utils import options
    from shapeclipper_amd.model import runner
    d = options.HIP_DEFAULTS["hip"]
    assert d["surface_render"] is False and d["surface_refine"] == 3 and d["surface_scale"] == 1
    o = _opt()
    assert (o.hip.surface_render, o.hip.surface_refine, o.hip.surface_scale) == (False, 3, 1) and not runner._surface_render(o)
    o = _opt("--hip.surface_render", "--hip.surface_refine=0", "--hip.surface_scale=4")
    assert (o.hip.surface_render, o.hip.surface_refine, o.hip.surface_scale) == (True, 0, 4) and runner._surface_render(o)
    assert _opt("--hip.surface_refine=16").hip.surface_refine == 16
    assert _opt("--hip.surface_render!").hip.surface_render is False
    for bad in ("--hip.surface_refine=-1", "--hip.surface_refine=17", "--hip.surface_refine=2.5", "--hip.surface_scale=0", "--hip.surface_scale=5",
                "--hip.surface_scale=1.5", "--hip.surface_scale=true"):
        with pytest.raises(ValueError, match="hip.surface_"):
            _opt(bad)


def test_ops_refuse_cpu_tensors_wrong_dtypes_shapes_and_sample_counts():
    from shapeclipper_amd import ops
    z, s = torch.zeros(5, 64), torch.zeros(5 * 64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ray_first_crossing(z, s)
    for S in (48, 16, 288, 65):
        with pytest.raises(ValueError, match="samples per ray"):
            ops.ray_first_crossing(torch.zeros(5, S), torch.zeros(5 * S))
    for bad_z, bad_s in ((z.double(), s), (z, s.double()), (z, s.half()), (z, s.view(5, 64)), (z, s[:-1]), (z.view(-1), s), (z[None], s)):
        with pytest.raises(ValueError):
            ops.ray_first_crossing(bad_z, bad_s)
    f = lambda: torch.zeros(5)
    br = ops.RayBracket(f(), f(), f(), f(), torch.zeros(5, dtype=torch.int32))
    cam, d = torch.zeros(5, 3), torch.zeros(5, 3)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ray_bracket_step(br, cam, d)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.ray_bracket_step(br, cam, d, f(), f())
    for args in ((br, cam[:4], d), (br, cam, d.view(-1)), (br, cam.double(), d), (br, cam, d, f().double(), f()), (br, cam, d, f(), f()[:4]),
                 (br, cam, d, f(), None), (br, cam, d, None, f()), (br._replace(hit=torch.zeros(5, dtype=torch.int64)), cam, d),
                 (br._replace(f_lo=torch.zeros(4)), cam, d), (br._replace(t_hi=torch.zeros(10)[::2]), cam, d), (tuple(br), cam, d)):
        with pytest.raises(ValueError):
            ops.ray_bracket_step(*args)


def test_header_declares_both_entry_points_and_lib_binds_them():
    from shapeclipper_amd import _lib
    text = open(os.path.join(ROOT, "include", "shapeclipper_hip.h")).read()
    assert re.search(r"^int sc_ray_first_crossing\(const float\* z_vals, const float\* sdf, int n_rays, int n_samples, float iso, float\* t_lo, "
                     r"float\* t_hi,\s+float\* f_lo, float\* f_hi, int32_t\* hit, void\* stream\);", text, flags=re.M)
    assert re.search(r"^int sc_ray_bracket_step\(const float\* cam_loc, const float\* ray_dirs, const float\* f_new, const float\* t_prev, int n_rays, "
                     r"float iso,\s+float\* t_lo, float\* t_hi, float\* f_lo, float\* f_hi, const int32_t\* hit, float\* t, float\* points, "
                     r"void\* stream\);", text, flags=re.M)
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["sc_ray_first_crossing"] == (I, [P, P, I, I, Fl, P, P, P, P, P, P])
    assert _lib.SIGNATURES["sc_ray_bracket_step"] == (I, [P, P, P, P, I, Fl, P, P, P, P, P, P, P, P])
    assert "sc_ray_first_crossing" in _lib.SYMBOLS and "sc_ray_bracket_step" in _lib.SYMBOLS
    comment = text[text.index("Surface render (csrc/surface_hit.hip)"):text.index("int sc_ray_first_crossing")]
    for phrase in ("f_i = sdf_i - iso", "f_0 <= 0", "SMALLEST i", "f_i > 0 and f_{i+1} <= 0", "NaN", "w = f_lo / d", "w = 0.5",
                   "t_lo + w * (t_hi - t_lo)", "cam_loc + t * ray_dirs", "hit != 1:  t = t_lo", "no atomics"):
        assert phrase in comment, phrase
    lib = _lib.load()
    assert callable(lib.sc_ray_first_crossing) and callable(lib.sc_ray_bracket_step)
    # refused before anything is launched: no device is needed to see the status
    null, st = ctypes.c_void_p(0), ctypes.c_void_p(0)
    assert lib.sc_ray_first_crossing(null, null, 4, 48, 0.0, null, null, null, null, null, st) == 1
    assert lib.sc_ray_first_crossing(null, null, 4, 64, 0.0, null, null, null, null, null, st) == 1
    assert lib.sc_ray_first_crossing(null, null, 0, 64, 0.0, null, null, null, null, null, st) == 0
    assert lib.sc_ray_bracket_step(null, null, null, null, 4, 0.0, null, null, null, null, null, null, null, st) == 1
    assert lib.sc_ray_bracket_step(null, null, null, null, 0, 0.0, null, null, null, null, null, null, null, st) == 0


def _renderer(o):
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    return Renderer(o, SDFNetwork(o), RGBNetwork(o))


def test_render_surface_refuses_what_the_hip_chain_does_not_take():
    B = 2
    pose, intr, sd, z = torch.zeros(B, 3, 4), torch.eye(3).repeat(B, 1, 1), torch.ones(B), torch.zeros(B, 64)
    for extra in (["--render.n_samples_uniform=48"], ["--arch.impl_sdf.n_channels=128"]):          # eager: sample count / architecture
        o = _opt(*extra)
        o.H = o.W = 16
        r = _renderer(o)
        assert r.eager
        with pytest.raises(NotImplementedError):
            r.render_surface(o, pose, intr, sd, z, z)
        with pytest.raises(NotImplementedError):
            r.render_views(o, pose, intr, z, z, surface=True)
    o = _opt()
    o.H = o.W = 16
    r = _renderer(o)
    assert not r.eager
    o.camera.model = "orthographic"
    with pytest.raises(NotImplementedError):
        r.render_surface(o, pose, intr, sd, z, z)
    o.camera.model = "perspective"
    for kw in (dict(scale=0), dict(scale=5), dict(scale=1.0), dict(scale=True), dict(n_refine=-1), dict(n_refine=17), dict(n_refine=1.0)):
        with pytest.raises(ValueError, match="render_surface takes an integer"):
            r.render_surface(o, pose, intr, sd, z, z, **kw)
    o.H, o.W = 6, 6                                                         # 36 rays: not a multiple of 16 (144 at scale 2 is)
    with pytest.raises(ValueError, match="multiple of 16"):
        r.render_surface(o, pose, intr, sd, z, z)
    with pytest.raises(ValueError, match="multiple of 16"):
        r.render_surface(o, pose, intr, sd, z, z, scale=3)
    # training with render.normal_model: surface keeps raising, as the reference does
    o = _opt("--render.normal_model=surface")
    with pytest.raises(NotImplementedError):
        _renderer(o)


# ---- the numpy restatement on rays worked out by hand -------------------------------------------------------------------------------------
def _z(n, S):
    return np.tile(np.arange(S, dtype=F) * F(0.25) + F(4.0), (n, 1))       # z_i = 4 + i / 4, exact


def test_restatement_first_crossing_by_hand():
    S = 32
    f = np.ones((6, S), F)
    f[0, 5:] = -2.0                                   # enters at (4,5)
    f[1, 0] = -1.0                                    # starts inside
    # row 2 never enters
    f[3, 2:4] = -1.0; f[3, 9:] = -3.0                 # enters at (1,2), leaves at (3,4), enters again at (8,9): the first wins
    f[4, 6] = np.nan; f[4, 7:] = -1.0                 # the only entry is hidden by a NaN
    f[5, 31] = 0.0                                    # touches zero at the last sample
    br = ref.first_crossing(_z(6, S), f.reshape(-1))
    assert br.hit.tolist() == [1, 2, 0, 1, 0, 1] and br.hit.dtype == np.int32
    assert br.t_lo.tolist() == [5.0, 4.0, 4.0, 4.25, 4.0, 11.5] and br.t_hi.tolist() == [5.25, 4.0, 4.0, 4.5, 4.0, 11.75]
    assert br.f_lo.tolist() == [1.0, -1.0, 1.0, 1.0, 1.0, 1.0] and br.f_hi.tolist() == [-2.0, -1.0, 1.0, -1.0, 1.0, 0.0]
    # iso = 0.5 moves the solid: 1 - 0.5 > 0 stays outside, 0 - 0.5 and below are inside
    br = ref.first_crossing(_z(6, S), f.reshape(-1), iso=0.5)
    assert br.hit.tolist() == [1, 2, 0, 1, 0, 1] and br.f_lo.tolist() == [0.5, -1.5, 0.5, 0.5, 0.5, 0.5] and br.f_hi[5] == -0.5
    # a seam pair at S = 128
    f = np.ones((1, 128), F)
    f[0, 64:] = -1.0
    br = ref.first_crossing(_z(1, 128), f)
    assert (int(br.hit[0]), float(br.t_lo[0]), float(br.t_hi[0])) == (1, 4.0 + 63 / 4, 4.0 + 64 / 4)
    # every crafted row of the GPU tests gives what its name says
    for S in (32, 64, 96, 128, 256):
        for iso in (0.0, 0.5):
            z, sdf, want = ref.crossing_case(S, iso=iso)
            assert z.shape == (130, S) and sdf.shape == (130 * S,) and len(want) >= 20
            br = ref.first_crossing(z, sdf, iso)
            for k, (hit, i) in enumerate(want):
                assert int(br.hit[k]) == hit, (S, iso, k, ref.crafted_rows(S)[k][0])
                if i is not None:
                    assert br.t_lo[k] == z[k, i] and br.t_hi[k] == z[k, i + 1], (S, k)
                else:
                    assert br.t_lo[k] == z[k, 0] and br.t_hi[k] == z[k, 0], (S, k)
            assert {0, 1, 2} <= set(br.hit[len(want):].tolist())
        names = [n for n, _, _ in ref.crafted_rows(S)]
        assert sum(n.startswith("seam") for n in names) == 2 * sum(s + 1 < S for s in ref.SEAMS)


def test_restatement_bracket_step_by_hand():
    one = lambda *v: np.array(v, F)
    cam, d = np.array([[1.0, 2.0, 3.0]] * 4, F), np.array([[0.0, 0.5, -1.0]] * 4, F)
    br = ref.Bracket(one(4, 4, 4, 4), one(5, 5, 4, 4), one(1, 3, 1, -1), one(-1, -1, 1, -1), np.array([1, 1, 0, 2], np.int32))
    nb, t, p = ref.bracket_step(br, cam, d)
    assert t.tolist() == [4.5, 4.75, 4.0, 4.0]                     # w = 1/2, 3/4; misses and inside starts stay at t_lo
    assert p[0].tolist() == [1.0, 4.25, -1.5] and p[1].tolist() == [1.0, 4.375, -1.75]
    assert all(ref.same_bits(a, b) for a, b in zip(nb, br))         # no f_new: the bracket is untouched
    # f_new > 0 moves the lower end, <= 0 (zero included) the upper end, NaN nothing; hit != 1 rays never move
    nb, t2, _ = ref.bracket_step(br, cam, d, one(0.5, 0.0, -9, 9), t)
    assert nb.t_lo.tolist() == [4.5, 4.0, 4.0, 4.0] and nb.f_lo.tolist() == [0.5, 3.0, 1.0, -1.0]
    assert nb.t_hi.tolist() == [5.0, 4.75, 4.0, 4.0] and nb.f_hi.tolist() == [-1.0, 0.0, 1.0, -1.0]
    assert t2[0] == F(4.5) + (F(0.5) / (F(0.5) - F(-1.0))) * (F(5.0) - F(4.5)) and t2[2:].tolist() == [4.0, 4.0]
    assert t2[1] == 4.75                                           # f_hi = 0: w = 1, the query is t_hi itself
    nb2, t3, _ = ref.bracket_step(br, cam, d, one(np.nan, np.nan, np.nan, np.nan), t)
    assert all(ref.same_bits(a, b) for a, b in zip(nb2, br)) and ref.same_bits(t3, t)
    # the safeguard: an overflowing difference and an infinite end bisect; a NaN end bisects too
    br = ref.Bracket(one(4, 4, 4), one(5, 5, 5), one(3e38, np.inf, 1), one(-3e38, -1, np.nan), np.array([1, 1, 1], np.int32))
    _, t, _ = ref.bracket_step(br, cam[:3], d[:3])
    assert t.tolist() == [4.5, 4.5, 4.5]
    # f_hi = -Inf: w = f_lo / Inf... the difference is not finite, so it bisects instead of standing still at t_lo
    br = ref.Bracket(one(4), one(5), one(1), one(-np.inf), np.array([1], np.int32))
    assert ref.bracket_step(br, cam[:1], d[:1])[1].tolist() == [4.5]
    # iso shifts f_new
    br = ref.Bracket(one(4), one(5), one(1), one(-1), np.array([1], np.int32))
    nb, _, _ = ref.bracket_step(br, cam[:1], d[:1], one(0.75), one(4.5), iso=0.5)
    assert nb.t_lo.tolist() == [4.5] and nb.f_lo.tolist() == [0.25]
    # the step case of the GPU tests is what its docstring says
    br, cam, d = ref.step_case()
    assert set(br.hit.tolist()) == {0, 1, 2} and len(br.hit) == 130
    m = br.hit == 1
    assert (br.f_lo[m] > 0).all() and (br.f_hi[m] <= 0).all() and (br.t_lo[m] <= br.t_hi[m]).all()
    assert not np.isfinite(br.f_lo[0] - br.f_hi[0]) and np.isfinite(br.f_lo[0]) and np.isfinite(br.f_hi[0])
    _, t, _ = ref.bracket_step(br, cam, d)
    assert t[0] == br.t_lo[0] + F(0.5) * (br.t_hi[0] - br.t_lo[0]) and t[4] == br.t_lo[4] and t[3] == br.t_hi[3]
