"""ops.level_ambient_occlusion (csrc/level_ao.hip) against the numpy restatement tests/level_ao_ref.py: ao and mask bit for bit, with the
bit volume (cell_skip=True) and without, on every case below; an image alone and inside a batch, a permutation of the points, a side
stream, and the refusals.  Every reference is computed once and shared."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(__file__))
import level_ao_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grid_normals(level, verts):
    """The central-difference gradient of the level grid at the grid point nearest to each vertex: any length, zero where the grid is flat."""
    g = np.stack(np.gradient(level.astype(np.float64)), axis=-1)
    i = np.clip(np.rint(verts).astype(np.int64), 0, level.shape[0] - 1)
    return g[i[:, 0], i[:, 1], i[:, 2]].astype(np.float32)


def _shape(name):
    level = dict(sphere=ref.sphere_level, pit=ref.pit_level, two_spheres=ref.two_spheres_level)[name]()
    verts = ref.mc_vertices(name, level)
    return level, verts, _grid_normals(level, verts)


def _case(name):
    """-> dict(level [B,S,S,S], points, normals, image, radius, step, bias, iso)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = dict(radius=4.0, step=0.5, bias=1.0, iso=0.0)
    if name == "s2":                                        # one cell, one sample per ray
        level = np.array([[[0.5, -0.25], [0.75, 0.125]], [[-0.5, 0.25], [1.0, -1.0]]], np.float32)[None]
        points = rng.uniform(-0.2, 1.2, size=(40, 3)).astype(np.float32)
        normals = rng.normal(size=(40, 3)).astype(np.float32)
        return dict(level=level, points=points, normals=normals, image=np.zeros(40, np.int32), **dict(kw, radius=0.25, step=0.25, bias=0.125))
    if name in ("sphere", "pit", "two_spheres"):
        level, verts, normals = _shape(name)
        return dict(level=level[None], points=verts, normals=normals, image=np.zeros(len(verts), np.int32), **kw)
    if name in ("n1", "n3", "n67"):
        level, verts, normals = _shape("two_spheres")
        n = int(name[1:])
        pick = np.linspace(0, len(verts) - 1, n).astype(np.int64)
        return dict(level=level[None], points=verts[pick], normals=normals[pick], image=np.zeros(n, np.int32), **kw)
    if name == "crease":
        level = ref.crease_level(17, 5.0)
        xs = np.arange(5.0, 14.0, 0.25)
        floor = np.stack([xs, np.full_like(xs, 8.3), np.full_like(xs, 5.0)], axis=1)
        wall = np.stack([np.full_like(xs, 5.0), np.full_like(xs, 7.7), xs], axis=1)
        points = np.concatenate([floor, wall]).astype(np.float32)
        normals = np.concatenate([np.tile([[0, 0, 1.0]], (len(xs), 1)), np.tile([[2.5, 0, 0]], (len(xs), 1))]).astype(np.float32)
        return dict(level=level[None], points=points, normals=normals, image=np.zeros(len(points), np.int32), **dict(kw, radius=6.0))
    if name == "batch":                                     # three images, the middle one empty space, points interleaved
        a, va, na = _shape("pit")
        c, vc, nc = _shape("two_spheres")
        empty = np.full_like(a, 0.75)
        n = min(len(va), len(vc), 150)
        points = np.stack([va[:n], va[:n], vc[:n]], axis=1).reshape(-1, 3)
        normals = np.stack([na[:n], na[:n], nc[:n]], axis=1).reshape(-1, 3)
        image = np.tile(np.array([0, 1, 2], np.int32), n)
        return dict(level=np.stack([a, empty, c]), points=points, normals=normals, image=image, **kw)
    if name == "faces":                                     # on the grid's faces, edges and corners, and just outside them
        level, _, _ = _shape("sphere")
        top = np.float32(16.0)
        vals = [np.float32(0.0), np.nextafter(np.float32(0.0), np.float32(-1)), np.float32(-0.0), top, np.nextafter(top, np.float32(17)),
                np.nextafter(top, np.float32(0)), np.float32(8.0), np.float32(15.5)]
        points = np.array([[x, y, z] for x in vals for y in (vals[0], vals[3], vals[6]) for z in (vals[1], vals[4], vals[6], vals[7])], np.float32)
        normals = np.where(points > 8, -1.0, 1.0).astype(np.float32) * rng.uniform(0.2, 1.0, size=points.shape).astype(np.float32)
        # bias 0: the rays start on the faces themselves; the sphere is shifted so that it cuts the grid's faces
        shifted = ref.sphere_level(17, (2.0, 3.0, 14.0), 5.3)
        return dict(level=shifted[None], points=points, normals=normals, image=np.zeros(len(points), np.int32), **dict(kw, bias=0.0, radius=3.0))
    if name == "degenerate":
        level, verts, normals = _shape("sphere")
        nan, inf = np.float32("nan"), np.float32("inf")
        points, normals = verts[:16].copy(), normals[:16].copy()
        points[1, 0], points[3, 2], points[5, 1] = nan, inf, -inf
        normals[7, 1], normals[9, 0], normals[11] = nan, inf, 0.0
        points[14] = (40.0, 8.0, 8.0)                       # far outside the grid
        return dict(level=level[None], points=points, normals=normals, image=np.zeros(16, np.int32), **kw)
    if name == "iso":                                       # the level set 0.7: the spheres are 0.7 larger, the rays start outside it
        level, verts, normals = _shape("two_spheres")
        return dict(level=level[None], points=verts, normals=normals, image=np.zeros(len(verts), np.int32), **dict(kw, iso=0.7, bias=1.5, radius=6.0))
    if name == "nan_level":                                 # NaN grid values: never below iso
        level, verts, normals = _shape("pit")
        level = level.copy()
        level[6:9, 6:9, 5] = np.nan
        return dict(level=level[None], points=verts, normals=normals, image=np.zeros(len(verts), np.int32), **kw)
    if name == "odd_step":                                  # a step that is no dyadic fraction, M = ceil(5 / 0.3) = 17
        level, verts, normals = _shape("two_spheres")
        return dict(level=level[None], points=verts, normals=normals, image=np.zeros(len(verts), np.int32), **dict(kw, radius=5.0, step=0.3))
    if name == "s40":                                       # two words per bit row (S - 1 = 39 cells along z)
        level = np.minimum(ref.two_spheres_level(40), ref.sphere_level(40, (20.0, 20.0, 34.0), 5.0))
        pts = rng.uniform(0, 39, size=(300, 3)).astype(np.float32)
        nrm = rng.normal(size=(300, 3)).astype(np.float32)
        return dict(level=level[None], points=pts, normals=nrm, image=np.zeros(300, np.int32), **dict(kw, radius=12.0, bias=0.0))
    raise KeyError(name)


CASES = ("s2", "sphere", "crease", "pit", "two_spheres", "n1", "n3", "n67", "batch", "faces", "degenerate", "iso", "nan_level", "odd_step",
         "s40")
_REF = {}


def _reference(name):
    if name not in _REF:
        c = _case(name)
        _REF[name] = (c, ref.ambient_occlusion(**c))
    return _REF[name]


def _run(c, cell_skip=True, **over):
    from shapeclipper_amd import ops
    c = dict(c, **over)
    t = lambda k, dt: torch.as_tensor(np.ascontiguousarray(c[k])).to(DEV, dt)
    out = ops.level_ambient_occlusion(t("level", torch.float32), t("points", torch.float32), t("normals", torch.float32),
                                      t("image", torch.int32), c["radius"], step=c["step"], bias=c["bias"], iso=c["iso"], cell_skip=cell_skip)
    assert out.ao.dtype == torch.float32 and out.mask.dtype == torch.int64
    return out.ao.cpu().numpy(), out.mask.cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[1], want[1]), "mask: %d of %d rows differ" % ((got[1] != want[1]).sum(), len(want[1]))
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "ao: %d of %d rows differ" % (
        (got[0].view(np.uint32) != want[0].view(np.uint32)).sum(), len(want[0]))


@pytest.mark.parametrize("cell_skip", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_bits_equal_the_restatement(name, cell_skip):
    c, want = _reference(name)
    _same(_run(c, cell_skip), want)
    closed = (want[1] != -1).sum()
    print(name, "rows", len(want[0]), "with a closed ray", closed, "ao mean %.4f" % want[0].mean())
    assert closed > 0 or name in ("sphere", "degenerate", "n1")         # every other case has closed rays


def test_the_cases_cover_what_they_name():
    c, want = _reference("degenerate")
    assert (want[0][[1, 3, 5, 7, 9, 11, 14]] == 1).all() and (want[1][[1, 3, 5, 7, 9, 11, 14]] == -1).all()
    c, want = _reference("batch")
    assert (want[1][1::3] == -1).all() and (want[0][1::3] == 1).all() and (want[1][0::3] != -1).any() and (want[1][2::3] != -1).any()
    c, want = _reference("faces")
    outside = ((c["points"] < 0) | (c["points"] > 16)).any(axis=1)
    assert outside.any() and (~outside).any() and (want[1][~outside] != -1).any()
    c, _ = _reference("s2")
    assert ref.step_count(c["radius"], c["step"]) == 1
    assert ref.cell_bits(_reference("s40")[0]["level"]).shape[-1] == 39


def test_an_image_alone_and_inside_a_batch_gives_the_same_bits():
    c, want = _reference("batch")
    for b in (0, 2):
        rows = c["image"] == b
        alone = _run(dict(c, level=c["level"][b:b + 1], points=c["points"][rows], normals=c["normals"][rows],
                          image=np.zeros(rows.sum(), np.int32)))
        _same(alone, (want[0][rows], want[1][rows]))


def test_a_permutation_of_the_points_permutes_the_outputs():
    c, want = _reference("batch")
    perm = np.random.default_rng(5).permutation(len(c["points"]))
    for cell_skip in (True, False):
        got = _run(dict(c, points=c["points"][perm], normals=c["normals"][perm], image=c["image"][perm]), cell_skip)
        _same(got, (want[0][perm], want[1][perm]))


def test_a_side_stream_and_a_second_call_give_the_same_bits():
    c, want = _reference("two_spheres")
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        first = _run(c)
        second = _run(c, False)
    stream.synchronize()
    _same(first, want)
    _same(second, want)


def test_an_image_out_of_range_raises_and_the_call_after_it_is_right():
    c, want = _reference("n67")
    for bad in (1, -1, 2 ** 31 - 1):
        image = c["image"].copy()
        image[33] = bad
        for cell_skip in (True, False):
            with pytest.raises(ValueError, match="image index lies outside"):
                _run(c, cell_skip, image=image)
    _same(_run(c), want)


def test_no_points_and_bad_arguments():
    from shapeclipper_amd import ops
    c, _ = _reference("n3")
    level = torch.as_tensor(c["level"]).to(DEV)
    f = lambda *shape: torch.zeros(*shape, device=DEV)
    i = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    out = ops.level_ambient_occlusion(level, f(0, 3), f(0, 3), i(0), 4.0)
    assert out.ao.shape == (0,) and out.mask.shape == (0,) and out.mask.dtype == torch.int64
    bad = [dict(level=level.cpu()), dict(level=level.double()), dict(level=level[0]), dict(level=level[:, :, :, :5]), dict(level=level[:, :1, :1, :1]),
           dict(points=f(3, 2)), dict(normals=f(4, 3)), dict(image=i(4)), dict(image=torch.zeros(3, dtype=torch.int64, device=DEV)),
           dict(points=f(3, 3).cpu()), dict(radius=0.0), dict(radius=float("nan")), dict(step=0.0), dict(radius=3000.0), dict(bias=float("inf")),
           dict(iso=float("nan")), dict(cell_skip=1)]
    for kw in bad:
        args = dict(level=level, points=f(3, 3), normals=f(3, 3), image=i(3), radius=4.0)
        args.update(kw)
        with pytest.raises(ValueError, match="level_ambient_occlusion"):
            ops.level_ambient_occlusion(**args)
