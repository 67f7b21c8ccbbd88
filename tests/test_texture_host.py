"""`--eval.texture` without a GPU: the atlas layout as tests/texture_ref.py restates it (and ops.texture_layout / eval_3D.texture_face_uv
beside it), the OBJ / MTL writers, the options, and the header's declarations.  CPU only."""
import os
import re

import numpy as np
import pytest
import torch

import texture_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _first_f_needing(A_from, T):
    """The smallest face count whose atlas is larger than A_from at cell side T."""
    return 2 * (A_from // T) ** 2 + 1


def _face_counts(T):
    f128 = _first_f_needing(64, T)
    return [0, 1, 2, 3, 7, 8, 9, 1000, f128 - 1, f128]


@pytest.mark.parametrize("T", list(ref.T_RANGE))
def test_layout(T):
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    rng = np.random.RandomState(T)
    f128 = _first_f_needing(64, T)
    assert ref.layout(f128 - 1, T)[0] == 64 and ref.layout(f128, T)[0] == 128
    for F in _face_counts(T):
        A, n, rows = ref.layout(F, T)
        # the choice of A: a power of two in 64..8192 that holds the cells, and the next smaller one does not
        cells = (F + 1) // 2
        assert 64 <= A <= 8192 and A & (A - 1) == 0 and n == A // T and n * n >= cells
        assert A == 64 or ((A // 2) // T) ** 2 < cells
        assert rows == T * -(-cells // n) and rows <= A and rows % T == 0
        assert tuple(ops.texture_layout(F, T)) == (A, n, rows)
        # every used texel belongs to exactly one face; every face owns its half cell; nothing is used below `rows`
        face, i, j, h = ref.texel_faces(A, T, F)
        used = face >= 0
        assert not used[rows:].any()
        assert np.array_equal(ref.texel_faces(A, T, F, rows)[0], face[:rows])
        count = np.bincount(face[used].astype(np.int64), minlength=F)
        lower, upper = T * (T + 1) // 2, T * (T - 1) // 2
        assert np.array_equal(count, np.where(np.arange(F) % 2 == 0, lower, upper))
        assert used.sum() == count.sum()
        if F == 0:
            continue
        # corners are exact texel centres of texels that carry the face's index, and the look-up there has zero weights elsewhere
        uv = ref.face_uv(F, A, T)
        assert np.array_equal(uv.astype(np.float32).astype(np.float64), uv)
        assert np.array_equal(eval_3D.texture_face_uv(F, A, T).numpy(), uv.astype(np.float32))
        px, py = uv[..., 0] * A - 0.5, (1 - uv[..., 1]) * A - 0.5
        assert np.array_equal(px, np.round(px)) and np.array_equal(py, np.round(py))
        fidx = np.repeat(np.arange(F), 3)
        assert np.array_equal(face[py.astype(int).reshape(-1), px.astype(int).reshape(-1)], fidx)
        xa, xb, ya, yb, fx, fy = ref.footprint(uv.reshape(-1, 2).astype(np.float32), A)
        assert not fx.any() and not fy.any() and np.array_equal(xa, px.reshape(-1)) and np.array_equal(ya, py.reshape(-1))
        # the corner texels' barycentrics are the unit vectors, exactly
        b = np.stack(ref.texel_barycentrics(i[ya, xa], j[ya, xa], h[ya, xa], T), -1).reshape(F, 3, 3)
        assert np.array_equal(b, np.broadcast_to(np.eye(3, dtype=np.float32), (F, 3, 3)))
        # UV orientation = the chart's orientation in the atlas (x right, y down -> v up flips the sign once) for both halves
        e1, e2 = uv[:, 1] - uv[:, 0], uv[:, 2] - uv[:, 0]
        cross = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        assert (cross < 0).all()                        # lower: p1 - p0 = (+, 0), p2 - p0 = (0, +) in y-down texels = (0, -) in v
        assert np.allclose(np.abs(cross), ((T - 3) / A) ** 2)
    # the footprint of strictly interior points stays inside the face's own texels, in the first cell and in one with neighbours all around
    n = 64 // T
    F = 2 * (n + 1) + 2
    A, n, rows = ref.layout(F, T)
    assert A == 64
    face, i, j, h = ref.texel_faces(A, T, F)
    uv = ref.face_uv(F, A, T)
    bary = rng.dirichlet((1.0, 1.0, 1.0), 10000)
    bary = np.maximum(bary, 1e-4)                       # strictly interior, by more than the fp32 rounding of a texture coordinate
    bary /= bary.sum(axis=1, keepdims=True)
    for f in (0, 1, F - 2, F - 1):
        pts = (bary @ uv[f]).astype(np.float32)
        xa, xb, ya, yb, fx, fy = ref.footprint(pts, A)
        for yy, xx in ((ya, xa), (ya, xb), (yb, xa), (yb, xb)):
            assert (face[yy, xx] == f).all()
            s = i[yy, xx] + j[yy, xx]
            assert (s <= T - 2).all() if f % 2 == 0 else (s >= T).all()


def test_layout_refuses_what_8192_cannot_hold():
    from shapeclipper_amd import ops
    most = 2 * (8192 // 32) ** 2
    assert ops.texture_layout(most, 32)[0] == 8192 and ref.layout(most, 32)[0] == 8192
    with pytest.raises(ValueError, match="eval.texture_texels"):
        ops.texture_layout(most + 1, 32)
    with pytest.raises(ValueError, match="eval.texture_texels"):
        ref.layout(most + 1, 32)
    for bad in (3, 33, True, 8.0):
        with pytest.raises(ValueError):
            ops.texture_layout(10, bad)


def test_reference_sampler_and_pack():
    """The numpy restatement itself on values known by hand."""
    A = 64
    atlas = np.zeros((A, A, 1), np.float32)
    atlas[0, 0], atlas[0, 1], atlas[1, 0], atlas[1, 1] = 1, 3, 5, 9
    uv = np.array([[0.5 / A, 1 - 0.5 / A], [1.0 / A, 1 - 0.5 / A], [1.0 / A, 1 - 1.0 / A], [-3.0, 7.0], [9.0, -9.0]], np.float32)
    atlas[A - 1, A - 1] = 4
    assert ref.sample(atlas, uv)[:, 0].tolist() == [1.0, 2.0, 4.5, 1.0, 4.0]
    assert ref.unit_byte(np.array([-1, 0, 0.5, 1, 2, np.nan, 0.999999], np.float32)).tolist() == [0, 0, 127, 255, 255, 0, 254]
    rgb = np.full((4 * A, 3), 0.5, np.float32)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (4 * A, 1))
    face = np.full(4 * A, -1)
    face[:10] = 0
    a, m = ref.pack(rgb, nrm, face, A, 4)
    assert (a.reshape(-1, 3)[:10] == 127).all() and (m.reshape(-1, 3)[:10] == [127, 127, 255]).all()
    assert (a.reshape(-1, 3)[10:] == 127).all() and (m.reshape(-1, 3)[10:] == 127).all()


def _parse_obj(path):
    out = dict(v=[], vt=[], f=[], mtllib=[], usemtl=[])
    for line in open(path).read().splitlines():
        key, *rest = line.split()
        if key in ("v", "vt"):
            out[key].append([float(x) for x in rest])
        elif key == "f":
            out["f"].append([[int(k) for k in c.split("/")] for c in rest])
        else:
            out[key].append(rest[0])
    return out


def test_obj_and_mtl_writers(tmp_path):
    from shapeclipper_amd.utils import util_vis
    rng = np.random.RandomState(0)
    V, F = 11, 7
    v = rng.randn(V, 3).astype(np.float32)
    f = rng.randint(0, V, (F, 3)).astype(np.int32)
    uv = rng.rand(F, 3, 2).astype(np.float32)
    obj, mtl, png = (str(tmp_path / ("3_mesh_tex" + e)) for e in (".obj", ".mtl", ".png"))
    util_vis.write_obj_textured(obj, torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(uv), mtl)
    util_vis.write_mtl(mtl, png)
    o = _parse_obj(obj)
    assert o["mtllib"] == ["3_mesh_tex.mtl"] and o["usemtl"] == ["tex"]
    assert len(o["v"]) == V and len(o["vt"]) == 3 * F and len(o["f"]) == F
    assert np.array_equal(np.array(o["v"], np.float32), v) and np.array_equal(np.array(o["vt"], np.float32).reshape(F, 3, 2), uv)
    idx = np.array(o["f"])                              # [F, 3, (vertex, texture coordinate)], 1-based
    assert idx[..., 0].min() >= 1 and idx[..., 0].max() <= V and np.array_equal(idx[..., 0] - 1, f)
    assert np.array_equal(idx[..., 1].reshape(-1), np.arange(1, 3 * F + 1))
    text = open(obj).read()
    assert text.index("usemtl tex") > text.rindex("\nvt ") and text.index("\nf ") > text.index("usemtl tex")
    lines = open(mtl).read().splitlines()
    assert lines[:3] == ["newmtl tex", "Ka 1 1 1", "Kd 1 1 1"]
    (map_kd,) = [l.split(None, 1)[1] for l in lines if l.startswith("map_Kd ")]
    assert map_kd == "3_mesh_tex.png" and os.sep not in map_kd
    # no faces: a valid OBJ with vertices only
    util_vis.write_obj_textured(obj, v, np.zeros((0, 3), np.int32), np.zeros((0, 3, 2), np.float32), mtl)
    o = _parse_obj(obj)
    assert len(o["v"]) == V and o["vt"] == [] and o["f"] == [] and o["usemtl"] == ["tex"]


def test_textured_dump_files(tmp_path):
    """dump_textured_meshes writes the four files per sample, the PNGs holding the atlas bytes; an empty mesh its grey 64 x 64 atlases."""
    PIL = pytest.importorskip("PIL.Image")
    from shapeclipper_amd.utils import eval_3D, util_vis
    from shapeclipper_amd.utils.util import EasyDict as edict
    rng = np.random.RandomState(1)
    atlas, atlas_n = (torch.from_numpy(rng.randint(0, 256, (128, 128, 3)).astype(np.uint8)) for _ in range(2))
    uv = eval_3D.texture_face_uv(2, 128, 8)
    full = eval_3D.TexturedMesh(torch.rand(4, 3), torch.tensor([[0, 1, 2], [2, 1, 3]], dtype=torch.int32), uv, atlas, atlas_n, {})
    grey = torch.full((64, 64, 3), 127, dtype=torch.uint8)
    none = eval_3D.TexturedMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3, 2), grey, grey, {})
    os.makedirs(tmp_path / "dump")
    util_vis.dump_textured_meshes(edict(output_path=str(tmp_path)), [5, 6], "mesh_tex", [full, none])
    want = sorted("%d_mesh_tex%s" % (i, e) for i in (5, 6) for e in (".obj", ".mtl", ".png", "_normal.png"))
    assert sorted(os.listdir(tmp_path / "dump")) == want
    read = lambda name: np.asarray(PIL.open(str(tmp_path / "dump" / name)))
    assert np.array_equal(read("5_mesh_tex.png"), atlas.numpy()) and np.array_equal(read("5_mesh_tex_normal.png"), atlas_n.numpy())
    assert read("6_mesh_tex.png").shape == (64, 64, 3) and (read("6_mesh_tex.png") == 127).all()
    assert len(_parse_obj(str(tmp_path / "dump" / "6_mesh_tex.obj"))["f"]) == 0
    assert open(tmp_path / "dump" / "5_mesh_tex.mtl").read().splitlines()[-1] == "map_Kd 5_mesh_tex.png"


def test_textured_dump_without_pil_is_skipped_with_one_warning(tmp_path, monkeypatch, capsys):
    from shapeclipper_amd.utils import eval_3D, util_vis
    from shapeclipper_amd.utils.util import EasyDict as edict
    monkeypatch.setattr(util_vis, "Image", None)
    monkeypatch.setattr(util_vis, "_WARNED_NO_PIL", [])
    grey = torch.full((64, 64, 3), 127, dtype=torch.uint8)
    none = eval_3D.TexturedMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32), torch.zeros(0, 3, 2), grey, grey, {})
    os.makedirs(tmp_path / "dump")
    for _ in range(2):
        util_vis.dump_textured_meshes(edict(output_path=str(tmp_path)), [1], "mesh_tex", [none])
    assert os.listdir(tmp_path / "dump") == [] and capsys.readouterr().out.count("PIL is not importable") == 1


def _parse(tmp_path, *extra):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_texture",
                                                "--output_root=%s" % tmp_path, *extra]), verbose=False)


def test_options(tmp_path):
    from shapeclipper_amd.utils import options
    off = _parse(tmp_path)
    assert "texture" not in off.eval and options.texture_texels(off) is None            # absent means off
    assert options.texture_texels(off, always=True) == 8
    assert options.texture_texels(_parse(tmp_path, "--eval.texture")) == 8
    assert options.texture_texels(_parse(tmp_path, "--eval.texture", "--eval.texture_texels=4")) == 4
    assert options.texture_texels(_parse(tmp_path, "--eval.texture", "--eval.texture_texels=32")) == 32
    assert options.texture_texels(_parse(tmp_path, "--eval.texture!", "--eval.texture_texels=16")) is None
    assert options.texture_texels(options.edict()) is None                               # a tree built by hand without an `eval` node
    for switch in ("--eval.texture", "--eval.texture!", None):
        for bad in ("3", "33", "8.0", "true", "eight", "-8"):
            with pytest.raises(ValueError, match="eval.texture_texels"):
                _parse(tmp_path, *([switch] if switch else []), "--eval.texture_texels=%s" % bad)
    for bad in ("1", "yes_please", "0.5"):
        for texels in ((), ("--eval.texture_texels=8",)):
            with pytest.raises(ValueError, match="eval.texture must be a bool"):
                _parse(tmp_path, "--eval.texture=%s" % bad, *texels)


def test_header_declares_the_entry_points():
    from shapeclipper_amd import _lib
    text = open(os.path.join(ROOT, "include", "shapeclipper_hip.h")).read()
    for name, n_args in (("sc_texture_queries", 18), ("sc_texture_pack", 9), ("sc_texture_sample", 10)):
        assert re.search(r"^int %s\(" % name, text, flags=re.M)
        assert name in _lib.SYMBOLS and len(_lib.SIGNATURES[name][1]) == n_args
    comment = text[text.index("Per-triangle texture atlas"):text.index("int sc_texture_queries")]
    for phrase in ("b0 = (1 - b1) - b2", "v = (b0 v0 + b1 v1) + b2 v2", "x = u * A - 0.5", "trunc(clamp(c, 0, 1) * 255)", "127"):
        assert phrase in comment
    lib = _lib.load()
    # refusals that need no device: they return before anything is launched
    null = None
    assert lib.sc_texture_queries(null, null, null, null, null, 1, 0, 0, 96, 8, -0.5, 0.5, 16, 8, 8 * 96, null, null, null) == 1    # A
    assert lib.sc_texture_queries(null, null, null, null, null, 1, 0, 0, 64, 3, -0.5, 0.5, 16, 8, 8 * 64, null, null, null) == 1    # T
    assert lib.sc_texture_queries(null, null, null, null, null, 1, 0, 0, 64, 8, -0.5, 0.5, 16, 8, 8 * 64 - 1, null, null, null) == 1  # stride
    assert lib.sc_texture_queries(null, null, null, null, null, 0, 0, 0, 64, 8, -0.5, 0.5, 16, 8, 8 * 64, null, null, null) == 0
    assert lib.sc_texture_pack(null, null, null, 1, 64, 65, null, null, null) == 1
    assert lib.sc_texture_pack(null, null, null, 0, 64, 8, null, null, null) == 0
    assert lib.sc_texture_sample(null, 0, null, null, 4, 1, 100, 3, null, null) == 1
    assert lib.sc_texture_sample(null, 0, null, null, 0, 1, 64, 3, null, null) == 0


def test_ops_refuse_host_tensors():
    from shapeclipper_amd import ops
    with pytest.raises(ValueError, match="device tensor"):
        ops.texture_queries(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32), [0], [0], [1], 64, 8, -0.5, 0.5, 16, 8)
    with pytest.raises(ValueError, match="device tensor"):
        ops.texture_pack(torch.zeros(512, 3), torch.zeros(512, 3), torch.zeros(1, 512, dtype=torch.int32), 64, 8)
    with pytest.raises(ValueError, match="device tensor"):
        ops.texture_sample(torch.zeros(1, 64, 64, 3), torch.zeros(4, 2), torch.zeros(4, dtype=torch.int32))
