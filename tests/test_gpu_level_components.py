"""ops.level_largest_component (csrc/level_components.hip) and `--hip.largest_component`.

The rule in every case: level_out is bit-identical (compared as int32) to the numpy flood fill of tests/level_components_ref.py and the
three counts are equal.  Sides 2..65 cover a grid smaller than a tile, one tile exactly, tiles that S does not fill (9, 17, 33, 65 leave
a one-voxel layer) and several hundred workgroups; the grids cover long label chains across tile faces (serpentine), thousands of
components around the percolation threshold (random occupancy), the tie rule, the bit-identical cases and non-finite values.  Then:
batch independence, run-to-run and side-stream equality, the raw C ABI, and eval_metrics / Runner dumps with the switch off and on."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import level_components_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SIDES = (2, 5, 8, 9, 17, 33, 65)
ISOS = (0.0, 0.05)


def _batch(kind, S, iso, B):
    return torch.from_numpy(np.stack([ref.image(kind, S, iso, k) for k in range(B)])).to(DEV)


def _check(kind, S, iso, B, out, stats):
    out, stats = out.cpu().numpy(), [s.cpu().numpy() for s in stats]
    assert out.dtype == np.float32 and out.shape == (B, S, S, S) and all(s.dtype == np.int32 and s.shape == (B,) for s in stats)
    for k in range(B):
        want = ref.expected(kind, S, iso, k)
        got = (int(stats[0][k]), int(stats[1][k]), int(stats[2][k]))
        print("%s S=%d iso=%g B=%d image %d: components / inside / kept = %s (want %s), voxels that differ: %d"
              % (kind, S, iso, B, k, got, (want["n_components"], want["inside_voxels"], want["kept_voxels"]),
                 int((out[k].view(np.int32) != want["out"].view(np.int32)).sum())))
        assert got == (want["n_components"], want["inside_voxels"], want["kept_voxels"]), (kind, S, iso, B, k)
        assert np.array_equal(out[k].view(np.int32), want["out"].view(np.int32)), (kind, S, iso, B, k)
    return out


@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("kind", ref.KINDS)
def test_matches_the_flood_fill_bit_for_bit(kind, S):
    from shapeclipper_amd import ops
    for iso in ISOS:
        for B in (1, 3):
            level = _batch(kind, S, iso, B)
            keep = level.clone()
            out, stats = ops.level_largest_component(level, iso)
            assert isinstance(stats, ops.ComponentStats) and stats.n_components is stats[0] and stats.kept_voxels is stats[2]
            got = _check(kind, S, iso, B, out, stats)
            assert torch.equal(level.view(torch.int32), keep.view(torch.int32))             # the input is not written
            for k in range(B):
                want = ref.expected(kind, S, iso, k)
                if kind == "serpentine":
                    assert want["n_components"] == 1                                        # the whole path is one component
                if want["n_components"] <= 1:                                               # none / all / one: the input's bits come back
                    assert np.array_equal(got[k].view(np.int32), ref.image(kind, S, iso, k).view(np.int32))
                if kind == "nonfinite":
                    src = ref.image(kind, S, iso, k)
                    nan, pinf, ninf = np.isnan(src), np.isposinf(src), np.isneginf(src)
                    assert np.array_equal(got[k].view(np.int32)[nan | pinf], src.view(np.int32)[nan | pinf])    # outside: untouched, payloads kept
                    assert np.isin(got[k][ninf], (-np.inf, np.inf)).all() and want["inside_voxels"] >= int(ninf.sum())   # -Inf counts as inside


def test_an_image_does_not_depend_on_its_batch():
    from shapeclipper_amd import ops
    for S, iso in ((17, 0.05), (65, 0.0)):
        imgs = [ref.image("random31", S, iso, 0), ref.image("two_balls", S, iso, 1), ref.image("nonfinite", S, iso, 2)]
        full, fs = ops.level_largest_component(torch.from_numpy(np.stack(imgs)).to(DEV), iso)
        for b, img in enumerate(imgs):
            one, os_ = ops.level_largest_component(torch.from_numpy(img[None].copy()).to(DEV), iso)
            assert torch.equal(one[0].view(torch.int32), full[b].view(torch.int32))
            assert all(int(a[0]) == int(c[b]) for a, c in zip(os_, fs))


def test_same_bits_run_to_run_and_on_a_side_stream():
    from shapeclipper_amd import ops
    level = torch.from_numpy(np.stack([ref.image("random31", 65, 0.0, 0), ref.image("serpentine", 65, 0.0, 1), ref.image("random50", 65, 0.0, 2)])).to(DEV)
    a, sa = ops.level_largest_component(level)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        b, sb = ops.level_largest_component(level)
    c, sc = ops.level_largest_component(level)
    torch.cuda.synchronize()
    for other, so in ((b, sb), (c, sc)):
        assert torch.equal(a.view(torch.int32), other.view(torch.int32))
        assert all(torch.equal(x, y) for x, y in zip(sa, so))
    _check("random31", 65, 0.0, 1, a[:1], [s[:1] for s in sa])


def test_raw_c_abi():
    """The entry point with raw pointers and a scratch of the queried size; in place (level_out = level) as the header allows."""
    from shapeclipper_amd import _lib
    lib = _lib.load()
    S, B, iso = 33, 2, 0.05
    level = torch.from_numpy(np.stack([ref.image("two_balls", S, iso, 0), ref.image("random31", S, iso, 1)])).to(DEV)
    out = torch.full_like(level, float("nan"))
    stats = torch.full((3, B), -7, device=DEV, dtype=torch.int32)
    fn = lib._cdll.sc_level_largest_component_scratch_bytes
    nbytes = int(fn(ctypes.c_int(B), ctypes.c_int(S)))
    assert nbytes >= 8 * B * S ** 3
    ws = torch.full((nbytes,), 0xA5, device=DEV, dtype=torch.uint8)                         # contents irrelevant on entry
    p, ci, cf = _lib.ptr, ctypes.c_int, ctypes.c_float
    rc = lib.sc_level_largest_component(p(level), ci(B), ci(S), cf(iso), p(out), p(stats[0]), p(stats[1]), p(stats[2]), p(ws), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    want = [ref.expected("two_balls", S, iso, 0), ref.expected("random31", S, iso, 1)]
    for k in range(B):
        assert np.array_equal(out[k].cpu().numpy().view(np.int32), want[k]["out"].view(np.int32))
        assert stats[:, k].tolist() == [want[k]["n_components"], want[k]["inside_voxels"], want[k]["kept_voxels"]]
    rc = lib.sc_level_largest_component(p(level), ci(B), ci(S), cf(iso), p(level), p(stats[0]), p(stats[1]), p(stats[2]), p(ws), _lib.stream())
    assert rc == 0 and torch.equal(level.view(torch.int32), out.view(torch.int32))
    # refused sizes launch nothing
    for n, s in ((B, 1), (B, 1025), (65536, S)):
        assert lib.sc_level_largest_component(p(level), ci(n), ci(s), cf(iso), p(out), p(stats[0]), p(stats[1]), p(stats[2]), p(ws), _lib.stream()) == 1
    assert lib.sc_level_largest_component(p(level), ci(0), ci(S), cf(iso), p(out), p(stats[0]), p(stats[1]), p(stats[2]), p(ws), _lib.stream()) == 0
    torch.cuda.synchronize()


# ---- end to end: eval_metrics and the Runner's dumps -------------------------------------------------------------------------------------
BIG_R, SMALL_R, SMALL_C = 0.3, 0.05, (0.5, 0.5, 0.5)


def _opt(extra, output_root):
    from shapeclipper_amd.utils import options
    return options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=pytest_largest_component", "--output_root=%s" % output_root,
                                                "--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.num_points=5000", "--tb!", *extra]),
                       verbose=False)


def _runner(o):
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    from shapeclipper_amd.model.runner import Runner
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    r.graph.eval()
    return r


def _crafted(o):
    """(grid [65,65,65] of a ball of radius 0.3 at the origin and one of radius 0.05 at (0.5, 0.5, 0.5), the large ball alone, the small
    ball's inside mask), at the sample positions of get_dense_3D_grid."""
    lo, hi = o.eval.range
    g = torch.linspace(lo, hi, o.eval.vox_res + 1, device=DEV)
    pts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), dim=-1)
    big = pts.norm(dim=-1) - BIG_R
    small = (pts - torch.tensor(SMALL_C, device=DEV)).norm(dim=-1) - SMALL_R
    return torch.minimum(big, small).contiguous(), big.contiguous(), small < 0


def _near_small(points, o):
    """points [..., 3] in written coordinates (v / S (hi - lo) + lo) -> mask of those within 0.1 of the small ball.  The written
    coordinates sit up to (hi - lo) / S below the sampled position per axis; the ball's centre is moved the same way."""
    lo, hi = o.eval.range
    S = o.eval.vox_res + 1
    c = torch.tensor(SMALL_C, device=points.device)
    c = (c - lo) * (S - 1) / S + lo
    return (points - c).norm(dim=-1) <= SMALL_R + 0.1


def _sample_var(r, o, it=0):
    from shapeclipper_amd.utils.util import EasyDict as edict
    sample = r.test_data[it]
    batch = {k: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for k, v in sample.items()}
    o.H, o.W = o.eval.image_size
    with torch.no_grad():
        return r.evaluate_batch(o, edict(batch), 0, it, single_gpu=True)


def test_eval_metrics_drops_the_floater_only_with_the_switch_on(tmp_path, monkeypatch):
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    o = _opt([], str(tmp_path))
    assert o.eval.vox_res == 64 and o.hip.largest_component is False
    r = _runner(o)
    grid, big_only, small_inside = _crafted(o)
    n_small = int(small_inside.sum())
    assert n_small >= 20 and not bool((small_inside & (big_only < 0)).any())
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    calls, sampled = [], []
    op, sample = ops.level_largest_component, eval_3D.surface_points_device
    monkeypatch.setattr(ops, "level_largest_component", lambda *a, **k: calls.append(1) or op(*a, **k))

    def spy(level, lo, hi, n, **kw):
        res = sample(level, lo, hi, n, **kw)
        sampled.append(res[0].clone())
        return res
    monkeypatch.setattr(eval_3D, "surface_points_device", spy)
    lo, hi = o.eval.range
    net = r.graph.module.sdf_network

    # ---- off: the op is never called, the floater is in the cloud and in the mesh ----
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert calls == [] and "component_stats" not in var
    assert torch.equal(var.level_vox[0], grid)
    near = _near_small(sampled[-1][0], o)
    verts_off = eval_3D.meshes_device(var.level_vox, lo, hi)[0][0]
    print("off: %d of %d samples and %d of %d vertices near the small ball" % (int(near.sum()), near.numel(), int(_near_small(verts_off, o).sum()), len(verts_off)))
    assert int(near.sum()) > 0 and int(_near_small(verts_off, o).sum()) > 0
    cd_off = (float(var.cd_acc[0]), float(var.cd_comp[0]))

    # ---- on ----
    o.hip.largest_component = True
    var = _sample_var(r, o)
    eval_3D.eval_metrics(o, var, net)
    assert calls == [1]
    near = _near_small(sampled[-1][0], o)
    verts_on, faces_on = eval_3D.meshes_device(var.level_vox, lo, hi)[0]
    print("on: %d samples and %d of %d vertices near the small ball" % (int(near.sum()), int(_near_small(verts_on, o).sum()), len(verts_on)))
    assert int(near.sum()) == 0 and int(_near_small(verts_on, o).sum()) == 0
    assert torch.equal(var.level_vox[0] != grid, small_inside)
    assert torch.equal(var.level_vox[0][small_inside], -grid[small_inside])
    st = var.component_stats
    assert (int(st.n_components[0]), int(st.inside_voxels[0]), int(st.kept_voxels[0])) == (2, int((grid < 0).sum()), int((big_only < 0).sum()))
    big_verts, big_faces, _, _ = ops.isosurface_mesh(big_only[None])
    assert len(verts_on) == len(big_verts) and len(faces_on) == len(big_faces) and len(verts_off) > len(verts_on)
    assert (float(var.cd_acc[0]), float(var.cd_comp[0])) != cd_off


def test_evaluate_writes_filtered_meshes_and_components_txt(tmp_path, monkeypatch):
    from shapeclipper_amd import ops
    from shapeclipper_amd.utils import eval_3D
    o = _opt(["--hip.largest_component"], str(tmp_path))
    r = _runner(o)
    grid, big_only, small_inside = _crafted(o)
    monkeypatch.setattr(eval_3D, "HAVE_MESHING", False)
    monkeypatch.setattr(eval_3D, "compute_level_grid", lambda opt, net, z, pts: grid[None].repeat(pts.shape[0], 1, 1, 1))
    n_big_verts = int(ops.isosurface_mesh(big_only[None])[2][0])
    n_both_verts = int(ops.isosurface_mesh(grid[None])[2][0])
    assert n_both_verts > n_big_verts > 0
    line = "%d %d %d" % (2, int((grid < 0).sum()), int((big_only < 0).sum()))
    n = len(r.test_data)
    dump = os.path.join(o.output_path, "dump")
    comp = os.path.join(o.output_path, "components.txt")

    def vertex_counts():
        out = {}
        for f in os.listdir(dump):
            if f.endswith("_mesh.ply"):
                head = open(os.path.join(dump, f), "rb").read(400).decode("ascii", "replace")
                out[int(f.split("_")[0])] = int([l for l in head.splitlines() if l.startswith("element vertex")][0].split()[2])
        return out

    for mode in ("evaluate", "evaluate_sharded"):
        for f in os.listdir(dump) if os.path.isdir(dump) else []:
            os.remove(os.path.join(dump, f))
        if os.path.exists(comp):
            os.remove(comp)
        o.hip.largest_component = True
        getattr(r, mode)(o, ep=0)
        assert vertex_counts() == {i: n_big_verts for i in range(n)}, mode
        assert open(comp).read().splitlines() == ["%d %s" % (i, line) for i in range(n)], mode
        chamfer_on = open(os.path.join(o.output_path, "chamfer.txt")).read()
        # the switch off: no components.txt, the floater is back in the mesh
        for f in os.listdir(dump):
            os.remove(os.path.join(dump, f))
        os.remove(comp)
        o.hip.largest_component = False
        getattr(r, mode)(o, ep=0)
        assert not os.path.exists(comp), mode
        assert vertex_counts() == {i: n_both_verts for i in range(n)}, mode
        assert open(os.path.join(o.output_path, "chamfer.txt")).read() != chamfer_on
