"""`--mesh.ao` through Runner.evaluate and Runner.evaluate_sharded on the synthetic evaluation (vox_res 16, 1000 points), each into a clean
folder, with --eval.texture and --eval.mesh_render on: every sample has {idx}_mesh_ao.ply -- the vertices and faces of {idx}_mesh.ply,
normals, and a grey that a direct ops.level_ambient_occlusion call on the file's own vertices and normals gives -- and an 8-field
{idx}_mesh_ao.txt, the AO atlas in the layout of the colour atlas, and the shaded and clay pictures, which are eval_3D.mesh_shade of the
stored render (restated in numpy here); the vis_{ep}/ dump writes the same files and the two shaded turn-tables; a run without the switch
lists the same files otherwise and keeps the bytes of chamfer.txt, {idx}_mesh.ply, the OBJ, the MTL and the atlases.

The untrained SDF network is a sphere, on which every ray is open, so the level grid is cut in two by an empty slab 2.5 pitches thick
(compute_level_grid is wrapped for all runs alike): the cut faces look at each other."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIELDS = "idx vertices radius step ao_mean ao_min ao_max open_share".split()
OURS = ("_mesh_ao.ply", "_mesh_ao.txt", "_mesh_tex_ao.png", "_image_mesh_shaded.png", "_clay_mesh.png")
RADIUS = 0.5


def _ply(fname):
    """A binary PLY of this project -> (dict of per-vertex columns, faces [F,3])."""
    data = open(fname, "rb").read()
    head, body = data.split(b"end_header\n", 1)
    lines = head.decode("ascii").splitlines()
    nv, nf = (int([l for l in lines if l.startswith("element " + e)][0].split()[2]) for e in ("vertex", "face"))
    props = [l.split() for l in lines[lines.index("element vertex %d" % nv) + 1:lines.index("element face %d" % nf)]]
    dt = np.dtype([(p[2], "<f4" if p[1] == "float" else "u1") for p in props])
    vert = np.frombuffer(body[:dt.itemsize * nv], dt)
    face = np.frombuffer(body[dt.itemsize * nv:], np.dtype([("n", "u1"), ("v", "<i4", (3,))]))
    assert len(face) == nf and (face["n"] == 3).all()
    return vert, face["v"]


def _listing(path):
    return sorted(os.listdir(path)) + sorted(os.path.join("dump", f) for f in os.listdir(os.path.join(path, "dump")))


def _files(path, pick, folder="dump"):
    d = os.path.join(path, folder)
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d)) if pick(f)}


def _shade_numpy(render, ao_vertex, faces, pose, bg):
    """eval_3D.mesh_shade restated for one image and one view: render's face [H,W], bary [H,W,3], normal, rgb [H,W,3] as numpy."""
    face, bary, normal, rgb = render
    hit = face >= 0
    a = ao_vertex[faces[np.where(hit, face, 0)]]                                       # [H,W,3]
    ao = (bary[..., 0] * a[..., 0] + bary[..., 1] * a[..., 1]) + bary[..., 2] * a[..., 2]
    n = 2 * normal.astype(np.float64) - 1
    with np.errstate(all="ignore"):                                                    # a miss has n = 0 and is not used
        lambert = np.abs(n @ pose[2, :3].astype(np.float64)) / np.linalg.norm(n, axis=-1)
    shade = ao * (0.3 + 0.7 * lambert)
    shaded = np.where(hit[..., None], rgb * shade[..., None], bg)
    clay = np.where(hit[..., None], np.repeat(0.8 * shade[..., None], 3, axis=-1), bg)
    return shaded, clay


def test_evaluation_bakes_the_occlusion_and_shades_the_pictures(tmp_path, monkeypatch):
    PIL = pytest.importorskip("PIL.Image")
    os.environ.setdefault("MIOPEN_FIND_MODE", "FAST")
    import torch.distributed as dist
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.runner import Runner
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    o = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=pytest_ao", "--output_root=%s" % (tmp_path / "out"),
                                             "--arch.enc_pretrained!", "--data.dataset=synthetic", "--eval.vox_res=16", "--eval.num_points=1000",
                                             "--tb!", "--eval.texture", "--eval.mesh_render", "--mesh.ao", "--mesh.ao_radius=%r" % RADIUS]),
                    verbose=False)
    o.device, o.world_size, o.port = 0, 1, 0
    torch.manual_seed(0)
    r = Runner(o)
    r.load_dataset(o, eval_split="test")
    r.build_networks(o)
    n = len(r.test_data)
    bg = float(o.data.bgcolor)
    level_grid = eval_3D.compute_level_grid

    def cut(*args, **kw):
        level = level_grid(*args, **kw)
        S = level.shape[1]
        y = torch.arange(S, device=level.device, dtype=level.dtype).view(1, 1, S, 1)
        return torch.maximum(level, 1.25 - (y - (S - 1) / 2).abs())             # the slab |y - centre| < 1.25 is empty

    monkeypatch.setattr(eval_3D, "compute_level_grid", cut)
    seen = {}
    dump = r.dump_visuals

    def spy(opt, var, ep, train=False):
        """After the dump: what the files of each sample must hold, from what the dump left in var."""
        out = dump(opt, var, ep, train=train)
        if "mesh_ao" not in var:
            for i in var.idx.cpu().tolist():
                seen[i] = None
            return out
        S = var.level_vox.shape[1]
        mesh = ops.PackedMesh(*var.mesh_packed)
        render = var.mesh_render.render
        shaded, clay = eval_3D.mesh_shade(opt, var, render, var.pose)
        atlases = eval_3D.mesh_ao_atlas(opt, var, var.texture)
        per_vertex = mesh.split(var.mesh_ao["ao"])
        for b, i in enumerate(var.idx.cpu().tolist()):
            cpu = lambda x: x[b, 0].cpu().numpy()
            seen[i] = dict(S=S, level=var.level_vox[b].float().cpu(), verts=mesh.split()[b][0].cpu(), faces=mesh.split()[b][1].cpu().numpy(),
                           ao=per_vertex[b][0].cpu().numpy(), render=(cpu(render.face), cpu(render.bary), cpu(render.normal), cpu(render.rgb)),
                           shaded=cpu(shaded), clay=cpu(clay), atlas=atlases[b].cpu().numpy(), pose=var.pose[b].float().cpu().numpy())
        return out

    r.dump_visuals = spy

    def run(mode, name):
        o.output_path = str(tmp_path / "out" / name)                    # a clean folder each
        os.makedirs(o.output_path)
        seen.clear()
        value = getattr(r, mode)(o, ep=0)
        assert sorted(seen) == list(range(n))
        return dict(value=value, seen=dict(seen), listing=_listing(o.output_path), path=o.output_path,
                    ours=_files(o.output_path, lambda f: f.endswith(OURS)),
                    kept=_files(o.output_path, lambda f: f.endswith(("_mesh.ply", ".obj", ".mtl", "_mesh_tex.png", "_mesh_tex_normal.png",
                                                                     "_image_mesh.png"))),
                    reports={f: open(os.path.join(o.output_path, f), "rb").read() for f in ("chamfer.txt", "texture.txt", "mesh_render.txt")})

    to_bytes = lambda x: (np.clip(x, 0, 1) * 255).astype(np.uint8)

    def check_files(res, folder="dump", samples=range(n)):
        lit = 0
        for i in samples:
            d = os.path.join(res["path"], folder)
            want = res["seen"][i]
            line = open(os.path.join(d, "%d_mesh_ao.txt" % i)).read()
            assert line.endswith("\n") and line.count("\n") == 1 and len(line.split()) == len(FIELDS) == 8
            f = dict(zip(FIELDS, line.split()))
            print(folder, line.strip())
            S, V = want["S"], len(want["verts"])
            assert int(f["idx"]) == i and int(f["vertices"]) == V and float(f["radius"]) == RADIUS * (S - 1) and float(f["step"]) == 0.5
            plain, ours = (os.path.join(d, "%d_%s.ply" % (i, name)) for name in ("mesh", "mesh_ao"))
            assert os.path.exists(plain) == os.path.exists(ours)        # an empty mesh writes neither
            for name in OURS[2:]:
                assert os.path.exists(os.path.join(d, "%d%s" % (i, name)))
            if not os.path.exists(plain):
                continue
            # the PLY: {idx}_mesh.ply's vertices and faces, unit normals, and the grey of a direct call on the file's own normals
            mv, mf = _ply(plain)
            av, af = _ply(ours)
            assert av.dtype.names == ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue") and mv.dtype.names == ("x", "y", "z")
            assert all(np.array_equal(av[k].view(np.uint32), mv[k].view(np.uint32)) for k in "xyz") and np.array_equal(af, mf) and len(av) == V
            normals = np.stack([av["nx"], av["ny"], av["nz"]], axis=1)
            assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1).max() < 1e-5
            direct = ops.level_ambient_occlusion(want["level"][None].cuda().contiguous(), want["verts"].cuda().contiguous(),
                                                 torch.from_numpy(normals.copy()).cuda(), torch.zeros(V, dtype=torch.int32, device="cuda"),
                                                 RADIUS * (S - 1), step=0.5, bias=1.0)
            ao = direct.ao.cpu().numpy()
            assert np.array_equal(ao.view(np.uint32), want["ao"].view(np.uint32))
            grey = to_bytes(ao)
            assert all(np.array_equal(av[k], grey) for k in ("red", "green", "blue"))
            # the sidecar: a float64 mean printed to nine digits (5e-10 of a value below 1; the order of a float64 sum of V <= 2^12 values
            # moves it by less than 1e-12), the exact extremes, the share of fully open vertices
            assert abs(float(f["ao_mean"]) - ao.astype(np.float64).mean()) <= 1e-9
            assert f["ao_min"] == "%.9g" % ao.min() and f["ao_max"] == "%.9g" % ao.max()
            assert f["open_share"] == "%.9g" % ((direct.mask == -1).double().mean().item())
            # the pictures: mesh_shade of the stored render, which is the restatement within fp32 rounding
            shaded_np, clay_np = _shade_numpy(want["render"], want["ao"], want["faces"], want["pose"], bg)
            assert np.abs(shaded_np - want["shaded"]).max() <= 1e-5 and np.abs(clay_np - want["clay"]).max() <= 1e-5
            for name, x in (("image_mesh_shaded", want["shaded"]), ("clay_mesh", want["clay"])):
                png = np.asarray(PIL.open(os.path.join(d, "%d_%s.png" % (i, name))))
                assert np.array_equal(png, to_bytes(x))
            hit = want["render"][0] >= 0
            plain_png = np.asarray(PIL.open(os.path.join(d, "%d_image_mesh.png" % i)))
            shaded_png = np.asarray(PIL.open(os.path.join(d, "%d_image_mesh_shaded.png" % i)))
            assert hit.any() and not np.array_equal(shaded_png[hit], plain_png[hit]) and np.array_equal(shaded_png[~hit], plain_png[~hit])
            # the atlas: the colour atlas's layout -- a texel is 127 exactly where the normal atlas is unused
            atlas = np.asarray(PIL.open(os.path.join(d, "%d_mesh_tex_ao.png" % i)))
            normal_atlas = np.asarray(PIL.open(os.path.join(d, "%d_mesh_tex_normal.png" % i)))
            assert atlas.shape == normal_atlas.shape[:2] and np.array_equal(atlas, want["atlas"])
            unused = (normal_atlas == 127).all(axis=-1)
            assert (atlas[unused] == 127).all() and unused.any() and not unused.all()
            used = atlas[~unused]
            assert used.max() == 255                                    # the sphere's outer side is open
            if (ao < 1).any():
                assert used.min() < 255
                lit += 1
        assert lit >= 1                                                 # the cut faces are occluded: the greys are not all white

    plain = run("evaluate", "on")
    check_files(plain)
    assert len(plain["ours"]) == len(OURS) * n
    # sharded, one sample at a time, inside a gloo process group (of this one process: the gather has nobody to wait for)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("gloo", store=dist.FileStore(str(tmp_path / "store"), 1), rank=0, world_size=1)
    try:
        sharded = run("evaluate_sharded", "on_sharded")
    finally:
        if created:
            dist.destroy_process_group()
    check_files(sharded)
    # (the atlas side follows the largest mesh of a batch, so only the files that do not go through the atlas are compared byte for byte)
    per_vertex = lambda res: {f: data for f, data in res["ours"].items() if f.endswith(OURS[:2])}
    assert sharded["listing"] == plain["listing"] and per_vertex(sharded) == per_vertex(plain) and len(per_vertex(plain)) == 2 * n
    # the switch off: none of the new files, the same listing otherwise, the same bytes in every other file named above
    del o.mesh.ao
    off = run("evaluate", "off")
    assert off["value"] == plain["value"] and all(v is None for v in off["seen"].values())
    assert not off["ours"] and not [f for f in off["listing"] if "_ao." in f or "shaded" in f or "clay" in f]
    assert off["listing"] == [f for f in plain["listing"] if not f.endswith(OURS)]
    assert off["kept"] == plain["kept"] and len(off["kept"]) >= 6 * n and off["reports"] == plain["reports"]
    o.mesh.ao = True
    # vis_{ep}/ of the training-time visualisation: the vis_only pass bakes too, dump_geometry writes the same files, the turn-table the GIFs
    r.dump_visuals = dump
    r.graph.eval()
    o.H, o.W = o.eval.image_size
    o.output_path = plain["path"]
    os.makedirs(os.path.join(o.output_path, "vis_3"), exist_ok=True)
    sample = r.test_data[0]
    batch = {key: ({kk: vv[None] for kk, vv in v.items()} if isinstance(v, dict) else torch.as_tensor(v)[None]) for key, v in sample.items()}
    with torch.no_grad():
        var = r.evaluate_batch(o, edict(batch), 0, 0, single_gpu=True)
        var = r.graph.module.get_rotate_pose(o, var, n_views=3)
        eval_3D.eval_metrics(o, var, r.graph.module.sdf_network, vis_only=True)
        assert "mesh_ao" in var and "mesh_ao_world" in var
        r.dump_geometry(o, var, "vis_3")
        r.dump_mesh_turntable(o, var, "vis_3")
    i = int(var.idx[0])
    in_vis = _files(o.output_path, lambda f: f.endswith(OURS[:2]), "vis_3")
    assert len(in_vis) == 2 and in_vis == {f: data for f, data in plain["ours"].items() if f.startswith("%d_" % i) and f.endswith(OURS[:2])}
    names = os.listdir(os.path.join(o.output_path, "vis_3"))
    assert "%d_mesh_tex_ao.png" % i in names
    for name in ("image_mesh_shaded", "clay_mesh"):
        assert "%d_%s.png" % (i, name) in names
        gif = PIL.open(os.path.join(o.output_path, "vis_3", "%d_%s_rotate.gif" % (i, name)))
        assert gif.n_frames == 3
