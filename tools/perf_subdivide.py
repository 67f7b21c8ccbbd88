"""Cost and effect of the refinement of `--mesh.subdivide`: ops.mesh_subdivide (csrc/mesh_subdivide.hip: edge table with owner and
opposite vertices, degree and owner scans, sorted neighbour rows, one emit launch) for 1, 2 and 3 levels and the whole
eval_3D.meshes_subdivided at one level with 0 and 2 Newton steps, B = 1, beside eval_3D.compute_level_grid and ops.isosurface_mesh on the
same box -- a geometric-init SDF network (roughly a sphere of radius 0.5, zero latent) at vox_res 64 and 128.  Device events around
windows of `reps` calls (reps sized so that a window is at least --window-ms long), after warm-up, the runs alternating, in one process;
medians and bests per call (each level of the op ends with its host read, so the figure is the op as the evaluation pays for it).
Then the comparison the feature is for: the mean |sdf| of the network at the vertices and at the face centroids of the vox_res-64 mesh,
of its one-level subdivision with two Newton steps, and of the vox_res-128 mesh, each beside what it costs (level grid + mesher
[+ refinement]).  One JSON line per case.
python tools/perf_subdivide.py [--iters N] [--window-ms T] [--res 64,128]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch

from perf_mesh_stats import _time


def _measure(runs, iters, window_ms):
    """{name: f} -> ({name: median ms}, {name: best ms}, {name: reps}), the runs alternating."""
    reps = {}
    for name, f in runs.items():                                        # warm-up, then the size of a window
        f(); f()
        torch.cuda.synchronize()
        reps[name] = max(1, min(1000, int(window_ms / max(_time(f, 1), 1e-3))))
    t = {name: [] for name in runs}
    for _ in range(iters):
        for name, f in runs.items():
            t[name].append(_time(f, reps[name]))
    return {name: sorted(v)[len(v) // 2] for name, v in t.items()}, {name: min(v) for name, v in t.items()}, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=20.0)
    ap.add_argument("--res", default="64,128")
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import SDFNetwork
    from shapeclipper_amd.utils import eval_3D, options
    from shapeclipper_amd.utils.util import EasyDict as edict
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_subdivide",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    torch.manual_seed(0)
    sdf_net = SDFNetwork(opt).to(dev)
    lo, hi = opt.eval.range
    zs = torch.zeros(1, opt.arch.impl_sdf.proj_latent_dim, device=dev)
    w_pack, cbias = sdf_net.packed(zs)
    sym = bool(sdf_net.force_symmetry)

    def mean_abs_sdf(points):
        """The mean |sdf| of the network at points [n,3] in object units (float64 mean of the fp32 values)."""
        n = points.shape[0]
        P = 16 * ((n + 15) // 16)
        q = torch.cat([points, points[:1].expand(P - n, 3)]).contiguous()
        sdf, _, _ = ops.sdf_forward(q, w_pack, cbias, P, symmetric=sym, want_grad=False, want_feat=False)
        return float(sdf.reshape(-1)[:n].double().abs().mean())

    def residuals(verts_grid, faces, S):
        """(at vertices, at face centroids) of a one-image mesh with vertices in grid-index units."""
        v = eval_3D.sampled_position(verts_grid, lo, hi, S)
        return mean_abs_sdf(v), mean_abs_sdf(v[faces.long()].mean(dim=1))

    for vox in (int(v) for v in a.res.split(",")):
        opt.eval.vox_res = vox
        with torch.no_grad():
            var = edict(idx=torch.arange(1, device=dev), proj_latent_sdf=zs)
            grid = eval_3D.get_dense_3D_grid(opt, var)
            level = eval_3D.compute_level_grid(opt, sdf_net, zs, grid)
            S = level.shape[1]
            packed = ops.isosurface_mesh(level)

            def whole(k):
                o = edict(eval=dict(range=[lo, hi]), mesh=dict(subdivide=1, subdivide_project=k))
                v = edict(idx=var.idx, proj_latent_sdf=zs, level_vox=level, mesh_packed=list(packed))
                eval_3D.meshes_subdivided(o, v, sdf_net)
                return v

            runs = {"level_grid": lambda: eval_3D.compute_level_grid(opt, sdf_net, zs, grid),
                    "isosurface_mesh": lambda: ops.isosurface_mesh(level),
                    "subdivide_1": lambda: ops.mesh_subdivide(*packed, 1),
                    "subdivide_2": lambda: ops.mesh_subdivide(*packed, 2),
                    "subdivide_3": lambda: ops.mesh_subdivide(*packed, 3),
                    "meshes_subdivided_k0": lambda: whole(0),
                    "meshes_subdivided_k2": lambda: whole(2)}
            med, best, reps = _measure(runs, a.iters, a.window_ms)
            fine = whole(2).mesh_subdivided
            at_v, at_c = residuals(packed.verts, packed.faces, S)
            fine_v, fine_c = residuals(fine["verts"], fine["faces"], S)
            print(json.dumps(dict(vox_res=vox, grid_points=S ** 3, vertices=int(packed.v_count[0]), faces=int(packed.f_count[0]),
                                  vertices_out=int(fine["v_count"][0]), faces_out=int(fine["f_count"][0]), edges=int(fine["edges"][0]),
                                  sharp_edges=int(fine["sharp_edges"][0]), grid_pitch=(hi - lo) / (S - 1),
                                  **{name + "_ms": round(v, 4) for name, v in med.items()},
                                  **{name + "_ms_best": round(v, 4) for name, v in best.items()},
                                  resid_before=float(fine["resid_before"][0]), resid_after=float(fine["resid_after"][0]),
                                  disp_mean=float(fine["disp_mean"][0]), disp_max=float(fine["disp_max"][0]),
                                  mean_abs_sdf_vertices=at_v, mean_abs_sdf_centroids=at_c,
                                  subdivided_k2_mean_abs_sdf_vertices=fine_v, subdivided_k2_mean_abs_sdf_centroids=fine_c,
                                  cost_mesh_ms=round(med["level_grid"] + med["isosurface_mesh"], 4),
                                  cost_mesh_subdivided_k2_ms=round(med["level_grid"] + med["isosurface_mesh"] + med["meshes_subdivided_k2"], 4),
                                  network_evaluations_k2=3 * int(fine["v_count"][0]), reps=reps, iters=a.iters)), flush=True)
            del level, grid
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
