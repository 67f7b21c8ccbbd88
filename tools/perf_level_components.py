"""ops.level_largest_component (csrc/level_components.hip) timed with device events beside the two stages it sits between: the level grid
of the same size (ops.sdf_forward, value only, what eval_3D.compute_level_grid runs) and its marching cubes (ops.isosurface_triangles).
Sizes: S = 65, B = 1; S = 65, B = 32; S = 257, B = 1.  Inputs: a ball with floaters, and a random occupancy of 0.3 (thousands of components
around the percolation threshold: the label-merging worst case).  One JSON line per (size, input).  Per-kernel times of the five launches:
run this tool under `rocprofv3 --kernel-trace --stats` (the kernels are named lc_*_kernel).
python tools/perf_level_components.py [--iters N]"""
import argparse, json, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch


def ball_with_floaters(B, S, dev):
    """A ball of radius 0.3..0.4 (drawn per image) and 12 floaters of radius 0.03..0.06 spread over [-0.6, 0.6]^3: signed distances."""
    ax = torch.linspace(-0.6, 0.6, S, device=dev)
    P = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1)
    gen = torch.Generator(device=dev).manual_seed(0)
    level = P.norm(dim=-1)[None] - (0.3 + 0.1 * torch.rand(B, 1, 1, 1, device=dev, generator=gen))
    c = torch.rand(12, 3, device=dev, generator=gen) * 1.1 - 0.55
    r = 0.03 + 0.03 * torch.rand(12, device=dev, generator=gen)
    for k in range(12):
        level = torch.minimum(level, ((P - c[k]).norm(dim=-1) - r[k])[None])
    return level.contiguous()


def random_occupancy(B, S, dev, p=0.3):
    gen = torch.Generator(device=dev).manual_seed(1)
    return (torch.rand(B, S, S, S, device=dev, generator=gen) - p).contiguous()


def timed(fn, iters):
    fn(); fn()                                                       # warm-up: code objects, allocator, scratch
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return round(sorted(ms)[len(ms) // 2], 4), round(min(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from shapeclipper_amd import ops
    from shapeclipper_amd.model.implicit import SDFNetwork
    from shapeclipper_amd.utils import options
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=%s/options/pix3d/config.yaml" % ROOT, "--name=perf_level_components",
                                               "--output_root=/tmp/sc_perf"]), verbose=False)
    torch.manual_seed(0)
    net = SDFNetwork(opt).to(dev)
    for B, S in ((1, 65), (32, 65), (1, 257)):
        with torch.no_grad():
            w_pack, cbias = net.packed(torch.randn(B, net.proj_latent_dim, device=dev) * 0.3)
        ax = torch.linspace(-0.6, 0.6, S, device=dev)
        pts = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3).repeat(B, 1).contiguous()
        grid_ms = timed(lambda: ops.sdf_forward(pts, w_pack, cbias, S ** 3, symmetric=bool(net.force_symmetry), want_grad=False,
                                                want_feat=False), a.iters)
        del pts
        for name, level in (("ball + 12 floaters", ball_with_floaters(B, S, dev)), ("random occupancy 0.3", random_occupancy(B, S, dev))):
            filt_ms = timed(lambda: ops.level_largest_component(level, 0.0), a.iters)
            out, st = ops.level_largest_component(level, 0.0)
            mc_ms = timed(lambda: ops.isosurface_triangles(out, 0.0), max(a.iters // 2, 3))
            print(json.dumps(dict(S=S, B=B, input=name, components=int(st.n_components.sum()), inside_voxels=int(st.inside_voxels.sum()),
                                  kept_voxels=int(st.kept_voxels.sum()), filter_ms=filt_ms[0], filter_ms_best=filt_ms[1],
                                  level_grid_ms=grid_ms[0], level_grid_ms_best=grid_ms[1], marching_cubes_ms=mc_ms[0],
                                  marching_cubes_ms_best=mc_ms[1], iters=a.iters,
                                  note="medians of device-event times; marching cubes (of the filtered grid) includes its one host read")),
                  flush=True)


if __name__ == "__main__":
    main()
