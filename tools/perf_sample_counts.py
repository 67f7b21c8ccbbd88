"""Render cost against the sample count S (render.n_samples_uniform), HIP kernels against model/eager_path.py.

For S in --samples (default 32, 64, 128, 256): the training render plus its backward at B images x R rays, and the evaluation render of
one FULL x FULL image, each on the HIP path and on the eager path (stock device operators, the path these sample counts took before the
render kernels walked a ray in chunks of 64 samples).  Method: every (path, S, case) is warmed up, then timed with device events around
--iters calls, --repeats times; the median of the repeats is reported, in ms per call and in ns per sample point (B * R * S points for
training, FULL^2 * S for evaluation).  One process, one device, so the whole table comes from one box.  Prints the table and one JSON line.

    python tools/perf_sample_counts.py [--B 32 --R 512 --full 64 --samples 32,64,128,256 --iters 5 --repeats 5 --no-eager]
"""
import argparse
import json
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402


def build(S, B, R, full, eager):
    from shapeclipper_amd.model.implicit import RGBNetwork, SDFNetwork
    from shapeclipper_amd.model.renderer import Renderer
    from shapeclipper_amd.utils import camera, options
    dev = torch.device("cuda:0")
    opt = options.set(options.parse_arguments(["--yaml=options/pix3d/config.yaml", "--name=perf_ns", "--output_root=/tmp/sc_perf",
                                               "--render.n_samples_uniform=%d" % S]), verbose=False)
    torch.manual_seed(0)
    sdf, rgb = SDFNetwork(opt), RGBNetwork(opt)
    if eager:
        sdf.eager = rgb.eager = True
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = Renderer(opt, sdf, rgb).to(dev)
    assert r.eager == eager, (S, eager)
    az = (torch.rand(B) * 2 - 1) * 3.14159
    trig = lambda t: torch.stack([torch.cos(t), torch.sin(t)], 1)
    Ry = camera.azim_to_rotation_matrix(trig(az), "trig")
    Rx = camera.elev_to_rotation_matrix(trig(torch.zeros(B)), "trig")
    P = torch.tensor([[-1., 0, 0], [0, 0, -1], [0, -1, 0]])[None].expand(B, 3, 3)
    pose = camera.pose.compose([camera.pose(R=Rx @ Ry @ P), camera.pose(t=torch.tensor([[0., 0, 5.]]).expand(B, 3))]).to(dev)
    leaves = dict(pose=pose.requires_grad_(True), sd=torch.ones(B, device=dev, requires_grad=True),
                  zs=torch.randn(B, 64, device=dev, requires_grad=True), zr=torch.randn(B, 64, device=dev, requires_grad=True))
    opt.H = opt.W = 224
    intr = camera.get_intr(opt, torch.ones(B)).to(dev)
    ray_idx = torch.stack([torch.randperm(224 * 224)[:R] for _ in range(B)]).to(dev)

    def train():
        opt.H = opt.W = 224
        out = r(opt, leaves["pose"], intr, leaves["sd"], leaves["zs"], leaves["zr"], ray_idx=ray_idx, training=True)
        (out[0].sum() + out[1].sum() + out[3].sum() + out[4].sum() + ((out[5] - 1) ** 2).mean()).backward()

    opt_e = dict(H=full, W=full)
    intr_e = None

    def evaluate():
        nonlocal intr_e
        opt.H, opt.W = opt_e["H"], opt_e["W"]
        if intr_e is None:
            intr_e = camera.get_intr(opt, torch.ones(1)).to(dev)
        with torch.no_grad():
            r(opt, leaves["pose"][:1].detach(), intr_e, leaves["sd"][:1].detach(), leaves["zs"][:1].detach(), leaves["zr"][:1].detach(),
              ray_idx=None, training=False)
    return train, evaluate


def timed(fn, iters, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e) / iters)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--R", type=int, default=512)
    ap.add_argument("--full", type=int, default=64)
    ap.add_argument("--samples", default="32,64,128,256")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-eager", action="store_true", help="HIP path only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perf_sample_counts: no GPU -- nothing to measure")
    rows = []
    print("%-6s %5s %-6s %10s %10s %10s %12s" % ("path", "S", "case", "ms median", "ms min", "ms max", "ns / point"))
    for S in [int(x) for x in a.samples.split(",")]:
        for eager in ([False] if a.no_eager else [False, True]):
            train, evaluate = build(S, a.B, a.R, a.full, eager)
            for case, fn, pts in (("train", train, a.B * a.R * S), ("eval", evaluate, a.full * a.full * S)):
                med, lo, hi = timed(fn, a.iters, a.repeats)
                row = dict(path="eager" if eager else "hip", S=S, case=case, ms=round(med, 3), ms_min=round(lo, 3), ms_max=round(hi, 3),
                           ns_per_point=round(med * 1e6 / pts, 3))
                rows.append(row)
                print("%-6s %5d %-6s %10.3f %10.3f %10.3f %12.3f" % (row["path"], S, case, med, lo, hi, row["ns_per_point"]))
            torch.cuda.empty_cache()
    print(json.dumps(dict(B=a.B, R=a.R, full=a.full, iters=a.iters, repeats=a.repeats, rows=rows)))


if __name__ == "__main__":
    main()
