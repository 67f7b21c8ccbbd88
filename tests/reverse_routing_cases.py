"""Case tables of tests/test_gpu_reverse_image_routing.py and the launch partitions of the two fused reverse kernels restated in plain
Python (no GPU, no torch): tests/test_reverse_partition_host.py proves with them that every case runs the branch it is named for.

csrc/sdf_bwdw.hip (sc_sdf_backward_fused): 16-point tiles; blocks = clamp(ceil(ntiles / 4), 1, 256) workgroups; a workgroup owns the
tiles [b per_wg, min(ntiles, (b + 1) per_wg)) with per_wg = ceil(ntiles / blocks) rounded up to a multiple of the 4 chain waves, and
walks them 4 at a time.  The weight-gradient waves keep ONE per-image bias accumulator while an iteration lies in one image (flushed
when the image changes and after the last iteration) and add per tile when the first and the last tile of an iteration belong to
different images ("mixed").  Up to 256 images the sums go into a per-workgroup [n_images][5][64] block behind the packed weight
gradient ("dense": partial stride = pack + 320 n_images floats); beyond, by float atomicAdd into the caller-zeroed g_cbias.

csrc/rgb_bwd.hip (the FUSED forms): grid = clamp(ceil(n_rays / 4), 1, 256) workgroups; the ray of (iteration, block, wave) is
(it grid + block) 4 + wave; the same accumulator / mixed scheme per 4-ray iteration; at most 256 images, always dense."""
BW_CHAIN = 4            # chain waves = tiles (SDF) or rays (RGB) of one iteration
TILE = 16
MAX_WORKGROUPS = 256    # both kernels
DENSE_MAX_IMAGES = 256  # sc_sdf_backward_fused_partial_floats; the fused RGB entry points refuse more
SDF_PACK_FLOATS = 64 * 48 + 2 * 64 * 112 + 2 * 64 * 64 + 65 * 64 + 65
RGB_V3_OFFSET = 64 * 112 + 2 * 64 * 64      # floats of dV0 | dV1 | dV2 in a partial image of the RGB kernel

# ---------------------------------------------------------------------------------------------------------------------------------
# SDF fused reverse: (B, N) -> what the case is there for.  idle: workgroups with an empty tile range; iters / mixed: iterations of the
# launch and those of them that straddle images; span: most images in one iteration; flushes: accumulator flushes that carry a sum;
# dense: False = the atomic form.  FEAT_ABSENT also runs with g_feat = None.
# Measured on the MI355X, the same in three runs: worst of the default / twins arms in units of the fp32 oracle's error (K_SDF_BWD = 4 each):
#   (B, N)      w_sdf     z  points     (B, N)      w_sdf     z  points     (B, N)      w_sdf     z  points
#   (5, 16)      1.33  0.62    0.96     (130, 64)    1.33  0.78    0.71     (300, 32)    3.70  0.99    0.69
#   (7, 48)      1.27  1.14    0.83     (256, 16)    1.45  0.94    1.51     (5, 3296)    1.02  0.83    1.25
#   (64, 32)     1.04  0.91    1.02     (257, 16)    1.64  1.04    0.76     (260, 64)    1.68  1.14    1.35
# (7, 48) without the feature term: 1.27, 1.14, 0.82.  The 3.70 is lin5.bias, a sum of one term per point (4.5e-7 of max against the oracle's
# 1.2e-7; 0.62 of rule (b)'s bound); every other tensor of that case is at most 1.44.  Leak test, image h's g_cbias rows / g_points:
# at most 2.74 / 2.28 (one image of 16 points).  The atomic cases add at most two terms per address, so their sums do not depend on the
# order either: the atomic form is no further from float64 than the dense one and K_SDF_BWD holds for it unchanged.
# ---------------------------------------------------------------------------------------------------------------------------------
SDF_CASES = {
    (5, 16): dict(blocks=2, idle=0, iters=2, mixed=1, span=4, flushes=1, dense=True),          # 4 images in one iteration, then a lone tile
    (7, 48): dict(blocks=6, idle=0, iters=6, mixed=5, span=2, flushes=1, dense=True),          # 3 tiles / image: an iteration never fits
    (64, 32): dict(blocks=32, idle=0, iters=32, mixed=32, span=2, flushes=0, dense=True),      # every iteration mixed across 2 images
    (130, 64): dict(blocks=130, idle=0, iters=130, mixed=0, span=1, flushes=130, dense=True),  # never mixed, a flush per iteration
    (256, 16): dict(blocks=64, idle=0, iters=64, mixed=64, span=4, flushes=0, dense=True),     # largest dense form, 4 images / iteration
    (257, 16): dict(blocks=65, idle=0, iters=65, mixed=64, span=4, flushes=1, dense=False),    # smallest atomic form
    (300, 32): dict(blocks=150, idle=0, iters=150, mixed=150, span=2, flushes=0, dense=False),  # atomic form, 2-image iterations
    (5, 3296): dict(blocks=256, idle=127, iters=258, mixed=2, span=2, flushes=130, dense=True),  # 1030 tiles: 129 workgroups work
    (260, 64): dict(blocks=256, idle=126, iters=260, mixed=0, span=1, flushes=260, dense=False),  # idle workgroups + atomic form
}
SDF_FEAT_ABSENT = (7, 48)                   # the case that also runs without the feature term
SDF_LEAK_CASES = [(256, 16), (257, 16), (64, 32), (5, 3296)]
SDF_BATCH_CASES = [(7, 48), (257, 16), (5, 3296)]

# ---------------------------------------------------------------------------------------------------------------------------------
# RGB fused reverse: (n_images, rays / image, S).
# Measured on the MI355X: worst of the default / twins arms in units of the fp32 oracle's error (K_RGB = 4, 8, 4, 4); in brackets the
# largest share of rule (b)'s bound K err(oracle) + 2^-22:
#   case            out   point  w_rgb  latent      case            out   point         w_rgb  latent
#   (5, 1, 64)     0.84    3.63   1.84  < floor     (256, 1, 64)   0.67    2.36   4.82 (0.86)    1.32
#   (7, 3, 64)     1.45    1.76   1.56    1.37      (256, 1, 32)   1.22    1.48   5.08 (0.68)    1.65
#   (64, 2, 64)    1.01    2.28   2.27    1.60
# The two w_rgb figures above K are the bias gradients of lin0 (S = 64) and lin2 (S = 32) -- sums over all 256 images' rows, 7.2e-7 and 3.5e-7 of
# max where the fp32 oracle happens to be at 1.5e-7 and 7.0e-8, one ulp -- and lie inside the rule through its 2^-22 floor; every other tensor
# is at most 2.27.  The rows themselves pass the leak test (other images exactly zero, image h's g_dbias rows at most 1.74, per-sample
# gradients at most 4.19 x the oracle on one ray of 64 samples): rounding of a sum, not routing.
# ---------------------------------------------------------------------------------------------------------------------------------
RGB_CASES = {
    (5, 1, 64): dict(blocks=2, iters=2, mixed=1, span=4, flushes=1),
    (7, 3, 64): dict(blocks=6, iters=6, mixed=5, span=2, flushes=1),
    (64, 2, 64): dict(blocks=32, iters=32, mixed=32, span=2, flushes=0),
    (256, 1, 64): dict(blocks=64, iters=64, mixed=64, span=4, flushes=0),
    (256, 1, 32): dict(blocks=64, iters=64, mixed=64, span=4, flushes=0),
}
RGB_LEAK_CASES = [(256, 1, 64), (7, 3, 64)]


def hot_images(B):
    return sorted({0, B // 2, B - 1})


def _walk(ranges, unit_image, n_images):
    """The accumulator state machine of the weight-gradient waves over every workgroup's iterations.  ranges: per workgroup the list of
    iterations, each the list of its (at most 4) units in range; unit_image: unit -> image.  Returns the counts of the case tables."""
    iters = mixed = flushes = span = 0
    for its in ranges:
        cur = -1
        for units in its:
            img0, img3 = min(unit_image(units[0]), n_images - 1), min(unit_image(units[-1]), n_images - 1)
            if img0 != cur or img3 != img0:
                flushes += cur >= 0
                cur = img0 if img0 == img3 else -2
            iters += 1
            mixed += cur == -2
            span = max(span, len({unit_image(u) for u in units}))
        flushes += cur >= 0
    return dict(iters=iters, mixed=mixed, flushes=flushes, span=span)


def sdf_parts(n_points):
    ntiles = (n_points + TILE - 1) // TILE
    return max(1, min(MAX_WORKGROUPS, (ntiles + BW_CHAIN - 1) // BW_CHAIN))


def sdf_partial_floats(n_images):
    return SDF_PACK_FLOATS + (320 * n_images if 0 < n_images <= DENSE_MAX_IMAGES else 0)


def sdf_partition(B, N):
    assert N % TILE == 0
    ntiles = (B * N + TILE - 1) // TILE
    blocks = sdf_parts(B * N)
    per_wg = -(-(-(-ntiles // blocks)) // BW_CHAIN) * BW_CHAIN
    ranges, idle = [], 0
    for b in range(blocks):
        t0, t1 = b * per_wg, min(ntiles, (b + 1) * per_wg)
        idle += t1 <= t0
        ranges.append([list(range(base, min(base + BW_CHAIN, t1))) for base in range(t0, t1, BW_CHAIN)])
    tiles_per_image = N // TILE
    out = _walk(ranges, lambda t: t // tiles_per_image, B)
    out.update(blocks=blocks, idle=idle, per_wg=per_wg, ntiles=ntiles, dense=sdf_partial_floats(B) > SDF_PACK_FLOATS,
               stride=sdf_partial_floats(B), covered=sorted(t for its in ranges for units in its for t in units) == list(range(ntiles)))
    return out


def rgb_parts(n_rays):
    return max(1, min(MAX_WORKGROUPS, (n_rays + 3) // 4))


def rgb_partial_floats(n_images):
    return RGB_V3_OFFSET + 192 * n_images


def rgb_partition(n_images, rpi):
    n_rays = n_images * rpi
    grid = rgb_parts(n_rays)
    n_iter = (n_rays + grid * 4 - 1) // (grid * 4)
    ranges = []
    for b in range(grid):
        its = []
        for it in range(n_iter):
            ray0 = (it * grid + b) * 4
            # the kernel walks an iteration past the last ray with both ends clamped to it: an accumulator of the last image that
            # receives zeros only
            its.append(list(range(ray0, min(ray0 + 4, n_rays))) or [n_rays - 1])
        ranges.append(its)
    out = _walk(ranges, lambda r: r // rpi, n_images)
    rays = sorted(r for its in ranges for units in its for r in units)
    out.update(blocks=grid, n_iter=n_iter, stride=rgb_partial_floats(n_images), covered=sorted(set(rays)) == list(range(n_rays)))
    return out
