"""numpy restatement of sc_level_largest_component (include/shapeclipper_hip.h) and the grids its tests run on.  Not a test module.

The restatement is a plain flood fill: seeds are taken in increasing linear index (x S + y) S + z, so a component's seed is its label;
a fill visits the six face neighbours; the first component of the largest size is kept; every other inside voxel becomes
iso + (iso - level) in fp32."""
import functools

import numpy as np


def largest_component(level, iso=0.0):
    """level [S,S,S] fp32 -> dict(out [S,S,S] fp32, n_components, inside_voxels, kept_voxels, kept_label, components [(label, size)])."""
    level = np.ascontiguousarray(level, np.float32)
    iso = np.float32(iso)
    S = level.shape[0]
    assert level.shape == (S, S, S)
    with np.errstate(invalid="ignore"):
        inside = level < iso                                        # NaN: False
    P = S + 2                                                       # one layer of outside voxels all round: no bounds checks in the fill
    pad = np.zeros((P, P, P), np.uint8)
    pad[1:-1, 1:-1, 1:-1] = inside
    todo = bytearray(pad.tobytes())                                 # 1: inside and not yet visited
    offsets = (1, -1, P, -P, P * P, -P * P)
    unpad = lambda v: ((v // (P * P) - 1) * S + (v // P % P - 1)) * S + (v % P - 1)
    components, best = [], []
    for seed in np.flatnonzero(pad.reshape(-1)).tolist():           # increasing padded index = increasing grid index
        if not todo[seed]:
            continue
        todo[seed] = 0
        stack, members = [seed], []
        while stack:
            v = stack.pop()
            members.append(v)
            for d in offsets:
                w = v + d
                if todo[w]:
                    todo[w] = 0
                    stack.append(w)
        components.append((unpad(seed), len(members)))
        if len(members) > len(best):                                # strictly larger: on a tie the earlier (smaller) label stays
            best = members
    keep = np.zeros(P * P * P, bool)
    keep[best] = True
    keep = keep.reshape(P, P, P)[1:-1, 1:-1, 1:-1]
    flip = inside & ~keep
    out = level.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        out[flip] = iso + (iso - level[flip])
    return dict(out=out, n_components=len(components), inside_voxels=int(inside.sum()), kept_voxels=len(best),
                kept_label=unpad(best[0]) if best else -1, components=components)


# ---- grids ---------------------------------------------------------------------------------------------------------------------------
KINDS = ("two_balls", "ball_floater", "checker", "serpentine", "random25", "random31", "random50", "tie", "none", "all", "one", "nonfinite")
NAN_PAYLOADS = (0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FFFFFFF)


def _coords(S):
    g = np.linspace(-1.0, 1.0, S, dtype=np.float32)
    return np.meshgrid(g, g, g, indexing="ij")


def _ball(S, centre, radius):
    x, y, z = _coords(S)
    return (np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2) - np.float32(radius)).astype(np.float32)


def serpentine_mask(S):
    """A one-voxel-wide path through the whole grid: rows along z at even y, joined at alternating ends by one voxel at odd y, in every
    even x layer; consecutive layers joined by one voxel at odd x, alternately at the layer path's end and at its start."""
    m = np.zeros((S, S, S), bool)
    layer = np.zeros((S, S), bool)
    layer[0::2, :] = True
    for y in range(1, S, 2):
        if y + 1 < S:
            layer[y, S - 1 if (y // 2) % 2 == 0 else 0] = True
    rows = (S + 1) // 2
    end = (2 * (rows - 1), S - 1 if rows % 2 == 1 else 0)
    for x in range(0, S, 2):
        m[x] = layer
        if x + 2 < S:
            m[(x + 1,) + (end if (x // 2) % 2 == 0 else (0, 0))] = True
    return m


def base_grid(kind, S, iso):
    """The first image of `kind` at side S: fp32 [S,S,S] whose inside set (level < iso) is the shape the kind names."""
    iso = np.float32(iso)
    rng = np.random.RandomState(1000 + S)
    mag = rng.uniform(0.01, 1.0, (S, S, S)).astype(np.float32)
    signed = lambda mask: (np.where(mask, -mag, mag) + iso).astype(np.float32)
    if kind == "two_balls":
        return np.minimum(_ball(S, (-0.3, -0.2, -0.1), 0.45), _ball(S, (0.55, 0.5, 0.45), 0.22)) + iso
    if kind == "ball_floater":
        g = _ball(S, (0.0, 0.0, 0.0), 0.5) + iso
        g[S - 1, S - 1, S - 1] = iso - np.float32(0.25)
        return g
    if kind == "one":
        return _ball(S, (0.1, 0.0, -0.1), 0.7) + iso
    if kind == "checker":                                           # no two inside voxels share a face; all touch by edges and corners
        x, y, z = np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij")
        return signed((x + y + z) % 2 == 0)
    if kind == "serpentine":
        return signed(serpentine_mask(S))
    if kind.startswith("random"):
        p = int(kind[len("random"):]) / 100.0
        return (rng.uniform(0.0, 1.0, (S, S, S)) - p).astype(np.float32) + iso
    if kind == "tie":                                               # two bars of equal length in opposite corners
        L = max(1, S // 2)
        m = np.zeros((S, S, S), bool)
        m[0, 0, :L] = True
        m[S - 1, S - 1, S - L:] = True
        return signed(m)
    if kind == "none":
        return signed(np.zeros((S, S, S), bool))
    if kind == "all":
        return signed(np.ones((S, S, S), bool))
    if kind == "nonfinite":
        g = (rng.uniform(0.0, 1.0, (S, S, S)) - 0.31).astype(np.float32) + iso
        what = rng.randint(0, 40, (S, S, S))
        bits = g.view(np.uint32).copy()
        for k, payload in enumerate(NAN_PAYLOADS):
            bits[what == k] = np.uint32(payload)
        g = bits.view(np.float32).copy()
        g[what == 4] = np.inf
        g[what == 5] = -np.inf
        return g
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def image(kind, S, iso, k):
    """Image k of a batch of `kind`: the base grid (k = 0), mirrored along x (1), with its axes rotated (2).  Read-only."""
    g = base_grid(kind, S, iso)
    g = (g, g[::-1], g.transpose(2, 0, 1))[k % 3]
    g = np.ascontiguousarray(g, np.float32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expected(kind, S, iso, k):
    """The restatement on image(kind, S, iso, k), computed once and shared; out is read-only."""
    r = largest_component(image(kind, S, iso, k), iso)
    r["out"].setflags(write=False)
    return r
