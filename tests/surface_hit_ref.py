"""numpy restatement, in fp32, of the two algorithms include/shapeclipper_hip.h states for csrc/surface_hit.hip (sc_ray_first_crossing and
sc_ray_bracket_step), and the crafted rays the GPU tests feed both.  Written from the header's text: every operation is one fp32
operation, every comparison a true comparison (false with a NaN).  tests/test_surface_render_host.py checks it on rays worked out by hand."""
import collections

import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
Bracket = collections.namedtuple("Bracket", ["t_lo", "t_hi", "f_lo", "f_hi", "hit"])


def first_crossing(z_vals, sdf, iso=0.0):
    """z_vals [n,S], sdf [n*S] or [n,S] -> Bracket of fp32 [n] arrays and int32 hit [n]."""
    z = np.asarray(z_vals, F)
    n, S = z.shape
    with np.errstate(all="ignore"):
        f = np.asarray(sdf, F).reshape(n, S) - F(iso)
    assert f.dtype == F
    inside0 = f[:, 0] <= 0
    pair = (f[:, :-1] > 0) & (f[:, 1:] <= 0)                    # pair[r, i]: outside at i, inside at i + 1
    has = pair.any(axis=1) & ~inside0
    i = np.where(has, pair.argmax(axis=1), 0)                    # argmax of booleans: the smallest i that is True
    r = np.arange(n)
    t_lo, t_hi = np.where(has, z[r, i], z[:, 0]), np.where(has, z[r, i + 1], z[:, 0])
    f_lo, f_hi = np.where(has, f[r, i], f[:, 0]), np.where(has, f[r, i + 1], f[:, 0])
    hit = np.where(inside0, 2, np.where(has, 1, 0)).astype(np.int32)
    return Bracket(t_lo.astype(F), t_hi.astype(F), f_lo.astype(F), f_hi.astype(F), hit)


def bracket_step(br, cam_loc, ray_dirs, f_new=None, t_prev=None, iso=0.0):
    """-> (Bracket after the update, t [n], points [n,3]); the inputs are left alone."""
    t_lo, t_hi, f_lo, f_hi = (np.array(a, F) for a in br[:4])
    hit = np.asarray(br.hit, np.int32)
    one = hit == 1
    with np.errstate(all="ignore"):
        if f_new is not None:
            f = np.asarray(f_new, F) - F(iso)
            tp = np.asarray(t_prev, F)
            up, down = one & (f > 0), one & (f <= 0)            # NaN: neither
            t_lo, f_lo = np.where(up, tp, t_lo), np.where(up, f, f_lo)
            t_hi, f_hi = np.where(down, tp, t_hi), np.where(down, f, f_hi)
        d = f_lo - f_hi
        w = f_lo / d
        w = np.where(~(d <= FLT_MAX) | ~((w >= 0) & (w <= 1)), F(0.5), w).astype(F)
        x = t_lo + w * (t_hi - t_lo)
        x = np.where(~(x >= t_lo), t_lo, x)
        x = np.where(~(x <= t_hi), t_hi, x)
        t = np.where(one, x, t_lo).astype(F)
        points = np.asarray(cam_loc, F) + t[:, None] * np.asarray(ray_dirs, F)
    assert points.dtype == F and t.dtype == F
    return Bracket(t_lo.astype(F), t_hi.astype(F), f_lo.astype(F), f_hi.astype(F), hit), t, points


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the rays of the GPU tests ---------------------------------------------------------------------------------------------------------
SEAMS = (63, 127, 191)
NAN, INF = F(np.nan), F(np.inf)


def crafted_rows(S):
    """[(name, f [S] fp32, (hit, i))]: rows of sdf - iso values with the expected hit code and bracket index i (None without one)."""
    rows = []

    def add(name, f, hit, i=None):
        f = np.asarray(f, F)
        assert f.shape == (S,)
        rows.append((name, f, (hit, i)))

    out = np.full(S, 1.0, F)
    add("no crossing", out, 0)
    add("all inside", -out, 2)
    f = out.copy(); f[1:] = -1
    add("pair (0,1)", f, 1, 0)
    f = out.copy(); f[S - 1] = -0.5
    add("pair (S-2,S-1)", f, 1, S - 2)
    for s in SEAMS:
        if s + 1 < S:
            f = out.copy(); f[s + 1:] = -0.25
            add("seam (%d,%d)" % (s, s + 1), f, 1, s)
            f = out.copy(); f[s + 1] = -0.25; f[s + 2:] = 2.0           # one inside sample right behind the seam, outside again after it
            add("seam (%d,%d) alone" % (s, s + 1), f, 1, s)
    f = out.copy(); f[7] = 0.0
    add("f_{i+1} == 0", f, 1, 6)
    f = out.copy(); f[7] = -0.0
    add("f_{i+1} == -0", f, 1, 6)
    f = out.copy(); f[0] = 0.0
    add("f_0 == 0", f, 2)
    f = out.copy(); f[0] = -3.0; f[5:] = -1.0
    add("f_0 < 0 with a later crossing", f, 2)
    # starts outside, dips inside at 3..5 (crossing (2,3)), leaves at (5,6), enters again at (9,10): the first entry wins
    f = out.copy(); f[3:6] = -1.0; f[10:] = -2.0
    add("several crossings", f, 1, 2)
    # an inside -> outside pair before the first outside -> inside pair cannot exist after f_0 > 0 without an entry before it; what can is a
    # start that dips to exactly 0 at sample 1 (an entry, (0,1)), or a NaN dip that hides the entry: samples 1..2 NaN, 3 inside, 4 outside
    # ((3,4) is inside -> outside and is passed over), then the entry at (8,9)
    f = out.copy(); f[1:3] = NAN; f[3] = -1.0; f[9:] = -1.0
    add("inside->outside pair first", f, 1, 8)
    f = out.copy(); f[10] = NAN; f[11:] = -1.0
    add("NaN at the bracket's outside end", f, 0)
    f = out.copy(); f[10:] = -1.0; f[11] = NAN
    add("NaN right after the bracket", f, 1, 9)
    f = out.copy(); f[4] = NAN; f[10:] = -1.0
    add("NaN before the bracket", f, 1, 9)
    f = out.copy(); f[10] = NAN; f[11] = 1.0; f[20:] = -1.0
    add("NaN at the inside end, later entry", f, 1, 19)
    f = out.copy(); f[0] = NAN; f[1:] = -1.0
    add("NaN at sample 0", f, 0)
    f = out.copy(); f[9] = INF; f[10:] = -INF
    add("+Inf -> -Inf", f, 1, 9)
    f = out.copy(); f[:5] = INF; f[12] = -INF; f[13:] = 3.0
    add("Inf before, -Inf alone", f, 1, 11)
    f = out.copy(); f[0] = -INF
    add("f_0 == -Inf", f, 2)
    f = np.full(S, NAN, F)
    add("all NaN", f, 0)
    f = out.copy(); f[S - 1] = 0.0
    add("zero at the last sample", f, 1, S - 2)
    f = out.copy(); f[S - 1] = NAN
    add("NaN at the last sample", f, 0)
    return rows


def crossing_case(S, n_rays=130, seed=0, iso=0.0):
    """(z_vals [n_rays,S], sdf [n_rays*S], expected [(hit, i)] of the crafted rows that lead the batch): the crafted rows (as sdf = f + iso
    would not be exact, they are used with iso = 0 as they are and shifted by an exactly representable iso otherwise), then seeded random
    rows: white noise (a crossing almost at once), noise with NaN / Inf sprinkled in, and smooth |z - c| - r profiles."""
    rng = np.random.RandomState(seed + S)
    rows = crafted_rows(S)
    assert len(rows) < n_rays
    f = np.empty((n_rays, S), F)
    for k, (_, row, _) in enumerate(rows):
        f[k] = row
    near = rng.uniform(3.8, 5.0, n_rays).astype(F)
    z = np.stack([np.linspace(a, a + F(1.4), S, dtype=F) for a in near])
    for k in range(len(rows), n_rays):
        kind = k % 4
        if kind == 0:
            f[k] = rng.standard_normal(S)
        elif kind == 1:
            f[k] = rng.standard_normal(S) + 1.5
            f[k, rng.randint(0, S, 3)] = (NAN, INF, -INF)
        else:
            c, r = rng.uniform(z[k, 0] - 0.2, z[k, -1] + 0.2), rng.uniform(0.0, 0.6)
            f[k] = np.abs(z[k] - F(c)) - F(r) if kind == 2 else np.minimum(np.abs(z[k] - F(c)) - F(r), np.abs(z[k] - z[k, S // 2]) - F(0.05))
    if iso:
        with np.errstate(all="ignore"):
            f = (f.astype(np.float64) + iso).astype(F)
    return z, f.reshape(-1), [e for _, _, e in rows]


def step_case(n_rays=130, seed=0):
    """Brackets for the step kernel: hit codes 0 / 1 / 2 mixed, f_lo > 0 >= f_hi on the hit == 1 rays, the first rows crafted:
    0: f_lo - f_hi overflows (finite values)   1: f_lo = +Inf   2: f_hi = -Inf   3: f_hi = 0   4: t_lo == t_hi   5: tiny f_lo (w rounds to 0)
    -> (Bracket, cam_loc [n,3], ray_dirs [n,3])."""
    rng = np.random.RandomState(seed)
    t_lo = rng.uniform(4.0, 5.0, n_rays).astype(F)
    t_hi = (t_lo + rng.uniform(0.001, 0.05, n_rays).astype(F)).astype(F)
    f_lo = rng.uniform(1e-4, 0.05, n_rays).astype(F)
    f_hi = (-rng.uniform(0.0, 0.05, n_rays)).astype(F)
    hit = rng.choice([0, 1, 1, 1, 2], n_rays).astype(np.int32)
    hit[:6] = 1
    f_lo[0], f_hi[0] = F(3e38), F(-3e38)
    f_lo[1] = INF
    f_hi[2] = -INF
    f_hi[3] = 0.0
    t_hi[4] = t_lo[4]
    f_lo[5], f_hi[5] = F(1e-45), F(-1.0)
    same = hit != 1                                               # what the crossing kernel leaves on those rays
    t_hi[same], f_hi[same] = t_lo[same], f_lo[same]
    f_lo[hit == 2] = -np.abs(f_lo[hit == 2])
    f_hi[hit == 2] = f_lo[hit == 2]
    cam = rng.uniform(-5, 5, (n_rays, 3)).astype(F)
    d = rng.standard_normal((n_rays, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    return Bracket(t_lo, t_hi, f_lo, f_hi, hit), cam, d


def step_values(t, k):
    """A made-up fp32 'SDF along the ray' for the step tests: a cubic through the middle of [4, 5.05] per ray, with NaN, 0, +-Inf and huge
    values at a few fixed rays of round k."""
    t = np.asarray(t, F)
    with np.errstate(all="ignore"):
        f = (F(4.5) - t) * (F(1.0) + (t - F(4.2)) * (t - F(4.2)))
    f = f.astype(F)
    n = len(f)
    f[(7 + k) % n] = NAN
    f[(11 + k) % n] = 0.0
    f[(13 + k) % n] = INF
    f[(17 + k) % n] = -INF
    f[(19 + k) % n] = F(3e38)
    f[(23 + k) % n] = F(-3e38)
    return f
