"""numpy restatement of sc_emd3d_match (include/shapeclipper_hip.h states the rule; csrc/emd3d.hip implements it) and the exact optimum
it is measured against.  Everything a bid is made of is fp32 and rounds once per operation, the order of the header; numpy's fp32 sqrt is
correctly rounded like the kernel's.  The rounds are Jacobi -- every bid of a round is computed from the state at its start -- and the
winner of an object is the maximum of a total order on (bid, person), so the result does not depend on the order the bids are made in:
the restatement makes them all at once by array operations."""
import collections

import numpy as np

F32 = np.float32
EPS_LIST_MAX = 80           # SC_EMD3D_MAX_PHASES of the header

EmdRef = collections.namedtuple("EmdRef", ["assignment", "cost", "price", "emd", "rounds", "converged"])


def eps_list(eps=1e-4, eps_start=0.25):
    """The epsilon of every phase, fp32: e = eps_start; while e > eps: emit e, e = fl(e / 4); then emit eps."""
    eps, e, out = F32(eps), F32(eps_start), []
    while e > eps:
        out.append(e)
        e = F32(e / F32(4))
    out.append(eps)
    return np.array(out, dtype=F32)


def cost_matrix(a, b):
    """[n,n] fp32, c[i,j] = sqrt((dx dx + dy dy) + dz dz) of person i and object j, one rounding per operation."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    dx = a[:, None, 0] - b[None, :, 0]
    dy = a[:, None, 1] - b[None, :, 1]
    dz = a[:, None, 2] - b[None, :, 2]
    return np.sqrt((dx * dx + dy * dy) + dz * dz)


def emd_match_one(a, b, eps=1e-4, eps_start=0.25, max_rounds=1 << 18):
    """One image: a, b [n,3] fp32 -> EmdRef of arrays / scalars."""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32)
    n = a.shape[0]
    assert a.shape == b.shape == (n, 3) and 2 <= n <= 2048
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return EmdRef(np.arange(n, dtype=np.int32), np.zeros(n, F32), np.zeros(n, F32), np.float64("nan"), np.int32(0), np.int32(0))
    with np.errstate(all="ignore"):
        c = cost_matrix(a, b)
        neg_c = -c
        price = np.zeros(n, F32)
        obj_of = np.full(n, -1, np.int64)           # the object of a person, -1 = unassigned
        owner = np.full(n, -1, np.int64)            # the person of an object, -1 = unowned
        rounds, converged = 0, 1
        for e in eps_list(eps, eps_start):
            obj_of[:] = -1
            owner[:] = -1
            while True:
                bidders = np.flatnonzero(obj_of < 0)
                if bidders.size == 0:
                    break
                if rounds >= max_rounds:
                    converged = 0
                    break
                w = neg_c[bidders] - price[None, :]                                 # fl(fl(-c) - p)
                rows = np.arange(bidders.size)
                j1 = np.argmax(w, axis=1)                                           # the lowest j among the maxima
                w1 = w[rows, j1]
                w[rows, j1] = -np.inf
                w2 = np.max(w, axis=1)
                bid = price[j1] + ((w1 - w2) + e)
                key = (bid.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - bidders.astype(np.uint64))
                best = np.zeros(n, np.uint64)
                np.maximum.at(best, j1, key)
                js = np.flatnonzero(best)                                           # the objects that received a bid
                winners = (np.uint64(0xFFFFFFFF) - (best[js] & np.uint64(0xFFFFFFFF))).astype(np.int64)
                prev = owner[js]
                obj_of[prev[prev >= 0]] = -1                                        # (an owner did not bid: never a winner of this round)
                owner[js] = winners
                obj_of[winners] = js
                price[js] = (best[js] >> np.uint64(32)).astype(np.uint32).view(F32)
                rounds += 1
            if not converged:
                break
        if not converged:                           # the unassigned persons in ascending index take the unowned objects in ascending index
            obj_of[np.flatnonzero(obj_of < 0)] = np.flatnonzero(owner < 0)
        cost = c[np.arange(n), obj_of]
    total = np.float64(0)
    for v in cost:                                  # ascending i, float64
        total = total + np.float64(v)
    return EmdRef(obj_of.astype(np.int32), cost.astype(F32), price, total / np.float64(n), np.int32(rounds), np.int32(converged))


def emd_match(a, b, eps=1e-4, eps_start=0.25, max_rounds=1 << 18):
    """a, b [B,n,3] -> EmdRef of stacked arrays: assignment [B,n] int32, cost, price [B,n] fp32, emd [B] float64, rounds, converged [B] int32."""
    res = [emd_match_one(x, y, eps, eps_start, max_rounds) for x, y in zip(np.asarray(a), np.asarray(b))]
    return EmdRef(*(np.stack([np.asarray(r[k]) for r in res]) for k in range(6)))


def exact_emd(a, b):
    """(emd, assignment) of the optimal bijection for the float64 view of the same fp32 cost matrix."""
    from scipy.optimize import linear_sum_assignment
    c = cost_matrix(a, b).astype(np.float64)
    rows, cols = linear_sum_assignment(c)
    return c[rows, cols].sum() / c.shape[0], cols


def slack_delta(c, price):
    """The rounding slack of epsilon-complementary slackness: the five fp32 roundings that form a bid each err by at most 2^-24 of a
    magnitude at most max c + max p; 8 of them bound the sum with room."""
    return 8.0 * 2.0 ** -24 * (float(np.max(c)) + float(np.max(price)))


def slackness_excess(a, b, assignment, price):
    """max_i [ max_j(-c_ij - p_j) - (-c_i,phi(i) - p_phi(i)) ] in float64: at most eps + slack_delta for a converged auction."""
    c = cost_matrix(a, b).astype(np.float64)
    v = -c - np.asarray(price, dtype=np.float64)[None, :]
    return float(np.max(v.max(axis=1) - v[np.arange(c.shape[0]), np.asarray(assignment)]))


# ---- the inputs of the tests ---------------------------------------------------------------------------------------------------------
def sphere_cube(n, seed=0):
    """n points on the sphere of radius 0.5 against n uniform points of [-0.5, 0.5]^3."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((n, 3))
    s = 0.5 * s / np.linalg.norm(s, axis=1, keepdims=True)
    return s.astype(F32), rng.uniform(-0.5, 0.5, (n, 3)).astype(F32)


def lattice_reverse():
    """The 4 x 4 x 4 lattice of pitch 0.25 against its reverse shifted by 0.125: every coordinate is a dyadic fraction, many exact ties."""
    g = np.arange(4, dtype=F32) * F32(0.25) - F32(0.375)
    a = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3).astype(F32)
    return a, (a[::-1] + F32(0.125)).astype(F32)


def permuted_noise(n=192, seed=0):
    """A cloud of [-0.5, 0.5]^3 against a permuted copy with Gaussian noise of 0.01."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 0.5, (n, 3)).astype(F32)
    b = a[rng.permutation(n)] + rng.normal(0, 0.01, (n, 3)).astype(F32)
    return a, b.astype(F32)


def random_pair(n, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.5, 0.5, (n, 3)).astype(F32), rng.uniform(-0.5, 0.5, (n, 3)).astype(F32)
