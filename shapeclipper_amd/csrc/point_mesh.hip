// point_mesh.hip -- EXACT distance from points to a triangle mesh (ops.point_mesh_distance; the evaluation's --eval.mesh_dist).
// include/shapeclipper_hip.h states the arithmetic of one (point, triangle) pair one rounding at a time; tests/point_mesh_ref.py
// restates it in numpy.  Built without contraction.
//
// For every query the result is the candidate (d, f) that wins  d < best || (d == best && f < best_f)  over ALL valid triangles of the
// query's image: the lowest face index among the exact minima, whatever order the candidates are met in (a triangle may be met more than
// once: the rule is idempotent).  Two ways to get there, bit for bit the same:
//   * sc_point_mesh_distance_brute: all pairs.  A workgroup stages 256 triangles at a time in LDS (gathered through the face indices,
//     out-of-range faces flagged), every thread keeps its query and its best candidate in registers and reads the staged triangles at
//     wave-uniform addresses (LDS broadcasts).
//   * sc_point_mesh_distance: the triangle counterpart of chamfer_grid.hip.  The grid is built by triangle_grid.hpp (steps 0 to 5, shared
//     with mesh_intersect.hip): a uniform grid over the bounding box of the image's valid triangles; a triangle is referenced from every cell its AABB (padded by `slack`) overlaps: count pass, exclusive scan, fill pass
//     (integer atomics; the order inside a cell is arbitrary).  The cell side is max(2 x mean AABB extent, cbrt(volume / F)), grown
//     until the grid has at most 2 F + 64 cells, so a typical triangle overlaps at most 2 x 2 x 2 cells.  A triangle that overlaps more
//     than PM_CELL_CAP cells (one huge triangle across the box) goes on the image's "large" list instead, which every query of the image
//     tests first: the references never exceed PM_CELL_CAP x F whatever the mesh, so the workspace has a FIXED capacity and nothing is
//     read back to the host.  A query (one THREAD per query in this first version; the wave-per-tile walk of cg_query_wave_kernel is the
//     known next step) walks Chebyshev rings of cells around its own (clamped) cell.  After ring r every triangle not yet seen has no
//     point inside the (2r+1)^3 block of cells: a triangle with a point x inside the block is referenced from cell(x), because the
//     binning is monotone per axis.  So every point of it is at least `lb` away from the query, lb the distance to the nearest block
//     face that is not a face of the grid.  Every region of the pair arithmetic returns a point within a few ulp of the triangle (vertex
//     regions exactly, edge and interior regions with weights in [0, 1]; a triangle too thin for its interior weights to mean anything is
//     taken as its three edges), so its computed d is at least (lb - slack)^2 up to the rounding
//     of d: the walk stops when  best < (lb - slack)^2 * 0.9999  (slack = 16 ulp of the coordinate scale: Geometry.slack of
//     uniform_grid.hpp, where the box, the geometry and the cell of a coordinate live) or when the block covers the grid.  No unseen
//     triangle can beat or tie `best`.
//   * queries that do not stop within PM_RMAX rings or PM_BUDGET candidates, that start more than PM_REMPTY cells outside the box, and
//     every query of an image whose grid is invalid (a non-finite or huge vertex, a mesh of zero extent) go on a list and are answered by
//     the brute kernel's inner loop, split over PM_SLICES slices of the faces and merged with 64-bit atomicMin keys
//     (bits of d) << 32 | face  (d >= +0: the unsigned order is the numeric order, ties to the lower face); the closest point of the
//     winner is recomputed by the same pair arithmetic.
// Integer atomics only, plain stores, no cooperative launch: the same bits run to run, on any stream, whatever else is in the batch.
// Bound: latency / L2 gathers (one thread per query fetches every candidate through dependent 16-byte gathers).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "shapeclipper_hip.h"
#include "triangle_grid.hpp"

#pragma clang fp contract(off)

namespace sc_pm {

using namespace sc_tgrid;             // steps 0 to 5: the offsets, the box, the geometry, the references and the large lists (triangle_grid.hpp)
constexpr int PM_CELL_CAP = CELL_CAP; // cells a triangle may be referenced from; more: the image's large list
constexpr int PM_RMAX = 6;            // rings before a query is handed to the all-pairs scan
constexpr int PM_BUDGET = 4096;       // candidates before a query is handed to the scan
constexpr int PM_REMPTY = 2;          // cells outside the box / rings without a candidate before a query is handed to the scan
constexpr int PM_SLICES = 16;         // slices of the faces the scan of the listed queries is split over
constexpr long long MAX_QUERIES = 1ll << 30;
constexpr float PM_FLAT = 1.0e-5f;   // den = |ab|^2 |ac|^2 sin^2: below this sin^2 the interior weights are rounding noise, the triangle counts as its edges
constexpr float PM_HUGE = HUGE_COORD; // magnitudes the padding / slack arithmetic is not made for
constexpr unsigned long long EMPTY = ~0ull;

// ---- one (point, triangle) pair: include/shapeclipper_hip.h, "Arithmetic of one pair" ---------------------------------------------------
__device__ __forceinline__ float pm_dot(float x0, float x1, float x2, float y0, float y1, float y2) { return (x0 * y0 + x1 * y1) + x2 * y2; }

// clamped closest point of the segment a + t e, t in [0, 1]
__device__ __forceinline__ void pm_segment(const float p[3], const float a[3], const float e[3], float q[3], float& d) {
    const float l = pm_dot(e[0], e[1], e[2], e[0], e[1], e[2]);
    float t = pm_dot(p[0] - a[0], p[1] - a[1], p[2] - a[2], e[0], e[1], e[2]) / l;
    if (!(l > 0.f)) t = 0.f;
    if (!(t >= 0.f)) t = 0.f;
    if (t > 1.f) t = 1.f;
    for (int i = 0; i < 3; ++i) q[i] = a[i] + t * e[i];
    const float r0 = p[0] - q[0], r1 = p[1] - q[1], r2 = p[2] - q[2];
    d = pm_dot(r0, r1, r2, r0, r1, r2);
}

__device__ __forceinline__ void pm_pair(const float p[3], const float a[3], const float b[3], const float c[3], float q[3], float& d) {
    float ab[3], ac[3], bc[3], ap[3], bp[3], cp[3];
    for (int i = 0; i < 3; ++i) {
        ab[i] = b[i] - a[i]; ac[i] = c[i] - a[i]; bc[i] = c[i] - b[i];
        ap[i] = p[i] - a[i]; bp[i] = p[i] - b[i]; cp[i] = p[i] - c[i];
    }
    const float d1 = pm_dot(ab[0], ab[1], ab[2], ap[0], ap[1], ap[2]), d2 = pm_dot(ac[0], ac[1], ac[2], ap[0], ap[1], ap[2]);
    const float d3 = pm_dot(ab[0], ab[1], ab[2], bp[0], bp[1], bp[2]), d4 = pm_dot(ac[0], ac[1], ac[2], bp[0], bp[1], bp[2]);
    const float d5 = pm_dot(ab[0], ab[1], ab[2], cp[0], cp[1], cp[2]), d6 = pm_dot(ac[0], ac[1], ac[2], cp[0], cp[1], cp[2]);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e1 = d4 - d3, e2 = d5 - d6;
    const float nab = d1 - d3, nac = d2 - d6, nbc = e1 + e2;
    bool claimed = true;
    if (d1 <= 0.f && d2 <= 0.f) {                                               // vertex A
        for (int i = 0; i < 3; ++i) q[i] = a[i];
    } else if (d3 >= 0.f && d4 <= d3) {                                         // vertex B
        for (int i = 0; i < 3; ++i) q[i] = b[i];
    } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f && nab > 0.f) {              // edge AB
        const float v = d1 / nab;
        for (int i = 0; i < 3; ++i) q[i] = a[i] + v * ab[i];
    } else if (d6 >= 0.f && d5 <= d6) {                                         // vertex C
        for (int i = 0; i < 3; ++i) q[i] = c[i];
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f && nac > 0.f) {              // edge AC
        const float w = d2 / nac;
        for (int i = 0; i < 3; ++i) q[i] = a[i] + w * ac[i];
    } else if (va <= 0.f && e1 >= 0.f && e2 >= 0.f && nbc > 0.f) {              // edge BC
        const float w = e1 / nbc;
        for (int i = 0; i < 3; ++i) q[i] = b[i] + w * bc[i];
    } else {
        const float den = (va + vb) + vc;
        const float flat = PM_FLAT * (pm_dot(ab[0], ab[1], ab[2], ab[0], ab[1], ab[2]) * pm_dot(ac[0], ac[1], ac[2], ac[0], ac[1], ac[2]));
        if (den > 0.f && va >= 0.f && vb >= 0.f && vc >= 0.f && den > flat) {   // interior
            const float v = vb / den, w = vc / den;
            for (int i = 0; i < 3; ++i) q[i] = (a[i] + v * ab[i]) + w * ac[i];
        } else {
            claimed = false;
        }
    }
    if (claimed) {
        const float r0 = p[0] - q[0], r1 = p[1] - q[1], r2 = p[2] - q[2];
        d = pm_dot(r0, r1, r2, r0, r1, r2);
    } else {                                                                     // no region: first minimum over the segments AB, AC, BC
        pm_segment(p, a, ab, q, d);
        float q2[3], dd;
        pm_segment(p, a, ac, q2, dd);
        if (dd < d) { d = dd; for (int i = 0; i < 3; ++i) q[i] = q2[i]; }
        pm_segment(p, b, bc, q2, dd);
        if (dd < d) { d = dd; for (int i = 0; i < 3; ++i) q[i] = q2[i]; }
    }
}

struct Best {
    float d, q[3];
    int f;
};
__device__ __forceinline__ void pm_init(Best& s) { s.d = __builtin_inff(); s.f = INT_MAX; s.q[0] = s.q[1] = s.q[2] = 0.f; }
__device__ __forceinline__ void pm_test(Best& s, const float p[3], const float a[3], const float b[3], const float c[3], int f) {
    float q[3], d;
    pm_pair(p, a, b, c, q, d);
    if (d < s.d || (d == s.d && f < s.f)) { s.d = d; s.f = f; s.q[0] = q[0]; s.q[1] = q[1]; s.q[2] = q[2]; }
}
__device__ __forceinline__ bool pm_finite(const float p[3]) {
    return fabsf(p[0]) <= 3.4028234664e38f && fabsf(p[1]) <= 3.4028234664e38f && fabsf(p[2]) <= 3.4028234664e38f;
}
__device__ __forceinline__ void pm_write(const Best& s, bool finite_query, size_t at, float* __restrict__ dist2, int32_t* __restrict__ face,
                                         float* __restrict__ closest) {
    const float nan = __builtin_nanf("");
    if (!finite_query) {
        dist2[at] = nan; face[at] = -1;
        closest[at * 3 + 0] = nan; closest[at * 3 + 1] = nan; closest[at * 3 + 2] = nan;
    } else if (s.f == INT_MAX) {                        // no valid triangle (or none with a distance that compares)
        dist2[at] = __builtin_inff(); face[at] = -1;
        closest[at * 3 + 0] = 0.f; closest[at * 3 + 1] = 0.f; closest[at * 3 + 2] = 0.f;
    } else {
        dist2[at] = s.d; face[at] = s.f;
        closest[at * 3 + 0] = s.q[0]; closest[at * 3 + 1] = s.q[1]; closest[at * 3 + 2] = s.q[2];
    }
}

// ---- 6. the ring walk, one thread per query -----------------------------------------------------------------------------------------------
__device__ __forceinline__ void pm_test_packed(Best& s, const float p[3], const float4* __restrict__ tris, int f0, int local) {
    const float4 ta = tris[(size_t)(f0 + local) * 3 + 0], tb = tris[(size_t)(f0 + local) * 3 + 1], tc = tris[(size_t)(f0 + local) * 3 + 2];
    const float a[3] = {ta.x, ta.y, ta.z}, b[3] = {tb.x, tb.y, tb.z}, c[3] = {tc.x, tc.y, tc.z};
    pm_test(s, p, a, b, c, local);
}

__global__ __launch_bounds__(THREADS) void pm_query_kernel(int n, const float* __restrict__ pts, const Meta* __restrict__ meta,
                                                           const int* __restrict__ f_start, const int* __restrict__ start,
                                                           const int* __restrict__ refs, const float4* __restrict__ tris,
                                                           const int* __restrict__ large, const int* __restrict__ large_count,
                                                           float* __restrict__ dist2, int32_t* __restrict__ face, float* __restrict__ closest,
                                                           int* __restrict__ todo, int* __restrict__ todo_count,
                                                           unsigned long long* __restrict__ keys) {
    const int b = blockIdx.y, j = blockIdx.x * THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = j < n;
    const size_t at = (size_t)b * n + (in ? j : 0);
    const float q[3] = {pts[at * 3 + 0], pts[at * 3 + 1], pts[at * 3 + 2]};
    Best s;
    pm_init(s);
    const int f0 = f_start[b], nf = f_start[b + 1] - f0;
    const bool direct = !pm_finite(q) || nf == 0;      // answered without a search
    const Meta g = meta[b];
    bool done = false;
    if (in && !direct && g.valid && fabsf(q[0]) < PM_HUGE && fabsf(q[1]) < PM_HUGE && fabsf(q[2]) < PM_HUGE) {
        int c[3];
        bool outside = false;          // more than PM_REMPTY cells off the box: the walk could only confirm a candidate after many rings
        for (int a = 0; a < 3; ++a) {
            c[a] = sc_grid::axis_cell_far(q[a], g.lo[a], g.inv_h[a], g.g[a]);
            const float off = fmaxf(g.lo[a] - q[a], q[a] - (g.lo[a] + (float)g.g[a] * g.h[a]));
            outside |= off > (float)PM_REMPTY * g.h[a];
        }
        if (!outside) {
            const int nl = large_count[b];
            for (int k = 0; k < nl; ++k) pm_test_packed(s, q, tris, f0, large[f0 + k]);
        }
        int seen = 0;
        for (int r = 1; r <= PM_RMAX && !done && !outside && seen <= PM_BUDGET; ++r) {
            const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.g[2] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.g[1] - 1);
            const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.g[0] - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = g.cbase + (z * g.g[1] + y) * g.g[0];
                    // ring 1 takes the whole 3x3x3 block (ring 0 included); from ring 2 on only the shell
                    const bool full = r == 1 || z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r;
                    for (int side = 0; side < (full ? 1 : 2); ++side) {
                        int xa, xb;
                        if (full) { xa = x0; xb = x1; }
                        else {
                            xa = xb = side == 0 ? c[0] - r : c[0] + r;
                            if (xa < 0 || xa >= g.g[0]) continue;
                        }
                        const int sb = start[row + xa], se = start[row + xb + 1];      // a run of cells along x is one run of references
                        seen += se - sb;
                        for (int k = sb; k < se; ++k) pm_test_packed(s, q, tris, f0, refs[k]);
                    }
                }
            // every triangle not seen yet lies beyond a face of the block that is not a face of the grid
            float lb = __builtin_inff();
            for (int a = 0; a < 3; ++a) {
                if (c[a] - r > 0) lb = fminf(lb, q[a] - (g.lo[a] + (float)(c[a] - r) * g.h[a]));
                if (c[a] + r < g.g[a] - 1) lb = fminf(lb, (g.lo[a] + (float)(c[a] + r + 1) * g.h[a]) - q[a]);
            }
            const float safe = lb - g.slack;
            done = lb == __builtin_inff() ? true : (safe > 0.f && s.d < safe * safe * 0.9999f);
            if (r >= PM_REMPTY && s.f == INT_MAX) break;           // empty rings: the scan is the cheaper way
        }
    }
    if (in && (direct || done)) pm_write(s, pm_finite(q), at, dist2, face, closest);
    // the others go on the scan's list: one atomic per wave
    const bool listed = in && !direct && !done;
    const unsigned long long m = __ballot(listed);
    if (m) {
        const int leader = __builtin_ctzll(m);
        int base = 0;
        if (lane == leader) base = atomicAdd(&todo_count[b], __builtin_popcountll(m));
        base = __shfl(base, leader);
        if (listed) {
            const int pos = base + __builtin_popcountll(m & ((1ull << lane) - 1ull));
            todo[(size_t)b * n + pos] = j;
            keys[(size_t)b * n + pos] = EMPTY;          // the scan publishes (distance bits, face) with atomicMin
        }
    }
}

// ---- 7. all pairs.  LIST = false: every query of the image, results written directly.  LIST = true: the listed queries against slice
// blockIdx.z of the faces, winners published as keys. -------------------------------------------------------------------------------------
template <bool LIST>
__global__ __launch_bounds__(THREADS) void pm_brute_kernel(int n, const float* __restrict__ pts, const float* __restrict__ verts,
                                                           const int32_t* __restrict__ faces, const int* __restrict__ v_start,
                                                           const int* __restrict__ f_start, const int* __restrict__ todo,
                                                           const int* __restrict__ todo_count, unsigned long long* __restrict__ keys,
                                                           float* __restrict__ dist2, int32_t* __restrict__ face,
                                                           float* __restrict__ closest) {
    __shared__ float tri[THREADS][9];
    __shared__ int tri_ok[THREADS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int cnt = LIST ? todo_count[b] : n;
    if ((int)blockIdx.x * THREADS >= cnt) return;                   // uniform for the workgroup
    const int e = blockIdx.x * THREADS + tid;
    const bool live = e < cnt;
    const int j = LIST ? todo[(size_t)b * n + (live ? e : cnt - 1)] : (live ? e : cnt - 1);
    const size_t at = (size_t)b * n + j;
    const float q[3] = {pts[at * 3 + 0], pts[at * 3 + 1], pts[at * 3 + 2]};
    const int f0 = f_start[b], nf = f_start[b + 1] - f0;
    int begin = 0, end = nf;
    if (LIST) {
        const int per = ((nf + PM_SLICES - 1) / PM_SLICES + THREADS - 1) / THREADS * THREADS;
        begin = (int)blockIdx.z * per;
        end = min(nf, begin + per);
        if (begin >= end) return;                                   // uniform
    }
    Best s;
    pm_init(s);
    for (int k0 = begin; k0 < end; k0 += THREADS) {
        const int chunk = min(THREADS, end - k0);
        __syncthreads();
        if (tid < chunk) {
            float a[3], bb[3], c[3];
            const bool ok = load_face(f0 + k0 + tid, b, verts, faces, v_start, a, bb, c);
            tri_ok[tid] = ok ? 1 : 0;
            if (ok)
                for (int i = 0; i < 3; ++i) { tri[tid][i] = a[i]; tri[tid][3 + i] = bb[i]; tri[tid][6 + i] = c[i]; }
        }
        __syncthreads();
        for (int t = 0; t < chunk; ++t) {
            if (!tri_ok[t]) continue;                               // uniform: every thread reads the same staged triangle
            const float a[3] = {tri[t][0], tri[t][1], tri[t][2]}, bb[3] = {tri[t][3], tri[t][4], tri[t][5]};
            const float c[3] = {tri[t][6], tri[t][7], tri[t][8]};
            pm_test(s, q, a, bb, c, k0 + t);
        }
    }
    if (!live) return;
    if (LIST) {
        if (s.f != INT_MAX)
            atomicMin(&keys[(size_t)b * n + e], ((unsigned long long)__float_as_uint(s.d) << 32) | (unsigned int)s.f);
    } else {
        pm_write(s, pm_finite(q), at, dist2, face, closest);
    }
}

__global__ __launch_bounds__(THREADS) void pm_unpack_kernel(int n, const float* __restrict__ pts, const float* __restrict__ verts,
                                                            const int32_t* __restrict__ faces, const int* __restrict__ v_start,
                                                            const int* __restrict__ f_start, const int* __restrict__ todo,
                                                            const int* __restrict__ todo_count, const unsigned long long* __restrict__ keys,
                                                            float* __restrict__ dist2, int32_t* __restrict__ face,
                                                            float* __restrict__ closest) {
    const int b = blockIdx.y, cnt = todo_count[b];
    const int e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= cnt) return;
    const unsigned long long key = keys[(size_t)b * n + e];
    const int j = todo[(size_t)b * n + e];
    const size_t at = (size_t)b * n + j;
    const float q[3] = {pts[at * 3 + 0], pts[at * 3 + 1], pts[at * 3 + 2]};
    Best s;
    pm_init(s);
    if (key != EMPTY) {                                             // the winner's closest point: the same pair, the same bits
        const int f = (int)(unsigned int)(key & 0xFFFFFFFFull);
        float a[3], bb[3], c[3];
        if (load_face(f_start[b] + f, b, verts, faces, v_start, a, bb, c)) pm_test(s, q, a, bb, c, f);
    }
    pm_write(s, true, at, dist2, face, closest);                    // non-finite queries never reach the list
}

// workspace, in 4-byte words: the grid's regions (triangle_grid.hpp) and the scan's list
struct Workspace : sc_tgrid::Carve {
    size_t todo_count, cleared;         // cleared by one memset: todo_count and the grid's cleared regions, first and adjacent
    size_t todo, keys, total;
};
inline Workspace carve(int b, int n, int f_total) {
    Workspace c;
    sc_grid::WordCarver w;
    c.todo_count = w.take((size_t)b);
    carve_cleared(w, b, f_total, c);
    c.cleared = w.words;
    carve_rest(w, b, f_total, c);
    c.todo = w.take((size_t)b * n);
    c.keys = w.take((size_t)b * n * 2);                               // 64-bit: offsets are multiples of 4 words
    c.total = w.words;
    return c;
}

inline bool refused(int b, int n, int v_total, int f_total) {
    return b > MAX_IMAGES || n < 1 || v_total < 0 || f_total < 0 || f_total > MAX_FACES || (long long)b * n > MAX_QUERIES;
}

}  // namespace sc_pm

extern "C" {

// See include/shapeclipper_hip.h for the contract.
long long sc_point_mesh_workspace_bytes(int n_images, int n_points, int v_total, int f_total) {
    if (n_images <= 0) return 0;
    if (sc_pm::refused(n_images, n_points, v_total, f_total)) return -1;
    return (long long)(sc_pm::carve(n_images, n_points, f_total).total * sizeof(int));
}

int sc_point_mesh_distance_brute(const float* points, const float* verts, const int32_t* faces, const int32_t* v_count,
                                 const int32_t* f_count, int n_images, int n_points, int v_total, int f_total, void* workspace,
                                 float* dist2, int32_t* face, float* closest, void* stream_) {
    using namespace sc_pm;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images <= 0) return 0;
    if (refused(n_images, n_points, v_total, f_total) || !points || !v_count || !f_count || !workspace || !dist2 || !face || !closest ||
        (v_total > 0 && !verts) || (f_total > 0 && !faces) || ((uintptr_t)workspace & 15))
        return (int)hipErrorInvalidValue;
    const Workspace c = carve(n_images, n_points, f_total);
    int* ws = (int*)workspace;
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, stream, n_images, v_count, f_count, v_total, f_total, ws + c.v_start,
                       ws + c.f_start);
    hipLaunchKernelGGL(pm_brute_kernel<false>, dim3((n_points + THREADS - 1) / THREADS, n_images), dim3(THREADS), 0, stream, n_points, points,
                       verts, faces, ws + c.v_start, ws + c.f_start, (const int*)nullptr, (const int*)nullptr,
                       (unsigned long long*)nullptr, dist2, face, closest);
    return (int)hipGetLastError();
}

int sc_point_mesh_distance(const float* points, const float* verts, const int32_t* faces, const int32_t* v_count, const int32_t* f_count,
                           int n_images, int n_points, int v_total, int f_total, void* workspace, float* dist2, int32_t* face,
                           float* closest, void* stream_) {
    using namespace sc_pm;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images <= 0) return 0;
    if (f_total <= 0 || refused(n_images, n_points, v_total, f_total) || !points || !verts || !faces || !v_count || !f_count || !workspace ||
        !dist2 || !face || !closest || ((uintptr_t)workspace & 15))           // no face at all: the twin writes the empty result
        return sc_point_mesh_distance_brute(points, verts, faces, v_count, f_count, n_images, n_points, v_total, f_total, workspace, dist2,
                                            face, closest, stream_);
    const Workspace c = carve(n_images, n_points, f_total);
    int* ws = (int*)workspace;
    int *v_start = ws + c.v_start, *f_start = ws + c.f_start;
    unsigned long long* keys = (unsigned long long*)(ws + c.keys);
    Meta* meta = (Meta*)(ws + c.meta);
    float4* tris = (float4*)(ws + c.tris);
    const int query_blocks = (n_points + THREADS - 1) / THREADS;
    (void)hipMemsetAsync(ws, 0, c.cleared * sizeof(int), stream);
    build(ws, c, verts, faces, v_count, f_count, n_images, v_total, f_total, stream);
    hipLaunchKernelGGL(pm_query_kernel, dim3(query_blocks, n_images), dim3(THREADS), 0, stream, n_points, points, meta, f_start,
                       ws + c.counts, ws + c.refs, tris, ws + c.large, ws + c.large_count, dist2, face, closest, ws + c.todo,
                       ws + c.todo_count, keys);
    hipLaunchKernelGGL(pm_brute_kernel<true>, dim3(query_blocks, n_images, PM_SLICES), dim3(THREADS), 0, stream, n_points, points, verts,
                       faces, v_start, f_start, ws + c.todo, ws + c.todo_count, keys, dist2, face, closest);
    hipLaunchKernelGGL(pm_unpack_kernel, dim3(query_blocks, n_images), dim3(THREADS), 0, stream, n_points, points, verts, faces, v_start,
                       f_start, ws + c.todo, ws + c.todo_count, keys, dist2, face, closest);
    return (int)hipGetLastError();
}

}  // extern "C"
