// point_normals.hip -- k nearest neighbours inside one cloud, PCA normals from them, and the normal consistency of two clouds
// (ops.knn_points / point_normals / normal_consistency; the evaluation's --eval.normals).  include/shapeclipper_hip.h states the
// arithmetic one rounding at a time; tests/point_normals_ref.py restates it in numpy.  Built without contraction.
//
// sc_knn_points is EXACT: for every point the k smallest keys (float bits of d) << 32 | index over its own cloud, ascending, with
// d = (dx*dx + dy*dy) + dz*dz in fp32.  The key order is total, so the result does not depend on the order candidates are met in.
//   * the cloud is binned into a uniform grid of its own (uniform_grid.hpp: bounding box by integer atomicMax on order-preserving keys,
//     histogram and cursors by integer atomicAdd; the order inside a cell is arbitrary) and copied into cell order as
//     {x, y, z, original index};
//   * the queries ARE that sorted array: thread t of the walk answers sorted point t, so the lanes of a wave sit in the same or
//     neighbouring cells and walk the same rows of cells;
//   * a thread keeps its k keys ascending in LDS, laid out [k][thread]: slot i of lane l is at ((i * KNN_THREADS) + l) * 8 bytes, so a wave's
//     ds_read_b64 / ds_write_b64 of one slot touches 64 consecutive 8-byte words (conflict-free), and the list costs no registers for any
//     k in 3..32 (a register list for a runtime k would be indexed dynamically and go to scratch).  k = 32 takes 32 KiB per workgroup of
//     128 threads, k = 16 16 KiB: 5 to 10 workgroups fit a CU's 160 KiB, more than the walk's ~40 VGPRs need to hide the gathers;
//   * after Chebyshev ring r every point not yet seen lies outside the (2r+1)^3 block of cells, at least `lb` away along one axis (faces
//     on the grid boundary bound nothing).  The walk stops when the list is full and  kth d < (lb - slack)^2 * 0.9999:  slack (16 ulp of
//     the cloud's coordinate scale) covers the rounding of the binning and of the face coordinates, the factor the rounding of d (three
//     products and two sums, < 4 ulp), so an unseen point can neither beat nor tie the k-th key -- chamfer_grid.hip's argument, for
//     the k-th instead of the first;
//   * queries that do not stop within KNN_RMAX rings or KNN_BUDGET candidates (a sparse neighbourhood, one huge cell) and every query
//     of an image whose grid is invalid (a non-finite or huge coordinate, a single point position) go on a list; knn_scan_kernel
//     answers them from scratch by going through ALL points with the same key and the same list.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "block_scan.hpp"
#include "shapeclipper_hip.h"
#include "uniform_grid.hpp"

namespace sc_pn {

constexpr int KNN_THREADS = 128;
constexpr int KNN_TPC = 2;            // aimed-at points per cell (of the bounding box's volume)
constexpr int KNN_GMAX = 128;         // cells per axis
constexpr int KNN_RMAX = 4;           // rings before a query is handed to the scan
constexpr int KNN_BUDGET = 4096;      // candidates before a query is handed to the scan
constexpr int KNN_TILE = 256;         // points staged per round of the scan
constexpr int K_MIN = 3, K_MAX = 32;
constexpr int MAX_IMAGES = 65535;
constexpr int SCAN_THREADS = 1024;
constexpr int JACOBI_SWEEPS = 8;
constexpr int THREADS = 256, WAVES = THREADS / 64, PER_THREAD = 4, CHUNK = THREADS * PER_THREAD;
constexpr unsigned long long EMPTY = ~0ull;

static_assert(CHUNK == SC_ICP_CHUNK, "sc_normal_consistency sums in the chunks the header states for sc_icp_objective");

using GridMeta = sc_grid::Geometry;    // one per image
constexpr int META_WORDS = sizeof(GridMeta) / 4;

__host__ __device__ inline int cells_capacity(int n) { return n / KNN_TPC * 2 + 64; }

// ---- 1, 2, 4. bounding box -> grid geometry; cell of every point + histogram; points into cell order as {x, y, z, original index}:
// uniform_grid.hpp.  One thread per image turns the box into the geometry with this file's constants.
using sc_grid::axis_cell;

__global__ void knn_meta_kernel(int n, int n_images, int force_scan, const unsigned* __restrict__ box_all, GridMeta* __restrict__ meta) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_images) return;
    GridMeta g;
    const float h = sc_grid::geometry_from_box(box_all + (size_t)b * sc_grid::BOX_WORDS, cells_capacity(n), KNN_GMAX, 8,
                                               [=](float vol, float) { return cbrtf(vol * (float)KNN_TPC / (float)n); }, g);
    g.valid = (g.valid && !force_scan && h > 0.f) ? 1 : 0;
    if (!g.valid) {
        g.g[0] = g.g[1] = g.g[2] = 1;
        for (int a = 0; a < 3; ++a) { g.lo[a] = 0.f; g.h[a] = 1.f; g.inv_h[a] = 1.f; }
        g.slack = 0.f;
    }
    meta[b] = g;
}

// ---- 3. exclusive scan of the histogram in place over [0, cells] inclusive (the last entry receives the total) ---------------------
// One workgroup per image: thread t owns a run of consecutive entries, the 1,024 run totals are scanned through LDS.
__global__ __launch_bounds__(SCAN_THREADS) void knn_scan_cells_kernel(const GridMeta* __restrict__ meta, int cap, int* __restrict__ counts) {
    __shared__ int wtot[SCAN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GridMeta& g = meta[b];
    const int entries = g.g[0] * g.g[1] * g.g[2] + 1;
    int* c = counts + (size_t)b * (cap + 1);
    const int per = (entries + SCAN_THREADS - 1) / SCAN_THREADS;
    const int first = tid * per, last = min(first + per, entries);
    int sum = 0;
    for (int i = first; i < last; ++i) sum += c[i];
    const int incl = sc_scan::wave_inclusive(sum);         // the run totals: wave scan, then the totals of the waves in front (no block total needed)
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < wave; ++w) run += wtot[w];
    for (int i = first; i < last; ++i) { const int v = c[i]; c[i] = run; run += v; }
}

// ---- the k-entry list of one thread: keys ascending, slot i at list[i * KNN_THREADS] -----------------------------------------------
__device__ __forceinline__ float dist2(float px, float py, float pz, float qx, float qy, float qz) {
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    return (dx * dx + dy * dy) + dz * dz;           // the file is built with -ffp-contract=off: five roundings
}
__device__ __forceinline__ unsigned long long make_key(float d, int index) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned int)index;
}
// key < the list's last entry: shift the larger entries up one slot and put key in its place; returns the new last entry
__device__ __forceinline__ unsigned long long list_insert(unsigned long long* list, int k, unsigned long long key) {
    int j = k - 1;
    while (j > 0) {
        const unsigned long long prev = list[(j - 1) * KNN_THREADS];
        if (prev < key) break;
        list[j * KNN_THREADS] = prev;
        --j;
    }
    list[j * KNN_THREADS] = key;
    return list[(k - 1) * KNN_THREADS];
}
__device__ __forceinline__ void list_write(const unsigned long long* list, int k, int* __restrict__ idx, float* __restrict__ dist) {
    for (int i = 0; i < k; ++i) {
        const unsigned long long key = list[i * KNN_THREADS];
        idx[i] = (int)(unsigned int)(key & 0xFFFFFFFFull);
        dist[i] = __uint_as_float((unsigned int)(key >> 32));
    }
}

// ---- 5. the ring walk: thread t answers sorted point t ---------------------------------------------------------------------------
__global__ __launch_bounds__(KNN_THREADS) void knn_walk_kernel(int n, int k, const GridMeta* __restrict__ meta, int cap,
                                                               const int* __restrict__ start_all, const float4* __restrict__ sorted_all,
                                                               int* __restrict__ idx, float* __restrict__ dist, int* __restrict__ todo,
                                                               int* __restrict__ todo_count) {
    extern __shared__ unsigned long long lists[];                   // [k][KNN_THREADS]
    const int b = blockIdx.y, t = blockIdx.x * KNN_THREADS + threadIdx.x;
    if (t >= n) return;
    const GridMeta g = meta[b];
    const int* start = start_all + (size_t)b * (cap + 1);
    const float4* sorted = sorted_all + (size_t)b * n;
    const float4 qv = sorted[t];
    const float q[3] = {qv.x, qv.y, qv.z};
    const int j = __float_as_int(qv.w);
    unsigned long long* list = lists + threadIdx.x;
    bool done = false;
    if (g.valid) {
        for (int i = 0; i < k; ++i) list[i * KNN_THREADS] = EMPTY;
        unsigned long long worst = EMPTY;
        int c[3];
        for (int a = 0; a < 3; ++a) c[a] = axis_cell(q[a], g.lo[a], g.inv_h[a], g.g[a]);
        int seen = 0;
        for (int r = 1; r <= KNN_RMAX && !done && seen <= KNN_BUDGET; ++r) {
            const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g.g[2] - 1), y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g.g[1] - 1);
            const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g.g[0] - 1);
            for (int z = z0; z <= z1 && seen <= KNN_BUDGET; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * g.g[1] + y) * g.g[0];
                    // ring 1 takes the whole 3x3x3 block (the query's own cell included); from ring 2 on only the shell
                    const bool full = r == 1 || z == c[2] - r || z == c[2] + r || y == c[1] - r || y == c[1] + r;
                    for (int side = 0; side < (full ? 1 : 2); ++side) {
                        int xa, xb;
                        if (full) { xa = x0; xb = x1; }
                        else {
                            xa = xb = side == 0 ? c[0] - r : c[0] + r;
                            if (xa < 0 || xa >= g.g[0]) continue;
                        }
                        const int s = start[row + xa], e = start[row + xb + 1];
                        seen += e - s;
                        for (int p = s; p < e; ++p) {
                            const float4 v = sorted[p];
                            const unsigned long long key = make_key(dist2(v.x, v.y, v.z, q[0], q[1], q[2]), __float_as_int(v.w));
                            if (key < worst) worst = list_insert(list, k, key);
                        }
                    }
                }
            if (seen > KNN_BUDGET) break;           // the ring may be incomplete: no bound holds, the scan answers
            // everything not seen yet lies beyond a face of the block that is not a face of the grid
            float lb = __builtin_inff();
            for (int a = 0; a < 3; ++a) {
                if (c[a] - r > 0) lb = fminf(lb, q[a] - (g.lo[a] + (float)(c[a] - r) * g.h[a]));
                if (c[a] + r < g.g[a] - 1) lb = fminf(lb, (g.lo[a] + (float)(c[a] + r + 1) * g.h[a]) - q[a]);
            }
            const float safe = lb - g.slack;
            const float kth = __uint_as_float((unsigned int)(worst >> 32));
            done = worst != EMPTY && (lb == __builtin_inff() || (safe > 0.f && kth < safe * safe * 0.9999f));
        }
    }
    if (done) {
        list_write(list, k, idx + ((size_t)b * n + j) * k, dist + ((size_t)b * n + j) * k);
    } else {
        const int pos = atomicAdd(&todo_count[b], 1);
        todo[(size_t)b * n + pos] = j;
    }
}

// ---- 6. the exact scan of the listed queries over all points, in index order -------------------------------------------------------
__global__ __launch_bounds__(KNN_THREADS) void knn_scan_kernel(int n, int k, const float* __restrict__ pts_all, const int* __restrict__ todo,
                                                               const int* __restrict__ todo_count, int* __restrict__ idx,
                                                               float* __restrict__ dist) {
    extern __shared__ unsigned long long lists[];                   // [k][KNN_THREADS], then KNN_TILE staged points {x, y, z, -}
    const int b = blockIdx.y, cnt = todo_count[b];
    if ((int)blockIdx.x * KNN_THREADS >= cnt) return;               // uniform over the workgroup
    float4* tile = reinterpret_cast<float4*>(lists + (size_t)k * KNN_THREADS);        // 16-byte aligned: k * 1024 bytes in
    const float* pts = pts_all + (size_t)b * n * 3;
    const int e = blockIdx.x * KNN_THREADS + threadIdx.x;
    const bool live = e < cnt;
    const int j = todo[(size_t)b * n + (live ? e : cnt - 1)];
    const float q[3] = {pts[(size_t)j * 3 + 0], pts[(size_t)j * 3 + 1], pts[(size_t)j * 3 + 2]};
    unsigned long long* list = lists + threadIdx.x;
    for (int i = 0; i < k; ++i) list[i * KNN_THREADS] = EMPTY;
    unsigned long long worst = EMPTY;
    for (int base = 0; base < n; base += KNN_TILE) {
        const int cnt_t = min(KNN_TILE, n - base);
        __syncthreads();
        for (int w = threadIdx.x; w < cnt_t; w += KNN_THREADS) {
            const float* v = pts + (size_t)(base + w) * 3;
            tile[w] = make_float4(v[0], v[1], v[2], 0.f);
        }
        __syncthreads();
        if (live) {
            for (int p = 0; p < cnt_t; ++p) {
                const float4 v = tile[p];                           // a wave-uniform address: one broadcast ds_read_b128
                const unsigned long long key = make_key(dist2(v.x, v.y, v.z, q[0], q[1], q[2]), base + p);
                if (key < worst) worst = list_insert(list, k, key);
            }
        }
    }
    if (live) list_write(list, k, idx + ((size_t)b * n + j) * k, dist + ((size_t)b * n + j) * k);
}

struct Carve { size_t box, counts, cursor, todo_count, zeroed, meta, cell_of, todo, sorted, total; };   // in 4-byte words
inline Carve carve(int b, int n) {
    Carve c;
    const size_t cap = (size_t)cells_capacity(n);
    sc_grid::WordCarver w;
    c.box = w.take((size_t)b * sc_grid::BOX_WORDS);                 // the first four are cleared by one memset
    c.counts = w.take((size_t)b * (cap + 1));
    c.cursor = w.take((size_t)b * cap);
    c.todo_count = w.take((size_t)b);
    c.zeroed = w.words;
    c.meta = w.take((size_t)b * META_WORDS);
    c.cell_of = w.take((size_t)b * n);
    c.todo = w.take((size_t)b * n);
    c.sorted = w.take((size_t)b * n * 4);            // float4: offsets are multiples of 4 words
    c.total = w.words;
    return c;
}

__host__ inline bool knn_sizes_ok(int n_images, int n, int k) { return n_images <= MAX_IMAGES && k >= K_MIN && k <= K_MAX && n >= k; }

// ---- PCA normals ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // false for NaN and Inf

// One two-sided Jacobi rotation on the symmetric A = [a00 a01 a02; . a11 a12; . . a22] for the pair (p, q), r the third index:
// app, aqq, apq the pair's entries, arp, arq the third row's; vp, vq the columns p and q of V.
__device__ __forceinline__ void jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double vp[3], double vq[3]) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    double t;
    if (fabs(theta) > 1.0e150) t = 0.5 / theta;            // theta * theta would overflow; the limit of the formula below
    else t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double np = c * arp - s * arq, nq = s * arp + c * arq;
    arp = np; arq = nq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = c * vp[i] - s * vq[i], bq = s * vp[i] + c * vq[i];
        vp[i] = a; vq[i] = bq;
    }
}

__global__ __launch_bounds__(256) void normals_kernel(int n, int k, const float* __restrict__ pts_all, const int* __restrict__ idx_all,
                                                      float* __restrict__ normals, float* __restrict__ variation) {
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* pts = pts_all + (size_t)b * n * 3;
    const int* idx = idx_all + ((size_t)b * n + i) * k;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double m[3] = {0.0, 0.0, 0.0};
    for (int r = 0; r < k; ++r) {
        const int j = idx[r];
        const bool in = (unsigned int)j < (unsigned int)n;          // an index outside the cloud: NaN, not a read out of bounds
#pragma unroll
        for (int a = 0; a < 3; ++a) m[a] = m[a] + (in ? (double)pts[(size_t)j * 3 + a] : nan);
    }
    const double kk = (double)k;
#pragma unroll
    for (int a = 0; a < 3; ++a) m[a] = m[a] / kk;
    double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
    for (int r = 0; r < k; ++r) {
        const int j = idx[r];
        const bool in = (unsigned int)j < (unsigned int)n;
        double d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = (in ? (double)pts[(size_t)j * 3 + a] : nan) - m[a];
        a00 = a00 + d[0] * d[0]; a01 = a01 + d[0] * d[1]; a02 = a02 + d[0] * d[2];
        a11 = a11 + d[1] * d[1]; a12 = a12 + d[1] * d[2]; a22 = a22 + d[2] * d[2];
    }
    a00 = a00 / kk; a01 = a01 / kk; a02 = a02 / kk; a11 = a11 / kk; a12 = a12 / kk; a22 = a22 / kk;
    bool ok = finite(m[0]) && finite(m[1]) && finite(m[2]) && finite(a00) && finite(a01) && finite(a02) && finite(a11) && finite(a12) && finite(a22);
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    if (ok) {
        for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
            jacobi_rotate(a00, a11, a01, a02, a12, v0, v1);         // (0, 1), third index 2
            jacobi_rotate(a00, a22, a02, a01, a12, v0, v2);         // (0, 2), third index 1
            jacobi_rotate(a11, a22, a12, a01, a02, v1, v2);         // (1, 2), third index 0
        }
    }
    // ascending eigenvalues; equal values keep their index order
    double l[3] = {a00, a11, a22};
    int o0 = 0, o1 = 1, o2 = 2;
    if (l[o1] < l[o0]) { const int s = o0; o0 = o1; o1 = s; }
    if (l[o2] < l[o1]) { const int s = o1; o1 = o2; o2 = s; }
    if (l[o1] < l[o0]) { const int s = o0; o0 = o1; o1 = s; }
    const double l0 = l[o0], l1 = l[o1], l2 = l[o2];
    ok = ok && finite(l0) && finite(l1) && finite(l2) && !(l1 <= 1.0e-12 * l2);
    float out[3] = {0.f, 0.f, 0.f}, var = 0.f;
    if (ok) {
        const double* v = o0 == 0 ? v0 : (o0 == 1 ? v1 : v2);
        double e[3] = {v[0], v[1], v[2]};
        int big = 0;
        if (fabs(e[1]) > fabs(e[big])) big = 1;
        if (fabs(e[2]) > fabs(e[big])) big = 2;
        const double sign = e[big] < 0.0 ? -1.0 : 1.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) out[a] = (float)(sign * e[a]);
        var = (float)(l0 / ((l0 + l1) + l2));
    }
    float* o = normals + ((size_t)b * n + i) * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    variation[(size_t)b * n + i] = var;
}

// ---- normal consistency: sc_icp_objective's three-stage sums of |n . n'| -----------------------------------------------------------
__host__ __device__ __forceinline__ int chunks_of(int n) { return (n + CHUNK - 1) / CHUNK; }

// grid (c1 + c2, n_images): half 0 sums |n1[i] . n2[idx1[i]]| over one chunk of i, half 1 |n2[j] . n1[idx2[j]]| -> ws[image][chunk]
__global__ void __launch_bounds__(THREADS) consistency_partial_kernel(const float* __restrict__ n1, const float* __restrict__ n2,
                                                                      const int* __restrict__ idx1, const int* __restrict__ idx2, int n, int m,
                                                                      double* __restrict__ ws) {
    __shared__ double lds[WAVES];
    const int c1 = chunks_of(n), c2 = chunks_of(m), b = blockIdx.y;
    const int chunk = blockIdx.x, half = chunk < c1 ? 0 : 1;
    const int first = (half == 0 ? chunk : chunk - c1) * CHUNK, count = half == 0 ? n : m, other = half == 0 ? m : n;
    const float* own = half == 0 ? n1 + (size_t)b * n * 3 : n2 + (size_t)b * m * 3;
    const float* oth = half == 0 ? n2 + (size_t)b * m * 3 : n1 + (size_t)b * n * 3;
    const int* idx = half == 0 ? idx1 + (size_t)b * n : idx2 + (size_t)b * m;
    double v = 0.0;
#pragma unroll
    for (int r = 0; r < PER_THREAD; ++r) {
        const int i = first + r * THREADS + (int)threadIdx.x;
        if (i < count) {
            const int j = idx[i];
            double term = __longlong_as_double(0x7ff8000000000000LL);
            if ((unsigned int)j < (unsigned int)other) {
                const double x = (double)own[(size_t)i * 3], y = (double)own[(size_t)i * 3 + 1], z = (double)own[(size_t)i * 3 + 2];
                const double xo = (double)oth[(size_t)j * 3], yo = (double)oth[(size_t)j * 3 + 1], zo = (double)oth[(size_t)j * 3 + 2];
                term = fabs((x * xo + y * yo) + z * zo);
            }
            v += term;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) ws[(size_t)b * (c1 + c2) + chunk] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// grid n_images, one lane each: the chunk partials of a half in ascending chunk number, divided by the half's count
__global__ void __launch_bounds__(64) consistency_finish_kernel(const double* __restrict__ ws, int n, int m, double* __restrict__ acc,
                                                                double* __restrict__ comp) {
    if (threadIdx.x != 0) return;
    const int c1 = chunks_of(n), c2 = chunks_of(m), b = blockIdx.x;
    const double* rows = ws + (size_t)b * (c1 + c2);
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < c1; ++c) s1 += rows[c];
    for (int c = c1; c < c1 + c2; ++c) s2 += rows[c];
    acc[b] = s1 / (double)n;
    comp[b] = s2 / (double)m;
}

}  // namespace sc_pn

extern "C" long long sc_knn_workspace_bytes(int n_images, int n, int k) {
    using namespace sc_pn;
    if (n_images <= 0) return 0;
    if (!knn_sizes_ok(n_images, n, k)) return -1;
    return (long long)(carve(n_images, n).total * sizeof(int));
}

extern "C" int sc_knn_points(const float* points, int n_images, int n, int k, void* workspace, int* idx, float* dist, void* stream) {
    using namespace sc_pn;
    if (n_images <= 0) return 0;
    if (!knn_sizes_ok(n_images, n, k) || !points || !workspace || !idx || !dist) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const int b = n_images, cap = cells_capacity(n);
    const Carve c = carve(b, n);
    int* ws = (int*)workspace;
    GridMeta* meta = reinterpret_cast<GridMeta*>(ws + c.meta);
    float4* sorted = reinterpret_cast<float4*>(ws + c.sorted);
    static const int force_scan = [] { const char* e = getenv("SC_KNN_FORCE_SCAN"); return e ? atoi(e) : 0; }();      // timing: every query by the scan
    (void)hipMemsetAsync(ws, 0, c.zeroed * sizeof(int), s);
    const int bbox_blocks = (n + 256 * 8 - 1) / (256 * 8);
    const dim3 per_point((unsigned)((n + 255) / 256), (unsigned)b);
    hipLaunchKernelGGL(sc_grid::bbox_kernel, dim3(bbox_blocks < 64 ? bbox_blocks : 64, b), dim3(256), 0, s, n, points, reinterpret_cast<unsigned*>(ws + c.box));
    hipLaunchKernelGGL(knn_meta_kernel, dim3((b + 63) / 64), dim3(64), 0, s, n, b, force_scan, reinterpret_cast<const unsigned*>(ws + c.box), meta);
    hipLaunchKernelGGL((sc_grid::count_kernel<false, GridMeta>), per_point, dim3(256), 0, s, n, points, meta, cap, ws + c.cell_of, ws + c.counts);
    hipLaunchKernelGGL(knn_scan_cells_kernel, dim3(b), dim3(SCAN_THREADS), 0, s, meta, cap, ws + c.counts);
    hipLaunchKernelGGL((sc_grid::scatter_kernel<false, GridMeta>), per_point, dim3(256), 0, s, n, points, cap, ws + c.cell_of, ws + c.counts,
                       ws + c.cursor, sorted, meta);
    const dim3 per_query((unsigned)((n + KNN_THREADS - 1) / KNN_THREADS), (unsigned)b);
    const size_t list_bytes = (size_t)k * KNN_THREADS * sizeof(unsigned long long);
    hipLaunchKernelGGL(knn_walk_kernel, per_query, dim3(KNN_THREADS), list_bytes, s, n, k, meta, cap, ws + c.counts, sorted, idx, dist,
                       ws + c.todo, ws + c.todo_count);
    // as many workgroups as the longest possible list needs; those past the actual list exit at once
    hipLaunchKernelGGL(knn_scan_kernel, per_query, dim3(KNN_THREADS), list_bytes + KNN_TILE * sizeof(float4), s, n, k, points, ws + c.todo,
                       ws + c.todo_count, idx, dist);
    return (int)hipGetLastError();
}

extern "C" int sc_point_normals(const float* points, const int* idx, int n_images, int n, int k, float* normals, float* variation,
                                void* stream) {
    using namespace sc_pn;
    if (n_images <= 0) return 0;
    if (!knn_sizes_ok(n_images, n, k) || !points || !idx || !normals || !variation) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(normals_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_images), dim3(256), 0, (hipStream_t)stream, n, k, points,
                       idx, normals, variation);
    return (int)hipGetLastError();
}

extern "C" int sc_normal_consistency(const float* n1, const float* n2, const int* idx1, const int* idx2, int n_images, int n, int m,
                                     double* workspace, double* acc, double* comp, void* stream) {
    using namespace sc_pn;
    if (n_images <= 0) return 0;
    if (n_images > MAX_IMAGES || n < 1 || m < 1 || !n1 || !n2 || !idx1 || !idx2 || !workspace || !acc || !comp) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned int)(chunks_of(n) + chunks_of(m)), (unsigned int)n_images);
    hipLaunchKernelGGL(consistency_partial_kernel, grid, dim3(THREADS), 0, s, n1, n2, idx1, idx2, n, m, workspace);
    hipLaunchKernelGGL(consistency_finish_kernel, dim3((unsigned int)n_images), dim3(64), 0, s, (const double*)workspace, n, m, acc, comp);
    return (int)hipGetLastError();
}
