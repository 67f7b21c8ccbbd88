// mesh_smooth.hip -- Taubin lambda|mu smoothing of a batch of indexed triangle meshes by the umbrella operator (ops.mesh_smooth, the
// evaluation's {idx}_mesh_smooth.ply; definition in include/shapeclipper_hip.h, sc_mesh_smooth; restated in numpy by
// tests/mesh_smooth_ref.py).  Built without contraction: every float64 operation of a half-step and of the measures rounds once.
//
// 7 + (mu != 0 ? 2 : 1) iters launches on one stream (5 + ... when n_faces == 0), no spin barrier, no cooperative launch, no host read:
//   1. sm_init_kernel      the edge table (keys empty, count 0), the per-vertex degree, cursor and fixed words, the two flags.
//   2. sm_insert_kernel    a thread per face: range check, then its DISTINCT undirected edges go into the open-addressing table of
//                          mesh_edges.hpp; the thread that claims a slot adds one to the degree of both ends; every face adds one to
//                          the slot's count.
//   3. sm_scan_kernel      ONE workgroup: row[i] = the exclusive running sum of the degrees (scan_array).
//   4. sm_fill_kernel      grid-stride over table slots: the rows in arrival order; an edge of one face fixes both its ends (fill_rows).
//   5. sm_rows_kernel      a thread per vertex: the float64 start state, the finite check, and its row put into ASCENDING order in a second
//                          buffer (sort_rows).
//   6. sm_step_kernel      one launch per half-step, a thread per vertex, from one state buffer into the other (Jacobi).
//   7. sm_measure_kernel   a workgroup per chunk of SC_MESH_SMOOTH_CHUNK vertices of ONE image: a thread per vertex writes the output
//                          vertex and its three float64 terms to LDS, one lane per column folds it in ascending vertex number; the
//                          integers by LDS integer atomics; plain stores of the chunk's partials.
//   8. sm_final_kernel     a thread per image: the chunk partials in ascending chunk number, the means.
// mesh_edges.hpp states why every probe ends and why the sorted rows keep no trace of the arrival order.  Only integer atomics decide
// anything and no float is accumulated by an atomic: the same bits run to run, for any batch, stream, face order or table size.
// Bound: launch latency (a few thousand to a few ten thousand vertices) and the latency of the dependent row gathers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "shapeclipper_hip.h"
#include "mesh_edges.hpp"

namespace sc {
namespace sm {

constexpr int THREADS = 256;
constexpr int CHUNK = 256;                                  // vertices per chunk of the float64 sums: one workgroup
constexpr int SCAN_THREADS = 1024;                          // the one workgroup of the degree scan
constexpr int SCAN_ITEMS = 4;                               // consecutive degrees per thread and round
constexpr int SHORT_ROW = 32;                               // a row up to this long is ranked by its own thread
constexpr int MAX_BLOCKS = 4096;                            // cap of the grid-stride passes
constexpr int MAX_IMAGES = 65535;
constexpr int MAX_FACES = 1 << 26;                          // 6 F < 2^29: row offsets fit an int
constexpr int MAX_VERTS = 1 << 30;                          // a grid-stride index plus one stride fits an int
using sc_mesh::EMPTY;
using sc_mesh::image_of;
static_assert(CHUNK == SC_MESH_SMOOTH_CHUNK && CHUNK == THREADS, "the header states the chunk size; one thread per vertex of a chunk");

enum { FREE, FIXED_BOUNDARY, ISOLATED, DEGREE_MAX, FIELDS };             // rows of counts [FIELDS][n_images]
enum { ROUGH_BEFORE, ROUGH_AFTER, DISP_MEAN, DISP_MAX, MEASURES };       // rows of measures [MEASURES][n_images]
static_assert(FIELDS == SC_MESH_SMOOTH_FIELDS && MEASURES == SC_MESH_SMOOTH_MEASURES, "the header states the number of rows");

struct Scratch : sc_mesh::Rings {
    double *state[2];               // [V][3] each: the half-steps go from one into the other
    double* part;                   // [chunk slots][MEASURES]
    int* ipart;                     // [chunk slots][FIELDS]
};

__global__ __launch_bounds__(THREADS) void sm_init_kernel(Scratch s, int T, int V, int* bad_vertex, int* bad_index) {
    const int step = gridDim.x * THREADS, t0 = blockIdx.x * THREADS + threadIdx.x;
    for (int i = t0; i < T; i += step) s.keys[i] = EMPTY, s.count[i] = 0;
    for (int i = t0; i < V; i += step) s.deg[i] = 0, s.cursor[i] = 0, s.fixed[i] = 0;
    if (t0 == 0) *bad_vertex = 0, *bad_index = 0;
}

__global__ __launch_bounds__(THREADS) void sm_insert_kernel(const int* __restrict__ faces, const long long* __restrict__ v_off,
                                                            const long long* __restrict__ f_off, int B, int F, Scratch s, int T, int shift,
                                                            int* bad_index) {
    for (int f = blockIdx.x * THREADS + threadIdx.x; f < F; f += gridDim.x * THREADS) {
        const int b = image_of(f_off, B, f);
        const long long vs = v_off[b], nv = v_off[b + 1] - vs;
        const int i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        if (!(i[0] >= 0 && i[1] >= 0 && i[2] >= 0 && i[0] < nv && i[1] < nv && i[2] < nv)) {
            atomicOr(bad_index, 1);                         // takes part in nothing
            continue;
        }
        int lo[3], hi[3], n = 0;                            // the face's distinct undirected edges
        for (int k = 0; k < 3; ++k) {
            const int a = i[k], c = i[k == 2 ? 0 : k + 1];
            if (a == c) continue;
            const int l = a < c ? a : c, h = a < c ? c : a;
            bool seen = false;
            for (int e = 0; e < n; ++e) seen = seen || (lo[e] == l && hi[e] == h);
            if (!seen) lo[n] = l, hi[n] = h, ++n;
        }
        for (int e = 0; e < n; ++e) {
            const unsigned long long glo = (unsigned long long)(vs + lo[e]), ghi = (unsigned long long)(vs + hi[e]);
            const sc_mesh::EdgeSlot slot = sc_mesh::edge_slot(s.keys, T, shift, glo, ghi);
            if (slot.claimed) atomicAdd(s.deg + glo, 1), atomicAdd(s.deg + ghi, 1);
            atomicAdd(s.count + slot.at, 1);
        }
    }
}

// ONE workgroup: row[i] = deg[0] + ... + deg[i - 1], row[V] = the number of row entries
__global__ __launch_bounds__(SCAN_THREADS) void sm_scan_kernel(Scratch s, int V) {
    __shared__ int wave_tot[SCAN_THREADS / 64];
    sc_mesh::scan_array<SCAN_THREADS, SCAN_ITEMS>(s.deg, s.row, V, wave_tot);
}

__global__ __launch_bounds__(THREADS) void sm_fill_kernel(Scratch s, int T) { sc_mesh::fill_rows<THREADS, true>(s, T); }

__global__ __launch_bounds__(THREADS) void sm_rows_kernel(const float* __restrict__ verts, Scratch s, int V, int* bad_vertex) {
    for (int base = blockIdx.x * THREADS; base < V; base += gridDim.x * THREADS) {   // wave-uniform: the waves cooperate in sort_rows
        const int i = base + threadIdx.x;
        int r0 = 0, d = 0;
        if (i < V) {
            r0 = s.row[i], d = s.row[i + 1] - r0;
            bool finite = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float x = verts[3 * (size_t)i + c];
                finite = finite && sc_mesh::finite(x);
                s.state[0][3 * (size_t)i + c] = (double)x;
            }
            if (!finite) atomicOr(bad_vertex, 1);
        }
        sc_mesh::sort_rows<SHORT_ROW>(s, r0, d);
    }
}

// the mean of x (float64, or fp32 widened exactly) over row [r0, r1) in ascending neighbour number, from +0.0, one addition and one
// division per component
template <class X>
__device__ __forceinline__ void umbrella_mean(const X* __restrict__ x, const int* __restrict__ nbr, int r0, int r1, double (&m)[3]) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int r = r0; r < r1; ++r) {
        const size_t j = 3 * (size_t)nbr[r];
        sx = sx + (double)x[j], sy = sy + (double)x[j + 1], sz = sz + (double)x[j + 2];
    }
    const double n = (double)(r1 - r0);
    m[0] = sx / n, m[1] = sy / n, m[2] = sz / n;
}

__global__ __launch_bounds__(THREADS) void sm_step_kernel(const double* __restrict__ src, double* __restrict__ dst, Scratch s, int V,
                                                          double factor) {
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < V; i += gridDim.x * THREADS) {
        const int r0 = s.row[i], r1 = s.row[i + 1];
        double x[3] = {src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]};
        if (r1 > r0 && !s.fixed[i]) {
            double m[3];
            umbrella_mean(src, s.nbr, r0, r1, m);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double d = m[c] - x[c];
                const double t = factor * d;
                x[c] = x[c] + t;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[3 * (size_t)i + c] = x[c];
    }
}

__device__ __forceinline__ double norm3(double dx, double dy, double dz) { return __dsqrt_rn((dx * dx + dy * dy) + dz * dz); }

// grid: one workgroup per chunk slot
__global__ __launch_bounds__(THREADS) void sm_measure_kernel(const float* __restrict__ verts, const long long* __restrict__ v_off, int B,
                                                             Scratch s, const double* __restrict__ last, float* __restrict__ verts_out) {
    __shared__ double term[3][CHUNK];
    __shared__ int tally[FIELDS];
    long long first;
    const int b = sc_mesh::chunk_image<CHUNK>(v_off, B, first);
    const long long end = v_off[b + 1];
    if (first >= end) return;                               // a slot no image uses (workgroup-uniform)
    if (threadIdx.x < FIELDS) tally[threadIdx.x] = 0;
    __syncthreads();
    const long long i = first + threadIdx.x;
    double before = 0.0, after = 0.0, moved = 0.0;          // a vertex that is not free adds +0.0
    if (i < end) {
        const int r0 = s.row[i], r1 = s.row[i + 1], d = r1 - r0;
        const bool fixed = d > 0 && s.fixed[i] != 0, is_free = d > 0 && !fixed;
        atomicAdd(tally + (is_free ? FREE : fixed ? FIXED_BOUNDARY : ISOLATED), 1);
        atomicMax(tally + DEGREE_MAX, d);
        if (is_free) {
            double m[3];
            const double x0[3] = {(double)verts[3 * i], (double)verts[3 * i + 1], (double)verts[3 * i + 2]};       // the start state
            const double x1[3] = {last[3 * i], last[3 * i + 1], last[3 * i + 2]};
            umbrella_mean(verts, s.nbr, r0, r1, m);
            before = norm3(m[0] - x0[0], m[1] - x0[1], m[2] - x0[2]);
            umbrella_mean(last, s.nbr, r0, r1, m);
            after = norm3(m[0] - x1[0], m[1] - x1[1], m[2] - x1[2]);
            moved = norm3(x1[0] - x0[0], x1[1] - x0[1], x1[2] - x0[2]);
#pragma unroll
            for (int c = 0; c < 3; ++c) verts_out[3 * i + c] = (float)x1[c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) verts_out[3 * i + c] = verts[3 * i + c];     // a fixed vertex keeps its bits
        }
    }
    term[0][threadIdx.x] = before, term[1][threadIdx.x] = after, term[2][threadIdx.x] = moved;
    __syncthreads();
    const int n = end - first < CHUNK ? (int)(end - first) : CHUNK;
    if ((threadIdx.x & 63) == 0) {                          // lane 0 of the four waves: one column each, ascending vertex number
        const int q = threadIdx.x >> 6;
        double acc = 0.0;
        if (q < 3) for (int t = 0; t < n; ++t) acc = acc + term[q][t];
        else for (int t = 0; t < n; ++t) acc = term[2][t] > acc ? term[2][t] : acc;
        s.part[MEASURES * (size_t)blockIdx.x + q] = acc;
    }
    if (threadIdx.x < FIELDS) s.ipart[FIELDS * (size_t)blockIdx.x + threadIdx.x] = tally[threadIdx.x];
}

__global__ __launch_bounds__(THREADS) void sm_final_kernel(const long long* __restrict__ v_off, int B, Scratch s, long long* __restrict__ counts,
                                                           double* __restrict__ measures) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    const long long chunks = (v_off[b + 1] - v_off[b] + CHUNK - 1) / CHUNK, start = sc_mesh::chunk_start<CHUNK>(v_off, b);
    double sum[3] = {0.0, 0.0, 0.0}, top = 0.0;
    long long n[FIELDS] = {0, 0, 0, 0};
    for (long long c = 0; c < chunks; ++c) {
        const double* p = s.part + MEASURES * (start + c);
        const int* q = s.ipart + FIELDS * (start + c);
#pragma unroll
        for (int k = 0; k < 3; ++k) sum[k] = sum[k] + p[k];
        top = p[3] > top ? p[3] : top;
        n[FREE] += q[FREE], n[FIXED_BOUNDARY] += q[FIXED_BOUNDARY], n[ISOLATED] += q[ISOLATED];
        n[DEGREE_MAX] = q[DEGREE_MAX] > n[DEGREE_MAX] ? q[DEGREE_MAX] : n[DEGREE_MAX];
    }
#pragma unroll
    for (int k = 0; k < FIELDS; ++k) counts[(size_t)k * B + b] = n[k];
    const bool any = n[FREE] > 0;
    const double free_count = (double)n[FREE];
    measures[(size_t)ROUGH_BEFORE * B + b] = any ? sum[0] / free_count : 0.0;
    measures[(size_t)ROUGH_AFTER * B + b] = any ? sum[1] / free_count : 0.0;
    measures[(size_t)DISP_MEAN * B + b] = any ? sum[2] / free_count : 0.0;
    measures[(size_t)DISP_MAX * B + b] = any ? top : 0.0;
}

using sc_mesh::align16;
static inline bool sizes_ok(int n_images, long long n_verts, long long n_faces, long long table_slots) {
    return n_images >= 1 && n_images <= MAX_IMAGES && n_verts >= 0 && n_verts <= MAX_VERTS && n_faces >= 0 && n_faces <= MAX_FACES &&
           sc_mesh::slots_ok(table_slots, n_faces);
}
constexpr auto chunk_slots = sc_mesh::chunk_slots<CHUNK>;
constexpr auto blocks = sc_mesh::blocks<THREADS, MAX_BLOCKS>;

}  // namespace sm
}  // namespace sc

// scratch layout: keys [T] u64 | state 0, state 1 [V][3] f64 | part [slots][4] f64 | count [T] | deg, cursor, fixed [V] | row [V + 1] |
// raw, nbr [6 F] | ipart [slots][4]
extern "C" long long sc_mesh_smooth_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots) {
    using namespace sc::sm;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots)) return 0;
    const long long T = table_slots, F = n_faces, V = n_verts, slots = chunk_slots(n_images, V);
    return align16(8 * T) + 2 * align16(24 * V) + align16(8 * MEASURES * slots) + align16(4 * T) + 3 * align16(4 * V) + align16(4 * (V + 1)) +
           2 * align16(24 * F) + align16(4 * FIELDS * slots) + 16;
}

extern "C" int sc_mesh_smooth(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images, int n_verts,
                              int n_faces, int table_slots, int iters, double lam, double mu, void* scratch, float* verts_out,
                              int64_t* counts, double* measures, int32_t* bad_vertex, int32_t* bad_index, void* stream_) {
    using namespace sc::sm;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots) || iters < 0 || iters > SC_MESH_SMOOTH_MAX_ITERS || !(lam > 0.0 && lam <= 1.0) ||
        !(mu >= -1.0 && mu <= 0.0) || !v_off || !f_off || !counts || !measures || !bad_vertex || !bad_index || !scratch ||
        ((uintptr_t)scratch & 15) || (n_verts > 0 && (!verts || !verts_out)) || (n_faces > 0 && !faces))
        return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = n_images, V = n_verts, F = n_faces, T = table_slots;
    const int shift = sc_mesh::table_shift(T);
    const long long slots = chunk_slots(B, V);
    sc_mesh::Carver ws{(char*)scratch};
    Scratch s;
    ws.take(s.keys, T);
    ws.take(s.state[0], 3LL * V), ws.take(s.state[1], 3LL * V);
    ws.take(s.part, MEASURES * slots);
    ws.take(s.count, T);
    ws.take(s.deg, V), ws.take(s.cursor, V), ws.take(s.fixed, V);
    ws.take(s.row, V + 1LL);
    ws.take(s.raw, 6LL * F), ws.take(s.nbr, 6LL * F);
    ws.take(s.ipart, FIELDS * slots);
    const long long *vo = (const long long*)v_off, *fo = (const long long*)f_off;
    hipLaunchKernelGGL(sm_init_kernel, dim3(blocks(T > V ? T : V)), dim3(THREADS), 0, stream, s, T, V, bad_vertex, bad_index);
    if (F > 0)
        hipLaunchKernelGGL(sm_insert_kernel, dim3(blocks(F)), dim3(THREADS), 0, stream, faces, vo, fo, B, F, s, T, shift, bad_index);
    hipLaunchKernelGGL(sm_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, s, V);
    if (F > 0) hipLaunchKernelGGL(sm_fill_kernel, dim3(blocks(T)), dim3(THREADS), 0, stream, s, T);
    int at = 0;                                             // the state buffer that holds the current state
    if (V > 0) {
        hipLaunchKernelGGL(sm_rows_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, verts, s, V, bad_vertex);
        for (int it = 0; it < iters; ++it) {
            hipLaunchKernelGGL(sm_step_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, (const double*)s.state[at], s.state[at ^ 1], s, V, lam);
            at ^= 1;
            if (mu != 0.0) {
                hipLaunchKernelGGL(sm_step_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, (const double*)s.state[at], s.state[at ^ 1], s, V, mu);
                at ^= 1;
            }
        }
    }
    hipLaunchKernelGGL(sm_measure_kernel, dim3((unsigned)slots), dim3(THREADS), 0, stream, verts, vo, B, s, (const double*)s.state[at],
                       verts_out);
    hipLaunchKernelGGL(sm_final_kernel, dim3((unsigned)((B + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, vo, B, s, (long long*)counts,
                       measures);
    return (int)hipGetLastError();
}
