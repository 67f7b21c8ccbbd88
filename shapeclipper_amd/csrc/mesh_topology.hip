// mesh_topology.hip -- watertightness, manifoldness, orientation, components, genus, area and volume of a batch of indexed triangle
// meshes (ops.mesh_topology, the evaluation's mesh_stats.txt; definition in include/shapeclipper_hip.h, sc_mesh_topology; restated
// in numpy by tests/mesh_topology_ref.py).  Built without contraction: the float64 terms of area and volume round once per operation.
//
// Seven launches on one stream, no spin barrier, no cooperative launch, no host read:
//   1. mt_init_kernel      the edge table (keys empty, count 0, fwd 0, minface INT_MAX), the per-vertex words and the outputs.
//   2. mt_insert_kernel    a thread per face: range check, degenerate check, then its three undirected edges go into the open-addressing
//                          table of mesh_edges.hpp; integer atomicAdd on count and fwd, atomicMin on minface.  The slot of every
//                          half-edge is kept.
//   3. mt_unite_kernel     a thread per half-edge: the face unites with the edge's minface, its two corners on the edge with minface's
//                          corners at the same vertices.  Two union-finds (faces, corners), the one of mesh_edges.hpp.
//   4. mt_flatten_kernel   a thread per face: face_component = root - first face of the image; roots count components, every face adds
//                          one to its root's size; every corner root adds one fan to its vertex.
//   5. mt_count_kernel     grid-stride over table slots (edges by count and fwd), vertices (referenced, fans) and faces (largest
//                          component): wave-folded integer sums, one integer atomic per wave and field.
//   6. mt_measure_kernel   a workgroup per chunk of SC_MESH_TOPOLOGY_CHUNK faces of ONE image: a thread per face writes its two
//                          float64 terms to LDS, one lane adds each of the two columns in ascending face index; plain stores.
//   7. mt_final_kernel     a thread per image: the chunk partials in ascending chunk number, euler, the three flags, genus.
// mesh_edges.hpp states why every probe and every find loop ends.  Only integer atomics decide integer outputs and no float is
// accumulated by an atomic: the same bits run to run, for any batch, stream or table size.
// Bound: latency of scattered 8- and 4-byte atomics on the table and of dependent label loads; not a hot path of training.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "shapeclipper_hip.h"
#include "mesh_edges.hpp"

namespace sc {
namespace mt {

constexpr int THREADS = 256;
constexpr int CHUNK = 256;                                  // faces per chunk of the float64 sums: one workgroup
constexpr int MAX_BLOCKS = 4096;                            // cap of the grid-stride passes
constexpr int MAX_IMAGES = 65535;
constexpr int MAX_FACES = 1 << 26;                          // 3 F < 2^28: half-edge and corner numbers fit an int
using sc_mesh::EMPTY;
using sc_mesh::image_of;
static_assert(CHUNK == SC_MESH_TOPOLOGY_CHUNK && CHUNK == THREADS, "the header states the chunk size; one thread per face of a chunk");

// rows of counts [SC_MESH_TOPOLOGY_FIELDS][n_images]
enum { VERTICES, UNREFERENCED, FACES, DEGENERATE, EDGES, BOUNDARY, NONMANIFOLD_E, INCONSISTENT, COMPONENTS, LARGEST, NONMANIFOLD_V, EULER,
       GENUS, WATERTIGHT, ORIENTED, MANIFOLD, FIELDS };
static_assert(FIELDS == SC_MESH_TOPOLOGY_FIELDS, "the header states the number of rows");

struct Scratch {
    unsigned long long* keys;       // [T]
    double* part;                   // [chunk slots][2]: area, volume
    int *count, *fwd, *minface;     // [T]
    int *slot;                      // [3 F] table slot of every half-edge
    int *flabel, *fsize;            // [F]
    int *clabel;                    // [3 F]
    int *vref, *vfans;              // [V]
};

__global__ __launch_bounds__(THREADS) void mt_init_kernel(Scratch s, int T, int V, int B, unsigned long long* counts, double* area,
                                                          double* volume, int* bad) {
    const int step = gridDim.x * THREADS, t0 = blockIdx.x * THREADS + threadIdx.x;
    for (int i = t0; i < T; i += step) s.keys[i] = EMPTY, s.count[i] = 0, s.fwd[i] = 0, s.minface[i] = INT_MAX;
    for (int i = t0; i < V; i += step) s.vref[i] = 0, s.vfans[i] = 0;
    for (int i = t0; i < B * FIELDS; i += step) counts[i] = 0ull;
    for (int i = t0; i < B; i += step) area[i] = 0.0, volume[i] = 0.0;
    if (t0 == 0) *bad = 0;
}

__global__ __launch_bounds__(THREADS) void mt_insert_kernel(const int* __restrict__ faces, const long long* __restrict__ v_off,
                                                            const long long* __restrict__ f_off, int B, int F, Scratch s, int T, int shift,
                                                            unsigned long long* counts, int* __restrict__ face_component, int* bad) {
    for (int base = blockIdx.x * THREADS; base < F; base += gridDim.x * THREADS) {
        const int f = base + threadIdx.x;
        int b = -1;
        int v[2] = {0, 0};
        if (f < F) {
            b = image_of(f_off, B, f);
            const long long vs = v_off[b], nv = v_off[b + 1] - vs;
            const int i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
            const bool in_range = i[0] >= 0 && i[1] >= 0 && i[2] >= 0 && i[0] < nv && i[1] < nv && i[2] < nv;
            const bool degenerate = i[0] == i[1] || i[1] == i[2] || i[0] == i[2];
            if (!in_range || degenerate) {                  // takes part in nothing else
                if (!in_range) atomicOr(bad, 1), b = -1; else v[1] = 1;
                s.flabel[f] = -1, s.fsize[f] = 0, face_component[f] = -1;
                for (int k = 0; k < 3; ++k) s.clabel[3 * f + k] = -1, s.slot[3 * f + k] = -1;
            } else {
                v[0] = 1;
                s.flabel[f] = f, s.fsize[f] = 0;
                for (int k = 0; k < 3; ++k) {
                    s.clabel[3 * f + k] = 3 * f + k;
                    s.vref[vs + i[k]] = 1;                  // every writer stores the same word
                    const int a = i[k], c = i[k == 2 ? 0 : k + 1];
                    const unsigned long long glo = (unsigned long long)(vs + (a < c ? a : c)), ghi = (unsigned long long)(vs + (a < c ? c : a));
                    const int at = sc_mesh::edge_slot(s.keys, T, shift, glo, ghi).at;
                    atomicAdd(s.count + at, 1);
                    if (a < c) atomicAdd(s.fwd + at, 1);    // the face lists the lower end first
                    atomicMin(s.minface + at, f);
                    s.slot[3 * f + k] = at;
                }
            }
        }
        const int field[2] = {FACES, DEGENERATE};
        sc_mesh::image_add<2>(counts, B, b, field, v);
    }
}

__global__ __launch_bounds__(THREADS) void mt_unite_kernel(const int* __restrict__ faces, int F, Scratch s) {
    for (int h = blockIdx.x * THREADS + threadIdx.x; h < 3 * F; h += gridDim.x * THREADS) {
        const int at = s.slot[h];
        if (at < 0) continue;
        const int f = h / 3, k = h - 3 * f, m = s.minface[at];
        if (m == f) continue;
        sc_mesh::unite(s.flabel, f, m);
        const int k1 = k == 2 ? 0 : k + 1;
        const int a = faces[3 * f + k], c = faces[3 * f + k1];
        const int m0 = faces[3 * m], m1 = faces[3 * m + 1];     // m lies on the edge: it holds a and c
        sc_mesh::unite(s.clabel, 3 * f + k, 3 * m + (m0 == a ? 0 : m1 == a ? 1 : 2));
        sc_mesh::unite(s.clabel, 3 * f + k1, 3 * m + (m0 == c ? 0 : m1 == c ? 1 : 2));
    }
}

__global__ __launch_bounds__(THREADS) void mt_flatten_kernel(const int* __restrict__ faces, const long long* __restrict__ v_off,
                                                             const long long* __restrict__ f_off, int B, int F, Scratch s,
                                                             unsigned long long* counts, int* __restrict__ face_component) {
    for (int base = blockIdx.x * THREADS; base < F; base += gridDim.x * THREADS) {
        const int f = base + threadIdx.x;
        int b = -1;
        int v[1] = {0};
        if (f < F && s.slot[3 * f] >= 0) {                  // a face that takes part
            b = image_of(f_off, B, f);
            const int r = sc_mesh::find(s.flabel, f);
            face_component[f] = r - (int)f_off[b];
            atomicAdd(s.fsize + r, 1);
            v[0] = r == f;
            const long long vs = v_off[b];
            for (int k = 0; k < 3; ++k)
                if (sc_mesh::find(s.clabel, 3 * f + k) == 3 * f + k) atomicAdd(s.vfans + vs + faces[3 * f + k], 1);
        }
        const int field[1] = {COMPONENTS};
        sc_mesh::image_add<1>(counts, B, b, field, v);
    }
}

__global__ __launch_bounds__(THREADS) void mt_count_kernel(const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B,
                                                           int V, int F, int T, Scratch s, unsigned long long* counts) {
    const int step = gridDim.x * THREADS;
    for (int base = blockIdx.x * THREADS; base < T; base += step) {
        const int i = base + threadIdx.x;
        int b = -1;
        int v[4] = {0, 0, 0, 0};
        if (i < T) {
            const unsigned long long key = s.keys[i];
            if (key != EMPTY) {
                b = image_of(v_off, B, (long long)(key >> 32));
                const int c = s.count[i];
                v[0] = 1, v[1] = c == 1, v[2] = c >= 3, v[3] = c == 2 && s.fwd[i] != 1;
            }
        }
        const int field[4] = {EDGES, BOUNDARY, NONMANIFOLD_E, INCONSISTENT};
        sc_mesh::image_add<4>(counts, B, b, field, v);
    }
    for (int base = blockIdx.x * THREADS; base < V; base += step) {
        const int i = base + threadIdx.x;
        int b = -1;
        int v[3] = {0, 0, 0};
        if (i < V) {
            b = image_of(v_off, B, i);
            const int ref = s.vref[i];
            v[0] = ref, v[1] = !ref, v[2] = s.vfans[i] > 1;
        }
        const int field[3] = {VERTICES, UNREFERENCED, NONMANIFOLD_V};
        sc_mesh::image_add<3>(counts, B, b, field, v);
    }
    for (int f = blockIdx.x * THREADS + threadIdx.x; f < F; f += step)
        if (s.flabel[f] == f) atomicMax(counts + (size_t)LARGEST * B + image_of(f_off, B, f), (unsigned long long)s.fsize[f]);
}

// grid: one workgroup per chunk slot
__global__ __launch_bounds__(THREADS) void mt_measure_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                             const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B,
                                                             double* __restrict__ part) {
    __shared__ double term[2][CHUNK];
    long long first;
    const int b = sc_mesh::chunk_image<CHUNK>(f_off, B, first);
    const long long end = f_off[b + 1];
    if (first >= end) return;                               // a slot no image uses (workgroup-uniform)
    const long long f = first + threadIdx.x, vs = v_off[b], nv = v_off[b + 1] - vs;
    double a = 0.0, w = 0.0;                                // a face that takes part in nothing adds +0.0
    if (f < end) {
        const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
        const bool in_range = i0 >= 0 && i1 >= 0 && i2 >= 0 && i0 < nv && i1 < nv && i2 < nv;
        if (in_range && i0 != i1 && i1 != i2 && i0 != i2) {
            double p[3][3];
            const int idx[3] = {i0, i1, i2};
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int c = 0; c < 3; ++c) p[k][c] = (double)verts[(vs + idx[k]) * 3 + c];
            const double e1[3] = {p[1][0] - p[0][0], p[1][1] - p[0][1], p[1][2] - p[0][2]};
            const double e2[3] = {p[2][0] - p[0][0], p[2][1] - p[0][1], p[2][2] - p[0][2]};
            const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
            a = __dsqrt_rn((nx * nx + ny * ny) + nz * nz) * 0.5;
            const double cx = p[1][1] * p[2][2] - p[1][2] * p[2][1], cy = p[1][2] * p[2][0] - p[1][0] * p[2][2],
                         cz = p[1][0] * p[2][1] - p[1][1] * p[2][0];
            w = ((p[0][0] * cx + p[0][1] * cy) + p[0][2] * cz) / 6.0;
        }
    }
    term[0][threadIdx.x] = a, term[1][threadIdx.x] = w;
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {      // lane 0 of waves 0 and 1: one column each, ascending face index
        const int q = threadIdx.x >> 6;
        const int n = end - first < CHUNK ? (int)(end - first) : CHUNK;
        double sum = 0.0;
        for (int t = 0; t < n; ++t) sum += term[q][t];
        part[2 * (size_t)blockIdx.x + q] = sum;
    }
}

__global__ __launch_bounds__(THREADS) void mt_final_kernel(const long long* __restrict__ f_off, int B, const double* __restrict__ part,
                                                           long long* counts, double* __restrict__ area, double* __restrict__ volume) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= B) return;
    const long long chunks = (f_off[b + 1] - f_off[b] + CHUNK - 1) / CHUNK, start = sc_mesh::chunk_start<CHUNK>(f_off, b);
    double a = 0.0, w = 0.0;
    for (long long c = 0; c < chunks; ++c) a += part[2 * (start + c)], w += part[2 * (start + c) + 1];
    area[b] = a, volume[b] = w;
    auto at = [&](int field) -> long long& { return counts[(size_t)field * B + b]; };
    const long long euler = at(VERTICES) - at(EDGES) + at(FACES);
    const bool watertight = at(BOUNDARY) == 0 && at(NONMANIFOLD_E) == 0, oriented = at(INCONSISTENT) == 0;
    const bool manifold = at(NONMANIFOLD_E) == 0 && at(NONMANIFOLD_V) == 0;
    at(EULER) = euler;
    at(WATERTIGHT) = watertight, at(ORIENTED) = oriented, at(MANIFOLD) = manifold;
    at(GENUS) = (watertight && oriented && manifold && at(FACES) > 0) ? at(COMPONENTS) - euler / 2 : -1;
}

using sc_mesh::align16;
static inline bool sizes_ok(int n_images, long long n_verts, long long n_faces, long long table_slots) {
    return n_images >= 1 && n_images <= MAX_IMAGES && n_verts >= 0 && n_verts <= INT_MAX && n_faces >= 0 && n_faces <= MAX_FACES &&
           sc_mesh::slots_ok(table_slots, n_faces);
}
constexpr auto chunk_slots = sc_mesh::chunk_slots<CHUNK>;
constexpr auto blocks = sc_mesh::blocks<THREADS, MAX_BLOCKS>;

}  // namespace mt
}  // namespace sc

// scratch layout: keys [T] u64 | part [slots][2] f64 | count, fwd, minface [T] | slot [3F] | flabel, fsize [F] | clabel [3F] | vref, vfans [V]
extern "C" long long sc_mesh_topology_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots) {
    using namespace sc::mt;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots)) return 0;
    const long long T = table_slots, F = n_faces, V = n_verts;
    return align16(8 * T) + align16(16 * chunk_slots(n_images, F)) + 3 * align16(4 * T) + 2 * align16(12 * F) + 2 * align16(4 * F) +
           2 * align16(4 * V) + 16;
}

extern "C" int sc_mesh_topology(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images,
                                int n_verts, int n_faces, int table_slots, void* scratch, int64_t* counts, double* area, double* volume,
                                int32_t* face_component, int32_t* bad_index, void* stream_) {
    using namespace sc::mt;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots) || !v_off || !f_off || !counts || !area || !volume || !bad_index || !scratch ||
        ((uintptr_t)scratch & 15) || (n_verts > 0 && !verts) || (n_faces > 0 && (!faces || !face_component)))
        return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = n_images, V = n_verts, F = n_faces, T = table_slots;
    const int shift = sc_mesh::table_shift(T);
    sc_mesh::Carver ws{(char*)scratch};
    Scratch s;
    ws.take(s.keys, T);
    ws.take(s.part, 2 * chunk_slots(B, F));
    ws.take(s.count, T), ws.take(s.fwd, T), ws.take(s.minface, T);
    ws.take(s.slot, 3LL * F);
    ws.take(s.flabel, F), ws.take(s.fsize, F);
    ws.take(s.clabel, 3LL * F);
    ws.take(s.vref, V), ws.take(s.vfans, V);
    const long long widest = T > V ? T : V;
    const long long *vo = (const long long*)v_off, *fo = (const long long*)f_off;
    unsigned long long* acc = (unsigned long long*)counts;
    hipLaunchKernelGGL(mt_init_kernel, dim3(blocks(widest)), dim3(THREADS), 0, stream, s, T, V, B, acc, area, volume, bad_index);
    if (F > 0) {
        hipLaunchKernelGGL(mt_insert_kernel, dim3(blocks(F)), dim3(THREADS), 0, stream, faces, vo, fo, B, F, s, T, shift, acc, face_component,
                           bad_index);
        hipLaunchKernelGGL(mt_unite_kernel, dim3(blocks(3LL * F)), dim3(THREADS), 0, stream, faces, F, s);
        hipLaunchKernelGGL(mt_flatten_kernel, dim3(blocks(F)), dim3(THREADS), 0, stream, faces, vo, fo, B, F, s, acc, face_component);
    }
    hipLaunchKernelGGL(mt_count_kernel, dim3(blocks(widest > F ? widest : F)), dim3(THREADS), 0, stream, vo, fo, B, V, F, F > 0 ? T : 0, s, acc);
    if (F > 0)
        hipLaunchKernelGGL(mt_measure_kernel, dim3((unsigned)chunk_slots(B, F)), dim3(THREADS), 0, stream, verts, faces, vo, fo, B, s.part);
    hipLaunchKernelGGL(mt_final_kernel, dim3((unsigned)((B + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, fo, B,
                       (const double*)s.part, (long long*)counts, area, volume);
    return (int)hipGetLastError();
}
