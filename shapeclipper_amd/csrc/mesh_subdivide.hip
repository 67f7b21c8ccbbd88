// mesh_subdivide.hip -- one Loop subdivision step of a batch of indexed triangle meshes (Warren's weights, sharp edges and their ends held
// fixed) and one clamped Newton step of vertices onto the zero set of an SDF (ops.mesh_subdivide / ops.mesh_project_step, the evaluation's
// {idx}_mesh_subdiv.ply; definitions in include/shapeclipper_hip.h, sc_mesh_subdivide and sc_mesh_project_step; restated in numpy by
// tests/mesh_subdivide_ref.py).  Built without contraction: every float64 operation of the subdivision rules and every fp32 operation of
// the Newton step rounds once.
//
// sc_mesh_subdivide: 8 launches on one stream (5 when n_faces == 0), no spin barrier, no cooperative launch, no host read:
//   1. sd_init_kernel     the edge table (keys empty, count 0, owner and omin INT_MAX, omax -1), the per-vertex degree, cursor and fixed
//                         words, the three flags.
//   2. sd_insert_kernel   a thread per face: range and repeated-index check, then its three undirected edges go into the open-addressing
//                         table of mesh_edges.hpp; the thread that claims a slot adds one to the degree of both ends; every half-edge
//                         adds one to the slot's count, takes part in the atomicMin of `owner` with its number 3 f + c and in the
//                         atomicMin / atomicMax of omin / omax with its opposite corner, and remembers its slot.
//   3. sd_owner_kernel    a thread per half-edge: the flag "I am my edge's owner".
//   4. sd_scan_kernel     ONE workgroup: row[i] = the exclusive running sum of the degrees, rank[h] = the exclusive running sum of the owner
//                         flags (scan_array, twice).  rank[3 f_off[b+1]] - rank[3 f_off[b]] is image b's edge count, and
//                         rank[3 f_off[b]] the new vertices of the images before it: the output offsets.
//   5. sd_fill_kernel     grid-stride over table slots: the rows in arrival order; an edge whose count is not 2 is sharp and fixes both
//                         its ends (fill_rows).
//   6. sd_rows_kernel     a thread per vertex: the finite check, and its row put into ASCENDING order in a second buffer (sort_rows).
//   7. sd_emit_kernel     grid-stride, three passes: a thread per old vertex (the even rule), per half-edge (an owner writes its edge's new
//                         vertex) and per face (its four faces).  All read the input vertices only.
//   8. sd_final_kernel    a workgroup per image: the six counts by LDS integer atomics.
// mesh_edges.hpp states why every probe ends and why the sorted rows keep no trace of the arrival order.  Only integer atomics decide
// anything and no float is accumulated by an atomic: the same bits run to run, for any batch, stream and table size; the numbering follows
// the input face order.
// Bound: launch latency (a few thousand to a few hundred thousand faces), the scattered 8-byte compare-and-swaps and the one-workgroup scan.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "shapeclipper_hip.h"
#include "mesh_edges.hpp"

namespace sc {
namespace sd {

constexpr int THREADS = 256;
constexpr int SCAN_THREADS = 1024;                          // the one workgroup of the two scans
constexpr int SCAN_ITEMS = 8;                               // consecutive values per thread and round
constexpr int FINAL_THREADS = 1024;                         // the workgroup of an image's counts
constexpr int SHORT_ROW = 32;                               // a row up to this long is ranked by its own thread
constexpr int MAX_BLOCKS = 4096;                            // cap of the grid-stride passes
constexpr int MAX_IMAGES = 65535;
constexpr int MAX_FACES = 1 << 24;                          // 4 F <= 2^26: the output is an input of the next level
constexpr int MAX_VERTS = 1 << 30;                          // V + 3 F < 2^31
using sc_mesh::EMPTY;
using sc_mesh::image_of;

enum { VERTICES_OUT, EDGES, SHARP_EDGES, FIXED_VERTICES, ISOLATED, DEGREE_MAX, FIELDS };     // rows of counts [FIELDS][n_images]
static_assert(FIELDS == SC_MESH_SUBDIVIDE_FIELDS, "the header states the number of rows");

struct Scratch : sc_mesh::Rings {
    int *owner, *omin, *omax;       // [T] the edge's lowest half-edge, its lowest and highest opposite vertex (global)
    int* hslot;                     // [3 F] the slot of half-edge 3 f + c; -1 for a face that takes part in nothing
    int* rank;                      // [3 F + 1] owner flags, then their exclusive running sum
};

__global__ __launch_bounds__(THREADS) void sd_init_kernel(Scratch s, int T, int V, int* bad_vertex, int* bad_index, int* bad_face) {
    const int step = gridDim.x * THREADS, t0 = blockIdx.x * THREADS + threadIdx.x;
    for (int i = t0; i < T; i += step) s.keys[i] = EMPTY, s.count[i] = 0, s.owner[i] = INT_MAX, s.omin[i] = INT_MAX, s.omax[i] = -1;
    for (int i = t0; i < V; i += step) s.deg[i] = 0, s.cursor[i] = 0, s.fixed[i] = 0;
    if (t0 == 0) *bad_vertex = 0, *bad_index = 0, *bad_face = 0;
}

__global__ __launch_bounds__(THREADS) void sd_insert_kernel(const int* __restrict__ faces, const long long* __restrict__ v_off,
                                                            const long long* __restrict__ f_off, int B, int F, Scratch s, int T, int shift,
                                                            int* bad_index, int* bad_face) {
    for (int f = blockIdx.x * THREADS + threadIdx.x; f < F; f += gridDim.x * THREADS) {
        const int b = image_of(f_off, B, f);
        const long long vs = v_off[b], nv = v_off[b + 1] - vs;
        const int i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        const bool in_range = i[0] >= 0 && i[1] >= 0 && i[2] >= 0 && i[0] < nv && i[1] < nv && i[2] < nv;
        if (!in_range || i[0] == i[1] || i[1] == i[2] || i[2] == i[0]) {
            atomicOr(in_range ? bad_face : bad_index, 1);   // takes part in nothing
            s.hslot[3 * f] = -1, s.hslot[3 * f + 1] = -1, s.hslot[3 * f + 2] = -1;
            continue;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {                       // corner c's edge runs from i_c to i_{c+1}; i_{c+2} lies opposite
            const int a = i[c], e = i[c == 2 ? 0 : c + 1], opp = (int)vs + i[c == 0 ? 2 : c - 1];
            const unsigned long long glo = (unsigned long long)(vs + (a < e ? a : e)), ghi = (unsigned long long)(vs + (a < e ? e : a));
            const sc_mesh::EdgeSlot slot = sc_mesh::edge_slot(s.keys, T, shift, glo, ghi);
            const int at = slot.at;
            if (slot.claimed) atomicAdd(s.deg + glo, 1), atomicAdd(s.deg + ghi, 1);
            atomicAdd(s.count + at, 1);
            atomicMin(s.owner + at, 3 * f + c);
            atomicMin(s.omin + at, opp);
            atomicMax(s.omax + at, opp);
            s.hslot[3 * f + c] = at;
        }
    }
}

__global__ __launch_bounds__(THREADS) void sd_owner_kernel(Scratch s, int H) {
    for (int h = blockIdx.x * THREADS + threadIdx.x; h < H; h += gridDim.x * THREADS) {
        const int at = s.hslot[h];
        s.rank[h] = at >= 0 && s.owner[at] == h;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void sd_scan_kernel(Scratch s, int V, int H) {
    __shared__ int wave_tot[SCAN_THREADS / 64];
    sc_mesh::scan_array<SCAN_THREADS, SCAN_ITEMS>(s.deg, s.row, V, wave_tot);
    sc_mesh::scan_array<SCAN_THREADS, SCAN_ITEMS>(s.rank, s.rank, H, wave_tot);
}

__global__ __launch_bounds__(THREADS) void sd_fill_kernel(Scratch s, int T) { sc_mesh::fill_rows<THREADS, false>(s, T); }

__global__ __launch_bounds__(THREADS) void sd_rows_kernel(const float* __restrict__ verts, Scratch s, int V, int* bad_vertex) {
    for (int base = blockIdx.x * THREADS; base < V; base += gridDim.x * THREADS) {   // wave-uniform: the waves cooperate in sort_rows
        const int i = base + threadIdx.x;
        int r0 = 0, d = 0;
        if (i < V) {
            r0 = s.row[i], d = s.row[i + 1] - r0;
            bool finite = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) finite = finite && sc_mesh::finite(verts[3 * (size_t)i + c]);
            if (!finite) atomicOr(bad_vertex, 1);
        }
        sc_mesh::sort_rows<SHORT_ROW>(s, r0, d);
    }
}

__global__ __launch_bounds__(THREADS) void sd_emit_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B,
                                                          int V, int F, Scratch s, float* __restrict__ verts_out, int* __restrict__ faces_out,
                                                          unsigned char* __restrict__ fixed_out) {
    const int step = gridDim.x * THREADS, t0 = blockIdx.x * THREADS + threadIdx.x;
    // even: old vertex i of image b keeps its number; its row is i + the new vertices of the images before b
    for (int i = t0; i < V; i += step) {
        const int b = image_of(v_off, B, i);
        const size_t out = (size_t)i + s.rank[3 * f_off[b]];
        const int r0 = s.row[i], r1 = s.row[i + 1], n = r1 - r0;
        const bool fixed = s.fixed[i] != 0;
        fixed_out[out] = fixed;
        if (n == 0 || fixed) {
#pragma unroll
            for (int c = 0; c < 3; ++c) verts_out[3 * out + c] = verts[3 * (size_t)i + c];       // keeps its bits
            continue;
        }
        double sx = 0.0, sy = 0.0, sz = 0.0;
        for (int r = r0; r < r1; ++r) {
            const size_t j = 3 * (size_t)s.nbr[r];
            sx = sx + (double)verts[j], sy = sy + (double)verts[j + 1], sz = sz + (double)verts[j + 2];
        }
        const double beta = n == 3 ? 0.1875 : 0.375 / (double)n, w = n == 3 ? 0.4375 : 0.625;
        const double sum[3] = {sx, sy, sz};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double own = w * (double)verts[3 * (size_t)i + c];
            const double ring = beta * sum[c];
            const double x = own + ring;
            verts_out[3 * out + c] = (float)x;
        }
    }
    // odd: the owner of an edge writes its vertex, number V_b + its rank among the image's owners
    for (int h = t0; h < 3 * F; h += step) {
        const int at = s.hslot[h];
        if (at < 0 || s.owner[at] != h) continue;
        const int b = image_of(f_off, B, h / 3);
        const size_t out = (size_t)v_off[b + 1] + s.rank[h];
        const unsigned long long key = s.keys[at];
        const size_t lo = 3 * (size_t)(key >> 32), hi = 3 * (size_t)(key & 0xFFFFFFFFull);
        const bool interior = s.count[at] == 2;
        const size_t p = 3 * (size_t)s.omin[at], q = 3 * (size_t)s.omax[at];
        fixed_out[out] = !interior;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double ends = (double)verts[lo + c] + (double)verts[hi + c];
            double x;
            if (interior) {
                const double wings = (double)verts[p + c] + (double)verts[q + c];
                const double near = 0.375 * ends;
                const double far = 0.125 * wings;
                x = near + far;
            } else {
                x = 0.5 * ends;
            }
            verts_out[3 * out + c] = (float)x;
        }
    }
    // faces: face f becomes 4 f .. 4 f + 3, the winding kept
    for (int f = t0; f < F; f += step) {
        const int b = image_of(f_off, B, f);
        const int first = s.rank[3 * f_off[b]], nv = (int)(v_off[b + 1] - v_off[b]);
        int i[3], m[3];
        bool ok = true;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int at = s.hslot[3 * f + c];
            ok = ok && at >= 0;
            i[c] = faces[3 * f + c];
            m[c] = at >= 0 ? nv + s.rank[s.owner[at]] - first : 0;
        }
        const int quad[12] = {i[0], m[0], m[2], i[1], m[1], m[0], i[2], m[2], m[1], m[0], m[1], m[2]};
#pragma unroll
        for (int k = 0; k < 12; ++k) faces_out[12 * (size_t)f + k] = ok ? quad[k] : 0;           // a refused face: the caller raises
    }
}

// grid: one workgroup per image
__global__ __launch_bounds__(FINAL_THREADS) void sd_final_kernel(const long long* __restrict__ v_off, const long long* __restrict__ f_off, int F,
                                                                 Scratch s, long long* __restrict__ counts) {
    __shared__ int tally[4];                                // sharp edges, fixed old vertices, isolated, degree_max
    const int b = blockIdx.x, B = gridDim.x;
    if (threadIdx.x < 4) tally[threadIdx.x] = 0;
    __syncthreads();
    int sharp = 0, fixed = 0, isolated = 0, top = 0;
    if (F > 0)
        for (long long h = 3 * f_off[b] + threadIdx.x; h < 3 * f_off[b + 1]; h += FINAL_THREADS) {
            const int at = s.hslot[h];
            sharp += at >= 0 && s.owner[at] == h && s.count[at] != 2;
        }
    for (long long i = v_off[b] + threadIdx.x; i < v_off[b + 1]; i += FINAL_THREADS) {
        const int d = s.row[i + 1] - s.row[i];
        fixed += s.fixed[i] != 0, isolated += d == 0, top = d > top ? d : top;
    }
    if (sharp) atomicAdd(tally, sharp);
    if (fixed) atomicAdd(tally + 1, fixed);
    if (isolated) atomicAdd(tally + 2, isolated);
    if (top) atomicMax(tally + 3, top);
    __syncthreads();
    if (threadIdx.x == 0) {
        const long long edges = s.rank[3 * f_off[b + 1]] - s.rank[3 * f_off[b]];
        counts[(size_t)VERTICES_OUT * B + b] = v_off[b + 1] - v_off[b] + edges;
        counts[(size_t)EDGES * B + b] = edges;
        counts[(size_t)SHARP_EDGES * B + b] = tally[0];
        counts[(size_t)FIXED_VERTICES * B + b] = (long long)tally[1] + tally[0];
        counts[(size_t)ISOLATED * B + b] = tally[2];
        counts[(size_t)DEGREE_MAX * B + b] = tally[3];
    }
}

// one thread per vertex: v' = v - clamp(scale f g / |g|^2), fp32, every operation rounded once
__global__ __launch_bounds__(THREADS) void sd_project_kernel(const float* __restrict__ verts, const float* __restrict__ sdf,
                                                             const float* __restrict__ grad, const unsigned char* __restrict__ fixed, int V,
                                                             float scale, float max_step, float* __restrict__ verts_out) {
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < V; i += gridDim.x * THREADS) {
        const size_t at = 3 * (size_t)i;
        const float v[3] = {verts[at], verts[at + 1], verts[at + 2]}, g[3] = {grad[at], grad[at + 1], grad[at + 2]};
        const float f = sdf[i];
        const float g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
        float out[3] = {v[0], v[1], v[2]};
        if (!fixed[i] && sc_mesh::finite(f) && sc_mesh::finite(g2) && !(g2 < 1e-12f)) {
            const float t = __fdiv_rn(f, g2);
            float d[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float tg = t * g[c];
                d[c] = tg * scale;
            }
            // sqrtf is the correctly rounded one (hipcc's default); __fsqrt_rn is not, see emd3d.hip
            const float l = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            if (sc_mesh::finite(l)) {
                if (l > max_step) {
                    const float r = __fdiv_rn(max_step, l);
#pragma unroll
                    for (int c = 0; c < 3; ++c) d[c] = d[c] * r;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) out[c] = v[c] - d[c];
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) verts_out[at + c] = out[c];
    }
}

using sc_mesh::align16;
static inline bool sizes_ok(int n_images, long long n_verts, long long n_faces, long long table_slots) {
    return n_images >= 1 && n_images <= MAX_IMAGES && n_verts >= 0 && n_verts <= MAX_VERTS && n_faces >= 0 && n_faces <= MAX_FACES &&
           sc_mesh::slots_ok(table_slots, n_faces);
}
constexpr auto blocks = sc_mesh::blocks<THREADS, MAX_BLOCKS>;

}  // namespace sd
}  // namespace sc

// scratch layout: keys [T] u64 | count, owner, omin, omax [T] | deg, cursor, fixed [V] | row [V + 1] | raw, nbr [6 F] | hslot [3 F] |
// rank [3 F + 1]
extern "C" long long sc_mesh_subdivide_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots) {
    using namespace sc::sd;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots)) return 0;
    const long long T = table_slots, F = n_faces, V = n_verts;
    return align16(8 * T) + 4 * align16(4 * T) + 3 * align16(4 * V) + align16(4 * (V + 1)) + 2 * align16(24 * F) + align16(12 * F) +
           align16(4 * (3 * F + 1)) + 16;
}

extern "C" int sc_mesh_subdivide(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images,
                                 int n_verts, int n_faces, int table_slots, void* scratch, float* verts_out, int32_t* faces_out,
                                 uint8_t* fixed_out, int64_t* counts, int32_t* bad_vertex, int32_t* bad_index, int32_t* bad_face,
                                 void* stream_) {
    using namespace sc::sd;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots) || !v_off || !f_off || !counts || !bad_vertex || !bad_index || !bad_face ||
        !scratch || ((uintptr_t)scratch & 15) || (n_verts > 0 && !verts) || (n_verts + n_faces > 0 && (!verts_out || !fixed_out)) ||
        (n_faces > 0 && (!faces || !faces_out)))
        return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = n_images, V = n_verts, F = n_faces, T = table_slots;
    const int shift = sc_mesh::table_shift(T);
    sc_mesh::Carver ws{(char*)scratch};
    Scratch s;
    ws.take(s.keys, T);
    ws.take(s.count, T), ws.take(s.owner, T), ws.take(s.omin, T), ws.take(s.omax, T);
    ws.take(s.deg, V), ws.take(s.cursor, V), ws.take(s.fixed, V);
    ws.take(s.row, V + 1LL);
    ws.take(s.raw, 6LL * F), ws.take(s.nbr, 6LL * F);
    ws.take(s.hslot, 3LL * F);
    ws.take(s.rank, 3LL * F + 1);
    const long long *vo = (const long long*)v_off, *fo = (const long long*)f_off;
    hipLaunchKernelGGL(sd_init_kernel, dim3(blocks(T > V ? T : V)), dim3(THREADS), 0, stream, s, T, V, bad_vertex, bad_index, bad_face);
    if (F > 0) {
        hipLaunchKernelGGL(sd_insert_kernel, dim3(blocks(F)), dim3(THREADS), 0, stream, faces, vo, fo, B, F, s, T, shift, bad_index, bad_face);
        hipLaunchKernelGGL(sd_owner_kernel, dim3(blocks(3LL * F)), dim3(THREADS), 0, stream, s, 3 * F);
    }
    hipLaunchKernelGGL(sd_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, s, V, 3 * F);
    if (F > 0) hipLaunchKernelGGL(sd_fill_kernel, dim3(blocks(T)), dim3(THREADS), 0, stream, s, T);
    if (V > 0) hipLaunchKernelGGL(sd_rows_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, verts, s, V, bad_vertex);
    if (V + F > 0)
        hipLaunchKernelGGL(sd_emit_kernel, dim3(blocks(3LL * F > V ? 3LL * F : V)), dim3(THREADS), 0, stream, verts, faces, vo, fo, B, V, F, s,
                           verts_out, faces_out, fixed_out);
    hipLaunchKernelGGL(sd_final_kernel, dim3((unsigned)B), dim3(FINAL_THREADS), 0, stream, vo, fo, F, s, (long long*)counts);
    return (int)hipGetLastError();
}

extern "C" int sc_mesh_project_step(const float* verts, const float* sdf, const float* grad, const uint8_t* fixed, int n_verts, float scale,
                                    float max_step, float* verts_out, void* stream_) {
    using namespace sc::sd;
    if (n_verts == 0) return 0;
    if (n_verts < 0 || n_verts > MAX_VERTS || !verts || !sdf || !grad || !fixed || !verts_out) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sd_project_kernel, dim3(blocks(n_verts)), dim3(THREADS), 0, (hipStream_t)stream_, verts, sdf, grad, fixed, n_verts, scale,
                       max_step, verts_out);
    return (int)hipGetLastError();
}
