// mesh_intersect.hip -- how many pairs of faces of a mesh properly cross (ops.mesh_self_intersections; the evaluation's --mesh.self_intersect).
// include/shapeclipper_hip.h states the rule of one pair one rounding at a time ("sc_mesh_self_intersections"); tests/mesh_intersect_ref.py
// restates it in numpy.  Built without contraction.
//
// A pair (A, B), A the lower-numbered face, is a HIT by the strict rule of the header: a filtered float64 orientation sign (mi_sign3: zero
// unless it is the sign of the exact determinant), an edge PIERCES a triangle when its ends lie strictly on both sides of the plane and
// the edge passes strictly inside all three sides.  Faces that share two or three indices are never a pair, faces that share one test the
// two edges opposite it, a face that repeats an index takes no part.  A hit implies that the closed fp32 boxes overlap (a non-zero sign is
// exact, so every hit is a true crossing), so the box test that precedes every pair test loses nothing, and counting the pairs that pass
// it (box_pairs) depends on the mesh alone.
// Every pair is owned by its LOWER-numbered face and tested once.  Two ways to get there, the same integers:
//   * brute (mi_brute_kernel): a thread per face; the workgroup stages 256 higher-numbered faces of the image at a time in LDS, as
//     pm_brute_kernel does.  Also the path of an image whose grid is invalid.
//   * grid: the triangle grid of triangle_grid.hpp (steps 0 to 5 of point_mesh.hip).  A face that is not on its image's large list is
//     walked by its own thread (mi_walk_kernel): the references of the cells of its padded box, and the higher-numbered faces of the large
//     list.  Two boxes that overlap share the point p = component-wise max of their minima, a coordinate of both on every axis, so both
//     are referenced from cell(p) (axis_cell_far is monotone): the pair is tested in THAT cell only, by the lower-numbered of the two.
//     The box overlap is a closed comparison of raw fp32 coordinates: exact, no slack.  A face on the large list is walked by a wave
//     (mi_large_kernel) against all higher-numbered faces of its image, on the list or not.
// hits and the counters by integer atomicAdd, partner by atomicMin, per-thread partial counts in registers: the same bits from run to run,
// for any batch, stream and face order.  One stream, no wait on another workgroup, no host read.
// Bound: float64 vector arithmetic (about 50 operations a sign, up to 24 signs a pair) and dependent 16-byte gathers; one thread per face.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "shapeclipper_hip.h"
#include "triangle_grid.hpp"

#pragma clang fp contract(off)

namespace sc_mi {

using namespace sc_tgrid;

constexpr int LARGE_WAVES = 1024;     // waves that share the large faces of the batch, grid-stride

struct Tri {
    float v[3][3];
    int i[3];
};

// ---- the rule: include/shapeclipper_hip.h, "sign of a point against a plane" ------------------------------------------------------------
// (not inlined: a pair test holds up to 24 of these, and one copy of the float64 expression keeps the walks' register count down)
__device__ __noinline__ int mi_sign3_scalars(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz,
                                             float dx, float dy, float dz) {
    const double adx = (double)ax - (double)dx, ady = (double)ay - (double)dy, adz = (double)az - (double)dz;
    const double bdx = (double)bx - (double)dx, bdy = (double)by - (double)dy, bdz = (double)bz - (double)dz;
    const double cdx = (double)cx - (double)dx, cdy = (double)cy - (double)dy, cdz = (double)cz - (double)dz;
    const double m1 = bdx * cdy, m2 = bdy * cdx, m3 = cdx * ady, m4 = cdy * adx, m5 = adx * bdy, m6 = ady * bdx;
    const double det = (adz * (m1 - m2) + bdz * (m3 - m4)) + cdz * (m5 - m6);
    const double perm = ((fabs(m1) + fabs(m2)) * fabs(adz) + (fabs(m3) + fabs(m4)) * fabs(bdz)) + (fabs(m5) + fabs(m6)) * fabs(cdz);
    if (fabs(det) <= 0x1p-49 * perm) return 0;
    return det > 0.0 ? 1 : -1;
}
__device__ __forceinline__ int mi_sign3(const float a[3], const float b[3], const float c[3], const float d[3]) {
    return mi_sign3_scalars(a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], d[0], d[1], d[2]);
}

// segment p q, whose ends have the signs sp, sq against the plane of t, against the triangle t
__device__ __forceinline__ bool mi_pierces(const float p[3], const float q[3], int sp, int sq, const Tri& t) {
    if (sp * sq != -1) return false;
    const int s0 = mi_sign3(p, q, t.v[0], t.v[1]);
    if (s0 == 0) return false;
    if (mi_sign3(p, q, t.v[1], t.v[2]) != s0) return false;
    return mi_sign3(p, q, t.v[2], t.v[0]) == s0;
}

// the edge of t opposite its corner s: (v[s + 1], v[s + 2]), corners counted modulo 3 (selects, so that t stays in registers)
__device__ __forceinline__ void mi_opposite(const Tri& t, int s, float p[3], float q[3]) {
    for (int d = 0; d < 3; ++d) {
        p[d] = s == 0 ? t.v[1][d] : (s == 1 ? t.v[2][d] : t.v[0][d]);
        q[d] = s == 0 ? t.v[2][d] : (s == 1 ? t.v[0][d] : t.v[1][d]);
    }
}

// 0: not a pair (two or three shared indices); 1: a pair, no hit; 2: a hit without a shared vertex; 3: a hit with one.
// A is the lower-numbered face; neither repeats an index.
__device__ __forceinline__ int mi_pair(const Tri& A, const Tri& B) {
    int shared = 0, sa = 0, sb = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            if (A.i[i] == B.i[j]) { ++shared; sa = i; sb = j; }
    if (shared >= 2) return 0;
    if (shared == 1) {
        float p[3], q[3];
        mi_opposite(A, sa, p, q);
        if (mi_pierces(p, q, mi_sign3(B.v[0], B.v[1], B.v[2], p), mi_sign3(B.v[0], B.v[1], B.v[2], q), B)) return 3;
        mi_opposite(B, sb, p, q);
        return mi_pierces(p, q, mi_sign3(A.v[0], A.v[1], A.v[2], p), mi_sign3(A.v[0], A.v[1], A.v[2], q), A) ? 3 : 1;
    }
    int ab[3], ba[3];                  // A's vertices against B's plane, B's against A's
    for (int i = 0; i < 3; ++i) ab[i] = mi_sign3(B.v[0], B.v[1], B.v[2], A.v[i]);
    // all of A strictly on one side of B's plane: no edge of A crosses it, and no point of A lies where an edge of B could pass
    if (ab[0] != 0 && ab[0] == ab[1] && ab[1] == ab[2]) return 1;
    for (int i = 0; i < 3; ++i) ba[i] = mi_sign3(A.v[0], A.v[1], A.v[2], B.v[i]);
    if (ba[0] != 0 && ba[0] == ba[1] && ba[1] == ba[2]) return 1;
    for (int e = 0; e < 3; ++e)
        if (mi_pierces(A.v[e], A.v[(e + 1) % 3], ab[e], ab[(e + 1) % 3], B)) return 2;
    for (int e = 0; e < 3; ++e)
        if (mi_pierces(B.v[e], B.v[(e + 1) % 3], ba[e], ba[(e + 1) % 3], A)) return 2;
    return 1;
}

__device__ __forceinline__ bool mi_repeats(const int i[3]) { return i[0] == i[1] || i[1] == i[2] || i[0] == i[2]; }

// closed overlap of the boxes of two triangles, raw fp32 coordinates
__device__ __forceinline__ bool mi_boxes_meet(const float amn[3], const float amx[3], const float bmn[3], const float bmx[3]) {
    return amn[0] <= bmx[0] && bmn[0] <= amx[0] && amn[1] <= bmx[1] && bmn[1] <= amx[1] && amn[2] <= bmx[2] && bmn[2] <= amx[2];
}
__device__ __forceinline__ void mi_box(const Tri& t, float mn[3], float mx[3]) {
    for (int i = 0; i < 3; ++i) {
        mn[i] = fminf(t.v[0][i], fminf(t.v[1][i], t.v[2][i]));
        mx[i] = fmaxf(t.v[0][i], fmaxf(t.v[1][i], t.v[2][i]));
    }
}

struct Tally {                          // a thread's partial counts of one image
    unsigned long long pairs, pairs_vertex, box_pairs;
};

// the pair (A = local face la, B = local face lb > la) whose boxes meet: test it and book the outcome
__device__ __forceinline__ void mi_book(const Tri& A, const Tri& B, int la, int lb, int f0, Tally& t, int32_t* __restrict__ hits,
                                        int32_t* __restrict__ partner) {
    const int r = mi_pair(A, B);
    if (r == 0) return;
    ++t.box_pairs;
    if (r == 1) return;
    ++t.pairs;
    if (r == 3) ++t.pairs_vertex;
    atomicAdd(&hits[f0 + la], 1);
    atomicAdd(&hits[f0 + lb], 1);
    atomicMin((unsigned*)&partner[f0 + la], (unsigned)lb);          // -1, "none", is the largest unsigned
    atomicMin((unsigned*)&partner[f0 + lb], (unsigned)la);
}
__device__ __forceinline__ void mi_flush(const Tally& t, int b, int n_images, unsigned long long* __restrict__ counts) {
    if (t.pairs) atomicAdd(&counts[b], t.pairs);
    if (t.pairs_vertex) atomicAdd(&counts[(size_t)n_images + b], t.pairs_vertex);
    if (t.box_pairs) atomicAdd(&counts[2 * (size_t)n_images + b], t.box_pairs);
}

// ---- outputs and flags -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void mi_init_kernel(int n_images, int v_total, int f_total, const float* __restrict__ verts,
                                                          const int32_t* __restrict__ faces, const int* __restrict__ v_start,
                                                          const int* __restrict__ f_start, int32_t* __restrict__ hits,
                                                          int32_t* __restrict__ partner, int32_t* __restrict__ face_counts,
                                                          int32_t* __restrict__ flags) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k < v_total) {
        const float x = verts[(size_t)k * 3 + 0], y = verts[(size_t)k * 3 + 1], z = verts[(size_t)k * 3 + 2];
        if (!(fabsf(x) < HUGE_COORD) || !(fabsf(y) < HUGE_COORD) || !(fabsf(z) < HUGE_COORD)) flags[0] = 1;
    }
    if (k < f_total) {
        hits[k] = 0;
        partner[k] = -1;
        if (k < f_start[n_images]) {
            const int b = image_of(k, f_start, n_images), nv = v_start[b + 1] - v_start[b];
            const int i[3] = {faces[(size_t)k * 3 + 0], faces[(size_t)k * 3 + 1], faces[(size_t)k * 3 + 2]};
            if (i[0] < 0 || i[0] >= nv || i[1] < 0 || i[1] >= nv || i[2] < 0 || i[2] >= nv) flags[1] = 1;
            else if (mi_repeats(i)) atomicAdd(&face_counts[(size_t)n_images + b], 1);
        }
    }
}

__global__ __launch_bounds__(THREADS) void mi_final_kernel(int n_images, int f_total, const int* __restrict__ f_start,
                                                           const int32_t* __restrict__ hits, int32_t* __restrict__ face_counts) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= f_total || k >= f_start[n_images]) return;
    if (hits[k] > 0) atomicAdd(&face_counts[image_of(k, f_start, n_images)], 1);
}

// ---- all pairs ---------------------------------------------------------------------------------------------------------------------------
// A thread per packed face; the workgroup's 256 faces may belong to several images, which it takes one after the other.
// ONLY_INVALID: only the images whose grid is invalid (the grid search's fallback).
template <bool ONLY_INVALID>
__global__ __launch_bounds__(THREADS) void mi_brute_kernel(int n_images, int f_total, const float* __restrict__ verts,
                                                           const int32_t* __restrict__ faces, const int* __restrict__ v_start,
                                                           const int* __restrict__ f_start, const Meta* __restrict__ meta,
                                                           unsigned long long* __restrict__ counts, int32_t* __restrict__ hits,
                                                           int32_t* __restrict__ partner) {
    __shared__ float tv[THREADS][9];
    __shared__ int ti[THREADS][3];
    __shared__ int tok[THREADS];
    const int tid = threadIdx.x, k0 = blockIdx.x * THREADS;
    const int n_faces = min(f_total, f_start[n_images]);
    if (k0 >= n_faces) return;                                          // uniform for the workgroup
    const int kend = min(k0 + THREADS, n_faces);
    const int k = k0 + tid;
    const bool in = k < kend;
    const int mine = in ? image_of(k, f_start, n_images) : -1;
    Tri A;
    bool active = false;
    if (in) {
        for (int i = 0; i < 3; ++i) A.i[i] = faces[(size_t)k * 3 + i];
        active = load_face(k, mine, verts, faces, v_start, A.v[0], A.v[1], A.v[2]) && !mi_repeats(A.i);
    }
    float amn[3], amx[3];
    if (active) mi_box(A, amn, amx);
    const int la = in ? k - f_start[mine] : 0;
    Tally t = {0, 0, 0};
    const int b_first = image_of(k0, f_start, n_images), b_last = image_of(kend - 1, f_start, n_images);
    for (int b = b_first; b <= b_last; ++b) {                           // uniform
        if (ONLY_INVALID && meta[b].valid) continue;
        const int f0 = f_start[b], nf = f_start[b + 1] - f0;
        const int low = max(k0, f0) - f0;                               // the workgroup's lowest face of this image: partners lie above
        for (int x0 = low + 1; x0 < nf; x0 += THREADS) {
            const int chunk = min(THREADS, nf - x0);
            __syncthreads();
            if (tid < chunk) {
                float a[3], bb[3], c[3];
                const int kk = f0 + x0 + tid;
                const int i[3] = {faces[(size_t)kk * 3 + 0], faces[(size_t)kk * 3 + 1], faces[(size_t)kk * 3 + 2]};
                const bool ok = load_face(kk, b, verts, faces, v_start, a, bb, c) && !mi_repeats(i);
                tok[tid] = ok ? 1 : 0;
                if (ok)
                    for (int d = 0; d < 3; ++d) { tv[tid][d] = a[d]; tv[tid][3 + d] = bb[d]; tv[tid][6 + d] = c[d]; ti[tid][d] = i[d]; }
            }
            __syncthreads();
            if (!active || mine != b) continue;                         // (the barriers above are met by every thread)
            for (int s = max(0, la + 1 - x0); s < chunk; ++s) {
                if (!tok[s]) continue;
                Tri B;
                for (int d = 0; d < 3; ++d) { B.v[0][d] = tv[s][d]; B.v[1][d] = tv[s][3 + d]; B.v[2][d] = tv[s][6 + d]; B.i[d] = ti[s][d]; }
                float bmn[3], bmx[3];
                mi_box(B, bmn, bmx);
                if (mi_boxes_meet(amn, amx, bmn, bmx)) mi_book(A, B, la, x0 + s, f0, t, hits, partner);
            }
        }
    }
    if (active) mi_flush(t, mine, n_images, counts);
}

// ---- the grid walk -----------------------------------------------------------------------------------------------------------------------
// local face `local` of the image whose faces start at f0: false for a face with an index out of range or a repeated index
__device__ __forceinline__ bool mi_load_packed(const float4* __restrict__ tris, const int32_t* __restrict__ faces, int f0, int local, Tri& t) {
    const size_t k = (size_t)(f0 + local);
    const float4 a = tris[k * 3 + 0];
    if (a.w == 0.f) return false;
    const float4 b = tris[k * 3 + 1], c = tris[k * 3 + 2];
    t.v[0][0] = a.x; t.v[0][1] = a.y; t.v[0][2] = a.z;
    t.v[1][0] = b.x; t.v[1][1] = b.y; t.v[1][2] = b.z;
    t.v[2][0] = c.x; t.v[2][1] = c.y; t.v[2][2] = c.z;
    for (int i = 0; i < 3; ++i) t.i[i] = faces[k * 3 + i];
    return !mi_repeats(t.i);
}

__global__ __launch_bounds__(THREADS) void mi_walk_kernel(int n_images, int f_total, const int32_t* __restrict__ faces,
                                                          const int* __restrict__ f_start, const Meta* __restrict__ meta,
                                                          const int* __restrict__ start, const int* __restrict__ refs,
                                                          const float4* __restrict__ tris, const int* __restrict__ large,
                                                          const int* __restrict__ large_count, unsigned long long* __restrict__ counts,
                                                          int32_t* __restrict__ hits, int32_t* __restrict__ partner) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= f_total || k >= f_start[n_images]) return;
    const int b = image_of(k, f_start, n_images);
    const Meta g = meta[b];
    if (!g.valid) return;                                               // the all-pairs twin answers this image
    const int f0 = f_start[b], la = k - f0;
    Tri A;
    if (!mi_load_packed(tris, faces, f0, la, A)) return;
    float amn[3], amx[3];
    mi_box(A, amn, amx);
    int c0[3], c1[3];
    if (face_cells(g, amn, amx, c0, c1) > CELL_CAP) return;             // on the large list: a wave walks it
    Tally t = {0, 0, 0};
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const int cell = g.cbase + (z * g.g[1] + y) * g.g[0] + x;
                const int sb = start[cell], se = start[cell + 1];
                for (int r = sb; r < se; ++r) {
                    const int lb = refs[r];
                    if (lb <= la) continue;                             // the lower-numbered face owns the pair
                    Tri B;
                    if (!mi_load_packed(tris, faces, f0, lb, B)) continue;
                    float bmn[3], bmx[3];
                    mi_box(B, bmn, bmx);
                    if (!mi_boxes_meet(amn, amx, bmn, bmx)) continue;
                    // the one cell the pair is tested in: that of the component-wise maximum of the two box minima
                    if (sc_grid::axis_cell_far(fmaxf(amn[0], bmn[0]), g.lo[0], g.inv_h[0], g.g[0]) != x ||
                        sc_grid::axis_cell_far(fmaxf(amn[1], bmn[1]), g.lo[1], g.inv_h[1], g.g[1]) != y ||
                        sc_grid::axis_cell_far(fmaxf(amn[2], bmn[2]), g.lo[2], g.inv_h[2], g.g[2]) != z)
                        continue;
                    mi_book(A, B, la, lb, f0, t, hits, partner);
                }
            }
    const int nl = large_count[b];
    for (int i = 0; i < nl; ++i) {
        const int lb = large[f0 + i];
        if (lb <= la) continue;                                         // that face's wave owns the pair
        Tri B;
        if (!mi_load_packed(tris, faces, f0, lb, B)) continue;
        float bmn[3], bmx[3];
        mi_box(B, bmn, bmx);
        if (mi_boxes_meet(amn, amx, bmn, bmx)) mi_book(A, B, la, lb, f0, t, hits, partner);
    }
    mi_flush(t, b, n_images, counts);
}

// a wave per face of the large lists, against every higher-numbered face of its image
__global__ __launch_bounds__(THREADS) void mi_large_kernel(int n_images, const int32_t* __restrict__ faces, const int* __restrict__ f_start,
                                                           const float4* __restrict__ tris, const int* __restrict__ large,
                                                           const int* __restrict__ large_count, unsigned long long* __restrict__ counts,
                                                           int32_t* __restrict__ hits, int32_t* __restrict__ partner) {
    const int lane = threadIdx.x & 63, wave = (blockIdx.x * THREADS + threadIdx.x) >> 6, n_waves = (gridDim.x * THREADS) >> 6;
    for (int b = 0; b < n_images; ++b) {
        const int nl = large_count[b];
        if (nl == 0) continue;
        const int f0 = f_start[b], nf = f_start[b + 1] - f0;
        Tally t = {0, 0, 0};
        for (int i = wave; i < nl; i += n_waves) {
            const int la = large[f0 + i];
            Tri A;
            if (!mi_load_packed(tris, faces, f0, la, A)) continue;     // uniform for the wave
            float amn[3], amx[3];
            mi_box(A, amn, amx);
            for (int lb = la + 1 + lane; lb < nf; lb += 64) {
                Tri B;
                if (!mi_load_packed(tris, faces, f0, lb, B)) continue;
                float bmn[3], bmx[3];
                mi_box(B, bmn, bmx);
                if (mi_boxes_meet(amn, amx, bmn, bmx)) mi_book(A, B, la, lb, f0, t, hits, partner);
            }
        }
        mi_flush(t, b, n_images, counts);
    }
}

// workspace, in 4-byte words: the grid's regions only
struct Workspace : sc_tgrid::Carve {
    size_t cleared, total;
};
inline Workspace carve(int b, int f_total) {
    Workspace c;
    sc_grid::WordCarver w;
    carve_cleared(w, b, f_total, c);
    c.cleared = w.words;
    carve_rest(w, b, f_total, c);
    c.total = w.words;
    return c;
}

inline bool refused(int b, int v_total, int f_total) { return b > MAX_IMAGES || v_total < 0 || f_total < 0 || f_total > MAX_FACES; }

}  // namespace sc_mi

extern "C" {

// See include/shapeclipper_hip.h for the contract.
long long sc_mesh_self_intersections_scratch_bytes(int n_images, int n_verts, int n_faces) {
    if (n_images <= 0) return 0;
    if (sc_mi::refused(n_images, n_verts, n_faces)) return -1;
    return (long long)(sc_mi::carve(n_images, n_faces).total * sizeof(int));
}

int sc_mesh_self_intersections(const float* verts, const int32_t* faces, const int32_t* v_count, const int32_t* f_count, int n_images,
                               int n_verts, int n_faces, int brute, void* scratch, long long* counts, int32_t* face_counts,
                               int32_t* hits, int32_t* partner, int32_t* flags, void* stream_) {
    using namespace sc_mi;
    hipStream_t stream = (hipStream_t)stream_;
    if (n_images <= 0) return 0;
    if (refused(n_images, n_verts, n_faces) || !v_count || !f_count || !scratch || !counts || !face_counts || !flags ||
        (n_verts > 0 && !verts) || (n_faces > 0 && (!faces || !hits || !partner)) || ((uintptr_t)scratch & 15))
        return (int)hipErrorInvalidValue;
    const Workspace c = carve(n_images, n_faces);
    int* ws = (int*)scratch;
    int *v_start = ws + c.v_start, *f_start = ws + c.f_start;
    unsigned long long* counts_u = (unsigned long long*)counts;
    (void)hipMemsetAsync(counts, 0, 3 * (size_t)n_images * sizeof(long long), stream);
    (void)hipMemsetAsync(face_counts, 0, 2 * (size_t)n_images * sizeof(int32_t), stream);
    (void)hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), stream);
    const int face_blocks = (n_faces + THREADS - 1) / THREADS;
    const int init_blocks = ((n_faces > n_verts ? n_faces : n_verts) + THREADS - 1) / THREADS;
    const bool grid = !brute && n_faces > 0;
    if (grid) {
        (void)hipMemsetAsync(ws, 0, c.cleared * sizeof(int), stream);
        build(ws, c, verts, faces, v_count, f_count, n_images, n_verts, n_faces, stream);
    } else {
        hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, stream, n_images, v_count, f_count, n_verts, n_faces, v_start, f_start);
    }
    if (init_blocks > 0)
        hipLaunchKernelGGL(mi_init_kernel, dim3(init_blocks), dim3(THREADS), 0, stream, n_images, n_verts, n_faces, verts, faces, v_start,
                           f_start, hits, partner, face_counts, flags);
    if (n_faces > 0) {
        const Meta* meta = (const Meta*)(ws + c.meta);
        if (grid) {
            const float4* tris = (const float4*)(ws + c.tris);
            hipLaunchKernelGGL(mi_walk_kernel, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, n_faces, faces, f_start, meta,
                               ws + c.counts, ws + c.refs, tris, ws + c.large, ws + c.large_count, counts_u, hits, partner);
            hipLaunchKernelGGL(mi_large_kernel, dim3(LARGE_WAVES * 64 / THREADS), dim3(THREADS), 0, stream, n_images, faces, f_start, tris,
                               ws + c.large, ws + c.large_count, counts_u, hits, partner);
            hipLaunchKernelGGL(mi_brute_kernel<true>, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, n_faces, verts, faces, v_start,
                               f_start, meta, counts_u, hits, partner);
        } else {
            hipLaunchKernelGGL(mi_brute_kernel<false>, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, n_faces, verts, faces, v_start,
                               f_start, meta, counts_u, hits, partner);
        }
        hipLaunchKernelGGL(mi_final_kernel, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, n_faces, f_start, hits, face_counts);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
