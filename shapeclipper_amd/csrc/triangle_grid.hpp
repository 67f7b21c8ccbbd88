// triangle_grid.hpp -- the uniform grid of TRIANGLES the exact mesh searches bin a batch of packed meshes into before they walk it
// (point_mesh.hip: the rings around a query point; mesh_intersect.hip: the cells of a face's own box).  The triangle counterpart of the
// point binning of uniform_grid.hpp, on that header's box, geometry and cell of a coordinate; what the walks may lean on:
//   * a triangle is referenced from every cell its AABB, padded by Geometry.slack, overlaps (face_cells): count pass, exclusive scan,
//     fill pass (integer atomics; the order inside a cell is arbitrary).  axis_cell_far is monotone in the coordinate, so a triangle
//     whose closed box holds the coordinate x on every axis is referenced from cell(x);
//   * the cell side is max(2 x mean AABB extent, cbrt(volume / F)), grown until the grid has at most 2 F + 64 cells, so a typical
//     triangle overlaps at most 2 x 2 x 2 cells.  A triangle that overlaps more than CELL_CAP cells (one huge triangle across the box)
//     goes on its image's "large" list instead: the references never exceed CELL_CAP x F whatever the mesh, so the workspace has a FIXED
//     capacity and nothing is read back to the host;
//   * a face with an index outside its image's vertex range is never dereferenced: its gathered triangle carries w == 0 and it is in
//     no cell and on no list.  An image whose grid is invalid (a non-finite or huge vertex, a mesh of zero extent, no valid face) has
//     no reference and no large face at all: the includer answers it by its all-pairs twin.
// Every __global__ below sits in an anonymous namespace, as in uniform_grid.hpp: each including object carries, and launches, its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.hpp"
#include "uniform_grid.hpp"

namespace sc_tgrid {

constexpr int THREADS = 256;
constexpr int GMAX = 128;             // cells per axis
constexpr int CELL_CAP = 16;          // cells a triangle may be referenced from; more: the image's large list
constexpr int MAX_IMAGES = 65535;
constexpr int MAX_FACES = 1 << 26;    // CELL_CAP * f_total stays below 2^31
constexpr float HUGE_COORD = 1.0e15f; // magnitudes the padding / slack arithmetic is not made for

struct Meta : sc_grid::Geometry {     // one per image; valid: finite vertices of sensible magnitude, a box of positive extent
    int cbase;                        // first cell of the image in the packed cell arrays
};

// image of packed face k: the last b with f_start[b] <= k (k < f_start[n_images])
__device__ __forceinline__ int image_of(int k, const int* __restrict__ f_start, int n_images) {
    int lo = 0, hi = n_images;                          // invariant: f_start[lo] <= k < f_start[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (f_start[mid] <= k) lo = mid; else hi = mid;
    }
    return lo;
}

// the vertices of packed face k of image b, or false when an index is outside [0, v_count[b])
__device__ __forceinline__ bool load_face(int k, int b, const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                          const int* __restrict__ v_start, float a[3], float bb[3], float c[3]) {
    const int v0 = v_start[b], nv = v_start[b + 1] - v0;
    const int i0 = faces[(size_t)k * 3 + 0], i1 = faces[(size_t)k * 3 + 1], i2 = faces[(size_t)k * 3 + 2];
    if (i0 < 0 || i0 >= nv || i1 < 0 || i1 >= nv || i2 < 0 || i2 >= nv) return false;
    for (int i = 0; i < 3; ++i) {
        a[i] = verts[(size_t)(v0 + i0) * 3 + i]; bb[i] = verts[(size_t)(v0 + i1) * 3 + i]; c[i] = verts[(size_t)(v0 + i2) * 3 + i];
    }
    return true;
}

// the lanes of a wave whose `ok` is set: all of one image -> the first such lane (it issues the wave's atomics after a reduction);
// of several images -> -1 (every lane issues its own); none -> -2.  Every lane of the wave calls it.
__device__ __forceinline__ int wave_leader(bool ok, int b) {
    const unsigned long long m = __ballot(ok);
    if (!m) return -2;
    const int first = __builtin_ctzll(m);
    const int b0 = __shfl(b, first);
    return __all(!ok || b == b0) ? first : -1;
}

// the cells [c0, c1] per axis that the box [mn, mx] of a triangle, padded by the slack, overlaps; returns their number
__device__ __forceinline__ long long face_cells(const Meta& g, const float mn[3], const float mx[3], int c0[3], int c1[3]) {
    long long ncells = 1;
    for (int i = 0; i < 3; ++i) {
        c0[i] = sc_grid::axis_cell_far(mn[i] - g.slack, g.lo[i], g.inv_h[i], g.g[i]);
        c1[i] = sc_grid::axis_cell_far(mx[i] + g.slack, g.lo[i], g.inv_h[i], g.g[i]);
        ncells *= (c1[i] - c0[i] + 1);
    }
    return ncells;
}

namespace {

// ---- 0. the images' slices of the packed arrays: starts[0..B] of the vertices and of the faces, never past the packed lengths ----------
__global__ void offsets_kernel(int n_images, const int32_t* __restrict__ v_count, const int32_t* __restrict__ f_count, int v_total,
                               int f_total, int* __restrict__ v_start, int* __restrict__ f_start) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long v = 0, f = 0;
    for (int b = 0; b < n_images; ++b) {
        v_start[b] = (int)v; f_start[b] = (int)f;
        const int vc = v_count[b], fc = f_count[b];
        v += vc > 0 ? vc : 0; f += fc > 0 ? fc : 0;
        v = v < v_total ? v : v_total; f = f < f_total ? f : f_total;
    }
    v_start[n_images] = (int)v; f_start[n_images] = (int)f;
}

// ---- 1. bounding box of the valid triangles (the box of uniform_grid.hpp; its free word counts the valid faces) ------------------------------
__global__ __launch_bounds__(THREADS) void bbox_kernel(int n_images, int f_total, const float* __restrict__ verts,
                                                       const int32_t* __restrict__ faces, const int* __restrict__ v_start,
                                                       const int* __restrict__ f_start, unsigned* __restrict__ box_all,
                                                       float4* __restrict__ tris) {
    const int k = blockIdx.x * THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = k < f_total && k < f_start[n_images];
    const int b = in ? image_of(k, f_start, n_images) : 0;
    float a[3] = {0.f, 0.f, 0.f}, bb[3] = {0.f, 0.f, 0.f}, c[3] = {0.f, 0.f, 0.f};
    const bool ok = in && load_face(k, b, verts, faces, v_start, a, bb, c);
    if (in) {       // the gathered triangle, for the walk: w of the first vertex says whether the face is valid
        tris[(size_t)k * 3 + 0] = ok ? make_float4(a[0], a[1], a[2], 1.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        tris[(size_t)k * 3 + 1] = ok ? make_float4(bb[0], bb[1], bb[2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
        tris[(size_t)k * 3 + 2] = ok ? make_float4(c[0], c[1], c[2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float mn[3], mx[3];
    int bad = 0;
    for (int i = 0; i < 3; ++i) {
        bad |= ok && (!(fabsf(a[i]) < HUGE_COORD) || !(fabsf(bb[i]) < HUGE_COORD) || !(fabsf(c[i]) < HUGE_COORD));
        mn[i] = ok ? fminf(a[i], fminf(bb[i], c[i])) : __builtin_inff();
        mx[i] = ok ? fmaxf(a[i], fmaxf(bb[i], c[i])) : -__builtin_inff();
    }
    const int leader = wave_leader(ok, b);
    unsigned count = ok ? 1u : 0u;
    if (leader >= 0) {
        sc_grid::wave_minmax(mn, mx);
        bad = __any(bad);
        count = (unsigned)__builtin_popcountll(__ballot(ok));
    }
    if (ok && (leader == -1 || lane == leader)) {
        unsigned* box = box_all + (size_t)b * sc_grid::BOX_WORDS;
        sc_grid::box_merge(box, mn, mx, bad);
        atomicAdd(&box[sc_grid::BOX_USER], count);
    }
}

// ---- 2. sum of the triangles' largest AABB extents, in units of (largest box extent) / 65536, as a 64-bit integer ------------------------
__global__ __launch_bounds__(THREADS) void extent_kernel(int n_images, int f_total, const int* __restrict__ f_start,
                                                         const unsigned* __restrict__ box_all, const float4* __restrict__ tris,
                                                         unsigned long long* __restrict__ ext_sum) {
    const int k = blockIdx.x * THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = k < f_total && k < f_start[n_images];
    const float4 a = in ? tris[(size_t)k * 3 + 0] : make_float4(0.f, 0.f, 0.f, 0.f);
    bool ok = in && a.w != 0.f;
    const int b = ok ? image_of(k, f_start, n_images) : 0;
    unsigned q = 0;
    if (ok) {
        float lo[3], hi[3], emax = 0.f;
        const bool bad = sc_grid::box_read(box_all + (size_t)b * sc_grid::BOX_WORDS, lo, hi);
        for (int i = 0; i < 3; ++i) emax = fmaxf(emax, hi[i] - lo[i]);
        ok = !bad && emax > 0.f;
        if (ok) {
            const float4 bb = tris[(size_t)k * 3 + 1], c = tris[(size_t)k * 3 + 2];
            const float ex = fmaxf(a.x, fmaxf(bb.x, c.x)) - fminf(a.x, fminf(bb.x, c.x));
            const float ey = fmaxf(a.y, fmaxf(bb.y, c.y)) - fminf(a.y, fminf(bb.y, c.y));
            const float ez = fmaxf(a.z, fmaxf(bb.z, c.z)) - fminf(a.z, fminf(bb.z, c.z));
            const float e = fminf(fmaxf(ex, fmaxf(ey, ez)) / emax * 65536.f, 65536.f);
            q = (unsigned)(e >= 0.f ? e : 0.f);
        }
    }
    const int leader = wave_leader(ok, b);
    if (leader >= 0)
        for (int d = 32; d >= 1; d >>= 1) q += __shfl_xor(q, d);
    if (ok && (leader == -1 || lane == leader)) atomicAdd(&ext_sum[b], (unsigned long long)q);
}

// ---- 3. grid geometry of every image, then the images' first cells -----------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void meta_kernel(int n_images, const unsigned* __restrict__ box_all,
                                                       const unsigned long long* __restrict__ ext_sum, Meta* __restrict__ meta) {
    for (int b = threadIdx.x; b < n_images; b += THREADS) {
        const unsigned* box = box_all + (size_t)b * sc_grid::BOX_WORDS;
        const int nf = (int)box[sc_grid::BOX_USER];
        const float count = (float)(nf > 0 ? nf : 1), ext_units = (float)ext_sum[b];
        Meta g;
        // (24 growth rounds where the two point grids take 8: possibly drift between the copies; kept, the geometry is not to change)
        const float h = sc_grid::geometry_from_box(box, 2ll * nf + 64, GMAX, 24, [=](float vol, float emax) {
            const float mean_ext = emax * (ext_units / (65536.f * count));
            return fmaxf(2.f * mean_ext, cbrtf(vol / count));
        }, g);
        g.valid = (g.valid && nf > 0 && h > 0.f) ? 1 : 0;
        if (!g.valid) g.g[0] = g.g[1] = g.g[2] = 1;
        g.cbase = 0;
        meta[b] = g;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int base = 0;                                   // at most 2 F_b + 64 cells each: the sum fits the packed arrays (and an int)
        for (int b = 0; b < n_images; ++b) { meta[b].cbase = base; base += meta[b].g[0] * meta[b].g[1] * meta[b].g[2]; }
    }
}

// ---- 4. references: count pass (FILL = false; also builds the large lists) and fill pass (FILL = true) -----------------------------------
template <bool FILL>
__global__ __launch_bounds__(THREADS) void bin_kernel(int n_images, int f_total, const int* __restrict__ f_start,
                                                      const Meta* __restrict__ meta, const float4* __restrict__ tris,
                                                      int* __restrict__ counts, int* __restrict__ cursor, int* __restrict__ refs,
                                                      int* __restrict__ large, int* __restrict__ large_count) {
    const int k = blockIdx.x * THREADS + threadIdx.x;
    if (k >= f_total || k >= f_start[n_images]) return;
    const float4 a = tris[(size_t)k * 3 + 0];
    if (a.w == 0.f) return;
    const int b = image_of(k, f_start, n_images);
    const Meta& g = meta[b];
    if (!g.valid) return;
    const float4 bb = tris[(size_t)k * 3 + 1], c = tris[(size_t)k * 3 + 2];
    const float mn[3] = {fminf(a.x, fminf(bb.x, c.x)), fminf(a.y, fminf(bb.y, c.y)), fminf(a.z, fminf(bb.z, c.z))};
    const float mx[3] = {fmaxf(a.x, fmaxf(bb.x, c.x)), fmaxf(a.y, fmaxf(bb.y, c.y)), fmaxf(a.z, fmaxf(bb.z, c.z))};
    int c0[3], c1[3];
    const long long ncells = face_cells(g, mn, mx, c0, c1);
    const int local = k - f_start[b];
    if (ncells > CELL_CAP) {
        if (!FILL) large[f_start[b] + atomicAdd(&large_count[b], 1)] = local;      // at most F_b entries: the image's own slice
        return;
    }
    for (int z = c0[2]; z <= c1[2]; ++z)
        for (int y = c0[1]; y <= c1[1]; ++y)
            for (int x = c0[0]; x <= c1[0]; ++x) {
                const int cell = g.cbase + (z * g.g[1] + y) * g.g[0] + x;
                if (FILL) refs[counts[cell] + atomicAdd(&cursor[cell], 1)] = local;
                else atomicAdd(&counts[cell], 1);
            }
}

// ---- 5. exclusive scan of the packed histogram, in place, over [0, n): entry `cells` of the last image ends up holding the total ---------
__global__ __launch_bounds__(1024) void scan_local_kernel(int n, int* __restrict__ counts, int* __restrict__ block_tot) {
    __shared__ int wtot[16];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * 1024 + tid;
    const int v = i < n ? counts[i] : 0;
    int total;
    const int before = sc_scan::block_exclusive<16>(v, wtot, total);
    if (i < n) counts[i] = before;
    if (tid == 0) block_tot[blockIdx.x] = total;
}

// exclusive scan of the block totals, in place: one workgroup, 1,024 totals per round with a running carry
__global__ __launch_bounds__(1024) void scan_totals_kernel(int nblk, int* __restrict__ block_tot) {
    __shared__ int wtot[16];
    __shared__ int carry_s;
    const int tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += 1024) {
        const int i = base + tid;
        const int v = i < nblk ? block_tot[i] : 0;
        int total;
        const int before = sc_scan::block_exclusive<16>(v, wtot, total);      // the round's two barriers below free wtot for the next
        const int carry = carry_s;
        if (i < nblk) block_tot[i] = carry + before;
        __syncthreads();
        if (tid == 0) carry_s = carry + total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(1024) void scan_add_kernel(int n, int* __restrict__ counts, const int* __restrict__ block_tot) {
    const int i = blockIdx.x * 1024 + threadIdx.x;
    const int off = block_tot[blockIdx.x];
    if (i < n && off) counts[i] += off;
}

}  // namespace

// ---- the grid's regions of the includer's workspace, in 4-byte words ---------------------------------------------------------------------
// carve_cleared's regions are adjacent and must be zero before build(): the includer takes them, and what else it wants cleared, at the
// start of its workspace and clears all of it with ONE memset.
struct Carve {
    size_t box, ext_sum, large_count, counts, cursor;       // cleared
    size_t v_start, f_start, meta, block_tot, large, tris, refs;
    size_t n_cells, nblk;
};
inline void carve_cleared(sc_grid::WordCarver& w, int b, int f_total, Carve& c) {
    c.n_cells = 2 * (size_t)f_total + 64 * (size_t)b + 1;           // sum of the images' cell budgets, and the entry behind the last cell
    c.nblk = (c.n_cells + 1023) / 1024;
    c.box = w.take((size_t)b * sc_grid::BOX_WORDS);
    c.ext_sum = w.take((size_t)b * 2);
    c.large_count = w.take((size_t)b);
    c.counts = w.take(c.n_cells);
    c.cursor = w.take(c.n_cells);
}
inline void carve_rest(sc_grid::WordCarver& w, int b, int f_total, Carve& c) {
    c.v_start = w.take((size_t)b + 1);
    c.f_start = w.take((size_t)b + 1);
    c.meta = w.take((size_t)b * (sizeof(Meta) / 4));
    c.block_tot = w.take(c.nblk);
    c.large = w.take((size_t)f_total);
    c.tris = w.take((size_t)f_total * 12);
    c.refs = w.take((size_t)f_total * CELL_CAP);
}

namespace {

// steps 0 to 5 on `stream`, after the includer cleared the cleared regions: offsets, box, extents, geometry, count, scan, fill.
// Afterwards counts[cell] .. counts[cell + 1] delimit the cell's references in refs.
inline void build(int* ws, const Carve& c, const float* verts, const int32_t* faces, const int32_t* v_count, const int32_t* f_count,
                  int n_images, int v_total, int f_total, hipStream_t stream) {
    int *v_start = ws + c.v_start, *f_start = ws + c.f_start;
    unsigned* box = (unsigned*)(ws + c.box);
    unsigned long long* ext_sum = (unsigned long long*)(ws + c.ext_sum);
    Meta* meta = (Meta*)(ws + c.meta);
    float4* tris = (float4*)(ws + c.tris);
    const int face_blocks = (f_total + THREADS - 1) / THREADS;
    const int n_cells = (int)c.n_cells, nblk = (int)c.nblk;
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(64), 0, stream, n_images, v_count, f_count, v_total, f_total, v_start, f_start);
    hipLaunchKernelGGL(bbox_kernel, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, f_total, verts, faces, v_start, f_start, box, tris);
    hipLaunchKernelGGL(extent_kernel, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, f_total, f_start, box, tris, ext_sum);
    hipLaunchKernelGGL(meta_kernel, dim3(1), dim3(THREADS), 0, stream, n_images, box, ext_sum, meta);
    hipLaunchKernelGGL(bin_kernel<false>, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, f_total, f_start, meta, tris,
                       ws + c.counts, ws + c.cursor, ws + c.refs, ws + c.large, ws + c.large_count);
    hipLaunchKernelGGL(scan_local_kernel, dim3(nblk), dim3(1024), 0, stream, n_cells, ws + c.counts, ws + c.block_tot);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(1024), 0, stream, nblk, ws + c.block_tot);
    hipLaunchKernelGGL(scan_add_kernel, dim3(nblk), dim3(1024), 0, stream, n_cells, ws + c.counts, ws + c.block_tot);
    hipLaunchKernelGGL(bin_kernel<true>, dim3(face_blocks), dim3(THREADS), 0, stream, n_images, f_total, f_start, meta, tris,
                       ws + c.counts, ws + c.cursor, ws + c.refs, ws + c.large, ws + c.large_count);
}

}  // namespace

}  // namespace sc_tgrid
