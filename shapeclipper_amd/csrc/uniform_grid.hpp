// uniform_grid.hpp -- the uniform grid the exact searches bin their data into before they walk it (chamfer_grid.hip: the target cloud
// and, for the wave walk, the query cloud; point_normals.hip: the cloud itself; triangle_grid.hpp, for point_mesh.hip and
// mesh_intersect.hip: triangles by their boxes).
//
// The correctness argument of every walk leans on these pieces and on nothing else of the build:
//   * the box is exact: minima and maxima travel as order-preserving integer keys through atomicMax, so lo / hi are coordinates of the
//     data, whatever the order the waves arrive in;
//   * the cells tile [lo, lo + g * h) per axis and axis_cell is monotone in v, so data at x lies in cell(x) up to the rounding of
//     (v - lo) * inv_h and of the face coordinates lo + c * h the walks compute: both stay below `slack` = 16 ulp of (largest
//     magnitude + largest extent), which is what the walks subtract from their bound;
//   * everything is integer atomics and plain stores: the same cells run to run (the order INSIDE a cell is arbitrary, the walks'
//     acceptance rules do not depend on it).
// The constants (points per cell, cells per axis, cell budget, growth rounds) are the includer's: they were tuned per search and only
// show as time, never in a result, so they are arguments here.
//
// Every __global__ below sits in an anonymous namespace: the including objects are built with different -ffp-contract settings
// (csrc/Makefile) and each must carry, and launch, the copy compiled with its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace sc_grid {

// ---- order-preserving float -> unsigned map -------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned key(float f) {
    const unsigned u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

// ---- the box: 8 words per image -------------------------------------------------------------------------------------------------
// [0..2] = ~key(min), [3..5] = key(max): both only ever grow, so atomicMax merges them and the all-zero state a memset leaves means
// "nothing yet"; [6] = a coordinate is not a plain finite number of sensible magnitude; [7] is the includer's (point_mesh.hip counts its
// valid faces there).
constexpr int BOX_WORDS = 8, BOX_BAD = 6, BOX_USER = 7;

// minima / maxima over the 64 lanes, left in every lane
__device__ __forceinline__ void wave_minmax(float mn[3], float mx[3]) {
    for (int a = 0; a < 3; ++a)
        for (int d = 32; d >= 1; d >>= 1) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], d)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], d)); }
}
__device__ __forceinline__ void box_merge(unsigned* box, const float mn[3], const float mx[3], int bad) {
    for (int a = 0; a < 3; ++a) { atomicMax(&box[a], ~key(mn[a])); atomicMax(&box[3 + a], key(mx[a])); }
    if (bad) atomicOr(&box[BOX_BAD], 1u);
}
// returns the bad flag; an untouched box reads as NaN bounds
__device__ __forceinline__ bool box_read(const unsigned* box, float lo[3], float hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = unkey(~box[a]); hi[a] = unkey(box[3 + a]); }
    return box[BOX_BAD] != 0;
}

// ---- grid geometry --------------------------------------------------------------------------------------------------------------
struct Geometry {                      // one per image; the includers' meta structs extend it
    float lo[3], h[3], inv_h[3];
    int g[3];
    float slack;
    int valid;
};

// Box -> geometry.  start_h(volume, largest extent) gives the cell side to start from (both taken after thin axes were widened to 1e-3
// of the largest extent, so that a flat cloud still gets cells of a sensible size); the per-axis ceil can overshoot the budget of `cap`
// cells, so the side grows by 1.26 (a factor 2 in cells) for up to `rounds` rounds until the grid fits.  Then the cells tile the extent
// exactly (the last cell also takes x == hi by clamping).  g.valid = a good box of positive extent whose grid fits; the caller adds its
// own conditions and resets what it wants reset when the grid is invalid.  Returns the side the loop ended with.
template <class StartH>
__device__ __forceinline__ float geometry_from_box(const unsigned* box, long long cap, int gmax, int rounds, StartH start_h, Geometry& g) {
    float hi[3], ext[3], scale = 0.f, emax = 0.f;
    const bool bad = box_read(box, g.lo, hi);
    for (int a = 0; a < 3; ++a) {
        ext[a] = hi[a] - g.lo[a];
        emax = fmaxf(emax, ext[a]);
        scale = fmaxf(scale, fmaxf(fabsf(g.lo[a]), fabsf(hi[a])));
    }
    float vol = 1.f;
    for (int a = 0; a < 3; ++a) { ext[a] = fmaxf(ext[a], emax * 1.0e-3f); vol *= ext[a]; }
    float h = start_h(vol, emax);
    long long cells = 1;
    for (int it = 0; it < rounds; ++it) {
        cells = 1;
        for (int a = 0; a < 3; ++a) {
            int n = (int)fminf(ceilf(ext[a] / h), (float)gmax);        // clamped as a float: the quotient may be past INT_MAX (h == 0)
            n = n < 1 ? 1 : n;
            g.g[a] = n;
            cells *= n;
        }
        if (cells <= cap) break;
        h *= 1.26f;
    }
    g.valid = (!bad && emax > 0.f && cells <= cap) ? 1 : 0;
    for (int a = 0; a < 3; ++a) {
        g.h[a] = ext[a] / (float)g.g[a];
        g.inv_h[a] = (float)g.g[a] / ext[a];
    }
    g.slack = 16.f * 1.1920929e-7f * (scale + emax);
    return h;
}

// cell of coordinate v along one axis, clamped into the grid: for points inside the box or a few cells around it
__device__ __forceinline__ int axis_cell(float v, float lo, float inv_h, int g) {
    const int c = (int)floorf((v - lo) * inv_h);
    return c < 0 ? 0 : (c >= g ? g - 1 : c);
}
// The same cell for a coordinate that may lie ANYWHERE: point_mesh.hip feeds it mn - slack / mx + slack of triangle boxes and queries
// far outside the grid, where (v - lo) * inv_h can be past the int range; so the clamp to [-1, g] happens on the float, before the
// conversion.  Inside the int range the two functions agree.
__device__ __forceinline__ int axis_cell_far(float v, float lo, float inv_h, int g) {
    const int c = (int)fminf(fmaxf(floorf((v - lo) * inv_h), -1.f), (float)g);
    return c < 0 ? 0 : (c >= g ? g - 1 : c);
}

// ---- binning a point cloud [image][n][3] ----------------------------------------------------------------------------------------
// Meta is the includer's struct (a Geometry, plus `dense` where ONLY_DENSE / QUERY_TILES are used: chamfer_grid.hip's query side, which
// is binned for images with surface-like targets only, and by 2 x 2 x 2 TILE of cells).  counts and start are [image][cap + 1],
// cursor is [image][cap].
namespace {

// 1. Many workgroups per image (one 1024-thread workgroup per image took 40 us for 100,000 points): per-wave minima / maxima -> box.
__global__ __launch_bounds__(256) void bbox_kernel(int n, const float* __restrict__ pts, unsigned* __restrict__ box_all) {
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* p = pts + (size_t)b * n * 3;
    float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    int bad = 0, any = 0;
    for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
        any = 1;
        for (int a = 0; a < 3; ++a) {
            const float v = p[(size_t)i * 3 + a];
            bad |= !(fabsf(v) < 1.0e15f);          // NaN, Inf and magnitudes the padding / slack arithmetic is not made for
            mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v);
        }
    }
    wave_minmax(mn, mx);
    any = __any(any);
    bad = __any(bad);
    if ((tid & 63) == 0 && any) box_merge(box_all + (size_t)b * BOX_WORDS, mn, mx, bad);
}

// 2. cell of every point + histogram
template <bool QUERY_TILES, class Meta>
__global__ __launch_bounds__(256) void count_kernel(int n, const float* __restrict__ pts, const Meta* __restrict__ meta, int cap,
                                                    int* __restrict__ cell_of, int* __restrict__ counts) {
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Meta& g = meta[b];
    if constexpr (QUERY_TILES)
        if (!g.dense) return;
    const float* p = pts + ((size_t)b * n + i) * 3;
    int c = 0;
    if (g.valid) {
        const int cx = axis_cell(p[0], g.lo[0], g.inv_h[0], g.g[0]), cy = axis_cell(p[1], g.lo[1], g.inv_h[1], g.g[1]);
        const int cz = axis_cell(p[2], g.lo[2], g.inv_h[2], g.g[2]);
        c = (cz * g.g[1] + cy) * g.g[0] + cx;       // x fastest: a run of cells along x is one contiguous run of sorted points
        if constexpr (QUERY_TILES) c = ((cz >> 1) * ((g.g[1] + 1) >> 1) + (cy >> 1)) * ((g.g[0] + 1) >> 1) + (cx >> 1);
    }
    cell_of[(size_t)b * n + i] = c;
    atomicAdd(&counts[(size_t)b * (cap + 1) + c], 1);
}

// 3. (after the includer's exclusive scan of counts into start) points into cell order as {x, y, z, original index}
template <bool ONLY_DENSE, class Meta>
__global__ __launch_bounds__(256) void scatter_kernel(int n, const float* __restrict__ pts, int cap, const int* __restrict__ cell_of,
                                                      const int* __restrict__ start, int* __restrict__ cursor,
                                                      float4* __restrict__ sorted, const Meta* __restrict__ meta) {
    const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if constexpr (ONLY_DENSE)
        if (!meta[b].dense) return;
    const int c = cell_of[(size_t)b * n + i];
    const int pos = start[(size_t)b * (cap + 1) + c] + atomicAdd(&cursor[(size_t)b * cap + c], 1);
    const float* p = pts + ((size_t)b * n + i) * 3;
    sorted[(size_t)b * n + pos] = make_float4(p[0], p[1], p[2], __int_as_float(i));
}

}  // namespace

// ---- the workspace, carved in 4-byte words: every region starts at a multiple of 4 words (16 bytes: float4 and 64-bit regions) -----
struct WordCarver {
    size_t words = 0;
    size_t take(size_t n) {
        const size_t at = words;
        words += (n + 3) & ~(size_t)3;
        return at;
    }
};

}  // namespace sc_grid
