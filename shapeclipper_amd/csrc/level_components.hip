// level_components.hip -- keep the largest connected component of the solid {level < iso} of a level grid (the stage between
// compute_level_grid and the mesher of csrc/isosurface.hip; definition in include/shapeclipper_hip.h, sc_level_largest_component).
//
// Integer work on a regular grid, five launches on one stream, no spin barrier and no cooperative launch:
//   1. lc_tile_kernel      one workgroup per 8 x 8 x 8 tile: union-find of its inside voxels in LDS over the three in-tile face
//                          neighbours; every voxel gets the image-linear index of its tile-local root (-1 outside), every tile-local
//                          root the voxel count of its piece (0 elsewhere).  Tiles that S does not fill mask their missing voxels.
//   2. lc_merge_kernel     every inside voxel on a low tile face unites with the inside voxel across the face: integer atomicMin on
//                          the global label array (find / unite of mesh_edges.hpp, shared with mesh_topology.hip).
//   3. lc_flatten_kernel   label[v] = root(v); a tile-local root that is not the global root adds its piece's count to the root's.
//   4. lc_select_kernel    per image: number of roots, sum of their counts, max of (count << 32 | ~label) -- the largest component,
//                          the smaller label on a tie -- reduced per workgroup, then one integer atomic each.
//   5. lc_mask_kernel      level_out = level, but iso + (iso - level) at inside voxels whose label is not the kept one; the three
//                          int32 outputs of each image.
// A parent is always a SMALLER index of the same component (a root points at itself), so the root of a component is its smallest
// linear index, every find loop walks strictly decreasing labels and ends whatever other threads do meanwhile, and a value read late
// (another CU's update not yet seen) is still an ancestor: it costs steps, never the result.  What decides a union is the value the
// atomicMin returns.  Only integer atomics, so the result does not depend on arrival order: the same bits run to run, for any batch,
// stream or grid size.
// Bound: latency of the dependent label loads (3 x 4 B per voxel per pass otherwise); not a hot path of training.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "shapeclipper_hip.h"
#include "mesh_edges.hpp"

namespace sc {
namespace lc {

constexpr int TILE = 8, TILE_VOX = TILE * TILE * TILE;      // one thread per voxel of a tile
constexpr int MAX_IMAGES = 65535;                           // images ride on gridDim.y
constexpr int FLAT_BLOCKS = 2048;                           // cap of the grid-stride passes (x dimension)

// ---- union-find on labels in LDS (workgroup-coherent) ----
__device__ __forceinline__ int find_lds(const int* lab, int x) {
    for (;;) {
        const int p = lab[x];
        if (p >= x || p < 0) return x;
        x = p;
    }
}
__device__ __forceinline__ void unite_lds(int* lab, int a, int b) {
    for (;;) {
        a = find_lds(lab, a);
        b = find_lds(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&lab[a], b);               // a > b: a's parent becomes min(its parent, b)
        if (old == a) return;                                // a was a root: linked
        a = old;                                             // a had a parent: that one and b are still to be united
    }
}

// ---- the same on the global label array of one image: sc_mesh::find / sc_mesh::unite (mesh_edges.hpp) ----

// grid (T^3, n_images), T = ceil(S / 8)
__global__ __launch_bounds__(TILE_VOX) void lc_tile_kernel(const float* __restrict__ level, int S, int T, float iso, int* __restrict__ label,
                                                           int* __restrict__ count, unsigned long long* __restrict__ best,
                                                           int* __restrict__ totals) {
    __shared__ int lab[TILE_VOX];
    __shared__ int num[TILE_VOX];
    const int t = threadIdx.x, lz = t & 7, ly = (t >> 3) & 7, lx = t >> 6;
    const int tile = blockIdx.x, tz = tile % T, tq = tile / T, ty = tq % T, tx = tq / T;
    const int x = tx * TILE + lx, y = ty * TILE + ly, z = tz * TILE + lz;
    const bool valid = x < S && y < S && z < S;
    const size_t base = (size_t)blockIdx.y * S * S * S;
    const int v = (x * S + y) * S + z;                      // S <= 1024: fits 31 bits (used when valid only)
    if (tile == 0 && t == 0) {                              // the per-image accumulators of lc_select_kernel, three launches ahead
        best[blockIdx.y] = 0ull;
        totals[2 * blockIdx.y] = 0, totals[2 * blockIdx.y + 1] = 0;
    }
    const bool inside = valid && level[base + v] < iso;     // NaN compares false: outside
    lab[t] = inside ? t : -1;
    num[t] = 0;
    __syncthreads();
    if (inside) {
        if (lx > 0 && lab[t - 64] >= 0) unite_lds(lab, t, t - 64);
        if (ly > 0 && lab[t - 8] >= 0) unite_lds(lab, t, t - 8);
        if (lz > 0 && lab[t - 1] >= 0) unite_lds(lab, t, t - 1);
    }
    __syncthreads();
    const int root = inside ? find_lds(lab, t) : -1;
    if (inside) atomicAdd(&num[root], 1);
    __syncthreads();
    if (valid) {
        // the tile's index order is the image's: the local root is the smallest image-linear index of the piece
        label[base + v] = inside ? ((tx * TILE + (root >> 6)) * S + (ty * TILE + ((root >> 3) & 7))) * S + (tz * TILE + (root & 7)) : -1;
        count[base + v] = root == t ? num[t] : 0;
    }
}

// grid (<= FLAT_BLOCKS, n_images)
__global__ __launch_bounds__(256) void lc_merge_kernel(int* label, int S, int per) {
    int* L = label + (size_t)blockIdx.y * per;
    const int SS = S * S;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < per; v += gridDim.x * 256) {
        if (L[v] < 0) continue;                             // the sign of a label never changes
        const int q = v / S, z = v - q * S, x = q / S, y = q - x * S;
        if ((x & 7) == 0 && x > 0 && L[v - SS] >= 0) sc_mesh::unite(L, v, v - SS);
        if ((y & 7) == 0 && y > 0 && L[v - S] >= 0) sc_mesh::unite(L, v, v - S);
        if ((z & 7) == 0 && z > 0 && L[v - 1] >= 0) sc_mesh::unite(L, v, v - 1);
    }
}

// Roots keep label[r] == r and nobody adds to a count that is read here: only global roots receive, only the others give.
__global__ __launch_bounds__(256) void lc_flatten_kernel(int* label, int* count, int per) {
    int* L = label + (size_t)blockIdx.y * per;
    int* C = count + (size_t)blockIdx.y * per;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < per; v += gridDim.x * 256) {
        if (L[v] < 0) continue;
        const int r = sc_mesh::find(L, v);
        if (r == v) continue;
        L[v] = r;                                           // a reader sees the old parent or the root: both are ancestors
        const int c = C[v];
        if (c > 0) atomicAdd(C + r, c);
    }
}

__global__ __launch_bounds__(256) void lc_select_kernel(const int* __restrict__ label, const int* __restrict__ count, int per,
                                                        unsigned long long* best, int* totals) {
    __shared__ unsigned long long s_key[4];
    __shared__ int s_n[4], s_in[4];
    const int* L = label + (size_t)blockIdx.y * per;
    const int* C = count + (size_t)blockIdx.y * per;
    unsigned long long key = 0ull;
    int n = 0, in = 0;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < per; v += gridDim.x * 256) {
        if (L[v] != v) continue;
        const int c = C[v];
        const unsigned long long k = ((unsigned long long)(unsigned)c << 32) | (0xFFFFFFFFu - (unsigned)v);
        key = k > key ? k : key;
        n += 1, in += c;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long k = __shfl_xor(key, d);
        key = k > key ? k : key;
        n += __shfl_xor(n, d), in += __shfl_xor(in, d);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_key[wave] = key, s_n[wave] = n, s_in[wave] = in;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            key = s_key[w] > key ? s_key[w] : key;
            n += s_n[w], in += s_in[w];
        }
        if (n > 0) {
            atomicMax(best + blockIdx.y, key);
            atomicAdd(totals + 2 * blockIdx.y, n);
            atomicAdd(totals + 2 * blockIdx.y + 1, in);
        }
    }
}

// level_out may be level itself: every voxel is read and written by one thread
__global__ __launch_bounds__(256) void lc_mask_kernel(const float* level, const int* __restrict__ label, int per, float iso,
                                                      const unsigned long long* __restrict__ best, const int* __restrict__ totals,
                                                      float* level_out, int* __restrict__ n_components, int* __restrict__ inside_voxels,
                                                      int* __restrict__ kept_voxels) {
    const size_t base = (size_t)blockIdx.y * per;
    const unsigned long long key = best[blockIdx.y];
    const int keep = (int)(0xFFFFFFFFu - (unsigned)key);    // no inside voxel: key 0, keep -1, and no label is >= 0
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        n_components[blockIdx.y] = totals[2 * blockIdx.y];
        inside_voxels[blockIdx.y] = totals[2 * blockIdx.y + 1];
        kept_voxels[blockIdx.y] = (int)(key >> 32);
    }
    const uint32_t* in = reinterpret_cast<const uint32_t*>(level) + base;
    uint32_t* out = reinterpret_cast<uint32_t*>(level_out) + base;
    const int* L = label + base;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < per; v += gridDim.x * 256) {
        const uint32_t bits = in[v];                        // untouched voxels keep their bits (NaN payloads included)
        const int l = L[v];
        out[v] = (l >= 0 && l != keep) ? __float_as_uint(iso + (iso - __uint_as_float(bits))) : bits;
    }
}

using sc_mesh::align16;

}  // namespace lc
}  // namespace sc

// scratch layout: best [n] u64 | totals [n][2] int | (pad to 16 B) | label [n * S^3] int | count [n * S^3] int
extern "C" long long sc_level_largest_component_scratch_bytes(int n_images, int n_axis) {
    if (n_images <= 0 || n_images > sc::lc::MAX_IMAGES || n_axis < 2 || n_axis > 1024) return 0;
    const long long per = (long long)n_axis * n_axis * n_axis;
    return sc::lc::align16(16LL * n_images) + 8LL * per * n_images;
}

extern "C" int sc_level_largest_component(const float* level, int n_images, int n_axis, float iso, float* level_out, int32_t* n_components,
                                          int32_t* inside_voxels, int32_t* kept_voxels, void* scratch, void* stream_) {
    using namespace sc::lc;
    if (n_images <= 0) return 0;
    if (n_images > MAX_IMAGES || n_axis < 2 || n_axis > 1024 || !level || !level_out || !n_components || !inside_voxels || !kept_voxels ||
        !scratch || ((uintptr_t)scratch & 15))
        return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int S = n_axis, T = (S + TILE - 1) / TILE, per = S * S * S;          // per <= 2^30
    char* ws = (char*)scratch;
    unsigned long long* best = (unsigned long long*)ws;
    int* totals = (int*)(ws + 8LL * n_images);
    int* label = (int*)(ws + align16(16LL * n_images));
    int* count = label + (size_t)per * n_images;
    const int fb = (per + 255) / 256 < FLAT_BLOCKS ? (per + 255) / 256 : FLAT_BLOCKS;
    const dim3 flat((unsigned)fb, (unsigned)n_images), tiles((unsigned)(T * T * T), (unsigned)n_images);
    hipLaunchKernelGGL(lc_tile_kernel, tiles, dim3(TILE_VOX), 0, stream, level, S, T, iso, label, count, best, totals);
    hipLaunchKernelGGL(lc_merge_kernel, flat, dim3(256), 0, stream, label, S, per);
    hipLaunchKernelGGL(lc_flatten_kernel, flat, dim3(256), 0, stream, label, count, per);
    hipLaunchKernelGGL(lc_select_kernel, flat, dim3(256), 0, stream, (const int*)label, (const int*)count, per, best, totals);
    hipLaunchKernelGGL(lc_mask_kernel, flat, dim3(256), 0, stream, level, (const int*)label, per, iso, (const unsigned long long*)best,
                       (const int*)totals, level_out, n_components, inside_voxels, kept_voxels);
    return (int)hipGetLastError();
}
