// dual_contour.hip -- dual contouring of the level grid from the state of the indexed marching-cubes mesh (ops.dual_contour_mesh).
//
// Marching cubes puts every vertex on a grid edge, so a corner or a crease inside a cell comes out chamfered at the grid pitch.  With a
// normal per crossing vertex (the SDF gradient, which this build evaluates exactly) the crossings are Hermite data, and dual contouring
// places ONE vertex per surface cell where the tangent planes of the cell's crossings meet, and one quad per sign-changing grid edge
// between the four cells around it.
//
//   sc_dual_contour_count      per 1,024-cube block: owning cells, and triangles (2 per crossing edge with four cells around it), both
//                              from the case byte alone (1 byte per cube; the level grid is not read again)
//   sc_dual_contour_cell_emit  owning cells are compacted per block, then their (cell, edge) pairs are dealt out to all lanes for the
//                              gather through vmap (up to 12 x 24 bytes per cell; about one cell in thirty owns a vertex), the Hermite
//                              data meet in LDS and one lane per cell runs the fixed-order sums and the 3 x 3 solve
//   sc_dual_contour_face_emit  quads re-dealt to lanes by a binary search in the block's prefix, as mc_block_emit_kernel does
//
// include/shapeclipper_hip.h states the cell solve one fp32 rounding at a time; tests/dual_contour_ref.py restates it in numpy and the GPU
// tests compare bits.  No contraction (the Makefile compiles this file with -ffp-contract=off and the kernels carry the pragma), true
// comparisons (a NaN fails them all), plain vector stores, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "block_scan.hpp"
#include "../../include/shapeclipper_hip.h"

namespace sc {

constexpr int DC_BLOCK_CELLS = 1024;            // the cube block of isosurface.hip (ISO_BLOCK_CUBES): sc_isosurface_block_scan serves both
constexpr int DC_CHUNK = 64;                    // cells solved per round of the emit: 64 x 12 (cell, edge) pairs = 3 per thread
constexpr int DC_EDGE_FLOATS = 7;               // p[3], n[3], crossing flag
constexpr int DC_CELL_STRIDE = 12 * DC_EDGE_FLOATS + 1;     // odd: one lane per cell walks its edges without LDS bank conflicts

// cube edge e = (lower corner, axis), the order of kMcEdge in mc_table.hpp: (0,1) (0,2) (0,4) (1,3) (1,5) (2,3) (2,6) (3,7) (4,5) (4,6)
// (5,7) (6,7); corner id bit 0 = +x, bit 1 = +y, bit 2 = +z.  Packed 3 + 2 bits per edge so a lane's edge needs no table load.
constexpr unsigned long long DC_EDGE_CORNER = 0ull | (0ull << 3) | (0ull << 6) | (1ull << 9) | (1ull << 12) | (2ull << 15) | (2ull << 18) |
                                              (3ull << 21) | (4ull << 24) | (4ull << 27) | (5ull << 30) | (6ull << 33);
constexpr unsigned int DC_EDGE_AXIS = 0u | (1u << 2) | (2u << 4) | (1u << 6) | (2u << 8) | (0u << 10) | (2u << 12) | (2u << 14) | (0u << 16) |
                                      (1u << 18) | (1u << 20) | (0u << 22);

__device__ __forceinline__ bool dc_owns(int mask) { return mask != 0 && mask != 255; }

// bit a: the grid edge from the cell's corner 0 along axis a changes sign and has four cells around it (the other two coordinates of
// its lower end are >= 1; they are <= n_axis - 2 because the lower end is a cell)
__device__ __forceinline__ int dc_quad_axes(int mask, int gx, int gy, int gz) {
    const int c0 = mask & 1;
    int f = 0;
    if (((mask >> 1) & 1) != c0 && gy >= 1 && gz >= 1) f |= 1;
    if (((mask >> 2) & 1) != c0 && gz >= 1 && gx >= 1) f |= 2;
    if (((mask >> 4) & 1) != c0 && gx >= 1 && gy >= 1) f |= 4;
    return f;
}

__global__ __launch_bounds__(256) void dc_count_kernel(const unsigned char* __restrict__ masks, int S, int bpi, int* __restrict__ cell_counts,
                                                       int* __restrict__ face_counts) {
    __shared__ int wave_tot[2][4];
    const int Nc = S - 1, per = Nc * Nc * Nc;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cells = 0, tris = 0;
#pragma unroll
    for (int j = 0; j < DC_BLOCK_CELLS / 256; ++j) {
        const int r = blk * DC_BLOCK_CELLS + j * 256 + tid;
        if (r < per) {
            const int m = masks[(size_t)b * per + r];
            const int q = r / Nc, gz = r - q * Nc, gx = q / Nc, gy = q - gx * Nc;
            cells += dc_owns(m) ? 1 : 0;
            tris += 2 * __popc(dc_quad_axes(m, gx, gy, gz));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cells += __shfl_xor(cells, d), tris += __shfl_xor(tris, d);
    if (lane == 0) wave_tot[0][wave] = cells, wave_tot[1][wave] = tris;
    __syncthreads();
    if (tid == 0) {
        cell_counts[blockIdx.x] = wave_tot[0][0] + wave_tot[0][1] + wave_tot[0][2] + wave_tot[0][3];
        face_counts[blockIdx.x] = wave_tot[1][0] + wave_tot[1][1] + wave_tot[1][2] + wave_tot[1][3];
    }
}

// The cell solve of include/shapeclipper_hip.h on the 12 edge records h[e * DC_EDGE_FLOATS ..] of one cell (g = its lower corner).
__device__ __forceinline__ void dc_solve_cell(const float* h, int gx, int gy, int gz, float reg, float* x) {
#pragma clang fp contract(off)
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
    int k = 0;
    for (int e = 0; e < 12; ++e) {
        const float* r = h + e * DC_EDGE_FLOATS;
        if (r[6] != 0.0f) {
            s0 = __fadd_rn(s0, r[0]), s1 = __fadd_rn(s1, r[1]), s2 = __fadd_rn(s2, r[2]);
            ++k;
        }
    }
    const float kf = (float)k;                                  // k >= 1: an owning cell has a sign-changing edge
    const float c0 = __fdiv_rn(s0, kf), c1 = __fdiv_rn(s1, kf), c2 = __fdiv_rn(s2, kf);
    float a00 = 0.0f, a01 = 0.0f, a02 = 0.0f, a11 = 0.0f, a12 = 0.0f, a22 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
    for (int e = 0; e < 12; ++e) {
        const float* r = h + e * DC_EDGE_FLOATS;
        const float n0 = r[3], n1 = r[4], n2 = r[5];
        // a normal with a non-finite component counts for c and k only
        if (r[6] != 0.0f && fabsf(n0) <= 3.402823466e+38f && fabsf(n1) <= 3.402823466e+38f && fabsf(n2) <= 3.402823466e+38f) {
            const float d0 = __fsub_rn(r[0], c0), d1 = __fsub_rn(r[1], c1), d2 = __fsub_rn(r[2], c2);
            const float w = __fadd_rn(__fadd_rn(__fmul_rn(n0, d0), __fmul_rn(n1, d1)), __fmul_rn(n2, d2));
            a00 = __fadd_rn(a00, __fmul_rn(n0, n0)), a01 = __fadd_rn(a01, __fmul_rn(n0, n1)), a02 = __fadd_rn(a02, __fmul_rn(n0, n2));
            a11 = __fadd_rn(a11, __fmul_rn(n1, n1)), a12 = __fadd_rn(a12, __fmul_rn(n1, n2)), a22 = __fadd_rn(a22, __fmul_rn(n2, n2));
            b0 = __fadd_rn(b0, __fmul_rn(n0, w)), b1 = __fadd_rn(b1, __fmul_rn(n1, w)), b2 = __fadd_rn(b2, __fmul_rn(n2, w));
        }
    }
    const float rk = __fmul_rn(reg, kf);
    a00 = __fadd_rn(a00, rk), a11 = __fadd_rn(a11, rk), a22 = __fadd_rn(a22, rk);
    // LDL^T, divisions only
    const float l10 = __fdiv_rn(a01, a00), l20 = __fdiv_rn(a02, a00);
    const float e1 = __fsub_rn(a11, __fmul_rn(l10, a01));
    const float t21 = __fsub_rn(a12, __fmul_rn(l20, a01));
    const float l21 = __fdiv_rn(t21, e1);
    const float e2 = __fsub_rn(__fsub_rn(a22, __fmul_rn(l20, a02)), __fmul_rn(l21, t21));
    const float z1 = __fsub_rn(b1, __fmul_rn(l10, b0));
    const float z2 = __fsub_rn(__fsub_rn(b2, __fmul_rn(l20, b0)), __fmul_rn(l21, z1));
    const float y2 = __fdiv_rn(z2, e2);
    const float y1 = __fsub_rn(__fdiv_rn(z1, e1), __fmul_rn(l21, y2));
    const float y0 = __fsub_rn(__fsub_rn(__fdiv_rn(b0, a00), __fmul_rn(l10, y1)), __fmul_rn(l20, y2));
    const float y[3] = {y0, y1, y2}, c[3] = {c0, c1, c2};
    const int g[3] = {gx, gy, gz};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float lo = (float)g[i], hi = (float)(g[i] + 1);
        float v = __fadd_rn(c[i], y[i]);
        if (!(v >= lo)) v = lo;                                 // (a NaN lands on the cell's lower corner)
        if (!(v <= hi)) v = hi;
        x[i] = v;
    }
}

__global__ __launch_bounds__(256) void dc_cell_emit_kernel(const unsigned char* __restrict__ masks, const float* __restrict__ verts,
                                                           const float* __restrict__ normals, const int* __restrict__ vmap,
                                                           const long long* __restrict__ vertex_block_offsets, int vbpi, int S, int bpi, float reg,
                                                           const long long* __restrict__ block_offsets, float* __restrict__ dual_verts,
                                                           int* __restrict__ cell_map) {
    __shared__ unsigned int list[DC_BLOCK_CELLS];               // owning cells of the block in ascending order: local index | case byte << 16
    __shared__ int wave_tot[4];
    __shared__ float herm[DC_CHUNK * DC_CELL_STRIDE];
    const int Nc = S - 1, per = Nc * Nc * Nc;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long base = block_offsets[blockIdx.x];
    if (block_offsets[blockIdx.x + 1] == base) return;          // no owning cell in this block
    const long long first = block_offsets[(size_t)b * bpi];     // the image's first dual vertex / first crossing vertex
    const long long vfirst = vertex_block_offsets[(size_t)b * vbpi];
    const size_t points = (size_t)S * S * S;
    int total = 0;
#pragma unroll 1
    for (int j = 0; j < DC_BLOCK_CELLS / 256; ++j) {
        const int loc = j * 256 + tid, r = blk * DC_BLOCK_CELLS + loc;
        const int m = r < per ? masks[(size_t)b * per + r] : 0;
        const bool own = dc_owns(m);
        const unsigned long long bal = __ballot(own);
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int t = wave_tot[w];
            if (w < wave) before += t;
            tot += t;
        }
        if (own) list[total + before + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned)loc | ((unsigned)m << 16);
        total += tot;
        __syncthreads();
    }
#pragma unroll 1
    for (int c0 = 0; c0 < total; c0 += DC_CHUNK) {
        const int n = total - c0 < DC_CHUNK ? total - c0 : DC_CHUNK;
#pragma unroll
        for (int k = 0; k < DC_CHUNK * 12 / 256; ++k) {         // gather: all three rounds' loads in flight
            const int i = k * 256 + tid, slot = i / 12, e = i - slot * 12;
            if (slot < n) {
                const unsigned ent = list[c0 + slot];
                const int r = blk * DC_BLOCK_CELLS + (int)(ent & 0xffffu), m = (int)(ent >> 16);
                const int ca = (int)((DC_EDGE_CORNER >> (3 * e)) & 7ull), axis = (int)((DC_EDGE_AXIS >> (2 * e)) & 3u);
                float* h = herm + slot * DC_CELL_STRIDE + e * DC_EDGE_FLOATS;
                if (((m >> ca) ^ (m >> (ca + (1 << axis)))) & 1) {
                    const int q = r / Nc, gz = r - q * Nc, gx = q / Nc, gy = q - gx * Nc;
                    const int owner = ((gx + (ca & 1)) * S + (gy + ((ca >> 1) & 1))) * S + (gz + ((ca >> 2) & 1));
                    const size_t row = (size_t)(vfirst + vmap[((size_t)b * points + owner) * 3 + axis]) * 3;
                    h[0] = verts[row], h[1] = verts[row + 1], h[2] = verts[row + 2];
                    h[3] = normals[row], h[4] = normals[row + 1], h[5] = normals[row + 2];
                    h[6] = 1.0f;
                } else {
                    h[6] = 0.0f;
                }
            }
        }
        __syncthreads();
        if (tid < n) {
            const unsigned ent = list[c0 + tid];
            const int r = blk * DC_BLOCK_CELLS + (int)(ent & 0xffffu);
            const int q = r / Nc, gz = r - q * Nc, gx = q / Nc, gy = q - gx * Nc;
            float x[3];
            dc_solve_cell(herm + tid * DC_CELL_STRIDE, gx, gy, gz, reg, x);
            const long long v = base + c0 + tid;
            float* dst = dual_verts + (size_t)v * 3;
            dst[0] = x[0], dst[1] = x[1], dst[2] = x[2];
            cell_map[(size_t)b * per + r] = (int)(v - first);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void dc_face_emit_kernel(const unsigned char* __restrict__ masks, const int* __restrict__ cell_map, int S, int bpi,
                                                           const long long* __restrict__ block_offsets, int* __restrict__ faces) {
    __shared__ int excl[256];
    __shared__ int wave_tot[4];
    __shared__ unsigned char flag_s[256];                       // dc_quad_axes | (corner 0 inside) << 3
    const int Nc = S - 1, per = Nc * Nc * Nc;
    const int b = blockIdx.x / bpi, blk = blockIdx.x - b * bpi;
    const int tid = threadIdx.x;
    long long running = block_offsets[blockIdx.x];              // in triangles
    if (block_offsets[blockIdx.x + 1] == running) return;
    const int* cm = cell_map + (size_t)b * per;
#pragma unroll 1
    for (int j = 0; j < DC_BLOCK_CELLS / 256; ++j) {
        const int r0 = blk * DC_BLOCK_CELLS + j * 256, r = r0 + tid;
        int fl = 0;
        if (r < per) {
            const int m = masks[(size_t)b * per + r];
            const int q = r / Nc, gz = r - q * Nc, gx = q / Nc, gy = q - gx * Nc;
            fl = dc_quad_axes(m, gx, gy, gz) | ((m & 1) << 3);
        }
        const int n = __popc(fl & 7);
        int total;
        excl[tid] = sc_scan::block_exclusive<4>(n, wave_tot, total);            // the round's closing barrier frees wave_tot for the next
        flag_s[tid] = (unsigned char)fl;
        __syncthreads();
        for (int qd = tid; qd < total; qd += 256) {
            int lo = 0;                                          // the largest cell index whose exclusive prefix is <= qd
#pragma unroll
            for (int step = 128; step >= 1; step >>= 1)
                if (excl[lo + step] <= qd) lo += step;
            const int f = flag_s[lo];
            int which = qd - excl[lo], axis = 0;                 // the which-th set bit of the cell's axes
            for (; axis < 3; ++axis)
                if ((f >> axis) & 1) {
                    if (which == 0) break;
                    --which;
                }
            // (a, b, c) cyclic: the cells (P_b - 1, P_c - 1), (P_b, P_c - 1), (P_b, P_c), (P_b - 1, P_c) around the edge, P = this cell
            const int stb = axis == 0 ? Nc : axis == 1 ? 1 : Nc * Nc, stc = axis == 0 ? 1 : axis == 1 ? Nc * Nc : Nc;
            const int rc = r0 + lo;
            const int i0 = cm[rc - stb - stc], i1 = cm[rc - stc], i2 = cm[rc], i3 = cm[rc - stb];
            int* dst = faces + (size_t)(running + 2 * qd) * 3;
            if (f & 8) {                                         // lower end inside: the quad's normal points along +a, out of the solid
                dst[0] = i0, dst[1] = i1, dst[2] = i2;
                dst[3] = i0, dst[4] = i2, dst[5] = i3;
            } else {
                dst[0] = i0, dst[1] = i2, dst[2] = i1;
                dst[3] = i0, dst[4] = i3, dst[5] = i2;
            }
        }
        running += 2 * total;
        __syncthreads();
    }
}

static int dc_blocks(int n_images, int n_axis) {                // workgroups of a launch, or -1 where the entry points refuse
    if (n_axis < 2 || n_axis > 1024) return -1;
    const long long Nc = n_axis - 1, bpi = (Nc * Nc * Nc + DC_BLOCK_CELLS - 1) / DC_BLOCK_CELLS;
    return bpi * n_images >= (1LL << 31) ? -1 : (int)(bpi * n_images);
}

}  // namespace sc

extern "C" {

int sc_dual_contour_count(const unsigned char* masks, int n_images, int n_axis, int* cell_block_counts, int* face_block_counts, void* stream_) {
    if (n_images <= 0) return 0;
    const int blocks = sc::dc_blocks(n_images, n_axis);
    if (blocks < 0 || !masks || !cell_block_counts || !face_block_counts) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sc::dc_count_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, masks, n_axis, blocks / n_images,
                       cell_block_counts, face_block_counts);
    return (int)hipGetLastError();
}

int sc_dual_contour_cell_emit(const unsigned char* masks, const float* verts, const float* normals, const int* vmap,
                              const long long* vertex_block_offsets, int n_images, int n_axis, float reg, const long long* cell_block_offsets,
                              float* dual_verts, int* cell_map, void* stream_) {
    if (n_images <= 0) return 0;
    const int blocks = sc::dc_blocks(n_images, n_axis);
    const int vbpi = sc_marching_cubes_mesh_vertex_blocks_per_image(n_axis);
    if (blocks < 0 || vbpi <= 0 || !(reg > 0.0f && reg <= 3.402823466e+38f) || !masks || !verts || !normals || !vmap || !vertex_block_offsets ||
        !cell_block_offsets || !dual_verts || !cell_map)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sc::dc_cell_emit_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, masks, verts, normals, vmap,
                       vertex_block_offsets, vbpi, n_axis, blocks / n_images, reg, cell_block_offsets, dual_verts, cell_map);
    return (int)hipGetLastError();
}

int sc_dual_contour_face_emit(const unsigned char* masks, const int* cell_map, int n_images, int n_axis, const long long* face_block_offsets,
                              int* faces, void* stream_) {
    if (n_images <= 0) return 0;
    const int blocks = sc::dc_blocks(n_images, n_axis);
    if (blocks < 0 || !masks || !cell_map || !face_block_offsets || !faces) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(sc::dc_face_emit_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, masks, cell_map, n_axis,
                       blocks / n_images, face_block_offsets, faces);
    return (int)hipGetLastError();
}

}  // extern "C"
