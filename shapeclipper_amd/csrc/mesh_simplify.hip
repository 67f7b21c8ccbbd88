// mesh_simplify.hip -- decimation of a batch of indexed triangle meshes by vertex clustering with quadric placement (ops.mesh_cluster_simplify,
// the evaluation's {idx}_mesh_simplified.ply; definition in include/shapeclipper_hip.h, sc_mesh_cluster_simplify; restated in numpy by
// tests/mesh_simplify_ref.py).  Built without contraction: every float64 operation of a term and of the solve rounds once.
//
// Ten launches on one stream (six when n_faces == 0), no spin barrier, no cooperative launch, no host read:
//   1. ms_init_kernel      the cell masks, the accumulators, the face table (keys empty, counts 0, lowest faces INT_MAX), counts, flags.
//   2. ms_mark_kernel      a thread per vertex: its cell, or the bad_vertex flag; one 64-bit atomicOr sets the cell's bit of the image's mask.
//   3. ms_rank_kernel      a workgroup per image: the block scan of block_scan.hpp over the popcounts of the mask words -> the number
//                          of occupied cells in front of every word, and the image's cluster count.
//   4. ms_offsets_kernel   one workgroup: the running sum of the cluster counts over the images.
//   5. ms_vertex_kernel    a thread per vertex: its cluster number (rank of its cell's bit), n and s by 64-bit integer atomicAdd.
//   6. ms_face_kernel      a thread per face: the nine quadric terms to each distinct cluster of its corners (integer atomicAdd), then,
//                          unless it collapses, its ascending cluster triple goes into the image's region of the open-addressing table
//                          (64-bit atomicCAS on the empty key, linear probing); atomicAdd on its parity's count, atomicMin on its
//                          parity's lowest face.
//   7. ms_solve_kernel     a thread per cluster: the regularised 3x3 solve, the clamp, the output vertex.
//   8. ms_decide_kernel    a workgroup per 256 faces: which faces are written; the workgroup's count; the per-image counts.
//   9. ms_block_kernel     one workgroup: the running sum of the workgroup counts.
//  10. ms_emit_kernel      a workgroup per 256 faces: block-scan compaction -> faces_out and face_source in ascending source face number.
// Every probe ends: an image's region has more slots than it has faces.  Only integer atomics decide anything, so no output depends on
// the arrival order: the same bits run to run, for any batch, stream and face order (the face LIST follows the source order).
// image_of, image_add and the scratch carver are those of mesh_edges.hpp; the face table (cluster triples, a region per image) is this file's.
// Bound: latency of scattered 8-byte atomics (thirteen accumulators per cluster, up to 27 adds per face); not privatised in LDS --
// docs/LAB_NOTEBOOK.md holds the measured times; not a hot path of training.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "shapeclipper_hip.h"
#include "mesh_edges.hpp"

namespace sc {
namespace ms {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_BLOCKS = 4096;                            // cap of the grid-stride passes
constexpr int MAX_IMAGES = 65535;
constexpr int MAX_FACES = 1 << 26;
constexpr int MAX_CELLS = 128;                              // 128^3 = 2^21 cells: three cluster numbers fit a 63-bit key
constexpr long long MAX_WORDS = 1LL << 28;                  // mask words of the whole batch (2 GiB)
constexpr int ACC = 13;                                     // n, s[3], A00 A01 A02 A11 A12 A22, b[3]
constexpr unsigned long long EMPTY = ~0ull;                 // no key looks like this: a key is < 2^63
using sc_mesh::image_of;
constexpr double SCALE = 16777216.0;                        // 2^24
constexpr double CLAMP = 4096.0;                            // 2^12
static_assert(MAX_CELLS == SC_MESH_SIMPLIFY_MAX_CELLS && ACC == SC_MESH_SIMPLIFY_ACC, "the header states both");

enum { VERTICES_OUT, FACES_OUT, COLLAPSED, CANCELLED, FIELDS };     // rows of counts [SC_MESH_SIMPLIFY_FIELDS][n_images]
static_assert(FIELDS == SC_MESH_SIMPLIFY_FIELDS, "the header states the number of rows");

struct Frame {
    double o[3], h;
    int G;
};

struct Scratch {
    unsigned long long* mask;       // [B][W] a bit per cell
    long long* acc;                 // [V][ACC] per global cluster (an image has at most as many clusters as vertices)
    unsigned long long* keys;       // [T] T = 2 F + B: image b owns slots [2 f_off[b] + b, 2 f_off[b+1] + b + 1)
    long long* c_off;               // [B + 1] running sum of the cluster counts
    int* wprefix;                   // [B][W] occupied cells of the image in front of the word
    int* vcell;                     // [V] cell id, -1 for a bad vertex
    int* ccell;                     // [V] cell id of a global cluster
    int* cnt;                       // [T][2] faces of the group, even / odd
    int* minf;                      // [T][2] lowest global face number of each parity
    int* fcode;                     // [F] 2 slot + odd, -1 for a face that is not in the table
    int* block_cnt;                 // [ceil(F / THREADS)]
    int* block_off;                 // [ceil(F / THREADS)]
};

// q = (p - o) / h of packed vertex gv and its cell; false for a vertex that takes part in nothing
__device__ __forceinline__ bool locate(const float* __restrict__ verts, long long gv, const Frame& fr, double (&q)[3], int (&c)[3]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double p = (double)verts[3 * gv + j];
        q[j] = (p - fr.o[j]) / fr.h;
        ok = ok && isfinite(p) && q[j] >= 0.0 && q[j] <= (double)fr.G;
    }
    if (!ok) return false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int f = (int)floor(q[j]);
        c[j] = f < fr.G - 1 ? f : fr.G - 1;
    }
    return true;
}

__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd((unsigned long long*)p, (unsigned long long)v); }

__device__ __forceinline__ long long fixed(double t) {
    t = t > CLAMP ? CLAMP : (t < -CLAMP ? -CLAMP : t);
    return __double2ll_rn(t * SCALE);
}

__global__ __launch_bounds__(THREADS) void ms_init_kernel(Scratch s, long long words, long long accs, long long T, int B,
                                                          unsigned long long* counts, int* bad_vertex, int* bad_index) {
    const long long step = (long long)gridDim.x * THREADS, t0 = (long long)blockIdx.x * THREADS + threadIdx.x;
    for (long long i = t0; i < words; i += step) s.mask[i] = 0ull;
    for (long long i = t0; i < accs; i += step) s.acc[i] = 0ll;
    for (long long i = t0; i < T; i += step) s.keys[i] = EMPTY;
    for (long long i = t0; i < 2 * T; i += step) s.cnt[i] = 0, s.minf[i] = INT_MAX;
    for (long long i = t0; i < (long long)B * FIELDS; i += step) counts[i] = 0ull;
    if (t0 == 0) *bad_vertex = 0, *bad_index = 0;
}

__global__ __launch_bounds__(THREADS) void ms_mark_kernel(const float* __restrict__ verts, const long long* __restrict__ v_off, int B, int V,
                                                          Frame fr, int W, Scratch s, int* __restrict__ vertex_cluster, int* bad_vertex) {
    for (long long v = (long long)blockIdx.x * THREADS + threadIdx.x; v < V; v += (long long)gridDim.x * THREADS) {
        double q[3];
        int c[3];
        if (!locate(verts, v, fr, q, c)) {
            atomicOr(bad_vertex, 1);
            s.vcell[v] = -1, vertex_cluster[v] = -1;
            continue;
        }
        const int id = (c[0] * fr.G + c[1]) * fr.G + c[2];
        s.vcell[v] = id;
        atomicOr(s.mask + (size_t)image_of(v_off, B, v) * W + (id >> 6), 1ull << (id & 63));
    }
}

// grid: one workgroup per image
__global__ __launch_bounds__(THREADS) void ms_rank_kernel(int W, int B, Scratch s, long long* counts) {
    __shared__ int wave_tot[WAVES];
    const size_t row = (size_t)blockIdx.x * W;
    int carry = 0;
    for (int base = 0; base < W; base += THREADS) {
        const int w = base + threadIdx.x;
        const int c = w < W ? __popcll(s.mask[row + w]) : 0;
        int total;
        const int before = sc_scan::block_exclusive<WAVES>(c, wave_tot, total);
        if (w < W) s.wprefix[row + w] = carry + before;
        carry += total;
        __syncthreads();                                    // wave_tot is written again in the next round
    }
    if (threadIdx.x == 0) counts[(size_t)VERTICES_OUT * B + blockIdx.x] = carry;
}

// grid: one workgroup
__global__ __launch_bounds__(THREADS) void ms_offsets_kernel(int B, const long long* __restrict__ counts, long long* __restrict__ c_off) {
    __shared__ long long wave_tot[WAVES];
    long long carry = 0;
    for (int base = 0; base < B; base += THREADS) {
        const int b = base + threadIdx.x;
        const long long c = b < B ? counts[(size_t)VERTICES_OUT * B + b] : 0;
        long long total;
        const long long before = sc_scan::block_exclusive<WAVES>(c, wave_tot, total);
        if (b < B) c_off[b] = carry + before;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) c_off[B] = carry;
}

__global__ __launch_bounds__(THREADS) void ms_vertex_kernel(const float* __restrict__ verts, const long long* __restrict__ v_off, int B, int V,
                                                            Frame fr, int W, Scratch s, int* __restrict__ vertex_cluster) {
    for (long long v = (long long)blockIdx.x * THREADS + threadIdx.x; v < V; v += (long long)gridDim.x * THREADS) {
        const int id = s.vcell[v];
        if (id < 0) continue;
        const int b = image_of(v_off, B, v);
        const size_t word = (size_t)b * W + (id >> 6);
        const int k = s.wprefix[word] + __popcll(s.mask[word] & ((1ull << (id & 63)) - 1ull));
        vertex_cluster[v] = k;
        const long long gc = s.c_off[b] + k;
        s.ccell[gc] = id;                                   // every writer stores the same word
        double q[3];
        int c[3];
        locate(verts, v, fr, q, c);
        long long* a = s.acc + gc * ACC;
        add64(a, 1);
#pragma unroll
        for (int j = 0; j < 3; ++j) add64(a + 1 + j, __double2ll_rn((q[j] - ((double)c[j] + 0.5)) * SCALE));
    }
}

__global__ __launch_bounds__(THREADS) void ms_face_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B, int F,
                                                          Frame fr, Scratch s, const int* __restrict__ vertex_cluster,
                                                          unsigned long long* counts, int* bad_index) {
    for (long long base = (long long)blockIdx.x * THREADS; base < F; base += (long long)gridDim.x * THREADS) {
        const long long f = base + threadIdx.x;
        int b = -1;
        int v[1] = {0};
        if (f < F) {
            const int img = image_of(f_off, B, f);
            const long long vs = v_off[img], nv = v_off[img + 1] - vs;
            const int i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
            const bool in_range = i[0] >= 0 && i[1] >= 0 && i[2] >= 0 && i[0] < nv && i[1] < nv && i[2] < nv;
            int code = -1;
            if (!in_range) atomicOr(bad_index, 1);
            const bool part = in_range && i[0] != i[1] && i[1] != i[2] && i[0] != i[2] && s.vcell[vs + i[0]] >= 0 && s.vcell[vs + i[1]] >= 0 &&
                              s.vcell[vs + i[2]] >= 0;
            if (part) {
                double q[3][3];
                int c[3][3], k[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) locate(verts, vs + i[r], fr, q[r], c[r]), k[r] = vertex_cluster[vs + i[r]];
                const double e1[3] = {q[1][0] - q[0][0], q[1][1] - q[0][1], q[1][2] - q[0][2]};
                const double e2[3] = {q[2][0] - q[0][0], q[2][1] - q[0][1], q[2][2] - q[0][2]};
                const double N[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
                const long long A[6] = {fixed(N[0] * N[0]), fixed(N[0] * N[1]), fixed(N[0] * N[2]),
                                        fixed(N[1] * N[1]), fixed(N[1] * N[2]), fixed(N[2] * N[2])};
                const long long c0 = s.c_off[img];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    if ((r >= 1 && k[r] == k[0]) || (r == 2 && k[2] == k[1])) continue;     // once to each distinct cluster
                    const double w[3] = {q[0][0] - ((double)c[r][0] + 0.5), q[0][1] - ((double)c[r][1] + 0.5), q[0][2] - ((double)c[r][2] + 0.5)};
                    const double d = (N[0] * w[0] + N[1] * w[1]) + N[2] * w[2];
                    long long* a = s.acc + (c0 + k[r]) * ACC + 4;
#pragma unroll
                    for (int t = 0; t < 6; ++t) add64(a + t, A[t]);
#pragma unroll
                    for (int j = 0; j < 3; ++j) add64(a + 6 + j, fixed(N[j] * d));
                }
                b = img;
                if (k[0] == k[1] || k[1] == k[2] || k[0] == k[2]) {
                    v[0] = 1;                                                               // collapsed
                } else {
                    const int m = k[0] < k[1] ? (k[0] < k[2] ? 0 : 2) : (k[1] < k[2] ? 1 : 2);   // where the lowest stands
                    const unsigned long long lo = (unsigned long long)k[m], n1 = (unsigned long long)k[m == 2 ? 0 : m + 1],
                                             n2 = (unsigned long long)k[m == 0 ? 2 : m - 1];
                    const int odd = n1 > n2;                                                // (lo, hi, mid): the other orientation
                    const unsigned long long key = (lo << 42) | ((odd ? n2 : n1) << 21) | (odd ? n1 : n2);
                    const long long start = 2 * f_off[img] + img, n = 2 * (f_off[img + 1] - f_off[img]) + 1;
                    long long at = (long long)((key * 0x9E3779B97F4A7C15ull >> 20) % (unsigned long long)n);
                    for (long long p = 0; p < n; ++p) {                                     // n > the image's faces: an empty or matching slot comes first
                        const unsigned long long old = atomicCAS(s.keys + start + at, EMPTY, key);
                        if (old == EMPTY || old == key) break;
                        at = at + 1 == n ? 0 : at + 1;
                    }
                    const long long slot = start + at;
                    atomicAdd(s.cnt + 2 * slot + odd, 1);
                    atomicMin(s.minf + 2 * slot + odd, (int)f);
                    code = (int)(2 * slot + odd);
                }
            }
            s.fcode[f] = code;
        }
        const int field[1] = {COLLAPSED};
        sc_mesh::image_add<1>(counts, B, b, field, v);
    }
}

__global__ __launch_bounds__(THREADS) void ms_solve_kernel(int B, Frame fr, double reg, Scratch s, float* __restrict__ verts_out) {
    const long long C = s.c_off[B];
    for (long long g = (long long)blockIdx.x * THREADS + threadIdx.x; g < C; g += (long long)gridDim.x * THREADS) {
        const long long* a = s.acc + g * ACC;
        const double inv = 1.0 / SCALE;                     // 2^-24: the scalings below are exact
        const double n = (double)a[0];
        const double c[3] = {(double)a[1] * inv / n, (double)a[2] * inv / n, (double)a[3] * inv / n};
        double a00 = (double)a[4] * inv, a01 = (double)a[5] * inv, a02 = (double)a[6] * inv, a11 = (double)a[7] * inv,
               a12 = (double)a[8] * inv, a22 = (double)a[9] * inv;
        double b0 = (double)a[10] * inv, b1 = (double)a[11] * inv, b2 = (double)a[12] * inv;
        const double lam = reg * ((a00 + a11) + a22);
        double x[3] = {c[0], c[1], c[2]};
        if (lam > 0.0) {
            a00 = a00 + lam, a11 = a11 + lam, a22 = a22 + lam;
            b0 = b0 + lam * c[0], b1 = b1 + lam * c[1], b2 = b2 + lam * c[2];
            const double l10 = a01 / a00, l20 = a02 / a00;
            const double e1 = a11 - l10 * a01, t21 = a12 - l20 * a01;
            const double l21 = t21 / e1;
            const double e2 = (a22 - l20 * a02) - l21 * t21;
            const double z1 = b1 - l10 * b0, z2 = (b2 - l20 * b0) - l21 * z1;
            x[2] = z2 / e2;
            x[1] = z1 / e1 - l21 * x[2];
            x[0] = (b0 / a00 - l10 * x[1]) - l20 * x[2];
        }
        const int id = s.ccell[g];
        const int cell[3] = {id / (fr.G * fr.G), id / fr.G % fr.G, id % fr.G};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (!(x[j] >= -0.5)) x[j] = -0.5;
            if (!(x[j] <= 0.5)) x[j] = 0.5;
            verts_out[3 * g + j] = (float)(fr.o[j] + (((double)cell[j] + 0.5) + x[j]) * fr.h);
        }
    }
}

// is face f written: the lowest face of its parity in its group, and that parity has strictly more faces than the other
__device__ __forceinline__ bool written(const Scratch& s, long long f, int code) {
    return code >= 0 && s.minf[code] == (int)f && s.cnt[code] > s.cnt[code ^ 1];
}

// grid: one workgroup per THREADS faces
__global__ __launch_bounds__(THREADS) void ms_decide_kernel(const long long* __restrict__ f_off, int B, int F, Scratch s,
                                                            unsigned long long* counts) {
    __shared__ int wave_tot[WAVES];
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int b = -1;
    int v[2] = {0, 0};
    if (f < F) {
        const int code = s.fcode[f];
        if (code >= 0) {
            b = image_of(f_off, B, f);
            v[0] = written(s, f, code), v[1] = !v[0];
        }
    }
    int total;
    sc_scan::block_exclusive<WAVES>(v[0], wave_tot, total);
    if (threadIdx.x == 0) s.block_cnt[blockIdx.x] = total;
    const int field[2] = {FACES_OUT, CANCELLED};
    sc_mesh::image_add<2>(counts, B, b, field, v);
}

// grid: one workgroup
__global__ __launch_bounds__(THREADS) void ms_block_kernel(int blocks, Scratch s) {
    __shared__ int wave_tot[WAVES];
    int carry = 0;
    for (int base = 0; base < blocks; base += THREADS) {
        const int i = base + threadIdx.x;
        const int c = i < blocks ? s.block_cnt[i] : 0;
        int total;
        const int before = sc_scan::block_exclusive<WAVES>(c, wave_tot, total);
        if (i < blocks) s.block_off[i] = carry + before;
        carry += total;
        __syncthreads();
    }
}

// grid: one workgroup per THREADS faces
__global__ __launch_bounds__(THREADS) void ms_emit_kernel(const int* __restrict__ faces, const long long* __restrict__ v_off,
                                                          const long long* __restrict__ f_off, int B, int F, Scratch s,
                                                          const int* __restrict__ vertex_cluster, int* __restrict__ faces_out,
                                                          int* __restrict__ face_source) {
    __shared__ int wave_tot[WAVES];
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    const int keep = f < F && written(s, f, s.fcode[f]);
    int total;
    const int before = sc_scan::block_exclusive<WAVES>(keep, wave_tot, total);
    if (!keep) return;
    const long long at = (long long)s.block_off[blockIdx.x] + before;
    const int b = image_of(f_off, B, f);
    const long long vs = v_off[b];
#pragma unroll
    for (int r = 0; r < 3; ++r) faces_out[3 * at + r] = vertex_cluster[vs + faces[3 * f + r]];
    face_source[at] = (int)(f - f_off[b]);
}

using sc_mesh::align16;
static inline long long words_per_image(int cells) { return ((long long)cells * cells * cells + 63) / 64; }
static inline bool sizes_ok(int n_images, long long n_verts, long long n_faces, int cells) {
    return n_images >= 1 && n_images <= MAX_IMAGES && n_verts >= 0 && n_verts <= INT_MAX && n_faces >= 0 && n_faces <= MAX_FACES &&
           cells >= 1 && cells <= MAX_CELLS && n_images * words_per_image(cells) <= MAX_WORDS;
}
static inline long long face_blocks(long long n_faces) { return (n_faces + THREADS - 1) / THREADS; }

}  // namespace ms
}  // namespace sc

// scratch layout: mask [B W] u64 | acc [V][13] i64 | keys [T] u64 | c_off [B+1] i64 | wprefix [B W] | vcell, ccell [V] | cnt, minf [2T] |
// fcode [F] | block_cnt, block_off [ceil(F / 256)]
extern "C" long long sc_mesh_cluster_simplify_scratch_bytes(int n_images, int n_verts, int n_faces, int cells) {
    using namespace sc::ms;
    if (!sizes_ok(n_images, n_verts, n_faces, cells)) return 0;
    const long long B = n_images, V = n_verts, F = n_faces, words = B * words_per_image(cells), T = 2 * F + B;
    return align16(8 * words) + align16(8 * ACC * V) + align16(8 * T) + align16(8 * (B + 1)) + align16(4 * words) + 2 * align16(4 * V) +
           2 * align16(8 * T) + align16(4 * F) + 2 * align16(4 * face_blocks(F)) + 16;
}

extern "C" int sc_mesh_cluster_simplify(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images,
                                        int n_verts, int n_faces, float origin_x, float origin_y, float origin_z, float pitch, int cells,
                                        double reg, void* scratch, float* verts_out, int32_t* faces_out, int64_t* counts,
                                        int32_t* vertex_cluster, int32_t* face_source, int32_t* bad_vertex, int32_t* bad_index, void* stream_) {
    using namespace sc::ms;
    if (n_images <= 0) return 0;
    const auto finite = [](double x) { return x - x == 0.0; };
    if (!sizes_ok(n_images, n_verts, n_faces, cells) || !v_off || !f_off || !counts || !bad_vertex || !bad_index || !scratch ||
        ((uintptr_t)scratch & 15) || !finite(origin_x) || !finite(origin_y) || !finite(origin_z) || !finite(pitch) || !(pitch > 0.0f) ||
        !finite(reg) || !(reg > 0.0) || (n_verts > 0 && (!verts || !verts_out || !vertex_cluster)) ||
        (n_faces > 0 && (!faces || !faces_out || !face_source)))
        return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = n_images, V = n_verts, F = n_faces;
    const long long Wl = words_per_image(cells), words = (long long)B * Wl, T = 2LL * F + B, FB = face_blocks(F);
    const int W = (int)Wl;
    sc_mesh::Carver ws{(char*)scratch};
    Scratch s;
    ws.take(s.mask, words);
    ws.take(s.acc, (long long)ACC * V);
    ws.take(s.keys, T);
    ws.take(s.c_off, B + 1LL);
    ws.take(s.wprefix, words);
    ws.take(s.vcell, V), ws.take(s.ccell, V);
    ws.take(s.cnt, 2 * T), ws.take(s.minf, 2 * T);
    ws.take(s.fcode, F);
    ws.take(s.block_cnt, FB), ws.take(s.block_off, FB);
    Frame fr;
    fr.o[0] = (double)origin_x, fr.o[1] = (double)origin_y, fr.o[2] = (double)origin_z, fr.h = (double)pitch, fr.G = cells;
    constexpr auto blocks = sc_mesh::blocks<THREADS, MAX_BLOCKS>;
    const long long *vo = (const long long*)v_off, *fo = (const long long*)f_off;
    unsigned long long* acc = (unsigned long long*)counts;
    long long widest = words > (long long)ACC * V ? words : (long long)ACC * V;
    widest = widest > 2 * T ? widest : 2 * T;
    hipLaunchKernelGGL(ms_init_kernel, dim3(blocks(widest)), dim3(THREADS), 0, stream, s, words, (long long)ACC * V, T, B, acc, bad_vertex,
                       bad_index);
    if (V > 0)
        hipLaunchKernelGGL(ms_mark_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, verts, vo, B, V, fr, W, s, vertex_cluster, bad_vertex);
    hipLaunchKernelGGL(ms_rank_kernel, dim3((unsigned)B), dim3(THREADS), 0, stream, W, B, s, (long long*)counts);
    hipLaunchKernelGGL(ms_offsets_kernel, dim3(1), dim3(THREADS), 0, stream, B, (const long long*)counts, s.c_off);
    if (V > 0)
        hipLaunchKernelGGL(ms_vertex_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, verts, vo, B, V, fr, W, s, vertex_cluster);
    if (F > 0)
        hipLaunchKernelGGL(ms_face_kernel, dim3(blocks(F)), dim3(THREADS), 0, stream, verts, faces, vo, fo, B, F, fr, s,
                           (const int*)vertex_cluster, acc, bad_index);
    if (V > 0) hipLaunchKernelGGL(ms_solve_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, B, fr, reg, s, verts_out);
    if (F > 0) {
        hipLaunchKernelGGL(ms_decide_kernel, dim3((unsigned)FB), dim3(THREADS), 0, stream, fo, B, F, s, acc);
        hipLaunchKernelGGL(ms_block_kernel, dim3(1), dim3(THREADS), 0, stream, (int)FB, s);
        hipLaunchKernelGGL(ms_emit_kernel, dim3((unsigned)FB), dim3(THREADS), 0, stream, faces, vo, fo, B, F, s, (const int*)vertex_cluster,
                           faces_out, face_source);
    }
    return (int)hipGetLastError();
}
