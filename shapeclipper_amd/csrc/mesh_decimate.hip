// mesh_decimate.hip -- one round of quadric edge-collapse decimation of a batch of indexed triangle meshes towards a face budget, and the
// final vertex compaction (ops.mesh_decimate, the evaluation's {idx}_mesh_decimated.ply; definitions in include/shapeclipper_hip.h,
// sc_mesh_decimate_round and sc_mesh_decimate_compact; restated in numpy by tests/mesh_decimate_ref.py).  Built without contraction: every
// float64 operation of the quadrics, the solve, the cost and the flip test rounds once.
//
// sc_mesh_decimate_round: 14 launches on one stream (3 when n_faces == 0), no spin barrier, no cooperative launch, no host read:
//   1. dc_init_kernel     the edge table (keys empty, count 0, owner and omin INT_MAX, omax -1, state 0), the per-vertex degree, cursor,
//                         fixed and claim words, the per-image list lengths, the counts, the three flags.
//   2. dc_insert_kernel   a thread per face: range and repeated-index check, then its three undirected edges go into the table of
//                         mesh_edges.hpp (count, owner, omin, omax by integer atomics, as mesh_subdivide.hip).
//   3. dc_scan_kernel     ONE workgroup: row[i] = the exclusive running sum of the degrees.
//   4. dc_fill_kernel     the rows in arrival order; an edge whose count is not 2 fixes both its ends (fill_rows).
//   5. dc_rows_kernel     a thread per vertex: the finite check, its row in ASCENDING order (sort_rows), the fixed count.
//   6. dc_quadric_kernel  a thread per vertex: the slot of every ring edge (edge_find) and Q_v, summed in ring order.
//   7. dc_cost_kernel     a thread per table slot: candidate or not (link condition by a merge of the two sorted rows), the LDL^T target,
//                         the cost, the key.
//   8. dc_flip_kernel     a thread per face corner: walks the corner's ring and marks the candidates that would flip this face.
//   9. dc_claim_kernel    a thread per slot: a valid candidate's 64-bit atomicMin on the claim word of its closed neighbourhood.
//  10. dc_select_kernel   a thread per slot: selected iff it holds every claim; appended to its image's list (the list ORDER is
//                         arbitrary and never read: only the keys' ranks are).
//  11. dc_apply_kernel    a workgroup per image: when more are selected than needed, an all-pairs rank over the list staged in LDS; the
//                         edges that go move their survivor and point the other end at it.
//  12. dc_decide_kernel, 13. dc_block_kernel, 14. dc_emit_kernel: block-scan compaction of the faces that do not hold both ends of a
//                         collapsed edge, remapped, in their order.
// sc_mesh_decimate_compact: 4 launches: the vertices still referenced in ascending number, the faces renumbered, the map of every input
// vertex through the chain of its survivors.
// mesh_edges.hpp states why every probe ends and why the sorted rows keep no trace of the arrival order.  Only integer atomics decide
// anything and no float is accumulated by an atomic: the same bits run to run, for any batch, stream and table size.  Ties between equal
// costs break by owner (the lowest half-edge), so the result is NOT invariant under a permutation of the faces.
// Bound: launch latency and the one host read a round; the number of rounds is the cost (docs/LAB_NOTEBOOK.md).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "shapeclipper_hip.h"
#include "mesh_edges.hpp"

namespace sc {
namespace dc {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;
constexpr int SCAN_THREADS = 1024;                          // the one workgroup of the scans
constexpr int SCAN_ITEMS = 8;
constexpr int APPLY_THREADS = 1024;                         // the workgroup of an image's budget and collapses
constexpr int SHORT_ROW = 32;
constexpr int MAX_BLOCKS = 4096;
constexpr int MAX_IMAGES = 65535;
constexpr int MAX_FACES = 1 << 26;
constexpr int MAX_VERTS = 1 << 30;
using sc_mesh::EMPTY;
using sc_mesh::image_of;

enum { FACES_OUT, SELECTED, COLLAPSED, CANDIDATES, REJECTED_LINK, REJECTED_FLIP, FIXED_VERTICES, FIELDS };      // rows of counts
static_assert(FIELDS == SC_MESH_DECIMATE_FIELDS, "the header states the number of rows");
enum { NONE = 0, VALID = 1, FLIPS = 2 };                    // an edge slot's state

struct Scratch : sc_mesh::Rings {
    int *owner, *omin, *omax;       // [T] the edge's lowest half-edge, its lowest and highest opposite vertex (global)
    int* state;                     // [T]
    unsigned long long* ekey;       // [T] (cost bits << 32) | owner of a candidate
    float* target;                  // [T][3] where a candidate's survivor goes, rounded to fp32
    int* rslot;                     // [6 F] the slot of the edge to nbr[r]
    double* Q;                      // [V][10] A00 A01 A02 A11 A12 A22 b0 b1 b2 c
    unsigned long long* claim;      // [V]
    int* fok;                       // [F] 0 for a face that takes part in nothing
    unsigned long long* lkey;       // [3 F] image b's selected keys at 3 f_off[b] ...
    int* lslot;                     // [3 F] ... and their slots
    int* sel_n;                     // [B]
    int *block_cnt, *block_off;     // [ceil(F / THREADS)]
};

__global__ __launch_bounds__(THREADS) void dc_init_kernel(Scratch s, int T, int V, int B, unsigned long long* counts, int* flags) {
    const int step = gridDim.x * THREADS, t0 = blockIdx.x * THREADS + threadIdx.x;
    for (int i = t0; i < T; i += step)
        s.keys[i] = EMPTY, s.count[i] = 0, s.owner[i] = INT_MAX, s.omin[i] = INT_MAX, s.omax[i] = -1, s.state[i] = NONE;
    for (int i = t0; i < V; i += step) s.deg[i] = 0, s.cursor[i] = 0, s.fixed[i] = 0, s.claim[i] = ~0ull;
    for (int i = t0; i < B; i += step) s.sel_n[i] = 0;
    for (int i = t0; i < B * FIELDS; i += step) counts[i] = 0ull;
    if (t0 < 3) flags[t0] = 0;
}

__global__ __launch_bounds__(THREADS) void dc_insert_kernel(const int* __restrict__ faces, const long long* __restrict__ v_off,
                                                            const long long* __restrict__ f_off, int B, int F, Scratch s, int T, int shift,
                                                            int* flags) {
    for (int f = blockIdx.x * THREADS + threadIdx.x; f < F; f += gridDim.x * THREADS) {
        const int b = image_of(f_off, B, f);
        const long long vs = v_off[b], nv = v_off[b + 1] - vs;
        const int i[3] = {faces[3 * f], faces[3 * f + 1], faces[3 * f + 2]};
        const bool in_range = i[0] >= 0 && i[1] >= 0 && i[2] >= 0 && i[0] < nv && i[1] < nv && i[2] < nv;
        if (!in_range || i[0] == i[1] || i[1] == i[2] || i[2] == i[0]) {
            atomicOr(flags + (in_range ? 2 : 1), 1);        // takes part in nothing
            s.fok[f] = 0;
            continue;
        }
        s.fok[f] = 1;
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
        }
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void dc_scan_kernel(Scratch s, int V) {
    __shared__ int wave_tot[SCAN_THREADS / 64];
    sc_mesh::scan_array<SCAN_THREADS, SCAN_ITEMS>(s.deg, s.row, V, wave_tot);
}

__global__ __launch_bounds__(THREADS) void dc_fill_kernel(Scratch s, int T) { sc_mesh::fill_rows<THREADS, false>(s, T); }

__global__ __launch_bounds__(THREADS) void dc_rows_kernel(const float* __restrict__ verts, const long long* __restrict__ v_off, int B, Scratch s,
                                                          int V, unsigned char* __restrict__ fixed_out, unsigned long long* counts, int* flags) {
    for (int base = blockIdx.x * THREADS; base < V; base += gridDim.x * THREADS) {   // wave-uniform: the waves cooperate below
        const int i = base + threadIdx.x;
        int r0 = 0, d = 0, b = -1;
        int v[1] = {0};
        if (i < V) {
            r0 = s.row[i], d = s.row[i + 1] - r0;
            bool finite = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) finite = finite && sc_mesh::finite(verts[3 * (size_t)i + c]);
            if (!finite) atomicOr(flags, 1);
            v[0] = s.fixed[i] != 0;
            if (fixed_out) fixed_out[i] = (unsigned char)v[0];
            if (v[0]) b = image_of(v_off, B, i);
        }
        sc_mesh::sort_rows<SHORT_ROW>(s, r0, d);
        const int field[1] = {FIXED_VERTICES};
        sc_mesh::image_add<1>(counts, B, b, field, v);
    }
}

struct P3 {
    double x, y, z;
};
__device__ __forceinline__ P3 load(const float* __restrict__ verts, int v) {
    const size_t j = 3 * (size_t)v;
    return {(double)verts[j], (double)verts[j + 1], (double)verts[j + 2]};
}
__device__ __forceinline__ P3 sub(const P3& a, const P3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ P3 cross(const P3& a, const P3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(const P3& a, const P3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// q += the ten terms of triangle (v, u, w) for vertex v at p
__device__ __forceinline__ void add_terms(double (&q)[10], const P3& p, const P3& xu, const P3& xw) {
    const P3 N = cross(sub(xu, p), sub(xw, p));
    const double d = dot(N, p);
    q[0] = q[0] + N.x * N.x, q[1] = q[1] + N.x * N.y, q[2] = q[2] + N.x * N.z;
    q[3] = q[3] + N.y * N.y, q[4] = q[4] + N.y * N.z, q[5] = q[5] + N.z * N.z;
    q[6] = q[6] + N.x * d, q[7] = q[7] + N.y * d, q[8] = q[8] + N.z * d;
    q[9] = q[9] + d * d;
}

__global__ __launch_bounds__(THREADS) void dc_quadric_kernel(const float* __restrict__ verts, Scratch s, int V, int T, int shift) {
    for (int v = blockIdx.x * THREADS + threadIdx.x; v < V; v += gridDim.x * THREADS) {
        double q[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const P3 p = load(verts, v);
        for (int r = s.row[v]; r < s.row[v + 1]; ++r) {     // ascending neighbour, then omin, omax of the edge
            const int u = s.nbr[r];
            const int at = sc_mesh::edge_find(s.keys, T, shift, (unsigned long long)(v < u ? v : u), (unsigned long long)(v < u ? u : v));
            s.rslot[r] = at;
            if (at < 0) continue;                           // never: the row came from the table
            const P3 xu = load(verts, u);
            const int w0 = s.omin[at], w1 = s.omax[at];
            add_terms(q, p, xu, load(verts, w0));
            if (w1 != w0) add_terms(q, p, xu, load(verts, w1));
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) s.Q[10 * (size_t)v + k] = q[k];
    }
}

__device__ __forceinline__ bool finite64(double x) { return x - x == 0.0; }

__global__ __launch_bounds__(THREADS) void dc_cost_kernel(const float* __restrict__ verts, const long long* __restrict__ v_off, int B, Scratch s,
                                                          int T, double reg, unsigned long long* counts) {
    for (int base = blockIdx.x * THREADS; base < T; base += gridDim.x * THREADS) {   // wave-uniform: image_add
        const int i = base + threadIdx.x;
        int b = -1;
        int n[2] = {0, 0};                                  // candidates, rejected_link
        const unsigned long long key = i < T ? s.keys[i] : EMPTY;
        if (key != EMPTY) {
            const int lo = (int)(key >> 32), hi = (int)(key & 0xFFFFFFFFull);
            const bool fa = s.fixed[lo] != 0, fb = s.fixed[hi] != 0;
            if (s.count[i] == 2 && !(fa && fb)) {
                b = image_of(v_off, B, lo);
                const int a0 = s.row[lo], a1 = s.row[lo + 1], b0 = s.row[hi], b1 = s.row[hi + 1];
                int common = 0;
                for (int p = a0, q = b0; p < a1 && q < b1;) {           // both rows ascend
                    const int x = s.nbr[p], y = s.nbr[q];
                    common += x == y, p += x <= y, q += y <= x;
                }
                if (common == 2 && !(a1 - a0 == 3 && b1 - b0 == 3)) {
                    n[0] = 1;
                    double A[10];
#pragma unroll
                    for (int k = 0; k < 10; ++k) A[k] = s.Q[10 * (size_t)lo + k] + s.Q[10 * (size_t)hi + k];
                    const P3 xa = load(verts, lo), xb = load(verts, hi);
                    const double m[3] = {0.5 * (xa.x + xb.x), 0.5 * (xa.y + xb.y), 0.5 * (xa.z + xb.z)};
                    double x[3] = {m[0], m[1], m[2]};
                    if (fa) {
                        x[0] = xa.x, x[1] = xa.y, x[2] = xa.z;
                    } else if (fb) {
                        x[0] = xb.x, x[1] = xb.y, x[2] = xb.z;
                    } else {
                        const double lam = reg * ((A[0] + A[3]) + A[5]);
                        if (lam > 0.0) {
                            const double d00 = A[0] + lam, d11 = A[3] + lam, d22 = A[5] + lam;
                            const double r0 = A[6] + lam * m[0], r1 = A[7] + lam * m[1], r2 = A[8] + lam * m[2];
                            const double l10 = A[1] / d00, l20 = A[2] / d00;
                            const double e1 = d11 - l10 * A[1], t21 = A[4] - l20 * A[1];
                            const double l21 = t21 / e1;
                            const double e2 = (d22 - l20 * A[2]) - l21 * t21;
                            const double z1 = r1 - l10 * r0;
                            const double z2 = (r2 - l20 * r0) - l21 * z1;
                            const double x2 = z2 / e2;
                            const double x1 = z1 / e1 - l21 * x2;
                            const double x0 = (r0 / d00 - l10 * x1) - l20 * x2;
                            if (finite64(x0) && finite64(x1) && finite64(x2)) x[0] = x0, x[1] = x1, x[2] = x2;
                        }
                    }
                    const double ax0 = (A[0] * x[0] + A[1] * x[1]) + A[2] * x[2];
                    const double ax1 = (A[1] * x[0] + A[3] * x[1]) + A[4] * x[2];
                    const double ax2 = (A[2] * x[0] + A[4] * x[1]) + A[5] * x[2];
                    const double xax = (x[0] * ax0 + x[1] * ax1) + x[2] * ax2;
                    const double bx = (A[6] * x[0] + A[7] * x[1]) + A[8] * x[2];
                    double cost = (xax - 2.0 * bx) + A[9];
                    if (!(cost > 0.0)) cost = 0.0;
                    s.ekey[i] = ((unsigned long long)__float_as_uint((float)cost) << 32) | (unsigned long long)s.owner[i];
#pragma unroll
                    for (int c = 0; c < 3; ++c) s.target[3 * (size_t)i + c] = (float)x[c];
                    s.state[i] = VALID;
                } else {
                    n[1] = 1;
                }
            }
        }
        const int field[2] = {CANDIDATES, REJECTED_LINK};
        sc_mesh::image_add<2>(counts, B, b, field, n);
    }
}

// a thread per face corner: would the face, with this corner at the target of a candidate edge of the corner's ring, turn over?
__global__ __launch_bounds__(THREADS) void dc_flip_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B, int F,
                                                          Scratch s) {
    for (long long h = (long long)blockIdx.x * THREADS + threadIdx.x; h < 3LL * F; h += (long long)gridDim.x * THREADS) {
        const int f = (int)(h / 3), c = (int)(h - 3LL * f);
        if (!s.fok[f]) continue;
        const int vs = (int)v_off[image_of(f_off, B, f)];
        const int g0 = vs + faces[3 * f], g1 = vs + faces[3 * f + 1], g2 = vs + faces[3 * f + 2];
        const int v = c == 0 ? g0 : c == 1 ? g1 : g2, p = c == 0 ? g1 : c == 1 ? g2 : g0, q = c == 0 ? g2 : c == 1 ? g0 : g1;
        if (s.fixed[v]) continue;                           // never moves
        const P3 P0 = load(verts, g0), P1 = load(verts, g1), P2 = load(verts, g2);
        const P3 N = cross(sub(P1, P0), sub(P2, P0));
        for (int r = s.row[v]; r < s.row[v + 1]; ++r) {
            const int u = s.nbr[r];
            if (u == p || u == q) continue;                 // the face holds both ends: it goes with the edge
            const int at = s.rslot[r];
            if (at < 0 || s.state[at] != VALID) continue;   // (a slot another thread has marked already is skipped or marked again)
            const P3 t = {(double)s.target[3 * (size_t)at], (double)s.target[3 * (size_t)at + 1], (double)s.target[3 * (size_t)at + 2]};
            const P3 M0 = c == 0 ? t : P0, M1 = c == 1 ? t : P1, M2 = c == 2 ? t : P2;
            const P3 N2 = cross(sub(M1, M0), sub(M2, M0));
            if (!(dot(N2, N) > 0.0)) s.state[at] = FLIPS;   // every writer stores the same word
        }
    }
}

// f(vertex) over the closed neighbourhood of edge (lo, hi): ring(lo) holds hi and ring(hi) holds lo
template <class Fn>
__device__ __forceinline__ void closed_neighbourhood(const Scratch& s, int lo, int hi, Fn f) {
    for (int r = s.row[lo]; r < s.row[lo + 1]; ++r) f(s.nbr[r]);
    for (int r = s.row[hi]; r < s.row[hi + 1]; ++r) f(s.nbr[r]);
}

__global__ __launch_bounds__(THREADS) void dc_claim_kernel(const long long* __restrict__ v_off, int B, Scratch s, int T,
                                                           unsigned long long* counts) {
    for (int base = blockIdx.x * THREADS; base < T; base += gridDim.x * THREADS) {   // wave-uniform: image_add
        const int i = base + threadIdx.x;
        int b = -1;
        int n[1] = {0};
        const int state = i < T ? s.state[i] : NONE;
        if (state != NONE) {
            const unsigned long long key = s.keys[i];
            const int lo = (int)(key >> 32), hi = (int)(key & 0xFFFFFFFFull);
            if (state == FLIPS) {
                n[0] = 1, b = image_of(v_off, B, lo);
            } else {
                const unsigned long long mine = s.ekey[i];
                closed_neighbourhood(s, lo, hi, [&](int v) { atomicMin(s.claim + v, mine); });
            }
        }
        const int field[1] = {REJECTED_FLIP};
        sc_mesh::image_add<1>(counts, B, b, field, n);
    }
}

__global__ __launch_bounds__(THREADS) void dc_select_kernel(const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B,
                                                            Scratch s, int T) {
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < T; i += gridDim.x * THREADS) {
        if (s.state[i] != VALID) continue;
        const unsigned long long key = s.keys[i], mine = s.ekey[i];
        const int lo = (int)(key >> 32), hi = (int)(key & 0xFFFFFFFFull);
        bool all = true;
        closed_neighbourhood(s, lo, hi, [&](int v) { all = all && s.claim[v] == mine; });
        if (!all) continue;
        const int b = image_of(v_off, B, lo);
        const long long at = 3 * f_off[b] + atomicAdd(s.sel_n + b, 1);              // an image has at most 3 F_b edges
        s.lkey[at] = mine, s.lslot[at] = i;
    }
}

// grid: one workgroup per image
__global__ __launch_bounds__(APPLY_THREADS) void dc_apply_kernel(float* __restrict__ verts, const long long* __restrict__ f_off, int target,
                                                                 Scratch s, int* __restrict__ parent, long long* __restrict__ counts) {
    __shared__ unsigned long long tile[APPLY_THREADS];
    __shared__ int done;
    const int b = blockIdx.x, B = gridDim.x;
    const long long first = 3 * f_off[b], Fb = f_off[b + 1] - f_off[b];
    const int n = s.sel_n[b];
    const long long need = Fb > target ? (Fb - target + 1) / 2 : 0;
    if (threadIdx.x == 0) done = 0;
    __syncthreads();
    for (int base = 0; base < n; base += APPLY_THREADS) {   // workgroup-uniform
        const int t = base + threadIdx.x;
        const unsigned long long mine = t < n ? s.lkey[first + t] : ~0ull;
        long long rank = 0;
        if (n > need) {                                     // only such a round ranks: the keys of an image are distinct
            for (int from = 0; from < n; from += APPLY_THREADS) {
                __syncthreads();
                tile[threadIdx.x] = from + threadIdx.x < n ? s.lkey[first + from + threadIdx.x] : ~0ull;
                __syncthreads();
                const int m = n - from < APPLY_THREADS ? n - from : APPLY_THREADS;
                for (int j = 0; j < m; ++j) rank += tile[j] < mine;
            }
        }
        if (t < n && rank < need) {
            const int at = s.lslot[first + t];
            const unsigned long long key = s.keys[at];
            const int lo = (int)(key >> 32), hi = (int)(key & 0xFFFFFFFFull);
            const bool keep_hi = s.fixed[hi] != 0 && s.fixed[lo] == 0;              // the survivor: the fixed end, else the lower number
            const int sv = keep_hi ? hi : lo, rv = keep_hi ? lo : hi;
            if (!s.fixed[sv]) {
#pragma unroll
                for (int c = 0; c < 3; ++c) verts[3 * (size_t)sv + c] = s.target[3 * (size_t)at + c];
            }
            parent[rv] = sv;
            atomicAdd(&done, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[(size_t)SELECTED * B + b] = n, counts[(size_t)COLLAPSED * B + b] = done;
}

// the face's corners after the round, image-local; false for a face that holds both ends of a collapsed edge
__device__ __forceinline__ bool remapped(const int* __restrict__ faces, const int* __restrict__ parent, int vs, const Scratch& s, int f,
                                         int (&m)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = faces[3 * (size_t)f + c];
    if (!s.fok[f]) return true;                             // a refused face is passed on: the caller raises
#pragma unroll
    for (int c = 0; c < 3; ++c) m[c] = parent[vs + m[c]] - vs;
    return m[0] != m[1] && m[1] != m[2] && m[2] != m[0];
}

// grid: one workgroup per THREADS faces
__global__ __launch_bounds__(THREADS) void dc_decide_kernel(const int* __restrict__ faces, const int* __restrict__ parent,
                                                            const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B, int F,
                                                            Scratch s) {
    __shared__ int wave_tot[WAVES];
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int keep = 0, m[3];
    if (f < F) keep = remapped(faces, parent, (int)v_off[image_of(f_off, B, f)], s, (int)f, m);
    int total;
    sc_scan::block_exclusive<WAVES>(keep, wave_tot, total);
    if (threadIdx.x == 0) s.block_cnt[blockIdx.x] = total;
}

// grid: one workgroup
__global__ __launch_bounds__(THREADS) void dc_block_kernel(int blocks, Scratch s) {
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
__global__ __launch_bounds__(THREADS) void dc_emit_kernel(const int* __restrict__ faces, const int* __restrict__ parent,
                                                          const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B, int F,
                                                          Scratch s, int* __restrict__ faces_out, unsigned long long* counts) {
    __shared__ int wave_tot[WAVES];
    const long long f = (long long)blockIdx.x * THREADS + threadIdx.x;
    int b = -1, m[3];
    int keep[1] = {0};
    if (f < F) {
        const int img = image_of(f_off, B, f);
        keep[0] = remapped(faces, parent, (int)v_off[img], s, (int)f, m);
        if (keep[0]) b = img;
    }
    int total;
    const int before = sc_scan::block_exclusive<WAVES>(keep[0], wave_tot, total);
    if (keep[0]) {
        const size_t out = 3 * ((size_t)s.block_off[blockIdx.x] + before);
        faces_out[out] = m[0], faces_out[out + 1] = m[1], faces_out[out + 2] = m[2];
    }
    const int field[1] = {FACES_OUT};
    sc_mesh::image_add<1>(counts, B, b, field, keep);
}

// ---- the final compaction ---------------------------------------------------------------------------------------------------------
struct Compact {
    int *used, *rank;               // [V + 1]
};

__global__ __launch_bounds__(THREADS) void cp_init_kernel(Compact s, int V) {
    for (int i = blockIdx.x * THREADS + threadIdx.x; i <= V; i += gridDim.x * THREADS) s.used[i] = 0;
}

__global__ __launch_bounds__(THREADS) void cp_mark_kernel(const int* __restrict__ faces, const long long* __restrict__ v_off,
                                                          const long long* __restrict__ f_off, int B, int F, Compact s) {
    for (long long h = (long long)blockIdx.x * THREADS + threadIdx.x; h < 3LL * F; h += (long long)gridDim.x * THREADS) {
        const int b = image_of(f_off, B, h / 3);
        const long long vs = v_off[b], nv = v_off[b + 1] - vs;
        const int i = faces[h];
        if (i >= 0 && i < nv) s.used[vs + i] = 1;           // every writer stores the same word
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void cp_scan_kernel(Compact s, int V) {
    __shared__ int wave_tot[SCAN_THREADS / 64];
    sc_mesh::scan_array<SCAN_THREADS, SCAN_ITEMS>(s.used, s.rank, V, wave_tot);
}

__global__ __launch_bounds__(THREADS) void cp_emit_kernel(const float* __restrict__ verts, const int* __restrict__ faces,
                                                          const long long* __restrict__ v_off, const long long* __restrict__ f_off, int B,
                                                          int V, int F, const int* __restrict__ parent,
                                                          const unsigned char* __restrict__ fixed, Compact s, float* __restrict__ verts_out,
                                                          int* __restrict__ faces_out, int* __restrict__ vertex_map,
                                                          unsigned char* __restrict__ fixed_out, long long* __restrict__ v_count_out) {
    const long long step = (long long)gridDim.x * THREADS, t0 = (long long)blockIdx.x * THREADS + threadIdx.x;
    for (long long i = t0; i < V; i += step) {
        if (s.used[i]) {
            const size_t out = (size_t)s.rank[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) verts_out[3 * out + c] = verts[3 * (size_t)i + c];
            fixed_out[out] = fixed[i];
        }
        int r = (int)i;                                     // the survivor at the end of the chain; a parent outside [0, V) ends it
        for (int hop = 0; hop < V; ++hop) {
            const int p = parent[r];
            if (p == r || p < 0 || p >= V) break;
            r = p;
        }
        const int b = image_of(v_off, B, i);
        const long long vs = v_off[b];
        vertex_map[i] = s.used[r] && r >= vs && r < v_off[b + 1] ? s.rank[r] - s.rank[vs] : -1;
    }
    for (long long h = t0; h < 3LL * F; h += step) {
        const int b = image_of(f_off, B, h / 3);
        const long long vs = v_off[b], nv = v_off[b + 1] - vs;
        const int i = faces[h];
        faces_out[h] = i >= 0 && i < nv ? s.rank[vs + i] - s.rank[vs] : 0;
    }
    for (long long b = t0; b < B; b += step) v_count_out[b] = s.rank[v_off[b + 1]] - s.rank[v_off[b]];
}

using sc_mesh::align16;
static inline bool sizes_ok(int n_images, long long n_verts, long long n_faces, long long table_slots) {
    return n_images >= 1 && n_images <= MAX_IMAGES && n_verts >= 0 && n_verts <= MAX_VERTS && n_faces >= 0 && n_faces <= MAX_FACES &&
           sc_mesh::slots_ok(table_slots, n_faces);
}
constexpr auto blocks = sc_mesh::blocks<THREADS, MAX_BLOCKS>;
static inline long long face_blocks(long long F) { return (F + THREADS - 1) / THREADS; }

}  // namespace dc
}  // namespace sc

// scratch layout: keys, ekey [T] u64 | count, owner, omin, omax, state [T] | target [3 T] f32 | deg, cursor, fixed [V] | row [V + 1] |
// raw, nbr, rslot [6 F] | Q [10 V] f64 | claim [V] u64 | fok [F] | lkey [3 F] u64 | lslot [3 F] | sel_n [B] | block_cnt, block_off
// [ceil(F / 256)].  sc_mesh_decimate_compact carves used, rank [V + 1] from the start of the same buffer.
extern "C" long long sc_mesh_decimate_scratch_bytes(int n_images, int n_verts, int n_faces, int table_slots) {
    using namespace sc::dc;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots)) return 0;
    const long long T = table_slots, F = n_faces, V = n_verts, B = n_images, K = face_blocks(F);
    return 2 * align16(8 * T) + 5 * align16(4 * T) + align16(12 * T) + 3 * align16(4 * V) + align16(4 * (V + 1)) + 3 * align16(24 * F) +
           align16(80 * V) + align16(8 * V) + align16(4 * F) + align16(24 * F) + align16(12 * F) + align16(4 * B) + 2 * align16(4 * K) + 16;
}

extern "C" int sc_mesh_decimate_round(float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images,
                                      int n_verts, int n_faces, int table_slots, int target_faces, double reg, void* scratch,
                                      int32_t* parent, int32_t* faces_out, uint8_t* fixed_out, int64_t* counts, int32_t* flags,
                                      void* stream_) {
    using namespace sc::dc;
    if (n_images <= 0) return 0;
    if (!sizes_ok(n_images, n_verts, n_faces, table_slots) || !v_off || !f_off || !counts || !flags || !scratch || ((uintptr_t)scratch & 15) ||
        target_faces < 0 || !(reg > 0.0) || (n_verts > 0 && (!verts || !parent)) || (n_faces > 0 && (!faces || !faces_out)))
        return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = n_images, V = n_verts, F = n_faces, T = table_slots;
    const int shift = sc_mesh::table_shift(T);
    const long long K = face_blocks(F);
    sc_mesh::Carver ws{(char*)scratch};
    Scratch s;
    ws.take(s.keys, T), ws.take(s.ekey, T);
    ws.take(s.count, T), ws.take(s.owner, T), ws.take(s.omin, T), ws.take(s.omax, T), ws.take(s.state, T);
    ws.take(s.target, 3LL * T);
    ws.take(s.deg, V), ws.take(s.cursor, V), ws.take(s.fixed, V);
    ws.take(s.row, V + 1LL);
    ws.take(s.raw, 6LL * F), ws.take(s.nbr, 6LL * F), ws.take(s.rslot, 6LL * F);
    ws.take(s.Q, 10LL * V);
    ws.take(s.claim, V);
    ws.take(s.fok, F);
    ws.take(s.lkey, 3LL * F), ws.take(s.lslot, 3LL * F);
    ws.take(s.sel_n, B);
    ws.take(s.block_cnt, K), ws.take(s.block_off, K);
    const long long *vo = (const long long*)v_off, *fo = (const long long*)f_off;
    unsigned long long* cnt = (unsigned long long*)counts;
    const long long most = T > V ? T : V;
    hipLaunchKernelGGL(dc_init_kernel, dim3(blocks(most > B * FIELDS ? most : B * FIELDS)), dim3(THREADS), 0, stream, s, T, V, B, cnt, flags);
    if (F > 0) hipLaunchKernelGGL(dc_insert_kernel, dim3(blocks(F)), dim3(THREADS), 0, stream, faces, vo, fo, B, F, s, T, shift, flags);
    hipLaunchKernelGGL(dc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, s, V);
    if (F > 0) hipLaunchKernelGGL(dc_fill_kernel, dim3(blocks(T)), dim3(THREADS), 0, stream, s, T);
    if (V > 0) hipLaunchKernelGGL(dc_rows_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, verts, vo, B, s, V, fixed_out, cnt, flags);
    if (F > 0) {
        hipLaunchKernelGGL(dc_quadric_kernel, dim3(blocks(V)), dim3(THREADS), 0, stream, verts, s, V, T, shift);
        hipLaunchKernelGGL(dc_cost_kernel, dim3(blocks(T)), dim3(THREADS), 0, stream, verts, vo, B, s, T, reg, cnt);
        hipLaunchKernelGGL(dc_flip_kernel, dim3(blocks(3LL * F)), dim3(THREADS), 0, stream, verts, faces, vo, fo, B, F, s);
        hipLaunchKernelGGL(dc_claim_kernel, dim3(blocks(T)), dim3(THREADS), 0, stream, vo, B, s, T, cnt);
        hipLaunchKernelGGL(dc_select_kernel, dim3(blocks(T)), dim3(THREADS), 0, stream, vo, fo, B, s, T);
        hipLaunchKernelGGL(dc_apply_kernel, dim3((unsigned)B), dim3(APPLY_THREADS), 0, stream, verts, fo, target_faces, s, parent,
                           (long long*)counts);
        hipLaunchKernelGGL(dc_decide_kernel, dim3((unsigned)K), dim3(THREADS), 0, stream, faces, parent, vo, fo, B, F, s);
        hipLaunchKernelGGL(dc_block_kernel, dim3(1), dim3(THREADS), 0, stream, (int)K, s);
        hipLaunchKernelGGL(dc_emit_kernel, dim3((unsigned)K), dim3(THREADS), 0, stream, faces, parent, vo, fo, B, F, s, faces_out, cnt);
    }
    return (int)hipGetLastError();
}

extern "C" int sc_mesh_decimate_compact(const float* verts, const int32_t* faces, const int64_t* v_off, const int64_t* f_off, int n_images,
                                        int n_verts, int n_faces, const int32_t* parent, const uint8_t* fixed, void* scratch,
                                        float* verts_out, int32_t* faces_out, int32_t* vertex_map, uint8_t* fixed_out, int64_t* v_count_out,
                                        void* stream_) {
    using namespace sc::dc;
    if (n_images <= 0) return 0;
    if (n_images > MAX_IMAGES || n_verts < 0 || n_verts > MAX_VERTS || n_faces < 0 || n_faces > MAX_FACES || !v_off || !f_off || !v_count_out ||
        !scratch || ((uintptr_t)scratch & 15) || (n_verts > 0 && (!verts || !parent || !fixed || !verts_out || !vertex_map || !fixed_out)) ||
        (n_faces > 0 && (!faces || !faces_out)))
        return (int)hipErrorInvalidValue;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = n_images, V = n_verts, F = n_faces;
    sc_mesh::Carver ws{(char*)scratch};
    Compact s;
    ws.take(s.used, V + 1LL), ws.take(s.rank, V + 1LL);
    const long long *vo = (const long long*)v_off, *fo = (const long long*)f_off;
    hipLaunchKernelGGL(cp_init_kernel, dim3(blocks(V + 1LL)), dim3(THREADS), 0, stream, s, V);
    if (F > 0) hipLaunchKernelGGL(cp_mark_kernel, dim3(blocks(3LL * F)), dim3(THREADS), 0, stream, faces, vo, fo, B, F, s);
    hipLaunchKernelGGL(cp_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, stream, s, V);
    const long long most = 3LL * F > V ? 3LL * F : V;
    hipLaunchKernelGGL(cp_emit_kernel, dim3(blocks(most > B ? most : B)), dim3(THREADS), 0, stream, verts, faces, vo, fo, B, V, F, parent, fixed,
                       s, verts_out, faces_out, vertex_map, fixed_out, (long long*)v_count_out);
    return (int)hipGetLastError();
}
