// mesh_edges.hpp -- what the mesh post-processing kernels share: packed batches (mesh_topology.hip, mesh_simplify.hip, mesh_smooth.hip,
// mesh_subdivide.hip, mesh_decimate.hip), the union-find on a global label array (mesh_topology.hip, level_components.hip), the
// open-addressing table of undirected edges (mesh_topology.hip, mesh_smooth.hip, mesh_subdivide.hip, mesh_decimate.hip) and the sorted
// vertex rings built from it (mesh_smooth.hip, mesh_subdivide.hip, mesh_decimate.hip).
//
// The correctness argument of every includer leans on these pieces and on nothing else of the header:
//   * every probe ends: the table has T > 3 F slots (slots_ok) and at most 3 F keys ever go in, so an empty or matching slot comes first;
//   * only integer atomics decide anything and no float is accumulated by an atomic: the same bits run to run, for any batch, stream,
//     arrival order or table size;
//   * the elements of a row are distinct (an edge is in the table once), so ranks are unique and the arrival order leaves no trace in
//     the sorted rows;
//   * a union-find parent is a SMALLER index (a root points at itself), so every find loop walks strictly decreasing labels and ends
//     whatever other threads do; a value read late is still an ancestor: it costs steps, never the result.
// The constants (THREADS, CHUNK, SCAN_THREADS, SCAN_ITEMS, SHORT_ROW, MAX_BLOCKS) are the includer's: they only show as time, never in
// a result, so they are template arguments here.
//
// There is no __global__ below and every device function is inlined: the including objects are built with -ffp-contract settings of
// their own (csrc/Makefile), and each carries, and launches, kernels of its own name around these pieces.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include "block_scan.hpp"

namespace sc_mesh {

// ---- packed batches: items of image b are [off[b], off[b + 1]) --------------------------------------------------------------------
// the image of packed item i: the largest b with off[b] <= i (off[0] = 0 <= i < off[B]; empty images share their offset with the next)
__device__ __forceinline__ int image_of(const long long* __restrict__ off, int B, long long i) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}
// first chunk slot of image b: chunks of different images never share a slot (ceil(n / CHUNK) <= floor(n / CHUNK) + 1)
template <int CHUNK>
__device__ __forceinline__ long long chunk_start(const long long* __restrict__ off, int b) { return off[b] / CHUNK + b; }
// the image of chunk slot blockIdx.x -- the largest b with chunk_start(b) <= blockIdx.x -- and, in `first`, the slot's first item;
// first >= off[b + 1] for a slot no image uses
template <int CHUNK>
__device__ __forceinline__ int chunk_image(const long long* __restrict__ off, int B, long long& first) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start<CHUNK>(off, mid) <= (long long)blockIdx.x) lo = mid; else hi = mid;
    }
    first = off[lo] + ((long long)blockIdx.x - chunk_start<CHUNK>(off, lo)) * CHUNK;
    return lo;
}
template <int CHUNK>
static inline long long chunk_slots(int n_images, long long n_items) { return n_items / CHUNK + n_images; }

// counts[field[k]][b] += v[k] for every lane with b >= 0.  Called by whole waves: when the lanes that have something agree on the image
// the wave folds its values and lane 0 adds them, else every lane adds its own.  Integer sums: the order does not matter.
template <int K>
__device__ __forceinline__ void image_add(unsigned long long* counts, int B, int b, const int (&field)[K], int (&v)[K]) {
    int lo = b < 0 ? INT_MAX : b, hi = b;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int l = __shfl_xor(lo, d), h = __shfl_xor(hi, d);
        lo = l < lo ? l : lo, hi = h > hi ? h : hi;
    }
    if (hi < 0) return;                                     // wave-uniform
    if (lo == hi) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            int s = b < 0 ? 0 : v[k];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
            if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(counts + (size_t)field[k] * B + lo, (unsigned long long)s);
        }
    } else if (b >= 0) {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (v[k] != 0) atomicAdd(counts + (size_t)field[k] * B + b, (unsigned long long)v[k]);
    }
}

// ---- union-find on a global label array; loads go past this CU's L1 (relaxed, agent scope) ----------------------------------------
__device__ __forceinline__ int find(const int* L, int x) {
    for (;;) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x || p < 0) return x;
        x = p;
    }
}
__device__ __forceinline__ void unite(int* L, int a, int b) {
    for (;;) {
        a = find(L, a);
        b = find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(L + a, b);                // a > b: a's parent becomes min(its parent, b)
        if (old == a) return;                               // a was a root: linked
        a = old;                                            // a had a parent: that one and b are still to be united
    }
}

// ---- the edge table: T slots, a power of two, keyed by (global lo << 32) | global hi ----------------------------------------------
constexpr int MAX_SLOTS = 1 << 30;
constexpr unsigned long long EMPTY = ~0ull;                 // no key looks like this: hi < 2^31

static inline bool slots_ok(long long table_slots, long long n_faces) {
    return table_slots >= 1 && table_slots <= MAX_SLOTS && (table_slots & (table_slots - 1)) == 0 && table_slots > 3 * n_faces;
}
// the hash keeps the top log2(T) bits of the mixed key (T >= 4 when F > 0)
static inline int table_shift(int T) {
    int shift = 64;
    for (int t = T; t > 1; t >>= 1) --shift;
    return shift;
}

struct EdgeSlot {
    int at;
    bool claimed;                   // this thread put the key there: exactly one thread per edge sees it
};
// the slot of undirected edge glo < ghi (batch-global vertex numbers): claimed by a 64-bit atomicCAS on the empty key, linear probing
__device__ __forceinline__ EdgeSlot edge_slot(unsigned long long* keys, int T, int shift, unsigned long long glo, unsigned long long ghi) {
    const unsigned long long key = (glo << 32) | ghi;
    int at = (int)((key * 0x9E3779B97F4A7C15ull) >> shift);
    unsigned long long old = EMPTY;
    for (int p = 0; p < T; ++p) {                           // T > 3 F: an empty or matching slot comes first
        old = atomicCAS(keys + at, EMPTY, key);
        if (old == EMPTY || old == key) break;
        at = (at + 1) & (T - 1);
    }
    return {at, old == EMPTY};
}

// the slot of an edge that IS in the finished table (read only, after the launch that filled it); -1 if an empty slot comes first
__device__ __forceinline__ int edge_find(const unsigned long long* __restrict__ keys, int T, int shift, unsigned long long glo,
                                         unsigned long long ghi) {
    const unsigned long long key = (glo << 32) | ghi;
    int at = (int)((key * 0x9E3779B97F4A7C15ull) >> shift);
    for (int p = 0; p < T; ++p) {
        const unsigned long long k = keys[at];
        if (k == key) return at;
        if (k == EMPTY) return -1;
        at = (at + 1) & (T - 1);
    }
    return -1;
}

// ---- vertex rings: the neighbours of every vertex over the table's edges, in ascending order --------------------------------------
struct Rings {                      // the includers' Scratch structs extend it
    unsigned long long* keys;       // [T]
    int* count;                     // [T] faces on the edge
    int *deg, *cursor, *fixed;      // [V] deg: one per claimed edge at the vertex; cursor 0 and fixed 0 before fill_rows
    int* row;                       // [V + 1] first entry of every vertex's row
    int *raw, *nbr;                 // [6 F] the rows in arrival order / in ascending order (batch-global vertex numbers)
};

// ONE workgroup of SCAN_THREADS: out[i] = in[0] + ... + in[i - 1] for i < n (out may be in), out[n] = the total.  The barrier contract
// of block_scan.hpp: wave_tot is LDS for SCAN_THREADS / 64 values, every round ends with a barrier because the next one writes wave_tot
// again, so a second call with the same wave_tot may follow at once.
template <int SCAN_THREADS, int SCAN_ITEMS>
__device__ __forceinline__ void scan_array(const int* in, int* out, int n, int* wave_tot) {
    int carry = 0;
    for (long long base = 0; base < n; base += SCAN_THREADS * SCAN_ITEMS) {             // workgroup-uniform
        const long long i0 = base + (long long)threadIdx.x * SCAN_ITEMS;
        int d[SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) d[k] = i0 + k < n ? in[i0 + k] : 0, sum += d[k];
        int total;
        int before = carry + sc_scan::block_exclusive<SCAN_THREADS / 64>(sum, wave_tot, total);
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            if (i0 + k < n) out[i0 + k] = before;
            before += d[k];
        }
        carry += total;
        __syncthreads();                                    // the next round writes wave_tot again
    }
    if (threadIdx.x == 0) out[n] = carry;
}

// grid-stride over table slots: each end of an edge goes into the other's row at an integer atomic cursor; a sharp edge -- one face
// (RIM_ONLY), or any number of faces but two -- stores 1 into the fixed word of both ends (every writer stores the same word)
template <int THREADS, bool RIM_ONLY>
__device__ __forceinline__ void fill_rows(const Rings& r, int T) {
    for (int i = blockIdx.x * THREADS + threadIdx.x; i < T; i += gridDim.x * THREADS) {
        const unsigned long long key = r.keys[i];
        if (key == EMPTY) continue;
        const int lo = (int)(key >> 32), hi = (int)(key & 0xFFFFFFFFull);
        r.raw[r.row[lo] + atomicAdd(r.cursor + lo, 1)] = hi;
        r.raw[r.row[hi] + atomicAdd(r.cursor + hi, 1)] = lo;
        if (RIM_ONLY ? r.count[i] == 1 : r.count[i] != 2) r.fixed[lo] = 1, r.fixed[hi] = 1;
    }
}

// raw[r0 + k], k in lanes `first`, first + stride, ... of a row of d distinct elements -> nbr[r0 + rank]
__device__ __forceinline__ void rank_row(const int* __restrict__ raw, int* __restrict__ nbr, int r0, int d, int first, int stride) {
    for (int k = first; k < d; k += stride) {
        const int e = raw[r0 + k];
        int rank = 0;
        for (int t = 0; t < d; ++t) rank += raw[r0 + t] < e;
        nbr[r0 + rank] = e;
    }
}
// Called by whole waves, every lane with its row [r0, r0 + d) or d = 0: a row up to SHORT_ROW long is ranked by its own thread, the
// longer ones by the whole wave, one after the other.
template <int SHORT_ROW>
__device__ __forceinline__ void sort_rows(const Rings& r, int r0, int d) {
    if (d <= SHORT_ROW) rank_row(r.raw, r.nbr, r0, d, 0, 1);
    unsigned long long todo = __ballot(d > SHORT_ROW);
    while (todo) {                                          // wave-uniform
        const int lane = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        rank_row(r.raw, r.nbr, __shfl(r0, lane), __shfl(d, lane), threadIdx.x & 63, 64);
    }
}

// false for an infinity and for a NaN
__device__ __forceinline__ bool finite(float x) { return x - x == 0.0f; }

// ---- host helpers -----------------------------------------------------------------------------------------------------------------
static inline long long align16(long long n) { return (n + 15) / 16 * 16; }

struct Carver {                     // hands out the arrays of a 16-byte aligned scratch buffer one after the other, each padded to 16 bytes
    char* at;
    template <class T>
    void take(T*& p, long long n) { p = (T*)at, at += align16((long long)sizeof(T) * n); }
};

// workgroups of a grid-stride pass over n items
template <int THREADS, int MAX_BLOCKS>
static inline unsigned blocks(long long n) {
    const long long g = (n + THREADS - 1) / THREADS;
    return (unsigned)(g < 1 ? 1 : g > MAX_BLOCKS ? MAX_BLOCKS : g);
}

}  // namespace sc_mesh
