// chamfer_bwd.hip -- Chamfer3D backward without float atomics: bitwise reproducible (contract: include/shapeclipper_hip.h).
//
// chamfer_grad_kernel (chamfer.hip; the reference's NmDistanceGradKernel, chamfer3D.cu:155-174) scatter-adds with six float atomicAdd per
// source: the sum of a row depends on the order the adders arrive in, and a row that many sources share (a small cloud against a large
// one, a collapsed prediction) takes all of them one after the other.  Here every contribution is STORED once, at its place in the
// inverted index of idx (per destination row, the list of its sources in ascending source index), and every row is summed from its list:
//   row = own term + S,  S = chunk partials added in chunk order,  a chunk = CB_CHUNK consecutive list entries summed in list order.
// Both directions run in the same launches (blockIdx.z): direction 0 has cloud 1 as sources (own terms -> gradxyz1, scattered terms ->
// gradxyz2), direction 1 is the mirror image.  Launches:
//   1. cb_count_kernel    histogram of idx per destination, and of its RUNS: the sources of one wave (64 consecutive source indices)
//                         that share a destination are one run (found with ballots, cb_match); integer atomics, order-free results
//   2. cb_scan_*_kernel   exclusive scans of both histograms (1,024-entry blocks + block totals, as chamfer_grid.hip scans its cells)
//   3. cb_runs_kernel     every run's (first source index, length) into its destination's run list: a slot claimed with an integer atomic,
//                         so the list's order is arbitrary -- nothing below depends on it
//   4. cb_place_kernel    a run's place in the row's list = the lengths of the row's runs with a smaller first source index (their
//                         sum does not depend on the list's order); a source's place = its run's place + its rank inside the run.  That
//                         is the stable counting placement: list order == ascending source index.  Stores the scattered term there and
//                         the own term in the source's output row.
//   5. cb_sum_kernel      a lane per row: lists of at most one chunk are summed and finished; longer ones are cut into chunk items
//   6. cb_chunk_kernel    a WAVE per chunk item (64 rows per coalesced fetch, added one by one in list order): a row with 50,000 sources
//                         is summed by 50,000 / CB_CHUNK waves at once, not by one lane walking the list
//   7. cb_finish_kernel   a lane per long row adds its partials in chunk order
// The quadratic part of 4 is bounded: a row's runs number at most min(its sources, waves of the cloud), 1,563 for 100,000 sources; it is
// the longest launch of the hub case (125 of 210 us: 782 first lanes walk 782 runs each).
// CB_CHUNK = 256: chunks of 64 / 128 / 256 / 512 measured within 2 % of each other on evenly loaded clouds and 0.82 / 0.78 / 0.77 / 0.76 ms
// on the hub case (profiles/chamfer_bwd_ordered.json); 256 keeps 196 waves on a 50,000-source row and short partial lists.
// Bound: latency / L2 (12-byte rows gathered by index); about 40 bytes of traffic per source.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "block_scan.hpp"
#include "shapeclipper_hip.h"

#pragma clang fp contract(off)      // t = (2 g) * (a - b) and the sums below: every operation rounded on its own, whatever the build's flags

namespace sc {

#ifndef SC_CHAMFER_BWD_CHUNK
#define SC_CHAMFER_BWD_CHUNK 256
#endif
constexpr int CB_CHUNK = SC_CHAMFER_BWD_CHUNK;      // list entries per chunk: a compile-time constant, part of the result's definition
static_assert(CB_CHUNK >= 64 && CB_CHUNK % 64 == 0, "a chunk is whole wave fetches");
constexpr int CB_THREADS = 256;

struct CbDir {                  // one direction; offsets into the workspace in 4-byte words
    const float* src;           // [b, ns, 3] the sources
    const float* dst;           // [b, nd, 3] the cloud idx points into
    const float* gd;            // [b, ns]
    const int32_t* idx;         // [b, ns] in [0, nd)
    float* own;                 // [b, ns, 3] gradient of the sources (own terms; NULL: not wanted)
    float* out;                 // [b, nd, 3] gradient of the destinations (own terms already there, scattered sums added; NULL: not wanted)
    int ns, nd, nbits, nblk, max_items, max_long;
    size_t cnt, rcnt, rcur, item_count, long_count, block_tot, runs, contrib, items, longs, part;
};
struct CbArgs { CbDir d[2]; };

// lanes of the wave that hold the same key as this one (bit `lane` included); meaningful on valid lanes
__device__ __forceinline__ unsigned long long cb_match(int key, bool valid, int nbits) {
    unsigned long long m = __ballot(valid);
    for (int bit = 0; bit < nbits; ++bit) {
        const bool one = (key >> bit) & 1;
        const unsigned long long s = __ballot(valid && one);
        m &= one ? s : ~s;
    }
    return m;
}

__device__ __forceinline__ int cb_key(const CbDir& D, int b, int j) {
    const int k = D.idx[(size_t)b * D.ns + j];
    return k < 0 ? 0 : (k >= D.nd ? D.nd - 1 : k);      // the forward never writes one out of range; this keeps a foreign one inside the workspace
}

// ---- 1. sources per destination, runs per destination ---------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_count_kernel(CbArgs A, int* __restrict__ ws) {
    const CbDir& D = A.d[blockIdx.z];
    if (!D.out) return;
    const int b = blockIdx.y, j = blockIdx.x * CB_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = j < D.ns;
    const int k = valid ? cb_key(D, b, j) : 0;
    const unsigned long long m = cb_match(k, valid, D.nbits);
    if (!valid) return;
    if ((m & ((1ull << lane) - 1ull)) != 0) return;                            // one pair of atomics per RUN: a row that 50,000 sources share takes
    atomicAdd(&ws[D.cnt + (size_t)b * (D.nd + 1) + k], __builtin_popcountll(m));   // 782 adds, not 50,000 on one address (570 us -> 12 us)
    atomicAdd(&ws[D.rcnt + (size_t)b * (D.nd + 1) + k], 1);
}

// ---- 2. exclusive scans, in place, of [0, nd] inclusive (the entry behind the last row ends up holding the total) ----------------------
// blockIdx.z = direction * 2 + (0: source histogram, 1: run histogram)
__global__ __launch_bounds__(1024) void cb_scan_local_kernel(CbArgs A, int* __restrict__ ws) {
    __shared__ int wtot[16];
    const CbDir& D = A.d[blockIdx.z >> 1];
    if (!D.out) return;
    const int which = blockIdx.z & 1, b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= D.nblk) return;
    int* c = ws + (which ? D.rcnt : D.cnt) + (size_t)b * (D.nd + 1);
    const int i = blk * 1024 + tid;
    const int v = i <= D.nd ? c[i] : 0;
    int total;
    const int before = sc_scan::block_exclusive<16>(v, wtot, total);
    if (i <= D.nd) c[i] = before;
    if (tid == 0) ws[D.block_tot + ((size_t)b * 2 + which) * D.nblk + blk] = total;
}

__global__ __launch_bounds__(1024) void cb_scan_add_kernel(CbArgs A, int* __restrict__ ws) {
    __shared__ int off_s;
    const CbDir& D = A.d[blockIdx.z >> 1];
    if (!D.out) return;
    const int which = blockIdx.z & 1, b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    if (blk >= D.nblk || blk == 0) return;
    if (tid < 64) {
        int part = 0;
        for (int k = tid; k < blk; k += 64) part += ws[D.block_tot + ((size_t)b * 2 + which) * D.nblk + k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
        if (tid == 0) off_s = part;
    }
    __syncthreads();
    const int off = off_s, i = blk * 1024 + tid;
    if (i <= D.nd && off) ws[(which ? D.rcnt : D.cnt) + (size_t)b * (D.nd + 1) + i] += off;
}

// ---- 3. the runs into their destination's run list (arbitrary order inside a list) -----------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_runs_kernel(CbArgs A, int* __restrict__ ws) {
    const CbDir& D = A.d[blockIdx.z];
    if (!D.out) return;
    const int b = blockIdx.y, j = blockIdx.x * CB_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = j < D.ns;
    const int k = valid ? cb_key(D, b, j) : 0;
    const unsigned long long m = cb_match(k, valid, D.nbits);
    if (!valid || (m & ((1ull << lane) - 1ull)) != 0) return;
    const int slot = ws[D.rcnt + (size_t)b * (D.nd + 1) + k] + atomicAdd(&ws[D.rcur + (size_t)b * D.nd + k], 1);      // < runs of b <= ns
    int* run = ws + D.runs + ((size_t)b * D.ns + slot) * 2;
    run[0] = j;
    run[1] = __builtin_popcountll(m);
}

// ---- 4. every term to its place: own term -> the source's output row, scattered term -> contrib[list position] -----------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_place_kernel(CbArgs A, int* __restrict__ ws) {
    const CbDir& D = A.d[blockIdx.z];
    if (!D.out && !D.own) return;
    const int b = blockIdx.y, j = blockIdx.x * CB_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    const bool valid = j < D.ns;
    const int k = valid ? cb_key(D, b, j) : 0;
    float t[3] = {0.f, 0.f, 0.f};
    if (valid) {
        const float* s = D.src + ((size_t)b * D.ns + j) * 3;
        const float* d = D.dst + ((size_t)b * D.nd + k) * 3;
        const float g = D.gd[(size_t)b * D.ns + j] * 2;
        for (int a = 0; a < 3; ++a) t[a] = g * (s[a] - d[a]);
        if (D.own) {
            float* o = D.own + ((size_t)b * D.ns + j) * 3;
            for (int a = 0; a < 3; ++a) o[a] = t[a];
        }
    }
    if (!D.out) return;                                                       // uniform: the ballots below are the whole wave's
    const unsigned long long m = cb_match(k, valid, D.nbits);
    const unsigned long long below = m & ((1ull << lane) - 1ull);
    const int head = (valid && m) ? __builtin_ctzll(m) : lane;
    int off = 0;
    if (valid && below == 0) {                                                // the run's first lane: sources of this row in earlier waves
        const int* rs = ws + D.rcnt + (size_t)b * (D.nd + 1) + k;
        const int* runs = ws + D.runs + (size_t)b * D.ns * 2;
        for (int r = rs[0]; r < rs[1]; ++r) off += runs[2 * r] < j ? runs[2 * r + 1] : 0;
    }
    off = __shfl(off, head);
    if (!valid) return;
    const int pos = ws[D.cnt + (size_t)b * (D.nd + 1) + k] + off + __builtin_popcountll(below);      // < ns
    float* c = reinterpret_cast<float*>(ws + D.contrib) + ((size_t)b * D.ns + pos) * 3;
    for (int a = 0; a < 3; ++a) c[a] = -t[a];
}

// ---- 5. a lane per destination row: short lists are finished here, long ones become chunk items --------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_sum_kernel(CbArgs A, int* __restrict__ ws) {
    const CbDir& D = A.d[blockIdx.z];
    if (!D.out) return;
    const int b = blockIdx.y, k = blockIdx.x * CB_THREADS + threadIdx.x;
    if (k >= D.nd) return;
    const int* st = ws + D.cnt + (size_t)b * (D.nd + 1) + k;
    const int s = st[0], len = st[1] - s;
    if (len <= CB_CHUNK) {
        const float* c = reinterpret_cast<const float*>(ws + D.contrib) + ((size_t)b * D.ns + s) * 3;
        float p[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < len; ++i)
            for (int a = 0; a < 3; ++a) p[a] += c[3 * i + a];
        float* o = D.out + ((size_t)b * D.nd + k) * 3;
        for (int a = 0; a < 3; ++a) o[a] = o[a] + p[a];                      // S = +0 + P0 = P0 (P0 starts from +0: never -0)
        return;
    }
    const int nch = (len + CB_CHUNK - 1) / CB_CHUNK;
    const int li = atomicAdd(&ws[D.long_count + b], 1);                      // <= ns / CB_CHUNK rows are long
    const int first = atomicAdd(&ws[D.item_count + b], nch);                 // sum over long rows of ceil(len / CB_CHUNK) < 2 ns / CB_CHUNK
    int* L = ws + D.longs + ((size_t)b * D.max_long + li) * 3;
    L[0] = k; L[1] = first; L[2] = nch;
    int* it = ws + D.items + ((size_t)b * D.max_items + first) * 2;
    for (int c = 0; c < nch; ++c) {
        it[2 * c] = s + c * CB_CHUNK;
        it[2 * c + 1] = min(CB_CHUNK, len - c * CB_CHUNK);
    }
}

// ---- 6. a wave per chunk item ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CB_THREADS) void cb_chunk_kernel(CbArgs A, int* __restrict__ ws) {
    const CbDir& D = A.d[blockIdx.z];
    if (!D.out) return;
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int n_items = ws[D.item_count + b];
    const float* contrib = reinterpret_cast<const float*>(ws + D.contrib) + (size_t)b * D.ns * 3;
    for (int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6))); item < n_items; item += (int)gridDim.x * 4) {
        const int* it = ws + D.items + ((size_t)b * D.max_items + item) * 2;
        const int row0 = __builtin_amdgcn_readfirstlane(it[0]), len = __builtin_amdgcn_readfirstlane(it[1]);
        float p[3] = {0.f, 0.f, 0.f};
        for (int base = 0; base < len; base += 64) {
            const int cnt = min(64, len - base);
            float v[3] = {0.f, 0.f, 0.f};
            if (lane < cnt)
                for (int a = 0; a < 3; ++a) v[a] = contrib[(size_t)(row0 + base + lane) * 3 + a];
            for (int i = 0; i < cnt; ++i)                                      // list order: lane 0's row first
                for (int a = 0; a < 3; ++a) p[a] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[a]), i));
        }
        if (lane < 3) reinterpret_cast<float*>(ws + D.part)[((size_t)b * D.max_items + item) * 3 + lane] = lane == 0 ? p[0] : (lane == 1 ? p[1] : p[2]);
    }
}

// ---- 7. a lane per long row: partials in chunk order ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cb_finish_kernel(CbArgs A, int* __restrict__ ws) {
    const CbDir& D = A.d[blockIdx.z];
    if (!D.out) return;
    const int b = blockIdx.y, n_long = ws[D.long_count + b];
    for (int li = blockIdx.x * 64 + threadIdx.x; li < n_long; li += gridDim.x * 64) {
        const int* L = ws + D.longs + ((size_t)b * D.max_long + li) * 3;
        const int k = L[0], first = L[1], nch = L[2];
        const float* part = reinterpret_cast<const float*>(ws + D.part) + ((size_t)b * D.max_items + first) * 3;
        float sm[3] = {0.f, 0.f, 0.f};
        for (int c = 0; c < nch; ++c)
            for (int a = 0; a < 3; ++a) sm[a] += part[3 * c + a];
        float* o = D.out + ((size_t)b * D.nd + k) * 3;
        for (int a = 0; a < 3; ++a) o[a] = o[a] + sm[a];
    }
}

// The workspace: the words cleared on entry (histograms, cursors, counters) of both directions first and adjacent, one memset.
struct CbCarve { CbArgs args; size_t zeroed, total; };
inline CbCarve cb_carve(int b, int n, int m) {
    CbCarve c{};
    size_t o = 0;
    auto take = [&](size_t words) { const size_t at = o; o += (words + 3) & ~(size_t)3; return at; };
    for (int d = 0; d < 2; ++d) {
        CbDir& D = c.args.d[d];
        D.ns = d == 0 ? n : m;
        D.nd = d == 0 ? m : n;
        D.nbits = 0;
        while (D.nbits < 31 && (1 << D.nbits) < D.nd) ++D.nbits;
        D.nblk = D.nd / 1024 + 1;                                              // covers [0, nd] inclusive
        D.max_long = D.ns / CB_CHUNK + 1;
        D.max_items = 2 * (D.ns / CB_CHUNK) + 2;
        D.cnt = take((size_t)b * (D.nd + 1));
        D.rcnt = take((size_t)b * (D.nd + 1));
        D.rcur = take((size_t)b * D.nd);
        D.item_count = take((size_t)b);
        D.long_count = take((size_t)b);
    }
    c.zeroed = o;
    for (int d = 0; d < 2; ++d) {
        CbDir& D = c.args.d[d];
        D.block_tot = take((size_t)b * 2 * D.nblk);
        D.runs = take((size_t)b * D.ns * 2);
        D.contrib = take((size_t)b * D.ns * 3);
        D.items = take((size_t)b * D.max_items * 2);
        D.longs = take((size_t)b * D.max_long * 3);
        D.part = take((size_t)b * D.max_items * 3);
    }
    c.total = o;
    return c;
}

}  // namespace sc

extern "C" {

long long sc_chamfer3d_backward_ordered_workspace_bytes(int b, int n, int m) {
    if (b <= 0 || n <= 0 || m <= 0) return 0;
    return (long long)(sc::cb_carve(b, n, m).total * sizeof(int));
}

int sc_chamfer3d_backward_ordered_chunk(void) { return sc::CB_CHUNK; }

int sc_chamfer3d_backward_ordered(const float* xyz1, const float* xyz2, float* gradxyz1, float* gradxyz2,
                                  const float* graddist1, const float* graddist2, const int32_t* idx1,
                                  const int32_t* idx2, int b, int n, int m, void* workspace, void* stream_) {
    using namespace sc;
    hipStream_t stream = (hipStream_t)stream_;
    if (b <= 0 || n < 0 || m < 0) return 0;
    if (n == 0 || m == 0) {                      // an empty opposite cloud gives no terms
        if (gradxyz1 && n > 0) (void)hipMemsetAsync(gradxyz1, 0, (size_t)b * n * 3 * sizeof(float), stream);
        if (gradxyz2 && m > 0) (void)hipMemsetAsync(gradxyz2, 0, (size_t)b * m * 3 * sizeof(float), stream);
        return (int)hipGetLastError();
    }
    if (!gradxyz1 && !gradxyz2) return 0;
    CbCarve c = cb_carve(b, n, m);
    CbDir& D0 = c.args.d[0];
    CbDir& D1 = c.args.d[1];
    D0.src = xyz1; D0.dst = xyz2; D0.gd = graddist1; D0.idx = idx1; D0.own = gradxyz1; D0.out = gradxyz2;
    D1.src = xyz2; D1.dst = xyz1; D1.gd = graddist2; D1.idx = idx2; D1.own = gradxyz2; D1.out = gradxyz1;
    int* ws = (int*)workspace;
    const int big = n > m ? n : m;               // both directions share a grid: sources and destinations of either fit in `big`
    const dim3 per_point((big + CB_THREADS - 1) / CB_THREADS, b, 2), scan(big / 1024 + 1, b, 4);
    (void)hipMemsetAsync(ws, 0, c.zeroed * sizeof(int), stream);
    hipLaunchKernelGGL(cb_count_kernel, per_point, dim3(CB_THREADS), 0, stream, c.args, ws);
    hipLaunchKernelGGL(cb_scan_local_kernel, scan, dim3(1024), 0, stream, c.args, ws);
    hipLaunchKernelGGL(cb_scan_add_kernel, scan, dim3(1024), 0, stream, c.args, ws);
    hipLaunchKernelGGL(cb_runs_kernel, per_point, dim3(CB_THREADS), 0, stream, c.args, ws);
    hipLaunchKernelGGL(cb_place_kernel, per_point, dim3(CB_THREADS), 0, stream, c.args, ws);
    hipLaunchKernelGGL(cb_sum_kernel, per_point, dim3(CB_THREADS), 0, stream, c.args, ws);
    const int max_items = D0.max_items > D1.max_items ? D0.max_items : D1.max_items;
    const int max_long = D0.max_long > D1.max_long ? D0.max_long : D1.max_long;
    hipLaunchKernelGGL(cb_chunk_kernel, dim3((max_items + 3) / 4 < 1024 ? (max_items + 3) / 4 : 1024, b, 2), dim3(CB_THREADS), 0, stream, c.args, ws);
    hipLaunchKernelGGL(cb_finish_kernel, dim3((max_long + 63) / 64 < 64 ? (max_long + 63) / 64 : 64, b, 2), dim3(64), 0, stream, c.args, ws);
    return (int)hipGetLastError();
}

}  // extern "C"
