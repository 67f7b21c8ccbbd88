// emd3d.hip -- the one-to-one matching of two equal-sized point clouds by Bertsekas' forward auction (Jacobi rounds, epsilon scaling) and
// the Earth Mover's Distance it gives (ops.emd_match, the evaluation's emd.txt under --eval.emd).  include/shapeclipper_hip.h states the
// rule operation by operation; tests/emd_ref.py restates it in numpy.  Built without contraction: every operation rounds once.
//
// One workgroup per image, the whole auction inside it: workgroup barriers only, no other workgroup is waited for, nothing is read back
// by the host, no float atomics.  A round is three steps with a barrier after each:
//   bid    : one wave per unassigned person (the waves stride over the list of them), lanes striding over the objects; the lanes' (best,
//            lowest index, second best) fold by shfl_down, lane 0 makes the bid by ONE 64-bit integer LDS max on the object's key
//            (bits(b) << 32) | (0xFFFFFFFF - person): the maximum of a total order, so the order the waves arrive in does not matter;
//   award  : one thread per object with a key: the bidder becomes the owner, the previous owner unassigned, the price the bid, key = 0;
//   list   : the unassigned persons are listed again (ballot + one integer LDS add per wave; the order of the list is arbitrary and
//            without effect: every entry bids against the same start-of-round state).
// LDS, dynamic, 48 n bytes -- 96 KiB at n = 2048 (above the 64 KiB default, so the launch raises the kernel's limit the way the other
// large-LDS kernels of the library do; a CU has 160 KiB):
//   key [n] 8 B, object x / y / z [n] 4 B each, price [n] 4 B, owner [n] 4 B, object-of-person [n] 4 B, list [n] 4 B,
//   person x / y / z [n] 4 B each (late rounds have a handful of bidders: a global load per bid would sit on the round's critical path).
// A lane scans its objects four at a time: the four positions and prices are loaded first and the four square roots interleave; the
// (best, lowest index, second best) update is then made in ascending j, by selects.
//
// The square root is sqrtf, which hipcc rounds correctly in its default mode (-fhip-fp32-correctly-rounded-divide-sqrt: v_sqrt_f32
// plus a fused residual correction).  __fsqrt_rn is NOT used: without OCML_BASIC_ROUNDED_OPERATIONS the compiler's header maps it to
// the native 1-ulp v_sqrt_f32.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "shapeclipper_hip.h"

namespace sc_emd {

constexpr int MAX_N = SC_EMD3D_MAX_POINTS;
constexpr int MAX_PHASES = SC_EMD3D_MAX_PHASES;
constexpr int MAX_IMAGES = 65535;
constexpr int THREADS = 1024;
constexpr int LDS_PER_POINT = 48;
constexpr int LDS_MAX = LDS_PER_POINT * MAX_N;            // 98,304 bytes

struct Phases { float e[MAX_PHASES]; int count; };       // passed by value (324 bytes of kernel argument)

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }      // false for NaN and Inf

// c = sqrt((dx dx + dy dy) + dz dz), one rounding per operation; recomputed by this expression wherever a cost is needed
__device__ __forceinline__ float pair_cost(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    return sqrtf(d2);
}

__global__ void __launch_bounds__(THREADS) match_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2, int n, Phases phases,
                                                     int max_rounds, int* __restrict__ assignment, float* __restrict__ cost,
                                                     float* __restrict__ price_out, int* __restrict__ rounds_out,
                                                     int* __restrict__ converged_out, double* __restrict__ emd_out) {
    extern __shared__ unsigned long long lds_raw[];
    unsigned long long* key = lds_raw;                  // [n] the best bid an object received this round, 0 = none
    float* ox = (float*)(key + n);                      // [n] x 3 object coordinates
    float* oy = ox + n;
    float* oz = oy + n;
    float* price = oz + n;                              // [n]
    int* owner = (int*)(price + n);                     // [n] the person that holds an object, -1 = nobody
    int* obj_of = owner + n;                            // [n] the object a person holds, -1 = unassigned
    int* list = obj_of + n;                             // [n] the unassigned persons, `count` of them
    float* px = (float*)(list + n);                     // [n] x 3 person coordinates
    float* py = px + n;
    float* pz = py + n;
    __shared__ int s_count, s_bad;

    const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nwaves = nthreads >> 6;
    const float* p1 = xyz1 + (long long)b * n * 3;
    const float* p2 = xyz2 + (long long)b * n * 3;
    assignment += (long long)b * n; cost += (long long)b * n; price_out += (long long)b * n;

    if (tid == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int k = tid; k < 3 * n; k += nthreads) bad = bad || !finite(p1[k]) || !finite(p2[k]);
    for (int j = tid; j < n; j += nthreads) {
        ox[j] = p2[3 * j + 0]; oy[j] = p2[3 * j + 1]; oz[j] = p2[3 * j + 2];
        px[j] = p1[3 * j + 0]; py[j] = p1[3 * j + 1]; pz[j] = p1[3 * j + 2];
        price[j] = 0.f; key[j] = 0ull;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (s_bad) {                                        // a non-finite coordinate: identity, zeros, emd = NaN
        for (int i = tid; i < n; i += nthreads) { assignment[i] = i; cost[i] = 0.f; price_out[i] = 0.f; }
        if (tid == 0) { rounds_out[b] = 0; converged_out[b] = 0; emd_out[b] = __longlong_as_double(0x7ff8000000000000LL); }
        return;
    }

    int rounds = 0, converged = 1;                      // the same in every thread
    for (int phase = 0; phase < phases.count && converged; ++phase) {
        const float e = phases.e[phase];
        for (int j = tid; j < n; j += nthreads) { owner[j] = -1; obj_of[j] = -1; list[j] = j; }
        int count = n;
        __syncthreads();
        while (count > 0) {
            if (rounds >= max_rounds) { converged = 0; break; }
            // ---- bid: wave `wave` takes the list entries wave, wave + nwaves, ...
            for (int k = wave; k < count; k += nwaves) {
                const int i = __builtin_amdgcn_readfirstlane(list[k]);
                const float ax = px[i], ay = py[i], az = pz[i];
                float w1 = -INFINITY, w2 = -INFINITY;
                int j1 = 0x7fffffff;
                for (int j0 = lane; j0 < n; j0 += 4 * 64) {
                    float w[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {       // an index past the end reads entry n - 1 and counts as -Inf: it changes nothing below
                        const int j = j0 + 64 * u, jj = j < n ? j : n - 1;
                        const float v = (-pair_cost(ax, ay, az, ox[jj], oy[jj], oz[jj])) - price[jj];
                        w[u] = j < n ? v : -INFINITY;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {       // ascending j and a strict >: the lowest j among a lane's maxima
                        const bool first = w[u] > w1;
                        w2 = first ? w1 : (w[u] > w2 ? w[u] : w2);
                        j1 = first ? j0 + 64 * u : j1;
                        w1 = first ? w[u] : w1;
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const float u1 = __shfl_down(w1, off, 64), u2 = __shfl_down(w2, off, 64);
                    const int uj = __shfl_down(j1, off, 64);
                    const bool other = u1 > w1 || (u1 == w1 && uj < j1);
                    const float loser = other ? w1 : u1;
                    w2 = fmaxf(other ? u2 : w2, loser);
                    if (other) { w1 = u1; j1 = uj; }
                }
                if (lane == 0) {
                    if ((unsigned int)j1 >= (unsigned int)n) j1 = 0;       // costs that overflowed to Inf (no w compares greater): stay in bounds
                    const float bid = price[j1] + ((w1 - w2) + e);
                    const unsigned long long k64 = ((unsigned long long)__float_as_uint(bid) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned int)i);
                    atomicMax(&key[j1], k64);
                }
            }
            __syncthreads();
            // ---- award: the owner of j held it at the start of the round, so it did not bid and is nobody's winner: no two threads
            // write one obj_of entry
            if (tid == 0) s_count = 0;
            for (int j = tid; j < n; j += nthreads) {
                const unsigned long long k64 = key[j];
                if (k64 != 0ull) {
                    const int i = (int)(0xFFFFFFFFu - (unsigned int)(k64 & 0xFFFFFFFFull));
                    const int prev = owner[j];
                    if (prev >= 0) obj_of[prev] = -1;
                    owner[j] = i;
                    obj_of[i] = j;
                    price[j] = __uint_as_float((unsigned int)(k64 >> 32));
                    key[j] = 0ull;
                }
            }
            __syncthreads();
            // ---- list the unassigned persons (every wave runs every trip: the ballot is of whole waves)
            for (int i0 = 0; i0 < n; i0 += nthreads) {
                const int i = i0 + tid;
                const bool un = i < n && obj_of[i] < 0;
                const unsigned long long mask = __ballot(un);
                if (mask != 0ull) {
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&s_count, __popcll(mask));
                    base = __shfl(base, 0, 64);
                    if (un) list[base + __popcll(mask & ((1ull << lane) - 1ull))] = i;
                }
            }
            __syncthreads();
            count = s_count;
            ++rounds;
        }
    }
    if (!converged) {                                   // the unassigned persons in ascending index take the unowned objects in ascending index
        if (tid == 0) {
            int j = 0;
            for (int i = 0; i < n; ++i) {
                if (obj_of[i] >= 0) continue;
                while (j < n - 1 && owner[j] >= 0) ++j;
                obj_of[i] = j; owner[j] = i; ++j;
            }
        }
        __syncthreads();
    }
    float* cost_lds = (float*)key;                      // the keys are done with
    for (int i = tid; i < n; i += nthreads) {
        const int j = obj_of[i];
        const float c = pair_cost(px[i], py[i], pz[i], ox[j], oy[j], oz[j]);
        assignment[i] = j; cost[i] = c; price_out[i] = price[i];
        cost_lds[i] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += (double)cost_lds[i];
        emd_out[b] = sum / (double)n;
        rounds_out[b] = rounds; converged_out[b] = converged;
    }
}

}  // namespace sc_emd

extern "C" int sc_emd3d_match(const float* xyz1, const float* xyz2, int n_images, int n, const float* eps_list, int n_eps, int max_rounds,
                              int* assignment, float* cost, float* price, int* rounds, int* converged, double* emd, void* stream) {
    using namespace sc_emd;
    if (n_images <= 0) return 0;
    if (n_images > MAX_IMAGES || n < 2 || n > MAX_N || n_eps < 1 || n_eps > MAX_PHASES || max_rounds < 1 || !xyz1 || !xyz2 || !eps_list ||
        !assignment || !cost || !price || !rounds || !converged || !emd)
        return (int)hipErrorInvalidValue;
    Phases phases;
    for (int k = 0; k < MAX_PHASES; ++k) phases.e[k] = k < n_eps ? eps_list[k] : 0.f;
    phases.count = n_eps;
    for (int k = 0; k < n_eps; ++k)
        if (!(phases.e[k] > 0.f) || !(phases.e[k] <= 3.402823466e+38f)) return (int)hipErrorInvalidValue;
    // 16 waves at every n: the rounds with many bids, which the waves share, outweigh the dearer barrier of the rounds with a handful
    // (measured against 4 and 8 waves from n = 16 to 2048: docs/LAB_NOTEBOOK.md section 18)
    const int threads = THREADS;
    const int lds_bytes = LDS_PER_POINT * n;
    (void)hipFuncSetAttribute((const void*)match_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);   // per launch: the attribute is per device, no process-wide state
    hipLaunchKernelGGL(match_kernel, dim3((unsigned int)n_images), dim3(threads), lds_bytes, (hipStream_t)stream, xyz1, xyz2, n, phases,
                       max_rounds, assignment, cost, price, rounds, converged, emd);
    return (int)hipGetLastError();
}
