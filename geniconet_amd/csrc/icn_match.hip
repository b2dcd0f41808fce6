// Optimal matching of two point clouds of one size by a synchronous (Jacobi) epsilon-scaling auction (icn_match_clouds in
// include/icn_match.h): what the earth mover's distance of the evaluation tables (geniconet_amd/metrics.py: optimal_matching,
// pairwise_emd, earth_movers_distance) is built on.  The definition -- cost, scale, early cases, phases, one round, the round cap -- is
// stated once in include/icn_match.h and restated in torch by metrics._torch_optimal_matching; max, the argmax with the lowest index
// and the second maximum do not depend on the order of evaluation, so match, rounds and prices are fixed bit for bit however the work
// is split, and only the final cost sum has an order (fixed by N alone).
// k_match_auction: grid (R, G) or, paired, (1, G); ONE WORKGROUP OF 1024 THREADS OWNS ONE PAIR from start to finish.  Nothing waits
// for another workgroup, nothing spins on memory, the launch is an ordinary one.  The only loops whose trip count depends on the data
// are the round loop, bounded by max_rounds, and the walk over the unassigned persons of a round, bounded by N; non-finite and
// all-coincident input leave by the early cases before any loop.
// LDS: price (double) and owner (one 32-bit word) of every object, 12 N bytes of dynamic shared memory -- 122 904 B at N = 10 242 --
// which is what bounds N at MATCH_MAX_N.  The list of unassigned persons (two copies, one read and one written in a round), person ->
// object and each bidder's (j1, bid) live in the pair's slice of the caller's workspace, 24 N bytes that stay in L2.
// ONE ROUND, five barriers:
//   A  every bidder scans all N objects against the prices as they stand: v = (-c) - price, c = sqrtf of the fp32 squared distance of
//      icn_nn.h, the best value with the lowest index and the second best.  A wave takes one bidder at a time, its lanes stride the
//      objects, (v1, j1, v2) are merged across the wave by shuffles and lane 0 writes (j1, bid).  Most rounds of an auction have a
//      handful of bidders (a far I5 pair averages 5.5), so below 16 bidders floor(16 / bidders) waves share one bidder's scan, each a
//      strided part of the objects, and one thread merges their partial results from LDS: one more barrier in those rounds.
//   B  no price moved in A; now price[j1] = max(price[j1], bid) by an LDS atomic max on the raw bits -- bids are non-negative doubles
//      (prices start at 0 and a bid is a price plus a non-negative gap plus eps), whose order is that of their bits as integers.  A bid
//      is never below the price it is built on, so afterwards price[j] is the highest bid where j received one and unchanged elsewhere.
//   D  the bidders whose bid equals price[j1] are the highest; the lowest person among them wins by an LDS atomic min.  The owner word
//      is (candidate << 16) | owner: between rounds the high half is 0x7fff, above every person, so the min needs no reset pass and
//      the previous owner stays readable in the low half (N <= MATCH_MAX_N < 0x7fff).
//   E  the winner unassigns the previous owner, who joins the next list, and records its object; a bidder that lost joins the next list.
//   F  the winner writes the owner word back as 0x7fff << 16 | itself.
// Integer max and min are order-free, so the result is deterministic although the order of the next list is not: that order only
// decides which wave scans for which bidder.  No floating-point atomic anywhere.
// The hot loop is the scan: per (bidder, object) 3 v_sub_f32, 3 v_mul_f32, 2 v_add_f32, the correctly rounded sqrtf, one conversion,
// one v_add_f64, two f64 compares and their selects, one ds_read_b64 and three dword loads of the target (global memory; the cloud
// stays in L2).  Timings on an MI355X: profiles/emd_matrix.txt (tools/time_emd.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

#pragma clang fp contract(off)

namespace icn {
namespace {

constexpr int MATCH_BLOCK = 1024;            // threads of the workgroup that owns a pair
constexpr int MATCH_WAVES = MATCH_BLOCK / 64;
constexpr int MATCH_MAX_N = 13312;           // 12 N bytes of LDS beside the static tables below: 159 744 of 163 840
constexpr unsigned MATCH_NONE = 0xffffu;     // low half of an owner word: nobody owns the object
constexpr unsigned MATCH_OPEN = 0x7fffu << 16;   // high half of an owner word between rounds: above every person

struct Top { double v1, v2; int j1; };       // best value, second best value, lowest index of the best

// (v1, j1, v2) of the union of two disjoint sets of objects
__device__ __forceinline__ void merge(Top& a, double v1, int j1, double v2) {
    if (v1 > a.v1 || (v1 == a.v1 && j1 < a.j1)) {
        a.v2 = v2 > a.v1 ? v2 : a.v1;
        a.v1 = v1;
        a.j1 = j1;
    } else {
        a.v2 = a.v2 > v1 ? a.v2 : v1;
    }
}

__device__ __forceinline__ float pair_cost(f3 p, f3 q) {
    const float dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// objects first, first + step, ... of one bidder, merged over the wave: every lane returns the same Top
__device__ __forceinline__ Top scan_objects(f3 p, const float* __restrict__ q, const double* price, int N, int first, int step) {
    Top t = {-INFINITY, -INFINITY, 0x7fffffff};
    for (int j = first; j < N; j += step) {
        const double v = -(double)pair_cost(p, load3(q + (size_t)j * 3)) - price[j];
        if (v > t.v1) {                                                      // ascending j: the lowest index among equals stays
            t.v2 = t.v1;
            t.v1 = v;
            t.j1 = j;
        } else if (v > t.v2) {
            t.v2 = v;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double v1 = __shfl_xor(t.v1, d), v2 = __shfl_xor(t.v2, d);
        const int j1 = __shfl_xor(t.j1, d);
        merge(t, v1, j1, v2);
    }
    return t;
}

// the bid of a finished scan, against the prices as they stand.  Only values that are no number leave j1 outside [0, N) (squared
// distances that overflow fp32; the header): object 0 then, so that nothing is indexed out of bounds.
__device__ __forceinline__ void place_bid(const Top& t, double eps, const double* price, int N, int b, int* bidj, double* bidv) {
    const int j1 = (unsigned)t.j1 < (unsigned)N ? t.j1 : 0;
    bidj[b] = j1;
    bidv[b] = ((t.v1 - t.v2) + eps) + price[j1];
}

__global__ __launch_bounds__(MATCH_BLOCK) void k_match_auction(const float* __restrict__ qry, const float* __restrict__ tgt, int N,
                                                                int paired, int phases, int max_rounds, int* __restrict__ match,
                                                                double* __restrict__ prices, double* __restrict__ cost,
                                                                int* __restrict__ rounds_out, char* __restrict__ ws, size_t slice) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* price = reinterpret_cast<double*>(smem);                         // [N]
    unsigned* owner = reinterpret_cast<unsigned*>(price + N);                // [N]  (candidate << 16) | owner
    __shared__ float box[MATCH_WAVES][7];
    __shared__ Top partial[MATCH_WAVES];
    __shared__ double red[MATCH_WAVES];
    __shared__ int next_count;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = blockIdx.y, r = paired ? g : (int)blockIdx.x;
    const size_t pair = paired ? (size_t)g : (size_t)g * gridDim.x + r;
    const float* P = qry + (size_t)g * N * 3;
    const float* Q = tgt + (size_t)r * N * 3;
    int* m_out = match ? match + pair * N : nullptr;
    double* p_out = prices ? prices + pair * N : nullptr;
    double* bidv = reinterpret_cast<double*>(ws + pair * slice);             // [N] the bid of bidder b of the round
    int* bidj = reinterpret_cast<int*>(bidv + N);                            // [N] its object
    int* p2o = bidj + N;                                                     // [N] person -> object, -1 unassigned
    int* ucur = p2o + N;                                                     // [N] the unassigned persons of the round
    int* unext = ucur + N;                                                   // [N] ... of the next

    // ---- the joint bounding box and whether every coordinate is finite ----
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, bad = 0.f;
    for (int i = tid; i < N; i += MATCH_BLOCK) {
        const f3 a = load3(P + (size_t)i * 3), b = load3(Q + (size_t)i * 3);
        const float av[3] = {a.x, a.y, a.z}, bv[3] = {b.x, b.y, b.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!__builtin_isfinite(av[c]) || !__builtin_isfinite(bv[c])) bad = 1.f;
            lo[c] = fminf(lo[c], fminf(av[c], bv[c]));                       // min and max of numbers are order-free
            hi[c] = fmaxf(hi[c], fmaxf(av[c], bv[c]));
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], d));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d));
        }
        bad = fmaxf(bad, __shfl_xor(bad, d));
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            box[wave][c] = lo[c];
            box[wave][3 + c] = hi[c];
        }
        box[wave][6] = bad;
    }
    __syncthreads();
    for (int w = 0; w < MATCH_WAVES; ++w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], box[w][c]);
            hi[c] = fmaxf(hi[c], box[w][3 + c]);
        }
        bad = fmaxf(bad, box[w][6]);
    }
    const double ex = (double)hi[0] - (double)lo[0], ey = (double)hi[1] - (double)lo[1], ez = (double)hi[2] - (double)lo[2];
    const double D = sqrt((ex * ex + ey * ey) + ez * ez);

    // ---- the cases decided before any loop ----
    if (bad != 0.f || !__builtin_isfinite(D) || D == 0.0 || N == 1) {
        const bool none = bad != 0.f || !__builtin_isfinite(D);
        for (int i = tid; i < N; i += MATCH_BLOCK) {
            if (m_out) m_out[i] = none ? -1 : i;
            if (p_out) p_out[i] = none ? (double)NAN : 0.0;
        }
        if (tid == 0) {
            cost[pair] = none ? (double)NAN : D == 0.0 ? 0.0 : (double)pair_cost(load3(P), load3(Q));
            rounds_out[pair] = 0;
        }
        return;
    }

    for (int j = tid; j < N; j += MATCH_BLOCK) price[j] = 0.0;
    if (tid == 0) next_count = 0;
    int rounds = 0;
    bool capped = false;
    for (int k = 1; k <= phases && !capped; ++k) {
        const double eps = scalbn(D, -2 * k);                                // D 4^-k: a power of two, exact
        for (int i = tid; i < N; i += MATCH_BLOCK) {
            owner[i] = MATCH_OPEN | MATCH_NONE;
            p2o[i] = -1;
            ucur[i] = i;
        }
        int nu = N;
        __syncthreads();
        while (nu > 0) {
            if (rounds == max_rounds) {
                capped = true;
                break;
            }
            ++rounds;
            // A: every bid of the round against the prices as they stand
            if (nu >= MATCH_WAVES) {
                for (int b = wave; b < nu; b += MATCH_WAVES) {
                    const Top t = scan_objects(load3(P + (size_t)ucur[b] * 3), Q, price, N, lane, 64);
                    if (lane == 0) place_bid(t, eps, price, N, b, bidj, bidv);
                }
            } else {
                const int team = MATCH_WAVES / nu;                           // waves that share one bidder's scan
                if (wave < nu * team) {
                    const int b = wave / team, part = wave % team;
                    const Top t = scan_objects(load3(P + (size_t)ucur[b] * 3), Q, price, N, part * 64 + lane, team * 64);
                    if (lane == 0) partial[wave] = t;
                }
                __syncthreads();
                if (tid < nu) {
                    Top t = partial[tid * team];
                    for (int w = 1; w < team; ++w) merge(t, partial[tid * team + w].v1, partial[tid * team + w].j1, partial[tid * team + w].v2);
                    place_bid(t, eps, price, N, tid, bidj, bidv);
                }
            }
            __syncthreads();
            // B: the highest bid of every object becomes its price
            for (int b = tid; b < nu; b += MATCH_BLOCK)
                atomicMax(reinterpret_cast<unsigned long long*>(price + bidj[b]), (unsigned long long)__double_as_longlong(bidv[b]));
            __syncthreads();
            // D: among the highest bidders of an object the lowest person
            for (int b = tid; b < nu; b += MATCH_BLOCK) {
                const int j1 = bidj[b];
                if (bidv[b] == price[j1]) {
                    const unsigned previous = __hip_atomic_load(owner + j1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) & 0xffffu;
                    atomicMin(owner + j1, ((unsigned)ucur[b] << 16) | previous);
                }
            }
            __syncthreads();
            // E: the winner unassigns the previous owner and records its object; everyone else bids again
            for (int b = tid; b < nu; b += MATCH_BLOCK) {
                const int i = ucur[b], j1 = bidj[b];
                const unsigned w = owner[j1];
                if (bidv[b] == price[j1] && (w >> 16) == (unsigned)i) {
                    const unsigned previous = w & 0xffffu;
                    if (previous != MATCH_NONE) {                            // a person of this pair: < N
                        p2o[previous] = -1;
                        unext[atomicAdd(&next_count, 1)] = (int)previous;
                    }
                    p2o[i] = j1;
                } else {
                    unext[atomicAdd(&next_count, 1)] = i;
                }
            }
            __syncthreads();
            // F: the owner words of the objects that changed hands, ready for the next round
            const int following = next_count;                                // at most N: a person is unassigned at most once a round
            for (int b = tid; b < nu; b += MATCH_BLOCK) {
                const int i = ucur[b], j1 = bidj[b];
                if (p2o[i] == j1) owner[j1] = MATCH_OPEN | (unsigned)i;
            }
            __syncthreads();
            if (tid == 0) next_count = 0;                                    // next touched in E of the next round, barriers away
            int* const swap = ucur;
            ucur = unext;
            unext = swap;
            nu = following;
        }
    }
    __syncthreads();

    // ---- the outputs ----
    double s = 0.0;
    for (int i = tid; i < N; i += MATCH_BLOCK) {
        const int j = p2o[i];
        if (m_out) m_out[i] = j;
        if (p_out) p_out[i] = price[i];
        if (!capped) s += (double)pair_cost(load3(P + (size_t)i * 3), load3(Q + (size_t)j * 3));   // every person owns an object
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        for (int w = 0; w < MATCH_WAVES; ++w) total += red[w];
        cost[pair] = capped ? (double)NAN : total;
        rounds_out[pair] = rounds;
    }
}

}  // namespace

bool match_clouds_fits(int N) { return N <= MATCH_MAX_N; }

size_t match_clouds_workspace_bytes(int G, int R, int N, int paired) {
    return (paired ? (size_t)G : (size_t)G * (size_t)R) * 16 * (((size_t)N * 3 + 1) / 2);
}

void launch_match_clouds(const float* qry, const float* tgt, int G, int R, int N, int paired, int phases, int max_rounds, int* match,
                         double* prices, double* cost, int* rounds, void* ws, hipStream_t s) {
    const size_t slice = 16 * (((size_t)N * 3 + 1) / 2), lds = (size_t)N * 12;
    // the most a launch may ask for: MATCH_MAX_N objects, which leaves the kernel's static tables (under 1 KiB) inside the 160 KiB
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_match_auction), hipFuncAttributeMaxDynamicSharedMemorySize, MATCH_MAX_N * 12);
    prof_mark_begin(PROF_MATCH_AUCTION, 0.0, s);
    hipLaunchKernelGGL(k_match_auction, dim3(paired ? 1 : R, G), dim3(MATCH_BLOCK), lds, s, qry, tgt, N, paired, phases, max_rounds, match,
                       prices, cost, rounds, static_cast<char*>(ws), slice);
    prof_mark_end(s);
}

}  // namespace icn
