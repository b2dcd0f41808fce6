// Directed sums of nearest squared distances for EVERY pair of clouds of two sets (icn_sided_sums in include/icn_pairs.h): what the
// G x R chamfer matrix of the generation metrics (MMD, coverage, 1-NN accuracy; geniconet_amd/metrics.py) is built on.
// queries (G, N, 3) fp32, targets (R, M, 3) fp32; sums (G, R) float64, sums[g, r] = sum_i best_i, best_i the `dist` of include/icn_nn.h
// for query i of cloud g against the targets of cloud r: fp32 on the values as stored, every product and sum rounded on its own in the
// order written (this file is compiled with fp contract(off)),
//   dx = p.x - q_j.x, dy = p.y - q_j.y, dz = p.z - q_j.z,  d_j = (dx dx + dy dy) + dz dz,  best = +inf, then best = min(best, d_j)
// over the acceptable d_j (a NaN d_j is passed over, +inf is never taken: best stays +inf where nothing is acceptable).
// THE FORM SHIPPED IS best = fminf(best, d).  No index is kept, so the compare and the two selects of k_nn_points are not needed, and
// fminf gives the same bits as `if (d < best) best = d`: it returns the operand that is not a NaN, min(+inf, +inf) is +inf, and d, a
// sum of squares, is never -0.  hipcc (ROCm 7, -O3) goes one further in the loop over four targets and folds two fminf into one
// v_min3_f32 (the minimum of the operands that are no NaN, the same rule): for four targets and two queries 24 v_sub_f32, 24 v_mul_f32,
// 16 v_add_f32 and 4 v_min3_f32, none fused, none packed, and one move: 8.6 VALU instructions a pair where the 9 of the plain form were
// expected and k_nn_points spends 11.6.  No canonicalising v_max_f32 is needed there (every operand comes out of arithmetic); the loop
// over the last one to three targets of a tile has one a query and target, which changes no bit of a value that is no NaN.
// tests/test_pairwise_chamfer_gpu.py holds the equality with k_nn_points, non-finite input included.
// k_pair_sums: grid (ceil(N / (MESH_BLOCK PAIR_QUERIES)), R, G): the pair is (blockIdx.z, blockIdx.y), a workgroup owns one chunk of
// MESH_BLOCK PAIR_QUERIES queries of cloud g, query q of thread t being chunk base + q MESH_BLOCK + t, and meets every target of cloud r
// in ascending order through LDS tiles of PAIR_TILE targets.  A tile is the packed (PAIR_TILE, 3) image of the targets, staged by a
// straight copy (thread t moves words t, t + 256, t + 512: coalesced loads, one bank a lane) and read four targets at a time as three
// ds_read_b128, every lane of a wave at the same address: broadcasts, 12 LDS cycles for four targets where the padded float4 entry
// of k_nn_points, which the compiler reads as ds_read_b96, asks for 32.  That matters here: at 9 VALU instructions a pair and two
// queries a thread the padded layout would ask the LDS for 32 cycles in every 36 the four SIMDs of a CU compute, the packed one for 12 in
// every 36.  The last targets of a cloud whose count is no multiple of four are read one by one.  Threads past N hold query 0 of the
// cloud and contribute an exact 0; a wave none of whose queries exist stages its share of each tile and skips the arithmetic.
// THE SUM, in double (the conversion of an fp32 value is exact and every term is >= 0, so no NaN can come out and a single +inf row
// makes the sum +inf), in an order fixed by N alone: a thread adds its queries in ascending q, block_sum_store adds the workgroup (xor
// shuffles inside a wave, then a tree over the four waves), and the workgroup's partial goes to ws[chunk][g R + r]; k_pair_sums_finish,
// one thread a pair, adds the partials of its pair in ascending chunk order and writes sums[g, r].  No atomics, every partial and every
// output written exactly once, bit-identical run to run, and nothing in the order depends on G, R or the pair's position: entry (g, r)
// of a G x R call is the 1 x 1 call on those two clouds bit for bit.
// WHY TWO LAUNCHES AND A WORKSPACE, not a chunk loop inside one workgroup a pair.  The metrics are used on small sets as well: G = R =
// 4 is 16 pairs, and one workgroup a pair would leave 240 of the 256 CUs idle while 16 of them walk 10 242 x 10 242 distances each, one
// wave a SIMD -- a VALU instruction every 4 cycles, not every 2.  With the chunks in the grid the same call is 16 x 21 = 336 workgroups
// at I5, and 64 x 64 pairs are 86 016; the price is 8 G R ceil(N / 512) bytes of scratch (0.7 MB at 64 x 64 x 10 242) and a finishing
// launch that reads it once, microseconds beside the search.  PAIR_QUERIES = 2 by the argument of icn_nn.hip for NN_QUERIES: four queries
// would halve the workgroups of a small call (176 at 4 x 4, fewer than there are CUs), and the LDS, which four queries relieve, is
// already at a third of its rate with the packed tile.
// hipcc reports for k_pair_sums 37 VGPRs, no scratch, 3 KiB + 32 bytes of LDS, 8 waves a SIMD; for k_pair_sums_finish 8 VGPRs, no scratch.
// The inner loop is 69 VALU instructions for 8 pairs (four targets x two queries) and three ds_read_b128; it is not unrolled further.
// Timings on an MI355X: profiles/chamfer_matrix.txt (tools/time_chamfer_matrix.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

#pragma clang fp contract(off)

namespace icn {
namespace {

constexpr int PAIR_QUERIES = 2;              // queries a thread holds in registers (the head of this file says why)
constexpr int PAIR_TILE = MESH_BLOCK;        // targets staged at once
constexpr int PAIR_CHUNK = MESH_BLOCK * PAIR_QUERIES;   // queries a workgroup owns: one partial sum each

__device__ __forceinline__ void nearer(const f3 (&q)[PAIR_QUERIES], float (&best)[PAIR_QUERIES], float x, float y, float z) {
#pragma unroll
    for (int k = 0; k < PAIR_QUERIES; ++k) {
        const float dx = q[k].x - x, dy = q[k].y - y, dz = q[k].z - z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        best[k] = fminf(best[k], d);                                         // the operand that is no NaN; +inf stays +inf
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_pair_sums(const float* __restrict__ qry, const float* __restrict__ tgt, int N, int M,
                                                           double* __restrict__ partial) {
    __shared__ float4 tile4[PAIR_TILE * 3 / 4];                              // the packed (PAIR_TILE, 3) image, 16-byte aligned
    float* tile = reinterpret_cast<float*>(tile4);
    const int tid = threadIdx.x, r = blockIdx.y, g = blockIdx.z;
    const size_t n0 = (size_t)blockIdx.x * PAIR_CHUNK + tid;                 // N <= 0x7fffffff / 3: far from overflow
    const float* p = qry + (size_t)g * N * 3;
    const float* t = tgt + (size_t)r * M * 3;
    f3 q[PAIR_QUERIES];
    float best[PAIR_QUERIES];
#pragma unroll
    for (int k = 0; k < PAIR_QUERIES; ++k) {
        const size_t n = n0 + (size_t)k * MESH_BLOCK;
        q[k] = load3(p + (n < (size_t)N ? n : 0) * 3);                       // threads past N read query 0 of the cloud and add nothing
        best[k] = INFINITY;
    }
    const bool wave_has_queries = n0 - (tid & 63) < (size_t)N;               // the wave's first query of k = 0 exists (wave-uniform)
    for (int j0 = 0; j0 < M; j0 += PAIR_TILE) {
        const int nt = min(PAIR_TILE, M - j0);                               // the same in every thread: words past 3 nt are never read
        __syncthreads();
        for (int w = tid; w < 3 * nt; w += MESH_BLOCK) tile[w] = t[(size_t)j0 * 3 + w];   // j0 + nt <= M: inside cloud r
        __syncthreads();
        if (!wave_has_queries) continue;
        const int whole = nt & ~3;
        for (int jj = 0; jj < whole; jj += 4) {                              // one address for the whole wave: broadcast reads
            const float4 a = tile4[(jj >> 2) * 3], b = tile4[(jj >> 2) * 3 + 1], c = tile4[(jj >> 2) * 3 + 2];
            nearer(q, best, a.x, a.y, a.z);                                  // ascending j
            nearer(q, best, a.w, b.x, b.y);
            nearer(q, best, b.z, b.w, c.x);
            nearer(q, best, c.y, c.z, c.w);
        }
        for (int jj = whole; jj < nt; ++jj) nearer(q, best, tile[3 * jj], tile[3 * jj + 1], tile[3 * jj + 2]);
    }
    double v[1] = {0.0};
#pragma unroll
    for (int k = 0; k < PAIR_QUERIES; ++k) v[0] += n0 + (size_t)k * MESH_BLOCK < (size_t)N ? (double)best[k] : 0.0;
    const size_t pairs = (size_t)gridDim.z * gridDim.y;
    block_sum_store(v, partial + (size_t)blockIdx.x * pairs + ((size_t)g * gridDim.y + r));
}

// sums[pair] = the partials of the pair in ascending chunk order; one thread a pair.
__global__ __launch_bounds__(MESH_BLOCK) void k_pair_sums_finish(const double* __restrict__ partial, size_t pairs, int chunks,
                                                                  double* __restrict__ sums) {
    const size_t at = (size_t)blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (at >= pairs) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += partial[(size_t)c * pairs + at];
    sums[at] = s;
}

}  // namespace

size_t sided_sums_workspace_bytes(int G, int R, int N) {
    return sizeof(double) * (size_t)G * (size_t)R * (size_t)((N + PAIR_CHUNK - 1) / PAIR_CHUNK);
}

void launch_sided_sums(const float* qry, const float* tgt, int G, int R, int N, int M, double* sums, void* ws, hipStream_t s) {
    const int chunks = (N + PAIR_CHUNK - 1) / PAIR_CHUNK;
    const size_t pairs = (size_t)G * R;
    double* partial = static_cast<double*>(ws);
    prof_mark_begin(PROF_PAIR_SUMS, 0.0, s);
    hipLaunchKernelGGL(k_pair_sums, dim3((unsigned)chunks, R, G), dim3(MESH_BLOCK), 0, s, qry, tgt, N, M, partial);
    prof_mark_end(s);
    prof_mark_begin(PROF_PAIR_SUMS_FINISH, 0.0, s);
    hipLaunchKernelGGL(k_pair_sums_finish, dim3((unsigned)((pairs + MESH_BLOCK - 1) / MESH_BLOCK)), dim3(MESH_BLOCK), 0, s, partial, pairs,
                       chunks, sums);
    prof_mark_end(s);
}

}  // namespace icn
