// Nearest-neighbour search between batched point sets (icn_nearest_points / icn_nearest_points_bwd in include/icn_nn.h): for every
// point of one set the squared distance to its nearest point in the other set and the index of that point.  points (B, N, 3) fp32,
// targets (B, M, 3) fp32; dist (B, N) fp32, idx (B, N) int32.
// The definition (one, for this kernel, metrics._torch_sided_distance and the tests), ALL OF IT IN fp32 on the values as stored, every
// product and sum rounded on its own in the order written (no contraction: this file is compiled with fp contract(off)):
//   dx = p.x - q_j.x, dy = p.y - q_j.y, dz = p.z - q_j.z,  d_j = (dx dx + dy dy) + dz dz
//   best = +inf, idx = -1; for j = 0 ... M - 1 ascending: if d_j < best then best = d_j, idx = j
// and nothing else: a NaN d_j is never <, a +inf d_j is not < +inf, a query with no acceptable target answers (+inf, -1).
// k_nn_points: grid (ceil(N / (MESH_BLOCK NN_QUERIES)), B).  The targets pass through LDS in tiles of MESH_BLOCK, one float4 per
// target (the fourth word is padding: a tile entry is one 16-byte aligned read), in ascending order; inside the tile loop every lane of a wave
// reads the same address, a broadcast, so the layout has no bank conflicts by construction, and the staging store of lane l goes to
// words 4 l .. 4 l + 3, which covers every bank once per eight lanes.  `d < best` alone, on targets met in ascending order, is the
// lowest-index rule: no minimum trick, the compare and the two selects are the definition.  Every thread keeps NN_QUERIES queries
// (3 coordinates, best, idx each) in registers, query q of thread t being block base + q MESH_BLOCK + t, so that one LDS read serves
// NN_QUERIES distance evaluations of 11 VALU operations each (3 sub, 3 mul, 2 add, 1 compare, 2 selects).  Threads past N hold query
// 0 of the cloud and write nothing; a wave none of whose queries exist stages its share of each tile and skips the arithmetic.
// Every output is written exactly once, (+inf, -1) rows included; no atomics, no workspace, bit-identical run to run.
// WHY NN_QUERIES = 2.  Registers do not decide: hipcc (ROCm 7, -O3) reports 43 / 44 / 52 VGPRs for 1 / 2 / 4 queries (it unrolls the
// tile loop four times), no scratch, 8 waves per SIMD for all of them; the unrolled loop of the two-query kernel is 88 VALU
// instructions and 5 moves for 8 pairs, 11.6 a pair, none of them fused.  The LDS decides against one query: the fourth word is
// never used, so the compiler reads a tile entry as ds_read_b96, 8 LDS cycles a wave, against 11 NN_QUERIES VALU instructions of 2
// cycles each on a SIMD; the four SIMDs of a CU then ask the LDS for 32 cycles in every 22 NN_QUERIES -- more than it has with one
// query, 73 % of it with two, 36 % with four.  The tail decides against four at the shape the library is used at (I5, batch 36:
// N = M = 10 242): a workgroup covers MESH_BLOCK NN_QUERIES queries, so two queries make 20 full workgroups per cloud, 720 for the
// 256 CUs -- at most 3 on a CU where the mean is 2.8 -- while four make 360, at most 2 where the mean is 1.4, and a CU with one
// workgroup, one wave on a SIMD, issues a VALU instruction every 4 cycles, not every 2.  Measured with two: 1.02 ms at that shape,
// 55 % of the VALU issue rate (profiles/nearest_neighbour.txt).  The LDS share is what is left to take: the packed (M, 3) image of a
// tile read as three ds_read_b128 per four targets would ask for 12 LDS cycles where this layout asks for 32.
// Timings on an MI355X: profiles/nearest_neighbour.txt (tools/time_nearest.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

#pragma clang fp contract(off)

namespace icn {
namespace {

constexpr int NN_QUERIES = 2;                // queries a thread holds in registers (the head of this file says why)
constexpr int NN_TILE = MESH_BLOCK;          // targets staged at once: one per thread

__global__ __launch_bounds__(MESH_BLOCK) void k_nn_points(const float* __restrict__ pts, const float* __restrict__ tgt, int N, int M,
                                                           float* __restrict__ dist, int32_t* __restrict__ idx) {
    __shared__ float4 tile[NN_TILE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const size_t n0 = (size_t)blockIdx.x * (MESH_BLOCK * NN_QUERIES) + tid;  // N <= 0x7fffffff / 3: far from overflow
    const float* p = pts + (size_t)b * N * 3;
    const float* t = tgt + (size_t)b * M * 3;
    f3 q[NN_QUERIES];
    float best[NN_QUERIES];
    int at[NN_QUERIES];
#pragma unroll
    for (int k = 0; k < NN_QUERIES; ++k) {
        const size_t n = n0 + (size_t)k * MESH_BLOCK;
        q[k] = load3(p + (n < (size_t)N ? n : 0) * 3);                       // threads past N read query 0 of the cloud and write nothing
        best[k] = INFINITY;
        at[k] = -1;
    }
    const bool wave_has_queries = n0 - (tid & 63) < (size_t)N;               // the wave's first query of k = 0 exists (wave-uniform)
    for (int j0 = 0; j0 < M; j0 += NN_TILE) {
        __syncthreads();
        const int j = j0 + tid;                                              // M <= 0x7fffffff / 3: no overflow
        if (j < M) {
            const f3 v = load3(t + (size_t)j * 3);
            tile[tid] = make_float4(v.x, v.y, v.z, 0.f);
        }
        __syncthreads();
        if (!wave_has_queries) continue;
        const int nt = min(NN_TILE, M - j0);                                 // the same in every thread: entries past it are never read
        for (int jj = 0; jj < nt; ++jj) {
            const float4 v = tile[jj];                                       // one address for the whole wave: a broadcast read
#pragma unroll
            for (int k = 0; k < NN_QUERIES; ++k) {
                const float dx = q[k].x - v.x, dy = q[k].y - v.y, dz = q[k].z - v.z;
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d < best[k]) best[k] = d, at[k] = j0 + jj;               // ascending j: the lowest index among equal d
            }
        }
    }
#pragma unroll
    for (int k = 0; k < NN_QUERIES; ++k) {
        const size_t n = n0 + (size_t)k * MESH_BLOCK;
        if (n < (size_t)N) {
            dist[(size_t)b * N + n] = best[k];
            idx[(size_t)b * N + n] = at[k];
        }
    }
}

// The backward at the forward's choice, one thread per query, in fp32 without contraction: e = p - q_idx, s = 2 g, dpts = s e, and the
// target's share leaves as one VertexRecords entry (id (idx, -1, -1), g = -(s e), w0 = 1) for launch_vertex_scatter.  A query whose idx
// is outside [0, M), or whose e or g is not finite, contributes nothing: id -1, an exact-zero row of dpts.  Nothing is read out of
// bounds whatever `idx` holds.  dpts and rec.id are null where not wanted.
__global__ __launch_bounds__(MESH_BLOCK) void k_nn_points_bwd_record(const float* __restrict__ pts, const float* __restrict__ tgt,
                                                                      const int32_t* __restrict__ idx, const float* __restrict__ ddist,
                                                                      int N, int M, float* __restrict__ dpts, VertexRecords rec) {
    const int b = blockIdx.y, n = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (n >= N) return;
    const size_t at = (size_t)b * N + n;
    int j = idx[at];
    f3 d = {0.f, 0.f, 0.f};
    bool ok = j >= 0 && j < M;
    if (ok) {
        const f3 e = load3(pts + at * 3) - load3(tgt + ((size_t)b * M + j) * 3);
        const float g = ddist[at], s = 2.f * g;
        ok = isfinite(e.x) && isfinite(e.y) && isfinite(e.z) && isfinite(g);
        d = {s * e.x, s * e.y, s * e.z};
    }
    if (!ok) {
        j = -1;
        d = {0.f, 0.f, 0.f};
    }
    if (dpts) dpts[at * 3] = d.x, dpts[at * 3 + 1] = d.y, dpts[at * 3 + 2] = d.z;
    if (rec.id) {
        rec.id[at] = make_int4(j, -1, -1, -1);
        rec.gw[at] = make_float4(-d.x, -d.y, -d.z, 1.f);
        rec.w12[at] = make_float2(0.f, 0.f);
    }
}

}  // namespace

void launch_nearest_points(const float* pts, const float* tgt, int B, int N, int M, float* dist, int32_t* idx, hipStream_t s) {
    const int per_block = MESH_BLOCK * NN_QUERIES;
    prof_mark_begin(PROF_NN, 0.0, s);
    hipLaunchKernelGGL(k_nn_points, dim3((unsigned)((N + per_block - 1) / per_block), B), dim3(MESH_BLOCK), 0, s, pts, tgt, N, M, dist, idx);
    prof_mark_end(s);
}

void launch_nearest_points_bwd(const float* pts, const float* tgt, const int32_t* idx, const float* ddist, int B, int N, int M,
                               float* dpts, float* dtgt, void* ws, hipStream_t s) {
    VertexRecords rec = {nullptr, nullptr, nullptr};
    if (dtgt) rec = vertex_records(ws, (size_t)B * N);
    prof_mark_begin(PROF_NN_BWD_RECORD, 0.0, s);
    hipLaunchKernelGGL(k_nn_points_bwd_record, dim3((unsigned)((N + MESH_BLOCK - 1) / MESH_BLOCK), B), dim3(MESH_BLOCK), 0, s, pts, tgt,
                       idx, ddist, N, M, dpts, rec);
    prof_mark_end(s);
    if (dtgt) launch_vertex_scatter(PROF_NN_BWD_VERTEX, ws, B, N, M, dtgt, s);
}

}  // namespace icn
