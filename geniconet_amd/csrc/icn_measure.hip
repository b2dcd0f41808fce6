// Surface area and enclosed volume of triangle meshes (icn_mesh_measure_fwd / icn_mesh_measure_bwd in include/icn_measure.h).
// vertices (B, V, 3), faces (F, 3) shared by the batch.  Per mesh b (blockIdx.y), per face (i0, i1, i2):
//   A_f = 0.5 |n|, n = (v1 - v0) x (v2 - v0) in fp32 with every product of the cross product rounded on its own (face_normal,
//         icn_mesh_device.h; exactly what k_msample_area computes): a face with two coincident vertices has area exactly 0
//   T_f = (v0 - o) . ((v1 - o) x (v2 - o)) in fp32, o = vertices[b, 0]: about the mesh's own vertex 0 the triple products stay of
//         the size of the mesh, wherever the mesh sits (about the origin a mesh of radius 0.75 translated by 10 loses three digits)
//   area[b] = sum_f A_f, volume[b] = sum_f T_f / 6, both sums in double in a fixed order, the results fp32.
// A face with a vertex id outside [0, V) contributes 0 to both and nothing is read out of bounds; non-finite vertices propagate.
//   k_mesh_measure_face    grid (blocks of MEASURE_SPAN faces, B): thread t of block k takes faces k * MEASURE_SPAN + t + 256 i,
//                          i = 0 .. MEASURE_PER_THREAD - 1; the block sums (A_f, T_f) in double -- xor shuffles inside a wave, then
//                          a tree over the 4 wave totals -- and writes two doubles into the workspace
//   k_mesh_measure_finish  one workgroup per mesh: lanes stride over the block partials, a fixed tree -> area[b], volume[b]
// Backward, from the upstream darea / dvolume (B,), either may be null (that term is skipped; both null: zeros).  For corner k of
// face f, with o held constant:
//   d volume / d v_k = ((v_{k+1} - o) x (v_{k+2} - o)) / 6;   d area / d v_k = (n^ x (v_{k+2} - v_{k+1})) / 2,  n^ = n / |n|,
//   the area term taken as 0 where |n|^2 is 0 or not finite (the subgradient: never NaN from a face without area).
//   k_mesh_measure_bwd     one thread per (mesh, vertex j): walks j's slice of the vertex -> corner incidence table -- offsets
//                          (V + 1), corners (3 F) with entries c = 3 f + k grouped by vertex, ascending within a vertex; the caller
//                          builds it once per face list -- gathers the three vertices of each incident face and writes
//                          dvertices[b, j] once.  O(valence) per vertex, O(F) per mesh, against the (records x V) integer compares
//                          of k_vertex_scatter; no atomics, a fixed order: bit-identical run to run, an exact 0 at a vertex no
//                          face references.  Safe whatever the tables hold: offsets are clamped into [0, 3 F], a corner entry c
//                          is used only if 0 <= c < 3 F and faces[c] == j, a face with a vertex id outside [0, V) is skipped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

namespace icn {

namespace {

constexpr int MEASURE_PER_THREAD = 4;
constexpr int MEASURE_SPAN = MESH_BLOCK * MEASURE_PER_THREAD;                // faces of one block: 1024

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_measure_face(const float* __restrict__ vts, const int32_t* __restrict__ faces, int V,
                                                                   int F, double* __restrict__ partial) {
    const int b = blockIdx.y;
    const float* v = vts + (size_t)b * V * 3;
    const f3 o = load3(v);                                                   // vertex 0 (V >= 1)
    double area = 0.0, trip = 0.0;
#pragma unroll
    for (int i = 0; i < MEASURE_PER_THREAD; ++i) {
        const long long f = (long long)blockIdx.x * MEASURE_SPAN + i * MESH_BLOCK + threadIdx.x;
        if (f >= F) break;
        const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        if (!ids_ok(i0, i1, i2, V)) continue;
        const f3 p0 = load3(v + (size_t)i0 * 3), p1 = load3(v + (size_t)i1 * 3), p2 = load3(v + (size_t)i2 * 3);
        area += (double)(0.5f * sqrtf(norm2(face_normal(p1 - p0, p2 - p0))));
        trip += (double)dot(p0 - o, cross(p1 - o, p2 - o));
    }
    double sums[2] = {area, trip};
    block_sum_store(sums, partial + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_measure_finish(const double* __restrict__ partial, int nblocks,
                                                                     float* __restrict__ area, float* __restrict__ volume) {
    double sums[2];
    partials_sum(partial + (size_t)blockIdx.x * nblocks * 2, nblocks, sums);
    if (threadIdx.x == 0) {
        area[blockIdx.x] = (float)sums[0];
        volume[blockIdx.x] = (float)(sums[1] / 6.0);
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_measure_bwd(const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                  const int32_t* __restrict__ offsets, const int32_t* __restrict__ corners,
                                                                  const float* __restrict__ darea, const float* __restrict__ dvolume,
                                                                  int V, int F, float* __restrict__ dvts) {
    const int b = blockIdx.y, j = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (j >= V) return;
    const float* v = vts + (size_t)b * V * 3;
    const int nc = 3 * F;                                                    // fits an int (checked by the entry)
    const int lo = min(max(offsets[j], 0), nc), hi = min(max(offsets[j + 1], 0), nc);
    const float ga = darea ? 0.5f * darea[b] : 0.f, gv = dvolume ? dvolume[b] / 6.f : 0.f;
    const f3 o = load3(v);
    f3 g = {0.f, 0.f, 0.f};
    for (int at = lo; at < hi; ++at) {
        const int c = corners[at];
        if (c < 0 || c >= nc || faces[c] != j) continue;
        const int f = c / 3, k = c - 3 * f;
        const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
        if (!ids_ok(i0, i1, i2, V)) continue;
        const f3 p0 = load3(v + (size_t)i0 * 3), p1 = load3(v + (size_t)i1 * 3), p2 = load3(v + (size_t)i2 * 3);
        const f3 q1 = k == 0 ? p1 : (k == 1 ? p2 : p0), q2 = k == 0 ? p2 : (k == 1 ? p0 : p1);      // vertices k + 1 and k + 2
        if (dvolume) g = g + scaled(cross(q1 - o, q2 - o), gv);
        if (darea) {
            const f3 n = face_normal(p1 - p0, p2 - p0);                      // as the forward: exactly 0 for coincident vertices
            const float nn = norm2(n);
            if (nn > 0.f && nn <= 3.4028234663852886e38f) {                  // not 0, NaN or overflowed: else the subgradient 0
                const float len = sqrtf(nn);
                g = g + scaled(cross(f3{n.x / len, n.y / len, n.z / len}, q2 - q1), ga);
            }
        }
    }
    float* out = dvts + ((size_t)b * V + j) * 3;
    out[0] = g.x; out[1] = g.y; out[2] = g.z;
}

}  // namespace

int mesh_measure_blocks(int F) { return (F + MEASURE_SPAN - 1) / MEASURE_SPAN; }

size_t mesh_measure_bytes(int B, int F) { return (size_t)B * mesh_measure_blocks(F) * 2 * sizeof(double); }

void launch_mesh_measure_fwd(const float* vts, const int32_t* faces, int B, int V, int F, float* area, float* volume, void* ws,
                             hipStream_t s) {
    double* partial = static_cast<double*>(ws);                              // mesh_measure_bytes(B, F), 16-byte aligned
    const int nblocks = mesh_measure_blocks(F);
    prof_mark_begin(PROF_MESH_MEASURE_FACE, 0.0, s);
    hipLaunchKernelGGL(k_mesh_measure_face, dim3(nblocks, B), dim3(MESH_BLOCK), 0, s, vts, faces, V, F, partial);
    prof_mark_end(s);
    prof_mark_begin(PROF_MESH_MEASURE_FINISH, 0.0, s);
    hipLaunchKernelGGL(k_mesh_measure_finish, dim3(B), dim3(MESH_BLOCK), 0, s, partial, nblocks, area, volume);
    prof_mark_end(s);
}

void launch_mesh_measure_bwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners, const float* darea,
                             const float* dvolume, int B, int V, int F, float* dvts, hipStream_t s) {
    prof_mark_begin(PROF_MESH_MEASURE_BWD, 0.0, s);
    hipLaunchKernelGGL(k_mesh_measure_bwd, dim3((V + MESH_BLOCK - 1) / MESH_BLOCK, B), dim3(MESH_BLOCK), 0, s, vts, faces, offsets, corners,
                       darea, dvolume, V, F, dvts);
    prof_mark_end(s);
}

}  // namespace icn
