// Discrete Gaussian curvature of triangle meshes by angle defect (icn_mesh_angle_defect_fwd / _bwd in include/icn_gauss.h).
// vertices (B, V, 3) fp32, faces (F, 3) shared by the batch.  EVERYTHING BETWEEN THE LOADS AND THE ONE ROUNDING OF THE STORE IS
// DOUBLE: in fp32 the defect carries an absolute error of about 1e-6 whatever the resolution, 1e-3 of the defect itself on a smooth
// I5 mesh, and the errors do not average out (the I5 total misses 4 pi by 1.8e-3).  Per mesh b (blockIdx.y), per face (i0, i1, i2)
// and corner k, corner indices modulo 3:
//   a = v_{k+1} - v_k, b = v_{k+2} - v_k (exact in double: differences of fp32 values less than 2^29 apart in exponent),
//   n = (v1 - v0) x (v2 - v0) with every product rounded on its own (dnormal: exactly 0 for coincident vertices),
//   theta_k = atan2(|n|, a . b);   the face is RESOLVED iff |n|^2 != 0 (NaN counts: it propagates, into its own mesh only)
// and per vertex i:  defect_i = 2 pi - sum_{resolved f at i} theta_k(f),  exactly 0 where no face at i is resolved.
// Both kernels: one thread per (mesh, vertex j), MESH_BLOCK threads, walking j's slice of the vertex -> corner incidence table as
// k_mesh_cotlap_fwd does (icn_curvature.hip; `incident`, icn_mesh_device.h): offsets clamped into [0, 3 F], a corner entry c used
// only if 0 <= c < 3 F and faces[c] == j, faces with ids out of range skipped.  No atomics, a fixed order: bit-identical run to run.
//   k_mesh_angle_defect_fwd   writes defect[b, j].  Vertex j itself is loaded once, the two others of each face per corner.
//   k_mesh_angle_defect_bwd   from the upstream g on defect.  A resolved face sends to its corner k, with n^ = n / |n|,
//                               (g_{k+1} - g_k) (n^ x a) / |a|^2 + (g_k - g_{k+2}) (n^ x b) / |b|^2
//                             in this difference form: equal upstreams give differences that are exactly 0, so a uniform upstream
//                             writes dvertices = 0 exactly (Gauss-Bonnet).  g_j is loaded once, the two others per corner.
// About six atan2 (forward) or thirty divisions (backward) per vertex: the kernels stay gathers out of L2, nothing is staged through
// LDS.  MI355X, I5 / batch 36: 0.024 ms each way beside 0.017 / 0.023 ms for k_mesh_cotlap_fwd / _bwd, the same gathers in fp32
// (profiles/mesh_gauss.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

namespace icn {
namespace {

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_angle_defect_fwd(const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                       const int32_t* __restrict__ offsets,
                                                                       const int32_t* __restrict__ corners, int V, int F,
                                                                       float* __restrict__ defect) {
    const int b = blockIdx.y;
    const long long jl = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;   // past V in the last block, also where V + 255 overflows an int
    if (jl >= V) return;
    const int j = (int)jl;
    const float* v = vts + (size_t)b * V * 3;
    const int nc = 3 * F;                                                    // fits an int (checked by the entry)
    const int lo = min(max(offsets[j], 0), nc), hi = min(max(offsets[j + 1], 0), nc);
    const d3 pj = widened(v + (size_t)j * 3);
    double sum = 0.0;
    bool any = false;
    for (int at = lo; at < hi; ++at) {
        const Incident t = incident(faces, corners, at, j, nc, V);
        if (!t.ok) continue;
        const Corner c = corner(v, t, pj);
        if (c.nn != 0.0) {                                                   // resolved (NaN too: it propagates)
            sum += atan2(sqrt(c.nn), dot(c.a, c.b));
            any = true;
        }
    }
    defect[(size_t)b * V + j] = any ? (float)(6.283185307179586476925 - sum) : 0.f;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_angle_defect_bwd(const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                       const int32_t* __restrict__ offsets,
                                                                       const int32_t* __restrict__ corners, const float* __restrict__ g,
                                                                       int V, int F, float* __restrict__ dvts) {
    const int b = blockIdx.y;
    const long long jl = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;   // past V in the last block, also where V + 255 overflows an int
    if (jl >= V) return;
    const int j = (int)jl;
    const float* v = vts + (size_t)b * V * 3;
    const float* g_b = g + (size_t)b * V;
    const int nc = 3 * F;                                                    // fits an int (checked by the entry)
    const int lo = min(max(offsets[j], 0), nc), hi = min(max(offsets[j + 1], 0), nc);
    const d3 pj = widened(v + (size_t)j * 3);
    const double gj = (double)g_b[j];
    d3 d = {0.0, 0.0, 0.0};
    for (int at = lo; at < hi; ++at) {
        const Incident t = incident(faces, corners, at, j, nc, V);
        if (!t.ok) continue;
        const Corner c = corner(v, t, pj);
        if (c.nn == 0.0) continue;                                           // unresolved: the subgradient 0
        const double g1 = (double)g_b[next_id(t)], g2 = (double)g_b[after_id(t)];
        const double len = sqrt(c.nn);
        const d3 nh = {c.n.x / len, c.n.y / len, c.n.z / len};
        const d3 ra = cross(nh, c.a), rb = cross(nh, c.b);
        const double wa = (g1 - gj) / dot(c.a, c.a), wb = (gj - g2) / dot(c.b, c.b);   // both exactly 0 under a uniform upstream
        d.x += wa * ra.x + wb * rb.x;
        d.y += wa * ra.y + wb * rb.y;
        d.z += wa * ra.z + wb * rb.z;
    }
    float* out = dvts + ((size_t)b * V + j) * 3;
    out[0] = (float)d.x; out[1] = (float)d.y; out[2] = (float)d.z;
}

dim3 vertex_grid(int B, int V) { return dim3((unsigned)(((long long)V + MESH_BLOCK - 1) / MESH_BLOCK), B); }

}  // namespace

void launch_mesh_angle_defect_fwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners, int B, int V,
                                  int F, float* defect, hipStream_t s) {
    prof_mark_begin(PROF_MESH_ANGLE_DEFECT_FWD, 0.0, s);
    hipLaunchKernelGGL(k_mesh_angle_defect_fwd, vertex_grid(B, V), dim3(MESH_BLOCK), 0, s, vts, faces, offsets, corners, V, F, defect);
    prof_mark_end(s);
}

void launch_mesh_angle_defect_bwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners,
                                  const float* ddefect, int B, int V, int F, float* dvts, hipStream_t s) {
    prof_mark_begin(PROF_MESH_ANGLE_DEFECT_BWD, 0.0, s);
    hipLaunchKernelGGL(k_mesh_angle_defect_bwd, vertex_grid(B, V), dim3(MESH_BLOCK), 0, s, vts, faces, offsets, corners, ddefect, V, F,
                       dvts);
    prof_mark_end(s);
}

}  // namespace icn
