// Cotangent Laplacian and Willmore bending energy of triangle meshes (icn_mesh_cotlap_* / icn_mesh_willmore_* in
// include/icn_curvature.h).  vertices (B, V, 3), faces (F, 3) shared by the batch.  Per mesh b (blockIdx.y), per face (i0, i1, i2):
//   n = (v1 - v0) x (v2 - v0) in fp32 with every product of the cross product rounded on its own (face_normal, icn_mesh_device.h;
//       what k_mesh_measure_face computes), A_f = 0.5 |n|; the face is RESOLVED iff |n|^2 > 0 and |n|^2 is finite
// and per vertex i, k = the corner of f that sits at i, corner indices modulo 3:
//   varea_i = (sum_{f at i} A_f) / 3                                       the barycentric vertex area
//   lap_i   = - sum_{f at i, resolved} 0.5 n^_f x (v_{k+2} - v_{k+1})      n^ = n / |n|
//   w_i     = |lap_i|^2 / (4 varea_i) where varea_i != 0, else 0;   energy[b] = sum_i w_i in double in a fixed order -> fp32
// lap_i is the integrated cotangent Laplacian sum_j 0.5 (cot alpha_ij + cot beta_ij)(v_j - v_i) = - d area / d v_i: the cross
// product form divides by |n| only, never by a sine, so a needle costs one factor of its aspect ratio and no cotangent overflows.
// lap_i = 2 varea_i H normal, so w_i = H^2 varea_i and the energy is the Willmore energy, 4 pi for a sphere of any radius.
// A face with a vertex id outside [0, V) takes no part in anything and nothing is read out of bounds; a vertex no face references
// has lap = 0, varea = 0, w = 0 exactly; non-finite vertices propagate (an unresolved NaN face adds NaN to varea).
// Every kernel: one thread per (mesh, vertex j), MESH_BLOCK threads, walking j's slice of the vertex -> corner incidence table
// exactly as k_mesh_measure_bwd does (icn_measure.hip): offsets clamped into [0, 3 F], a corner entry c used only if
// 0 <= c < 3 F and faces[c] == j, faces with ids out of range skipped.  No atomics, a fixed order: bit-identical run to run.
//   k_mesh_cotlap_fwd         writes lap[b, j], varea[b, j]; with `partial` the block's sum of w_j as one double (block_sum_store)
//   k_mesh_willmore_finish    one workgroup per mesh sums the block partials in double (partials_sum) -> energy[b]
//   k_mesh_willmore_upstream  (g_j, a_j) = d energy / d (lap_j, varea_j) = up (lap_j / (2 varea_j), -|lap_j|^2 / (4 varea_j^2)),
//                             0 where varea_j = 0, four floats per vertex
//   k_mesh_cotlap_bwd         from upstreams g on lap and a on varea (either may be null: that term is skipped).  An unresolved face
//                             sends nothing (the subgradient 0).  A resolved face with opposite edges e_k = v_{k+2} - v_{k+1} sends
//                             to its corner k, with m = sum_k e_k x g_k, m_perp = m - (n^ . m) n^, s = a_0 + a_1 + a_2:
//                               -0.5 [ (m_perp / |n|) x e_k + (g_{k+1} - g_{k+2}) x n^ ] + (s / 6) n^ x e_k
//                             thread j sums its own corner of every incident face and writes dvertices[b, j] once.  Each face is
//                             re-read about six times, from L2; nothing is staged through LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

namespace icn {

int mesh_curvature_blocks(int V) { return (int)(((long long)V + MESH_BLOCK - 1) / MESH_BLOCK); }

namespace {

__device__ __forceinline__ bool resolved(float nn) { return nn > 0.f && nn <= 3.4028234663852886e38f; }   // not 0, NaN or overflowed

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_cotlap_fwd(const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ offsets, const int32_t* __restrict__ corners,
                                                                 int V, int F, float* __restrict__ lap, float* __restrict__ varea,
                                                                 double* __restrict__ partial) {
    const int b = blockIdx.y;
    const long long jl = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;   // past V in the last block, also where V + 255 overflows an int
    const float* v = vts + (size_t)b * V * 3;
    const int nc = 3 * F;                                                    // fits an int (checked by the entry)
    double w[1] = {0.0};
    if (jl < V) {
        const int j = (int)jl;
        const int lo = min(max(offsets[j], 0), nc), hi = min(max(offsets[j + 1], 0), nc);
        f3 l = {0.f, 0.f, 0.f};
        float area = 0.f;
        for (int at = lo; at < hi; ++at) {
            const Incident t = incident(faces, corners, at, j, nc, V);
            if (!t.ok) continue;
            const f3 p0 = load3(v + (size_t)t.id[0] * 3), p1 = load3(v + (size_t)t.id[1] * 3), p2 = load3(v + (size_t)t.id[2] * 3);
            const f3 q1 = t.k == 0 ? p1 : (t.k == 1 ? p2 : p0), q2 = t.k == 0 ? p2 : (t.k == 1 ? p0 : p1);   // vertices k + 1 and k + 2
            const f3 n = face_normal(p1 - p0, p2 - p0);
            const float nn = norm2(n), len = sqrtf(nn);
            area += 0.5f * len;
            if (resolved(nn)) l = l - scaled(cross(f3{n.x / len, n.y / len, n.z / len}, q2 - q1), 0.5f);
        }
        area /= 3.f;
        float* out = lap + ((size_t)b * V + j) * 3;
        out[0] = l.x; out[1] = l.y; out[2] = l.z;
        varea[(size_t)b * V + j] = area;
        if (area != 0.f) w[0] = (double)(dot(l, l) / (4.f * area));
    }
    if (partial) block_sum_store(w, partial + (size_t)b * gridDim.x + blockIdx.x);     // uniform over the grid: every thread calls it
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_willmore_finish(const double* __restrict__ partial, int nblocks,
                                                                      float* __restrict__ energy) {
    double s[1];
    partials_sum(partial + (size_t)blockIdx.x * nblocks, nblocks, s);
    if (threadIdx.x == 0) energy[blockIdx.x] = (float)s[0];
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_willmore_upstream(const float* __restrict__ lap, const float* __restrict__ varea,
                                                                        const float* __restrict__ denergy, int V, float4* __restrict__ ga) {
    const int b = blockIdx.y;
    const long long jl = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;   // past V in the last block, also where V + 255 overflows an int
    if (jl >= V) return;
    const int j = (int)jl;
    const size_t at = (size_t)b * V + j;
    const float area = varea[at], up = denergy[b];
    float4 o = {0.f, 0.f, 0.f, 0.f};
    if (area != 0.f) {
        const f3 q = scaled(load3(lap + at * 3), 1.f / (2.f * area));         // H normal: g = up q, a = -up |q|^2 (no varea^2 to underflow)
        o = {up * q.x, up * q.y, up * q.z, -up * dot(q, q)};
    }
    ga[at] = o;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_cotlap_bwd(const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                 const int32_t* __restrict__ offsets, const int32_t* __restrict__ corners,
                                                                 const float* gl, int gl_stride, const float* ga,
                                                                 int ga_stride, int V, int F, float* __restrict__ dvts) {
    const int b = blockIdx.y;
    const long long jl = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;   // past V in the last block, also where V + 255 overflows an int
    if (jl >= V) return;
    const int j = (int)jl;
    const float* v = vts + (size_t)b * V * 3;
    const float* gl_b = gl ? gl + (size_t)b * V * gl_stride : nullptr;       // upstream on lap: 3 floats at gl_b + i * gl_stride
    const float* ga_b = ga ? ga + (size_t)b * V * ga_stride : nullptr;       // upstream on varea: 1 float at ga_b + i * ga_stride
    const int nc = 3 * F;                                                    // fits an int (checked by the entry)
    const int lo = min(max(offsets[j], 0), nc), hi = min(max(offsets[j + 1], 0), nc);
    f3 d = {0.f, 0.f, 0.f};
    for (int at = lo; at < hi; ++at) {
        const Incident t = incident(faces, corners, at, j, nc, V);
        if (!t.ok) continue;
        const f3 p0 = load3(v + (size_t)t.id[0] * 3), p1 = load3(v + (size_t)t.id[1] * 3), p2 = load3(v + (size_t)t.id[2] * 3);
        const f3 n = face_normal(p1 - p0, p2 - p0);                          // as the forward: exactly 0 for coincident vertices
        const float nn = norm2(n);
        if (!resolved(nn)) continue;                                         // the subgradient 0, through lap and through varea
        const float len = sqrtf(nn);
        const f3 nh = {n.x / len, n.y / len, n.z / len};
        const f3 e0 = p2 - p1, e1 = p0 - p2, e2 = p1 - p0;
        const f3 ek = t.k == 0 ? e0 : (t.k == 1 ? e1 : e2);
        if (gl_b) {
            const f3 g0 = load3(gl_b + (size_t)t.id[0] * gl_stride), g1 = load3(gl_b + (size_t)t.id[1] * gl_stride),
                     g2 = load3(gl_b + (size_t)t.id[2] * gl_stride);
            const f3 m = cross(e0, g0) + cross(e1, g1) + cross(e2, g2);
            const f3 mp = m - scaled(nh, dot(nh, m));
            const f3 q1 = t.k == 0 ? g1 : (t.k == 1 ? g2 : g0), q2 = t.k == 0 ? g2 : (t.k == 1 ? g0 : g1);    // g of corners k + 1, k + 2
            d = d - scaled(cross(scaled(mp, 1.f / len), ek) + cross(q1 - q2, nh), 0.5f);
        }
        if (ga_b) {
            const float s = ga_b[(size_t)t.id[0] * ga_stride] + ga_b[(size_t)t.id[1] * ga_stride] + ga_b[(size_t)t.id[2] * ga_stride];
            d = d + scaled(cross(nh, ek), s / 6.f);
        }
    }
    float* out = dvts + ((size_t)b * V + j) * 3;
    out[0] = d.x; out[1] = d.y; out[2] = d.z;
}

dim3 vertex_grid(int B, int V) { return dim3(mesh_curvature_blocks(V), B); }

void cotlap_bwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners, const float* gl, int gl_stride,
                const float* ga, int ga_stride, int B, int V, int F, float* dvts, hipStream_t s) {
    prof_mark_begin(PROF_MESH_COTLAP_BWD, 0.0, s);
    hipLaunchKernelGGL(k_mesh_cotlap_bwd, vertex_grid(B, V), dim3(MESH_BLOCK), 0, s, vts, faces, offsets, corners, gl, gl_stride, ga,
                       ga_stride, V, F, dvts);
    prof_mark_end(s);
}

}  // namespace

// one workspace for both directions: the backward's four floats per vertex; the forward's one double per mesh and block of
// MESH_BLOCK vertices fits in it
size_t mesh_willmore_bytes(int B, int V) { return (size_t)B * V * sizeof(float4); }

void launch_mesh_cotlap_fwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners, int B, int V, int F,
                            float* lap, float* varea, hipStream_t s) {
    prof_mark_begin(PROF_MESH_COTLAP_FWD, 0.0, s);
    hipLaunchKernelGGL(k_mesh_cotlap_fwd, vertex_grid(B, V), dim3(MESH_BLOCK), 0, s, vts, faces, offsets, corners, V, F, lap, varea,
                       static_cast<double*>(nullptr));
    prof_mark_end(s);
}

void launch_mesh_cotlap_bwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners, const float* dlap,
                            const float* dvarea, int B, int V, int F, float* dvts, hipStream_t s) {
    cotlap_bwd(vts, faces, offsets, corners, dlap, 3, dvarea, 1, B, V, F, dvts, s);
}

void launch_mesh_willmore_fwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners, int B, int V, int F,
                              float* lap, float* varea, float* energy, void* ws, hipStream_t s) {
    double* partial = static_cast<double*>(ws);                              // mesh_willmore_bytes(B, V), 16-byte aligned
    const int nblocks = mesh_curvature_blocks(V);
    prof_mark_begin(PROF_MESH_COTLAP_FWD, 0.0, s);
    hipLaunchKernelGGL(k_mesh_cotlap_fwd, vertex_grid(B, V), dim3(MESH_BLOCK), 0, s, vts, faces, offsets, corners, V, F, lap, varea,
                       partial);
    prof_mark_end(s);
    prof_mark_begin(PROF_MESH_WILLMORE_FINISH, 0.0, s);
    hipLaunchKernelGGL(k_mesh_willmore_finish, dim3(B), dim3(MESH_BLOCK), 0, s, partial, nblocks, energy);
    prof_mark_end(s);
}

void launch_mesh_willmore_bwd(const float* vts, const int32_t* faces, const int32_t* offsets, const int32_t* corners, const float* lap,
                              const float* varea, const float* denergy, int B, int V, int F, float* dvts, void* ws, hipStream_t s) {
    float4* ga = static_cast<float4*>(ws);                                   // mesh_willmore_bytes(B, V), 16-byte aligned
    prof_mark_begin(PROF_MESH_WILLMORE_UPSTREAM, 0.0, s);
    hipLaunchKernelGGL(k_mesh_willmore_upstream, vertex_grid(B, V), dim3(MESH_BLOCK), 0, s, lap, varea, denergy, V, ga);
    prof_mark_end(s);
    const float* g = reinterpret_cast<const float*>(ga);
    cotlap_bwd(vts, faces, offsets, corners, g, 4, g + 3, 4, B, V, F, dvts, s);
}

}  // namespace icn
