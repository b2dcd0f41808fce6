// Sign of the point-to-mesh distance by the angle-weighted pseudonormal (icn_point_to_mesh_sign in include/icn_sdf.h; Baerentzen &
// Aanaes 2005).  points (B, P, 3), vertices (B, V, 3) fp32, faces (F, 3) shared by the batch, (face, kind) (B, P) as the forward of
// icn_point_to_mesh / icn_point_to_mesh_grid left them.  EVERYTHING BETWEEN THE LOADS AND THE ONE COMPARISON IS DOUBLE, as in
// icn_gauss.hip, whose corner arithmetic this shares (Corner / corner, icn_mesh_device.h).  Per mesh b (blockIdx.y) and point p with
// its face f = (i0, i1, i2), n = (v1 - v0) x (v2 - v0) with every product rounded on its own (dnormal), RESOLVED iff |n|^2 != 0,
// n^ = n / |n|:
//   d = p - q, q recomputed from (f, kind) with the expressions of k_point_to_mesh_bwd_point (icn_loss.hip): the vertex; the clamped
//       projection on the edge's segment (a zero-length edge is its first point); the plane, d = n (ap . n / |n|^2), 0 where |n|^2 = 0
//   N = n                                      kind 0
//       n^_f + n^_g, g = adjacency[f][kind - 4]  kind 4 / 5 / 6: the face across that edge; an unresolved face adds nothing, and
//                                              neither does a g outside [0, F) or one with a vertex id outside [0, V)
//       sum theta n^ over the resolved faces   kind 1 / 2 / 3: over the slice of vertex j = faces[f][kind - 1] in the vertex -> corner
//                                              incidence table, in slice order, theta = atan2(|n|, a . b) the face's angle at j;
//                                              offsets clamped into [0, 3 F], entries filtered by `incident`
//   sign = -1 iff d . N < 0, else +1           (a point on the surface, an all-degenerate feature, a NaN: +1)
// A face outside [0, F), a kind outside [0, 6] or a vertex id of f outside [0, V) gives +1; nothing is read out of bounds whatever
// the tables hold.
//   k_p2m_sign   one thread per (mesh, point), MESH_BLOCK threads: no LDS, no atomics, no workspace, one float per point.  A gather
//                out of L2 like k_mesh_angle_defect_fwd: at most `valence` faces and about six atan2, on the vertex kinds only; the
//                lanes of a wave take different branches by kind.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

namespace icn {
namespace {

// p - (the closest point of the segment u + t uw, t in [0, 1]) for up = p - u: seg_diff of icn_loss.hip in double
__device__ __forceinline__ d3 dseg_diff(d3 up, d3 uw) {
    const double den = dot(uw, uw);
    double t = den != 0.0 ? dot(uw, up) / den : 0.0;
    t = !(t > 0.0) ? 0.0 : (t < 1.0 ? t : 1.0);
    return {up.x - uw.x * t, up.y - uw.y * t, up.z - uw.z * t};
}

// N += w n / |n| for a resolved normal (nn = |n|^2 != 0; NaN counts: it propagates)
__device__ __forceinline__ void add_unit(d3& N, d3 n, double nn, double w) {
    if (nn != 0.0) {
        const double len = sqrt(nn);
        N.x += w * (n.x / len);
        N.y += w * (n.y / len);
        N.z += w * (n.z / len);
    }
}

__global__ __launch_bounds__(MESH_BLOCK) void k_p2m_sign(const float* __restrict__ pts, const float* __restrict__ vts,
                                                          const int32_t* __restrict__ faces, const int32_t* __restrict__ adjacency,
                                                          const int32_t* __restrict__ offsets, const int32_t* __restrict__ corners,
                                                          const int32_t* __restrict__ face, const int32_t* __restrict__ kind, int P,
                                                          int V, int F, float* __restrict__ sign) {
    const int b = blockIdx.y;
    const long long il = (long long)blockIdx.x * MESH_BLOCK + threadIdx.x;   // past P in the last block, also where P + 255 overflows an int
    if (il >= P) return;
    const size_t at = (size_t)b * P + (size_t)il;
    const int f = face[at], k = kind[at];
    float out = 1.f;
    if (f >= 0 && f < F && k >= 0 && k <= 6) {
        const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
        if (ids_ok(i0, i1, i2, V)) {
            const float* v = vts + (size_t)b * V * 3;
            const d3 p = widened(pts + at * 3);
            const d3 a = widened(v + (size_t)i0 * 3), bb = widened(v + (size_t)i1 * 3), c = widened(v + (size_t)i2 * 3);
            d3 d, N = {0.0, 0.0, 0.0};
            if (k == 0 || k >= 4) {
                const d3 ab = bb - a, ac = c - a, ap = p - a;
                const d3 n = dnormal(ab, ac);
                const double nn = dot(n, n);
                if (k == 0) {                                                // the plane
                    const double s = nn != 0.0 ? dot(ap, n) / nn : 0.0;
                    d = {n.x * s, n.y * s, n.z * s};
                    N = n;
                } else {                                                     // an edge: this face and the one across it
                    d = k == 4 ? dseg_diff(ap, ab) : (k == 5 ? dseg_diff(p - bb, c - bb) : dseg_diff(ap, ac));
                    add_unit(N, n, nn, 1.0);
                    const int g = adjacency[(size_t)f * 3 + (k - 4)];
                    if (g >= 0 && g < F) {
                        const int g0 = faces[(size_t)g * 3], g1 = faces[(size_t)g * 3 + 1], g2 = faces[(size_t)g * 3 + 2];
                        if (ids_ok(g0, g1, g2, V)) {
                            const d3 ga = widened(v + (size_t)g0 * 3);
                            const d3 m = dnormal(widened(v + (size_t)g1 * 3) - ga, widened(v + (size_t)g2 * 3) - ga);
                            add_unit(N, m, dot(m, m), 1.0);
                        }
                    }
                }
            } else {                                                         // a vertex: every resolved face around it, by its angle
                const int j = k == 1 ? i0 : (k == 2 ? i1 : i2);
                const d3 pj = k == 1 ? a : (k == 2 ? bb : c);
                d = p - pj;
                const int nc = 3 * F;                                        // fits an int (checked by the entry)
                const int lo = min(max(offsets[j], 0), nc), hi = min(max(offsets[j + 1], 0), nc);
                for (int s = lo; s < hi; ++s) {
                    const Incident t = incident(faces, corners, s, j, nc, V);
                    if (!t.ok) continue;
                    const Corner cr = corner(v, t, pj);
                    if (cr.nn != 0.0) add_unit(N, cr.n, cr.nn, atan2(sqrt(cr.nn), dot(cr.a, cr.b)));
                }
            }
            if (dot(d, N) < 0.0) out = -1.f;                                 // NaN compares false: +1
        }
    }
    sign[at] = out;
}

}  // namespace

void launch_point_to_mesh_sign(const float* pts, const float* vts, const int32_t* faces, const int32_t* adjacency, const int32_t* offsets,
                               const int32_t* corners, const int32_t* face, const int32_t* kind, int B, int P, int V, int F, float* sign,
                               hipStream_t s) {
    prof_mark_begin(PROF_P2M_SIGN, 0.0, s);
    hipLaunchKernelGGL(k_p2m_sign, dim3((unsigned)(((long long)P + MESH_BLOCK - 1) / MESH_BLOCK), B), dim3(MESH_BLOCK), 0, s, pts, vts,
                       faces, adjacency, offsets, corners, face, kind, P, V, F, sign);
    prof_mark_end(s);
}

}  // namespace icn
