/* libicn: cotangent Laplacian and Willmore bending energy of triangle meshes, with their gradients to the vertices.
 *
 * include/icn.h, include/icn_ext.h and include/icn_measure.h are each held to a fixed set of prototypes (tests/test_abi*.py); these
 * entries are exported from the same libicn.so under the same conventions: plain device pointers and ints, the caller owns every
 * buffer, the library allocates nothing and never synchronises, an int entry returns 0 on success and a negative value with
 * icn_last_error() otherwise, and arguments are checked before any device call.  ICN_ABI_VERSION stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.SIGNATURES_CURV (checked against this header by tests/test_abi_curvature.py).
 *
 * One definition.  vertices (B, V, 3), faces (F, 3) int32 shared by the batch.  Per face (i0, i1, i2):
 *   n = (v1 - v0) x (v2 - v0) in fp32 with every product of the cross product rounded on its own (the normal of
 *   icn_mesh_measure_fwd), A_f = 0.5 |n|; the face is RESOLVED iff |n|^2 > 0 and |n|^2 is finite.
 * Per vertex i, with k the corner of f that sits at i and corner indices modulo 3:
 *   varea_i = (sum_{f at i} A_f) / 3                                    the barycentric vertex area
 *   lap_i   = - sum_{f at i, resolved} 0.5 n^_f x (v_{k+2} - v_{k+1})   n^ = n / |n|
 *   w_i     = |lap_i|^2 / (4 varea_i) where varea_i != 0, else 0;   energy[b] = sum_i w_i
 * lap_i is the integrated cotangent Laplace-Beltrami operator sum_j 0.5 (cot alpha_ij + cot beta_ij)(v_j - v_i), which equals
 * - d area / d v_i; this form divides by |n| only, never by a sine.  lap_i = 2 varea_i H normal, so energy[b] is the Willmore
 * energy, the integral of H^2: invariant under scaling, rotation and translation, 4 pi for a sphere of any radius.
 * A face with a vertex id outside [0, V) takes no part in anything; a vertex no face references has lap = 0, varea = 0, w = 0
 * exactly; non-finite vertices propagate.  The energy is summed in double in a fixed order, all outputs are fp32.
 *
 * vf_offsets (V + 1) / vf_corners (3 F): the vertex -> corner incidence table of `faces` (see icn_mesh_measure_bwd in
 * icn_measure.h), which the caller builds once per face list.  Every launch runs one thread per (mesh, vertex) that walks its
 * slice in order: no atomics, bit-identical run to run.  Safe whatever the tables hold: offsets are clamped into [0, 3 F], an
 * entry c is used only if 0 <= c < 3 F and faces[c] == j, and a face with a vertex id outside [0, V) is skipped (a wrong table
 * gives a wrong result, never an access out of bounds).
 * Every call: 1 <= B <= 65535 (the batch index is gridDim.y), V >= 1, F >= 1, 3 F must fit an int. */
#ifndef ICN_CURVATURE_H
#define ICN_CURVATURE_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lap (B, V, 3) and varea (B, V).  One launch on `stream`, no workspace. */
int icn_mesh_cotlap_fwd(const float* vertices, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners, int B, int V,
                        int F, float* lap, float* varea, void* stream);

/* Backward of icn_mesh_cotlap_fwd to the vertices from the upstream gradients dlap (B, V, 3) and dvarea (B, V); either may be NULL
 * and that term is then skipped, with both NULL dvertices (B, V, 3) is written with zeros.  An unresolved face sends nothing to its
 * vertices (the subgradient 0: never NaN from a face without area).  A resolved face with opposite edges e_k = v_{k+2} - v_{k+1},
 * upstreams g_k on lap and a_k on varea at its three vertices sends to its corner k
 *   -0.5 [ (m_perp / |n|) x e_k + (g_{k+1} - g_{k+2}) x n^ ] + (s / 6) n^ x e_k,
 *   m = sum_k e_k x g_k,  m_perp = m - (n^ . m) n^,  s = a_0 + a_1 + a_2.
 * One launch, dvertices[b, j] written once. */
int icn_mesh_cotlap_bwd(const float* vertices, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners,
                        const float* dlap, const float* dvarea, int B, int V, int F, float* dvertices, void* stream);

/* energy (B,), and lap / varea as icn_mesh_cotlap_fwd writes them: the backward needs both.
 * ws: icn_mesh_willmore_workspace_bytes(B, V, F) bytes (host-only query; 16 bytes per vertex of the batch, 0 for sizes the calls
 * reject), 16-byte aligned, owned by the caller; one size serves both directions.  Two launches. */
size_t icn_mesh_willmore_workspace_bytes(int B, int V, int F);
int icn_mesh_willmore_fwd(const float* vertices, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners, int B, int V,
                          int F, float* lap, float* varea, float* energy, void* ws, size_t ws_bytes, void* stream);

/* Backward of the energy to the vertices from denergy (B,), with lap and varea of the forward: per vertex the upstreams
 *   g_i = denergy[b] lap_i / (2 varea_i),  a_i = - denergy[b] |lap_i|^2 / (4 varea_i^2),  both 0 where varea_i = 0
 * into the workspace, then the gather of icn_mesh_cotlap_bwd.  Two launches. */
int icn_mesh_willmore_bwd(const float* vertices, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners,
                          const float* lap, const float* varea, const float* denergy, int B, int V, int F, float* dvertices, void* ws,
                          size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_CURVATURE_H */
