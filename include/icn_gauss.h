/* libicn: discrete Gaussian curvature of triangle meshes by angle defect, with its gradient to the vertices.
 *
 * include/icn.h, include/icn_ext.h, include/icn_measure.h and include/icn_curvature.h are each held to a fixed set of prototypes
 * (tests/test_abi*.py); these entries are exported from the same libicn.so under the same conventions: plain device pointers and
 * ints, the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on success and a
 * negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers, then sizes).
 * ICN_ABI_VERSION stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.SIGNATURES_GAUSS (checked against this header by tests/test_abi_gauss.py).
 *
 * One definition.  vertices (B, V, 3) fp32, faces (F, 3) int32 shared by the batch.  ALL ARITHMETIC UP TO THE FINAL ROUNDING IS
 * DOUBLE: the vertices are widened on load, the outputs are rounded once to fp32.  Per face (i0, i1, i2) and corner k, corner
 * indices modulo 3:
 *   a = v_{k+1} - v_k,  b = v_{k+2} - v_k,  n = (v1 - v0) x (v2 - v0), the cross product of corner 0 with every product rounded
 *   on its own;  theta_k = atan2(|n|, a . b)      (|a x b| = |n| at every corner; no rounded cosine ever meets an acos)
 * The face is RESOLVED iff |n|^2 != 0: a face with two coincident vertices has n exactly 0; a face with a vertex id outside
 * [0, V) takes no part; an unresolved face adds no angle and sends no gradient.  Non-finite vertices are not caught: they
 * propagate NaN into their own mesh only.  Per vertex i
 *   defect_i = 2 pi - sum_{resolved f at i} theta_k(f),   exactly 0 at a vertex that has no resolved face
 * (an unreferenced vertex, or one all of whose faces are unresolved, as lap and varea of icn_curvature.h).  defect_i is the
 * integrated Gaussian curvature of vertex i: intrinsic, dimensionless, and by Gauss-Bonnet sum_i defect_i = 2 pi chi for a closed
 * mesh, 4 pi for every sphere.  Why double: written in fp32 the defect carries an absolute error of 8 - 22 units of 2^-24 whatever
 * the resolution, which is 1e-3 of the defect itself on a smooth mesh of 10 242 vertices, and the errors do not average out.
 *
 * vf_offsets (V + 1) / vf_corners (3 F): the vertex -> corner incidence table of `faces` (see icn_mesh_measure_bwd in
 * icn_measure.h), which the caller builds once per face list.  Either launch runs one thread per (mesh, vertex) that walks its
 * slice in order: no atomics, every output written once, bit-identical run to run.  Safe whatever the tables hold: offsets are
 * clamped into [0, 3 F], an entry c is used only if 0 <= c < 3 F and faces[c] == j, and a face with a vertex id outside [0, V) is
 * skipped (a wrong table gives a wrong result, never an access out of bounds).
 * Every call: 1 <= B <= 65535 (the batch index is gridDim.y), V >= 1, F >= 1, 3 F must fit an int.  No workspace, one launch
 * each on `stream`, no synchronisation. */
#ifndef ICN_GAUSS_H
#define ICN_GAUSS_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* defect (B, V). */
int icn_mesh_angle_defect_fwd(const float* vertices, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners, int B,
                              int V, int F, float* defect, void* stream);

/* Backward of icn_mesh_angle_defect_fwd to the vertices from the upstream gradient ddefect (B, V), for L = sum_i g_i defect_i.
 * With n^ = n / |n|, a resolved face sends to its corner k
 *   (g_{k+1} - g_k) (n^ x a) / |a|^2  +  (g_k - g_{k+2}) (n^ x b) / |b|^2
 * computed in exactly this difference form: a uniform upstream gives dvertices = 0 exactly at every vertex (Gauss-Bonnet: the
 * total curvature cannot be changed).  dvertices (B, V, 3) is written everywhere, with zeros where nothing arrives. */
int icn_mesh_angle_defect_bwd(const float* vertices, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners,
                              const float* ddefect, int B, int V, int F, float* dvertices, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_GAUSS_H */
