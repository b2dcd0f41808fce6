/* libicn: the sign of the point-to-mesh distance -- inside or outside -- by the angle-weighted pseudonormal of the closest feature.
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS are each held to a fixed set of prototypes
 * (tests/test_abi*.py); this entry is exported from the same libicn.so under the same conventions: plain device pointers and ints,
 * the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on success and a
 * negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers, then sizes).
 * The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of this entry is _lib.LATER_HEADERS (checked against this header by tests/test_abi_sdf.py).
 *
 * One definition.  points (B, P, 3) and vertices (B, V, 3) fp32, faces (F, 3) int32 shared by the batch, face / kind (B, P) int32 as
 * icn_point_to_mesh or icn_point_to_mesh_grid wrote them: kind 0 the interior of the face, 1 / 2 / 3 its vertex 0 / 1 / 2, 4 / 5 / 6
 * its edge (0,1) / (1,2) / (2,0).  ALL ARITHMETIC FROM THE fp32 LOADS TO THE ONE COMPARISON IS DOUBLE.  Per face (i0, i1, i2):
 *   n = (v1 - v0) x (v2 - v0) with every product of the cross product rounded on its own; the face is RESOLVED iff |n|^2 != 0
 *   (a face with two coincident vertices has n exactly 0); n^ = n / |n|.
 * Per point p with its face f and kind:
 *   d = p - q, q the closest point recomputed from (f, kind) as icn_point_to_mesh_bwd does: the vertex; the clamped projection on
 *       the edge's segment (a zero-length edge is its first point); the plane, d = n (ap . n / |n|^2), 0 where |n|^2 = 0
 *   N = n                       for kind 0
 *     = n^_f + n^_g             for kind 4 / 5 / 6, g = adjacency[f][kind - 4] the face across that edge; an unresolved face adds
 *                               nothing, and where there is no g (-1) the edge takes n^_f alone
 *     = sum theta n^            for kind 1 / 2 / 3, over the resolved faces at vertex j = faces[f][kind - 1] in the order of j's slice
 *                               of the incidence table, theta = atan2(|n|, a . b) the face's angle at j (the corner of icn_gauss.h)
 *   sign = -1 (inside) iff d . N < 0, else +1.  A point on the surface, a feature all of whose faces are unresolved and a NaN give +1.
 * The angle-weighted pseudonormal (Baerentzen & Aanaes 2005) makes that sign exact for a closed, consistently wound mesh, counter-
 * clockwise seen from outside, whichever feature is the closest; topology goes by vertex id, two vertices at one position are two
 * vertices.  On an open mesh or one that passes through itself it is the sign defined above and nothing more.
 *
 * adjacency (F, 3): adjacency[f][e] is the face that holds the directed edge opposite to edge e of f, or -1.  vf_offsets (V + 1) /
 * vf_corners (3 F): the vertex -> corner incidence table of `faces` (see icn_mesh_measure_bwd in icn_measure.h).  The caller builds
 * both once per face list.  Safe whatever they and (face, kind) hold: a face outside [0, F), a kind outside [0, 6] or a face with a
 * vertex id outside [0, V) gives +1; an adjacency entry outside [0, F), or one naming a face with a vertex id outside [0, V), adds
 * nothing; offsets are clamped into [0, 3 F] and a corner entry c is used only if 0 <= c < 3 F and faces[c] == j (a wrong table
 * gives a wrong sign, never an access out of bounds).
 * 1 <= B <= 65535 (the batch index is gridDim.y), P >= 1, V >= 1, F >= 1, 3 F must fit an int.  One thread per (mesh, point), no
 * atomics, no workspace, one launch on `stream`, no synchronisation; bit-identical run to run. */
#ifndef ICN_SDF_H
#define ICN_SDF_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* sign (B, P): -1.f or +1.f. */
int icn_point_to_mesh_sign(const float* points, const float* vertices, const int32_t* faces, const int32_t* adjacency,
                           const int32_t* vf_offsets, const int32_t* vf_corners, const int32_t* face, const int32_t* kind,
                           int B, int P, int V, int F, float* sign, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_SDF_H */
