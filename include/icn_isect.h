/* libicn: self-intersection count of triangle meshes -- for every face, the number of other faces of the same mesh it passes through.
 *
 * include/icn.h, include/icn_ext.h, include/icn_measure.h, include/icn_curvature.h and include/icn_gauss.h are each held to a fixed
 * set of prototypes (tests/test_abi*.py); this entry is exported from the same libicn.so under the same conventions: plain device
 * pointers and ints, the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on
 * success and a negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers,
 * then sizes).  The ABI version stays 9: nothing of icn.h changed.
 * The ctypes binding of this entry is _lib.SIGNATURES_ISECT (checked against this header by tests/test_abi_isect.py).
 *
 * One definition.  vertices (B, V, 3) fp32, faces (F, 3) int32 shared by the batch.  ALL ARITHMETIC IS DOUBLE on the vertices as
 * stored, every product and sum rounded on its own (no fused multiply-add), in exactly the order written:
 *   orient(a, b, c, d) = u.x (v.y w.z - v.z w.y) - u.y (v.x w.z - v.z w.x) + u.z (v.x w.y - v.y w.x),  u = b - a, v = c - a, w = d - a
 *   crosses(p, q; a, b, c), a segment against a triangle, holds when
 *     orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs (the signs are compared; no product that could underflow), and
 *     orient(p,q,a,b), orient(p,q,b,c) and orient(p,q,c,a) are all > 0 or all < 0
 *   faces i < j INTERSECT iff one of six tests holds: crosses for each edge (A_k, A_{k+1}) of A = face i against the triangle
 *     B = face j, then for each edge of B against A.  The pair is always evaluated with the lower face index as A, whichever of the
 *     two faces is being counted, so the relation is symmetric by construction.
 * A pair is not tested, and does not intersect, when the two faces share a vertex id (neighbours, duplicate faces), when either has
 * a vertex id outside [0, V), or when either has a coordinate that is not finite.  The strict inequalities make every touching or
 * coplanar contact a non-intersection; in general position two triangles that meet always have an edge piercing an interior.  A face
 * without area can pierce another face with an edge; nothing can pierce it.
 * Because both sides do the same IEEE double operations in the same order, a float64 implementation of these lines reproduces the
 * device's integers exactly (metrics._torch_self_intersections; tests/test_self_intersect.py).
 *
 * One launch on `stream`, one thread per (mesh, face) that visits all other faces of its mesh through tiles in shared memory --
 * O(F^2) per mesh, which is why F is capped -- and rejects pairs whose fp32 bounding boxes do not overlap before any double
 * arithmetic (exact and conservative: it changes no result).  No atomics, every output written once, bit-identical run to run; safe
 * whatever `faces` holds.  No workspace, no synchronisation.
 * 1 <= B <= 65535 (the batch index is gridDim.y), V >= 1, 1 <= F <= ICN_SELF_INTERSECT_MAX_FACES. */
#ifndef ICN_ISECT_H
#define ICN_ISECT_H

#include "icn.h"

#define ICN_SELF_INTERSECT_MAX_FACES (1 << 20)

#ifdef __cplusplus
extern "C" {
#endif

/* hits (B, F): the number of faces of mesh b that face i intersects.  Every row sums to twice the mesh's intersecting pairs. */
int icn_mesh_self_intersect(const float* vertices, const int32_t* faces, int B, int V, int F, int32_t* hits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_ISECT_H */
