/* libicn: surface area and enclosed volume of triangle meshes, with their gradient to the vertices.
 *
 * include/icn.h and include/icn_ext.h are each held to a fixed set of prototypes (tests/test_abi.py, tests/test_abi_ext.py); these
 * entries are exported from the same libicn.so under the same conventions: plain device pointers and ints, the caller owns every
 * buffer, the library allocates nothing and never synchronises, an int entry returns 0 on success and a negative value with
 * icn_last_error() otherwise, and arguments are checked before any device call.  ICN_ABI_VERSION stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.SIGNATURES_MEASURE (checked against this header by tests/test_abi_measure.py). */
#ifndef ICN_MEASURE_H
#define ICN_MEASURE_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* area (B,) and volume (B,) of B meshes: vertices (B, V, 3), faces (F, 3) int32 shared by the batch.  Per face (i0, i1, i2):
 *   A_f = 0.5 |n|, n = (v1 - v0) x (v2 - v0) in fp32 with every product of the cross product rounded on its own (the area of
 *   icn_mesh_sample_fwd): a face with two coincident vertices has area exactly 0;
 *   T_f = (v0 - o) . ((v1 - o) x (v2 - o)) in fp32 with o = vertices[b, 0], the mesh's own vertex 0 (about the origin a mesh that
 *   sits away from it loses the digits of its offset);
 *   area[b] = sum_f A_f;  volume[b] = sum_f T_f / 6, signed: positive for outward (counter-clockwise seen from outside) winding.
 * For a closed, consistently wound mesh the volume does not depend on o; for an open mesh it is the volume of the cone over o.
 * Both sums run in double in a fixed order (bit-identical run to run), the outputs are fp32.  A face with a vertex id outside
 * [0, V) contributes 0 to both and nothing is read out of bounds.  Non-finite vertices propagate (NaN in, NaN out): these are
 * global measures of a mesh.
 * ws: icn_mesh_measure_workspace_bytes(B, V, F) bytes (host-only query; 16 bytes per mesh and block of 1024 faces, 0 for sizes the
 * call rejects), 16-byte aligned, owned by the caller.  Two launches on `stream`.  B <= 65535 per call (the batch index is
 * gridDim.y), 3 F must fit an int.  0 on success, negative with icn_last_error() otherwise. */
size_t icn_mesh_measure_workspace_bytes(int B, int V, int F);
int icn_mesh_measure_fwd(const float* vertices, const int32_t* faces, int B, int V, int F, float* area, float* volume, void* ws,
                         size_t ws_bytes, void* stream);

/* Backward of icn_mesh_measure_fwd to the vertices from the upstream gradients darea (B,) and dvolume (B,); either may be NULL and
 * that term is then skipped, with both NULL dvertices is written with zeros.  For corner k of face f, o held constant:
 *   d volume / d v_k = ((v_{k+1} - o) x (v_{k+2} - o)) / 6;   d area / d v_k = (n^ x (v_{k+2} - v_{k+1})) / 2,  n^ = n / |n|,
 * the area term taken as 0 where |n|^2 is 0 or not finite (the subgradient: never NaN from a face without area).
 * vf_offsets (V + 1) / vf_corners (3 F): the vertex -> corner incidence table of `faces`, which the caller builds once per face
 * list: vf_corners holds the corners c = 3 f + k grouped by the vertex faces[c], ascending in c within a vertex, and the corners
 * of vertex j are vf_corners[vf_offsets[j] .. vf_offsets[j + 1]).  One launch, one thread per (mesh, vertex): it walks its slice
 * in order, gathers the three vertices of each incident face and writes dvertices[b, j] (B, V, 3) once -- O(F) per mesh, no
 * atomics, no workspace; bit-identical run to run, and a vertex no face references gets an exact zero.  Safe whatever the tables
 * hold: offsets are clamped into [0, 3 F], an entry c is used only if 0 <= c < 3 F and faces[c] == j, and a face with a vertex id
 * outside [0, V) is skipped (a wrong table gives a wrong gradient, never an access out of bounds).
 * B <= 65535 per call, 3 F must fit an int.  0 on success, negative with icn_last_error() otherwise. */
int icn_mesh_measure_bwd(const float* vertices, const int32_t* faces, const int32_t* vf_offsets, const int32_t* vf_corners,
                         const float* darea, const float* dvolume, int B, int V, int F, float* dvertices, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_MEASURE_H */
