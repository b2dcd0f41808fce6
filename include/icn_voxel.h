/* libicn: solid voxelisation of closed triangle meshes by ray parity -- for every cell of a lattice, whether its centre lies inside.
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS and _lib.LATER_HEADERS are each held to a fixed set of
 * prototypes (tests/test_abi*.py); this entry is exported from the same libicn.so under the same conventions: plain device pointers,
 * ints and doubles, the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on
 * success and a negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers,
 * then sizes).  The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of this entry is _lib.UNPINNED_HEADERS (checked against this header by tests/test_abi_voxel.py).
 *
 * One definition.  vertices (B, V, 3) fp32, faces (F, 3) int32 shared by the batch.  The lattice: cell (i, j, k), 0 <= i < n0,
 * 0 <= j < n1, 0 <= k < n2, has its centre at origin + ((i, j, k) + 1/2) spacing.  Rays run along axis 0 and the mesh is projected
 * onto (y, z): a COLUMN is (j, k) with p = (py, pz), py = origin_y + (j + 0.5) h, pz = origin_z + (k + 0.5) h, h = spacing.
 * ALL ARITHMETIC IS DOUBLE on the vertices as stored, every product and sum rounded on its own (no fused multiply-add), in exactly
 * the order written:
 *   A face is TESTED for a column iff its three ids lie in [0, V), its nine coordinates are finite, and lo_y <= py <= hi_y and
 *     lo_z <= pz <= hi_z against the fp32 minimum / maximum of its vertices (exact comparisons).  The box test is part of the
 *     definition, not an optimisation that has to be proved conservative.
 *   The EDGE VALUE of a directed edge u -> w of the face is evaluated in canonical order: (a, b) = (u, w) if id_u < id_w, else (w, u),
 *       s = (b.y - a.y) * (pz - a.z) - (b.z - a.z) * (py - a.y)
 *       t = sign(s);  if t == 0, t = sign(-(b.z - a.z));  if still 0, t = sign(b.y - a.y)
 *     -- the last two are the symbolic perturbation p + (eps, eps^2) -- and if the ends were swapped both s and t are negated.  Two
 *     faces that share an edge therefore evaluate the same expression and get opposite values.
 *   The face COVERS the column iff t > 0 for all three edges or t < 0 for all three.
 *   Its CROSSING DEPTH: with s0, s1, s2 the values (the raw s, not t) of the edges opposite vertices 0, 1, 2, that is of v1 -> v2,
 *     v2 -> v0 and v0 -> v1,
 *       x = (s0 * v0.x + s1 * v1.x + s2 * v2.x) / (s0 + s1 + s2),   tau = (x - origin_x) / h - 0.5
 *     a crossing whose tau is not finite is dropped, otherwise k0 = clamp(ceil(tau), 0, n0).
 *   PARITY: cell i of the column is occupied iff the number of crossings with k0 <= i is odd.
 * It follows that a cell centre exactly on the surface counts the low side as inside ([0, 1) on every axis), that a mesh which
 * passes through itself gets the XOR fill, that the winding of the faces -- consistent or not -- plays no part, and that on a mesh
 * which is not closed a column through the hole is wrong for its whole length (the caller's check, metrics.voxelize, refuses such
 * meshes).  Both sides do the same IEEE double operations in the same order, so a float64 implementation of these lines reproduces
 * the device's bytes exactly (metrics._torch_voxelize; tests/test_voxelize.py).
 *
 * One launch on `stream`: one thread per (mesh, column), workgroups over 16 x 16 tiles of columns with k fastest; the faces pass
 * through tiles in shared memory, where a face that no column of the workgroup would test is dropped (exact: the centres are
 * monotone in j and k), and each column keeps its n0 parity bits private: a crossing flips bit k0, one prefix XOR gives the cells.
 * XOR commutes, so the order of the faces changes nothing.  No atomics, every byte of the output written exactly once, bit-identical
 * run to run; safe whatever `faces` holds.  No workspace, no synchronisation.
 * 1 <= B <= 65535 (the batch index is gridDim.y), V >= 1, 1 <= F <= 0x7fffffff / 3, 1 <= n0 <= ICN_VOXEL_MAX_DEPTH,
 * 1 <= n1, n2 <= ICN_VOXEL_MAX_SIDE; origin and spacing finite, spacing > 0 (anything else fails as `bad sizes`). */
#ifndef ICN_VOXEL_H
#define ICN_VOXEL_H

#include "icn.h"

#define ICN_VOXEL_MAX_DEPTH 512
#define ICN_VOXEL_MAX_SIDE 4096

#ifdef __cplusplus
extern "C" {
#endif

/* occupancy (B, n0, n1, n2) uint8: 1 where the centre of cell (i, j, k) lies inside mesh b, else 0. */
int icn_mesh_voxelize(const float* vertices, const int32_t* faces, int B, int V, int F,
                      double origin_x, double origin_y, double origin_z, double spacing, int n0, int n1, int n2,
                      uint8_t* occupancy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_VOXEL_H */
