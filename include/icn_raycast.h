/* libicn: ray casting against batched triangle meshes -- for every ray the first face it meets, the parameter of that hit and the
 * number of faces it crosses -- and the backward of that parameter.
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS and _lib.LATER_HEADERS are each held to a fixed set of
 * prototypes (tests/test_abi*.py); these entries are exported from the same libicn.so under the same conventions: plain device
 * pointers and ints, the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on
 * success and a negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers,
 * then sizes).  The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.UNPINNED_HEADERS (checked against this header by tests/test_abi_raycast.py).
 *
 * One definition.  vertices (B, V, 3) fp32, faces (F, 3) int32 shared by the batch, origins and directions (B, R, 3) fp32; a
 * direction need not be a unit vector.  ALL ARITHMETIC IS DOUBLE on the values as stored, every product and sum rounded on its own (no
 * fused multiply-add), in exactly the order written:
 *   A ray is LIVE iff its six values are finite and d != (0, 0, 0).  A ray that is not live answers a miss: depth +inf, face -1,
 *     count 0.
 *   A face is TESTED iff its three ids lie in [0, V) and its nine coordinates are finite.  For a tested face (i0, i1, i2) let
 *     p_k = v_k - o.
 *   The EDGE VALUE of a directed edge u -> w of the face is evaluated in canonical order: (a, b) = (p_u, p_w) if id_u < id_w, else
 *     (p_w, p_u),
 *       N = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x)
 *       s = (d.x * N.x + d.y * N.y) + d.z * N.z
 *       tau = sign(s);  if tau == 0, tau = sign(N.x);  if still 0, tau = sign(N.y);  if still 0, tau = sign(N.z)
 *     -- the last three are the symbolic perturbation d + (eps, eps^2, eps^3) -- and if the ends were swapped both s and tau are
 *     negated.  Two faces that share an edge therefore evaluate the same expression and get opposite values.  A face with a repeated
 *     id gets tau = 0 on that edge.
 *   The face COVERS the ray iff tau > 0 for all three edges or tau < 0 for all three.
 *   Its PARAMETER: with s0, s1, s2 the values (the raw s, not tau) of the edges opposite vertices 0, 1, 2, that is of v1 -> v2,
 *     v2 -> v0 and v0 -> v1,
 *       c_k = (p_k.x * d.x + p_k.y * d.y) + p_k.z * d.z,   S = (s0 + s1) + s2,   dd = (d.x * d.x + d.y * d.y) + d.z * d.z
 *       t = ((s0 * c0 + s1 * c1) + s2 * c2) / (S * dd)
 *   A HIT is a covering face whose t is finite and > 0.
 *   count = the number of hits.  face = the hit with the smallest t, the lowest face index among equal t, -1 if there is none.
 *   depth = that t rounded once to fp32, else +inf; it is in units of |d|.  A t beyond fp32 rounds to +inf while face >= 0: the face is
 *   what tells a hit.
 * It follows that on a closed mesh the parity of count is the inside test of the origin whatever the winding of the faces (every
 * edge is claimed by exactly one of its two faces, whatever passes through an edge or a vertex), that a mesh which passes through
 * itself gets the XOR, and that an origin exactly on the surface does not count that surface (t = 0 is no hit).  Both sides do the
 * same IEEE double operations in the same order, so a float64 implementation of these lines reproduces the device's bits exactly
 * (metrics._torch_ray_cast; tests/test_ray_cast.py).
 *
 * icn_mesh_raycast: one launch on `stream`, one thread per (mesh, ray); the faces pass through tiles in shared memory, where a face
 * that is not tested is dropped, in ascending order, so the tie rule costs nothing.  In front of the double arithmetic stands an fp32
 * filter that skips a face only where it is PROVED not to cover the ray -- the ray's line at least 1.5 radii from the face's centroid
 * and not within 2^-16 of the face's plane, and only where the filter's own fp32 values neither underflow nor overflow; the proof, which
 * bounds the rounding of the computed edge values, is in the kernel file
 * (geniconet_amd/csrc/icn_raycast.hip) -- so it is no part of the definition and changes no result.  No atomics, every output written
 * exactly once (misses too), bit-identical run to run; safe whatever `faces` holds.  No workspace, no synchronisation.
 *
 * icn_mesh_raycast_bwd: the gradient of depth at a FIXED face choice, from the forward's `face` and the upstream ddepth (B, R), in
 * double and rounded once.  With n = (v1 - v0) x (v2 - v0) (no contraction), nd = n . d, w_k = s_k / S and t as above:
 *       G = ddepth * n / nd;   d/dv_k = w_k G;   d/do = -G;   d/dd = -t G
 * A ray contributes nothing, and its rows of dorigins / ddirections are exact zeros, when its face is outside [0, F), the face has
 * an id outside [0, V), nd is 0, or any of the above is not finite; nothing is read out of bounds whatever `face` holds.  The vertex
 * gradient goes through one record per ray (ids, (float)G, (float)w_k) and is then summed per vertex in a fixed order with no atomics:
 * bit-identical run to run, and a vertex that no ray touches gets an exact 0.  The three gradient pointers are optional: one that is
 * given is written whole; with all three null nothing is launched and the call returns 0.  ws -- only looked at when dvertices is
 * given -- holds icn_mesh_raycast_bwd_workspace_bytes(B, R, V) = 40 * B * R bytes (0 for sizes the call rejects), 16-byte aligned.
 * One launch, and a second when dvertices is given.
 * 1 <= B <= 65535 (the batch index is gridDim.y), V >= 1, 1 <= F, R <= 0x7fffffff / 3 (anything else fails as `bad sizes`). */
#ifndef ICN_RAYCAST_H
#define ICN_RAYCAST_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* depth (B, R) fp32, face (B, R) int32, count (B, R) int32 of the rays origins + t directions against mesh b. */
int icn_mesh_raycast(const float* origins, const float* directions, const float* vertices, const int32_t* faces,
                     int B, int R, int V, int F, float* depth, int32_t* face, int32_t* count, void* stream);

size_t icn_mesh_raycast_bwd_workspace_bytes(int B, int R, int V);

/* dorigins, ddirections (B, R, 3) and dvertices (B, V, 3): each may be null. */
int icn_mesh_raycast_bwd(const float* origins, const float* directions, const float* vertices, const int32_t* faces,
                         const int32_t* face, const float* ddepth, int B, int R, int V, int F,
                         float* dorigins, float* ddirections, float* dvertices, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_RAYCAST_H */
