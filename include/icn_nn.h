/* libicn: nearest-neighbour search between batched point sets -- for every point of one set its nearest point in the other set and
 * which point that is -- and the backward of that distance.  What chamfer distance, F-score and the point-set Hausdorff distance
 * are built on (geniconet_amd/metrics.py).
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS and _lib.LATER_HEADERS are each held to a fixed set of
 * prototypes (tests/test_abi*.py); these entries are exported from the same libicn.so under the same conventions: plain device
 * pointers and ints, the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on
 * success and a negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers,
 * then sizes).  The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.UNPINNED_HEADERS (checked against this header by tests/test_abi_nn.py).
 *
 * One definition.  points (B, N, 3) fp32, targets (B, M, 3) fp32; N and M are independent.  ALL ARITHMETIC IS fp32 on the values as
 * stored, every product and sum rounded on its own (no fused multiply-add), in exactly the order written.  For query p and target q_j:
 *       dx = p.x - q_j.x;  dy = p.y - q_j.y;  dz = p.z - q_j.z
 *       d_j = (dx * dx + dy * dy) + dz * dz
 *   best = +inf, idx = -1; for j = 0 ... M - 1 in ascending order: if d_j < best then best = d_j, idx = j.
 *   dist = best (the SQUARED distance, fp32), idx int32.  Among equal distances the lowest index wins.
 * There are no special cases beyond that rule: a NaN anywhere makes d_j NaN, which is never <, so that target is passed over; an
 * infinite coordinate, or a d_j that overflows, gives +inf, which is not < +inf; a query with no acceptable target answers
 * (+inf, -1).  A NaN never comes out, and nothing is read out of bounds whatever the values are.  A CPU fp32 formulation written with
 * separate multiplies and adds reproduces these bits exactly (metrics._torch_sided_distance; tests/test_nearest_points.py).  Against
 * float64 on the same stored values |d32 - d64| <= 6 * 2^-24 * d64 while nothing underflows: five roundings on a sum of non-negative
 * terms.
 *
 * icn_nearest_points: one launch on `stream`; the batch index is gridDim.y.  The targets of a cloud pass through shared memory in
 * tiles, in ascending order, so the tie rule costs nothing; every thread holds a few queries in registers.  No atomics, every output
 * written exactly once ((+inf, -1) rows too), bit-identical run to run.  No workspace, no synchronisation.
 *
 * icn_nearest_points_bwd: the gradient of dist at a FIXED choice idx, from the forward's `idx` and the upstream ddist = g (B, N), in
 * fp32 without contraction:
 *       e = p - q_idx   (component-wise, rounded);   s = 2 * g   (exact);   dpoints = s * e;   dtargets[idx] += -(s * e)
 * A row whose idx is outside [0, M), or whose e or g is not finite, gives an exact-zero dpoints row and contributes nothing; nothing
 * is read out of bounds whatever `idx` holds.  dtargets goes through one record per query (id = (idx, -1, -1), g = -(s e), w0 = 1) and
 * is then summed per target in a fixed order with no atomics: bit-identical run to run, and a target that is nobody's neighbour gets
 * an exact 0.  Both gradient pointers are optional: one that is given is written whole; with both null nothing is launched and the
 * call returns 0.  ws -- only looked at when dtargets is given -- holds icn_nearest_points_bwd_workspace_bytes(B, N, M) =
 * 40 * B * N bytes (0 for sizes the call rejects), 16-byte aligned.  One launch, and a second when dtargets is given.
 * 1 <= B <= 65535 (the batch index is gridDim.y), 1 <= N, M <= 0x7fffffff / 3 (anything else fails as `bad sizes`). */
#ifndef ICN_NN_H
#define ICN_NN_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dist (B, N) fp32 squared, idx (B, N) int32 (-1: no acceptable target) of points against the targets of cloud b. */
int icn_nearest_points(const float* points, const float* targets, int B, int N, int M, float* dist, int32_t* idx, void* stream);

size_t icn_nearest_points_bwd_workspace_bytes(int B, int N, int M);

/* dpoints (B, N, 3) and dtargets (B, M, 3): each may be null. */
int icn_nearest_points_bwd(const float* points, const float* targets, const int32_t* idx, const float* ddist, int B, int N, int M,
                           float* dpoints, float* dtargets, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_NN_H */
