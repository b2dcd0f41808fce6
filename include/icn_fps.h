/* libicn: farthest point sampling of point clouds -- a fixed number of well-spread points of every cloud of a batch, the subsets that
 * the shape-generation tables (MMD / COV / 1-NNA on 2 048 points a shape) match instead of whole clouds
 * (geniconet_amd/sampling.py: farthest_point_sample, farthest_points; the `points=` option of metrics.generation_metrics,
 * metrics.evaluate_distance and generation.evaluate_generation).
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS, _lib.LATER_HEADERS, _lib.MATCH_HEADERS and
 * _lib.FUSED_HEADERS are each held to a fixed set of prototypes (tests/test_abi*.py); this entry is exported from the same libicn.so
 * under the same conventions: plain device pointers and ints, the caller owns every buffer, the library allocates nothing and never
 * synchronises, an int entry returns 0 on success and a negative value with icn_last_error() otherwise, and arguments are checked
 * before any device call (null pointers, then sizes).  The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of this entry is _lib.SUBSET_HEADERS (checked against this header by tests/test_abi_fps.py).
 *
 * One definition, restated in torch by sampling._torch_farthest_point_sample.  For each cloud b of points (B, N, 3) fp32:
 *   Distance.  d(i, c) is the d_j of include/icn_nn.h: dx = p_i.x - p_c.x, dy and dz likewise, d = (dx dx + dy dy) + dz dz in fp32,
 *           every product and sum rounded on its own (no fused multiply-add).  d is symmetric in (i, c) bit for bit.
 *   Case decided before any loop:
 *           a coordinate of the cloud is not finite             idx[b, :] = -1,  cover[b, :] = NaN
 *           (the other clouds of the batch are unaffected)
 *   Loop.   dist_i = +inf for all i, cur = start.  For s = 0 ... S - 1:
 *               idx[b, s] = cur
 *               dist_i = fminf(dist_i, d(i, cur)) for every i
 *               cover[b, s] = max_i dist_i
 *               cur = the LOWEST i with dist_i == cover[b, s]
 * fminf, the max and the argmax with the lowest index do not depend on the order of evaluation: idx and cover are fixed BIT FOR BIT
 * however the scan is split.  With finite coordinates no NaN can arise: d is a sum of squares, an overflowing d is +inf, dist is never
 * negative and never -0, so the bit pattern of dist orders like an unsigned integer.
 * What follows, exactly, in fp32:
 *   cover[b, .] is non-increasing;
 *   cover[b, S - 1] is the maximum over i of the squared distance of point i to its nearest selected point, bit for bit what
 *           icn_nearest_points answers for (points, points[idx]);
 *   for S >= 2 the smallest d between two selected points is cover[b, S - 2];
 *   S == N with distinct points selects a permutation, and cover[b, N - 1] == 0;
 *   once the distinct points are used up cover is 0 and idx repeats the lowest index of the cloud, 0: duplicates are defined, not
 *           an error.
 *
 * icn_farthest_points: one launch on `stream`, ONE WORKGROUP A CLOUD from start to finish (grid (B)): no workgroup waits for another,
 * nothing spins on memory, no atomics, the launch is an ordinary one and its only loop is s < S.  Every thread holds its points and
 * their dist in registers, a compile-time number of points per thread picked by N, hence N <= 13312 (which admits the 10 242 vertices
 * of an I5 grid); one barrier a step.  Bit-identical run to run; row b of a batch equals the B = 1 call on that cloud.
 * idx int32 (B, S) is required; cover fp32 (B, S) may be null and is then not written.  No workspace.
 * 1 <= B <= 65535, 1 <= N <= 13312, 1 <= S <= N, 0 <= start < N (anything else fails as `bad sizes`). */
#ifndef ICN_FPS_H
#define ICN_FPS_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

int icn_farthest_points(const float* points, int B, int N, int S, int start, int* idx, float* cover, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_FPS_H */
