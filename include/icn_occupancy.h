/* libicn: occupancy histograms of point clouds on a cubic lattice, and the Jensen-Shannon divergence of two such histograms -- the
 * first column of the shape-generation tables (JSD beside MMD, COV and 1-NNA; Achlioptas et al. 2018), the one figure of the four that
 * is a property of a whole SET of shapes: every point of every cloud of a set is dropped into a lattice (28^3 in the papers), and
 * the two normalised histograms are compared (geniconet_amd/metrics.py: occupancy_counts, occupancy_jsd, jensen_shannon_divergence,
 * the `jsd=` option of generation_metrics and generation.evaluate_generation).
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS, _lib.LATER_HEADERS, _lib.MATCH_HEADERS, _lib.FUSED_HEADERS
 * and _lib.SUBSET_HEADERS are each held to a fixed set of prototypes (tests/test_abi*.py); these entries are exported from the same
 * libicn.so under the same conventions: plain device pointers and ints, the caller owns every buffer, the library allocates nothing
 * and never synchronises, an int entry returns 0 on success and a negative value with icn_last_error() otherwise, and arguments are
 * checked before any device call (null pointers, then sizes).  The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.OCCUPANCY_HEADERS (checked against this header by tests/test_abi_occupancy.py).
 *
 * One definition, restated in torch by metrics._torch_occupancy_counts and metrics._torch_occupancy_jsd.
 *
 * THE HISTOGRAM.  The lattice has R lattice points per axis, 1 <= R <= 32, and is given by two fp32 numbers, lo and inv_spacing (the
 * caller computes inv_spacing, so that both sides use the same bits; for lattice points from lo to hi it is (R - 1) / (hi - lo)).
 * For a point (x, y, z) of points (B, N, 3) fp32:
 *   Dropped.  A point with any coordinate not finite is counted in no cell; it is counted in `dropped` instead.
 *   Cell index per axis, in fp32, every operation rounded on its own (no fused multiply-add):
 *               t = (x - lo) * inv_spacing
 *               u = floorf(t + 0.5f)
 *               i = (int) fminf(fmaxf(u, 0), R - 1)
 *           the nearest lattice point; a tie goes up; anything outside is clamped onto the boundary lattice point, a finite x
 *           whose t overflows to +-inf included.  With finite x, lo and inv_spacing > 0 no NaN can arise.
 *   Linear cell.  c = (ix R + iy) R + iz.
 *   Counts.   per_cloud == 0: counts[c] = the number of points of the whole set in cell c, int32 (R, R, R); dropped one int32.
 *             per_cloud != 0: counts[b, c], one histogram a cloud, int32 (B, R, R, R); dropped int32 (B,).
 * Integer counts do not depend on the order of evaluation, so both forms are fixed BIT FOR BIT however the work is split: row b of a
 * per-cloud call equals the B = 1 call on that cloud, the set histogram equals the sum of the per-cloud rows, and in both forms the
 * counts and the dropped points add up to the points given.  B N <= 2^31 - 1, so no count overflows.
 *
 * THE DIVERGENCE of two count vectors a, b of R^3 non-negative int32, ALL IN DOUBLE, with the totals A = sum a and B = sum b taken
 * as integers (64-bit, exact).  Per cell, in ascending c:
 *               p = a_c / A,  q = b_c / B
 *               m = 0.5 (p + q)
 *               tp = p log2(p / m) if a_c > 0, else 0;   tq = q log2(q / m) if b_c > 0, else 0
 *               s_c = 0.5 (tp + tq)
 *           jsd = sum_c s_c, base 2, in [0, 1].  A == 0 or B == 0 answers NaN.
 * Every product, quotient and sum is rounded on its own.  The order of the sum is fixed by R alone: thread k of the one workgroup of
 * T = 256 threads adds the s_c of cells k, k + T, k + 2 T, ... in ascending order, starting from 0; then a fixed tree over the
 * threads, x_k += x_(k + h) for h = 128, 64, ..., 1.  The answer is therefore bit-identical run to run, and:
 *   identical inputs give exactly 0.0 (p == q, so m == p, p / m == 1 and log2(1) == 0);
 *   swapping a and b gives the same bits (p + q and tp + tq commute);
 *   against the same summands in any other order |difference| <= (R^3 / T + log2 T) 2^-53 * 2, and every summand carries about ten
 *           roundings of relative size 2^-53 on terms bounded by p + q: within 2^-44 of a float64 evaluation in any order.
 *
 * icn_point_occupancy: k_point_occupancy, then k_occupancy_reduce when a histogram was split, on `stream`.  Every workgroup owns a
 * private histogram of R^3 32-bit words in shared memory (128 KiB at R = 32), zeroes it, streams its share of the points, adds with
 * integer shared-memory atomics and writes its whole histogram once -- to counts itself where a histogram has one workgroup, else to
 * its slice of the workspace, which the second launch sums.  No global atomics, no memset, no workgroup waits for another, every
 * loop is bounded by the sizes; every output word is written exactly once.  The set form takes one workgroup per 16 384 points, at
 * most 256 (one a compute unit); the per-cloud form as many a cloud, as long as the grid stays within 256 workgroups, and at least one.
 * `dropped` may be null and is then not written.  `workspace` holds icn_point_occupancy_workspace_bytes(B, N, R, per_cloud) bytes (0
 * for sizes the call rejects, never 0 otherwise; a host-only query), 16-byte aligned, and needs no initialisation.
 * 1 <= B <= 65535, 1 <= N, B N <= 2^31 - 1, 1 <= R <= 32, lo and inv_spacing finite, inv_spacing > 0, workspace_bytes at least the
 * query's answer (anything else fails as `bad sizes`).
 *
 * icn_occupancy_jsd: one launch of one workgroup (k_occupancy_jsd) on `stream`: the totals by an integer reduction, then the sum above;
 * writes one double to jsd (device memory).  counts_a and counts_b hold R^3 int32 each, 1 <= R <= 32 (else `bad sizes`); negative
 * counts are outside the definition (nothing is read or written out of bounds). */
#ifndef ICN_OCCUPANCY_H
#define ICN_OCCUPANCY_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t icn_point_occupancy_workspace_bytes(int B, int N, int R, int per_cloud);

/* counts int32 (R, R, R) or, per cloud, (B, R, R, R); dropped int32, 1 or B words, may be null. */
int icn_point_occupancy(const float* points, int B, int N, int R, float lo, float inv_spacing, int per_cloud,
                        int32_t* counts, int32_t* dropped, void* workspace, size_t workspace_bytes, void* stream);

int icn_occupancy_jsd(const int32_t* counts_a, const int32_t* counts_b, int R, double* jsd, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_OCCUPANCY_H */
