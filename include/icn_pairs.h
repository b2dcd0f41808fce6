/* libicn: directed sums of nearest squared distances for EVERY pair of clouds of two sets -- the G x R matrix that the chamfer matrix,
 * and with it the generation metrics minimum matching distance, coverage and 1-nearest-neighbour accuracy, are built on
 * (geniconet_amd/metrics.py: pairwise_sided_sums, pairwise_chamfer, generation_metrics).
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS and _lib.LATER_HEADERS are each held to a fixed set of
 * prototypes (tests/test_abi*.py); these entries are exported from the same libicn.so under the same conventions: plain device
 * pointers and ints, the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on
 * success and a negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers,
 * then sizes, then the workspace).  The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.LATER_HEADERS (checked against this header by tests/test_abi_pairs.py).
 *
 * One definition.  queries (G, N, 3) fp32, targets (R, M, 3) fp32; G, R, N and M are independent.  sums (G, R) float64:
 *       sums[g, r] = sum over the queries i of cloud g of best_i
 * best_i is exactly the `dist` of include/icn_nn.h for query i of cloud g against the targets of cloud r: ALL OF ITS ARITHMETIC IS fp32
 * on the values as stored, every product and sum rounded on its own (no fused multiply-add), in exactly the order written,
 *       dx = p.x - q_j.x;  dy = p.y - q_j.y;  dz = p.z - q_j.z
 *       d_j = (dx * dx + dy * dy) + dz * dz
 *       best = +inf; for j = 0 ... M - 1 in ascending order: if d_j < best then best = d_j
 * so a NaN d_j is passed over, +inf is never taken, and best_i = +inf where nothing is acceptable.  No index is kept.
 * The best_i are summed in double, in an order that N alone fixes: every thread its own queries in ascending order, a fixed tree
 * over the workgroup's 512 queries (one chunk), then the chunks of the pair in ascending order.  The conversion of an fp32 value to
 * double is exact and every term is >= 0: NO NaN CAN COME OUT, and a single +inf row makes sums[g, r] exactly +inf.  Against the sum of
 * the same best_i in any other order, in double, |difference| <= N 2^-53 sum.
 * sums[g, r] does not depend on G, on R or on where the two clouds sit in their sets: entry (g, r) of a G x R call equals the 1 x 1 call
 * on those two clouds bit for bit.  No atomics, every output written exactly once, bit-identical run to run.
 *
 * icn_sided_sums: two launches on `stream`.  The first indexes the pair itself (gridDim.z = G, gridDim.y = R, gridDim.x = the chunks of
 * 512 queries), passes the targets of cloud r through shared memory in tiles, in ascending order, and leaves one double per pair and
 * chunk in ws; the second adds the chunks of every pair and writes sums.  Nothing is read out of bounds whatever the values are.
 * ws holds icn_sided_sums_workspace_bytes(G, R, N, M) = 8 * G * R * ceil(N / 512) bytes (0 for sizes the call rejects; M takes no part
 * in the size), 16-byte aligned; a smaller, null or misaligned workspace fails before any device call.  Host-only query.
 * 1 <= G, R <= 65535 (grid dimensions), 1 <= N, M <= 0x7fffffff / 3 (anything else fails as `bad sizes`). */
#ifndef ICN_PAIRS_H
#define ICN_PAIRS_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t icn_sided_sums_workspace_bytes(int G, int R, int N, int M);

/* sums (G, R) float64: the queries of cloud g against the targets of cloud r, for every pair. */
int icn_sided_sums(const float* queries, const float* targets, int G, int R, int N, int M, double* sums, void* ws, size_t ws_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_PAIRS_H */
