/* libicn: optimal matching of two point clouds of ONE size by a synchronous (Jacobi) epsilon-scaling auction -- the assignment that
 * the earth mover's distance is the mean cost of, for every pair of clouds of two sets or for pair (b, b) only: the second half of the
 * evaluation tables that report chamfer and EMD side by side (geniconet_amd/metrics.py: optimal_matching, pairwise_emd,
 * earth_movers_distance, generation_metrics(distance='emd')).
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS and _lib.LATER_HEADERS are each held to a fixed set of
 * prototypes (tests/test_abi*.py); these entries are exported from the same libicn.so under the same conventions: plain device
 * pointers and ints, the caller owns every buffer, the library allocates nothing and never synchronises, an int entry returns 0 on
 * success and a negative value with icn_last_error() otherwise, and arguments are checked before any device call (null pointers,
 * then sizes, then the workspace).  The ABI version of icn.h stays 9: nothing of icn.h changed.
 * The ctypes binding of these entries is _lib.MATCH_HEADERS (checked against this header by tests/test_abi_match.py).
 *
 * One definition, restated in torch by metrics._torch_optimal_matching.  queries (G, N, 3) fp32 are the persons of a pair, targets
 * (R, N, 3) fp32 its objects.
 *   Cost.   d_ij is the d_j of include/icn_nn.h: fp32, no fused multiply-add, (dx dx + dy dy) + dz dz;  c_ij = sqrtf(d_ij), correctly
 *           rounded fp32.  Everything after this is double.
 *   Scale.  lo, hi: the joint bounding box of both clouds (fp32 min and max);  e = (double)hi - (double)lo;
 *           D = sqrt((e.x e.x + e.y e.y) + e.z e.z).
 *   Cases decided before any loop:
 *           a coordinate of either cloud, or D, is not finite   match all -1,  cost NaN,   rounds 0,  prices NaN
 *           D == 0 (every point coincides)                      match identity, cost 0,    rounds 0,  prices 0
 *           N == 1                                              match [0],     cost c_00,  rounds 0,  prices 0
 *   Phases  k = 1 ... phases with eps_k = D 4^-k (exact).  Prices start at 0 and carry over; every phase starts with all persons
 *           unassigned and all objects unowned.
 *   One round of a phase.  U = the unassigned persons.  U empty: the phase ends.  rounds == max_rounds: the auction stops.  Else
 *           rounds += 1 and, for each i in U, against the prices as they stand at the start of the round:
 *               v_ij = (-c_ij) - price_j;   j1 = argmax_j v_ij, the lowest j among equals;   v2 = max over j != j1 of v_ij
 *               bid_i = ((v_ij1 - v2) + eps_k) + price_j1
 *           then for each object that received bids: the highest bid wins, the lowest i among equals; price_j = that bid; the
 *           previous owner, if any, becomes unassigned; the winner owns j.
 *   Round cap.  When the cap stops the auction, match holds -1 for the unassigned persons, cost is NaN and rounds == max_rounds: no
 *           partial sum ever looks like a result.
 *   Result. match[i] = the object person i owns;  cost = sum_i c_{i, match[i]} in double;  rounds = the total over all phases;
 *           prices = the final price vector.
 * Max, the argmax with the lowest index and the second maximum do not depend on the order of evaluation: match, rounds and prices
 * are fixed bit for bit.  The cost is summed in an order that N alone fixes (thread t of 1024 its persons t, t + 1024, ... in
 * ascending order, a fixed tree over the workgroup); against the same terms in any other order |difference| <= N 2^-53 cost.
 * The cost is within N eps_phases of the optimal assignment's, so the mean cost cost / N -- the earth mover's distance -- is within
 * D 4^-phases of the optimum; epsilon-complementary slackness of (match, prices) certifies that from the outputs alone.
 * Clouds whose coordinates are finite but so far apart that a squared distance overflows fp32 are outside the definition: such a
 * call reads and writes nothing out of bounds and ends at the round cap at the latest.
 *
 * icn_match_clouds: one launch on `stream`, ONE WORKGROUP A PAIR from start to finish (grid (R, G), or (1, G) when paired): no
 * workgroup waits for another, nothing spins on memory, the launch is an ordinary one, and it ends in bounded time on any input: the
 * round loop is bounded by max_rounds, the walk over U by N, and the early cases leave before any loop.  Prices and owners of the N
 * objects sit in the workgroup's shared memory, 12 N bytes, hence N <= 13312 (which admits the 10 242 vertices of an I5 grid); the
 * targets are read from global memory.  No floating-point atomics; bit-identical run to run.
 *   paired == 0: every pair.  cost and rounds are (G, R), match and prices (G, R, N).
 *   paired == 1: requires G == R and handles pair (b, b) only.  cost and rounds are (G,), match and prices (G, N).
 * match and prices may each be null and are then not written; cost and rounds are required.
 * Entry (g, r) of a G x R call equals the 1 x 1 call and the paired call on those two clouds bit for bit, in all four outputs.
 * ws holds icn_match_clouds_workspace_bytes(G, R, N, paired) = pairs * 16 * ceil(3 N / 2) bytes, pairs = G if paired else G * R (0 for
 * sizes the call rejects), 16-byte aligned; a smaller, null or misaligned workspace fails before any device call.  Host-only query.
 * 1 <= G, R <= 65535 (grid dimensions), 1 <= N <= 13312, paired 0 or 1 and G == R when 1, 1 <= phases <= 26, 1 <= max_rounds
 * (anything else fails as `bad sizes`). */
#ifndef ICN_MATCH_H
#define ICN_MATCH_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t icn_match_clouds_workspace_bytes(int G, int R, int N, int paired);

/* match int32 and prices float64 (pairs, N), each may be null; cost float64 and rounds int32 (pairs,). */
int icn_match_clouds(const float* queries, const float* targets, int G, int R, int N, int paired, int phases, int max_rounds,
                     int* match, double* prices, double* cost, int* rounds, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_MATCH_H */
