/* libicn: the tail of the decoder as one operator,
 *     y = tanh(W relu(bn_a(a) + bn_b(b)) + bias)
 * training-mode BatchNorms over channels-last rows a, b (M, C) fp32, W (Cout, C), Cout <= 4 (geniconet_amd/fused.py:
 * bn_add_relu_head).  It computes what icn_bn_relu_fwd + icn_head_fwd and icn_head_bwd + icn_bn_relu_bwd of icn.h compute, without
 * the two (M, C) tensors those write only to read them back: the ReLU output x between BatchNorm and head, and the head's input
 * gradient dx between the two backward operators.  Both are recomputed in registers from a, b, dy and y.
 *
 * include/icn.h and the extension headers bound by _lib.EXTENSION_HEADERS, _lib.LATER_HEADERS and _lib.MATCH_HEADERS are each held
 * to a fixed set of prototypes (tests/test_abi*.py); these entries are exported from the same libicn.so under the same conventions:
 * plain device pointers and ints, the caller owns every buffer, the library allocates nothing and never synchronises, every launch
 * goes to `stream` in call order, an int entry returns 0 on success and a negative value with icn_last_error() otherwise, and
 * arguments are checked before any device call (null pointers, then sizes, then the workspace).  The ABI version of icn.h stays 9:
 * nothing of icn.h changed.  The ctypes binding of these entries is _lib.FUSED_HEADERS (checked against this header by
 * tests/test_abi_fused.py).
 *
 * Sizes: M >= 1 rows; C in {16, 32, 64, 128, 256} (C / 4 lanes share a row); 1 <= Cout <= 4; anything else fails as `bad sizes`.
 * stat_a, stat_b (2 C) are [mean | 1 / sqrt(var + eps)] as icn_bn_stats2 of icn.h leaves them: the statistics pass is that entry,
 * unchanged, and runs before icn_bn_head_fwd on the same stream.  gamma / beta (C) are the BatchNorms' weight and bias.
 *
 * icn_bn_head_fwd: one launch.  Reads a, b (M, C), writes y (M, Cout); nothing of M x C is written.
 * icn_bn_head_bwd: four launches.  dy, y (M, Cout) are the upstream gradient and the forward's output.
 *   1. one pass over a, b, dy, y: g3 = dy (1 - y^2), x = relu(v) and the mask v > 0 from the recomputed pre-activation v,
 *      g = (W^T g3) (v > 0); chunk partials of dW = sum g3 (x) x and dbias = sum g3 in the type and the order of icn_head_bwd (fp32
 *      from 1024 rows on, double below; one workgroup per chunk of ceil(M / chunks) rows, a thread every (1024 / C)-th row in ascending
 *      order), and of sum g, sum g ahat, sum g bhat (the BatchNorm sums) in double from the first add;
 *   2. the BatchNorm backward's finalize of icn_bn_relu_bwd: sums (3 C) = [sum g | sum g ahat | sum g bhat], also written to dbeta_a,
 *      dbeta_b (both sum g), dgamma_a, dgamma_b (C each; each may be null and is then not written);
 *   3. the head's reduce of icn_head_bwd over the chunks in double: dw (Cout, C), dbias (Cout);
 *   4. one pass over a, b, dy, y again: da, db (M, C) = gamma invstd (g - sum g / M - xhat sum g xhat / M), as icn_bn_relu_bwd.
 * The pre-activation v and g3 come from one device function each in all three kernels (and v from the one the unfused kernels use),
 * so the mask and g of the backward passes are the forward's and each other's, bit for bit.  y, da, db, dw and dbias are the bits the
 * unfused entries give on the same inputs; the BatchNorm sums are the same doubles grouped by other chunks before their one rounding
 * to fp32.  Fixed summation order, no atomics: bit-identical run to run.
 * ws holds icn_bn_head_workspace_bytes(M, C, Cout) = chunks (3 C + 4 (C + 4)) 8 bytes, chunks = min(1024, ceil(M / 64)) (0 for sizes the
 * calls reject), 16-byte aligned; a smaller, null or misaligned workspace fails before any device call.  Host-only query.
 * No buffer may alias another; a, b, dy, y, the statistics and the parameters are only read. */
#ifndef ICN_FUSED_H
#define ICN_FUSED_H

#include "icn.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t icn_bn_head_workspace_bytes(int M, int C, int Cout);

int icn_bn_head_fwd(const float* a, const float* b, const float* stat_a, const float* stat_b, const float* gamma_a, const float* beta_a,
                    const float* gamma_b, const float* beta_b, const float* w, const float* bias, float* y, int M, int C, int Cout,
                    void* stream);

int icn_bn_head_bwd(const float* dy, const float* y, const float* a, const float* b, const float* stat_a, const float* stat_b,
                    const float* gamma_a, const float* beta_a, const float* gamma_b, const float* beta_b, const float* w, float* da,
                    float* db, float* sums, float* dw, float* dbias, float* dbeta_a, float* dgamma_a, float* dbeta_b, float* dgamma_b,
                    int M, int C, int Cout, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICN_FUSED_H */
