// Fused tail of the decoder, training mode, channels-last rows (M = B*P, C):
//     y = tanh(W relu(bn_a(a) + bn_b(b)) + bias),   W (Cout, C), Cout <= 4
// (reference models.py:58-62 followed by 151-154).  The unfused operators of icn_bn.hip write the ReLU output x (M, C) only for the
// head to read it back, and the head's backward writes dx (M, C) only for the BatchNorm backward to read it twice.  Here x and dx
// live in registers: the forward reads a, b and writes y (M, Cout); the backward reads a, b, dy, y twice -- once for every sum
// (the three BatchNorm sums, the head's dW and dbias), once for da, db -- and recomputes x and dx = W^T g3 from them.
// The pre-activation comes from bn_pre4 and g3 = dy (1 - y^2) from head_g3 in all three kernels (icn_bn_device.h), so the ReLU mask
// and dx of the backward are the forward's and each other's, bit for bit.  Every output is the unfused operators' on the same inputs,
// bit for bit: the same expressions with the same roundings, the head's sums in k_head_bwd's type and order, the BatchNorm sums in
// double from the first add; chunk partials, then the second stages of the unfused operators (k_bn_finalize_bwd, k_head_reduce):
// two deterministic stages, fixed order.
// C / 4 lanes share a row (one 16-byte load of a and of b each, coalesced), as in k_head_fwd.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "icn_bn_device.h"
#include "icn_launch.h"

namespace icn {

// per-thread constants of the 4 channels a lane owns: [mean | invstd] of both BatchNorms, scale = invstd * gamma, beta
struct TailBn {
    f32x4 mean_a, inv_a, gam_a, be_a, mean_b, inv_b, gam_b, be_b;
    __device__ __forceinline__ TailBn(const float* stat_a, const float* stat_b, const float* ga, const float* ba, const float* gb,
                                      const float* bb, int C, int c)
        : mean_a(ldv(stat_a + c)), inv_a(ldv(stat_a + C + c)), gam_a(ldv(ga + c)), be_a(ldv(ba + c)), mean_b(ldv(stat_b + c)),
          inv_b(ldv(stat_b + C + c)), gam_b(ldv(gb + c)), be_b(ldv(bb + c)) {}
    __device__ __forceinline__ f32x4 pre(f32x4 a, f32x4 b) const {
        return bn_pre4<1>(a, mean_a, inv_a * gam_a, be_a, b, mean_b, inv_b * gam_b, be_b);
    }
};

// rows per thread and iteration, every load of an iteration issued before the first use (as the passes of icn_bn.hip do)
constexpr int TAIL_UN_FWD = 4, TAIL_UN_SUMS = 2, TAIL_UN_APPLY = 2;

template <int LPR>   // lanes per row = C / 4 (power of two, <= 64)
__global__ __launch_bounds__(256) void k_bn_head_fwd(const float* __restrict__ a, const float* __restrict__ b,
                                                      const float* __restrict__ stat_a, const float* __restrict__ stat_b,
                                                      const float* __restrict__ ga, const float* __restrict__ ba,
                                                      const float* __restrict__ gb, const float* __restrict__ bb,
                                                      const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ y, int M, int Cout) {
    constexpr int C = LPR * 4, RPB = 256 / LPR, UN = TAIL_UN_FWD;
    const int sub = threadIdx.x % LPR, rloc = threadIdx.x / LPR;
    const TailBn bn(stat_a, stat_b, ga, ba, gb, bb, C, 4 * sub);
    f32x4 wv[HEAD_MAX_OUT];
#pragma unroll
    for (int o = 0; o < HEAD_MAX_OUT; ++o) wv[o] = o < Cout ? ldv(w + o * C + 4 * sub) : f32x4{0.f, 0.f, 0.f, 0.f};
    const float bs = sub < Cout ? bias[sub] : 0.f;
    for (long r = (long)blockIdx.x * (RPB * UN) + rloc; r < M; r += (long)gridDim.x * (RPB * UN)) {
        f32x4 av[UN], bv[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const size_t o = (size_t)min(r + u * RPB, (long)M - 1) * C + 4 * sub;      // (clamped: loaded and computed, not stored)
            av[u] = ldv(a + o);
            bv[u] = ldv(b + o);
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const f32x4 xv = relu4(bn.pre(av[u], bv[u]));
            float acc[HEAD_MAX_OUT];
#pragma unroll
            for (int o = 0; o < HEAD_MAX_OUT; ++o) acc[o] = xv[0] * wv[o][0] + xv[1] * wv[o][1] + xv[2] * wv[o][2] + xv[3] * wv[o][3];
#pragma unroll
            for (int d = LPR / 2; d >= 1; d >>= 1)
#pragma unroll
                for (int o = 0; o < HEAD_MAX_OUT; ++o) acc[o] += __shfl_xor(acc[o], d, 64);
            float v = acc[0];
#pragma unroll
            for (int o = 1; o < HEAD_MAX_OUT; ++o) v = sub == o ? acc[o] : v;
            const long ru = r + u * RPB;
            if (ru < M && sub < Cout) y[(size_t)ru * Cout + sub] = tanhf(v + bs);
        }
    }
}

// what both backward passes recompute of one row for the 4 channels of a lane: the ReLU output x, the gradient g behind the ReLU
// (the head's dx under the forward's mask) and g3 in the head's sum type ACC (float from HEAD_F64_ROWS rows on, double below)
template <typename ACC> struct TailRow { f32x4 x, g; HeadG3<ACC> g3[HEAD_MAX_OUT]; };
template <typename ACC>
__device__ __forceinline__ TailRow<ACC> tail_row(const TailBn& bn, f32x4 av, f32x4 bv, const float* dyv, const float* yv,
                                                 const f32x4* wv, int Cout) {
    TailRow<ACC> t;
    float g3f[HEAD_MAX_OUT];
#pragma unroll
    for (int o = 0; o < HEAD_MAX_OUT; ++o) {
        t.g3[o] = head_g3<ACC>(dyv[o], yv[o]);                                          // (o >= Cout: dy = 0, unused)
        g3f[o] = (float)t.g3[o].g3;
    }
    const f32x4 v = bn.pre(av, bv);
    t.x = relu4(v);
    t.g = relu_mask4(v, head_dx4(g3f, wv, Cout));
    return t;
}

// One workgroup per chunk of the HEAD's backward (head_chunks(M) chunks, as k_head_bwd), a thread every (256 / LPR)-th row of it in
// ascending order with one accumulator per sum, the row groups combined through LDS in ascending order: dW and dbias are summed in
// the type and in the order of k_head_bwd, so the head's parameter gradients are the unfused operator's bit for bit.
//   head_part[chunk][o][C + 4] (ACC): sum g3[o] * x, and sum g3[o] at [C]                       (the layout of k_head_bwd)
//   bn_part[chunk][k][C] (double), k < 3: sum g, sum g * ahat, sum g * bhat                     (the layout of k_bn_partial<2>)
// The BatchNorm sums are double from the first add; their terms are exact in double, so another grouping of the rows than
// k_bn_partial's moves them by ~1e-13 of their value, far below the fp32 rounding k_bn_finalize_bwd ends with.
template <int LPR, typename ACC>
__global__ __launch_bounds__(256) void k_bn_head_bwd_sums(const float* __restrict__ dy, const float* __restrict__ y,
                                                           const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ stat_a, const float* __restrict__ stat_b,
                                                           const float* __restrict__ ga, const float* __restrict__ ba,
                                                           const float* __restrict__ gb, const float* __restrict__ bb,
                                                           const float* __restrict__ w, double* __restrict__ bn_part,
                                                           ACC* __restrict__ head_part, int M, int Cout, int rows_per_chunk) {
    using acc4 = typename HeadAcc<ACC>::v4;
    constexpr int C = LPR * 4, RPB = 256 / LPR, UN = TAIL_UN_SUMS;
    __shared__ f64x4 red[256];
    const int sub = threadIdx.x % LPR, rloc = threadIdx.x / LPR;
    const TailBn bn(stat_a, stat_b, ga, ba, gb, bb, C, 4 * sub);
    f32x4 wv[HEAD_MAX_OUT];
    acc4 dwv[HEAD_MAX_OUT];
    ACC dbv[HEAD_MAX_OUT];
#pragma unroll
    for (int o = 0; o < HEAD_MAX_OUT; ++o) {
        wv[o] = o < Cout ? ldv(w + o * C + 4 * sub) : f32x4{0.f, 0.f, 0.f, 0.f};
        dwv[o] = acc4{0, 0, 0, 0};
        dbv[o] = 0;
    }
    f64x4 q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int r0 = blockIdx.x * rows_per_chunk, r1 = min(M, r0 + rows_per_chunk);
    for (int r = r0 + rloc; r < r1; r += UN * RPB) {
        f32x4 av[UN], bv[UN];
        float dyv[UN][HEAD_MAX_OUT], yv[UN][HEAD_MAX_OUT];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const size_t row = (size_t)min(r + u * RPB, r1 - 1);                       // (clamped: loaded, not added)
            av[u] = ldv(a + row * C + 4 * sub);
            bv[u] = ldv(b + row * C + 4 * sub);
#pragma unroll
            for (int o = 0; o < HEAD_MAX_OUT; ++o) {
                dyv[u][o] = o < Cout ? dy[row * Cout + o] : 0.f;
                yv[u][o] = o < Cout ? y[row * Cout + o] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {                                                 // (ascending rows: k_head_bwd's order)
            if (r + u * RPB >= r1) continue;
            const TailRow<ACC> t = tail_row<ACC>(bn, av[u], bv[u], dyv[u], yv[u], wv, Cout);
            const acc4 xa = HeadAcc<ACC>::of(t.x);
#pragma unroll
            for (int o = 0; o < HEAD_MAX_OUT; ++o) {
                if (o < Cout) {
                    dwv[o] += t.g3[o].g3 * xa;
                    dbv[o] = head_dbias_add(dbv[o], t.g3[o]);
                }
            }
            const f64x4 gd = to_d(t.g);
            q[0] += gd;
            q[1] += gd * to_d((av[u] - bn.mean_a) * bn.inv_a);
            q[2] += gd * to_d((bv[u] - bn.mean_b) * bn.inv_b);
        }
    }
    // the row groups of the block through LDS, one quantity at a time, ascending group order (deterministic)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        __syncthreads();
        red[threadIdx.x] = q[k];
        __syncthreads();
        if (rloc == 0) {
            f64x4 t = red[sub];
#pragma unroll 4
            for (int g = 1; g < RPB; ++g) t += red[g * LPR + sub];
            *reinterpret_cast<f64x4*>(bn_part + ((size_t)blockIdx.x * 3 + k) * C + 4 * sub) = t;
        }
    }
    acc4* redw = reinterpret_cast<acc4*>(red);
    ACC* redb = reinterpret_cast<ACC*>(red);
    for (int o = 0; o < Cout; ++o) {
        __syncthreads();
        redw[threadIdx.x] = dwv[o];
        __syncthreads();
        if (rloc == 0) {
            acc4 t = redw[sub];
#pragma unroll 4
            for (int g = 1; g < RPB; ++g) t += redw[g * LPR + sub];
            *reinterpret_cast<acc4*>(head_part + ((size_t)blockIdx.x * HEAD_MAX_OUT + o) * (C + 4) + 4 * sub) = t;
        }
        __syncthreads();
        redb[threadIdx.x] = dbv[o];
        __syncthreads();
        if (threadIdx.x == 0) {
            ACC tb = 0;
            for (int g = 0; g < RPB; ++g) tb += redb[g * LPR];
            head_part[((size_t)blockIdx.x * HEAD_MAX_OUT + o) * (C + 4) + C] = tb;
        }
    }
}

// da, db as k_bn_relu_bwd<1> writes them, from the recomputed g
template <int LPR, typename ACC>
__global__ __launch_bounds__(256) void k_bn_head_bwd_apply(const float* __restrict__ dy, const float* __restrict__ y,
                                                            const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ stat_a, const float* __restrict__ stat_b,
                                                            const float* __restrict__ ga, const float* __restrict__ ba,
                                                            const float* __restrict__ gb, const float* __restrict__ bb,
                                                            const float* __restrict__ w, const float* __restrict__ sums,
                                                            float* __restrict__ da, float* __restrict__ db, int M, int Cout,
                                                            float inv_m) {
    constexpr int C = LPR * 4, RPB = 256 / LPR, UN = TAIL_UN_APPLY;
    const int sub = threadIdx.x % LPR, rloc = threadIdx.x / LPR;
    const TailBn bn(stat_a, stat_b, ga, ba, gb, bb, C, 4 * sub);
    f32x4 wv[HEAD_MAX_OUT];
#pragma unroll
    for (int o = 0; o < HEAD_MAX_OUT; ++o) wv[o] = o < Cout ? ldv(w + o * C + 4 * sub) : f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4 sg = ldv(sums + 4 * sub), sga = ldv(sums + C + 4 * sub), sgb = ldv(sums + 2 * C + 4 * sub);
    for (long r = (long)blockIdx.x * (RPB * UN) + rloc; r < M; r += (long)gridDim.x * (RPB * UN)) {
        f32x4 av[UN], bv[UN];
        float dyv[UN][HEAD_MAX_OUT], yv[UN][HEAD_MAX_OUT];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const size_t row = (size_t)min(r + u * RPB, (long)M - 1);                  // (clamped: loaded, not stored)
            av[u] = ldv(a + row * C + 4 * sub);
            bv[u] = ldv(b + row * C + 4 * sub);
#pragma unroll
            for (int o = 0; o < HEAD_MAX_OUT; ++o) {
                dyv[u][o] = o < Cout ? dy[row * Cout + o] : 0.f;
                yv[u][o] = o < Cout ? y[row * Cout + o] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const long ru = r + u * RPB;
            if (ru >= M) break;
            const TailRow<ACC> t = tail_row<ACC>(bn, av[u], bv[u], dyv[u], yv[u], wv, Cout);
            stv(da + (size_t)ru * C + 4 * sub, bn_dx4(t.g, av[u], bn.mean_a, bn.inv_a, bn.gam_a, sg, sga, inv_m));
            stv(db + (size_t)ru * C + 4 * sub, bn_dx4(t.g, bv[u], bn.mean_b, bn.inv_b, bn.gam_b, sg, sgb, inv_m));
        }
    }
}

// (the head partials take the space of doubles whichever type they have)
static size_t tail_bn_doubles(int M, int C) { return (size_t)head_chunks(M) * 3 * C; }
size_t bn_head_workspace_bytes(int M, int C) {
    return (tail_bn_doubles(M, C) + (size_t)head_chunks(M) * HEAD_MAX_OUT * (C + 4)) * sizeof(double);
}

#define ICN_TAIL_DISPATCH(KERNEL, ...)                                                  \
    switch (C) {                                                                        \
        case 16: hipLaunchKernelGGL((KERNEL<4>), __VA_ARGS__); break;                   \
        case 32: hipLaunchKernelGGL((KERNEL<8>), __VA_ARGS__); break;                   \
        case 64: hipLaunchKernelGGL((KERNEL<16>), __VA_ARGS__); break;                  \
        case 128: hipLaunchKernelGGL((KERNEL<32>), __VA_ARGS__); break;                 \
        default: hipLaunchKernelGGL((KERNEL<64>), __VA_ARGS__); break;                  \
    }
#define ICN_TAIL_DISPATCH_ACC(KERNEL, ACC, ...)                                         \
    switch (C) {                                                                        \
        case 16: hipLaunchKernelGGL((KERNEL<4, ACC>), __VA_ARGS__); break;              \
        case 32: hipLaunchKernelGGL((KERNEL<8, ACC>), __VA_ARGS__); break;              \
        case 64: hipLaunchKernelGGL((KERNEL<16, ACC>), __VA_ARGS__); break;             \
        case 128: hipLaunchKernelGGL((KERNEL<32, ACC>), __VA_ARGS__); break;            \
        default: hipLaunchKernelGGL((KERNEL<64, ACC>), __VA_ARGS__); break;             \
    }

static int tail_blocks(int M, int C, int un) {
    const int rows = 256 / (C / 4) * un;
    return std::min(4096, (M + rows - 1) / rows);
}

void launch_bn_head_fwd(const float* a, const float* b, const float* stat_a, const float* stat_b, const float* ga, const float* ba,
                        const float* gb, const float* bb, const float* w, const float* bias, float* y, int M, int C, int Cout,
                        hipStream_t s) {
    ICN_TAIL_DISPATCH(k_bn_head_fwd, dim3(tail_blocks(M, C, TAIL_UN_FWD)), dim3(256), 0, s, a, b, stat_a, stat_b, ga, ba, gb, bb, w, bias,
                      y, M, Cout)
}

template <typename ACC>
static void bn_head_bwd(const float* dy, const float* y, const float* a, const float* b, const float* stat_a, const float* stat_b,
                        const float* ga, const float* ba, const float* gb, const float* bb, const float* w, float* da, float* db,
                        float* sums, float* dw, float* dbias, float* dbeta_a, float* dgamma_a, float* dbeta_b, float* dgamma_b, void* ws,
                        int M, int C, int Cout, hipStream_t s) {
    const int chunks = head_chunks(M), rows = (M + chunks - 1) / chunks;
    double* bn_part = reinterpret_cast<double*>(ws);
    ACC* head_part = reinterpret_cast<ACC*>(bn_part + tail_bn_doubles(M, C));
    ICN_TAIL_DISPATCH_ACC(k_bn_head_bwd_sums, ACC, dim3(chunks), dim3(256), 0, s, dy, y, a, b, stat_a, stat_b, ga, ba, gb, bb, w, bn_part,
                          head_part, M, Cout, rows)
    launch_bn_finalize_bwd(bn_part, chunks, C, 3, sums, dbeta_a, dgamma_a, dbeta_b, dgamma_b, s);
    launch_head_reduce(head_part, sizeof(ACC) == sizeof(double), chunks, C, Cout, dw, dbias, s);
    ICN_TAIL_DISPATCH_ACC(k_bn_head_bwd_apply, ACC, dim3(tail_blocks(M, C, TAIL_UN_APPLY)), dim3(256), 0, s, dy, y, a, b, stat_a, stat_b,
                          ga, ba, gb, bb, w, sums, da, db, M, Cout, 1.f / M)
}

void launch_bn_head_bwd(const float* dy, const float* y, const float* a, const float* b, const float* stat_a, const float* stat_b,
                        const float* ga, const float* ba, const float* gb, const float* bb, const float* w, float* da, float* db,
                        float* sums, float* dw, float* dbias, float* dbeta_a, float* dgamma_a, float* dbeta_b, float* dgamma_b, void* ws,
                        int M, int C, int Cout, hipStream_t s) {
    if (head_sums_in_double(M))
        bn_head_bwd<double>(dy, y, a, b, stat_a, stat_b, ga, ba, gb, bb, w, da, db, sums, dw, dbias, dbeta_a, dgamma_a, dbeta_b, dgamma_b,
                            ws, M, C, Cout, s);
    else
        bn_head_bwd<float>(dy, y, a, b, stat_a, stat_b, ga, ba, gb, bb, w, da, db, sums, dw, dbias, dbeta_a, dgamma_a, dbeta_b, dgamma_b,
                           ws, M, C, Cout, s);
}
#undef ICN_TAIL_DISPATCH
#undef ICN_TAIL_DISPATCH_ACC

}  // namespace icn
