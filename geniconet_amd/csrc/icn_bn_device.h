// Device helpers shared by the BatchNorm / head kernels of icn_bn.hip and the fused decoder tail of icn_fused.hip.
// Every kernel that needs the pre-activation of the fused BatchNorm (+ residual) + ReLU, the tanh derivative of the head or the
// BatchNorm input gradient goes through the ONE function below, so that a value recomputed in another kernel -- or in another
// file -- is the value the first kernel had, bit for bit (the ReLU mask of a backward pass is the forward's).
#pragma once
#include <hip/hip_runtime.h>

namespace icn {

using f32x4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f32x4 ldv(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void stv(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)}; }

// Sums of the BatchNorm passes are accumulated in DOUBLE from the first add (round 3), as the CPU reference does (torch's
// acc_type<float> on the CPU is double; its device kernels sum in fp32).  A batch statistic enters every element of its channel,
// so its rounding error is a COHERENT perturbation of the tensor, unlike the element-wise rounding of the convolutions, and the
// next cancelling sum (a BatchNorm backward's sum g, sum g * xhat, where |sum g| is 10 - 400 x smaller than sum |g| in this
// network) amplifies exactly that kind of error.  The kernels are HBM-bound: the fp64 adds cost nothing measurable (same
// throughput in the bench).  (What this does NOT remove: gradients of this network are discontinuous at ReLU pre-activations
// within rounding of zero; see tests/test_gpu_training_parity.py for how the parity tests deal with that.)
using f64x4 = __attribute__((ext_vector_type(4))) double;
__device__ __forceinline__ f64x4 to_d(f32x4 v) { return f64x4{(double)v[0], (double)v[1], (double)v[2], (double)v[3]}; }

// pre-activation of the fused op for 4 channels: bn_a(a) [+ bn_b(b)]; scale = invstd * gamma.  Forward and both backward
// passes go through this one function, so the ReLU mask the backward recomputes is bit-identical to the forward's.
template <int DUAL>
__device__ __forceinline__ f32x4 bn_pre4(f32x4 a, f32x4 mean_a, f32x4 scale_a, f32x4 beta_a, f32x4 b, f32x4 mean_b, f32x4 scale_b,
                                         f32x4 beta_b) {
    f32x4 v = (a - mean_a) * scale_a + beta_a;
    if (DUAL) v += (b - mean_b) * scale_b + beta_b;
    return v;
}

// g = dy * (v > 0): the upstream gradient behind the ReLU, from the recomputed pre-activation
__device__ __forceinline__ f32x4 relu_mask4(f32x4 v, f32x4 dy) {
    f32x4 g;
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = v[j] > 0.f ? dy[j] : 0.f;
    return g;
}

// input gradient of a training-mode BatchNorm for 4 channels: gamma * invstd * (g - sum_g / M - xhat * sum_gx / M), with the roundings
// of k_bn_relu_bwd spelled out -- g - sum_g * inv_m as one fused multiply-add, sum_gx * inv_m rounded, then a second fused
// multiply-add: a caller whose sums are loop constants must not depend on where the compiler happens to contract
__device__ __forceinline__ f32x4 bn_dx4(f32x4 g, f32x4 x, f32x4 mean, f32x4 inv, f32x4 gamma, f32x4 sum_g, f32x4 sum_gx, float inv_m) {
    const f32x4 xh = (x - mean) * inv, scale = gamma * inv;
    f32x4 d;
#pragma unroll
    for (int j = 0; j < 4; ++j) d[j] = scale[j] * __builtin_fmaf(-xh[j], sum_gx[j] * inv_m, __builtin_fmaf(-sum_g[j], inv_m, g[j]));
    return d;
}

// The type the head's backward sums dW and dbias in up to the chunk partials (and computes g3 in): see HEAD_F64_ROWS in icn_bn.hip.
template <typename ACC> struct HeadAcc;
template <> struct HeadAcc<float> { using v4 = f32x4; static __device__ __forceinline__ v4 of(f32x4 v) { return v; } };
template <> struct HeadAcc<double> { using v4 = f64x4; static __device__ __forceinline__ v4 of(f32x4 v) { return to_d(v); } };

__device__ __forceinline__ float fma_acc(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_acc(double a, double b, double c) { return __builtin_fma(a, b, c); }

// tanh derivative of the head in ACC with the roundings k_head_bwd's code has, spelled out: f = 1 - y^2 as one fused multiply-add,
// g3 = dy * f rounded (what dx and dW use), and the dbias sum takes dy * f inside its own fused multiply-add (head_dbias_add).  The
// fused tail's two backward passes both recompute g3 here, and both round it to fp32 for the input gradient as k_head_bwd does.
template <typename ACC> struct HeadG3 { ACC dy, f, g3; };
template <typename ACC>
__device__ __forceinline__ HeadG3<ACC> head_g3(float dy, float y) {
    HeadG3<ACC> t;
    const ACC yy = y;
    t.dy = dy;
    t.f = fma_acc(-yy, yy, (ACC)1);
    t.g3 = t.dy * t.f;
    return t;
}
template <typename ACC>
__device__ __forceinline__ ACC head_dbias_add(ACC sum, const HeadG3<ACC>& t) { return fma_acc(t.dy, t.f, sum); }

constexpr int HEAD_MAX_OUT = 4;

// the head's input gradient for 4 channels, dx = sum_o g3[o] * W[o], outputs in ascending order (k_head_bwd's order)
__device__ __forceinline__ f32x4 head_dx4(const float* g3, const f32x4* wv, int Cout) {
    f32x4 dx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int o = 0; o < HEAD_MAX_OUT; ++o)
        if (o < Cout) dx += g3[o] * wv[o];
    return dx;
}

}  // namespace icn
