// Area-weighted surface sampling of triangle meshes (icn_mesh_sample_fwd / icn_mesh_sample_bwd in include/icn.h): the points that
// kaolin's sample_points / pytorch3d's sample_points_from_meshes draw, from uniforms the CALLER supplies -- the kernels draw no
// random numbers, so every output is a pure function of the inputs.  vertices (B, V, 3), faces (F, 3) shared by the batch,
// u (B, S, 3).  Per mesh (blockIdx.y):
//   k_msample_area    A_f = 0.5 |(v1 - v0) x (v2 - v0)| in fp32, every product of the cross product rounded on its own (no
//                     contraction into an fma), so a face with two coincident vertices has area exactly 0 -> c[f] as a double.
//                     A face with a vertex id outside [0, V) counts as area 0.
//   k_msample_scan    inclusive scan of c in place, in double, one workgroup per mesh over tiles of 1024 in a fixed order
//                     (wave scan, wave totals, running carry): c_f = A_0 + ... + A_f, T = c_{F - 1}.  Bit-identical run to run.
//                     Neighbouring c_f are summed in different association orders.  The areas are fp32 values, so every partial sum
//                     is exact in double -- c is then non-decreasing and constant across a zero-area face, whatever the order --
//                     while the largest and the smallest non-zero area of a mesh lie within a factor 2^29 / F of each other
//                     (2^14 at F = 20 480).  Beyond that a sum may round, c_f may differ from c_{f-1} by an ulp on a zero-area face
//                     or drop by one, and "never chosen" holds only up to a probability of about 1e-16 per sample; the searches
//                     below end inside [0, F) whatever c holds.
//   k_msample_point   one thread per sample.  Uniforms outside [0, 1] are clamped, NaN counts as 0.  t = (double) u0 T; face = the
//                     smallest f with c_f > t (binary search), so a zero-area face is never chosen while T > 0; for u0 = 1 (t = T,
//                     no such f) the smallest f with c_f >= T, the last face of positive area.  T not a positive finite number:
//                     face 0.  r = sqrt(u1), weights (1 - r, r (1 - u2), r u2), point = the weighted vertices.
// Backward (to the vertices through the weights, the face choice held constant): dvertices[b, faces[face_s, k]] += w[s, k] dpoints[s].
//   k_msample_bwd_record  one thread per sample: the three vertex ids (-1 where the face or a vertex id is out of range: such a sample
//                         contributes nothing and nothing is read out of bounds), dpoints and the weights -> workspace, 40 bytes
//   k_msample_bwd_vertex  one thread per vertex: the records of its mesh go through LDS in tiles of 256 samples and every thread
//                         adds those addressed to it IN SAMPLE ORDER (then vertex 0, 1, 2 of the face) -- the scheme of
//                         k_point_to_mesh_bwd_vertex (icn_loss.hip): a fixed order, no atomics, bit-identical run to run, S * V
//                         integer compares per mesh; a vertex no sample touches gets an exact zero.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"

namespace icn {

namespace {

constexpr int SAMPLE_BLOCK = 256;
constexpr int SAMPLE_SCAN_BLOCK = 1024;

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_msample_area(const float* __restrict__ vts, const int32_t* __restrict__ faces, int V,
                                                                int F, double* __restrict__ cdf) {
    const int b = blockIdx.y, f = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    float area = 0.f;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const float* p0 = vts + ((size_t)b * V + i0) * 3;
        const float* p1 = vts + ((size_t)b * V + i1) * 3;
        const float* p2 = vts + ((size_t)b * V + i2) * 3;
        const float ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const float bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        // a x b with each product rounded on its own: a x a is exactly 0 (an fma would leave one product's rounding error)
        const float nx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
        const float ny = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
        const float nz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
        area = 0.5f * sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
    }
    cdf[(size_t)b * F + f] = (double)area;
}

// inclusive scan in place of c[0 .. F), one block per mesh, tiles of SAMPLE_SCAN_BLOCK (the scheme of k_p2m_grid_scan, in double)
__global__ __launch_bounds__(SAMPLE_SCAN_BLOCK) void k_msample_scan(double* __restrict__ cdf, int F) {
    __shared__ double wsum[SAMPLE_SCAN_BLOCK / 64];
    double* c = cdf + (size_t)blockIdx.x * F;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    double carry = 0.0;
    for (int base = 0; base < F; base += SAMPLE_SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        double x = i < F ? c[i] : 0.0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        double before = 0.0, total = 0.0;
#pragma unroll
        for (int k = 0; k < SAMPLE_SCAN_BLOCK / 64; ++k) {
            const double s = wsum[k];
            if (k < w) before += s;
            total += s;
        }
        if (i < F) c[i] = (carry + before) + x;
        carry += total;
        __syncthreads();
    }
}

__device__ __forceinline__ float clamp01(float x) { return !(x > 0.f) ? 0.f : (x < 1.f ? x : 1.f); }   // NaN -> 0

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_msample_point(const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                 const float* __restrict__ u, const double* __restrict__ cdf, int S,
                                                                 int V, int F, float* __restrict__ points, int32_t* __restrict__ face,
                                                                 float* __restrict__ weights) {
    const int b = blockIdx.y, s = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    if (s >= S) return;
    const size_t at = (size_t)b * S + s;
    const float u0 = clamp01(u[at * 3]), u1 = clamp01(u[at * 3 + 1]), u2 = clamp01(u[at * 3 + 2]);
    const double* c = cdf + (size_t)b * F;
    const double T = c[F - 1];
    int f = 0;
    if (T > 0.0 && T <= 1.7976931348623157e308) {
        const double t = (double)u0 * T;
        int lo = 0, hi = F;                                                // smallest f with c[f] > t, F if none
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (c[mid] > t) hi = mid; else lo = mid + 1;
        }
        if (lo == F) {                                                     // only t = T (u0 = 1): the smallest f with c[f] >= T
            lo = 0; hi = F - 1;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (c[mid] >= T) hi = mid; else lo = mid + 1;
            }
        }
        f = lo;
    }
    const float r = sqrtf(u1);
    float w0 = 1.f - r, w1 = r * (1.f - u2), w2 = r * u2;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    float px = 0.f, py = 0.f, pz = 0.f;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const float* p0 = vts + ((size_t)b * V + i0) * 3;
        const float* p1 = vts + ((size_t)b * V + i1) * 3;
        const float* p2 = vts + ((size_t)b * V + i2) * 3;
        px = w0 * p0[0] + w1 * p1[0] + w2 * p2[0];
        py = w0 * p0[1] + w1 * p1[1] + w2 * p2[1];
        pz = w0 * p0[2] + w1 * p1[2] + w2 * p2[2];
    } else {
        w0 = w1 = w2 = 0.f;                                                // face 0 of a mesh without area, with a bad vertex id
    }
    points[at * 3] = px; points[at * 3 + 1] = py; points[at * 3 + 2] = pz;
    weights[at * 3] = w0; weights[at * 3 + 1] = w1; weights[at * 3 + 2] = w2;
    face[at] = f;
}

struct SampleRecords {              // the caller's workspace, cut into three arrays of B * S entries (16-byte aligned base)
    int4* id;                       // vertex ids of the face (or -1), .w unused
    float4* gw;                     // dpoints.x, .y, .z, weight of vertex 0
    float2* w12;                    // weights of vertex 1 and 2
};

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_msample_bwd_record(const int32_t* __restrict__ faces, const int32_t* __restrict__ face,
                                                                      const float* __restrict__ weights,
                                                                      const float* __restrict__ dpoints, int S, int V, int F,
                                                                      SampleRecords rec) {
    const int b = blockIdx.y, s = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    if (s >= S) return;
    const size_t at = (size_t)b * S + s;
    const int f = face[at];
    int i0 = -1, i1 = -1, i2 = -1;
    if (f >= 0 && f < F) {
        i0 = faces[(size_t)f * 3]; i1 = faces[(size_t)f * 3 + 1]; i2 = faces[(size_t)f * 3 + 2];
        if (!(i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V)) i0 = i1 = i2 = -1;
    }
    rec.id[at] = make_int4(i0, i1, i2, -1);
    rec.gw[at] = make_float4(dpoints[at * 3], dpoints[at * 3 + 1], dpoints[at * 3 + 2], weights[at * 3]);
    rec.w12[at] = make_float2(weights[at * 3 + 1], weights[at * 3 + 2]);
}

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_msample_bwd_vertex(SampleRecords rec, int S, int V, float* __restrict__ dvts) {
    __shared__ int4 s_id[SAMPLE_BLOCK];
    __shared__ float4 s_gw[SAMPLE_BLOCK];
    __shared__ float2 s_w12[SAMPLE_BLOCK];
    const int b = blockIdx.y, j = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    const int me = j < V ? j : -2;                                         // -2 matches no record (unused ids are -1)
    const size_t base = (size_t)b * S;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int s0 = 0; s0 < S; s0 += SAMPLE_BLOCK) {
        __syncthreads();
        const int i = s0 + threadIdx.x;
        if (i < S) {
            s_id[threadIdx.x] = rec.id[base + i];
            s_gw[threadIdx.x] = rec.gw[base + i];
            s_w12[threadIdx.x] = rec.w12[base + i];
        }
        __syncthreads();
        const int ns = min(SAMPLE_BLOCK, S - s0);                          // the same in every thread of the block
        for (int t = 0; t < ns; ++t) {
            const int4 id = s_id[t];                                       // one address for the whole wave: a broadcast read
            if (id.x == me || id.y == me || id.z == me) {
                const float4 gw = s_gw[t];
                const float2 w12 = s_w12[t];
                if (id.x == me) { ax += gw.w * gw.x; ay += gw.w * gw.y; az += gw.w * gw.z; }
                if (id.y == me) { ax += w12.x * gw.x; ay += w12.x * gw.y; az += w12.x * gw.z; }
                if (id.z == me) { ax += w12.y * gw.x; ay += w12.y * gw.y; az += w12.y * gw.z; }
            }
        }
    }
    if (j < V) {
        float* o = dvts + ((size_t)b * V + j) * 3;
        o[0] = ax; o[1] = ay; o[2] = az;
    }
}

}  // namespace

size_t mesh_sample_cdf_bytes(int B, int F) { return ((size_t)B * F * sizeof(double) + 15) / 16 * 16; }

void launch_mesh_sample_fwd(const float* vts, const int32_t* faces, const float* u, int B, int S, int V, int F, float* points,
                            int32_t* face, float* weights, void* ws, hipStream_t s) {
    double* cdf = static_cast<double*>(ws);                                // mesh_sample_cdf_bytes(B, F), 16-byte aligned
    prof_mark_begin(PROF_MSAMPLE_AREA, 0.0, s);
    hipLaunchKernelGGL(k_msample_area, dim3((F + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s, vts, faces, V, F, cdf);
    prof_mark_end(s);
    prof_mark_begin(PROF_MSAMPLE_SCAN, 0.0, s);
    hipLaunchKernelGGL(k_msample_scan, dim3(B), dim3(SAMPLE_SCAN_BLOCK), 0, s, cdf, F);
    prof_mark_end(s);
    prof_mark_begin(PROF_MSAMPLE_POINT, 0.0, s);
    hipLaunchKernelGGL(k_msample_point, dim3((S + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s, vts, faces, u, cdf, S, V,
                       F, points, face, weights);
    prof_mark_end(s);
}

size_t mesh_sample_bwd_record_bytes(int B, int S) { return (size_t)B * S * (sizeof(int4) + sizeof(float4) + sizeof(float2)); }

void launch_mesh_sample_bwd(const int32_t* faces, const int32_t* face, const float* weights, const float* dpoints, int B, int S, int V,
                            int F, float* dvts, void* ws, hipStream_t s) {
    const size_t n = (size_t)B * S;
    SampleRecords rec;
    rec.id = static_cast<int4*>(ws);
    rec.gw = reinterpret_cast<float4*>(rec.id + n);
    rec.w12 = reinterpret_cast<float2*>(rec.gw + n);
    prof_mark_begin(PROF_MSAMPLE_BWD_RECORD, 0.0, s);
    hipLaunchKernelGGL(k_msample_bwd_record, dim3((S + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s, faces, face,
                       weights, dpoints, S, V, F, rec);
    prof_mark_end(s);
    prof_mark_begin(PROF_MSAMPLE_BWD_VERTEX, 0.0, s);
    hipLaunchKernelGGL(k_msample_bwd_vertex, dim3((V + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s, rec, S, V, dvts);
    prof_mark_end(s);
}

}  // namespace icn
