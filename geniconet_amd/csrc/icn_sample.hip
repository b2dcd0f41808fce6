// Area-weighted surface sampling of triangle meshes (icn_mesh_sample_fwd / icn_mesh_sample_bwd in include/icn.h): the points that
// kaolin's sample_points / pytorch3d's sample_points_from_meshes draw, from uniforms the CALLER supplies -- the kernels draw no
// random numbers, so every output is a pure function of the inputs.  vertices (B, V, 3), faces (F, 3) shared by the batch,
// u (B, S, 3).  Per mesh (blockIdx.y):
//   k_msample_area    A_f = 0.5 |(v1 - v0) x (v2 - v0)| in fp32 -> c[f] as a double.  Every product of the cross product is rounded on
//                     its own (face_normal, icn_mesh_device.h), as in the torch formulation (sampling.py), so a face with two or
//                     three coincident vertices has area exactly 0.  A face with a vertex id outside [0, V) counts as area 0.
//   k_msample_scan    inclusive block_scan of c in place, in double, one workgroup per mesh: c_f = A_0 + ... + A_f, T = c_{F - 1}.
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
//                         contributes nothing and nothing is read out of bounds), dpoints and the weights -> a VertexRecords entry
//   k_vertex_scatter      the records -> dvertices, below; also the vertex pass of the point-to-mesh backward (icn_loss.hip)
//
// Normal agreement of two sampled surfaces (icn_face_normal_agree_fwd / _bwd in include/icn_ext.h): per sample s of mesh pair b the
// faces fa = face_a[b, s] of mesh a and fb = face_b[b, s] of mesh b, t = 1 - n^_a . n^_b (oriented) or 1 - |n^_a . n^_b|.
//   n = e1 x e2 (face_normal), resolved iff |n|^2 2^22 > |e1|^2 |e2|^2 with all of it finite (TRI_FLAT of tri_dist2, icn_loss.hip);
//   n^ = n / |n| where resolved.  An unresolved face on either side -- a face id outside [0, F) and a vertex id outside [0, V)
//   count as one, nothing is read out of bounds -- gives t = 1 and no gradient on either side.
//   k_fnormal_agree             one thread per sample: the six vertices -> t[b, s]
//   k_fnormal_agree_bwd_record  one thread per sample, for ONE side ("own", the other side's arguments swapped in for side b):
//                               h = -sigma dt (n^_other - c n^_own) / |n_own|, d/dv1 = e2 x h, d/dv2 = h x e1, d/dv0 = -(both):
//                               two VertexRecords entries, 2 s: ids (i1, i0, -1), vector d/dv1, weights (1, -1, 0); 2 s + 1:
//                               ids (i2, i0, -1), vector d/dv2, weights (1, -1, 0); ids (-1, -1, -1) where unresolved
//   k_vertex_scatter            n = 2 S records per mesh -> dvertices of that side, as above
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

namespace icn {

namespace {

constexpr int SAMPLE_BLOCK = 256;

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_msample_area(const float* __restrict__ vts, const int32_t* __restrict__ faces, int V,
                                                                int F, double* __restrict__ cdf) {
    const int b = blockIdx.y, f = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    float area = 0.f;
    if (i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V) {
        const f3 p0 = load3(vts + ((size_t)b * V + i0) * 3);
        const f3 a = load3(vts + ((size_t)b * V + i1) * 3) - p0, e = load3(vts + ((size_t)b * V + i2) * 3) - p0;
        // face_normal rounds every product on its own: a zero edge vector (v1 = v0 or v2 = v0) and equal edge vectors (v1 = v2)
        // both give a normal of exactly 0, so the area is exactly 0.  Contracted to one fma per component, v1 = v2 would leave
        // the rounding error of one product, about 6e-8 |v1 - v0|^2, and the face could be drawn.
        const f3 nrm = face_normal(a, e);
        area = 0.5f * sqrtf(fmaf(nrm.z, nrm.z, fmaf(nrm.x, nrm.x, nrm.y * nrm.y)));
    }
    cdf[(size_t)b * F + f] = (double)area;
}

__global__ __launch_bounds__(SCAN_BLOCK) void k_msample_scan(double* __restrict__ cdf, int F) {
    block_scan<double, true>(cdf + (size_t)blockIdx.x * F, F);
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

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_msample_bwd_record(const int32_t* __restrict__ faces, const int32_t* __restrict__ face,
                                                                      const float* __restrict__ weights,
                                                                      const float* __restrict__ dpoints, int S, int V, int F,
                                                                      VertexRecords rec) {
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

// ---- normal agreement -------------------------------------------------------------------------------------------------------
constexpr float NORMAL_FLAT = 4194304.f;       // 2^22: TRI_FLAT of tri_dist2 (icn_loss.hip), here a constant of the definition

struct FaceFrame {
    f3 e1, e2, unit;                            // edges from vertex 0, n / |n|
    float len;                                  // |n|
    int i0, i1, i2;
    bool ok;                                    // ids in range and the normal resolved; nothing else is valid otherwise
};

__device__ __forceinline__ FaceFrame face_frame(const float* __restrict__ vts, const int32_t* __restrict__ faces, int b, int f, int V,
                                                int F) {
    FaceFrame r;
    r.ok = false;
    r.i0 = r.i1 = r.i2 = -1;
    r.e1 = r.e2 = r.unit = f3{0.f, 0.f, 0.f};
    r.len = 1.f;
    if (f < 0 || f >= F) return r;
    const int i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
    if (!(i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V)) return r;
    const f3 p0 = load3(vts + ((size_t)b * V + i0) * 3);
    const f3 e1 = load3(vts + ((size_t)b * V + i1) * 3) - p0, e2 = load3(vts + ((size_t)b * V + i2) * 3) - p0;
    const f3 n = face_normal(e1, e2);           // every product rounded on its own: exactly 0 for coincident vertices
    const float nn = fmaf(n.z, n.z, fmaf(n.x, n.x, n.y * n.y));
    const float q = nn * NORMAL_FLAT, ll = dot(e1, e1) * dot(e2, e2);
    if (!(q > ll) || !(q <= 3.4028234663852886e38f)) return r;            // flat, NaN or overflowed (ll = inf fails q > ll)
    const float len = sqrtf(nn);
    r.e1 = e1; r.e2 = e2;
    r.unit = f3{n.x / len, n.y / len, n.z / len};
    r.len = len;
    r.i0 = i0; r.i1 = i1; r.i2 = i2;
    r.ok = true;
    return r;
}

__global__ __launch_bounds__(SAMPLE_BLOCK) void k_fnormal_agree(const float* __restrict__ va, const int32_t* __restrict__ faces_a,
                                                                 const int32_t* __restrict__ face_a, int Va, int Fa,
                                                                 const float* __restrict__ vb, const int32_t* __restrict__ faces_b,
                                                                 const int32_t* __restrict__ face_b, int Vb, int Fb, int S,
                                                                 int oriented, float* __restrict__ t) {
    const int b = blockIdx.y, s = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    if (s >= S) return;
    const size_t at = (size_t)b * S + s;
    const FaceFrame A = face_frame(va, faces_a, b, face_a[at], Va, Fa);
    const FaceFrame Bf = face_frame(vb, faces_b, b, face_b[at], Vb, Fb);
    float tv = 1.f;
    if (A.ok && Bf.ok) {
        const float c = dot(A.unit, Bf.unit);
        tv = 1.f - (oriented ? c : fabsf(c));
    }
    t[at] = tv;
}

// the records of side "own" (vo, faces_o, face_o); "other" (vx, ...) enters through its unit normal only
__global__ __launch_bounds__(SAMPLE_BLOCK) void k_fnormal_agree_bwd_record(const float* __restrict__ vo, const int32_t* __restrict__ faces_o,
                                                                            const int32_t* __restrict__ face_o, int Vo, int Fo,
                                                                            const float* __restrict__ vx, const int32_t* __restrict__ faces_x,
                                                                            const int32_t* __restrict__ face_x, int Vx, int Fx, int S,
                                                                            int oriented, const float* __restrict__ dt, VertexRecords rec) {
    const int b = blockIdx.y, s = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    if (s >= S) return;
    const size_t at = (size_t)b * S + s;
    const FaceFrame O = face_frame(vo, faces_o, b, face_o[at], Vo, Fo);
    const FaceFrame X = face_frame(vx, faces_x, b, face_x[at], Vx, Fx);
    int4 id1 = make_int4(-1, -1, -1, -1), id2 = id1;
    f3 d1 = {0.f, 0.f, 0.f}, d2 = d1;
    if (O.ok && X.ok) {
        const float c = dot(O.unit, X.unit);
        const float sigma = oriented ? 1.f : (c > 0.f ? 1.f : (c < 0.f ? -1.f : 0.f));     // d|c| / dc, 0 at c = 0
        const f3 h = scaled(X.unit - scaled(O.unit, c), -sigma * dt[at] / O.len);
        d1 = cross(O.e2, h);
        d2 = cross(h, O.e1);
        id1 = make_int4(O.i1, O.i0, -1, -1);
        id2 = make_int4(O.i2, O.i0, -1, -1);
    }
    rec.id[2 * at] = id1;
    rec.gw[2 * at] = make_float4(d1.x, d1.y, d1.z, 1.f);
    rec.w12[2 * at] = make_float2(-1.f, 0.f);
    rec.id[2 * at + 1] = id2;
    rec.gw[2 * at + 1] = make_float4(d2.x, d2.y, d2.z, 1.f);
    rec.w12[2 * at + 1] = make_float2(-1.f, 0.f);
}

// One thread per vertex: the n records of its mesh go through LDS in tiles of 256 and every thread adds those addressed to it IN
// RECORD ORDER (then vertex 0, 1, 2 of the face) -- a fixed order, no atomics, bit-identical run to run.  n * V integer compares
// per mesh, one broadcast ds_read_b128 per record and wave; a vertex no record addresses gets an exact zero.
__global__ __launch_bounds__(SAMPLE_BLOCK) void k_vertex_scatter(VertexRecords rec, int n, int V, float* __restrict__ dvts) {
    __shared__ int4 s_id[SAMPLE_BLOCK];
    __shared__ float4 s_gw[SAMPLE_BLOCK];
    __shared__ float2 s_w12[SAMPLE_BLOCK];
    const int b = blockIdx.y, j = blockIdx.x * SAMPLE_BLOCK + threadIdx.x;
    const int me = j < V ? j : -2;                                         // -2 matches no record (unused ids are -1)
    const size_t base = (size_t)b * n;
    float ax = 0.f, ay = 0.f, az = 0.f;
    for (int s0 = 0; s0 < n; s0 += SAMPLE_BLOCK) {
        __syncthreads();
        const int i = s0 + threadIdx.x;
        if (i < n) {
            s_id[threadIdx.x] = rec.id[base + i];
            s_gw[threadIdx.x] = rec.gw[base + i];
            s_w12[threadIdx.x] = rec.w12[base + i];
        }
        __syncthreads();
        const int ns = min(SAMPLE_BLOCK, n - s0);                          // the same in every thread of the block
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
    hipLaunchKernelGGL(k_msample_scan, dim3(B), dim3(SCAN_BLOCK), 0, s, cdf, F);
    prof_mark_end(s);
    prof_mark_begin(PROF_MSAMPLE_POINT, 0.0, s);
    hipLaunchKernelGGL(k_msample_point, dim3((S + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s, vts, faces, u, cdf, S, V,
                       F, points, face, weights);
    prof_mark_end(s);
}

size_t vertex_records_bytes(size_t n) { return n * VERTEX_RECORD_BYTES; }

void launch_vertex_scatter(int prof_kind, void* ws, int B, int n, int V, float* dvts, hipStream_t s) {
    prof_mark_begin(prof_kind, 0.0, s);
    hipLaunchKernelGGL(k_vertex_scatter, dim3((V + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s,
                       vertex_records(ws, (size_t)B * n), n, V, dvts);
    prof_mark_end(s);
}

void launch_mesh_sample_bwd(const int32_t* faces, const int32_t* face, const float* weights, const float* dpoints, int B, int S, int V,
                            int F, float* dvts, void* ws, hipStream_t s) {
    prof_mark_begin(PROF_MSAMPLE_BWD_RECORD, 0.0, s);
    hipLaunchKernelGGL(k_msample_bwd_record, dim3((S + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s, faces, face,
                       weights, dpoints, S, V, F, vertex_records(ws, (size_t)B * S));
    prof_mark_end(s);
    launch_vertex_scatter(PROF_MSAMPLE_BWD_VERTEX, ws, B, S, V, dvts, s);
}

void launch_face_normal_agree_fwd(const float* va, const int32_t* faces_a, const int32_t* face_a, int Va, int Fa, const float* vb,
                                  const int32_t* faces_b, const int32_t* face_b, int Vb, int Fb, int B, int S, int oriented, float* t,
                                  hipStream_t s) {
    prof_mark_begin(PROF_FNORMAL_AGREE, 0.0, s);
    hipLaunchKernelGGL(k_fnormal_agree, dim3((S + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B), dim3(SAMPLE_BLOCK), 0, s, va, faces_a, face_a, Va,
                       Fa, vb, faces_b, face_b, Vb, Fb, S, oriented, t);
    prof_mark_end(s);
}

void launch_face_normal_agree_bwd(const float* va, const int32_t* faces_a, const int32_t* face_a, int Va, int Fa, const float* vb,
                                  const int32_t* faces_b, const int32_t* face_b, int Vb, int Fb, int B, int S, int oriented,
                                  const float* dt, float* dva, float* dvb, void* ws, hipStream_t s) {
    const dim3 grid((S + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK, B);
    const VertexRecords rec = vertex_records(ws, (size_t)B * 2 * S);
    if (dva) {
        prof_mark_begin(PROF_FNORMAL_AGREE_BWD_RECORD, 0.0, s);
        hipLaunchKernelGGL(k_fnormal_agree_bwd_record, grid, dim3(SAMPLE_BLOCK), 0, s, va, faces_a, face_a, Va, Fa, vb, faces_b, face_b,
                           Vb, Fb, S, oriented, dt, rec);
        prof_mark_end(s);
        launch_vertex_scatter(PROF_FNORMAL_AGREE_BWD_VERTEX, ws, B, 2 * S, Va, dva, s);
    }
    if (dvb) {                                                             // the same workspace again, in stream order
        prof_mark_begin(PROF_FNORMAL_AGREE_BWD_RECORD, 0.0, s);
        hipLaunchKernelGGL(k_fnormal_agree_bwd_record, grid, dim3(SAMPLE_BLOCK), 0, s, vb, faces_b, face_b, Vb, Fb, va, faces_a, face_a,
                           Va, Fa, S, oriented, dt, rec);
        prof_mark_end(s);
        launch_vertex_scatter(PROF_FNORMAL_AGREE_BWD_VERTEX, ws, B, 2 * S, Vb, dvb, s);
    }
}

}  // namespace icn
