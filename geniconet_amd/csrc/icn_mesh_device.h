// Device code shared by the mesh kernels of icn_loss.hip, icn_sample.hip, icn_measure.hip, icn_curvature.hip, icn_gauss.hip, icn_isect.hip,
// icn_sdf.hip, icn_voxel.hip, icn_raycast.hip and icn_nn.hip: 3-vectors, the incident face of a per-vertex gather and its corner in double,
// one face of a shared face list as a thread loads it and the compacted LDS tile of such faces (for the kernels that sweep all faces),
// the pixel <-> vertex rule of the icosahedral grid, fixed-order block reductions, the tiled block scan and the per-record vertex
// scatter's record set.
// Everything here is inlined into its callers; every sum has a fixed order (bit-identical run to run).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icn {

constexpr int MESH_BLOCK = 256;              // workgroup of the reductions below (4 waves)
constexpr int SCAN_BLOCK = 1024;             // workgroup = tile of block_scan

// ---- vectors ---------------------------------------------------------------------------------------------------------------
struct f3 { float x, y, z; };
__device__ __forceinline__ f3 operator-(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ f3 operator+(f3 a, f3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ f3 cross(f3 a, f3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ f3 scaled(f3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ f3 load3(const float* __restrict__ p) { return {p[0], p[1], p[2]}; }

// Cross product with every product rounded on its own, for the zero test on a face normal (the 1e-12 clamp of the mesh
// regularisers).  Contracted to fma(a.y, b.z, -(a.z * b.y)), a x a is the rounding error of one
// product, about 6e-8 |a|^2 and far above the clamp, so a face with two coincident vertices would pass for a face with a
// direction; with both products rounded a x a is exactly 0, as in the torch formulation.
__device__ __forceinline__ f3 face_normal(f3 a, f3 b) {
#pragma clang fp contract(off)
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// |n|^2 of a face normal, and whether the three vertex ids of a face index V vertices (a face that fails takes no part in anything)
__device__ __forceinline__ float norm2(f3 n) { return fmaf(n.z, n.z, fmaf(n.x, n.x, n.y * n.y)); }
__device__ __forceinline__ bool ids_ok(int i0, int i1, int i2, int V) {
    return i0 >= 0 && i0 < V && i1 >= 0 && i1 < V && i2 >= 0 && i2 < V;
}

// One incident face of vertex j, as the per-vertex gathers of icn_curvature.hip and icn_gauss.hip meet it in j's slice of the
// vertex -> corner incidence table: its three vertex ids, j's corner k, and whether to use it at all.  Entry `at` of `corners` is
// used only if it names a corner c in [0, nc = 3 F) with faces[c] == j, and only if the face's three ids index V vertices: whatever
// the table holds, nothing is read out of bounds.
struct Incident {
    int id[3], k;
    bool ok;
};

__device__ __forceinline__ Incident incident(const int32_t* __restrict__ faces, const int32_t* __restrict__ corners, int at, int j, int nc,
                                             int V) {
    Incident t;
    t.ok = false;
    const int c = corners[at];
    if (c < 0 || c >= nc || faces[c] != j) return t;
    const int f = c / 3;
    t.k = c - 3 * f;
    t.id[0] = faces[(size_t)f * 3], t.id[1] = faces[(size_t)f * 3 + 1], t.id[2] = faces[(size_t)f * 3 + 2];
    t.ok = ids_ok(t.id[0], t.id[1], t.id[2], V);
    return t;
}

// ---- the same in double: what icn_gauss.hip and icn_sdf.hip compute between their fp32 loads and their one rounding --------------
struct d3 { double x, y, z; };
__device__ __forceinline__ d3 operator-(d3 a, d3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 cross(d3 a, d3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ d3 widened(const float* __restrict__ p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ d3 widened(f3 a) { return {(double)a.x, (double)a.y, (double)a.z}; }
__device__ __forceinline__ bool finite3(f3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
__device__ __forceinline__ int sign_of(double x) { return (x > 0.0) - (x < 0.0); }

// face_normal above in double: no contraction, so that a x a is exactly 0
__device__ __forceinline__ d3 dnormal(d3 a, d3 b) {
#pragma clang fp contract(off)
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// ---- one face of the shared face list, and a tile of them in LDS --------------------------------------------------------------
// Face f < F as a thread loads it: ids, vertices (zeros unless the ids index V vertices: nothing is read out of bounds whatever `faces`
// holds), valid = ids in range and nine finite coordinates.  What a kernel derives from it (a box, a filter) is arithmetic of its own file.
struct LoadedFace { int id[3]; f3 p[3]; bool valid; };

__device__ __forceinline__ LoadedFace load_face(const float* __restrict__ v, const int32_t* __restrict__ faces, int f, int V) {
    LoadedFace t = {};
#pragma unroll
    for (int k = 0; k < 3; ++k) t.id[k] = faces[(size_t)f * 3 + k];
    if (ids_ok(t.id[0], t.id[1], t.id[2], V)) {                              // the three loads in one region, the tests after them
#pragma unroll
        for (int k = 0; k < 3; ++k) t.p[k] = load3(v + (size_t)t.id[k] * 3);
        t.valid = finite3(t.p[0]) && finite3(t.p[1]) && finite3(t.p[2]);
    }
    return t;
}

// The words every staged face begins with: nine coordinates (vertex k at 3 k), the three ids as bit patterns; then the kernel's own.
constexpr int FACE_ID = 9, FACE_WORDS = 12;

__device__ __forceinline__ void store_face(float* __restrict__ e, const LoadedFace& t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        e[3 * k] = t.p[k].x, e[3 * k + 1] = t.p[k].y, e[3 * k + 2] = t.p[k].z;
        e[FACE_ID + k] = __int_as_float(t.id[k]);
    }
}

struct EveryValidFace {
    __device__ bool operator()(const LoadedFace&) const { return true; }
};

// Stages faces f0 .. f0 + MESH_BLOCK of the list (those below F) into `tile`, entries of WORDS floats (odd, so that the fill touches
// every bank once), one face per thread; every thread of the block calls it.  A face stays iff it is valid and keep_if(face) holds; the
// others are dropped and the survivors compacted by ballot and popcount: a wave's count through wave_count[], the waves before it summed
// in wave order.  No atomics, and THE SURVIVORS KEEP THE ASCENDING ORDER OF THEIR FACE INDEX: k_mesh_raycast's rule for equal
// parameters (the lowest index wins by `t < best` alone) rests on it.  fill(face, f, entry) writes the words from FACE_WORDS on.  Opens
// with the barrier that ends the readers of the tile's previous contents, closes with the one that publishes this one -> entries staged.
template <int WORDS, class Fill, class Keep = EveryValidFace>
__device__ __forceinline__ int stage_face_tile(float* tile, int (&wave_count)[MESH_BLOCK / 64], const float* __restrict__ v,
                                               const int32_t* __restrict__ faces, int f0, int F, int V, Fill fill, Keep keep_if = Keep()) {
    static_assert(WORDS >= FACE_WORDS && WORDS % 2 == 1, "an entry holds the common words and has an odd stride");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    const int f = f0 + threadIdx.x;                                          // F <= 0x7fffffff / 3: no overflow
    LoadedFace t = {};
    if (f < F) t = load_face(v, faces, f, V);
    const bool keep = t.valid && keep_if(t);
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(kept);
    __syncthreads();
    int before = 0, nf = 0;
#pragma unroll
    for (int w = 0; w < MESH_BLOCK / 64; ++w) {
        const int n = wave_count[w];
        before += w < wave ? n : 0;
        nf += n;
    }
    if (keep) {
        float* e = tile + (before + __popcll(kept & ((1ull << lane) - 1ull))) * WORDS;
        store_face(e, t);
        fill(t, f, e);
    }
    __syncthreads();
    return nf;
}

// the vertex ids of corners k + 1 and k + 2 of an incident face (selects, not a runtime index into registers)
__device__ __forceinline__ int next_id(const Incident& t) { return t.k == 0 ? t.id[1] : (t.k == 1 ? t.id[2] : t.id[0]); }
__device__ __forceinline__ int after_id(const Incident& t) { return t.k == 0 ? t.id[2] : (t.k == 1 ? t.id[0] : t.id[1]); }

// The face of `t` as thread j sees it: pj = vertex j = corner k, q1 / q2 the vertices of corners k + 1 / k + 2, and the normal of
// corner 0 whichever corner j sits at, so that the three threads of a face agree on whether it is resolved.
struct Corner {
    d3 a, b, n;        // q1 - pj, q2 - pj, (v1 - v0) x (v2 - v0)
    double nn;
};

__device__ __forceinline__ Corner corner(const float* __restrict__ v, const Incident& t, d3 pj) {
    const int i1 = next_id(t), i2 = after_id(t);
    const d3 q1 = widened(v + (size_t)i1 * 3), q2 = widened(v + (size_t)i2 * 3);
    Corner c;
    c.a = q1 - pj, c.b = q2 - pj;
    // corner 0 of the face: (pj, q1, q2) for k = 0, (q2, pj, q1) for k = 1, (q1, q2, pj) for k = 2
    c.n = t.k == 0 ? dnormal(c.a, c.b) : (t.k == 1 ? dnormal(pj - q2, q1 - q2) : dnormal(q2 - q1, pj - q1));
    c.nn = c.n.x * c.n.x + c.n.y * c.n.y + c.n.z * c.n.z;
    return c;
}

// ---- pixels and vertices of the icosahedral grid (n = 2^r) ------------------------------------------------------------------
// Vertex j < P is pixel j of the channels-last grid (B, P, 3); vertices P and P + 1 are the N / S pole, the mean of the 5 chart
// corners pole_corner(n, k, 0..4) (reference ico_utils.py:10-24).  Backwards, a pole's gradient goes to those 5 pixels, a fifth each.
__device__ __forceinline__ int pole_corner(int n, int k, int c) {
    return k == 0 ? (c * n) * 2 * n : ((c + 1) * n - 1) * 2 * n + (2 * n - 1);
}

// the pole (0 N, 1 S) that pixel j is a corner of, or -1: the inverse of pole_corner (first / last pixel of a chart of 2 n^2)
__device__ __forceinline__ int pole_of_pixel(int j, int n) {
    const int chart = 2 * n * n;
    return j % chart == 0 ? 0 : ((j + 1) % chart == 0 ? 1 : -1);
}

// vertex j of sample b; poles: sum of the 5 corners / 5 (torch .mean)
__device__ __forceinline__ f3 vertex(const float* __restrict__ g, int b, int j, int P, int n) {
    if (j < P) return load3(g + ((size_t)b * P + j) * 3);
    f3 s = {0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 5; ++c) s = s + load3(g + ((size_t)b * P + pole_corner(n, j - P, c)) * 3);
    return {s.x / 5.f, s.y / 5.f, s.z / 5.f};
}

// dg[b, j] = up * (grad(j) + grad(pole) / 5) for grad(x) = the gradient with respect to vertex x of sample b; one thread per
// (sample, pixel), every element of dg written once
template <class Grad>
__device__ __forceinline__ void store_pixel_grad(float* __restrict__ dg, int b, int j, int P, int n, float up, Grad grad) {
    __builtin_assume(j < P);                                             // a pixel: grad(j) needs no pole branch
    f3 d = grad(j);
    const int pole = pole_of_pixel(j, n);
    if (pole >= 0) {
        const f3 dp = grad(P + pole);
        d = d + f3{dp.x / 5.f, dp.y / 5.f, dp.z / 5.f};
    }
    float* o = dg + ((size_t)b * P + j) * 3;
    o[0] = up * d.x;
    o[1] = up * d.y;
    o[2] = up * d.z;
}

// ---- reductions -------------------------------------------------------------------------------------------------------------
// Block sum of N values per thread in a fixed order (xor shuffles inside a wave, then a tree over the 4 wave totals);
// thread 0 stores the N sums to out.  Every thread of the block calls it.  T: float or double.
template <int N, typename T>
__device__ __forceinline__ void block_sum_store(T (&v)[N], T* __restrict__ out) {
    __shared__ T red[N][MESH_BLOCK / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1)
#pragma unroll
        for (int c = 0; c < N; ++c) v[c] += __shfl_xor(v[c], d, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < N; ++c) red[c][threadIdx.x >> 6] = v[c];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < N; ++c) out[c] = (red[c][0] + red[c][1]) + (red[c][2] + red[c][3]);
}

// Second level: one block sums nblocks rows of N partials (float or double) in double (lanes stride over the rows, then a fixed
// tree); the N sums are valid in thread 0.
template <int N, typename T>
__device__ __forceinline__ void partials_sum(const T* __restrict__ partial, int nblocks, double (&s)[N]) {
    __shared__ double red[N][MESH_BLOCK];
    for (int c = 0; c < N; ++c) s[c] = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += MESH_BLOCK)
        for (int c = 0; c < N; ++c) s[c] += (double)partial[(size_t)k * N + c];
    for (int c = 0; c < N; ++c) red[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int d = MESH_BLOCK / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d)
            for (int c = 0; c < N; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + d];
        __syncthreads();
    }
    for (int c = 0; c < N; ++c) s[c] = red[c][0];
}

// ---- scan -------------------------------------------------------------------------------------------------------------------
// Scan in place of c[0 .. n) by one block of SCAN_BLOCK threads over tiles of SCAN_BLOCK in a fixed order: a shuffle scan
// inside each wave, the wave totals through LDS, a running carry from tile to tile.  Element i becomes
// (carry + the waves before) + the wave's inclusive prefix, less its own value when exclusive: bit-identical run to run, also in
// floating point, where neighbouring elements are summed in different association orders.
template <typename T, bool INCLUSIVE>
__device__ __forceinline__ void block_scan(T* __restrict__ c, int n) {
    __shared__ T wsum[SCAN_BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T carry = 0;
    for (int base = 0; base < n; base += SCAN_BLOCK) {
        const int i = base + threadIdx.x;
        const T v = i < n ? c[i] : T(0);
        T x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        T before = 0, total = 0;
#pragma unroll
        for (int k = 0; k < SCAN_BLOCK / 64; ++k) {
            const T s = wsum[k];
            if (k < w) before += s;
            total += s;
        }
        if (i < n) c[i] = INCLUSIVE ? (carry + before) + x : (carry + before) + x - v;
        carry += total;
        __syncthreads();
    }
}

// ---- records -> vertices ----------------------------------------------------------------------------------------------------
// What a per-point (per-sample) backward leaves for launch_vertex_scatter (icn_sample.hip): record i of mesh b, at b * n + i,
// adds w_k * g to vertex id_k of that mesh for k = 0, 1, 2; id -1 takes no part.  A workspace of vertex_records_bytes(B * n)
// bytes, 16-byte aligned, cut into three arrays of B * n entries.
struct VertexRecords {
    int4* id;                       // vertex ids of the face (or -1), .w unused
    float4* gw;                     // g.x, g.y, g.z, weight of vertex 0
    float2* w12;                    // weights of vertex 1 and 2
};
constexpr size_t VERTEX_RECORD_BYTES = sizeof(int4) + sizeof(float4) + sizeof(float2);      // 40

inline VertexRecords vertex_records(void* ws, size_t n) {
    VertexRecords rec;
    rec.id = static_cast<int4*>(ws);
    rec.gw = reinterpret_cast<float4*>(rec.id + n);
    rec.w12 = reinterpret_cast<float2*>(rec.gw + n);
    return rec;
}

}  // namespace icn
