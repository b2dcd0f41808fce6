// Self-intersection count of triangle meshes (icn_mesh_self_intersect in include/icn_isect.h): for every face the number of other
// faces of the same mesh that it passes through.  vertices (B, V, 3) fp32, faces (F, 3) shared by the batch, hits (B, F) int32.
// The definition (one, for this kernel, metrics._torch_self_intersections and the tests), ALL OF IT IN DOUBLE on the fp32 vertices:
//   orient(a, b, c, d) = u.x (v.y w.z - v.z w.y) - u.y (v.x w.z - v.z w.x) + u.z (v.x w.y - v.y w.x),  u = b - a, v = c - a, w = d - a
//     in exactly this order, every product and sum rounded on its own (no contraction: the float64 reference has no FMA)
//   crosses(p, q; a, b, c): orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs (signs compared, no product), and
//     orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0
//   faces i < j INTERSECT iff an edge (A_k, A_{k+1}) of A = face i crosses B = face j or an edge of B crosses A.  The lower face index
//     is always A, so the thread of face i and the thread of face j do the same arithmetic: the relation is symmetric by construction.
//   Not tested, and not intersecting: two faces that share a vertex id (neighbours, duplicates, a face and itself), a face with an id
//     outside [0, V), a face with a coordinate that is not finite.  Strict inequalities: touching and coplanar contact do not count.
// k_mesh_self_intersect: grid (ceil(F / MESH_BLOCK), B), one thread per face i; faces j are staged through LDS in tiles of MESH_BLOCK
// as k_point_to_mesh stages its triangles.  An entry is ISECT_WORDS = 19 words -- nine coordinates, three ids, the fp32 bounding box,
// a valid flag -- and 19 is odd, so the fill (thread t writes word 19 t + k) touches every bank once; the reads are broadcasts (all
// lanes read entry j).  Per j: the fp32 boxes overlap (lo_A <= hi_B && lo_B <= hi_A on every axis; min / max of fp32 values are
// exact and a crossing needs a common point, so the filter removes no hit), then valid, not i, no shared id, and only then the
// double arithmetic.
// Every thread visits all other faces and writes hits[b, i] once: no atomics, bit-identical run to run.  O(F^2) per mesh: the entry
// refuses F > ICN_SELF_INTERSECT_MAX_FACES.  MI355X, I5 / batch 36 (7.5e9 pairs): 8.7 ms on the unit sphere, where the scan over the
// boxes is everything, and 15.4 ms with vertex noise of sigma 0.05, where 19 pairs per face reach the double arithmetic and it takes
// 44 % of the time (few lanes of a wave are in it at once), beside 28 - 29 ms for k_point_to_mesh on as many points
// (profiles/self_intersect.txt).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

namespace icn {
namespace {

constexpr int ISECT_WORDS = 19;              // 9 coordinates, 3 ids, box lo / hi, valid: odd, so the fills are conflict-free
constexpr int ISECT_LO = FACE_WORDS, ISECT_HI = 15, ISECT_VALID = 18;

__device__ __forceinline__ d3 pick(bool first, d3 a, d3 b) { return {first ? a.x : b.x, first ? a.y : b.y, first ? a.z : b.z}; }

__device__ __forceinline__ double orient(d3 a, d3 b, d3 c, d3 d) {
#pragma clang fp contract(off)
    const d3 u = {b.x - a.x, b.y - a.y, b.z - a.z}, v = {c.x - a.x, c.y - a.y, c.z - a.z}, w = {d.x - a.x, d.y - a.y, d.z - a.z};
    return u.x * (v.y * w.z - v.z * w.y) - u.y * (v.x * w.z - v.z * w.x) + u.z * (v.x * w.y - v.y * w.x);
}

// segment (p, q) with the plane values sp = orient(a,b,c,p), sq = orient(a,b,c,q) against triangle (a, b, c)
__device__ __forceinline__ bool crosses(d3 p, d3 q, double sp, double sq, d3 a, d3 b, d3 c) {
    if (!((sp > 0.0 && sq < 0.0) || (sp < 0.0 && sq > 0.0))) return false;
    const double o0 = orient(p, q, a, b), o1 = orient(p, q, b, c), o2 = orient(p, q, c, a);
    return (o0 > 0.0 && o1 > 0.0 && o2 > 0.0) || (o0 < 0.0 && o1 < 0.0 && o2 < 0.0);
}

// the six tests of faces A (the lower index) and B; the plane value of a vertex is the same number for both edges it ends
__device__ __forceinline__ bool faces_intersect(const d3 (&A)[3], const d3 (&B)[3]) {
    const double a0 = orient(B[0], B[1], B[2], A[0]), a1 = orient(B[0], B[1], B[2], A[1]), a2 = orient(B[0], B[1], B[2], A[2]);
    if (crosses(A[0], A[1], a0, a1, B[0], B[1], B[2]) || crosses(A[1], A[2], a1, a2, B[0], B[1], B[2]) ||
        crosses(A[2], A[0], a2, a0, B[0], B[1], B[2]))
        return true;
    const double b0 = orient(A[0], A[1], A[2], B[0]), b1 = orient(A[0], A[1], A[2], B[1]), b2 = orient(A[0], A[1], A[2], B[2]);
    return crosses(B[0], B[1], b0, b1, A[0], A[1], A[2]) || crosses(B[1], B[2], b1, b2, A[0], A[1], A[2]) ||
           crosses(B[2], B[0], b2, b0, A[0], A[1], A[2]);
}

// One face as a thread loads it (load_face of icn_mesh_device.h) and its fp32 box.  f < F.
struct StagedFace : LoadedFace {
    f3 lo, hi;
};

__device__ __forceinline__ StagedFace staged_face(const float* __restrict__ v, const int32_t* __restrict__ faces, int f, int V) {
    StagedFace t = {load_face(v, faces, f, V), {}, {}};
    t.lo = {fminf(fminf(t.p[0].x, t.p[1].x), t.p[2].x), fminf(fminf(t.p[0].y, t.p[1].y), t.p[2].y), fminf(fminf(t.p[0].z, t.p[1].z), t.p[2].z)};
    t.hi = {fmaxf(fmaxf(t.p[0].x, t.p[1].x), t.p[2].x), fmaxf(fmaxf(t.p[0].y, t.p[1].y), t.p[2].y), fmaxf(fmaxf(t.p[0].z, t.p[1].z), t.p[2].z)};
    return t;
}

__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_self_intersect(const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                     int V, int F, int32_t* __restrict__ hits) {
    __shared__ float tile[MESH_BLOCK * ISECT_WORDS];
    const int b = blockIdx.y, i = blockIdx.x * MESH_BLOCK + threadIdx.x;     // F <= 2^20: no overflow
    const float* v = vts + (size_t)b * V * 3;
    const bool live = i < F;
    StagedFace me = {};
    if (live) me = staged_face(v, faces, i, V);
    const bool active = live && me.valid;
    int count = 0;
    for (int f0 = 0; f0 < F; f0 += MESH_BLOCK) {
        __syncthreads();
        const int f = f0 + threadIdx.x;
        if (f < F) {
            const StagedFace t = staged_face(v, faces, f, V);
            float* e = tile + threadIdx.x * ISECT_WORDS;
            store_face(e, t);
            e[ISECT_LO] = t.lo.x, e[ISECT_LO + 1] = t.lo.y, e[ISECT_LO + 2] = t.lo.z;
            e[ISECT_HI] = t.hi.x, e[ISECT_HI + 1] = t.hi.y, e[ISECT_HI + 2] = t.hi.z;
            e[ISECT_VALID] = __int_as_float(t.valid ? 1 : 0);
        }
        __syncthreads();
        const int nf = min(MESH_BLOCK, F - f0);
        if (active)
            for (int jj = 0; jj < nf; ++jj) {
                const float* e = tile + jj * ISECT_WORDS;
                const int j = f0 + jj;
                // the fp32 boxes.  The three rejections are independent, so their order changes no result; this one comes first
                // because it is the cheapest and ends almost every pair (all but 464 of 2.1e8 on the I5 sphere), which takes the id
                // compares and four of the ten LDS reads out of the hot loop: 19.8 ms with the ids first, 8.7 ms so, at I5 / batch 36
                const bool overlap = (me.lo.x <= e[ISECT_HI]) & (e[ISECT_LO] <= me.hi.x) & (me.lo.y <= e[ISECT_HI + 1]) &
                                     (e[ISECT_LO + 1] <= me.hi.y) & (me.lo.z <= e[ISECT_HI + 2]) & (e[ISECT_LO + 2] <= me.hi.z);
                if (!overlap) continue;
                // the face itself, invalid faces, shared vertex ids
                const int j0 = __float_as_int(e[FACE_ID]), j1 = __float_as_int(e[FACE_ID + 1]), j2 = __float_as_int(e[FACE_ID + 2]);
                const bool shared = (j0 == me.id[0]) | (j0 == me.id[1]) | (j0 == me.id[2]) | (j1 == me.id[0]) | (j1 == me.id[1]) |
                                    (j1 == me.id[2]) | (j2 == me.id[0]) | (j2 == me.id[1]) | (j2 == me.id[2]);
                if (j == i || __float_as_int(e[ISECT_VALID]) == 0 || shared) continue;
                // the six tests in double, the lower face index as A
                const bool first = i < j;
                d3 A[3], Bt[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const d3 mine = widened(me.p[k]), other = widened(f3{e[3 * k], e[3 * k + 1], e[3 * k + 2]});
                    A[k] = pick(first, mine, other);
                    Bt[k] = pick(first, other, mine);
                }
                count += faces_intersect(A, Bt) ? 1 : 0;
            }
    }
    if (live) hits[(size_t)b * F + i] = count;
}

}  // namespace

void launch_mesh_self_intersect(const float* vts, const int32_t* faces, int B, int V, int F, int32_t* hits, hipStream_t s) {
    prof_mark_begin(PROF_MESH_SELF_INTERSECT, 0.0, s);
    hipLaunchKernelGGL(k_mesh_self_intersect, dim3((unsigned)((F + MESH_BLOCK - 1) / MESH_BLOCK), B), dim3(MESH_BLOCK), 0, s, vts, faces, V,
                       F, hits);
    prof_mark_end(s);
}

}  // namespace icn
