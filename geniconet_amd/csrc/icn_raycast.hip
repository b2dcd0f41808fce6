// Ray casting against batched triangle meshes (icn_mesh_raycast / icn_mesh_raycast_bwd in include/icn_raycast.h): for every ray the
// first face it meets, the parameter of that hit and the number of faces it crosses.  vertices (B, V, 3) fp32, faces (F, 3) shared by
// the batch, origins / directions (B, R, 3) fp32; depth (B, R) fp32, face and count (B, R) int32.
// The definition (one, for this kernel, metrics._torch_ray_cast and the tests), ALL OF IT IN DOUBLE on the fp32 values as stored, every
// product and sum rounded on its own in the order written (no contraction: the float64 reference has no FMA):
//   a ray is LIVE iff its six values are finite and d != (0, 0, 0); any other ray answers a miss (depth +inf, face -1, count 0)
//   a face is TESTED iff its ids lie in [0, V) and its nine coordinates are finite; p_k = v_k - o
//   the edge value of a directed edge u -> w: with (a, b) = (p_u, p_w) if id_u < id_w, else (p_w, p_u),
//     N = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x),  s = (d.x N.x + d.y N.y) + d.z N.z,
//     tau = sign(s), if 0 sign(N.x), if still 0 sign(N.y), if still 0 sign(N.z)   (the symbolic perturbation d + (eps, eps^2, eps^3));
//     both negated if the ends were swapped: the two faces of an edge evaluate one expression and get opposite values, and an edge
//     from a vertex to itself gets N = 0 exactly, so tau = 0
//   the face COVERS the ray iff tau > 0 for its three edges or tau < 0 for all three
//   its parameter, from the raw values s0, s1, s2 of the edges opposite vertices 0, 1, 2 (v1 -> v2, v2 -> v0, v0 -> v1):
//     c_k = (p_k.x d.x + p_k.y d.y) + p_k.z d.z,  S = (s0 + s1) + s2,  dd = (d.x d.x + d.y d.y) + d.z d.z,
//     t = ((s0 c0 + s1 c1) + s2 c2) / (S dd)
//   a HIT is a covering face whose t is finite and > 0
//   count = the number of hits, face = the hit of smallest t (the lowest face index among equal t; -1 if none), depth = (float)t of
//   that face, else +inf.  The products of fp32 values stay far inside the range of a double (|s c| < 1e194), so a NaN arises only as
//   0 / 0 and is no hit: no NaN ever comes out.
// k_mesh_raycast: grid (ceil(R / MESH_BLOCK), B), one thread per ray.  Faces are staged through LDS in tiles of MESH_BLOCK in the
// sequence of stage_face_tile (icn_mesh_device.h), written out here: through the shared template this kernel measured 1 - 2 % slower on
// rays aimed at the vertices, more than the spread of three runs (profiles/mesh_face_tile.txt).  A face that is not TESTED is dropped
// while staging and the survivors are compacted by ballot and popcount, which keeps them in ascending face order: `t < best` alone gives the lowest index among equal t.  An entry is nine
// coordinates, three ids, the face index and the eight words of the filter below, 21 words -- odd, so the fill touches every bank once;
// the reads are broadcasts.  Each thread keeps (best t, best face, count) in registers and writes its three outputs once, misses and
// dead rays too.  No atomics, no workspace, safe whatever `faces` holds, bit-identical run to run and equal to the float64 formulation
// bit for bit.
//
// THE REJECT FILTER in front of the double arithmetic (template parameter CULL; -DICN_RAYCAST_NO_CULL builds the kernel without it, for
// tools/time_raycast.py).  It is not part of the definition: it may only skip a face that the definition would find NOT COVERING.
// Staged with the face, computed in double and rounded to fp32: c the centroid, R2 = 2.25 rho^2 (1 + 2^-18) with rho the largest
// distance of a vertex from c (as rounded), nh the unit normal, K = 2^30 rho w with w = |n| / l_max the smallest altitude (K = 0 when
// the face has no normal or w < 2^-10 rho).  Per ray u = d / |d| in double, rounded.  With m = c - o, all in fp32:
//     FAR   mm >= 2^-100  and  mm - (m.u)^2 > R2 + 2^-18 mm         (mm = m.m)
//     STEEP (|nh.u| - 2^-16) K > mm + R2
//     the face is skipped iff FAR and STEEP.  THE ENDS OF THE fp32 RANGE all fall on the side of "not skipped".  Overflow: a NaN or an
//     infinity on either side makes a comparison false (mm = inf gives inf > inf or NaN in FAR; mm + R2 = inf fails STEEP), and K is
//     clamped to 2^127 before it is rounded, so it is never inf and never above its true value by more than a rounding.  Underflow,
//     where an fp32 rounding is an absolute 2^-149 and no longer 2^-24 of the value: an R2 that rounds below 2^-100 is staged as +inf
//     (never FAR), and FAR asks for mm >= 2^-100, so that R2, mm and 2^-18 mm are normal numbers and the few underflowing products
//     inside m.u and mm (each off by at most 2^-149 <= 2^-49 mm) vanish in the margin; a difference c - o that is subnormal is exact;
//     a K that rounds into the subnormals is at most twice its true value and then K <= 2^-126 < mm + R2 fails STEEP anyway.  The double
//     arithmetic never underflows: its smallest products, of three fp32 subnormals, are about 1e-135.
// A distance test alone would NOT do.  COVERS is defined on the COMPUTED edge values; when the plane of a face holds the ray, all three
// exact values are 0, the computed ones are rounding noise, and where they agree in sign the definition counts a hit however far the
// face is from the ray (tests/test_ray_cast.py builds such faces on the plane x = 3 y).  STEEP keeps those for the double path.
// PROOF that a skipped face does not cover.  Exact quantities are those of the fp32 inputs; u0 = 2^-53.
//  1. FAR gives D >= 1.5 rho for the true distance D from c to the ray's line: the fp32 roundings of m, u (|u| = 1 +- 2^-23), m.u and
//     mm change mm - (m.u)^2 by less than 2^-20 mm (all of them relative roundings, or negligible, once mm >= 2^-100), the margin is
//     2^-18 mm, and R2 >= 2^-100 is rounded up from 2.25 rho^2: (1 - 2^-24)(1 + 2^-18)(1 - 2^-24) > 1.
//  2. STEEP gives |nh.d| / |d| >= 2^-17: nh.u carries at most 2^-21 of absolute error (2^-24 a component of nh and of u, three
//     roundings), and the computed value is at least 2^-16.  So the line meets the face's plane, at X say, and |X - c| >= D.
//  3. In that plane take coordinates about X with the first axis towards c.  Every vertex has first coordinate nu_k >= |X - c| - rho > 0
//     and lies within |X - c| + rho of X.  With lambda_k = (second coordinate) / nu_k, the tangent of the angle at which X sees vertex
//     k, the in-plane orientation of (X, v_i, v_j) is nu_i nu_j (lambda_j - lambda_i), and the exact edge value is
//         s(i -> j) = d . (p_i x p_j) = (d . nh) nu_i nu_j (lambda_j - lambda_i)
//     (p = v - o differs from v - X by a multiple of d, which the determinant ignores).  Round the triangle the three differences sum
//     to 0: the edge between the largest and the smallest lambda has |difference| = L, their spread, and of the other two edges -- whose
//     differences have the other sign -- one has at least L / 2.  Tangents spread at least as much as angles, and a triangle seen under
//     the angle A from a point it lies within r of has width at most r A in some direction, so L >= w / (|X - c| + rho).
//     Hence two edges have exact values of opposite sign, each at least
//         |d . nh| (|X - c| - rho)^2 w / (2 (|X - c| + rho)) >= |d . nh| rho w / 20       (increasing in |X - c| >= 1.5 rho).
//  4. A computed edge value differs from the exact one by less than 2^-49 |d| P^2, P = max |p_k| <= |m| + rho: p is rounded once (u0 a
//     component), N twice a product and once (3 u0 of |a_j b_k| + |a_k b_j|), s three times more; the sum of the six |d_i a_j b_k| is at
//     most sqrt(2) |d| |a| |b|; together below 12 u0 |d| P^2.  P^2 <= 2 (mm + rho^2).
//  5. STEEP, with at least three quarters of the computed |nh.u| true and K = 2^30 rho w, gives |d . nh| rho w / 20 > 2^-35 |d|
//     (mm + rho^2) >= 2^-36 |d| P^2, which is 2^13 times the error of 4.  So those two computed values have the signs of the exact ones,
//     are not 0 (no tie-break), and differ in sign: tau is not the same on all three edges, whichever ends were swapped.  QED.
// The constants are loose on purpose (2^13 to spare, 2^5 on the floor of |nh.u|): the filter loses only faces within 1.5 rho of the
// ray, faces thinner than 2^-10, rays within 2^-16 of a far face's plane and scenes below 2^-50 or above 2^63 in size to the double
// path, where nothing can go wrong.
// Timings on an MI355X, with and without it: profiles/raycast.txt (tools/time_raycast.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

#pragma clang fp contract(off)

namespace icn {
namespace {

constexpr int RAY_FACE = FACE_WORDS, RAY_CENTRE = 13, RAY_R2 = 16, RAY_NORMAL = 17, RAY_K = 20;   // after the common words
constexpr int RAY_WORDS = 21;               // 9 coordinates, 3 ids, the face index, c, R2, nh, K: odd, so the fills are conflict-free

// the raw value s and the decided sign tau of the directed edge u -> w for direction d, evaluated on its ends in the order of their ids
__device__ __forceinline__ void ray_edge(int iu, int iw, d3 pu, d3 pw, d3 d, double& s, int& tau) {
    const bool as_given = iu < iw;
    const d3 a = as_given ? pu : pw, b = as_given ? pw : pu;
    const d3 n = dnormal(a, b);
    const double v = (d.x * n.x + d.y * n.y) + d.z * n.z;
    int sign = sign_of(v);
    if (sign == 0) sign = sign_of(n.x);
    if (sign == 0) sign = sign_of(n.y);
    if (sign == 0) sign = sign_of(n.z);
    s = as_given ? v : -v;
    tau = as_given ? sign : -sign;
}

__device__ __forceinline__ double dot_in_order(d3 a, d3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

template <bool CULL>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_raycast(const float* __restrict__ org, const float* __restrict__ dir,
                                                              const float* __restrict__ vts, const int32_t* __restrict__ faces, int R, int V,
                                                              int F, float* __restrict__ depth, int32_t* __restrict__ face,
                                                              int32_t* __restrict__ count) {
    constexpr int WORDS = RAY_WORDS;
    __shared__ float tile[MESH_BLOCK * WORDS];
    __shared__ int wave_count[MESH_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, r = blockIdx.x * MESH_BLOCK + tid;
    const float* v = vts + (size_t)b * V * 3;
    const size_t at = (size_t)b * R + (r < R ? r : 0);                      // threads past R read ray 0 of the mesh and write nothing
    const f3 o32 = load3(org + at * 3), d32 = load3(dir + at * 3);
    const bool live = r < R && finite3(o32) && finite3(d32) && !(d32.x == 0.f && d32.y == 0.f && d32.z == 0.f);
    const d3 o = widened(o32), d = widened(d32);
    const double dd = dot_in_order(d, d);
    f3 u32 = {0.f, 0.f, 0.f};
    if (CULL) {
        const double len = sqrt(dd);
        u32 = {(float)(d.x / len), (float)(d.y / len), (float)(d.z / len)};
    }
    double best = INFINITY;
    int best_face = -1, hits = 0;
    for (int f0 = 0; f0 < F; f0 += MESH_BLOCK) {
        __syncthreads();
        const int f = f0 + tid;                                              // F <= 0x7fffffff / 3: no overflow
        int id[3] = {0, 0, 0};
        f3 p[3] = {};
        bool keep = false;
        if (f < F) {
#pragma unroll
            for (int c = 0; c < 3; ++c) id[c] = faces[(size_t)f * 3 + c];
            if (ids_ok(id[0], id[1], id[2], V)) {
                keep = true;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p[c] = load3(v + (size_t)id[c] * 3);
                    keep = keep && finite3(p[c]);
                }
            }
        }
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
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                e[3 * c] = p[c].x, e[3 * c + 1] = p[c].y, e[3 * c + 2] = p[c].z;
                e[FACE_ID + c] = __int_as_float(id[c]);
            }
            e[RAY_FACE] = __int_as_float(f);
            if (CULL) {                                                      // the filter's eight words, in double, rounded once
                const d3 q0 = widened(p[0]), q1 = widened(p[1]), q2 = widened(p[2]);
                const f3 c = {(float)((q0.x + q1.x + q2.x) / 3.0), (float)((q0.y + q1.y + q2.y) / 3.0), (float)((q0.z + q1.z + q2.z) / 3.0)};
                const d3 cd = widened(c), e01 = q1 - q0, e02 = q2 - q0, e12 = q2 - q1;
                const double rr = fmax(fmax(dot(q0 - cd, q0 - cd), dot(q1 - cd, q1 - cd)), dot(q2 - cd, q2 - cd));
                const double ll = fmax(fmax(dot(e01, e01), dot(e02, e02)), dot(e12, e12));
                const d3 n = dnormal(e01, e02);
                const double len = sqrt(dot(n, n)), rho = sqrt(rr), w = len / sqrt(ll);
                const bool shaped = len > 0.0 && w >= 0x1p-10 * rho;         // (NaN compares false)
                e[RAY_CENTRE] = c.x, e[RAY_CENTRE + 1] = c.y, e[RAY_CENTRE + 2] = c.z;
                const float r2 = (float)(2.25 * rr) * (1.f + 0x1p-18f);      // rounded up where it is normal; an overflow gives inf
                e[RAY_R2] = r2 >= 0x1p-100f ? r2 : INFINITY;                 // below that its rounding is absolute: never FAR
                e[RAY_NORMAL] = shaped ? (float)(n.x / len) : 0.f, e[RAY_NORMAL + 1] = shaped ? (float)(n.y / len) : 0.f;
                e[RAY_NORMAL + 2] = shaped ? (float)(n.z / len) : 0.f;
                e[RAY_K] = shaped ? (float)fmin(0x1p30 * rho * w, 0x1p127) : 0.f;   // clamped: never inf
            }
        }
        __syncthreads();
        if (!live) continue;
        for (int jj = 0; jj < nf; ++jj) {
            const float* e = tile + jj * WORDS;
            if (CULL) {
                const f3 m = {e[RAY_CENTRE] - o32.x, e[RAY_CENTRE + 1] - o32.y, e[RAY_CENTRE + 2] - o32.z};
                const float along = fmaf(m.z, u32.z, fmaf(m.y, u32.y, m.x * u32.x)), mm = fmaf(m.z, m.z, fmaf(m.y, m.y, m.x * m.x));
                const float steep = fabsf(fmaf(e[RAY_NORMAL + 2], u32.z, fmaf(e[RAY_NORMAL + 1], u32.y, e[RAY_NORMAL] * u32.x))) - 0x1p-16f;
                const bool far = (mm >= 0x1p-100f) & (fmaf(-along, along, mm) > fmaf(0x1p-18f, mm, e[RAY_R2]));
                if (far & (steep * e[RAY_K] > mm + e[RAY_R2])) continue;     // FAR and STEEP: proved not to cover (the head of this file)
            }
            const int i0 = __float_as_int(e[FACE_ID]), i1 = __float_as_int(e[FACE_ID + 1]), i2 = __float_as_int(e[FACE_ID + 2]);
            const d3 p0 = {(double)e[0] - o.x, (double)e[1] - o.y, (double)e[2] - o.z};
            const d3 p1 = {(double)e[3] - o.x, (double)e[4] - o.y, (double)e[5] - o.z};
            const d3 p2 = {(double)e[6] - o.x, (double)e[7] - o.y, (double)e[8] - o.z};
            double s0, s1, s2;
            int t0, t1, t2;
            ray_edge(i1, i2, p1, p2, d, s0, t0);
            ray_edge(i2, i0, p2, p0, d, s1, t1);
            ray_edge(i0, i1, p0, p1, d, s2, t2);
            if (!((t0 > 0 && t1 > 0 && t2 > 0) || (t0 < 0 && t1 < 0 && t2 < 0))) continue;
            const double c0 = dot_in_order(p0, d), c1 = dot_in_order(p1, d), c2 = dot_in_order(p2, d);
            const double t = ((s0 * c0 + s1 * c1) + s2 * c2) / (((s0 + s1) + s2) * dd);
            if (!(isfinite(t) && t > 0.0)) continue;
            ++hits;
            if (t < best) best = t, best_face = __float_as_int(e[RAY_FACE]);  // ascending face order: the lowest index among equal t
        }
    }
    if (r >= R) return;
    depth[at] = best_face >= 0 ? (float)best : INFINITY;
    face[at] = best_face;
    count[at] = hits;
}

// The backward at the forward's face choice, one thread per ray, in double and rounded once: with n = (v1 - v0) x (v2 - v0),
// nd = n . d, w_k = s_k / S and t as in the forward, G = ddepth n / nd, d/dv_k = w_k G, d/do = -G, d/dd = -t G.  The vertex part leaves
// as one VertexRecords entry (ids, (float)G, (float)w_k) for launch_vertex_scatter.  A ray whose face is outside [0, F), whose face has
// an id outside [0, V), whose nd is 0 or where any of these values is not finite contributes nothing: ids -1, exact zeros in its rows
// of dorg / ddir.  Nothing is read out of bounds whatever `face` holds.  dorg, ddir and rec.id are null where not wanted.
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_raycast_bwd_record(const float* __restrict__ org, const float* __restrict__ dir,
                                                                         const float* __restrict__ vts, const int32_t* __restrict__ faces,
                                                                         const int32_t* __restrict__ face, const float* __restrict__ ddepth,
                                                                         int R, int V, int F, float* __restrict__ dorg, float* __restrict__ ddir,
                                                                         VertexRecords rec) {
    const int b = blockIdx.y, r = blockIdx.x * MESH_BLOCK + threadIdx.x;
    if (r >= R) return;
    const size_t at = (size_t)b * R + r;
    const int f = face[at];
    int i0 = -1, i1 = -1, i2 = -1;
    d3 g = {0.0, 0.0, 0.0};
    double w0 = 0.0, w1 = 0.0, w2 = 0.0, t = 0.0;
    bool ok = f >= 0 && f < F;
    if (ok) {
        i0 = faces[(size_t)f * 3], i1 = faces[(size_t)f * 3 + 1], i2 = faces[(size_t)f * 3 + 2];
        ok = ids_ok(i0, i1, i2, V);
    }
    if (ok) {
        const float* v = vts + (size_t)b * V * 3;
        const d3 o = widened(org + at * 3), d = widened(dir + at * 3);
        const d3 v0 = widened(v + (size_t)i0 * 3), v1 = widened(v + (size_t)i1 * 3), v2 = widened(v + (size_t)i2 * 3);
        const d3 p0 = v0 - o, p1 = v1 - o, p2 = v2 - o;
        double s0, s1, s2;
        int t0, t1, t2;
        ray_edge(i1, i2, p1, p2, d, s0, t0);
        ray_edge(i2, i0, p2, p0, d, s1, t1);
        ray_edge(i0, i1, p0, p1, d, s2, t2);
        const double S = (s0 + s1) + s2, dd = dot_in_order(d, d);
        t = ((s0 * dot_in_order(p0, d) + s1 * dot_in_order(p1, d)) + s2 * dot_in_order(p2, d)) / (S * dd);
        const d3 n = dnormal(v1 - v0, v2 - v0);
        const double nd = dot_in_order(n, d), up = (double)ddepth[at];
        g = {up * n.x / nd, up * n.y / nd, up * n.z / nd};
        w0 = s0 / S, w1 = s1 / S, w2 = s2 / S;
        ok = nd != 0.0 && isfinite(t) && isfinite(g.x) && isfinite(g.y) && isfinite(g.z) && isfinite(w0) && isfinite(w1) && isfinite(w2) &&
             isfinite(t * g.x) && isfinite(t * g.y) && isfinite(t * g.z);
    }
    if (!ok) {
        i0 = i1 = i2 = -1;
        g = {0.0, 0.0, 0.0};
        w0 = w1 = w2 = t = 0.0;
    }
    if (rec.id) {
        rec.id[at] = make_int4(i0, i1, i2, -1);
        rec.gw[at] = make_float4((float)g.x, (float)g.y, (float)g.z, (float)w0);
        rec.w12[at] = make_float2((float)w1, (float)w2);
    }
    if (dorg) dorg[at * 3] = ok ? (float)-g.x : 0.f, dorg[at * 3 + 1] = ok ? (float)-g.y : 0.f, dorg[at * 3 + 2] = ok ? (float)-g.z : 0.f;
    if (ddir)
        ddir[at * 3] = ok ? (float)-(t * g.x) : 0.f, ddir[at * 3 + 1] = ok ? (float)-(t * g.y) : 0.f, ddir[at * 3 + 2] = ok ? (float)-(t * g.z) : 0.f;
}

}  // namespace

void launch_mesh_raycast(const float* org, const float* dir, const float* vts, const int32_t* faces, int B, int R, int V, int F, float* depth,
                         int32_t* face, int32_t* count, hipStream_t s) {
    const dim3 grid((unsigned)((R + MESH_BLOCK - 1) / MESH_BLOCK), B);
    prof_mark_begin(PROF_MESH_RAYCAST, 0.0, s);
#ifdef ICN_RAYCAST_NO_CULL                   // a timing build (tools/time_raycast.py): every tested face meets every live ray in double
    hipLaunchKernelGGL(k_mesh_raycast<false>, grid, dim3(MESH_BLOCK), 0, s, org, dir, vts, faces, R, V, F, depth, face, count);
#else
    hipLaunchKernelGGL(k_mesh_raycast<true>, grid, dim3(MESH_BLOCK), 0, s, org, dir, vts, faces, R, V, F, depth, face, count);
#endif
    prof_mark_end(s);
}

void launch_mesh_raycast_bwd(const float* org, const float* dir, const float* vts, const int32_t* faces, const int32_t* face,
                             const float* ddepth, int B, int R, int V, int F, float* dorg, float* ddir, float* dvts, void* ws, hipStream_t s) {
    VertexRecords rec = {nullptr, nullptr, nullptr};
    if (dvts) rec = vertex_records(ws, (size_t)B * R);
    prof_mark_begin(PROF_MESH_RAYCAST_BWD_RECORD, 0.0, s);
    hipLaunchKernelGGL(k_mesh_raycast_bwd_record, dim3((unsigned)((R + MESH_BLOCK - 1) / MESH_BLOCK), B), dim3(MESH_BLOCK), 0, s, org, dir,
                       vts, faces, face, ddepth, R, V, F, dorg, ddir, rec);
    prof_mark_end(s);
    if (dvts) launch_vertex_scatter(PROF_MESH_RAYCAST_BWD_VERTEX, ws, B, R, V, dvts, s);
}

}  // namespace icn
