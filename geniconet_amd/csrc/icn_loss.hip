// Point-to-point loss of the training step on the HIP path (reference losses.py:10-85 Point2Point_Loss; mesh helpers as
// restated in geniconet_amd/losses.py: vertex normals = area-weighted face-normal sums, generate.py:20-43; Laplacian =
// uniform umbrella mean(1-ring) - v by default -- upstream's mesh.utils.compute_laplacian is absent, so its sign and
// normalisation are a parameter: lap_mode bit 0 = opposite sign (v - mean), bit 1 = valence-weighted (sum(ring) - k v)).
// HBM/L2-bound, a few tens of microseconds; replaces ~25 torch launches per step.
//
//   v[b, i]   vertex i of sample b: the pixels of the network output (B, P, 3) and the two poles (vertex(), icn_mesh_device.h)
//   terms[0] = mean_{b,i,c} (v - t_pos)^2           terms[1] = mean_{b,i} (1 - cos(unit vertex normal, t_nor))
//   terms[2] = mean_{b,i,c} (lap(v) - t_lap)^2      terms[3] = f_pos * terms[0] + f_nor * terms[1] + f_lap * terms[2]
// target is (B, 9, V): rows 0:3 positions, 3:6 normals, 6:9 Laplacians (data.py:64-69).
// Sums are two-level with a fixed order (block_sum_store, then partials_sum in one block; deterministic).
//
// Backward (d terms[3] / d grid), all in gather form over the incident-face table, so no atomics and no write conflicts
// (derivation and finite-difference check: oracle/loss_ref.py p2p_grad):
//   position : 2 f_pos (v - t_pos) / (3 B V)
//   Laplacian: lap_i = c_i (mean(ring_i) - v_i), c_i = +-1 or +-k_i (lap_mode), e_i = lap_i - t_lap,i, k_i = valence:
//              2 f_lap (sum_{i in ring(j)} c_i e_i / k_i - c_j e_j) / (3 B V)                                    (ring symmetric)
//   normal   : w_i = sum of the face normals at i, u = w / |w|, c = u . t^ (t^ = t_nor / |t_nor|);
//              h_i = d(1 - c_i) / d w_i = -(t^ - (u . t^) u) / |w_i|;  face (j, p, q): d/d v_j = (h_j + h_p + h_q) x (v_q - v_p);
//              times f_nor / (B V).   Where a normalisation clamp is active (|w| <= 1e-10, |t_nor| <= 1e-8) h_i = 0.
//   vertex -> grid: store_pixel_grad (icn_mesh_device.h).
// k_p2p_bwd_prep stores c_i e_i / k_i and h_i per vertex (6 floats), k_p2p_bwd gathers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "icn_launch.h"
#include "icn_mesh_device.h"

namespace icn {

namespace {

constexpr int LOSS_BLOCK = MESH_BLOCK;

// factor c_i of the Laplacian convention: lap_i = c_i (mean(ring_i) - v_i)
__device__ __forceinline__ float lap_factor(int lap_mode, int k) {
    const float w = (lap_mode & 2) ? (float)k : 1.f;
    return (lap_mode & 1) ? -w : w;
}

// the fan of vertex i (position v) over the incident-face table vf[(i * 6 + f) * 2] = (p, q), p < 0: no face in slot f
struct VertexFan {
    f3 w, ring;                     // sum of the face normals (p - v) x (q - v), sum of the ring vertices p
    int k;                          // valence
};
__device__ __forceinline__ VertexFan p2p_vertex_fan(const float* __restrict__ g, const int32_t* __restrict__ vf, int b, int i, f3 v,
                                                    int P, int n) {
    VertexFan fan = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}, 0};
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int p = vf[((size_t)i * 6 + f) * 2], q = vf[((size_t)i * 6 + f) * 2 + 1];
        if (p < 0) continue;
        const f3 vp = vertex(g, b, p, P, n), vq = vertex(g, b, q, P, n);
        fan.w = fan.w + cross(vp - v, vq - v);
        fan.ring = fan.ring + vp;
        ++fan.k;
    }
    return fan;
}

// lap_i = c_i (mean(ring_i) - v_i)
__device__ __forceinline__ f3 p2p_laplacian(const VertexFan& fan, f3 v, int lap_mode) {
    const float inv = 1.f / (float)fan.k, cf = lap_factor(lap_mode, fan.k);
    const f3 um = f3{fan.ring.x * inv, fan.ring.y * inv, fan.ring.z * inv} - v;
    return {cf * um.x, cf * um.y, cf * um.z};
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_p2p_fwd(const float* __restrict__ g, const float* __restrict__ target,
                                                         const int32_t* __restrict__ vf, float* __restrict__ partial, int B, int P,
                                                         int n, int lap_mode) {
    const int V = P + 2;
    const long idx = (long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    float e[3] = {0.f, 0.f, 0.f};                                        // position, normal, Laplacian
    if (idx < (long)B * V) {
        const int b = (int)(idx / V), i = (int)(idx % V);
        const f3 v = vertex(g, b, i, P, n);
        const float* t = target + (size_t)b * 9 * V + i;                 // component c at t[c * V]
        const f3 tp = {t[0], t[(size_t)V], t[(size_t)2 * V]};
        const f3 tn = {t[(size_t)3 * V], t[(size_t)4 * V], t[(size_t)5 * V]};
        const f3 tl = {t[(size_t)6 * V], t[(size_t)7 * V], t[(size_t)8 * V]};
        const f3 d = v - tp;
        e[0] = dot(d, d);
        const VertexFan fan = p2p_vertex_fan(g, vf, b, i, v, P, n);
        const f3 vn = fan.w;
        const float len = fmaxf(sqrtf(dot(vn, vn)), 1e-10f);              // losses.py helper: vn / clamp_min(|vn|, eps)
        const f3 u = {vn.x / len, vn.y / len, vn.z / len};
        // F.cosine_similarity(u, tn, eps = 1e-8): each norm clamped separately
        const float cs = dot(u, tn) / (fmaxf(sqrtf(dot(u, u)), 1e-8f) * fmaxf(sqrtf(dot(tn, tn)), 1e-8f));
        e[1] = 1.f - cs;
        const f3 dl = p2p_laplacian(fan, v, lap_mode) - tl;
        e[2] = dot(dl, dl);
    }
    block_sum_store(e, partial + (size_t)blockIdx.x * 3);
}

// terms from the per-block partials, one block
// (also the finalize of the mesh regularisers below: count0 / count1 / count2 divide the three sums)
__global__ __launch_bounds__(LOSS_BLOCK) void k_p2p_finalize(const float* __restrict__ partial, int nblocks, double count0,
                                                              double count1, double count2, float f_pos, float f_nor, float f_lap,
                                                              float* __restrict__ terms) {
    double s[3];
    partials_sum(partial, nblocks, s);
    if (threadIdx.x == 0) {
        const float l_pos = (float)(s[0] / count0), l_nor = (float)(s[1] / count1), l_lap = (float)(s[2] / count2);
        terms[0] = l_pos;
        terms[1] = l_nor;
        terms[2] = l_lap;
        terms[3] = fmaf(f_lap, l_lap, fmaf(f_pos, l_pos, f_nor * l_nor));     // spelled out: the bits must not depend on which products
                                                                              // the compiler chooses to contract
    }
}

// d(f_pos * terms[0]) / d(grid) * upstream, the per-vertex term 2 (v - t_pos) / (B V 3) with its constant factor applied last
__global__ __launch_bounds__(LOSS_BLOCK) void k_p2p_bwd_pos(const float* __restrict__ g, const float* __restrict__ target,
                                                             const float* __restrict__ upstream, float scale,
                                                             float* __restrict__ dg, int B, int P, int n) {
    const int V = P + 2;
    const long idx = (long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (idx >= (long)B * P) return;
    const int b = (int)(idx / P), j = (int)(idx % P);
    const float* t = target + (size_t)b * 9 * V;
    store_pixel_grad(dg, b, j, P, n, scale * upstream[0], [&](int x) {
        return vertex(g, b, x, P, n) - f3{t[x], t[(size_t)V + x], t[(size_t)2 * V + x]};
    });
}

// per vertex: aux[0:3] = (lap - t_lap) / k,  aux[3:6] = h = d(1 - cos) / d w  (see the header comment)
__global__ __launch_bounds__(LOSS_BLOCK) void k_p2p_bwd_prep(const float* __restrict__ g, const float* __restrict__ target,
                                                              const int32_t* __restrict__ vf, float* __restrict__ aux, int B, int P,
                                                              int n, int lap_mode) {
    const int V = P + 2;
    const long idx = (long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (idx >= (long)B * V) return;
    const int b = (int)(idx / V), i = (int)(idx % V);
    const f3 v = vertex(g, b, i, P, n);
    const float* t = target + (size_t)b * 9 * V + i;
    const f3 tn = {t[(size_t)3 * V], t[(size_t)4 * V], t[(size_t)5 * V]};
    const f3 tl = {t[(size_t)6 * V], t[(size_t)7 * V], t[(size_t)8 * V]};
    const VertexFan fan = p2p_vertex_fan(g, vf, b, i, v, P, n);
    const f3 w = fan.w, e = p2p_laplacian(fan, v, lap_mode) - tl;
    f3 h = {0.f, 0.f, 0.f};
    const float wl = sqrtf(dot(w, w)), tl2 = sqrtf(dot(tn, tn));
    if (wl > 1e-10f && tl2 > 1e-8f) {
        const f3 u = {w.x / wl, w.y / wl, w.z / wl}, th = {tn.x / tl2, tn.y / tl2, tn.z / tl2};
        const float c = dot(u, th);
        h = {-(th.x - c * u.x) / wl, -(th.y - c * u.y) / wl, -(th.z - c * u.z) / wl};
    }
    float* a = aux + (size_t)idx * 6;
    const float ci = lap_factor(lap_mode, fan.k) * (1.f / (float)fan.k);
    a[0] = e.x * ci; a[1] = e.y * ci; a[2] = e.z * ci;
    a[3] = h.x; a[4] = h.y; a[5] = h.z;
}

__device__ __forceinline__ f3 aux3(const float* __restrict__ aux, int b, int x, int V, int off) {
    const float* a = aux + ((size_t)b * V + x) * 6 + off;
    return {a[0], a[1], a[2]};
}

// gradient of the weighted loss with respect to vertex x of sample b (cp, cl, cn: the three terms' constant factors)
__device__ __forceinline__ f3 vertex_grad(const float* __restrict__ g, const float* __restrict__ target,
                                          const int32_t* __restrict__ vf, const float* __restrict__ aux, int b, int x, int P, int n,
                                          float cp, float cl, float cn) {
    const int V = P + 2;
    const f3 v = vertex(g, b, x, P, n);
    const float* t = target + (size_t)b * 9 * V + x;
    f3 d = {cp * (v.x - t[0]), cp * (v.y - t[(size_t)V]), cp * (v.z - t[(size_t)2 * V])};
    const f3 ex = aux3(aux, b, x, V, 0), hx = aux3(aux, b, x, V, 3);
    f3 gl = {0.f, 0.f, 0.f}, gn = {0.f, 0.f, 0.f};
    int k = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int p = vf[((size_t)x * 6 + f) * 2], q = vf[((size_t)x * 6 + f) * 2 + 1];
        if (p < 0) continue;
        gl = gl + aux3(aux, b, p, V, 0);
        const f3 G = hx + aux3(aux, b, p, V, 3) + aux3(aux, b, q, V, 3);
        gn = gn + cross(G, vertex(g, b, q, P, n) - vertex(g, b, p, P, n));
        ++k;
    }
    const float kf = (float)k;
    d = d + f3{cl * (gl.x - kf * ex.x), cl * (gl.y - kf * ex.y), cl * (gl.z - kf * ex.z)};
    return d + f3{cn * gn.x, cn * gn.y, cn * gn.z};
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_p2p_bwd(const float* __restrict__ g, const float* __restrict__ target,
                                                         const int32_t* __restrict__ vf, const float* __restrict__ aux,
                                                         const float* __restrict__ upstream, float cp, float cl, float cn,
                                                         float* __restrict__ dg, int B, int P, int n) {
    const long idx = (long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (idx >= (long)B * P) return;
    const int b = (int)(idx / P), j = (int)(idx % P);
    store_pixel_grad(dg, b, j, P, n, upstream[0], [&](int x) { return vertex_grad(g, target, vf, aux, b, x, P, n, cp, cl, cn); });
}

}  // namespace

int p2p_loss_blocks(int B, int P) { return (int)(((long)B * (P + 2) + LOSS_BLOCK - 1) / LOSS_BLOCK); }

void launch_p2p_loss_fwd(const float* grid, const float* target, const int32_t* vf, float* partial, float* terms, int B, int P, int n,
                         float f_pos, float f_nor, float f_lap, int lap_mode, hipStream_t s) {
    const int nb = p2p_loss_blocks(B, P);
    hipLaunchKernelGGL(k_p2p_fwd, dim3(nb), dim3(LOSS_BLOCK), 0, s, grid, target, vf, partial, B, P, n, lap_mode);
    const double nv = (double)B * (P + 2);
    hipLaunchKernelGGL(k_p2p_finalize, dim3(1), dim3(LOSS_BLOCK), 0, s, partial, nb, nv * 3.0, nv, nv * 3.0, f_pos, f_nor,
                       f_lap, terms);
}

void launch_p2p_loss_bwd_pos(const float* grid, const float* target, const float* upstream, float f_pos, float* dgrid, int B, int P,
                             int n, hipStream_t s) {
    const long total = (long)B * P;
    const float scale = (float)(2.0 * (double)f_pos / ((double)B * (P + 2) * 3.0));
    hipLaunchKernelGGL(k_p2p_bwd_pos, dim3((unsigned)((total + LOSS_BLOCK - 1) / LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, s, grid, target,
                       upstream, scale, dgrid, B, P, n);
}

void launch_p2p_loss_bwd(const float* grid, const float* target, const int32_t* vf, const float* upstream, float f_pos, float f_nor,
                         float f_lap, int lap_mode, float* dgrid, float* aux, int B, int P, int n, hipStream_t s) {
    if (f_nor == 0.f && f_lap == 0.f) return launch_p2p_loss_bwd_pos(grid, target, upstream, f_pos, dgrid, B, P, n, s);
    const double nv = (double)B * (P + 2);
    const long tv = (long)B * (P + 2), tp = (long)B * P;
    hipLaunchKernelGGL(k_p2p_bwd_prep, dim3((unsigned)((tv + LOSS_BLOCK - 1) / LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, s, grid, target, vf, aux,
                       B, P, n, lap_mode);
    hipLaunchKernelGGL(k_p2p_bwd, dim3((unsigned)((tp + LOSS_BLOCK - 1) / LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, s, grid, target, vf, aux,
                       upstream, (float)(2.0 * f_pos / (3.0 * nv)), (float)(2.0 * f_lap / (3.0 * nv)), (float)(f_nor / nv), dgrid, B, P, n);
}

// ---------------------------------------------------------------------------------------------------------
// Mesh regularisers of the surface loss (not in the reference): edge length, normal consistency between adjacent faces, uniform
// Laplacian smoothness, on the static icosahedral topology.  Same input as the point-to-point loss above (grid (B, P, 3), V = P + 2
// vertices through vertex()); E = 3 P undirected edges.  Topology: the edge stencil table of icn_geometry.h, vs[(i * 6 + f) * 3] =
// (p, q, x) in cyclic order around i -- the kernels read p and x, q of slot f is p of slot f + 1.
//   terms[0] = T_e = 1 / (B E)   sum_b sum_edges (|v_i - v_j| - L)^2          (L = 0: |v_i - v_j|^2, no square root)
//   terms[1] = T_n = 1 / (B E)   sum_b sum_edges 1/2 |n^_F0 - n^_F1|^2        n_F = (v_b - v_a) x (v_c - v_a), n^ = n / max(|n|, 1e-12)
//   terms[2] = T_s = 1 / (3 B V) sum_b sum_i |mean(ring_i) - v_i|^2           terms[3] = f_edge T_e + f_ncons T_n + f_smooth T_s
// Forward, one thread per (sample, vertex i): every edge at i is a spoke (i, p_f) with the faces of slots f and f - 1 on its sides, and
// every edge of the mesh is a spoke of both of its ends, so each thread adds HALF of its spokes' edge and normal terms: the 1-ring is
// all it reads.  Sums as above: fixed tree per block, then one block in double.
//
// Backward (d terms[3] / d grid), gather form, one thread per (sample, pixel j); with d = v_j - v_p over the ring of j:
//   edge   : 2 f_edge / (B E) sum_p (1 - L / |d|) d;  L = 0: 2 d;  L > 0 and |d|^2 <= 1e-24: that edge adds nothing
//   smooth : u_i = mean(ring_i) - v_i:  2 f_smooth / (3 B V) (sum_{i in ring(j)} u_i / k_i - u_j)   (ring symmetric; k = valence).
//            u_i / k_i of a neighbour needs the neighbour's own ring, so k_mreg_bwd_prep stores it per vertex (3 floats) first.
//   normal : S = sum_edges 1/2 |n^_F - n^_G|^2.  For a face F with neighbours G1..G3 across its edges, g_F = dS / dn^_F = sum_G (n^_F - n^_G),
//            H_F = dS / dn_F = (g_F - (g_F . n^_F) n^_F) / |n_F|, or 0 where the clamp is active (|n_F| <= 1e-12; a clamped face still
//            enters its neighbours' g as the constant n_F / 1e-12).  With n_F = (v_p - v_j) x (v_q - v_j), dS / dv_j = sum over the faces
//            (j, p, q) at j of H_F x (v_q - v_p); times f_ncons / (B E).  RECOMPUTED per vertex, no workspace: the neighbours of the face in
//            slot f are slots f - 1 and f + 1 and, across (p_f, q_f), the face (q_f, p_f, x_f) -- the 1-ring and the six x suffice.
//   vertex -> grid as above (store_pixel_grad).
// A term whose factor is 0 is skipped in the backward (no loads of x without the normal term, no prep pass without smoothness).
// ---------------------------------------------------------------------------------------------------------
namespace {

constexpr float MREG_EPS = 1e-12f;

// n / max(|n|, 1e-12); len = |n|
__device__ __forceinline__ f3 unit_clamped(f3 nrm, float& len) {
    len = sqrtf(dot(nrm, nrm));
    return scaled(nrm, 1.f / fmaxf(len, MREG_EPS));
}

// v, the ring p_0 .. p_{k-1} of vertex i (slots beyond the valence hold v) and the valence
__device__ __forceinline__ int load_ring(const float* __restrict__ g, const int32_t* __restrict__ vs, int b, int i, int P, int n, f3& v,
                                         f3 (&pv)[6]) {
    v = vertex(g, b, i, P, n);
    int k = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        const int p = vs[((size_t)i * 6 + f) * 3];
        pv[f] = v;
        if (p >= 0) { pv[f] = vertex(g, b, p, P, n); ++k; }
    }
    return k;
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_mreg_fwd(const float* __restrict__ g, const int32_t* __restrict__ vs,
                                                          float* __restrict__ partial, int B, int P, int n, float L) {
    const int V = P + 2;
    const long idx = (long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    float e_edge = 0.f, e_nc = 0.f, e_sm = 0.f;
    if (idx < (long)B * V) {
        const int b = (int)(idx / V), i = (int)(idx % V);
        f3 v, pv[6], nh[6];
        const int k = load_ring(g, vs, b, i, P, n, v, pv);
        f3 ring = {0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            nh[f] = {0.f, 0.f, 0.f};
            if (f >= k) continue;
            const f3 d = pv[f] - v;
            const float d2 = dot(d, d);
            if (L > 0.f) { const float t = (d2 > MREG_EPS * MREG_EPS ? sqrtf(d2) : 0.f) - L; e_edge += t * t; }
            else e_edge += d2;
            ring = ring + pv[f];
            const f3 q = (f + 1 < k) ? pv[(f + 1) % 6] : pv[0];
            float len;
            nh[f] = unit_clamped(face_normal(d, q - v), len);
        }
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            if (f >= k) continue;
            const f3 prev = f > 0 ? nh[(f + 5) % 6] : (k == 6 ? nh[5] : nh[4]);
            const f3 dn = nh[f] - prev;
            e_nc += dot(dn, dn);
        }
        e_edge *= 0.5f;                                                      // each edge from both of its ends
        e_nc *= 0.25f;                                                       // ... and 1/2 |n^ - n^|^2
        const f3 u = scaled(ring, 1.f / (float)k) - v;
        e_sm = dot(u, u);
    }
    float e[3] = {e_edge, e_nc, e_sm};
    block_sum_store(e, partial + (size_t)blockIdx.x * 3);
}

// aux[(b V + i) * 3 ..] = (mean(ring_i) - v_i) / k_i
__global__ __launch_bounds__(LOSS_BLOCK) void k_mreg_bwd_prep(const float* __restrict__ g, const int32_t* __restrict__ vs,
                                                               float* __restrict__ aux, int B, int P, int n) {
    const int V = P + 2;
    const long idx = (long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (idx >= (long)B * V) return;
    const int b = (int)(idx / V), i = (int)(idx % V);
    f3 v, pv[6];
    const int k = load_ring(g, vs, b, i, P, n, v, pv);
    f3 ring = {0.f, 0.f, 0.f};
#pragma unroll
    for (int f = 0; f < 6; ++f)
        if (f < k) ring = ring + pv[f];
    const float inv = 1.f / (float)k;
    const f3 a = scaled(scaled(ring, inv) - v, inv);
    float* o = aux + (size_t)idx * 3;
    o[0] = a.x; o[1] = a.y; o[2] = a.z;
}

// gradient of the weighted sum with respect to vertex j of sample b (ce, cn, cs: the three terms' constant factors, see the launcher)
__device__ __forceinline__ f3 mreg_vertex_grad(const float* __restrict__ g, const int32_t* __restrict__ vs,
                                               const float* __restrict__ aux, int b, int j, int P, int n, float ce, float L, float cn,
                                               float cs) {
    const int V = P + 2;
    f3 v, pv[6];
    const int k = load_ring(g, vs, b, j, P, n, v, pv);
    f3 out = {0.f, 0.f, 0.f};
    if (ce != 0.f) {
        f3 ge = {0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            if (f >= k) continue;
            const f3 d = v - pv[f];
            if (L > 0.f) {
                const float d2 = dot(d, d);
                if (d2 > MREG_EPS * MREG_EPS) ge = ge + scaled(d, 1.f - L / sqrtf(d2));
            } else {
                ge = ge + d;
            }
        }
        out = out + scaled(ge, ce);
    }
    if (cs != 0.f) {
        f3 gs = {0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            const int p = vs[((size_t)j * 6 + f) * 3];
            if (p < 0) continue;
            const float* a = aux + ((size_t)b * V + p) * 3;
            gs = gs + f3{a[0], a[1], a[2]};
        }
        const float* a = aux + ((size_t)b * V + j) * 3;
        const float kf = (float)k;
        out = out + scaled(gs - f3{kf * a[0], kf * a[1], kf * a[2]}, cs);
    }
    if (cn != 0.f) {
        f3 nh[6], mh[6];
        float nl[6];
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            nh[f] = mh[f] = {0.f, 0.f, 0.f};
            nl[f] = 0.f;
            if (f >= k) continue;
            const f3 q = (f + 1 < k) ? pv[(f + 1) % 6] : pv[0];
            nh[f] = unit_clamped(face_normal(pv[f] - v, q - v), nl[f]);
            const f3 xv = vertex(g, b, vs[((size_t)j * 6 + f) * 3 + 2], P, n);
            float ml;
            mh[f] = unit_clamped(face_normal(pv[f] - q, xv - q), ml);      // face (q, p, x)
        }
        f3 gn = {0.f, 0.f, 0.f};
#pragma unroll
        for (int f = 0; f < 6; ++f) {
            if (f >= k || !(nl[f] > MREG_EPS)) continue;
            const f3 prev = f > 0 ? nh[(f + 5) % 6] : (k == 6 ? nh[5] : nh[4]);
            const f3 next = (f + 1 < k) ? nh[(f + 1) % 6] : nh[0];
            const f3 q = (f + 1 < k) ? pv[(f + 1) % 6] : pv[0];
            const f3 gf = scaled(nh[f], 3.f) - prev - next - mh[f];
            const f3 H = scaled(gf - scaled(nh[f], dot(gf, nh[f])), 1.f / nl[f]);
            gn = gn + cross(H, q - pv[f]);
        }
        out = out + scaled(gn, cn);
    }
    return out;
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_mreg_bwd(const float* __restrict__ g, const int32_t* __restrict__ vs,
                                                          const float* __restrict__ aux, const float* __restrict__ upstream, float ce,
                                                          float L, float cn, float cs, float* __restrict__ dg, int B, int P, int n) {
    const long idx = (long)blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (idx >= (long)B * P) return;
    const int b = (int)(idx / P), j = (int)(idx % P);
    store_pixel_grad(dg, b, j, P, n, upstream[0], [&](int x) { return mreg_vertex_grad(g, vs, aux, b, x, P, n, ce, L, cn, cs); });
}

}  // namespace

void launch_mesh_reg_fwd(const float* grid, const int32_t* vs, float* partial, float* terms, int B, int P, int n, float f_edge,
                         float f_ncons, float f_smooth, float edge_length, hipStream_t s) {
    const int nb = p2p_loss_blocks(B, P);
    hipLaunchKernelGGL(k_mreg_fwd, dim3(nb), dim3(LOSS_BLOCK), 0, s, grid, vs, partial, B, P, n, edge_length);
    const double ne = (double)B * 3.0 * P, nv = (double)B * (P + 2);
    hipLaunchKernelGGL(k_p2p_finalize, dim3(1), dim3(LOSS_BLOCK), 0, s, partial, nb, ne, ne, nv * 3.0, f_edge, f_ncons, f_smooth, terms);
}

void launch_mesh_reg_bwd(const float* grid, const int32_t* vs, const float* upstream, float f_edge, float f_ncons, float f_smooth,
                         float edge_length, float* dgrid, float* aux, int B, int P, int n, hipStream_t s) {
    const double ne = (double)B * 3.0 * P, nv = (double)B * (P + 2);
    const long tv = (long)B * (P + 2), tp = (long)B * P;
    if (f_smooth != 0.f)
        hipLaunchKernelGGL(k_mreg_bwd_prep, dim3((unsigned)((tv + LOSS_BLOCK - 1) / LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, s, grid, vs, aux, B,
                           P, n);
    hipLaunchKernelGGL(k_mreg_bwd, dim3((unsigned)((tp + LOSS_BLOCK - 1) / LOSS_BLOCK)), dim3(LOSS_BLOCK), 0, s, grid, vs, aux, upstream,
                       (float)(2.0 * f_edge / ne), edge_length, (float)(f_ncons / ne), (float)(2.0 * f_smooth / (3.0 * nv)), dgrid, B, P, n);
}

// ---------------------------------------------------------------------------------------------------------
// KL term of the VAE loss (reference losses.py:105) and the reparameterisation (models.py:89-92): elementwise over the
// n = B * D latent values; the sum is two-level with a fixed tree (deterministic).
// ---------------------------------------------------------------------------------------------------------
constexpr int KLD_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(LOSS_BLOCK) void k_kld_partial(const float* __restrict__ mu, const float* __restrict__ lv, size_t n,
                                                             float* __restrict__ partial) {
    float s[1] = {0.f};
    for (size_t i = (size_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * LOSS_BLOCK) {
        const float m = mu[i], l = lv[i];
        s[0] += 1.f + l - m * m - __expf(l);
    }
    block_sum_store(s, partial + blockIdx.x);
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_kld_finalize(const float* __restrict__ partial, int nblocks, double scale,
                                                              float* __restrict__ out) {
    double s[1];
    partials_sum(partial, nblocks, s);
    if (threadIdx.x == 0) out[0] = (float)(s[0] * scale);
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_kld_bwd(const float* __restrict__ mu, const float* __restrict__ lv,
                                                         const float* __restrict__ upstream, float inv_n, size_t n,
                                                         float* __restrict__ dmu, float* __restrict__ dlv) {
    const float w = upstream[0] * inv_n;
    for (size_t i = (size_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * LOSS_BLOCK) {
        dmu[i] = w * mu[i];
        dlv[i] = 0.5f * w * (__expf(lv[i]) - 1.f);
    }
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_reparam_fwd(const float* __restrict__ mu, const float* __restrict__ lv,
                                                             const float* __restrict__ eps, size_t n, float* __restrict__ z) {
    for (size_t i = (size_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * LOSS_BLOCK)
        z[i] = eps[i] * __expf(0.5f * lv[i]) + mu[i];
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_reparam_bwd(const float* __restrict__ dz, const float* __restrict__ lv,
                                                             const float* __restrict__ eps, size_t n, float* __restrict__ dmu,
                                                             float* __restrict__ dlv) {
    for (size_t i = (size_t)blockIdx.x * LOSS_BLOCK + threadIdx.x; i < n; i += (size_t)gridDim.x * LOSS_BLOCK) {
        const float g = dz[i];
        dmu[i] = g;
        dlv[i] = g * eps[i] * 0.5f * __expf(0.5f * lv[i]);
    }
}

static int ew_blocks(size_t n) { return (int)std::min((size_t)KLD_MAX_BLOCKS, (n + LOSS_BLOCK - 1) / LOSS_BLOCK); }

int kld_blocks(size_t n) { return ew_blocks(n); }

void launch_kld_fwd(const float* mu, const float* logvar, size_t n, float* out, float* partial, hipStream_t s) {
    const int nb = ew_blocks(n);
    hipLaunchKernelGGL(k_kld_partial, dim3(nb), dim3(LOSS_BLOCK), 0, s, mu, logvar, n, partial);
    hipLaunchKernelGGL(k_kld_finalize, dim3(1), dim3(LOSS_BLOCK), 0, s, partial, nb, -0.5 / (double)n, out);
}

void launch_kld_bwd(const float* mu, const float* logvar, const float* upstream, size_t n, float* dmu, float* dlogvar, hipStream_t s) {
    hipLaunchKernelGGL(k_kld_bwd, dim3(ew_blocks(n)), dim3(LOSS_BLOCK), 0, s, mu, logvar, upstream, (float)(1.0 / (double)n), n, dmu,
                       dlogvar);
}

void launch_reparam_fwd(const float* mu, const float* logvar, const float* eps, size_t n, float* z, hipStream_t s) {
    hipLaunchKernelGGL(k_reparam_fwd, dim3(ew_blocks(n)), dim3(LOSS_BLOCK), 0, s, mu, logvar, eps, n, z);
}

void launch_reparam_bwd(const float* dz, const float* logvar, const float* eps, size_t n, float* dmu, float* dlogvar, hipStream_t s) {
    hipLaunchKernelGGL(k_reparam_bwd, dim3(ew_blocks(n)), dim3(LOSS_BLOCK), 0, s, dz, logvar, eps, n, dmu, dlogvar);
}

// ---------------------------------------------------------------------------------------------------------
// Test-time metric of the reference (ico_utils.py:26-44, mode 'point2mesh'; upstream: kaolin 0.9.1's CUDA extension):
// squared distance of every point to the closest point of a triangle mesh.  One thread per point; the triangles of the
// point's sample go through LDS in tiles of 256 (each thread stages one triangle's three vertices), so every vertex is
// fetched once per block.  Region classification of Ericson, Real-Time Collision Detection 5.1.5; ties keep the lowest face.
// kind: 0 interior, 1 / 2 / 3 vertex 0 / 1 / 2, 4 / 5 / 6 edge (0,1) / (1,2) / (2,0).
// ---------------------------------------------------------------------------------------------------------
namespace {

// Accuracy.  The three edge functions of the region tests are taken from the normal n = ab x ac (vc = ab . (ap x n),
// vb = -ac . (ap x n), va = |n|^2 - vb - vc) and the interior distance from the plane, (ap . n)^2 / |n|^2; d3 .. d6 follow from
// d1, d2 and the triangle's Gram matrix.  n carries a relative error of about u / sin(angle at vertex 0), and every boundary
// between regions and the plane inherit it once: the error of the distance grows with the FIRST power of the aspect ratio
// (differences of products of dot products, as in the textbook form, lose its square).  Where n cannot be resolved,
// |n|^2 2^22 <= |ab|^2 |ac|^2 (sine below 1 / 2048: every coincident or collinear triangle, and slivers of aspect ratio above
// 2048 seen from a sharp corner), the triangle is the union of its three edge segments: the nearest of three clamped projections,
// at most the sliver's inradius from the true distance, never kind 0.  The test depends on the triangle alone, so it is uniform
// across a wave of the brute-force kernel.  Edge lengths are expected within about [1e-9, 3e9] (|ab|^2 |ac|^2 is an fp32 product).
// A triangle with a non-finite vertex returns NaN (never selected), a non-finite point NaN or infinity.
constexpr float TRI_FLAT = 4194304.f;        // 2^22

// p - q for q the clamped projection of p on the segment u + t uw, given up = p - u; a zero-length segment is its point
__device__ __forceinline__ f3 seg_diff(f3 up, f3 uw, float& t) {
    const float den = dot(uw, uw);
    t = den != 0.f ? dot(uw, up) / den : 0.f;
    t = !(t > 0.f) ? 0.f : (t < 1.f ? t : 1.f);
    return f3{up.x - uw.x * t, up.y - uw.y * t, up.z - uw.z * t};
}

__device__ __forceinline__ float tri_dist2(f3 p, f3 a, f3 b, f3 c, int& kind) {
    const f3 ab = b - a, ac = c - a, ap = p - a;
    const float lab = dot(ab, ab), lac = dot(ac, ac);
    const f3 n = cross(ab, ac);
    const float nn = dot(n, n);
    if (!(nn * TRI_FLAT > lab * lac)) {
        kind = 0;
        if (!(lab + lac <= 3.0e38f)) return __int_as_float(0x7fc00000);
        // Nearest of the three clamped projections.  A projection clamped to a vertex is dropped where the other segment through
        // that vertex projects inside itself: that one is nearer, by an amount that |p - q|^2 may be too coarse to show.
        float t0, t1, t2;
        const f3 e0 = seg_diff(ap, ab, t0), e1 = seg_diff(p - b, c - b, t1), e2 = seg_diff(ap, ac, t2);
        const bool in0 = t0 > 0.f && t0 < 1.f, in1 = t1 > 0.f && t1 < 1.f, in2 = t2 > 0.f && t2 < 1.f;
        const bool drop0 = t0 <= 0.f ? in2 : (t0 >= 1.f && in1), drop1 = t1 <= 0.f ? in0 : (t1 >= 1.f && in2),
                   drop2 = t2 <= 0.f ? in0 : (t2 >= 1.f && in1);
        float best = 3.4e38f;
        const float s0 = dot(e0, e0), s1 = dot(e1, e1), s2 = dot(e2, e2);
        if (!drop0) { best = s0; kind = t0 <= 0.f ? 1 : (t0 >= 1.f ? 2 : 4); }
        if (!drop1 && !(s1 >= best)) { best = s1; kind = t1 <= 0.f ? 2 : (t1 >= 1.f ? 3 : 5); }
        if (!drop2 && !(s2 >= best)) { best = s2; kind = t2 <= 0.f ? 1 : (t2 >= 1.f ? 3 : 6); }
        return best;
    }
    const float g = dot(ab, ac), d1 = dot(ab, ap), d2 = dot(ac, ap);
    f3 d;
    if (d1 <= 0.f && d2 <= 0.f) { kind = 1; d = ap; }
    else {
        const float d3 = d1 - lab, d4 = d2 - g;
        if (d3 >= 0.f && d4 <= d3) { kind = 2; d = p - b; }
        else {
            const float d5 = d1 - g, d6 = d2 - lac;
            if (d6 >= 0.f && d5 <= d6) { kind = 3; d = p - c; }
            else {
                const f3 r = cross(ap, n);
                const float vc = dot(ab, r), vb = -dot(ac, r), va = nn - vb - vc;
                if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                 // 0 <= d1 <= lab, lab > 0: t in [0, 1]
                    const float t = d1 / lab;
                    kind = 4; d = f3{ap.x - ab.x * t, ap.y - ab.y * t, ap.z - ab.z * t};
                } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
                    const float t = d2 / lac;
                    kind = 6; d = f3{ap.x - ac.x * t, ap.y - ac.y * t, ap.z - ac.z * t};
                } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
                    float t;
                    kind = 5; d = seg_diff(p - b, c - b, t);
                } else {
                    const float s = dot(ap, n) / nn;
                    kind = 0; d = f3{n.x * s, n.y * s, n.z * s};
                }
            }
        }
    }
    return dot(d, d);
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_point_to_mesh(const float* __restrict__ pts, const float* __restrict__ vts,
                                                               const int32_t* __restrict__ faces, int P, int V, int F,
                                                               float* __restrict__ dist, int32_t* __restrict__ face,
                                                               int32_t* __restrict__ kind) {
    __shared__ float tri[LOSS_BLOCK][9];
    const int b = blockIdx.y, i = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    const bool live = i < P;
    f3 p = {0.f, 0.f, 0.f};
    if (live) { const float* q = pts + ((size_t)b * P + i) * 3; p = {q[0], q[1], q[2]}; }
    float best = 3.4e38f;
    int best_f = 0, best_k = 0;
    for (int f0 = 0; f0 < F; f0 += LOSS_BLOCK) {
        __syncthreads();
        const int f = f0 + threadIdx.x;
        if (f < F) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int v = faces[(size_t)f * 3 + k];
                const float* q = vts + ((size_t)b * V + v) * 3;
                tri[threadIdx.x][3 * k] = q[0]; tri[threadIdx.x][3 * k + 1] = q[1]; tri[threadIdx.x][3 * k + 2] = q[2];
            }
        }
        __syncthreads();
        const int nf = min(LOSS_BLOCK, F - f0);
        if (live)
            for (int j = 0; j < nf; ++j) {
                int k;
                const float d2 = tri_dist2(p, f3{tri[j][0], tri[j][1], tri[j][2]}, f3{tri[j][3], tri[j][4], tri[j][5]},
                                           f3{tri[j][6], tri[j][7], tri[j][8]}, k);
                if (d2 < best) { best = d2; best_f = f0 + j; best_k = k; }
            }
    }
    if (live) {
        dist[(size_t)b * P + i] = best;
        face[(size_t)b * P + i] = best_f;
        kind[(size_t)b * P + i] = best_k;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Backward of the distance above.  With q = wa a + wb b + wc c the closest point of p on its selected triangle (a, b, c),
// p - q is orthogonal to the feature q lies on, so the derivative through the weights vanishes:
//     d dist / d p = 2 (p - q)        d dist / d a = -2 wa (p - q)   (likewise b, c)
// No second search: p - q and the weights are recomputed from the forward's (face, kind) with the expressions of tri_dist2: an edge
// kind is the clamped projection on that segment (a zero-length edge is its point, weight 1 on its first vertex), kind 0 the plane.
//   k_point_to_mesh_bwd_point   one thread per point: g = 2 ddist (p - q) -> dpoints; a VertexRecords entry (icn_mesh_device.h: the
//                               three vertex ids, -g, the three weights; id -1 where the weight is zero by construction) -> workspace
//   launch_vertex_scatter       (icn_sample.hip) the records -> dvertices, summed per vertex in point order without atomics
// A face index outside [0, F), a kind outside [0, 6] or a vertex id outside [0, V) gives that point a zero gradient (nothing
// is read out of bounds).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LOSS_BLOCK) void k_point_to_mesh_bwd_point(const float* __restrict__ pts, const float* __restrict__ vts,
                                                                         const int32_t* __restrict__ faces,
                                                                         const int32_t* __restrict__ face,
                                                                         const int32_t* __restrict__ kind,
                                                                         const float* __restrict__ ddist, int P, int V, int F,
                                                                         float* __restrict__ dpts, VertexRecords rec) {
    const int bi = blockIdx.y, i = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (i >= P) return;
    const size_t at = (size_t)bi * P + i;
    const int f = face[at], k = kind[at];
    int ia = -1, ib = -1, ic = -1;
    float wa = 0.f, wb = 0.f, wc = 0.f;
    f3 g = {0.f, 0.f, 0.f};
    bool ok = f >= 0 && f < F && k >= 0 && k <= 6;
    if (ok) {
        ia = faces[(size_t)f * 3]; ib = faces[(size_t)f * 3 + 1]; ic = faces[(size_t)f * 3 + 2];
        ok = ia >= 0 && ia < V && ib >= 0 && ib < V && ic >= 0 && ic < V;
    }
    if (ok) {
        const float* pp = pts + at * 3;
        const float* pa = vts + ((size_t)bi * V + ia) * 3;
        const float* pb = vts + ((size_t)bi * V + ib) * 3;
        const float* pc = vts + ((size_t)bi * V + ic) * 3;
        const f3 p = {pp[0], pp[1], pp[2]}, a = {pa[0], pa[1], pa[2]}, b = {pb[0], pb[1], pb[2]}, c = {pc[0], pc[1], pc[2]};
        const f3 ab = b - a, ac = c - a, ap = p - a;
        f3 d;
        float t;
        if (k == 1) { d = ap; wa = 1.f; }
        else if (k == 2) { d = p - b; wb = 1.f; }
        else if (k == 3) { d = p - c; wc = 1.f; }
        else if (k == 4) { d = seg_diff(ap, ab, t); wa = 1.f - t; wb = t; }
        else if (k == 6) { d = seg_diff(ap, ac, t); wa = 1.f - t; wc = t; }
        else if (k == 5) { d = seg_diff(p - b, c - b, t); wb = 1.f - t; wc = t; }
        else {                                                             // the plane: p - q = (ap . n / |n|^2) n
            const f3 n = cross(ab, ac), r = cross(ap, n);
            const float nn = dot(n, n), inv = nn != 0.f ? 1.f / nn : 0.f;
            const float v = -dot(ac, r) * inv, w = dot(ab, r) * inv, s = dot(ap, n) * inv;
            d = f3{n.x * s, n.y * s, n.z * s}; wa = 1.f - v - w; wb = v; wc = w;
        }
        const float up = 2.f * ddist[at];
        g = {up * d.x, up * d.y, up * d.z};
        // vertices whose weight is zero by the kind take no part in the accumulation
        if (k == 2 || k == 3 || k == 5) ia = -1;
        if (k == 1 || k == 3 || k == 6) ib = -1;
        if (k == 1 || k == 2 || k == 4) ic = -1;
    } else {
        ia = ib = ic = -1;
    }
    if (dpts) { dpts[at * 3] = g.x; dpts[at * 3 + 1] = g.y; dpts[at * 3 + 2] = g.z; }
    if (rec.id) {
        rec.id[at] = make_int4(ia, ib, ic, -1);
        rec.gw[at] = make_float4(-g.x, -g.y, -g.z, wa);
        rec.w12[at] = make_float2(wb, wc);
    }
}

// ---------------------------------------------------------------------------------------------------------
// Grid-accelerated forward of the same distance: the result of k_point_to_mesh, bit for bit (same tri_dist2, same tie rule),
// from a uniform grid of G^3 cells over the mesh's bounding cube (G a host-side function of F alone, p2m_grid_res).
//
// Build, per mesh (blockIdx.y):
//   k_p2m_grid_bounds  bounding box of the mesh's vertices -> header: lo, cell size h = largest extent / G, 1 / h, amax = largest
//                      |coordinate|, mode.  mode 1 (no grid, every triangle on the always-tested list) for a mesh with a non-finite
//                      vertex, extent or amax outside [1e-8, 1e8], or extent < 1e-3 amax.
//   k_p2m_grid_count   per triangle: centroid c (fp32), r = largest |vertex - c|, cell of c (clamped) or, if r > 2 h or mode 1, the
//                      always-tested list (stored as cell G^3) -> tcell[f]; integer atomicAdd on the cell's count, integer
//                      atomicMax (float bits, r >= 0) of r over the binned triangles -> rmax.
//   k_p2m_grid_scan    exclusive block_scan of the G^3 + 1 counts in place: e[c] = first slot of cell c, e[G^3 + 1] = F.
//   k_p2m_grid_fill    slot = atomicAdd(e[c + 1]) (afterwards e[c + 1] is the END of cell c = the begin of c + 1, e[0] stays 0);
//                      the triangle's three resolved vertices and its index go to the slot (three float4, 48 contiguous bytes: the
//                      query reads a triangle with three 16-byte loads and no faces -> vertices double gather).
// Every triangle is stored exactly once, so the index size depends on F alone.  The order inside a cell depends on the order of
// the atomics; the result does not, because the query's update rule is a total order on (d2, face index).
//
// Query (k_p2m_grid_query, one thread per point): the always-tested list, then shells of cells at Chebyshev distance k = 0, 1, ...
// from the point's clamped cell; cells of one x-row are one contiguous slot range.  After shell k the visited block is
// [c - k, c + k]^3 cut to the grid.  A binned triangle not yet visited has its centroid's cell beyond one of the block's faces that
// is not on the grid border, so |p - centroid| >= dmin, the smallest distance of p to such a face, and every point of the triangle
// is within rmax of the centroid (a convex function on a triangle peaks at a vertex, whatever fp32 value the centroid got): its
// distance is >= dmin - rmax.  The search stops when that bound is positive and its square exceeds the best distance strictly.
//
// The bound is evaluated in fp32 and made conservative (u = 2^-24 = 6e-8):
//   * cells are assigned by t(x) = fl(fl(x - lo) * inv_h), index = clamp(floor t), for centroids and points alike.  t is monotone
//     and t(x) = (x - lo) / h' (1 + e), |e| <= 2.1 u, h' = 1 / inv_h.  A centroid in a cell beyond the face at integer m has
//     t(c) >= m (clamping only moves indices at border faces, which are ignored), so whichever side of the nominal boundary
//     rounding put it, (c.x - p.x) / h' >= (m - t(p)) - 2.1 u (|t(c)| + |t(p)|) and |t(c)| <= G + 1.  Shrinking the cell-unit
//     distance by 1e-6 (G + 1 + |t(p)|) covers that and the rounding of the subtraction five times over; h vs h' and the product
//     are two more roundings (factor 1 - 1e-6).
//   * r is a square root of three squares of differences, a few u relative; the mesh extent is >= 1e-8, so h >= 1e-10 and an
//     underflowing square (r < 2e-19) is far below the absolute 1e-6 h that is added: rmax (1 + 1e-5) + 1e-6 h, and 1 % on top for the interior case below.
//   * the brute-force value itself is fp32 and may undercut the true distance.  On a vertex, an edge or a flattened triangle
//     tri_dist2 returns |p - q|^2 for a q on the triangle (a vertex, or u + t uw with t in [0, 1]) up to about 8 u (amax + |p|):
//     4e-6 (amax + |p|_inf) is subtracted.  In the interior it returns the distance to the plane of the COMPUTED normal, which is
//     off by an angle e <= 4 u / sin(angle at vertex 0) <= 2^13 u = 4.9e-4 (larger and the triangle is flattened), and the three
//     edge functions place the foot with an error of about (e + 5 u) |ap|, |ap| <= distance + 2 r.  A foot accepted that far
//     outside the triangle, on a plane tilted that much, undercuts by at most about 2 e |ap| < 1e-3 (distance + 2 r): rmax is
//     taken 1 % larger and the square is compared with a factor 1 - 1e-2, five times that.
// Cost bounds: a point far from the surface walks shells that are mostly empty, two dependent loads per slot range and at most
// 2 (2k + 1)^2 ranges in shell k -- latency-bound, and measured 8 x slower than the brute-force kernel when such a walk was allowed
// to cover the grid.  So the walk is cut after kmax = max(2, G / 4) shells (<= ~(8 / 3) kmax^3 range reads); a point that is not done
// by then (farther from the mesh than about a quarter of its extent, or NaN / infinite: it never stops early) scans the whole
// sorted list instead, F tests, which is the brute-force pass without its LDS staging.  The worst case per point is therefore the
// bounded walk plus F tests, and a NaN point ends with the brute-force output 3.4e38 / 0 / 0.  One huge triangle does not inflate
// rmax: it is on the always-tested list (length <= F, device side), as is every triangle of a mode-1 mesh.
// ---------------------------------------------------------------------------------------------------------
constexpr int GRID_SCAN_BLOCK = 1024;
constexpr int GRID_HDR_WORDS = 16;           // lo.xyz, h, inv_h, amax, mode (int), rmax (float bits); 64 bytes per mesh

struct P2MGrid {                             // the caller's workspace, per-mesh strides in elements
    uint32_t* hdr;                           // [B][GRID_HDR_WORDS]
    int32_t* e;                              // [B][e_stride]: G^3 + 2 used
    int32_t* tcell;                          // [B][t_stride]: F used
    float* tris;                             // [B][s_stride]: F * 12 used (a.xyz, face index bits | b.xyz, 0 | c.xyz, 0)
    size_t e_stride, t_stride, s_stride;
    int G;
};

__device__ __forceinline__ int grid_cell(float x, float lo, float inv_h, int G, float& t) {
    t = (x - lo) * inv_h;
    return !(t >= 0.f) ? 0 : (t >= (float)G ? G - 1 : (int)t);            // NaN -> 0
}

__global__ __launch_bounds__(GRID_SCAN_BLOCK) void k_p2m_grid_bounds(const float* __restrict__ vts, int V, P2MGrid g) {
    __shared__ float red[7][GRID_SCAN_BLOCK / 64];
    const int b = blockIdx.x;
    const float* v = vts + (size_t)b * V * 3;
    float lo[3] = {3.4e38f, 3.4e38f, 3.4e38f}, hi[3] = {-3.4e38f, -3.4e38f, -3.4e38f}, bad = 0.f;
    for (int i = threadIdx.x; i < V; i += GRID_SCAN_BLOCK)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float x = v[(size_t)i * 3 + c];
            if (!(fabsf(x) <= 3.0e38f)) bad = 1.f;
            lo[c] = fminf(lo[c], x);
            hi[c] = fmaxf(hi[c], x);
        }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lo[c] = fminf(lo[c], __shfl_xor(lo[c], d, 64));
            hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d, 64));
        }
        bad = fmaxf(bad, __shfl_xor(bad, d, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        for (int c = 0; c < 3; ++c) { red[c][w] = lo[c]; red[3 + c][w] = hi[c]; }
        red[6][w] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < GRID_SCAN_BLOCK / 64; ++k) {
            for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], red[c][k]); hi[c] = fmaxf(hi[c], red[3 + c][k]); }
            bad = fmaxf(bad, red[6][k]);
        }
        float ext = 0.f, amax = 0.f;
        for (int c = 0; c < 3; ++c) {
            ext = fmaxf(ext, hi[c] - lo[c]);
            amax = fmaxf(amax, fmaxf(fabsf(lo[c]), fabsf(hi[c])));
        }
        // grid only where the slack of the bound stays far below a cell: finite, extent in [1e-8, 1e8], not a speck far from the origin
        const bool ok = bad == 0.f && ext >= 1e-8f && ext <= 1e8f && amax <= 1e8f && ext >= 1e-3f * amax;
        const float h = ok ? ext / (float)g.G : 1.f;
        uint32_t* o = g.hdr + (size_t)b * GRID_HDR_WORDS;
        o[0] = __float_as_uint(ok ? lo[0] : 0.f);
        o[1] = __float_as_uint(ok ? lo[1] : 0.f);
        o[2] = __float_as_uint(ok ? lo[2] : 0.f);
        o[3] = __float_as_uint(h);
        o[4] = __float_as_uint(1.f / h);
        o[5] = __float_as_uint(ok ? amax : 0.f);
        o[6] = ok ? 0u : 1u;
        // o[7] (rmax bits) stays at the 0 of the caller's clear; k_p2m_grid_count raises it
    }
}

__device__ __forceinline__ void grid_load_tri(const float* __restrict__ vts, const int32_t* __restrict__ faces, int b, int V, int f,
                                              f3& a0, f3& a1, f3& a2) {
    const float* q0 = vts + ((size_t)b * V + faces[(size_t)f * 3]) * 3;
    const float* q1 = vts + ((size_t)b * V + faces[(size_t)f * 3 + 1]) * 3;
    const float* q2 = vts + ((size_t)b * V + faces[(size_t)f * 3 + 2]) * 3;
    a0 = {q0[0], q0[1], q0[2]}; a1 = {q1[0], q1[1], q1[2]}; a2 = {q2[0], q2[1], q2[2]};
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_p2m_grid_count(const float* __restrict__ vts, const int32_t* __restrict__ faces, int V,
                                                                int F, P2MGrid g) {
    const int b = blockIdx.y, f = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    uint32_t* hdr = g.hdr + (size_t)b * GRID_HDR_WORDS;
    const int G = g.G, NC = G * G * G;
    float r_binned = 0.f;
    if (f < F) {
        const f3 lo = {__uint_as_float(hdr[0]), __uint_as_float(hdr[1]), __uint_as_float(hdr[2])};
        const float h = __uint_as_float(hdr[3]), inv_h = __uint_as_float(hdr[4]);
        int cell = NC;
        if (hdr[6] == 0u) {
            f3 a0, a1, a2;
            grid_load_tri(vts, faces, b, V, f, a0, a1, a2);
            const f3 s = a0 + a1 + a2;
            const f3 c = {s.x * (1.f / 3.f), s.y * (1.f / 3.f), s.z * (1.f / 3.f)};
            const f3 e0 = a0 - c, e1 = a1 - c, e2 = a2 - c;
            const float r = sqrtf(fmaxf(dot(e0, e0), fmaxf(dot(e1, e1), dot(e2, e2))));
            if (r <= 2.f * h) {                                            // false for NaN: cannot happen in mode 0, harmless if it did
                float t;
                const int cx = grid_cell(c.x, lo.x, inv_h, G, t), cy = grid_cell(c.y, lo.y, inv_h, G, t),
                          cz = grid_cell(c.z, lo.z, inv_h, G, t);
                cell = (cz * G + cy) * G + cx;
                r_binned = r;
            }
        }
        g.tcell[(size_t)b * g.t_stride + f] = cell;
        atomicAdd(g.e + (size_t)b * g.e_stride + cell + 1, 1);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) r_binned = fmaxf(r_binned, __shfl_xor(r_binned, d, 64));
    if ((threadIdx.x & 63) == 0 && r_binned > 0.f) atomicMax(hdr + 7, __float_as_uint(r_binned));   // r >= 0: bits order as values
}

// exclusive scan in place of e[1 .. n] (n = G^3 + 1 counts), one block per mesh; e[0] stays 0
__global__ __launch_bounds__(SCAN_BLOCK) void k_p2m_grid_scan(P2MGrid g) {
    block_scan<int32_t, false>(g.e + (size_t)blockIdx.x * g.e_stride + 1, g.G * g.G * g.G + 1);
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_p2m_grid_fill(const float* __restrict__ vts, const int32_t* __restrict__ faces, int V,
                                                               int F, P2MGrid g) {
    const int b = blockIdx.y, f = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (f >= F) return;
    const int cell = g.tcell[(size_t)b * g.t_stride + f];
    const int slot = atomicAdd(g.e + (size_t)b * g.e_stride + cell + 1, 1);
    if (slot < 0 || slot >= F) return;                                     // cannot happen: the counts of this same tcell sum to F
    f3 a0, a1, a2;
    grid_load_tri(vts, faces, b, V, f, a0, a1, a2);
    float4* o = reinterpret_cast<float4*>(g.tris + (size_t)b * g.s_stride + (size_t)slot * 12);   // 48-byte records, 16-byte aligned
    o[0] = make_float4(a0.x, a0.y, a0.z, __int_as_float(f));
    o[1] = make_float4(a1.x, a1.y, a1.z, 0.f);
    o[2] = make_float4(a2.x, a2.y, a2.z, 0.f);
}

__global__ __launch_bounds__(LOSS_BLOCK) void k_p2m_grid_query(const float* __restrict__ pts, int P, int F, P2MGrid g,
                                                                float* __restrict__ dist, int32_t* __restrict__ face,
                                                                int32_t* __restrict__ kind) {
    const int b = blockIdx.y, i = blockIdx.x * LOSS_BLOCK + threadIdx.x;
    if (i >= P) return;
    const uint32_t* hdr = g.hdr + (size_t)b * GRID_HDR_WORDS;
    const int32_t* e = g.e + (size_t)b * g.e_stride;
    const float* tris = g.tris + (size_t)b * g.s_stride;
    const int G = g.G, NC = G * G * G;
    const float* pp = pts + ((size_t)b * P + i) * 3;
    const f3 p = {pp[0], pp[1], pp[2]};
    float best = 3.4e38f;
    int best_f = 0, best_k = 0;
    auto test = [&](int s0, int s1) {
        s0 = max(s0, 0); s1 = min(s1, F);                                  // the slots stay inside the list whatever e holds
        for (int s = s0; s < s1; ++s) {
            const float4* r = reinterpret_cast<const float4*>(tris + (size_t)s * 12);
            const float4 r0 = r[0], r1 = r[1], r2 = r[2];
            const int f = __float_as_int(r0.w);
            int k;
            const float d2 = tri_dist2(p, f3{r0.x, r0.y, r0.z}, f3{r1.x, r1.y, r1.z}, f3{r2.x, r2.y, r2.z}, k);
            if (d2 < best || (d2 == best && f < best_f)) { best = d2; best_f = f; best_k = k; }
        }
    };
    test(e[NC], e[NC + 1]);                                                // the always-tested list
    if (hdr[6] == 0u) {
        const f3 lo = {__uint_as_float(hdr[0]), __uint_as_float(hdr[1]), __uint_as_float(hdr[2])};
        const float h = __uint_as_float(hdr[3]), inv_h = __uint_as_float(hdr[4]), amax = __uint_as_float(hdr[5]);
        const float rmax = __uint_as_float(hdr[7]) * (1.f + 1e-2f) + 1e-6f * h;
        float tx, ty, tz;
        const int cx = grid_cell(p.x, lo.x, inv_h, G, tx), cy = grid_cell(p.y, lo.y, inv_h, G, ty), cz = grid_cell(p.z, lo.z, inv_h, G, tz);
        const float pmax = fmaxf(fabsf(p.x), fmaxf(fabsf(p.y), fabsf(p.z)));
        const bool finite = fabsf(p.x) <= 3.0e38f && fabsf(p.y) <= 3.0e38f && fabsf(p.z) <= 3.0e38f;
        const float tslack = 1e-6f * ((float)(G + 1) + fmaxf(fabsf(tx), fmaxf(fabsf(ty), fabsf(tz))));
        const float dslack = rmax + 4e-6f * (amax + pmax);
        const int kmax = max(2, G / 4);
        bool walked_out = false;
        for (int k = 0;; ++k) {                                            // ends at k = kmax + 1 <= G at the latest
            if (k > kmax) { walked_out = true; break; }
            const int x0 = max(cx - k, 0), x1 = min(cx + k, G - 1), y0 = max(cy - k, 0), y1 = min(cy + k, G - 1);
            const int z0 = max(cz - k, 0), z1 = min(cz + k, G - 1);
            for (int z = z0; z <= z1; ++z)
                for (int y = y0; y <= y1; ++y) {
                    const int row = (z * G + y) * G;
                    if (abs(z - cz) == k || abs(y - cy) == k) test(e[row + x0], e[row + x1 + 1]);
                    else {
                        if (cx - k >= 0) test(e[row + cx - k], e[row + cx - k + 1]);
                        if (cx + k <= G - 1) test(e[row + cx + k], e[row + cx + k + 1]);
                    }
                }
            // distance (in cells) to the nearest face of the visited block that is not on the grid border
            float dt = 3.4e38f;
            if (x0 > 0) dt = fminf(dt, tx - (float)x0);
            if (x1 < G - 1) dt = fminf(dt, (float)(x1 + 1) - tx);
            if (y0 > 0) dt = fminf(dt, ty - (float)y0);
            if (y1 < G - 1) dt = fminf(dt, (float)(y1 + 1) - ty);
            if (z0 > 0) dt = fminf(dt, tz - (float)z0);
            if (z1 < G - 1) dt = fminf(dt, (float)(z1 + 1) - tz);
            if (dt == 3.4e38f) break;                                      // every cell visited
            const float bound = (dt - tslack) * h * (1.f - 1e-6f) - dslack;
            if (finite && bound > 0.f && bound * bound * (1.f - 1e-2f) > best) break;
        }
        // not excluded after kmax shells (farther from the mesh than about a quarter of its extent, or not finite): the whole
        // list, linearly.  Re-testing a triangle changes nothing; such lanes of a wave scan in lockstep, reading the same slots.
        if (walked_out) test(0, F);
    }
    dist[(size_t)b * P + i] = best;
    face[(size_t)b * P + i] = best_f;
    kind[(size_t)b * P + i] = best_k;
}

}  // namespace

void launch_point_to_mesh(const float* pts, const float* vts, const int32_t* faces, int B, int P, int V, int F, float* dist,
                          int32_t* face, int32_t* kind, hipStream_t s) {
    prof_mark_begin(PROF_P2M, 0.0, s);
    hipLaunchKernelGGL(k_point_to_mesh, dim3((P + LOSS_BLOCK - 1) / LOSS_BLOCK, B), dim3(LOSS_BLOCK), 0, s, pts, vts, faces, P, V, F,
                       dist, face, kind);
    prof_mark_end(s);
}

void launch_point_to_mesh_bwd(const float* pts, const float* vts, const int32_t* faces, const int32_t* face, const int32_t* kind,
                              const float* ddist, int B, int P, int V, int F, float* dpts, float* dvts, void* ws, hipStream_t s) {
    const VertexRecords rec = dvts ? vertex_records(ws, (size_t)B * P) : VertexRecords{nullptr, nullptr, nullptr};
    prof_mark_begin(PROF_P2M_BWD_POINT, 0.0, s);
    hipLaunchKernelGGL(k_point_to_mesh_bwd_point, dim3((P + LOSS_BLOCK - 1) / LOSS_BLOCK, B), dim3(LOSS_BLOCK), 0, s, pts, vts, faces,
                       face, kind, ddist, P, V, F, dpts, rec);
    prof_mark_end(s);
    if (dvts) launch_vertex_scatter(PROF_P2M_BWD_VERTEX, ws, B, P, V, dvts, s);
}

// G = round(sqrt(F / 16)) in [1, 64]: about 16 triangles per occupied cell of a closed surface (which fills ~6 G^2 of the G^3
// cells); a function of F alone and non-decreasing in it, so that the workspace size is too.
int p2m_grid_res(int F) {
    int G = 1;
    while (G < 64 && (long)(2 * G + 1) * (2 * G + 1) * 4 <= (long)F) ++G;          // (G + 1/2)^2 * 16 <= F
    return G;
}

static size_t up16(size_t bytes) { return (bytes + 15) / 16 * 16; }

static size_t p2m_grid_layout(int B, int F, P2MGrid* g, void* ws, size_t* clear_bytes) {
    const int G = p2m_grid_res(F);
    const size_t hdr = (size_t)B * GRID_HDR_WORDS * 4, e1 = up16(((size_t)G * G * G + 2) * 4), t1 = up16((size_t)F * 4),
                 s1 = (size_t)F * 48;
    if (g) {
        char* base = static_cast<char*>(ws);
        g->G = G;
        g->hdr = reinterpret_cast<uint32_t*>(base);
        g->e = reinterpret_cast<int32_t*>(base + hdr);
        g->tcell = reinterpret_cast<int32_t*>(base + hdr + B * e1);
        g->tris = reinterpret_cast<float*>(base + hdr + B * (e1 + t1));
        g->e_stride = e1 / 4; g->t_stride = t1 / 4; g->s_stride = s1 / 4;
    }
    if (clear_bytes) *clear_bytes = hdr + B * e1;                           // headers (rmax) and cell counts start at zero
    return hdr + B * (e1 + t1 + s1);
}

size_t point_to_mesh_grid_bytes(int B, int F) { return p2m_grid_layout(B, F, nullptr, nullptr, nullptr); }

hipError_t launch_point_to_mesh_grid(const float* pts, const float* vts, const int32_t* faces, int B, int P, int V, int F, float* dist,
                                     int32_t* face, int32_t* kind, void* ws, hipStream_t s) {
    P2MGrid g;
    size_t clear = 0;
    p2m_grid_layout(B, F, &g, ws, &clear);
    const hipError_t rc = hipMemsetAsync(ws, 0, clear, s);
    if (rc != hipSuccess) return rc;
    const dim3 tri_grid((F + LOSS_BLOCK - 1) / LOSS_BLOCK, B);
    prof_mark_begin(PROF_P2M_GRID_BOUNDS, 0.0, s);
    hipLaunchKernelGGL(k_p2m_grid_bounds, dim3(B), dim3(GRID_SCAN_BLOCK), 0, s, vts, V, g);
    prof_mark_end(s);
    prof_mark_begin(PROF_P2M_GRID_COUNT, 0.0, s);
    hipLaunchKernelGGL(k_p2m_grid_count, tri_grid, dim3(LOSS_BLOCK), 0, s, vts, faces, V, F, g);
    prof_mark_end(s);
    prof_mark_begin(PROF_P2M_GRID_SCAN, 0.0, s);
    hipLaunchKernelGGL(k_p2m_grid_scan, dim3(B), dim3(SCAN_BLOCK), 0, s, g);
    prof_mark_end(s);
    prof_mark_begin(PROF_P2M_GRID_FILL, 0.0, s);
    hipLaunchKernelGGL(k_p2m_grid_fill, tri_grid, dim3(LOSS_BLOCK), 0, s, vts, faces, V, F, g);
    prof_mark_end(s);
    prof_mark_begin(PROF_P2M_GRID_QUERY, 0.0, s);
    hipLaunchKernelGGL(k_p2m_grid_query, dim3((P + LOSS_BLOCK - 1) / LOSS_BLOCK, B), dim3(LOSS_BLOCK), 0, s, pts, P, F, g, dist, face,
                       kind);
    prof_mark_end(s);
    return hipSuccess;
}

}  // namespace icn
