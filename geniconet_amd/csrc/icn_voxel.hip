// Solid voxelisation of closed triangle meshes by ray parity (icn_mesh_voxelize in include/icn_voxel.h): for every cell of a lattice
// whether its centre lies inside the mesh.  vertices (B, V, 3) fp32, faces (F, 3) shared by the batch, occupancy (B, n0, n1, n2) uint8.
// The definition (one, for this kernel, metrics._torch_voxelize and the tests), ALL OF IT IN DOUBLE on the fp32 vertices, every product
// and sum rounded on its own in the order written (no contraction: the float64 reference has no FMA).  Rays run along axis 0; a COLUMN
// is (j, k) with p = (py, pz), py = origin_y + (j + 0.5) h, pz likewise.
//   a face is TESTED for a column iff its ids lie in [0, V), its nine coordinates are finite and lo_y <= py <= hi_y, lo_z <= pz <= hi_z
//     against the fp32 min / max of its vertices (part of the definition, not a filter that has to be conservative)
//   the edge value of a directed edge u -> w: with (a, b) = (u, w) if id_u < id_w, else (w, u),
//     s = (b.y - a.y) (pz - a.z) - (b.z - a.z) (py - a.y);  t = sign(s), if 0 sign(-(b.z - a.z)), if still 0 sign(b.y - a.y)
//     (the symbolic perturbation p + (eps, eps^2)); both negated if the ends were swapped: the two faces of an edge get opposite values
//   the face COVERS the column iff t > 0 for its three edges or t < 0 for all three
//   its crossing: s0, s1, s2 the values of the edges opposite vertices 0, 1, 2 (the raw s),
//     x = (s0 v0.x + s1 v1.x + s2 v2.x) / (s0 + s1 + s2),  tau = (x - origin_x) / h - 0.5, dropped if not finite, k0 = clamp(ceil(tau), 0, n0)
//   cell i of the column is occupied iff the number of crossings with k0 <= i is odd.
// k_mesh_voxelize: grid (tiles of columns, B), one thread per column, a workgroup of MESH_BLOCK threads covers VOX_TJ x VOX_TK columns
// (j, k) with k fastest, as the output has it.  Faces are staged through LDS in tiles of MESH_BLOCK by stage_face_tile
// (icn_mesh_device.h); while staging, a face that no column of the workgroup would test -- invalid, or its (y, z) box misses the box of
// the tile's columns, which is exact because py and pz are monotone in j and k -- is dropped and the survivors are compacted by ballot and
// popcount (a fixed order, no atomics).  An entry is VOX_WORDS = 17 words -- nine coordinates, three ids, the (y, z) box, one of padding
// -- odd, so the fill touches every bank once; the reads are broadcasts.  The box test of the hot loop is four fp32 compares: for a
// float l and a double p, l <= p iff l <= the largest float <= p, and p <= l iff the smallest float >= p <= l.
// The n0 parity bits of a column live in a [word][thread] slab of LDS (thread-private, conflict-free, no register array that could be
// indexed dynamically): a crossing flips bit k0, one prefix XOR across the words at the end gives the cells, and every byte of the
// output is stored exactly once.  XOR commutes, so the order of the faces changes nothing: bit-identical run to run, and equal to the
// float64 formulation byte for byte.  No atomics, no workspace, safe whatever `faces` holds.
// Timings on an MI355X: profiles/voxelize.txt (tools/time_voxelize.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

#pragma clang fp contract(off)

namespace icn {
namespace {

constexpr int VOX_TJ = 16, VOX_TK = 16;     // the workgroup's tile of columns, k fastest
static_assert(VOX_TJ * VOX_TK == MESH_BLOCK, "one thread per column of the tile");
constexpr int VOX_WORDS = 17;               // 9 coordinates, 3 ids, lo_y hi_y lo_z hi_z, 1 of padding: odd, so the fills are conflict-free
constexpr int VOX_BOX = FACE_WORDS;
constexpr int VOX_BITS = VOXEL_MAX_DEPTH / 32;

struct VoxLattice {
    double ox, oy, oz, h;
    int n0, n1, n2, tiles_k;
};

__device__ __forceinline__ double centre(double origin, int i, double h) { return origin + ((double)i + 0.5) * h; }

// the largest float <= x and the smallest float >= x (x is not NaN; beyond the floats' range they are the infinities / FLT_MAX)
__device__ __forceinline__ float float_below(double x) {
    const float f = (float)x;
    return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
__device__ __forceinline__ float float_above(double x) {
    const float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
}

// the raw value s and the decided sign t of the directed edge u -> w at (py, pz), evaluated on its ends in the order of their ids
__device__ __forceinline__ void edge_value(int iu, int iw, double uy, double uz, double wy, double wz, double py, double pz, double& s,
                                           int& t) {
    const bool as_given = iu < iw;
    const double ay = as_given ? uy : wy, az = as_given ? uz : wz, by = as_given ? wy : uy, bz = as_given ? wz : uz;
    const double dy = by - ay, dz = bz - az;
    const double v = dy * (pz - az) - dz * (py - ay);
    int sign = (v > 0.0) - (v < 0.0);
    if (sign == 0) sign = (dz < 0.0) - (dz > 0.0);
    if (sign == 0) sign = (dy > 0.0) - (dy < 0.0);
    s = as_given ? v : -v;
    t = as_given ? sign : -sign;
}

// the fp32 (y, z) box of a face: min / max of fp32 values are exact
struct YZBox { float lo_y, hi_y, lo_z, hi_z; };
__device__ __forceinline__ YZBox yz_box(const LoadedFace& t) {
    return {fminf(fminf(t.p[0].y, t.p[1].y), t.p[2].y), fmaxf(fmaxf(t.p[0].y, t.p[1].y), t.p[2].y),
            fminf(fminf(t.p[0].z, t.p[1].z), t.p[2].z), fmaxf(fmaxf(t.p[0].z, t.p[1].z), t.p[2].z)};
}

template <bool CULL>
__global__ __launch_bounds__(MESH_BLOCK) void k_mesh_voxelize(const float* __restrict__ vts, const int32_t* __restrict__ faces, int V, int F,
                                                               VoxLattice L, uint8_t* __restrict__ occ) {
    __shared__ float tile[MESH_BLOCK * VOX_WORDS];
    __shared__ uint32_t bits[VOX_BITS * MESH_BLOCK];
    __shared__ int wave_count[MESH_BLOCK / 64];
    const int tid = threadIdx.x;
    const int b = blockIdx.y, tj = blockIdx.x / L.tiles_k, tk = blockIdx.x - tj * L.tiles_k;
    const int j0 = tj * VOX_TJ, k0 = tk * VOX_TK;
    const int j = j0 + tid / VOX_TK, k = k0 + tid % VOX_TK;
    const bool live = j < L.n1 && k < L.n2;
    const float* v = vts + (size_t)b * V * 3;
    const double py = centre(L.oy, j, L.h), pz = centre(L.oz, k, L.h);
    const float py_below = float_below(py), py_above = float_above(py), pz_below = float_below(pz), pz_above = float_above(pz);
    // the box of the tile's columns: centre() is monotone in its index
    const float ty_above = float_above(centre(L.oy, j0, L.h)), ty_below = float_below(centre(L.oy, min(j0 + VOX_TJ, L.n1) - 1, L.h));
    const float tz_above = float_above(centre(L.oz, k0, L.h)), tz_below = float_below(centre(L.oz, min(k0 + VOX_TK, L.n2) - 1, L.h));
    const int words = (L.n0 + 31) >> 5;
    for (int w = 0; w < words; ++w) bits[w * MESH_BLOCK + tid] = 0u;         // thread-private: no barrier needed
    for (int f0 = 0; f0 < F; f0 += MESH_BLOCK) {
        const int nf = stage_face_tile<VOX_WORDS>(
            tile, wave_count, v, faces, f0, F, V,
            [](const LoadedFace& t, int, float* e) {
                const YZBox box = yz_box(t);
                e[VOX_BOX] = box.lo_y, e[VOX_BOX + 1] = box.hi_y, e[VOX_BOX + 2] = box.lo_z, e[VOX_BOX + 3] = box.hi_z;
            },
            [&](const LoadedFace& t) {                                       // a face whose (y, z) box misses the tile's columns is dropped
                if (!CULL) return true;
                const YZBox box = yz_box(t);
                return (box.lo_y <= ty_below) && (ty_above <= box.hi_y) && (box.lo_z <= tz_below) && (tz_above <= box.hi_z);
            });
        if (!live) continue;
        for (int jj = 0; jj < nf; ++jj) {
            const float* e = tile + jj * VOX_WORDS;
            const bool tested = (e[VOX_BOX] <= py_below) & (py_above <= e[VOX_BOX + 1]) & (e[VOX_BOX + 2] <= pz_below) &
                                (pz_above <= e[VOX_BOX + 3]);
            if (!tested) continue;
            const int i0 = __float_as_int(e[FACE_ID]), i1 = __float_as_int(e[FACE_ID + 1]), i2 = __float_as_int(e[FACE_ID + 2]);
            const double y0 = e[1], z0 = e[2], y1 = e[4], z1 = e[5], y2 = e[7], z2 = e[8];
            double s0, s1, s2;
            int t0, t1, t2;
            edge_value(i1, i2, y1, z1, y2, z2, py, pz, s0, t0);
            edge_value(i2, i0, y2, z2, y0, z0, py, pz, s1, t1);
            edge_value(i0, i1, y0, z0, y1, z1, py, pz, s2, t2);
            if (!((t0 > 0 && t1 > 0 && t2 > 0) || (t0 < 0 && t1 < 0 && t2 < 0))) continue;
            const double x = (s0 * (double)e[0] + s1 * (double)e[3] + s2 * (double)e[6]) / (s0 + s1 + s2);
            const double tau = (x - L.ox) / L.h - 0.5;
            if (!isfinite(tau)) continue;
            const double first = ceil(tau);
            if (first >= (double)L.n0) continue;                             // k0 = n0: no cell of the lattice lies behind it
            const int at = first <= 0.0 ? 0 : (int)first;
            bits[(at >> 5) * MESH_BLOCK + tid] ^= 1u << (at & 31);
        }
    }
    if (!live) return;
    const size_t plane = (size_t)L.n1 * L.n2;
    uint8_t* o = occ + (size_t)b * L.n0 * plane + (size_t)j * L.n2 + k;
    uint32_t carry = 0u;                                                     // all ones iff the crossings before this word are odd
    for (int w = 0; w < words; ++w) {
        uint32_t x = bits[w * MESH_BLOCK + tid];
        x ^= x << 1, x ^= x << 2, x ^= x << 4, x ^= x << 8, x ^= x << 16;    // bit i = the parity of bits 0 .. i
        x ^= carry;
        carry = 0u - (x >> 31);
        const int n = min(32, L.n0 - 32 * w);
        for (int i = 0; i < n; ++i) o[(size_t)(32 * w + i) * plane] = (uint8_t)((x >> i) & 1u);
    }
}

}  // namespace

void launch_mesh_voxelize(const float* vts, const int32_t* faces, int B, int V, int F, double ox, double oy, double oz, double h, int n0,
                          int n1, int n2, uint8_t* occ, hipStream_t s) {
    const int tiles_j = (n1 + VOX_TJ - 1) / VOX_TJ, tiles_k = (n2 + VOX_TK - 1) / VOX_TK;
    const VoxLattice L = {ox, oy, oz, h, n0, n1, n2, tiles_k};
    prof_mark_begin(PROF_MESH_VOXELIZE, 0.0, s);
#ifdef ICN_VOXEL_NO_CULL                     // a timing build (tools/time_voxelize.py): every valid face reaches every column's box test
    hipLaunchKernelGGL(k_mesh_voxelize<false>, dim3((unsigned)(tiles_j * tiles_k), B), dim3(MESH_BLOCK), 0, s, vts, faces, V, F, L, occ);
#else
    hipLaunchKernelGGL(k_mesh_voxelize<true>, dim3((unsigned)(tiles_j * tiles_k), B), dim3(MESH_BLOCK), 0, s, vts, faces, V, F, L, occ);
#endif
    prof_mark_end(s);
}


// ---- occupancy histograms of point clouds and their Jensen-Shannon divergence (include/icn_occupancy.h, where the definition is written
// out; metrics._torch_occupancy_counts and _torch_occupancy_jsd restate it) -- the other "what lies in which lattice cell" operator.
// k_point_occupancy: grid (S, nb), 1024 threads.  A HISTOGRAM (the whole set: nb = 1; or one cloud: nb = B) is a run of P consecutive
// points of the flat (B N, 3) array, cut into S pieces of `per` points (a multiple of 4); workgroup (s, b) owns piece s of histogram b
// and a PRIVATE copy of all R^3 cells in dynamic LDS (87 808 bytes at R = 28, 131 072 at 32: one workgroup a CU, which is why a piece
// is not smaller than OCC_POINTS points -- zeroing, reading and storing R^3 words is the fixed cost, about what 7 300 points cost to
// read at R = 28).  It zeroes the copy, streams its piece, adds 1 with ds_add_u32 (integer, no return value: order-free, so the counts
// are the definition's whatever the split) and stores the copy once: to `counts` itself when S == 1, else to slice b S + s of the
// workspace for k_occupancy_reduce.  No global atomics, no memset, nothing waits on another workgroup, every loop is bounded by sizes.
// Loads: a thread takes an ALIGNED group of four points, 48 bytes = three float4 loads off a 16-byte aligned address (group g starts
// at float 12 g of the array, so the alignment is that of `points`), and masks the points of the group outside its piece -- a cloud may
// start anywhere in a group.  The group that would read past the array's end, and a `points` that is not 16-byte aligned (a view),
// take the same points with three scalar loads each.  A wave reads 3 KiB of consecutive bytes per group round either way.
// The worst case for the atomics is every point in one cell: the 64 lanes of a wave then hit one address and the LDS serialises them
// (bank conflicts of a spread-out cloud cost at most the few lanes that share a bank); profiles/occupancy_jsd.txt holds both.
// The cell arithmetic must not be contracted: the file is compiled with fp contract(off), and t + 0.5f stays an addition.
constexpr int OCC_BLOCK = 1024;             // threads of a k_point_occupancy workgroup
constexpr int OCC_POINTS = 16384;           // points a piece holds at least (while there are workgroups left): 4 group rounds
constexpr int OCC_MAX_WG = 256;             // workgroups a launch splits its histograms into at most: one a CU of an MI355X
constexpr int JSD_BLOCK = 256;              // T of the header: the order of the divergence's sum

namespace {

struct OccPlan {
    int nb, S;                              // histograms, pieces a histogram
    long long P, per;                       // points a histogram, points a piece (a multiple of 4)
};

OccPlan occupancy_plan(int B, int N, int per_cloud) {
    OccPlan p;
    p.nb = per_cloud ? B : 1;
    p.P = per_cloud ? (long long)N : (long long)B * N;
    const long long want = (p.P + OCC_POINTS - 1) / OCC_POINTS, room = OCC_MAX_WG / p.nb > 1 ? OCC_MAX_WG / p.nb : 1;
    p.S = (int)(want < room ? want : room);
    p.per = ((p.P + p.S - 1) / p.S + 3) & ~3LL;
    return p;
}

__device__ __forceinline__ int occ_axis(float x, float lo, float inv, float top) {
    const float t = (x - lo) * inv;
    const float u = floorf(t + 0.5f);
    return (int)fminf(fmaxf(u, 0.0f), top);
}

__device__ __forceinline__ void occ_point(float x, float y, float z, float lo, float inv, float top, int R, unsigned* hist, int& dropped) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) {
        ++dropped;
        return;
    }
    const int c = (occ_axis(x, lo, inv, top) * R + occ_axis(y, lo, inv, top)) * R + occ_axis(z, lo, inv, top);   // < R^3 by the clamps
    atomicAdd(&hist[c], 1u);
}

__global__ __launch_bounds__(OCC_BLOCK) void k_point_occupancy(const float* __restrict__ pts, long long total, long long P, long long per,
                                                                int R, float lo, float inv, int wide, int32_t* __restrict__ out,
                                                                int32_t* __restrict__ dropped_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned occ_hist[];      // [R^3]
    __shared__ int s_dropped;
    const int tid = threadIdx.x, cells = R * R * R;
    const size_t w = (size_t)blockIdx.y * gridDim.x + blockIdx.x;           // the piece: its slice of `out`, its word of `dropped_out`
    for (int i = tid; i < cells; i += OCC_BLOCK) occ_hist[i] = 0u;
    if (tid == 0) s_dropped = 0;
    __syncthreads();
    const long long h0 = (long long)blockIdx.y * P;                          // the histogram's first point
    const long long f0 = h0 + (long long)blockIdx.x * per;                   // the piece [f0, f1)
    const long long f1 = f0 + per < h0 + P ? f0 + per : h0 + P;
    const float top = (float)(R - 1);
    int nd = 0;
    for (long long g = (f0 >> 2) + tid; 4 * g < f1; g += OCC_BLOCK) {        // aligned groups of four points that meet the piece
        const long long first = 4 * g;
        if (wide && first + 4 <= total) {
            const float4* q = reinterpret_cast<const float4*>(pts + 12 * (size_t)g);
            const float4 a = q[0], b = q[1], c = q[2];
            if (first >= f0 && first < f1) occ_point(a.x, a.y, a.z, lo, inv, top, R, occ_hist, nd);
            if (first + 1 >= f0 && first + 1 < f1) occ_point(a.w, b.x, b.y, lo, inv, top, R, occ_hist, nd);
            if (first + 2 >= f0 && first + 2 < f1) occ_point(b.z, b.w, c.x, lo, inv, top, R, occ_hist, nd);
            if (first + 3 >= f0 && first + 3 < f1) occ_point(c.y, c.z, c.w, lo, inv, top, R, occ_hist, nd);
        } else {
            for (int k = 0; k < 4; ++k) {
                const long long p = first + k;
                if (p < f0 || p >= f1) continue;                             // f1 <= total: the loads below stay inside the array
                const float* q = pts + 3 * (size_t)p;
                occ_point(q[0], q[1], q[2], lo, inv, top, R, occ_hist, nd);
            }
        }
    }
    if (nd) atomicAdd(&s_dropped, nd);
    __syncthreads();
    int32_t* o = out + w * (size_t)cells;
    for (int i = tid; i < cells; i += OCC_BLOCK) o[i] = (int32_t)occ_hist[i];
    if (tid == 0 && dropped_out) dropped_out[w] = s_dropped;
}

// counts[b, c] = the sum over the S pieces of histogram b, dropped[b] likewise: one thread per output word, every word written once
__global__ __launch_bounds__(256) void k_occupancy_reduce(const int32_t* __restrict__ part, const int32_t* __restrict__ part_dropped, int S,
                                                           int cells, int nb, int32_t* __restrict__ counts, int32_t* __restrict__ dropped) {
    const long long n_out = (long long)nb * cells, i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_out) {
        const long long b = i / cells, c = i - b * cells;
        const int32_t* p = part + (size_t)b * S * cells + c;
        int32_t sum = 0;
#pragma unroll 8                                                             // eight loads in flight: the pieces are independent
        for (int s = 0; s < S; ++s) sum += p[(size_t)s * cells];
        counts[i] = sum;
    } else if (dropped && i - n_out < nb) {
        const long long b = i - n_out;
        int32_t sum = 0;
        for (int s = 0; s < S; ++s) sum += part_dropped[b * S + s];
        dropped[b] = sum;
    }
}

// the Jensen-Shannon divergence of two histograms: one workgroup, the totals as 64-bit integers, the sum in double in the header's order
__global__ __launch_bounds__(JSD_BLOCK) void k_occupancy_jsd(const int32_t* __restrict__ ca, const int32_t* __restrict__ cb, int cells,
                                                              double* __restrict__ jsd) {
    __shared__ long long tot_a[JSD_BLOCK], tot_b[JSD_BLOCK];
    __shared__ double part[JSD_BLOCK];
    const int tid = threadIdx.x;
    long long sa = 0, sb = 0;
    for (int c = tid; c < cells; c += JSD_BLOCK) sa += ca[c], sb += cb[c];
    tot_a[tid] = sa, tot_b[tid] = sb;
    __syncthreads();
    for (int h = JSD_BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) tot_a[tid] += tot_a[tid + h], tot_b[tid] += tot_b[tid + h];
        __syncthreads();
    }
    const long long A = tot_a[0], B = tot_b[0];
    if (A == 0 || B == 0) {                                                  // uniform: every thread leaves here
        if (tid == 0) *jsd = __longlong_as_double(0x7ff8000000000000LL);
        return;
    }
    const double dA = (double)A, dB = (double)B;
    double acc = 0.0;
    for (int c = tid; c < cells; c += JSD_BLOCK) {
        const int a = ca[c], b = cb[c];
        const double p = (double)a / dA, q = (double)b / dB;
        const double m = 0.5 * (p + q);
        const double tp = a > 0 ? p * log2(p / m) : 0.0;
        const double tq = b > 0 ? q * log2(q / m) : 0.0;
        acc += 0.5 * (tp + tq);
    }
    part[tid] = acc;
    __syncthreads();
    for (int h = JSD_BLOCK / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (tid == 0) *jsd = part[0];
}

}  // namespace

size_t point_occupancy_workspace_bytes(int B, int N, int R, int per_cloud) {
    const OccPlan p = occupancy_plan(B, N, per_cloud);
    return p.S == 1 ? 16 : (size_t)p.nb * p.S * ((size_t)R * R * R + 1) * sizeof(int32_t);
}

void launch_point_occupancy(const float* pts, int B, int N, int R, float lo, float inv_spacing, int per_cloud, int32_t* counts,
                            int32_t* dropped, void* ws, hipStream_t s) {
    const OccPlan p = occupancy_plan(B, N, per_cloud);
    const int cells = R * R * R;
    const size_t lds = (size_t)cells * sizeof(unsigned);
    // the most a launch may ask for: 32^3 words, which leaves the kernel's one static word inside the 160 KiB
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_point_occupancy), hipFuncAttributeMaxDynamicSharedMemorySize, 32 * 32 * 32 * 4);
    const int wide = reinterpret_cast<uintptr_t>(pts) % 16 == 0;
    int32_t* part = static_cast<int32_t*>(ws);
    int32_t* part_dropped = part + (size_t)p.nb * p.S * cells;
    prof_mark_begin(PROF_POINT_OCCUPANCY, 0.0, s);
    hipLaunchKernelGGL(k_point_occupancy, dim3(p.S, p.nb), dim3(OCC_BLOCK), lds, s, pts, (long long)B * N, p.P, p.per, R, lo, inv_spacing, wide,
                       p.S == 1 ? counts : part, p.S == 1 ? dropped : part_dropped);
    prof_mark_end(s);
    if (p.S == 1) return;
    const long long words = (long long)p.nb * cells + p.nb;
    prof_mark_begin(PROF_OCCUPANCY_REDUCE, 0.0, s);
    hipLaunchKernelGGL(k_occupancy_reduce, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, part, part_dropped, p.S, cells, p.nb, counts,
                       dropped);
    prof_mark_end(s);
}

void launch_occupancy_jsd(const int32_t* counts_a, const int32_t* counts_b, int R, double* jsd, hipStream_t s) {
    prof_mark_begin(PROF_OCCUPANCY_JSD, 0.0, s);
    hipLaunchKernelGGL(k_occupancy_jsd, dim3(1), dim3(JSD_BLOCK), 0, s, counts_a, counts_b, R * R * R, jsd);
    prof_mark_end(s);
}

}  // namespace icn
