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

}  // namespace icn
