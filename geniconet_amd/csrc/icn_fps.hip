// Farthest point sampling of batched point clouds (icn_farthest_points in include/icn_fps.h): S well-spread points of every cloud, the
// subsets the evaluation tables match instead of whole clouds (geniconet_amd/sampling.py: farthest_point_sample, farthest_points).
// The definition -- distance, the early case, the loop, the lowest-index rule -- is stated once in include/icn_fps.h and restated in
// torch by sampling._torch_farthest_point_sample; fminf, the max and the argmax with the lowest index do not depend on the order of
// evaluation, so idx and cover are fixed bit for bit however the scan is split.
// k_farthest_points<PPT>: grid (B); ONE WORKGROUP OF 512 THREADS OWNS ONE CLOUD from start to finish.  Nothing waits for another
// workgroup, nothing spins on memory, there are no atomics, the launch is an ordinary one.  The only loop whose trip count depends on
// an argument is s < S; a cloud with a non-finite coordinate leaves by the early case before it.
// Thread t holds points t, t + 512, ... t + 512 (PPT - 1) and their dist IN REGISTERS, PPT a compile-time constant the host picks by N
// (FPS_BUCKETS), so every array below is indexed by unrolled constants and nothing goes to scratch.  A slot past N holds the
// coordinates of the start point: its dist is 0 from step 0 on and its index is above every point's, so it never wins -- while cover > 0
// it is below the maximum, and once cover == 0 the lowest index wins, which is a point's -- and the loop needs no validity test.
// ONE STEP, one barrier:
//   every thread updates its dist against the centre (3 v_sub_f32, 3 v_mul_f32, 2 v_add_f32, 1 v_min_f32 a point, none fused) and
//   keeps the largest with its slot and coordinates (`>` on slots met in ascending order: the lowest index of the thread);
//   the local maximum becomes one 64-bit key (dist bits << 32) | ~index: dist is never negative and never -0, so a max of keys is the
//   maximum distance with the lowest index.  The key is reduced over the wave by shuffles; the one lane that holds the wave's maximum
//   writes key and coordinates to the wave's LDS slot;
//   after the barrier every thread reads the eight slots and knows cover, the next centre and its coordinates: no second exchange, no
//   global load.  The slots are double-buffered by the parity of s -- a wave writes the slots of step s + 2 only after the barrier of
//   step s + 1, which every wave passes after its reads of step s -- so one barrier a step is enough.
// Thread 0 writes idx and cover.  Registers, scratch (none) and occupancy of every instantiation, and timings on an MI355X:
// profiles/farthest_points.txt (tools/time_fps.py).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icn_launch.h"
#include "icn_mesh_device.h"

#pragma clang fp contract(off)

namespace icn {
namespace {

constexpr int FPS_BLOCK = 512;               // threads of the workgroup that owns a cloud
constexpr int FPS_WAVES = FPS_BLOCK / 64;
constexpr int FPS_MAX_N = 13312;             // FPS_BLOCK x 26 points: the bound of icn_match.h, admits I5

struct __attribute__((aligned(16))) FpsSlot {   // a wave's farthest point: 32 bytes, two 16-byte reads
    unsigned long long key;                  // (dist bits << 32) | ~index
    float x, y, z;
    float pad[3];
};

template <int PPT>
__global__ __launch_bounds__(FPS_BLOCK) void k_farthest_points(const float* __restrict__ pts, int N, int S, int start,
                                                                int* __restrict__ idx, float* __restrict__ cover) {
    __shared__ FpsSlot slot[2][FPS_WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.x;
    const float* P = pts + (size_t)b * N * 3;
    int* idx_b = idx + (size_t)b * S;
    float* cover_b = cover ? cover + (size_t)b * S : nullptr;

    f3 c = load3(P + (size_t)start * 3);                                     // 0 <= start < N (checked by the entry)
    float px[PPT], py[PPT], pz[PPT], dist[PPT];
    int bad = !(__builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z));
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int i = tid + k * FPS_BLOCK;
        const f3 p = i < N ? load3(P + (size_t)i * 3) : c;                   // a slot past N: the start point again, which never wins
        px[k] = p.x, py[k] = p.y, pz[k] = p.z;
        dist[k] = INFINITY;
        bad |= !(__builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z));
    }

    // ---- the case decided before any loop ----
    if (__syncthreads_or(bad)) {
        for (int s = tid; s < S; s += FPS_BLOCK) {
            idx_b[s] = -1;
            if (cover_b) cover_b[s] = NAN;
        }
        return;
    }

    int cur = start;
    for (int s = 0; s < S; ++s) {
        if (tid == 0) idx_b[s] = cur;
        float best = 0.f, bx = 0.f, by = 0.f, bz = 0.f;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const float dx = px[k] - c.x, dy = py[k] - c.y, dz = pz[k] - c.z;
            const float d = fminf(dist[k], (dx * dx + dy * dy) + dz * dz);
            dist[k] = d;
            if (k == 0 || d > best) best = d, bk = k, bx = px[k], by = py[k], bz = pz[k];   // ascending k: the lowest index among equals
        }
        const unsigned long long key = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned)~(unsigned)(tid + bk * FPS_BLOCK);
        unsigned long long top = key;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long other = __shfl_xor(top, d);
            top = other > top ? other : top;
        }
        FpsSlot* mine = &slot[s & 1][wave];
        if (key == top) {                                                    // one lane of the wave: an index occurs once
            mine->key = key;
            mine->x = bx, mine->y = by, mine->z = bz;
        }
        __syncthreads();
        const FpsSlot* all = slot[s & 1];
        unsigned long long win = all[0].key;
        c = {all[0].x, all[0].y, all[0].z};
#pragma unroll
        for (int w = 1; w < FPS_WAVES; ++w) {
            const unsigned long long other = all[w].key;
            if (other > win) {
                win = other;
                c = {all[w].x, all[w].y, all[w].z};
            }
        }
        cur = (int)~(unsigned)win;                                           // a point's index: below N (the head of this file)
        if (tid == 0 && cover_b) cover_b[s] = __uint_as_float((unsigned)(win >> 32));
    }
}

// points a thread holds, by N: the smallest bucket with FPS_BLOCK * PPT >= N
template <int PPT>
void launch_bucket(const float* pts, int B, int N, int S, int start, int* idx, float* cover, hipStream_t s) {
    hipLaunchKernelGGL(k_farthest_points<PPT>, dim3(B), dim3(FPS_BLOCK), 0, s, pts, N, S, start, idx, cover);
}

}  // namespace

bool farthest_points_fits(int N) { return N <= FPS_MAX_N; }

int farthest_points_per_thread(int N) {
    for (int ppt : {1, 2, 6, 13, 21, 26})
        if (N <= FPS_BLOCK * ppt) return ppt;
    return 0;
}

void launch_farthest_points(const float* pts, int B, int N, int S, int start, int* idx, float* cover, hipStream_t s) {
    prof_mark_begin(PROF_FARTHEST_POINTS, 0.0, s);
    switch (farthest_points_per_thread(N)) {
        case 1: launch_bucket<1>(pts, B, N, S, start, idx, cover, s); break;
        case 2: launch_bucket<2>(pts, B, N, S, start, idx, cover, s); break;
        case 6: launch_bucket<6>(pts, B, N, S, start, idx, cover, s); break;
        case 13: launch_bucket<13>(pts, B, N, S, start, idx, cover, s); break;
        case 21: launch_bucket<21>(pts, B, N, S, start, idx, cover, s); break;
        case 26: launch_bucket<26>(pts, B, N, S, start, idx, cover, s); break;
        default: break;                                                      // N > FPS_MAX_N: rejected by the entry
    }
    prof_mark_end(s);
}

}  // namespace icn
