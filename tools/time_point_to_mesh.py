"""Time the point-to-mesh distance and its backward in training use (developer tool; GPU only): Point2Mesh_Loss forward + backward
on an I5 / batch-36 network-sized input against a second synthetic batch as the reference surface (10 242 points against 20 480
triangles per mesh), gradients to the input AND to the reference vertices so that both backward kernels run.  Per-kernel times
from the library's HIP-event profiler (icn_profile_start / icn_profile_stop), median over the repetitions after a warm-up.

    python tools/time_point_to_mesh.py [repetitions=10] [batch=36] [subdivisions=5]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from geniconet_amd import _lib, data, geometry  # noqa: E402
from geniconet_amd.losses import Point2Mesh_Loss, grid_to_vertices  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5

x, _ = data.synthetic_batch(B, R, seed=1, device='cuda')
y, _ = data.synthetic_batch(B, R, seed=2, device='cuda')
ref_v = grid_to_vertices(y, R)
faces = torch.from_numpy(geometry.get_ico_faces(R)).cuda()
crit = Point2Mesh_Loss(R)
print('points %d, vertices %d, faces %d per mesh, batch %d' % (ref_v.shape[1], ref_v.shape[1], faces.shape[0], B))


def step():
    inp, ref = x.detach().requires_grad_(True), ref_v.detach().requires_grad_(True)
    loss = crit(inp, ref, faces)
    loss.backward()
    return loss


for _ in range(2):
    step()
torch.cuda.synchronize()
times, wall = {}, []
for _ in range(REPS):
    _lib.profile_start(16)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    loss = step()
    e1.record()
    for e in _lib.profile_stop():                       # synchronises the device
        times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
    wall.append(e0.elapsed_time(e1))
print('loss %.6g' % float(loss.detach()))
for k in ('k_point_to_mesh', 'k_point_to_mesh_bwd_point', 'k_point_to_mesh_bwd_vertex'):
    t = times[k]
    print('%-28s median %9.3f ms   min %9.3f   max %9.3f   (%d repetitions)' % (k, statistics.median(t), min(t), max(t), len(t)))
bwd = [a + b for a, b in zip(times['k_point_to_mesh_bwd_point'], times['k_point_to_mesh_bwd_vertex'])]
print('%-28s median %9.3f ms' % ('backward kernels together', statistics.median(bwd)))
print('%-28s median %9.3f ms   (forward + backward incl. grid_to_vertices, the mean and their gradients)'
      % ('Point2Mesh_Loss step', statistics.median(wall)))
