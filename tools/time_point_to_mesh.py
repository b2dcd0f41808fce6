"""Time the point-to-mesh distance and its backward in training use (developer tool; GPU only): Point2Mesh_Loss forward + backward
on an I5 / batch-36 network-sized input against a synthetic batch as the reference surface (10 242 points against 20 480 triangles
per mesh), gradients to the input AND to the reference vertices so that both backward kernels run.  Per-kernel times from the
library's HIP-event profiler (icn_profile_start / icn_profile_stop), median over the repetitions after two warm-ups.

    python tools/time_point_to_mesh.py [repetitions=10] [batch=36] [subdivisions=5] [search=both] [workload=all]

search: brute | grid | both.  With `both` the two searches run in the same process, alternating step by step, so that they see the
same clocks and the same neighbours on the machine; the yardstick for the grid search is k_point_to_mesh of that same run.
workload: the point cloud against the reference surface (synthetic batch, seed 2):
    shape   another synthetic batch (seed 1): a different shape, rms distance ~0.06 of a unit-sized mesh
    near    the reference's own vertices + 0.01 Gaussian noise: the loss near convergence
    far     a Gaussian cloud, sigma 0.8, mostly far outside the mesh: the hostile case for a spatial index
    all     the three, one after the other
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
SEARCH = sys.argv[4] if len(sys.argv) > 4 else 'both'
WORKLOAD = sys.argv[5] if len(sys.argv) > 5 else 'all'
if SEARCH not in ('brute', 'grid', 'both') or WORKLOAD not in ('shape', 'near', 'far', 'all'):
    sys.exit(__doc__)
SEARCHES = ('brute', 'grid') if SEARCH == 'both' else (SEARCH,)
BUILD = ('k_p2m_grid_bounds', 'k_p2m_grid_count', 'k_p2m_grid_scan', 'k_p2m_grid_fill')
FORWARD = {'brute': ('k_point_to_mesh',), 'grid': BUILD + ('k_p2m_grid_query',)}
BACKWARD = ('k_point_to_mesh_bwd_point', 'k_point_to_mesh_bwd_vertex')

y, _ = data.synthetic_batch(B, R, seed=2, device='cuda')
ref_v = grid_to_vertices(y, R)
faces = torch.from_numpy(geometry.get_ico_faces(R)).cuda()
print('points %d, vertices %d, faces %d per mesh, batch %d, %d repetitions after 2 warm-ups'
      % (ref_v.shape[1], ref_v.shape[1], faces.shape[0], B, REPS))


def cloud(name):
    g = torch.Generator(device='cuda').manual_seed(3)
    if name == 'shape':
        return data.synthetic_batch(B, R, seed=1, device='cuda')[0]
    if name == 'near':
        return y + 0.01 * torch.randn(y.shape, generator=g, device='cuda')
    return 0.8 * torch.randn(y.shape, generator=g, device='cuda')


def med(t):
    return statistics.median(t)


def line(name, t):
    print('  %-28s median %9.3f ms   min %9.3f   max %9.3f' % (name, med(t), min(t), max(t)))


def run(name):
    x = cloud(name)
    crits = {s: Point2Mesh_Loss(R, search=s) for s in SEARCHES}

    def step(s):
        inp, ref = x.detach().requires_grad_(True), ref_v.detach().requires_grad_(True)
        loss = crits[s](inp, ref, faces)
        loss.backward()
        return loss
    for _ in range(2):
        for s in SEARCHES:
            step(s)
    torch.cuda.synchronize()
    times = {s: {} for s in SEARCHES}
    wall = {s: [] for s in SEARCHES}
    loss = {}
    for _ in range(REPS):
        for s in SEARCHES:                                  # alternating: brute, grid, brute, grid, ...
            _lib.profile_start(16)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss[s] = step(s)
            e1.record()
            for e in _lib.profile_stop():                   # synchronises the device
                times[s].setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
            wall[s].append(e0.elapsed_time(e1))
    rms = float(loss[SEARCHES[0]].detach().sqrt())
    print('workload %s: loss %.6g (rms distance %.4f)' % (name, float(loss[SEARCHES[0]].detach()), rms))
    fwd = {}
    for s in SEARCHES:
        print(' search=%s' % s)
        for k in FORWARD[s] + BACKWARD:
            line(k, times[s][k])
        if s == 'grid':
            line('grid build (4 kernels)', [sum(v) for v in zip(*(times[s][k] for k in BUILD))])
        fwd[s] = [sum(v) for v in zip(*(times[s][k] for k in FORWARD[s]))]
        line('forward kernels together', fwd[s])
        line('backward kernels together', [a + b for a, b in zip(*(times[s][k] for k in BACKWARD))])
        line('Point2Mesh_Loss step', wall[s])
    if len(SEARCHES) == 2:
        assert float(loss['brute'].detach()) == float(loss['grid'].detach()), 'the two searches disagree'
        print(' grid forward (build + query) / k_point_to_mesh = %.4f  (%.1f x %s)'
              % (med(fwd['grid']) / med(fwd['brute']), max(med(fwd['brute']) / med(fwd['grid']), med(fwd['grid']) / med(fwd['brute'])),
                 'faster' if med(fwd['grid']) < med(fwd['brute']) else 'SLOWER'))


for w in (('shape', 'near', 'far') if WORKLOAD == 'all' else (WORKLOAD,)):
    run(w)
