"""Time the sign of the point-to-mesh distance and what is built on it (developer tool; GPU only), all in ONE process at I5 / batch 36
by default, one point per vertex:
  * k_p2m_sign beside the searches it rides on (k_point_to_mesh; the k_p2m_grid_* build and query) and beside
    k_mesh_angle_defect_fwd, the yardstick gather over the same incidence table, each from the library's HIP-event profiler
    (icn_profile_start / icn_profile_stop) in the same call, for the workloads `near` (the reference's vertices + 0.01 noise, rms
    distance 0.01) and `shape` (another synthetic batch, rms distance ~0.06) of tools/time_point_to_mesh.py,
  * signed_point_to_mesh_distance end to end (the unchecked form: search + sign + the root), both searches, by device events,
  * volumetric_iou of one I5 pair at resolution 32 and 64, both searches, by the host clock around the call (it ends in a read-back).
Median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_signed_distance.py [repetitions=10] [batch=36] [subdivisions=5] [output=profiles/signed_distance.txt]
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, geometry, losses, metrics  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'profiles', 'signed_distance.txt')
BUILD = ('k_p2m_grid_bounds', 'k_p2m_grid_count', 'k_p2m_grid_scan', 'k_p2m_grid_fill')
FORWARD = {'brute': ('k_point_to_mesh',), 'grid': BUILD + ('k_p2m_grid_query',)}

record = []


def say(text):
    print(text, flush=True)
    record.append(text)


def line(name, t):
    say('  %-58s median %9.4f ms   (%9.4f - %9.4f)' % (name, statistics.median(t), min(t), max(t)))
    return statistics.median(t)


y, _ = data.synthetic_batch(B, R, seed=2, device='cuda')
ref_v = losses.grid_to_vertices(y, R).contiguous()
f32 = torch.from_numpy(geometry.get_ico_faces(R)).to(device='cuda', dtype=torch.int32)
V, F = ref_v.shape[1], f32.shape[0]
tables = metrics.signed_distance_tables(f32, V)
say('Sign of the point-to-mesh distance (icn_point_to_mesh_sign), signed_point_to_mesh_distance and volumetric_iou')
say('%s, libicn sources %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12]))
say('I%d, batch %d: %d points, %d vertices, %d faces per mesh; %d repetitions after 2 warm-ups' % (R, B, V, V, F, REPS))


def cloud(name):
    g = torch.Generator(device='cuda').manual_seed(3)
    if name == 'near':
        return (ref_v + 0.01 * torch.randn(ref_v.shape, generator=g, device='cuda')).contiguous()
    return losses.grid_to_vertices(data.synthetic_batch(B, R, seed=1, device='cuda')[0], R).contiguous()


def signed(points, search):
    return metrics._signed_point_to_mesh_distance_unchecked(points, ref_v, f32, tables, search)[0]


for name in ('near', 'shape'):
    pts = cloud(name)

    def step(search):
        phi = signed(pts, search)
        metrics._angle_defect_unchecked(ref_v, f32, tables[1:])
        return phi
    for _ in range(2):
        for s in ('brute', 'grid'):
            step(s)
    torch.cuda.synchronize()
    times = {s: {} for s in ('brute', 'grid')}
    for _ in range(REPS):
        for s in ('brute', 'grid'):                                          # alternating: the same clocks, the same neighbours
            _lib.profile_start(32)
            phi = step(s)
            for e in _lib.profile_stop():                                      # synchronises the device
                times[s].setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
    say('workload %s: rms distance %.4f, %.1f %% of the points inside; kernels per launch (the library\'s event profiler):'
        % (name, float((phi * phi).mean().sqrt()), 100 * float((phi < 0).float().mean())))
    med = {}
    for s in ('brute', 'grid'):
        say(' search=%s' % s)
        for k in FORWARD[s] + ('k_p2m_sign', 'k_mesh_angle_defect_fwd'):
            med[s, k] = line(k, times[s][k])
    sign = statistics.median(times['brute']['k_p2m_sign'] + times['grid']['k_p2m_sign'])
    gather = statistics.median(times['brute']['k_mesh_angle_defect_fwd'] + times['grid']['k_mesh_angle_defect_fwd'])
    grid = sum(med['grid', k] for k in FORWARD['grid'])
    say('  k_p2m_sign / k_mesh_angle_defect_fwd %.2f; k_p2m_sign is %.3f of the brute search and %.3f of the grid search (build + query %.4f ms)'
        % (sign / gather, sign / med['brute', 'k_point_to_mesh'], sign / grid, grid))
    say(' signed_point_to_mesh_distance end to end (unchecked: search + sign + root), device events:')
    for s in ('brute', 'grid'):
        t = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            signed(pts, s)
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1))
        line('search=%s' % s, t)

say('volumetric_iou of one I%d pair (mesh 0 against its 0.9-scaled copy: 0.729), host clock around the call:' % R)
faces = f32.long()
for resolution in (32, 64):
    for s in ('brute', 'grid'):
        t = []
        for k in range(2 + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            iou = metrics.volumetric_iou(0.9 * ref_v[0], ref_v[0], faces, resolution=resolution, search=s)
            t.append((time.perf_counter() - t0) * 1e3)
        line('resolution=%d, search=%s: IoU %.5f' % (resolution, s, iou), t[2:])

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
