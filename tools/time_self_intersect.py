"""Time the self-intersection kernel (developer tool; GPU only), all in ONE process at I5 / batch 36 by default:
  * k_mesh_self_intersect on two inputs: the unit icosphere, where almost every pair dies at the box test, and the same sphere with
    Gaussian vertex noise of sigma 0.05, where many boxes overlap and the exact tests in double run,
  * beside it k_point_to_mesh on the same sizes (as many points as faces, the vertices of the same meshes against the same faces): the
    only other kernel here whose cost is F^2-shaped, so it is the yardstick,
  each from the library's HIP-event profiler (icn_profile_start / icn_profile_stop), and how many pairs pass the box test,
  * metrics.self_intersections end to end on the HIP path, and the torch float64 formulation on the same device -- at batch 1, because
    it takes seconds per mesh at this size; the HIP path is timed at batch 1 beside it.
HIP events; median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_self_intersect.py [repetitions=10] [batch=36] [subdivisions=5] [output=profiles/self_intersect.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, geometry, metrics  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'profiles', 'self_intersect.txt')
SIGMA = 0.05
TORCH_REPS = min(REPS, 3)
TORCH_ROWS = 64                                                              # rows of the torch formulation per chunk at batch 1
KERNELS = ('k_mesh_self_intersect', 'k_point_to_mesh')

record = []


def say(text):
    print(text, flush=True)
    record.append(text)


ico_v, ico_f = geometry.get_icosahedral_grid(R)
f32 = torch.from_numpy(ico_f).to(device='cuda', dtype=torch.int32)
clean = torch.from_numpy(ico_v).to(device='cuda', dtype=torch.float32)[None].repeat(B, 1, 1).contiguous()
noisy = (clean + SIGMA * torch.randn(clean.shape, generator=torch.Generator(device='cuda').manual_seed(3), device='cuda')).contiguous()
V, F = clean.shape[1], f32.shape[0]
say('Self-intersection count of meshes (icn_mesh_self_intersect, metrics.self_intersections)')
say('%s, libicn sources %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12]))
say('I%d, batch %d: %d vertices, %d faces, %.3g pairs of faces per launch; %d repetitions after 2 warm-ups, HIP events'
    % (R, B, V, F, B * F * (F - 1) / 2, REPS))


def line(name, t):
    say('  %-66s median %10.4f ms   (%10.4f - %10.4f)' % (name, statistics.median(t), min(t), max(t)))
    return statistics.median(t)


def timed(name, call, reps=REPS, warm=2):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return line(name, t)


def overlapping_boxes(v):
    """Pairs i < j of mesh 0 that share no vertex and whose fp32 boxes overlap: the pairs that reach the double arithmetic."""
    tri = v[0][f32.long()]
    lo, hi = tri.amin(1), tri.amax(1)
    ids = f32.long()
    count = 0
    for at in range(0, F, 512):
        over = ((lo[at:at + 512, None] <= hi[None]) & (lo[None] <= hi[at:at + 512, None])).all(-1)
        shared = (ids[at:at + 512, None, :, None] == ids[None, :, None, :]).any(-1).any(-1)
        count += int((over & ~shared).sum())
    return count // 2


say('kernels (per launch, the library\'s event profiler), %d points per mesh for k_point_to_mesh:' % F)
med = {}
for name, v in (('unit icosphere', clean), ('sigma %g vertex noise' % SIGMA, noisy)):
    points = v[:, :F].contiguous() if V >= F else v.repeat(1, (F + V - 1) // V, 1)[:, :F].contiguous()

    def both():
        metrics._self_intersections_unchecked(v, f32)
        metrics._point_to_mesh_unchecked(points, v, f32)
    for _ in range(2):
        both()
    torch.cuda.synchronize()
    times = {}
    for _ in range(REPS):
        _lib.profile_start(16)
        both()
        for e in _lib.profile_stop():                                        # synchronises the device
            if e['launches']:
                times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
    pairs, hits = metrics._self_intersections_unchecked(v, f32)
    say(' %s: %d intersecting pairs in mesh 0, %.4f of its faces hit; %d of its %d pairs pass the id and box tests'
        % (name, int(pairs[0]), float((hits[0] > 0).sum()) / F, overlapping_boxes(v), F * (F - 1) // 2))
    for k in KERNELS:
        med[name, k] = line(k, times[k])
    say('  k_mesh_self_intersect / k_point_to_mesh: %.2f' % (med[name, KERNELS[0]] / med[name, KERNELS[1]]))
names = [n for n, _ in med][::2]
say('  the exact tests: the noisy input takes %.2f x the clean one' % (med[names[1], KERNELS[0]] / med[names[0], KERNELS[0]]))

say('self_intersections end to end (the unchecked form: no read-back), HIP path:')
timed('batch %d, unit icosphere' % B, lambda: metrics._self_intersections_unchecked(clean, f32))
timed('batch %d, sigma %g vertex noise' % (B, SIGMA), lambda: metrics._self_intersections_unchecked(noisy, f32))
say('the torch float64 formulation on the device against the HIP path, batch 1, sigma %g vertex noise (%d repetitions, %d rows per chunk):'
    % (SIGMA, TORCH_REPS, TORCH_ROWS))
one = noisy[:1].contiguous()
a = timed('HIP, batch 1', lambda: metrics._self_intersections_unchecked(one, f32))
b = timed('torch formulation, batch 1', lambda: metrics._torch_self_intersections(one, f32, chunk=TORCH_ROWS), reps=TORCH_REPS, warm=1)
say('  torch / HIP: %.0f' % (b / a))
same = torch.equal(metrics._torch_self_intersections(one, f32, chunk=TORCH_ROWS), metrics._self_intersections_unchecked(one, f32)[1])
say('  the two give %s' % ('the same integers' if same else 'DIFFERENT integers'))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
