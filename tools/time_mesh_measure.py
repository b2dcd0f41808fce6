"""Time the surface-area / enclosed-volume measure and the volume and area terms of the surface loss (developer tool; GPU only), all in
ONE process at I5 / batch 36 by default:
  * the three kernels of icn_mesh_measure_fwd / icn_mesh_measure_bwd (per-face pass, finish, incidence-gather backward), each from
    the library's HIP-event profiler (icn_profile_start / icn_profile_stop),
  * metrics.mesh_area_volume through autograd, the HIP path against the torch formulation on the same device, forward and
    forward + backward, and the one-off build of the vertex -> corner incidence table,
  * losses.Surface_Loss forward + backward without and with factor_volume / factor_area, for samples = 0 and samples = S, search 'grid',
  * the accuracy figures of tests/test_mesh_measure.py on its own inputs: values in units of the bound's scale, gradients as rel-L2
    against float64 beside the fp32 torch formulation's (the test allows the HIP kernels twice that, floor 1e-6).
HIP events; median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_mesh_measure.py [repetitions=10] [batch=36] [subdivisions=5] [samples=10242] [output=profiles/mesh_measure.txt]
"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, geometry, losses, metrics  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
S = int(sys.argv[4]) if len(sys.argv) > 4 else 10242
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, 'profiles', 'mesh_measure.txt')
F_REG = (0.1, 0.01, 0.1)
KERNELS = ('k_mesh_measure_face', 'k_mesh_measure_finish', 'k_mesh_measure_bwd')

record = []


def say(text):
    print(text, flush=True)
    record.append(text)


x, target = data.synthetic_batch(B, R, seed=2, device='cuda')
near = (0.9 * x + 0.01 * torch.randn(x.shape, generator=torch.Generator(device='cuda').manual_seed(3), device='cuda')).contiguous()
out = losses.grid_to_vertices(near, R).contiguous()
f32 = torch.from_numpy(geometry.get_ico_faces(R)).to(device='cuda', dtype=torch.int32)
V, F = out.shape[1], f32.shape[0]
table = metrics.vertex_face_table(f32, V)
da = torch.randn(B, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
dv = torch.randn(B, generator=torch.Generator(device='cuda').manual_seed(5), device='cuda')
say('Surface area and enclosed volume of meshes (icn_mesh_measure_fwd / icn_mesh_measure_bwd) and losses.Surface_Loss(factor_volume, factor_area)')
say('%s, libicn sources %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12]))
say('I%d, batch %d: %d vertices, %d faces; %d repetitions after 2 warm-ups, HIP events' % (R, B, V, F, REPS))


def line(name, t):
    say('  %-58s median %9.4f ms   (%9.4f - %9.4f)' % (name, statistics.median(t), min(t), max(t)))
    return statistics.median(t)


def timed(name, call):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    t = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return line(name, t)


def step(fn, backward=True):
    v = out.detach().requires_grad_(backward)
    a, vol = fn(v)
    if backward:
        ((a * da).sum() + (vol * dv).sum()).backward()


hip = lambda v: metrics._mesh_area_volume_unchecked(v, f32, table)      # noqa: E731
hip_no_table = lambda v: metrics._mesh_area_volume_unchecked(v, f32)    # noqa: E731
plain = lambda v: metrics._torch_mesh_area_volume(v, f32)               # noqa: E731

say('kernels (per launch, the library\'s event profiler):')
for _ in range(2):
    step(hip)
torch.cuda.synchronize()
times = {}
for _ in range(REPS):
    _lib.profile_start(16)
    step(hip)
    for e in _lib.profile_stop():                                          # synchronises the device
        times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
for k in KERNELS:
    line(k, times[k])
line('forward + backward, kernels together', [sum(ts) for ts in zip(*(times[k] for k in KERNELS))])
say('  (beside the vertex scatters of the Surface_Loss docstring at the same size: k_msample_bwd_vertex about 1.0 ms, '
    'k_fnormal_agree_bwd_vertex 2.04 ms per side)')

say('mesh_area_volume through autograd, HIP path against the torch formulation on the device:')
a = timed('HIP, forward', lambda: step(hip, False))
b = timed('HIP, forward + backward (table passed)', lambda: step(hip))
timed('HIP, forward + backward (table built in the backward)', lambda: step(hip_no_table))
timed('vertex_face_table alone (once per face list)', lambda: metrics.vertex_face_table(f32, V))
c = timed('torch formulation, forward', lambda: step(plain, False))
d = timed('torch formulation, forward + backward', lambda: step(plain))
say('  torch / HIP: forward %.1f, forward + backward %.1f' % (c / a, d / b))
say('  the gather backward %s torch\'s atomic index_put backward' % ('beats' if b < d else 'does NOT beat'))

say('Surface_Loss forward + backward (factors 1 / 1, regularisers %s, edge_length 0.03, search \'grid\'), output = 0.9 target + 0.01 noise:' % (F_REG,))
for samples in (0, S):
    for fv, fa in ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0)):
        crit = losses.Surface_Loss(R, 1.0, 1.0, *F_REG, edge_length=0.03, search='grid', samples=samples, factor_volume=fv, factor_area=fa).cuda()

        def surface_step():
            inp = near.detach().requires_grad_(True)
            crit(inp, target).backward()
        timed('samples=%d, factor_volume=%g, factor_area=%g' % (samples, fv, fa), surface_step)
        say('    p2m %.3g, m2p %.3g, regulariser %.3g, total %.3g' % tuple(v for k, v in enumerate(crit.get_last_losses()) if k != 3)
            + ', l_vol %.3g, l_area %.3g' % (float(crit.last_volume), float(crit.last_area)))

say('accuracy on the inputs of tests/test_mesh_measure.py (B = 3), u = 2^-24:')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_mesh_measure as tmm  # noqa: E402
for mesh, shift in tmm.CASES:
    case = tmm._case(mesh, shift)
    ref = case['ref']
    area, vol = metrics.mesh_area_volume(case['v'].cuda(), case['f'].cuda())
    e_a = (np.abs(area.double().cpu().numpy() - ref['area']) / (tmm.U * ref['area_scale'])).max()
    e_v = (np.abs(vol.double().cpu().numpy() - ref['volume']) / (tmm.U * ref['volume_scale'])).max()
    say('  %-4s shift %4g: values, worst error / (u scale): area %.3f, volume %.3f (the bound: 8 + the final rounding)' % (mesh, shift, e_a, e_v))
    for term in ('area', 'volume', 'both'):
        e_hip = tmm.rel_l2(tmm._grad(case, term, torch.float32, 'cuda').numpy(), case['grad64'][term])
        say('       gradient, %-6s: rel-L2 against float64: HIP %.3g, torch fp32 %.3g' % (term, e_hip, case['e_torch'][term]))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
