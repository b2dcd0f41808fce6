"""Time the cotangent Laplacian / Willmore energy kernels and the Willmore term of the surface loss (developer tool; GPU only), all in
ONE process at I5 / batch 36 by default:
  * the four kernels of icn_mesh_willmore_fwd / icn_mesh_willmore_bwd (the operator with the block sums, finish, per-vertex
    upstreams, incidence-gather backward), each from the library's HIP-event profiler (icn_profile_start / icn_profile_stop),
  * metrics.willmore_energy and metrics.cotangent_laplacian through autograd, the HIP path against the torch formulation on the same
    device, forward and forward + backward,
  * losses.Surface_Loss forward + backward without and with factor_willmore, for samples = 0 and samples = S, search 'grid',
  * the accuracy figures of tests/test_mesh_curvature.py on its own inputs, in the terms of its bars, beside the fp32 torch
    formulation's on the CPU (the test allows the HIP kernels four times the worst of those).
HIP events; median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_mesh_curvature.py [repetitions=10] [batch=36] [subdivisions=5] [samples=10242] [output=profiles/mesh_curvature.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, geometry, losses, metrics  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
S = int(sys.argv[4]) if len(sys.argv) > 4 else 10242
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, 'profiles', 'mesh_curvature.txt')
F_REG = (0.1, 0.01, 0.1)
KERNELS = ('k_mesh_cotlap_fwd', 'k_mesh_willmore_finish', 'k_mesh_willmore_upstream', 'k_mesh_cotlap_bwd')

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
de = torch.randn(B, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
dl = torch.randn(B, V, 3, generator=torch.Generator(device='cuda').manual_seed(5), device='cuda')
da = torch.randn(B, V, generator=torch.Generator(device='cuda').manual_seed(6), device='cuda')
say('Cotangent Laplacian and Willmore energy of meshes (icn_mesh_cotlap_* / icn_mesh_willmore_*) and losses.Surface_Loss(factor_willmore)')
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


def energy_step(fn, backward=True):
    v = out.detach().requires_grad_(backward)
    w = fn(v)
    if backward:
        (w * de).sum().backward()


def operator_step(fn, backward=True):
    v = out.detach().requires_grad_(backward)
    lap, area = fn(v)
    if backward:
        ((lap * dl).sum() + (area * da).sum()).backward()


hip_w = lambda v: metrics._willmore_energy_unchecked(v, f32, table)            # noqa: E731
hip_w_no_table = lambda v: metrics._willmore_energy_unchecked(v, f32)          # noqa: E731
plain_w = lambda v: metrics._torch_willmore_energy(v, f32)                     # noqa: E731
hip_l = lambda v: metrics._cotangent_laplacian_unchecked(v, f32, table)        # noqa: E731
plain_l = lambda v: metrics._torch_cotangent_laplacian(v, f32)                 # noqa: E731

say('kernels (per launch, the library\'s event profiler), willmore_energy forward + backward:')
for _ in range(2):
    energy_step(hip_w)
torch.cuda.synchronize()
times = {}
for _ in range(REPS):
    _lib.profile_start(16)
    energy_step(hip_w)
    for e in _lib.profile_stop():                                          # synchronises the device
        times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
for k in KERNELS:
    line(k, times[k])
line('forward + backward, kernels together', [sum(ts) for ts in zip(*(times[k] for k in KERNELS))])

say('willmore_energy through autograd, HIP path against the torch formulation on the device:')
a = timed('HIP, forward', lambda: energy_step(hip_w, False))
b = timed('HIP, forward + backward (table passed)', lambda: energy_step(hip_w))
timed('HIP, forward + backward (table built on entry)', lambda: energy_step(hip_w_no_table))
c = timed('torch formulation, forward', lambda: energy_step(plain_w, False))
d = timed('torch formulation, forward + backward', lambda: energy_step(plain_w))
say('  torch / HIP: forward %.1f, forward + backward %.1f' % (c / a, d / b))
say('  the HIP forward + backward %s the torch formulation\'s' % ('beats' if b < d else 'does NOT beat'))
say('cotangent_laplacian through autograd, random upstreams on both outputs:')
a = timed('HIP, forward', lambda: operator_step(hip_l, False))
b = timed('HIP, forward + backward (table passed)', lambda: operator_step(hip_l))
c = timed('torch formulation, forward', lambda: operator_step(plain_l, False))
d = timed('torch formulation, forward + backward', lambda: operator_step(plain_l))
say('  torch / HIP: forward %.1f, forward + backward %.1f' % (c / a, d / b))
say('  the HIP forward + backward %s the torch formulation\'s' % ('beats' if b < d else 'does NOT beat'))

say('Surface_Loss forward + backward (factors 1 / 1, regularisers %s, edge_length 0.03, search \'grid\'), output = 0.9 target + 0.01 noise:' % (F_REG,))
for samples in (0, S):
    for fw in (0.0, 0.1):
        crit = losses.Surface_Loss(R, 1.0, 1.0, *F_REG, edge_length=0.03, search='grid', samples=samples, factor_willmore=fw).cuda()

        def surface_step():
            inp = near.detach().requires_grad_(True)
            crit(inp, target).backward()
        timed('samples=%d, factor_willmore=%g' % (samples, fw), surface_step)
        say('    p2m %.3g, m2p %.3g, regulariser %.3g, total %.3g' % tuple(v for k, v in enumerate(crit.get_last_losses()) if k != 3)
            + ', mean W / 4 pi %.4f' % (float(crit.last_willmore) / 12.566370614359172))

say('accuracy on the inputs of tests/test_mesh_curvature.py (B = 3), u = 2^-24; lap in u sum|e|, varea in u varea, the rest relative:')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_mesh_curvature as tmc  # noqa: E402
keys = ('lap', 'varea', 'w') + tuple('d_' + term for term in tmc.TERMS)
say('  bars (4 x the worst of the fp32 torch formulation on the CPU): ' + ', '.join('%s %.3g' % (k, tmc._bars()[k]) for k in keys))
worst = {}
for fam in tmc.FAMILIES:
    case = tmc._case(*fam)
    e = tmc._errors(case, *tmc._hip_forward(case), {term: tmc._grad(case, term, torch.float32, 'cuda') for term in tmc.TERMS})
    say('  r = %d, perturbed %4g, shift %4g: HIP   ' % fam + ', '.join('%s %.3g' % (k, e[k]) for k in keys))
    say('  %36s CPU   ' % '' + ', '.join('%s %.3g' % (k, case['cpu'][k]) for k in keys))
    for k in keys:
        if k in ('lap', 'varea', 'w') or fam[1] > 0:
            worst[k] = max(worst.get(k, 0.0), float(e[k]))
say('  worst on the device (gradients over the perturbed families): ' + ', '.join('%s %.3g' % (k, worst[k]) for k in keys))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
