"""Time the angle-defect kernels and the Gaussian-curvature term of the surface loss (developer tool; GPU only), all in ONE process at
I5 / batch 36 by default:
  * k_mesh_angle_defect_fwd / _bwd (double arithmetic) beside k_mesh_cotlap_fwd / _bwd (the same gather in fp32) in the same run, each
    from the library's HIP-event profiler (icn_profile_start / icn_profile_stop): the ratio is the price of the double arithmetic,
  * metrics.angle_defect through autograd, the HIP path against the torch formulation on the same device, forward and forward +
    backward,
  * losses.Surface_Loss forward + backward without and with factor_gauss, for samples = 0 and samples = S, search 'grid',
  * the accuracy figures of tests/test_mesh_gauss.py on its own inputs, as the worst ratio to each of its bars, and the Gauss-Bonnet
    miss of the fp32 outputs beside that of an fp32 torch formulation of the same angles.
HIP events; median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_mesh_gauss.py [repetitions=10] [batch=36] [subdivisions=5] [samples=10242] [output=profiles/mesh_gauss.txt]
"""
import math
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
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, 'profiles', 'mesh_gauss.txt')
F_REG = (0.1, 0.01, 0.1)
GAUSS = ('k_mesh_angle_defect_fwd', 'k_mesh_angle_defect_bwd')
COTLAP = ('k_mesh_cotlap_fwd', 'k_mesh_cotlap_bwd')

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
dd = torch.randn(B, V, generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
dl = torch.randn(B, V, 3, generator=torch.Generator(device='cuda').manual_seed(5), device='cuda')
da = torch.randn(B, V, generator=torch.Generator(device='cuda').manual_seed(6), device='cuda')
say('Angle defect / Gaussian curvature of meshes (icn_mesh_angle_defect_fwd / _bwd) and losses.Surface_Loss(factor_gauss)')
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


def defect_step(fn, backward=True):
    v = out.detach().requires_grad_(backward)
    d = fn(v)
    if backward:
        (d * dd).sum().backward()


def operator_step(backward=True):
    v = out.detach().requires_grad_(backward)
    lap, area = metrics._cotangent_laplacian_unchecked(v, f32, table)
    if backward:
        ((lap * dl).sum() + (area * da).sum()).backward()


hip_d = lambda v: metrics._angle_defect_unchecked(v, f32, table)               # noqa: E731
hip_d_no_table = lambda v: metrics._angle_defect_unchecked(v, f32)             # noqa: E731
plain_d = lambda v: metrics._torch_angle_defect(v, f32)                        # noqa: E731

say('kernels (per launch, the library\'s event profiler): the double gathers beside the fp32 gathers of the cotangent operator, one run:')
for _ in range(2):
    defect_step(hip_d)
    operator_step()
torch.cuda.synchronize()
times = {}
for _ in range(REPS):
    _lib.profile_start(16)
    defect_step(hip_d)
    operator_step()
    for e in _lib.profile_stop():                                          # synchronises the device
        times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
med = {k: line(k, times[k]) for k in GAUSS + COTLAP}
say('  double / fp32 gather: forward %.2f, backward %.2f' % (med[GAUSS[0]] / med[COTLAP[0]], med[GAUSS[1]] / med[COTLAP[1]]))

say('angle_defect through autograd, HIP path against the torch formulation (float64) on the device:')
a = timed('HIP, forward', lambda: defect_step(hip_d, False))
b = timed('HIP, forward + backward (table passed)', lambda: defect_step(hip_d))
timed('HIP, forward + backward (table built on entry)', lambda: defect_step(hip_d_no_table))
c = timed('torch formulation, forward', lambda: defect_step(plain_d, False))
d = timed('torch formulation, forward + backward', lambda: defect_step(plain_d))
say('  torch / HIP: forward %.1f, forward + backward %.1f' % (c / a, d / b))
say('  the HIP forward + backward %s the torch formulation\'s' % ('beats' if b < d else 'does NOT beat'))

say('Surface_Loss forward + backward (factors 1 / 1, regularisers %s, edge_length 0.03, search \'grid\'), output = 0.9 target + 0.01 noise:' % (F_REG,))
for samples in (0, S):
    for fg in (0.0, 0.1):
        crit = losses.Surface_Loss(R, 1.0, 1.0, *F_REG, edge_length=0.03, search='grid', samples=samples, factor_gauss=fg).cuda()

        def surface_step():
            inp = near.detach().requires_grad_(True)
            crit(inp, target).backward()
        timed('samples=%d, factor_gauss=%g' % (samples, fg), surface_step)
        say('    p2m %.3g, m2p %.3g, regulariser %.3g, total %.3g' % tuple(v for k, v in enumerate(crit.get_last_losses()) if k != 3)
            + ', l_gauss %.4g' % float(crit.last_gauss))

say('accuracy on the inputs of tests/test_mesh_gauss.py (B = 3): the worst ratio of the device\'s error to the test\'s bar, and Gauss-Bonnet:')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_mesh_gauss as tmg  # noqa: E402


def fp32_total(v, f):
    """sum of the defects with the same angles written in fp32 (atan2 of fp32 cross and dot products), summed in float64."""
    p = [v[:, f[:, k]] for k in range(3)]
    total = torch.zeros(v.shape[:2], device=v.device)
    for k in range(3):
        a_, b_ = p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]
        total = total.index_add(1, f[:, k], torch.atan2(torch.linalg.cross(a_, b_).norm(dim=-1), (a_ * b_).sum(-1)))
    return (2 * math.pi - total).double().sum(1)


worst = [0.0, 0.0]
cases = [('r = %d, perturbed %4g, shift %4g' % fam, tmg._case(*fam)) for fam in tmg.FAMILIES]
cases += [(name, tmg._make_case(*make())) for name, make in (('fan', tmg._fan), ('soup', tmg._soup), ('mixed', tmg._mixed))]
for name, case in cases:
    dev = tmg._hip_defect(case).double().cpu().numpy()
    r_d = tmg._ratio(np.abs(dev - case['defect64']), case['bar_defect'])
    r_g = tmg._ratio(np.abs(tmg._hip_grad(case).double().numpy() - case['grad64']), case['bar_grad'])
    worst = [max(worst[0], r_d), max(worst[1], r_g)]
    text = '  %-40s defect %.3g of its bar, gradient %.3g of its bar' % (name, r_d, r_g)
    if name.startswith('r ='):
        plain = fp32_total(case['v'].cuda(), case['f'].cuda()).cpu().numpy()
        text += '; |sum - 4 pi| HIP %.3g, fp32 formulation %.3g' % (np.abs(dev.sum(1) - 4 * math.pi).max(), np.abs(plain - 4 * math.pi).max())
    say(text)
say('  worst on the device: defect %.3g of its bar, gradient %.3g of its bar' % tuple(worst))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
