"""Time the normal-agreement term of the sampled surface loss (developer tool; GPU only), all in ONE process at I5 / batch 36 with
S = 10 242 samples per mesh by default:
  * the three kernels of icn_face_normal_agree_fwd / icn_face_normal_agree_bwd (forward, record pass, vertex scatter; the backward
    runs the last two once per side), each from the library's HIP-event profiler (icn_profile_start / icn_profile_stop),
  * metrics.face_normal_agreement through autograd, the HIP path against the torch formulation on the same device, forward and
    forward + backward (both sides),
  * losses.Surface_Loss forward + backward with samples = S, without and with factor_normal, for both searches,
  * the accuracy figures of tests/test_normal_agreement.py on its own inputs: the K that the fp32 torch formulation needs in
    |t - t_64| <= K u (1 / s_a + 1 / s_b) + 16 u against float64 (the test allows the HIP kernel twice that), and the HIP kernel's.
HIP events; median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_normal_agreement.py [repetitions=10] [batch=36] [subdivisions=5] [samples=10242] [output=profiles/normal_agreement.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, geometry, losses, metrics, sampling  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
S = int(sys.argv[4]) if len(sys.argv) > 4 else 10242
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, 'profiles', 'normal_agreement.txt')
F_REG = (0.1, 0.01, 0.1)
KERNELS = ('k_fnormal_agree', 'k_fnormal_agree_bwd_record', 'k_fnormal_agree_bwd_vertex')

record = []


def say(text):
    print(text, flush=True)
    record.append(text)


x, target = data.synthetic_batch(B, R, seed=2, device='cuda')
near = (x + 0.01 * torch.randn(x.shape, generator=torch.Generator(device='cuda').manual_seed(3), device='cuda')).contiguous()
out = losses.grid_to_vertices(near, R).contiguous()
ref = target[:, 0:3].transpose(1, 2).contiguous()
f32 = torch.from_numpy(geometry.get_ico_faces(R)).to(device='cuda', dtype=torch.int32)
u = torch.rand((B, S, 3), generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
dt = torch.rand((B, S), generator=torch.Generator(device='cuda').manual_seed(5), device='cuda')
points, on_out, _ = sampling._sample_points_unchecked(out, f32, u)
near_ref = metrics._point_to_mesh_unchecked(points, ref, f32, 'grid')[1]
V, F = out.shape[1], f32.shape[0]
say('Normal agreement of sampled surfaces (icn_face_normal_agree_fwd / icn_face_normal_agree_bwd) and losses.Surface_Loss(factor_normal)')
say('%s, libicn sources %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12]))
say('I%d, batch %d: %d vertices, %d faces, %d samples per mesh (faces: the sample\'s on the output, the closest on the target);'
    ' %d repetitions after 2 warm-ups, HIP events' % (R, B, V, F, S, REPS))


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
    a, b = out.detach().requires_grad_(backward), ref.detach().requires_grad_(backward)
    t = fn(a, f32, on_out, b, f32, near_ref)
    if backward:
        t.backward(dt)


say('kernels (per launch, the library\'s event profiler; the backward launches the record pass and the scatter once per side):')
for _ in range(2):
    step(metrics._face_normal_agreement_unchecked)
torch.cuda.synchronize()
times = {}
for _ in range(REPS):
    _lib.profile_start(16)
    step(metrics._face_normal_agreement_unchecked)
    for e in _lib.profile_stop():                                          # synchronises the device
        times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
for k in KERNELS:
    line(k, times[k])
line('forward + backward of both sides, kernels together',
     [f + 2 * (r + v) for f, r, v in zip(*(times[k] for k in KERNELS))])

say('face_normal_agreement through autograd, HIP path against the torch formulation on the device:')
a = timed('HIP, forward', lambda: step(metrics._face_normal_agreement_unchecked, False))
b = timed('HIP, forward + backward', lambda: step(metrics._face_normal_agreement_unchecked))
c = timed('torch formulation, forward', lambda: step(metrics._torch_face_normal_agreement, False))
d = timed('torch formulation, forward + backward', lambda: step(metrics._torch_face_normal_agreement))
say('  torch / HIP: forward %.1f, forward + backward %.1f' % (c / a, d / b))
say('  the fixed-order HIP backward %s torch\'s atomic index_put backward' % ('beats' if b < d else 'does NOT beat'))

say('Surface_Loss forward + backward (factors 1 / 1, regularisers %s, edge_length 0.03, samples %d), output = target + 0.01 noise:'
    % (F_REG, S))
for search in ('brute', 'grid'):
    for factor_normal in (0.0, 0.1):
        crit = losses.Surface_Loss(R, 1.0, 1.0, *F_REG, edge_length=0.03, search=search, samples=S, factor_normal=factor_normal).cuda()

        def surface_step():
            inp = near.detach().requires_grad_(True)
            crit(inp, target).backward()
        timed("search='%s', factor_normal=%g" % (search, factor_normal), surface_step)
        say('    p2m %.3g, m2p %.3g, regulariser %.3g, total %.3g' % tuple(v for k, v in enumerate(crit.get_last_losses()) if k != 3)
            + ', l_n %.3g' % float(crit.last_normal))

say('accuracy on the inputs of tests/test_normal_agreement.py (B = 3, r = 2 against r = 1), u = 2^-24:')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import test_normal_agreement as tna  # noqa: E402
for size in tna.SIZES:
    case = tna._case(size)
    args = tna._args(case, 'cuda')
    e_torch = (metrics._torch_face_normal_agreement(*args).double().cpu().numpy() - case['t64'])
    e_hip = (metrics.face_normal_agreement(*args).double().cpu().numpy() - case['t64'])
    say('  S = %3d: worst |t - t_64|: torch fp32 %.2f u, HIP %.2f u; K needed: torch fp32 %.3f, HIP %.3f; without the 16 u: %.3f, %.3f'
        % (size, abs(e_torch).max() / tna.U, abs(e_hip).max() / tna.U, tna._ratio(e_torch + case['t64'], case),
           tna._ratio(e_hip + case['t64'], case), (abs(e_torch) / (tna.U * case['inv_s'])).max(), (abs(e_hip) / (tna.U * case['inv_s'])).max()))
say('  K of the test = twice the worst torch fp32 figure over the three sizes')

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
