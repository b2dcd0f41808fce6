"""Time the area-weighted surface sampler and the sampled surface loss (developer tool; GPU only), all in ONE process at I5 / batch 36
with S = 10 242 samples per mesh by default:
  * the three forward kernels and the two backward kernels of icn_mesh_sample_fwd / icn_mesh_sample_bwd, each from the library's
    HIP-event profiler (icn_profile_start / icn_profile_stop),
  * the two entry points as wholes, and the torch formulation of the sampler on the same device, forward and forward + backward,
  * losses.Surface_Loss forward + backward for samples = 0 and samples = S with both searches, output = target + 0.01 noise,
  * one ico2ico training step (Trainer.step, the p2p loss: what bench.py measures), for scale.
HIP events; median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_surface_samples.py [repetitions=10] [batch=36] [subdivisions=5] [samples=10242] [output=profiles/surface_samples.txt]
"""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, geometry, losses, models, sampling  # noqa: E402
from geniconet_amd.train import Trainer  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
S = int(sys.argv[4]) if len(sys.argv) > 4 else 10242
OUT = sys.argv[5] if len(sys.argv) > 5 else os.path.join(ROOT, 'profiles', 'surface_samples.txt')
F_REG = (0.1, 0.01, 0.1)
FORWARD = ('k_msample_area', 'k_msample_scan', 'k_msample_point')
BACKWARD = ('k_msample_bwd_record', 'k_msample_bwd_vertex')

record = []


def say(text):
    print(text, flush=True)
    record.append(text)


x, target = data.synthetic_batch(B, R, seed=2, device='cuda')
near = (x + 0.01 * torch.randn(x.shape, generator=torch.Generator(device='cuda').manual_seed(3), device='cuda')).contiguous()
vts = losses.grid_to_vertices(near, R).contiguous()
f32 = torch.from_numpy(geometry.get_ico_faces(R)).to(device='cuda', dtype=torch.int32)
u = torch.rand((B, S, 3), generator=torch.Generator(device='cuda').manual_seed(4), device='cuda')
dp = torch.randn((B, S, 3), generator=torch.Generator(device='cuda').manual_seed(5), device='cuda')
V, F = vts.shape[1], f32.shape[0]
say('Area-weighted surface sampling (icn_mesh_sample_fwd / icn_mesh_sample_bwd) and the sampled losses.Surface_Loss')
say('%s, libicn sources %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12]))
say('I%d, batch %d: %d vertices, %d faces, %d samples per mesh; %d repetitions after 2 warm-ups, HIP events'
    % (R, B, V, F, S, REPS))


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


_, face, weights = sampling._hip_sample(vts, f32, u)


def hip_fwd():
    return sampling._hip_sample(vts, f32, u)


def hip_bwd():
    return sampling._hip_sample_bwd(f32, face, weights, dp, V)


say('kernels (per launch, the library\'s event profiler):')
for _ in range(2):
    hip_fwd(), hip_bwd()
torch.cuda.synchronize()
times = {}
for _ in range(REPS):
    _lib.profile_start(16)
    hip_fwd(), hip_bwd()
    for e in _lib.profile_stop():                                          # synchronises the device
        times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
for k in FORWARD + BACKWARD:
    line(k, times[k])
line('forward kernels together', [sum(v) for v in zip(*(times[k] for k in FORWARD))])
line('backward kernels together', [sum(v) for v in zip(*(times[k] for k in BACKWARD))])
say('entry points with their output and workspace allocations (sampling._hip_sample / _hip_sample_bwd):')
timed('icn_mesh_sample_fwd', hip_fwd)
timed('icn_mesh_sample_bwd', hip_bwd)


def step(fn, backward=True):
    v = vts.detach().requires_grad_(backward)
    points = fn(v, f32, u)[0]
    if backward:
        points.backward(dp)


say('sampler through autograd, HIP path against the torch formulation on the device:')
a = timed('HIP, forward', lambda: step(sampling._sample_points_unchecked, False))
b = timed('HIP, forward + backward', lambda: step(sampling._sample_points_unchecked))
c = timed('torch formulation, forward', lambda: step(sampling._torch_sample, False))
d = timed('torch formulation, forward + backward', lambda: step(sampling._torch_sample))
say('  torch / HIP: forward %.1f, forward + backward %.1f' % (c / a, d / b))

say('Surface_Loss forward + backward (factors 1 / 1, regularisers %s, edge_length 0.03), output = target + 0.01 noise:' % (F_REG,))
for samples in (0, S):
    for search in ('brute', 'grid'):
        crit = losses.Surface_Loss(R, 1.0, 1.0, *F_REG, edge_length=0.03, search=search, samples=samples).cuda()

        def surface_step():
            inp = near.detach().requires_grad_(True)
            crit(inp, target).backward()
        timed("samples=%d, search='%s'" % (samples, search), surface_step)
        say('    p2m %.3g, m2p %.3g, regulariser %.3g, total %.3g' % tuple(v for k, v in enumerate(crit.get_last_losses()) if k != 3))

say('for scale, one ico2ico training step at the same size (Trainer.step, p2p loss, eager):')
trainer = Trainer(models.default_params('ico2ico', subdivisions=R), 'cuda:0', seed=0)
xin = x.contiguous(memory_format=torch.channels_last)
for _ in range(3):
    trainer.step(xin, target)
timed('Trainer.step', lambda: trainer.step(xin, target))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
