"""Time the nearest-neighbour search between point sets (developer tool; GPU only), all in ONE process at I5 / batch 36 by default:
  1. k_nn_points for N = M = V points per cloud (the vertices of one synthetic batch against those of another) beside
     k_point_to_mesh on as many points, from the library's HIP-event profiler (icn_profile_start / icn_profile_stop) in the same call;
     the share of the VALU issue rate that follows from the 11.625 VALU instructions a pair of the compiled inner loop (88 and 5 moves
     for 8 pairs in the disassembly of icn_nn.hip; the definition itself needs 11: 3 sub, 3 mul, 2 add, 1 compare, 2 selects),
  2. the same search by torch on the same GPU, torch.cdist(...).min(-1) over chunks of queries sized to fit memory, by device events,
     alternating with the kernel's entry,
  3. the backward's two launches (k_nn_points_bwd_record, k_nn_points_bwd_vertex), the same way as 1.,
  4. metrics.evaluate_distance of one pair of meshes, modes chamfer and f_0.01, on the vertices and on `samples` = V surface samples,
     end to end by the host clock (each call ends in a read-back),
  5. the largest |got - ref| / (2^-24 A) of the backward's dtargets against float64 autograd at the device's choice, on the shapes of
     tests/test_nearest_points.py (batch 3, N = 1000, M = 300), as that test measures it.
Median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_nearest.py [repetitions=10] [batch=36] [subdivisions=5] [output=profiles/nearest_neighbour.txt]
"""
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, geometry, losses, metrics  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'profiles', 'nearest_neighbour.txt')
VALU_PER_PAIR = 93 / 8                       # the unrolled inner loop of k_nn_points: 88 VALU instructions and 5 moves for 8 pairs
CDIST_CHUNK = 1 << 28                        # distances torch.cdist may hold at once: 1 GiB in fp32

record = []


def say(text):
    print(text, flush=True)
    record.append(text)


def line(name, t):
    say('  %-66s median %10.4f ms   (%10.4f - %10.4f)' % (name, statistics.median(t), min(t), max(t)))
    return statistics.median(t)


def commit():
    """The commit of the tree: git's, else ICN_COMMIT (a copy of the tree without its history), else 'unknown'."""
    try:
        found = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    except OSError:
        found = ''
    return found or os.environ.get('ICN_COMMIT', 'unknown')


def profiled(call, kernels):
    """{kernel: per-launch times in ms} of REPS calls after two warm-ups, by the library's event profiler."""
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    times = {}
    for _ in range(REPS):
        _lib.profile_start(16)
        call()
        for e in _lib.profile_stop():                                        # synchronises the device
            if e['launches'] and e['kernel'] in kernels:
                times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
    return times


def by_events(calls):
    """{name: times in ms} of REPS rounds over the named calls, alternating, after two warm-up rounds, by device events."""
    t = {name: [] for name in calls}
    for _ in range(2 + REPS):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            e1.synchronize()
            t[name].append(e0.elapsed_time(e1))
    return {name: v[2:] for name, v in t.items()}


y, _ = data.synthetic_batch(B, R, seed=2, device='cuda')
vts = losses.grid_to_vertices(y, R).contiguous()
other, _ = data.synthetic_batch(B, R, seed=3, device='cuda')
points = losses.grid_to_vertices(other, R).contiguous()
f32 = torch.from_numpy(geometry.get_ico_faces(R)).to(device='cuda', dtype=torch.int32)
V, F = vts.shape[1], f32.shape[0]
props = torch.cuda.get_device_properties(0)
say('Nearest neighbours between point sets (icn_nearest_points / icn_nearest_points_bwd, metrics.sided_distance)')
say('%s, libicn sources %s, on top of commit %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12], commit()))
say('I%d, batch %d: N = M = %d points per cloud, %.3g pairs; %d repetitions after 2 warm-ups' % (R, B, V, B * V * V, REPS))

say('1. k_nn_points beside k_point_to_mesh on as many points (per launch, the library\'s event profiler):')


def both_searches():
    metrics._sided_distance_unchecked(points, vts)
    metrics._point_to_mesh_unchecked(points, vts, f32)


times = profiled(both_searches, ('k_nn_points', 'k_point_to_mesh'))
med = {k: line(k, times[k]) for k in ('k_nn_points', 'k_point_to_mesh')}
pairs = B * V * V
clock_hz = 2.4e9                                                            # the MI355X's maximum clock: the share below is a lower bound
lanes_per_second = props.multi_processor_count * 128 * clock_hz             # a CU issues 4 SIMDs x 32 lanes a cycle
say('  k_nn_points / k_point_to_mesh: %.3f; %.1f ps a pair' % (med['k_nn_points'] / med['k_point_to_mesh'], med['k_nn_points'] * 1e9 / pairs))
say('  %.3f VALU instructions a pair (disassembly) x %.3g pairs = %.3g lane-operations; %d CUs x 128 lanes x %.2f GHz (the maximum '
    'clock) = %.3g a second: %.1f %% of the VALU issue rate'
    % (VALU_PER_PAIR, pairs, VALU_PER_PAIR * pairs, props.multi_processor_count, clock_hz / 1e9, lanes_per_second,
       100 * VALU_PER_PAIR * pairs / (med['k_nn_points'] * 1e-3 * lanes_per_second)))

say('  what holds the rest back is NOT MEASURED (no counters were collected).  From the code: a tile entry is read as ds_read_b96, 8 LDS')
say('  cycles a wave for 22 VALU instructions of 2 cycles, so four SIMDs ask the LDS for 32 cycles in every 44, 73 % of it; and 756')
say('  workgroups of 4 waves on 256 CUs leave about 3 waves on a SIMD, with one CU in five a workgroup short of its neighbours.')

say('2. against torch on the same GPU: torch.cdist(...).min(-1) over chunks of queries of at most 2^%d distances, alternating, device events:'
    % (CDIST_CHUNK.bit_length() - 1))
step = max(1, CDIST_CHUNK // (B * V))
dist = torch.empty(B, V, device='cuda')
idx = torch.empty(B, V, dtype=torch.int32, device='cuda')


def by_cdist():
    out = [torch.cdist(points[:, lo:lo + step], vts).min(-1) for lo in range(0, V, step)]
    return torch.cat([o[0] for o in out], 1), torch.cat([o[1] for o in out], 1)


def by_kernel():
    _lib.api().icn_nearest_points(points.data_ptr(), vts.data_ptr(), B, V, V, dist.data_ptr(), idx.data_ptr(), _lib.stream())


t = by_events({'torch.cdist(...).min(-1), %d chunks of %d queries' % (-(-V // step), step): by_cdist, 'icn_nearest_points': by_kernel})
med2 = {name: line(name, v) for name, v in t.items()}
cd, ci = by_cdist()
agree = float((ci == idx.long()).float().mean())
say('  torch / kernel: %.2f; %.4f %% of the indices agree (cdist takes the root of a matmul expansion, so near-ties may differ), largest '
    '|sqrt(dist) - cdist| %.3g' % (list(med2.values())[0] / med2['icn_nearest_points'], 100 * agree, float((dist.sqrt() - cd).abs().max())))

say('3. the backward\'s two launches (per launch, the library\'s event profiler):')
upstream = torch.randn(B, V, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))


def forward_and_backward():
    p, q = points.detach().requires_grad_(), vts.detach().requires_grad_()
    metrics._sided_distance_unchecked(p, q)[0].backward(upstream)


times = profiled(forward_and_backward, ('k_nn_points_bwd_record', 'k_nn_points_bwd_vertex'))
back = {k: line(k, times[k]) for k in ('k_nn_points_bwd_record', 'k_nn_points_bwd_vertex')}
say('  the backward\'s two launches: %.4f ms, %.4f of the forward' % (sum(back.values()), sum(back.values()) / med['k_nn_points']))

say('4. metrics.evaluate_distance of one I%d mesh pair, end to end by the host clock (each call ends in a read-back):' % R)
for mode in ('chamfer', 'f_0.01'):
    for samples in (0, V):
        t = []
        for k in range(2 + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value = metrics.evaluate_distance(points[0], vts[0], f32, mode, samples=samples, seed=k)
            t.append((time.perf_counter() - t0) * 1e3)
        line('%s, samples = %d (last value %.6g)' % (mode, samples, value), t[2:])

say('5. dtargets against float64 autograd at the device\'s choice (batch 3, N = 1000, M = 300; tests/test_nearest_points.py):')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
try:
    import test_nearest_points  # noqa: E402
    import io
    import contextlib
    buffer = io.StringIO()
    with contextlib.redirect_stdout(buffer):
        test_nearest_points.test_hip_backward_bit_for_bit_in_the_points_and_within_its_roundings_in_the_targets(1000)
    for text in buffer.getvalue().splitlines():
        say('  ' + text)
except ImportError as e:                                                      # the tests are not part of an installed package
    say('  not measured: %s' % e)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
