"""Time the ray caster (developer tool; GPU only), all in ONE process at I5 / batch 36 by default:
  1. k_mesh_raycast for R = V rays per mesh (from a sphere of radius 2 about the origin at the mesh's own vertices) beside
     k_point_to_mesh on as many points (another mesh's vertices), and the backward's two launches for those rays, each from the
     library's HIP-event profiler (icn_profile_start / icn_profile_stop) in the same call,
  2. k_mesh_raycast for a 128 x 128 depth map of every mesh (metrics.depth_map along (1, 1, 1)), the same way,
  3. the forward of 1. and 2. with and without the reject filter of icn_raycast.hip, when the path of a library built with
     -DICN_RAYCAST_NO_CULL is given: both libraries are loaded into this process and their entries called alternately on the same
     buffers, by device events, and the outputs are compared bit for bit.  Such a library is the regular one with one object replaced:
         cd geniconet_amd/csrc && mkdir -p build_exp && hipcc <the Makefile's CXXFLAGS and NO_PACKED_F32> -DICN_RAYCAST_NO_CULL \
             -c -o build_exp/icn_raycast_nocull.o icn_raycast.hip && hipcc <CXXFLAGS> -shared -o build_exp/libicn_raycast_nocull.so \
             build_exp/icn_raycast_nocull.o <every other object of build/>
  4. the largest |got - ref| / (2^-24 A) of the backward against float64 autograd of the torch formulation, on the shapes of
     tests/test_ray_cast.py (the noisy I2 at batch 3, R = 1000), as that test measures it.
Median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_raycast.py [repetitions=10] [batch=36] [subdivisions=5] [output=profiles/raycast.txt] [no-filter library]
"""
import ctypes
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, geometry, losses, metrics  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
B = int(sys.argv[2]) if len(sys.argv) > 2 else 36
R = int(sys.argv[3]) if len(sys.argv) > 3 else 5
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'profiles', 'raycast.txt')
NO_CULL = sys.argv[5] if len(sys.argv) > 5 else None
SIDE = 128

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


y, _ = data.synthetic_batch(B, R, seed=2, device='cuda')
vts = losses.grid_to_vertices(y, R).contiguous()
other, _ = data.synthetic_batch(B, R, seed=3, device='cuda')
points = losses.grid_to_vertices(other, R).contiguous()
f32 = torch.from_numpy(geometry.get_ico_faces(R)).to(device='cuda', dtype=torch.int32)
V, F = vts.shape[1], f32.shape[0]
say('Ray casting against batched meshes (icn_mesh_raycast / icn_mesh_raycast_bwd, metrics.ray_cast, depth_map)')
say('%s, libicn sources %s, on top of commit %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12], commit()))
say('I%d, batch %d: %d vertices, %d faces per mesh; %d repetitions after 2 warm-ups' % (R, B, V, F, REPS))

g = torch.Generator(device='cuda').manual_seed(0)
origins = torch.randn(B, V, 3, generator=g, device='cuda')
origins = (2 * origins / origins.norm(dim=2, keepdim=True)).contiguous()
directions = (vts - origins).contiguous()
upstream = torch.randn(B, V, generator=g, device='cuda')

say('1. %d rays per mesh at the mesh\'s own vertices, beside k_point_to_mesh on as many points; then the backward of those rays' % V)
say('   (per launch, the library\'s event profiler):')


def forward_and_search():
    metrics._ray_cast_unchecked(origins, directions, vts, f32)
    metrics._point_to_mesh_unchecked(points, vts, f32)


def forward_and_backward():
    args = tuple(x.detach().requires_grad_() for x in (origins, directions, vts))
    depth, face, _ = metrics._ray_cast_unchecked(*args, f32)
    depth.backward(torch.where(face >= 0, upstream, torch.zeros_like(upstream)))


times = profiled(forward_and_search, ('k_mesh_raycast', 'k_point_to_mesh'))
med = {k: line(k, times[k]) for k in ('k_mesh_raycast', 'k_point_to_mesh')}
depth, face, count = metrics._ray_cast_unchecked(origins, directions, vts, f32)
say('  k_mesh_raycast / k_point_to_mesh: %.3f; %.3g (ray, face) pairs, %.1f ps a pair; %.1f %% of the rays hit, %.2f crossings a ray'
    % (med['k_mesh_raycast'] / med['k_point_to_mesh'], B * V * F, med['k_mesh_raycast'] * 1e9 / (B * V * F), 100 * float((face >= 0).float().mean()),
       float(count.float().mean())))
times = profiled(forward_and_backward, ('k_mesh_raycast_bwd_record', 'k_mesh_raycast_bwd_vertex'))
back = {k: line(k, times[k]) for k in ('k_mesh_raycast_bwd_record', 'k_mesh_raycast_bwd_vertex')}
say('  the backward\'s two launches: %.4f ms, %.4f of the forward' % (sum(back.values()), sum(back.values()) / med['k_mesh_raycast']))

say('2. a %d x %d depth map of every mesh along (1, 1, 1), %d rays per mesh:' % (SIDE, SIDE, SIDE * SIDE))
frame = metrics._joint_frame(vts)
times = profiled(lambda: metrics._depth_map_unchecked(vts, f32, (1, 1, 1), SIDE, frame), ('k_mesh_raycast',))
med_map = line('k_mesh_raycast', times['k_mesh_raycast'])
_, mask = metrics._depth_map_unchecked(vts, f32, (1, 1, 1), SIDE, frame)
say('  %.1f ps a (ray, face) pair; %.1f %% of the pixels covered' % (med_map * 1e9 / (B * SIDE * SIDE * F), 100 * float(mask.float().mean())))

if NO_CULL:
    say('3. the forward with and without the reject filter (%s), alternating, device events:' % os.path.basename(NO_CULL))
    res, argtypes, _ = _lib.EXTENSION_HEADERS['icn_raycast.h']['icn_mesh_raycast']
    entries = {}
    for name, path in (('with the filter', _lib.LIB_PATH), ('without the filter', NO_CULL)):
        fn = ctypes.CDLL(path).icn_mesh_raycast
        fn.restype, fn.argtypes = res, argtypes
        entries[name] = fn
    pixel_origins, w = metrics._pixel_rays((1, 1, 1), SIDE, frame, vts)
    workloads = (('%d rays at the vertices' % V, origins, directions),
                 ('the %d x %d depth map' % (SIDE, SIDE), pixel_origins[None].expand(B, -1, -1).contiguous(),
                  w.expand(B, SIDE * SIDE, 3).contiguous()))
    for what, org, dirs in workloads:
        n = org.shape[1]
        outs = {name: (torch.empty(B, n, device='cuda'), torch.empty(B, n, dtype=torch.int32, device='cuda'),
                       torch.empty(B, n, dtype=torch.int32, device='cuda')) for name in entries}

        def launch(name):
            rc = entries[name](org.data_ptr(), dirs.data_ptr(), vts.data_ptr(), f32.data_ptr(), B, n, V, F,
                               *(x.data_ptr() for x in outs[name]), _lib.stream())
            assert rc == 0, name
        t = {name: [] for name in entries}
        for k in range(2 + REPS):
            for name in entries:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(name)
                e1.record()
                e1.synchronize()
                t[name].append(e0.elapsed_time(e1))
        med = {name: line('%s, %s' % (what, name), t[name][2:]) for name in entries}
        a, b = outs['without the filter'], outs['with the filter']
        differ = int(((a[0].view(torch.int32) != b[0].view(torch.int32)) | (a[1] != b[1]) | (a[2] != b[2])).sum())
        say('  without / with: %.2f; %d of %d rays differ' % (med['without the filter'] / med['with the filter'], differ, B * n))

say('4. the backward against float64 autograd of the torch formulation (noisy I2, batch 3, 1000 rays; tests/test_ray_cast.py):')
sys.path.insert(0, os.path.join(ROOT, 'tests'))
try:
    import test_ray_cast  # noqa: E402
    import io
    import contextlib
    buffer = io.StringIO()
    with contextlib.redirect_stdout(buffer):
        test_ray_cast.test_hip_backward_against_float64_autograd_element_by_element(1000)
    for text in buffer.getvalue().splitlines():
        say('  ' + text)
except ImportError as e:                                                      # the tests are not part of an installed package
    say('  not measured: %s' % e)

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
