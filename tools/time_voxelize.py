"""Time the ray-parity voxeliser and the voxel IoU (developer tool; GPU only), all in ONE process at I5 / batch 36 by default:
  1. volumetric_iou of one I5 pair at resolution 32 and 64, method='search' with search='brute' against method='voxel', alternating,
     by the host clock around the call (it ends in a read-back),
  2. method='voxel' alone at resolution 128 and 256,
  3. k_mesh_voxelize on the whole batch on a 128^3 lattice beside k_mesh_self_intersect on the same meshes -- the comparable kernel:
     an all-pairs scan through LDS tiles with a box filter in front of double arithmetic -- each from the library's HIP-event profiler
     (icn_profile_start / icn_profile_stop) in the same call,
  4. the kernel with and without the tile culling of its staging loop, when the path of a library built with -DICN_VOXEL_NO_CULL is
     given: both libraries are loaded into this process and their entries called alternately on the same buffers, by device events,
     and the two outputs are compared byte for byte.  Such a library is the regular one with one object replaced:
         cd geniconet_amd/csrc && mkdir -p build_exp && hipcc <the Makefile's CXXFLAGS and NO_PACKED_F32> -DICN_VOXEL_NO_CULL \
             -c -o build_exp/icn_voxel_nocull.o icn_voxel.hip && hipcc <CXXFLAGS> -shared -o build_exp/libicn_voxel_nocull.so \
             build_exp/icn_voxel_nocull.o <every other object of build/>
Median (min - max) of the repetitions after two warm-ups.  The record goes to the output file and to stdout.

    python tools/time_voxelize.py [repetitions=10] [batch=36] [subdivisions=5] [output=profiles/voxelize.txt] [no-cull library]
"""
import ctypes
import math
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
OUT = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'profiles', 'voxelize.txt')
NO_CULL = sys.argv[5] if len(sys.argv) > 5 else None
KERNELS = ('k_mesh_voxelize', 'k_mesh_self_intersect')
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


y, _ = data.synthetic_batch(B, R, seed=2, device='cuda')
ref_v = losses.grid_to_vertices(y, R).contiguous()
f32 = torch.from_numpy(geometry.get_ico_faces(R)).to(device='cuda', dtype=torch.int32)
faces = f32.long()
V, F = ref_v.shape[1], f32.shape[0]
say('Solid voxelisation by ray parity (icn_mesh_voxelize, metrics.voxelize) and volumetric_iou(method=\'voxel\')')
say('%s, libicn sources %s, on top of commit %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12], commit()))
say('I%d, batch %d: %d vertices, %d faces per mesh; %d repetitions after 2 warm-ups' % (R, B, V, F, REPS))


def iou(resolution, method):
    return metrics.volumetric_iou(0.9 * ref_v[0], ref_v[0], faces, resolution=resolution, search='brute', method=method)


def host_clock(resolution, methods):
    """The methods alternating, 2 warm-ups each -> {method: (times in ms, the IoU)}."""
    t, value = {m: [] for m in methods}, {}
    for k in range(2 + REPS):
        for m in methods:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            value[m] = iou(resolution, m)
            t[m].append((time.perf_counter() - t0) * 1e3)
    return {m: (t[m][2:], value[m]) for m in methods}


say('1. volumetric_iou of one I%d pair (mesh 0 against its 0.9-scaled copy: 0.729), the two methods alternating, host clock around the call:' % R)
for resolution in (32, 64):
    got = host_clock(resolution, ('search', 'voxel'))
    med = {m: line('resolution=%d, method=%s%s: IoU %.5f' % (resolution, m, ", search='brute'" if m == 'search' else '', got[m][1]), got[m][0])
           for m in got}
    say('  search / voxel: %.2f' % (med['search'] / med['voxel']))
say('2. method=\'voxel\' on the lattices nobody ran through the search:')
for resolution in (128, 256):
    times, value = host_clock(resolution, ('voxel',))['voxel']
    line('resolution=%d, method=voxel: IoU %.5f' % (resolution, value), times)

lo, hi = ref_v.double().amin((0, 1)).tolist(), ref_v.double().amax((0, 1)).tolist()
h = max(b - a for a, b in zip(lo, hi)) / SIDE
lattice = (tuple(lo), h, tuple(max(1, math.ceil((b - a) / h)) for a, b in zip(lo, hi)))
say('3. k_mesh_voxelize on the batch, lattice %s of spacing %.5f over the batch\'s box, beside k_mesh_self_intersect on the same meshes'
    % (lattice[2], h))
say('   (per launch, the library\'s event profiler):')


def both():
    metrics._voxelize_unchecked(ref_v, f32, *lattice)
    metrics._self_intersections_unchecked(ref_v, f32)


for _ in range(2):
    both()
torch.cuda.synchronize()
times = {}
for _ in range(REPS):
    _lib.profile_start(16)
    both()
    for e in _lib.profile_stop():                                            # synchronises the device
        if e['launches']:
            times.setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
med = {k: line(k, times[k]) for k in KERNELS}
occupancy = metrics._voxelize_unchecked(ref_v, f32, *lattice)
columns = B * lattice[2][1] * lattice[2][2]
say('  k_mesh_voxelize / k_mesh_self_intersect: %.3f; %.3g (column, face) pairs against %.3g pairs of faces; %.1f %% of the %d cells inside;'
    % (med[KERNELS[0]] / med[KERNELS[1]], columns * F, B * F * (F - 1) / 2, 100 * float(occupancy.float().mean()), occupancy.numel()))
say('  %.1f MB of occupancy written, %.0f GB/s of it' % (occupancy.numel() / 1e6, occupancy.numel() / med[KERNELS[0]] / 1e6))

if NO_CULL:
    say('4. the kernel with and without the tile culling of its staging loop (%s), alternating, device events:' % os.path.basename(NO_CULL))
    res, argtypes, _ = _lib.EXTENSION_HEADERS['icn_voxel.h']['icn_mesh_voxelize']
    entries = {}
    for name, path in (('with culling', _lib.LIB_PATH), ('without culling', NO_CULL)):
        fn = ctypes.CDLL(path).icn_mesh_voxelize
        fn.restype, fn.argtypes = res, argtypes
        entries[name] = fn
    outs = {name: torch.empty(B, *lattice[2], dtype=torch.uint8, device='cuda') for name in entries}

    def launch(name):
        rc = entries[name](ref_v.data_ptr(), f32.data_ptr(), B, V, F, *lattice[0], lattice[1], *lattice[2], outs[name].data_ptr(), _lib.stream())
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
    med = {name: line(name, t[name][2:]) for name in entries}
    same = torch.equal(outs['with culling'], outs['without culling']) and torch.equal(outs['with culling'].view(torch.bool), occupancy)
    say('  without / with: %.2f; the two give %s' % (med['without culling'] / med['with culling'], 'the same bytes' if same else 'DIFFERENT bytes'))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
