"""Time the sided sums of every pair of clouds of two sets (developer tool; GPU only), all in ONE process, at G = R = 16 and 64 clouds a
set, on I5 vertices (N = M = 10 242) and on N = M = 2 048 of them:
  new       metrics.pairwise_sided_sums(p1, p2): icn_sided_sums, two launches (k_pair_sums, k_pair_sums_finish), G R doubles out;
  expanded  the route a user has without it: sided_distance on repeat_interleave / repeat copies of both sets, converted to double and
            summed per pair -- one k_nn_points launch over G R cloud pairs, the time to build the copies included.
The two alternate.  Per round and route: the whole route by device events (copies, conversion and sum included), and the launch times
from the library's HIP-event profiler (icn_profile_start / icn_profile_stop) in the same call.  Also: that the two agree within
2 N 2^-53 of the sum, the ps a pair of both kernels, and the share of the VALU issue rate that follows from the 8.625 VALU
instructions a pair of k_pair_sums' compiled inner loop (68 and one move for 8 pairs in the disassembly of icn_pairs.hip) beside the
11.625 of k_nn_points.  Median (min - max) of the repetitions after two warm-up rounds.  The record goes to the output file and to stdout.

    python tools/time_chamfer_matrix.py [repetitions=5] [output=profiles/chamfer_matrix.txt]
"""
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geniconet_amd import _lib, data, losses, metrics  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'chamfer_matrix.txt')
SHAPES = ((16, 10242), (64, 10242), (16, 2048), (64, 2048))                  # (clouds a set, points a cloud)
VALU_PER_PAIR = {'k_pair_sums': 69 / 8, 'k_nn_points': 93 / 8}               # the unrolled inner loops, moves included
CLOCK_HZ = 2.4e9                                                             # the MI355X's maximum clock: the shares below are lower bounds

record = []


def say(text):
    print(text, flush=True)
    record.append(text)


def spread(t):
    return 'median %10.4f ms   (%10.4f - %10.4f)' % (statistics.median(t), min(t), max(t))


def commit():
    """The commit of the tree: git's, else ICN_COMMIT (a copy of the tree without its history), else 'unknown'."""
    try:
        found = subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, text=True).stdout.strip()
    except OSError:
        found = ''
    return found or os.environ.get('ICN_COMMIT', 'unknown')


def new_route(p1, p2):
    return metrics.pairwise_sided_sums(p1, p2)


def expanded_route(p1, p2):
    G, R = p1.shape[0], p2.shape[0]
    dist, _ = metrics._sided_distance_unchecked(p1.repeat_interleave(R, 0), p2.repeat(G, 1, 1))
    return dist.double().sum(1).view(G, R)


def alternating(routes, p1, p2):
    """{route: (whole-route times by device events, {kernel: launch times by the library's profiler})} of REPS rounds over the routes in
    turn, after two warm-up rounds."""
    whole = {name: [] for name in routes}
    launches = {name: {} for name in routes}
    for k in range(2 + REPS):
        for name, route in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            _lib.profile_start(16)
            e0.record()
            route(p1, p2)
            e1.record()
            entries = _lib.profile_stop()                                    # synchronises the device
            if k >= 2:
                whole[name].append(e0.elapsed_time(e1))
                for e in entries:
                    launches[name].setdefault(e['kernel'], []).append(e['total_ms'] / e['launches'])
    return {name: (whole[name], launches[name]) for name in routes}


props = torch.cuda.get_device_properties(0)
lanes_per_second = props.multi_processor_count * 128 * CLOCK_HZ              # a CU issues 4 SIMDs x 32 lanes a cycle
y, _ = data.synthetic_batch(64, 5, seed=2, device='cuda')
first = losses.grid_to_vertices(y, 5).contiguous()
y, _ = data.synthetic_batch(64, 5, seed=3, device='cuda')
second = losses.grid_to_vertices(y, 5).contiguous()
del y
pick = torch.randperm(first.shape[1], generator=torch.Generator().manual_seed(0))[:2048].cuda()
say('Sided sums of every pair of clouds of two sets (icn_sided_sums, metrics.pairwise_sided_sums) against sided_distance on expanded copies')
say('%s, libicn sources %s, on top of commit %s; %d repetitions after 2 warm-up rounds, the two routes alternating'
    % (torch.cuda.get_device_name(0), _lib.source_sha256()[:12], commit(), REPS))
say('from the compiler (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage, and the disassembly of icn_pairs.hip):')
say('  k_pair_sums 37 VGPRs, 35 SGPRs, no scratch, 3104 bytes of LDS, 8 waves a SIMD; k_pair_sums_finish 8 VGPRs, no scratch')
say('  inner loop of k_pair_sums, four targets x two queries = 8 pairs: 24 v_sub_f32, 24 v_mul_f32, 16 v_add_f32, 4 v_min3_f32, 1 v_mov_b32')
say('  = 8.625 VALU instructions a pair, and 3 ds_read_b128; k_nn_points: 88 VALU instructions and 5 moves for 8 pairs = 11.625 a pair')
verdict = []
for clouds, n in SHAPES:
    p1, p2 = first[:clouds], second[:clouds]
    if n != first.shape[1]:
        p1, p2 = p1[:, pick].contiguous(), p2[:, pick].contiguous()
    pairs = clouds * clouds * n * n
    say('G = R = %d, N = M = %d: %.3g point pairs; the expanded copies hold %.0f MB, its dist and idx %.0f MB; the new entry writes %d bytes'
        % (clouds, n, pairs, 2 * clouds * clouds * n * 12 / 1e6, clouds * clouds * n * 8 / 1e6, 8 * clouds * clouds))
    got, want = new_route(p1, p2), expanded_route(p1, p2)
    worst = float(((got - want).abs() / (n * 2.0 ** -53 * want)).max())
    say('  largest |new - expanded| / (N 2^-53 sum) = %.3f (bound 2)' % worst)
    t = alternating({'new': new_route, 'expanded': expanded_route}, p1, p2)
    med = {}
    for name in ('new', 'expanded'):
        whole, launches = t[name]
        say('  %-9s whole route (device events)             %s' % (name, spread(whole)))
        med[name] = statistics.median(whole)
        for kernel, times in launches.items():
            say('  %-9s   launch %-34s %s' % ('', kernel, spread(times)))
            if kernel in VALU_PER_PAIR:
                m = statistics.median(times)
                med[kernel] = m
                say('  %-9s     %.4f ps a point pair; %.3f VALU instructions a pair: %.1f %% of the VALU issue rate at %.1f GHz'
                    % ('', m * 1e9 / pairs, VALU_PER_PAIR[kernel], 100 * VALU_PER_PAIR[kernel] * pairs / (m * 1e-3 * lanes_per_second),
                       CLOCK_HZ / 1e9))
    say('  new / expanded: whole route %.3f, search launch k_pair_sums / k_nn_points %.3f'
        % (med['new'] / med['expanded'], med['k_pair_sums'] / med['k_nn_points']))
    verdict.append(med['new'] <= med['expanded'])
    del got, want, t
    torch.cuda.empty_cache()
say('expectation (the new entry takes no longer than the expanded route on the same inputs): %s'
    % ('holds at every shape' if all(verdict) else 'FAILS at %s' % [s for s, ok in zip(SHAPES, verdict) if not ok]))

os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, 'w') as fh:
    fh.write('\n'.join(record) + '\n')
