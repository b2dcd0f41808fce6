"""Time the occupancy histogram and the Jensen-Shannon divergence (developer tool; GPU only): icn_point_occupancy and icn_occupancy_jsd
against their restatements metrics._torch_occupancy_counts and metrics._torch_occupancy_jsd ON THE SAME GPU TENSORS.
  1  histogram (set form and per cloud) and the whole jensen_shannon_divergence of two sets, kernel route against restatement, for
     G = R = 64 clouds of 2 048 points (farthest_points of I5 vertex sets) and of 10 242 points (the I5 vertex sets), resolution 28:
     the time of a call, the ratio, and whether the counts agree;
  2  what the LDS atomics cost when every point lies in ONE cell (all 64 lanes of a wave add to one address) beside the same number
     of spread-out points: the kernels' own times from HIP events around the launches;
  3  the measured error of icn_occupancy_jsd against a float64 numpy spelling, on those sets and on random and sparse histograms at
     R = 1, 2, 28 and 32, beside the bound 2^-44;
  4  the compiler's resource report of the three kernels (registers, scratch, occupancy, static LDS), from a compilation with the
     Makefile's flags whose object is thrown away.
The two arms of a comparison ALTERNATE in one process, every shape is warmed up first, a window lasts at least a second (and at least
one call), and the device is synchronised before every reading of the clock.  The source hash says which code was measured.

    python tools/time_jsd.py [output=profiles/occupancy_jsd.txt]
"""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = 64                            # clouds a set
RESOLUTION = 28
NOISE = 0.01
WINDOW = 1.0                         # seconds a timing window lasts at least
ROUNDS = 2                           # windows per arm, alternating
BOUND = 2.0 ** -44


def clouds(B, seed):
    """(B, 10242, 3) on the GPU: the vertex sets of sixteen synthetic I5 shapes, repeated to the batch with fresh noise per cloud."""
    import torch
    from geniconet_amd import data, losses
    base = losses.grid_to_vertices(data.synthetic_batch(16, 5, seed=seed, device='cuda')[0], 5)
    p = base.repeat(-(-B // 16), 1, 1)[:B]
    return (p + NOISE * torch.randn(p.shape, generator=torch.Generator().manual_seed(seed + 5)).cuda()).contiguous()


def window(call):
    """Seconds a call of `call` takes: calls repeated for at least WINDOW seconds, the device synchronised around the window."""
    import torch
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        call()
        n += 1
        torch.cuda.synchronize()
        took = time.perf_counter() - t0
        if took >= WINDOW:
            return took / n


def alternate(first, second):
    """The median time of a call of each arm over ROUNDS alternating windows, after one warm-up call of each."""
    import torch
    first(), second()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(ROUNDS):
        a.append(window(first))
        b.append(window(second))
    return statistics.median(a), statistics.median(b)


def kernel_times(call, repeats=20):
    """kernel -> mean milliseconds a launch, from HIP events around every launch of `repeats` calls after a warm-up call."""
    import torch
    from geniconet_amd import _lib
    call()
    torch.cuda.synchronize()
    _lib.profile_start(16 * repeats)
    try:
        for _ in range(repeats):
            call()
        torch.cuda.synchronize()
    finally:
        entries = _lib.profile_stop()
    return {e['kernel']: e['total_ms'] / e['launches'] for e in entries}


def numpy_jsd(a, b):
    """The divergence in float64 numpy: the header's formula, numpy's order of summation."""
    import numpy as np
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    p, q = a.astype(np.float64) / float(a.sum()), b.astype(np.float64) / float(b.sum())
    m = 0.5 * (p + q)
    tp, tq = np.zeros_like(p), np.zeros_like(q)
    tp[a > 0] = p[a > 0] * np.log2(p[a > 0] / m[a > 0])
    tq[b > 0] = q[b > 0] * np.log2(q[b > 0] / m[b > 0])
    return float((0.5 * (tp + tq)).sum())


def resource_report():
    """One line per occupancy kernel from hipcc's kernel-resource-usage remarks, compiled as the Makefile compiles."""
    csrc = os.path.join(ROOT, 'geniconet_amd', 'csrc')
    makefile = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS := (.*)$', makefile, flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    no_packed = re.search(r'^NO_PACKED_F32 := (.*)$', makefile, flags=re.M).group(1).split()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    res = subprocess.run([hipcc] + flags + no_packed + ['-Rpass-analysis=kernel-resource-usage', '-c', '-o', os.devnull, 'icn_voxel.hip'],
                         cwd=csrc, capture_output=True, text=True, timeout=600)
    lines, fields = [], {}
    for line in res.stderr.split('\n'):
        m = re.search(r'remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|'
                      r'LDS Size \[bytes/block\]): (\S+)', line)
        if not m:
            continue
        fields[m.group(1)] = m.group(2)
        if m.group(1).startswith('LDS'):
            name = re.search(r'k_(point_occupancy|occupancy_reduce|occupancy_jsd)', fields['Function Name'])
            if name:
                lines.append('%s: %s VGPRs, %s AGPRs, %s SGPRs, scratch %s bytes a lane, occupancy %s waves a SIMD, static LDS %s bytes'
                             % (name.group(0), fields['VGPRs'], fields.get('AGPRs', '0'), fields['TotalSGPRs'],
                                fields['ScratchSize [bytes/lane]'], fields['Occupancy [waves/SIMD]'], fields['LDS Size [bytes/block]']))
    return lines or ['no resource report: hipcc exit status %d\n%s' % (res.returncode, res.stderr[-1000:])]


def main(out):
    import torch
    from geniconet_amd import _lib, metrics, sampling
    record = []

    def say(text):
        print(text, flush=True)
        record.append(text)
    R = RESOLUTION
    lo, inv = metrics._check_lattice('time_jsd', R, (-1.0, 1.0))
    say('Occupancy histograms and the Jensen-Shannon divergence (icn_point_occupancy: k_point_occupancy, k_occupancy_reduce; '
        'icn_occupancy_jsd: k_occupancy_jsd)')
    say('device %s; source sha256 %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()))
    say('two arms alternate in one process, %d windows of at least %.0f s each after a warm-up call of each; host times around synchronised '
        'calls, allocation of the outputs included; resolution %d over (-1, 1)' % (ROUNDS, WINDOW, R))
    say('')
    say('1  kernel route against the restatement in torch on the same GPU tensors, G = R = %d clouds' % SETS)
    whole = clouds(SETS, 2), clouds(SETS, 9)
    sets = {2048: tuple(sampling.farthest_points(x, 2048).contiguous() for x in whole), 10242: whole}
    errors = []
    for N, (g, r) in sets.items():
        for per_cloud in (False, True):
            t_kernel, t_torch = alternate(lambda: metrics.occupancy_counts(g, R, per_cloud=per_cloud),
                                          lambda: metrics._torch_occupancy_counts(g, R, lo, inv, per_cloud))
            a, b = metrics.occupancy_counts(g, R, per_cloud=per_cloud), metrics._torch_occupancy_counts(g, R, lo, inv, per_cloud)
            say('occupancy_counts, %d x %d points, %s: kernel %.3f ms; restatement %.3f ms; ratio %.1f; same counts: %s'
                % (SETS, N, 'one histogram a cloud' if per_cloud else 'the set histogram', 1e3 * t_kernel, 1e3 * t_torch, t_torch / t_kernel,
                   torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])))

        def restated():
            return metrics._torch_occupancy_jsd(metrics._torch_occupancy_counts(g, R, lo, inv)[0], metrics._torch_occupancy_counts(r, R, lo, inv)[0])
        t_kernel, t_torch = alternate(lambda: metrics.jensen_shannon_divergence(g, r, R), restated)
        got, want = float(metrics.jensen_shannon_divergence(g, r, R)), float(restated())
        ca, cb = (metrics.occupancy_counts(x, R)[0] for x in (g, r))
        errors.append(('the two sets of %d x %d points' % (SETS, N), abs(got - numpy_jsd(ca.cpu().numpy(), cb.cpu().numpy()))))
        t_jsd, t_jsd_torch = alternate(lambda: metrics.occupancy_jsd(ca, cb), lambda: metrics._torch_occupancy_jsd(ca, cb))
        say('jensen_shannon_divergence, two sets of %d x %d points (two histograms and the divergence): kernels %.3f ms; restatement %.3f ms; '
            'ratio %.1f; jsd %.6f against %.6f' % (SETS, N, 1e3 * t_kernel, 1e3 * t_torch, t_torch / t_kernel, got, want))
        say('occupancy_jsd alone on those histograms: kernel %.3f ms; restatement %.3f ms; ratio %.1f'
            % (1e3 * t_jsd, 1e3 * t_jsd_torch, t_jsd_torch / t_jsd))
    say('')
    say('2  every point in one cell beside a spread-out cloud: HIP events around the launches, the mean of 20 calls')
    for N, (g, _) in sets.items():
        one = torch.full_like(g, 0.3)
        for per_cloud in (False, True):
            spread, same = (kernel_times(lambda: metrics.occupancy_counts(x, R, per_cloud=per_cloud)) for x in (g, one))
            say('%d x %d points, %s: k_point_occupancy %.1f us spread out, %.1f us in one cell (%.1f x); k_occupancy_reduce %.1f us'
                % (SETS, N, 'one histogram a cloud' if per_cloud else 'the set histogram', 1e3 * spread['k_point_occupancy'],
                   1e3 * same['k_point_occupancy'], same['k_point_occupancy'] / spread['k_point_occupancy'],
                   1e3 * spread.get('k_occupancy_reduce', 0.0)))
    say('')
    say('3  icn_occupancy_jsd against the float64 numpy spelling (bound 2^-44 = %.3g)' % BOUND)
    gen = torch.Generator().manual_seed(1)
    for res in (1, 2, 28, 32):
        cells = res ** 3
        dense = [torch.randint(1, 1000, (cells,), generator=gen, dtype=torch.int32).reshape(res, res, res) for _ in range(2)]
        sparse = [torch.zeros(cells, dtype=torch.int32) for _ in range(2)]
        for x in sparse:
            x[torch.randperm(cells, generator=gen)[:min(cells, 5)]] = 1
        sparse[1][sparse[0].nonzero()[0]] = 1
        for name, (a, b) in (('random', dense), ('sparse', [x.reshape(res, res, res) for x in sparse])):
            errors.append(('%s histograms, R = %d' % (name, res),
                           abs(float(metrics.occupancy_jsd(a.cuda(), b.cuda())) - numpy_jsd(a.numpy(), b.numpy()))))
    for name, err in errors:
        say('%s: |kernel - numpy| = %.3g = %.4f of the bound' % (name, err, err / BOUND))
    say('the largest: %.3g = %.4f of the bound' % (max(e for _, e in errors), max(e for _, e in errors) / BOUND))
    say('')
    say("4  the compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, the Makefile's flags; the histogram itself is "
        "dynamic LDS, 4 R^3 bytes: 87 808 at R = 28, 131 072 at 32)")
    for line in resource_report():
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(record) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'occupancy_jsd.txt'))
