"""Time farthest point sampling (developer tool; GPU only): icn_farthest_points, one workgroup a cloud, against its restatement
sampling._torch_farthest_point_sample ON THE SAME GPU TENSORS, and what subsets of 2 048 points buy the earth mover's distance tables.
  1  kernel against restatement on vertex sets of data.synthetic_batch (I5: N = 10 242, I4: N = 2 562; sixteen shapes, repeated with
     noise 0.01 to the batch): the time of a call, the time a step and the ratio, and whether the two chose the same points;
  2  pairwise_emd of 16 x 16 I5 shapes on all vertices against the same on farthest_points(., 2048), sampling included, and
     generation_metrics(distance='emd') for G = R = 16 with and without points=2048;
  3  the compiler's resource report of every instantiation of k_farthest_points (registers, scratch, occupancy), from a compilation
     with the Makefile's flags whose object is thrown away.
The two arms of a comparison ALTERNATE in one process, every shape is warmed up first, a window lasts at least a second (and at least
one call), and the device is synchronised before every reading of the clock.  The source hash says which code was measured.

    python tools/time_fps.py [output=profiles/farthest_points.txt]
"""
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1, 10242, 2048), (36, 10242, 2048), (256, 10242, 2048), (256, 2562, 1024))
LEVELS = {10242: 5, 2562: 4}
NOISE = 0.01
WINDOW = 1.0                         # seconds a timing window lasts at least
ROUNDS = 2                           # windows per arm, alternating


def clouds(B, level):
    """(B, N, 3) on the GPU: the vertex sets of sixteen synthetic shapes, repeated to the batch with fresh noise per cloud."""
    import torch
    from geniconet_amd import data, losses
    base = losses.grid_to_vertices(data.synthetic_batch(16, level, seed=2, device='cuda')[0], level)
    p = base.repeat(-(-B // 16), 1, 1)[:B]
    return (p + NOISE * torch.randn(p.shape, generator=torch.Generator().manual_seed(7)).cuda()).contiguous()


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


def resource_report():
    """One line per instantiation of k_farthest_points from hipcc's kernel-resource-usage remarks, compiled as the Makefile compiles."""
    csrc = os.path.join(ROOT, 'geniconet_amd', 'csrc')
    makefile = open(os.path.join(csrc, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS := (.*)$', makefile, flags=re.M).group(1).replace('$(ARCH)', 'gfx950').split()
    no_packed = re.search(r'^NO_PACKED_F32 := (.*)$', makefile, flags=re.M).group(1).split()
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    res = subprocess.run([hipcc] + flags + no_packed + ['-Rpass-analysis=kernel-resource-usage', '-c', '-o', os.devnull, 'icn_fps.hip'],
                         cwd=csrc, capture_output=True, text=True, timeout=600)
    lines, fields = [], {}
    for line in res.stderr.split('\n'):
        m = re.search(r'remark:\s+(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|'
                      r'LDS Size \[bytes/block\]): (\S+)', line)
        if not m:
            continue
        fields[m.group(1)] = m.group(2)
        if m.group(1).startswith('LDS'):
            ppt = re.search(r'k_farthest_pointsILi(\d+)E', fields['Function Name'])
            lines.append('k_farthest_points<%s>: %s VGPRs, %s AGPRs, %s SGPRs, scratch %s bytes a lane, occupancy %s waves a SIMD, LDS %s bytes'
                         % (ppt.group(1) if ppt else '?', fields['VGPRs'], fields.get('AGPRs', '0'), fields['TotalSGPRs'],
                            fields['ScratchSize [bytes/lane]'], fields['Occupancy [waves/SIMD]'], fields['LDS Size [bytes/block]']))
    return lines or ['no resource report: hipcc exit status %d\n%s' % (res.returncode, res.stderr[-1000:])]


def main(out):
    import torch
    from geniconet_amd import _lib, metrics, sampling
    record = []

    def say(text):
        print(text, flush=True)
        record.append(text)
    say('Farthest point sampling (icn_farthest_points, k_farthest_points: one workgroup of 512 threads a cloud, every point in a register)')
    say('device %s; source sha256 %s' % (torch.cuda.get_device_name(0), _lib.source_sha256()))
    say('two arms alternate in one process, %d windows of at least %.0f s each after a warm-up call of each; host times around synchronised '
        'calls, allocation of the outputs included' % (ROUNDS, WINDOW))
    say('')
    say('1  kernel against the restatement in torch on the same GPU tensors')
    for B, N, S in SHAPES:
        p = clouds(B, LEVELS[N])
        t_kernel, t_torch = alternate(lambda: sampling.farthest_point_sample(p, S), lambda: sampling._torch_farthest_point_sample(p, S))
        same = torch.equal(sampling.farthest_point_sample(p, S)[0], sampling._torch_farthest_point_sample(p, S)[0])
        say('(B, N, S) = (%d, %d, %d): kernel %.3f ms = %.2f us a step; restatement %.1f ms = %.1f us a step; ratio %.0f; same points: %s'
            % (B, N, S, 1e3 * t_kernel, 1e6 * t_kernel / S, 1e3 * t_torch, 1e6 * t_torch / S, t_torch / t_kernel, same))
    say('')
    say('2  what subsets of 2 048 points buy the EMD tables (I5, 16 x 16; whole clouds are the path of profiles/emd_matrix.txt)')
    g, r = clouds(32, 5).split(16)
    t_whole, t_sub = alternate(lambda: metrics.pairwise_emd(g, r),
                               lambda: metrics.pairwise_emd(sampling.farthest_points(g, 2048), sampling.farthest_points(r, 2048)))
    say('pairwise_emd, 16 x 16: all 10 242 vertices %.1f ms; farthest_points(., 2048) of both sets and the matrix on them %.1f ms; ratio %.1f'
        % (1e3 * t_whole, 1e3 * t_sub, t_whole / t_sub))
    t_whole, t_sub = alternate(lambda: metrics.generation_metrics(g, r, distance='emd'),
                               lambda: metrics.generation_metrics(g, r, distance='emd', points=2048))
    say("generation_metrics(distance='emd'), G = R = 16: whole clouds %.1f ms; points=2048 %.1f ms; ratio %.1f"
        % (1e3 * t_whole, 1e3 * t_sub, t_whole / t_sub))
    say('')
    say("3  the compiler's resource report (hipcc -Rpass-analysis=kernel-resource-usage, the Makefile's flags)")
    for line in resource_report():
        say(line)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(record) + '\n')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'farthest_points.txt'))
