"""Time the optimal matching behind the earth mover's distance (developer tool; GPU only): icn_match_clouds, one workgroup a pair, on
I5 vertex sets (N = 10 242) of data.synthetic_batch,
  far pairs   two different shapes;
  near pairs  a shape against itself, both with noise 0.01 added;
as one pair, a 4 x 4 matrix and a 16 x 16 matrix (match and prices not asked for, as pairwise_emd calls it), with the rounds of every
pair beside the time -- and, from the restatement metrics._torch_optimal_matching on the same GPU, the bids of one pair of each kind
and the time of one I3 pair, which shows what a round costs without the kernel.
EVERY STEP IS A PROCESS OF ITS OWN UNDER ITS OWN TIME LIMIT, started by this driver, which never touches the GPU itself.  The single
pairs come first and the limits of the later steps are sized from them (a matrix of up to 256 pairs is one wave of workgroups, one a
CU: about the time of its slowest pair).  A step that fails or runs out of time ends the run: nothing more is started.

    python tools/time_emd.py [output=profiles/emd_matrix.txt]
    python tools/time_emd.py --step NAME          (what the driver starts: one step, its record on stdout)
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = 6
NOISE = 0.01
FIRST_LIMIT = 180                    # seconds for the first step, a single pair: the estimate before any measurement is below 2 s
RESTATEMENT_LIMIT = 300             # seconds for a step that runs the restatement in torch
KERNEL_STEPS = ('far_1', 'near_1', 'far_4', 'near_4', 'far_16', 'near_16')
STEPS = KERNEL_STEPS + ('restatement_i3', 'bids_far', 'bids_near')


def clouds(kind, count, level=5):
    """(p1, p2), each (count, N, 3) on the GPU: far -- the shapes of two different seeds; near -- ONE shape with fresh noise per cloud."""
    import torch
    from geniconet_amd import data, losses
    shapes = [losses.grid_to_vertices(data.synthetic_batch(max(count, 2), level, seed=s, device='cuda')[0], level).contiguous() for s in (2, 3)]
    if kind == 'far':
        return shapes[0][:count].contiguous(), shapes[1][:count].contiguous()
    g = torch.Generator().manual_seed(7)
    one = shapes[0][:1]
    return tuple((one + NOISE * torch.randn((count,) + tuple(one.shape[1:]), generator=g).cuda()).contiguous() for _ in range(2))


def kernel_step(kind, count):
    import torch
    from geniconet_amd import metrics
    p1, p2 = clouds(kind, count)
    N = p1.shape[1]
    cap = 64 * N + 4096
    times = []
    for k in range(3):                                                       # the first call warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, cost, rounds, _ = metrics._optimal_matching_unchecked(p1, p2, PHASES, cap, False, want_match=False, want_prices=False)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    rounds, emd = rounds.cpu().double(), (cost / N).cpu()
    print('%s pairs, %d x %d of N = %d: %.1f ms (first call %.1f, then %.1f and %.1f); rounds / N per pair: mean %.2f, min %.2f, max %.2f; '
          'cap 64 N + 4096 = %.1f N; EMD mean %.5f; pairs at the cap: %d'
          % (kind, count, count, N, statistics.median(times[1:]), times[0], times[1], times[2], float(rounds.mean()) / N,
             float(rounds.min()) / N, float(rounds.max()) / N, cap / N, float(emd.mean()), int((rounds == cap).sum())))


def restatement_step():
    import torch
    from geniconet_amd import metrics
    p1, p2 = clouds('far', 2, level=3)
    p1, p2 = p1[:1].contiguous(), p2[1:].contiguous()                        # shape 0 of one seed against shape 1 of the other
    N = p1.shape[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    match, cost, rounds, prices = metrics._torch_optimal_matching(p1[0], p2[0], PHASES)
    torch.cuda.synchronize()
    t_torch = (time.perf_counter() - t0) * 1e3
    times = []
    for k in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = metrics.optimal_matching(p1, p2, PHASES)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    same = bool(torch.equal(got[0][0], match) and int(got[2]) == rounds and torch.equal(got[3][0], prices))
    print('one far I3 pair (N = %d), %d rounds: the restatement in torch on the GPU %.1f ms = %.3f ms a round; the kernel %.3f ms = %.2f us '
          'a round; match, rounds and prices of the two equal: %s'
          % (N, rounds, t_torch, t_torch / rounds, statistics.median(times[1:]), 1e3 * statistics.median(times[1:]) / rounds, same))


def bids_step(kind):
    from geniconet_amd import metrics
    p1, p2 = clouds(kind, 1)
    N = p1.shape[1]
    bidders = []
    _, cost, rounds, _ = metrics._torch_optimal_matching(p1[0], p2[0], PHASES, bidders=bidders)
    few = sum(1 for b in bidders if b < 16)
    print('one %s I5 pair by the restatement: %d rounds = %.2f N, %d bids = %.2f N, %.1f bidders a round, %.0f %% of the rounds with fewer '
          'than 16 bidders; EMD %.5f' % (kind, rounds, rounds / N, sum(bidders), sum(bidders) / N, sum(bidders) / max(rounds, 1),
                                        100.0 * few / max(rounds, 1), float(cost) / N))


def run_step(name):
    if name == 'restatement_i3':
        restatement_step()
    elif name.startswith('bids_'):
        bids_step(name[5:])
    else:
        kind, count = name.split('_')
        kernel_step(kind, int(count))


def drive(out):
    record = []

    def say(text):
        print(text, flush=True)
        record.append(text)
    say('Optimal matching by the epsilon-scaling auction (icn_match_clouds, k_match_auction: one workgroup of 1024 threads a pair), phases = %d'
        % PHASES)
    say('every step a process of its own under its own time limit; times are host times around a synchronised call, allocation included')
    limit, slowest = FIRST_LIMIT, 0.0
    for k, name in enumerate(STEPS):
        if k:                        # a matrix step is three calls of about its slowest pair; the restatement pays ~1 ms a round
            limit = int(60 + 6 * slowest) if name in KERNEL_STEPS else RESTATEMENT_LIMIT
        t0 = time.perf_counter()
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--step', name], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            say('step %s: no answer within its limit of %d s; the run ends here' % (name, limit))
            break
        took = time.perf_counter() - t0
        if res.returncode != 0:
            say('step %s: exit status %d; the run ends here\n%s' % (name, res.returncode, res.stderr[-2000:]))
            break
        say('[%s, limit %d s, took %.1f s] %s' % (name, limit, took, res.stdout.strip()))
        slowest = max(slowest, took)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as fh:
        fh.write('\n'.join(record) + '\n')


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--step':
        run_step(sys.argv[2])
    else:
        drive(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'emd_matrix.txt'))
