"""icn_match_clouds on the device (metrics.optimal_matching, pairwise_emd, earth_movers_distance).

The kernel is held to the restatement metrics._torch_optimal_matching evaluated on CPU tensors, whose root is correctly rounded like
the device's sqrtf (metrics._rounded_root: torch's own CPU sqrt is one unit off on AVX-512 builds): max, the argmax
with the lowest index and the second maximum are order-free, so match, rounds and prices must agree BIT FOR BIT however the kernel
splits the scans; the cost is a double sum of the same N terms in another order, within N 2^-53 cost.  The point counts sit around one
wave (63, 64, 65) and around the sixteen bidders below which several waves share a scan (every count above 16 passes through all team
sizes as a phase runs out of bidders); 642 has rounds with hundreds of bidders, many a wave, and 1100 more bidders in its first
rounds than the workgroup has threads.  The clouds are those of tests/test_optimal_matching.py, which holds that the restatement ends
every one of them below the cap."""
import math

import pytest
import torch

from geniconet_amd import metrics

from test_optimal_matching import GPU_CASES, NAN, PHASES, is_a_permutation, pair, restated, slackness_holds, sphere
from test_signed_distance import _profiled


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int64)


def same_outputs(got, want, N):
    """(match, cost, rounds, prices) of one pair against the restatement's: bits, but for the order of the cost's sum."""
    match, cost, rounds, prices = (x.cpu() for x in got)
    m, c, n, x = want
    assert torch.equal(match, m) and int(rounds) == n and torch.equal(_bits(prices), _bits(x))
    assert (math.isnan(float(c)) and math.isnan(float(cost))) or abs(float(cost) - float(c)) <= N * 2.0 ** -53 * float(c)
    return True


def every_output_equal(a, b):
    """Two results of the kernel, bit for bit in all four outputs (None where not asked for)."""
    return all((x is None and y is None) or torch.equal(_bits(x.double() if x.dtype == torch.float64 else x.long()),
                                                        _bits(y.double() if y.dtype == torch.float64 else y.long()))
               for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize('kind,N', GPU_CASES)
def test_the_kernel_equals_the_restatement_on_cpu_tensors(kind, N):
    p, q = pair(kind, N)
    want = restated(kind, N)
    assert want[2] < 64 * N + 4096                                           # below the cap: a real result, not the cap's
    got, kernels = _profiled(lambda: metrics.optimal_matching(p[None].cuda(), q[None].cuda()))
    assert kernels == {'k_match_auction': 1}
    match, cost, rounds, prices = got
    assert match.shape == prices.shape == (1, N) and cost.shape == rounds.shape == (1,) and match.is_cuda
    assert (match.dtype, cost.dtype, rounds.dtype, prices.dtype) == (torch.int64, torch.float64, torch.int32, torch.float64)
    assert same_outputs((match[0], cost[0], rounds[0], prices[0]), want, N)
    assert int(rounds[0]) < 64 * N + 4096 and is_a_permutation(match[0].cpu())
    # epsilon-complementary slackness from the kernel's own outputs
    assert slackness_holds(p, q, match[0].cpu(), prices[0].cpu())


@pytest.mark.gpu
def test_every_entry_of_a_matrix_call_is_the_one_by_one_call_and_the_paired_call():
    p1 = torch.stack([pair('sphere', 65)[0], pair('self', 65)[0], sphere(65, 5)]).cuda()
    p2 = torch.stack([pair('sphere', 65)[1], sphere(65, 6)]).cuda()
    full = metrics.optimal_matching(p1, p2, paired=False)
    assert full[0].shape == full[3].shape == (3, 2, 65) and full[1].shape == full[2].shape == (3, 2)
    assert same_outputs([x[0, 0] for x in full], restated('sphere', 65), 65)
    for g in range(3):
        for r in range(2):
            one = metrics.optimal_matching(p1[g:g + 1], p2[r:r + 1], paired=False)
            assert every_output_equal([x[0, 0] for x in one], [x[g, r] for x in full]), (g, r)
    paired = metrics.optimal_matching(p1[:2], p2)
    for b in range(2):
        assert every_output_equal([x[b] for x in paired], [x[b, b] for x in full]), b
    # with null match and prices: the same cost and rounds
    bare = metrics._optimal_matching_unchecked(p1, p2, PHASES, 64 * 65 + 4096, False, want_match=False, want_prices=False)
    assert bare[0] is None and bare[3] is None and every_output_equal(bare[1:3], full[1:3])
    bare = metrics._optimal_matching_unchecked(p1[:2], p2, PHASES, 64 * 65 + 4096, True, want_match=False, want_prices=False)
    assert every_output_equal(bare[1:3], paired[1:3])
    assert torch.equal(_bits(metrics.pairwise_emd(p1, p2)), _bits(full[1] / 65))


@pytest.mark.gpu
def test_launches_of_at_most_1024_pairs_change_no_bit(monkeypatch):
    p1 = torch.stack([sphere(3, s) for s in range(5)]).cuda()
    p2 = torch.stack([sphere(3, 10 + s) for s in range(5)]).cuda()
    whole = metrics.optimal_matching(p1, p2, paired=False)
    for most, launches in ((10, 3), (3, 10), (2, 15)):                       # whole rows of g; then pieces of one row
        monkeypatch.setattr(metrics, '_MATCH_PAIRS', most)
        got, kernels = _profiled(lambda: metrics.optimal_matching(p1, p2, paired=False))
        assert kernels == {'k_match_auction': launches} and every_output_equal(got, whole), most
    monkeypatch.setattr(metrics, '_MATCH_PAIRS', 2)
    got, kernels = _profiled(lambda: metrics.optimal_matching(p1, p2))
    assert kernels == {'k_match_auction': 3}
    for b in range(5):
        assert every_output_equal([x[b] for x in got], [x[b, b] for x in whole]), b


@pytest.mark.gpu
def test_a_nan_and_an_inf_take_the_early_case_and_leave_the_other_entry_alone():
    p1 = torch.stack([pair('sphere', 63)[0], pair('sphere', 63)[0]])
    p2 = torch.stack([pair('sphere', 63)[1], pair('sphere', 63)[1]])
    p1[1, 40, 2], p2[1, 62, 0] = NAN, float('inf')
    match, cost, rounds, prices = metrics.optimal_matching(p1.cuda(), p2.cuda(), paired=False)
    for g, r in ((0, 1), (1, 0), (1, 1)):
        assert (match[g, r] == -1).all() and math.isnan(float(cost[g, r])) and int(rounds[g, r]) == 0 and torch.isnan(prices[g, r]).all()
    assert same_outputs((match[0, 0], cost[0, 0], rounds[0, 0], prices[0, 0]), restated('sphere', 63), 63)
    one = metrics.optimal_matching(p1[:1].cuda(), p2[:1].cuda())
    assert every_output_equal([x[0] for x in one], [x[0, 0] for x in (match, cost, rounds, prices)])
    d = metrics.pairwise_emd(p1.cuda(), p2.cuda())
    assert torch.isnan(d).tolist() == [[False, True], [True, True]]


@pytest.mark.gpu
def test_the_other_early_cases_on_the_device():
    same = torch.full((1, 70, 3), 0.25).cuda()
    match, cost, rounds, prices = metrics.optimal_matching(same, same.clone())
    assert match[0].tolist() == list(range(70)) and float(cost) == 0 and int(rounds) == 0 and (prices == 0).all()
    a, b = torch.tensor([[[1.0, 2.0, 2.0]]]).cuda(), torch.zeros(1, 1, 3).cuda()
    match, cost, rounds, prices = metrics.optimal_matching(a, b)
    assert match.tolist() == [[0]] and float(cost) == 3.0 and int(rounds) == 0 and prices.tolist() == [[0.0]]


@pytest.mark.gpu
def test_the_round_cap_on_the_device():
    p, q = pair('sphere', 64)
    want = metrics._torch_optimal_matching(p, q, PHASES, 1)
    got = metrics.optimal_matching(p[None].cuda(), q[None].cuda(), max_rounds=1)
    assert same_outputs([x[0] for x in got], want, 64)
    assert int(got[2]) == 1 and math.isnan(float(got[1])) and (got[0] == -1).any()
    exact = restated('sphere', 64)[2]
    for cap in (exact - 1, exact):                                           # stopped one round short; reached but never needed
        got = metrics.optimal_matching(p[None].cuda(), q[None].cuda(), max_rounds=cap)
        assert same_outputs([x[0] for x in got], metrics._torch_optimal_matching(p, q, PHASES, cap), 64)
        assert math.isnan(float(got[1])) == (cap < exact)


@pytest.mark.gpu
def test_other_phase_counts_agree_with_the_restatement():
    p, q = pair('sphere', 63)
    for phases in (1, 10, 26):
        want = metrics._torch_optimal_matching(p, q, phases)
        assert want[2] < 64 * 63 + 4096
        got = metrics.optimal_matching(p[None].cuda(), q[None].cuda(), phases=phases)
        assert same_outputs([x[0] for x in got], want, 63), phases


@pytest.mark.gpu
def test_earth_movers_distance_against_autograd_of_the_same_formula_at_the_returned_matching():
    """The value is the mean of |p1_i - p2[match_i]| in fp32: against float64 on the same values the root of a sum of three squares is
    within 4 2^-24 of itself and the mean adds one rounding to fp32.  The gradient of a term is the unit vector e / |e| over N; in fp32
    e carries 2^-24 scale a component (scale the largest coordinate), so a component of e / |e| is within 8 2^-24 scale / |e|."""
    N = 162
    clouds = [torch.stack([pair('sphere', N)[k], pair('duplicates', N)[k]]) for k in (0, 1)]
    p1, p2 = (x.cuda().requires_grad_() for x in clouds)
    value = metrics.earth_movers_distance(p1, p2)
    assert value.shape == (2,) and value.dtype == torch.float32
    value.sum().backward()
    match = metrics.optimal_matching(p1, p2)[0].cpu()
    assert torch.equal(match[0], restated('sphere', N)[0])
    r1, r2 = (x.double().requires_grad_() for x in clouds)
    diff = r1 - torch.gather(r2, 1, match[..., None].expand(-1, -1, 3))
    want = diff.norm(dim=2).mean(1)
    want.sum().backward()
    assert ((value.detach().cpu().double() - want.detach()).abs() <= 6 * 2.0 ** -24 * want.detach()).all()
    scale = max(float(x.abs().max()) for x in clouds)
    bound = (8 * 2.0 ** -24 * scale / diff.detach().norm(dim=2, keepdim=True) + 2.0 ** -22) / N
    assert ((p1.grad.cpu().double() - r1.grad).abs() <= bound).all()
    moved = torch.gather(p2.grad.cpu().double(), 1, match[..., None].expand(-1, -1, 3))       # the target of i receives minus i's
    assert ((moved + r1.grad).abs() <= bound).all()
    assert metrics.evaluate_distance(clouds[0][0].cuda(), clouds[1][0].cuda(), torch.zeros(1, 3, dtype=torch.long), 'emd') == float(value[0].detach())
