"""icn_point_occupancy and icn_occupancy_jsd on the device (metrics.occupancy_counts, occupancy_jsd, jensen_shannon_divergence; the
`jsd=` option of metrics.generation_metrics and generation.evaluate_generation).

The histogram kernel is held to the restatement metrics._torch_occupancy_counts on CPU tensors BIT FOR BIT, in counts and in dropped:
integer counts are order-free, so nothing may differ however the launcher splits the points among workgroups.  The point counts sit
around a wave and one point either side of where the launcher takes another workgroup (a piece holds at least OCC_POINTS points, read
from the source), for the set form and the per-cloud form; the resolutions are the smallest, the papers' 28 and 32, the LDS maximum.
The divergence kernel is held to the float64 numpy spelling within 2^-44 (include/icn_occupancy.h derives the bound) and to its three
exact properties."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, data, generation, metrics, models

from test_abi import ROOT
from test_occupancy import INF, JSD_BOUND, NAN, bits, edge_cloud, histogram_pairs, lattices, numpy_jsd
from test_signed_distance import _profiled


def source_constants():
    """(points a piece holds at least, workgroups a launch takes at most) as csrc/icn_voxel.hip states them."""
    src = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'icn_voxel.hip')).read()
    return tuple(int(re.search(r'constexpr int %s = (\d+);' % name, src).group(1)) for name in ('OCC_POINTS', 'OCC_MAX_WG'))


PIECE, MAX_WG = source_constants()
COUNTS = (1, 63, 64, 65, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 2 * PIECE + 1)
RESOLUTIONS = (1, 2, 28, 32)
DEFAULT = (-1.0, 1.0)


def test_the_point_counts_sit_either_side_of_every_change_in_the_number_of_workgroups():
    """With B in (1, 3): one piece becomes two at PIECE + 1 points of a histogram (a cloud, or for the set form the heap of B N points),
    two become three at 2 PIECE + 1; for the set of three clouds the heap crosses 3 PIECE and 6 PIECE as well."""
    assert (PIECE, MAX_WG) == (16384, 256)
    L = _lib.lib()
    cells = 28 ** 3

    def pieces(B, N, per_cloud):
        size = L.icn_point_occupancy_workspace_bytes(B, N, 28, per_cloud)
        return 1 if size == 16 else size // ((cells + 1) * 4) // (B if per_cloud else 1)
    assert [pieces(1, N, 0) for N in COUNTS] == [pieces(1, N, 1) for N in COUNTS] == [pieces(3, N, 1) for N in COUNTS] == [1] * 6 + [2, 2, 3]
    assert [pieces(3, N, 0) for N in COUNTS] == [1] * 4 + [3, 3, 4, 6, 7]


@functools.lru_cache(maxsize=None)
def clouds(B, N):
    """(B, N, 3) on the CPU: uniform in a cube a fifth wider than the default lattice, every 97th point with a non-finite coordinate."""
    g = torch.Generator().manual_seed(1000 * B + N)
    p = torch.rand(B, N, 3, generator=g) * 2.4 - 1.2
    flat = p.view(-1, 3)
    flat[5::97, 1] = NAN
    flat[50::97 * 3, 2] = INF
    return p


@functools.lru_cache(maxsize=None)
def restated(B, N, R, per_cloud):
    """The restatement on the CPU, computed once per shape and shared."""
    return metrics.occupancy_counts(clouds(B, N), R, DEFAULT, per_cloud)


def same(got, want):
    return all(g.is_cuda and g.dtype == torch.int32 and g.shape == w.shape and torch.equal(g.cpu(), w) for g, w in zip(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize('R', RESOLUTIONS)
@pytest.mark.parametrize('B', (1, 3))
@pytest.mark.parametrize('N', COUNTS)
def test_the_kernel_equals_the_restatement_bit_for_bit_around_a_wave_and_every_piece_edge(N, B, R):
    pts = clouds(B, N).cuda()
    for per_cloud in (False, True):
        got = metrics.occupancy_counts(pts, R, DEFAULT, per_cloud)
        assert same(got, restated(B, N, R, per_cloud)), (N, B, R, per_cloud)
        assert int(got[0].sum()) + int(got[1].sum()) == B * N


@pytest.mark.gpu
def test_one_launch_for_one_piece_a_histogram_and_a_second_that_adds_the_pieces():
    small, large = clouds(3, PIECE).cuda(), clouds(3, PIECE + 1).cuda()
    assert _profiled(lambda: metrics.occupancy_counts(small, 28, per_cloud=True))[1] == {'k_point_occupancy': 1}
    assert _profiled(lambda: metrics.occupancy_counts(small[:1], 28))[1] == {'k_point_occupancy': 1}
    assert _profiled(lambda: metrics.occupancy_counts(small, 28))[1] == {'k_point_occupancy': 1, 'k_occupancy_reduce': 1}
    assert _profiled(lambda: metrics.occupancy_counts(large, 28, per_cloud=True))[1] == {'k_point_occupancy': 1, 'k_occupancy_reduce': 1}
    a, b = small[:2], large[:2]
    assert _profiled(lambda: metrics.jensen_shannon_divergence(a, b))[1] == {'k_point_occupancy': 2, 'k_occupancy_reduce': 2, 'k_occupancy_jsd': 1}


@pytest.mark.gpu
@pytest.mark.parametrize('R', RESOLUTIONS)
def test_ties_boundaries_overflowing_and_non_finite_points_land_where_the_restatement_puts_them(R):
    for bounds in lattices(R) if R > 1 else lattices(R)[:1]:
        pts = edge_cloud(R, bounds)
        for per_cloud in (False, True):
            assert same(metrics.occupancy_counts(pts.cuda(), R, bounds, per_cloud), metrics.occupancy_counts(pts, R, bounds, per_cloud)), (R, bounds)


@pytest.mark.gpu
def test_every_point_in_one_cell():
    pts = torch.full((8, 4096, 3), 0.3).cuda()                               # all 64 lanes of every wave add to one address
    counts, dropped = metrics.occupancy_counts(pts, 28)                      # two pieces of 16 384 points
    assert int(counts[18, 18, 18]) == 32768 == int(counts.sum()) and int(dropped) == 0          # (0.3 + 1) 13.5 = 17.55
    rows, row_dropped = metrics.occupancy_counts(pts, 28, per_cloud=True)
    assert (rows[:, 18, 18, 18] == 4096).all() and int(rows.sum()) == 32768 and not row_dropped.any()
    lost = metrics.occupancy_counts(torch.full((8, 4096, 3), NAN).cuda(), 32)                    # ... and every point dropped
    assert int(lost[1]) == 32768 and not lost[0].any()


@pytest.mark.gpu
def test_rows_equal_single_cloud_calls_their_sum_is_the_set_histogram_and_two_runs_give_the_same_bytes():
    for N, R in ((65, 2), (PIECE + 1, 28), (2 * PIECE + 1, 32)):
        pts = clouds(3, N).cuda()
        rows, row_dropped = metrics.occupancy_counts(pts, R, per_cloud=True)
        whole, dropped = metrics.occupancy_counts(pts, R)
        assert torch.equal(rows.sum(0, dtype=torch.int32), whole) and int(row_dropped.sum()) == int(dropped)
        for b in range(3):
            one, one_dropped = metrics.occupancy_counts(pts[b:b + 1], R)     # a view that starts anywhere: N is odd
            assert torch.equal(one, rows[b]) and int(one_dropped) == int(row_dropped[b])
        again = metrics.occupancy_counts(pts, R, per_cloud=True), metrics.occupancy_counts(pts, R)
        assert torch.equal(again[0][0], rows) and torch.equal(again[0][1], row_dropped)
        assert torch.equal(again[1][0], whole) and torch.equal(again[1][1], dropped)


@pytest.mark.gpu
def test_a_view_that_is_not_16_byte_aligned_takes_the_scalar_loads_and_counts_the_same():
    for N in (65, PIECE + 1):
        base = clouds(1, 3 * N + 1).cuda()[0]                                # (3 N + 1, 3)
        view = base[1:].view(3, N, 3)
        assert view.is_contiguous() and view.data_ptr() % 16 == 12
        want = metrics.occupancy_counts(view.cpu(), 28, per_cloud=True)
        assert same(metrics.occupancy_counts(view, 28, per_cloud=True), want)
        assert same(metrics.occupancy_counts(view, 28), metrics.occupancy_counts(view.cpu(), 28))


@pytest.mark.gpu
def test_a_set_larger_than_every_workgroup_s_least_piece_is_cut_into_the_most_workgroups():
    N = MAX_WG * PIECE + 5                                                   # 257 pieces wanted, 256 taken: a piece of 16 388 points
    pts = clouds(1, N)
    assert _lib.lib().icn_point_occupancy_workspace_bytes(1, N, 2, 0) == MAX_WG * (8 + 1) * 4
    assert same(metrics.occupancy_counts(pts.cuda(), 2), metrics.occupancy_counts(pts, 2))


@pytest.mark.gpu
def test_the_entry_with_no_dropped_counter_and_a_workspace_of_exactly_the_size_asked():
    L = _lib.api()
    for B, N, per_cloud in ((3, 65, 0), (3, 65, 1), (3, PIECE + 1, 0), (3, PIECE + 1, 1)):
        pts = clouds(B, N).cuda()
        want = restated(B, N, 28, bool(per_cloud))[0]
        size = L.icn_point_occupancy_workspace_bytes(B, N, 28, per_cloud)
        ws = torch.full((size,), 0xff, dtype=torch.uint8, device='cuda')     # needs no initialisation: garbage in
        counts = torch.full(want.shape, -7, dtype=torch.int32, device='cuda')
        L.icn_point_occupancy(pts.data_ptr(), B, N, 28, -1.0, 13.5, per_cloud, counts.data_ptr(), None, ws.data_ptr(), size, _lib.stream())
        assert torch.equal(counts.cpu(), want)
        with pytest.raises(RuntimeError, match='icn_point_occupancy failed: icn_point_occupancy: bad sizes'):
            L.icn_point_occupancy(pts.data_ptr(), B, N, 28, -1.0, 13.5, per_cloud, counts.data_ptr(), None, ws.data_ptr(), size - 1, _lib.stream())


# ---- the divergence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('R', RESOLUTIONS)
def test_the_divergence_kernel_holds_to_the_numpy_spelling_and_to_its_exact_properties(R):
    worst = 0.0
    for a, b in histogram_pairs(R):
        (got, kernels) = _profiled(lambda: metrics.occupancy_jsd(a.cuda(), b.cuda()))
        assert kernels == {'k_occupancy_jsd': 1} and got.is_cuda and got.dtype == torch.float64 and got.dim() == 0
        want = numpy_jsd(a.numpy(), b.numpy())
        worst = max(worst, abs(float(got) - want))
        print('R = %d: kernel %.17g, numpy %.17g, |difference| %.3g = %.3f of the bound' % (R, float(got), want, abs(float(got) - want),
                                                                                           abs(float(got) - want) / JSD_BOUND))
        assert abs(float(got) - want) <= JSD_BOUND, (R, float(got), want)
        assert abs(float(got) - float(metrics.occupancy_jsd(a, b))) <= JSD_BOUND                 # ... and to the restatement
        assert 0.0 <= float(got) <= 1.0 + JSD_BOUND
        assert torch.equal(bits(metrics.occupancy_jsd(b.cuda(), a.cuda()).cpu()), bits(got.cpu()))          # the same bits, swapped
        assert torch.equal(bits(metrics.occupancy_jsd(a.cuda(), b.cuda()).cpu()), bits(got.cpu()))          # ... and run to run
        assert float(metrics.occupancy_jsd(a.cuda(), a.cuda())) == 0.0 and float(metrics.occupancy_jsd(b.cuda(), b.cuda())) == 0.0
    assert worst <= JSD_BOUND


@pytest.mark.gpu
def test_the_known_answers_of_the_divergence_on_the_device():
    def h(*counts):
        x = torch.zeros(8, dtype=torch.int32)
        x[:len(counts)] = torch.tensor(counts, dtype=torch.int32)
        return x.reshape(2, 2, 2).cuda()
    assert abs(float(metrics.occupancy_jsd(h(2, 0), h(1, 1))) - 0.3112781244591328) <= JSD_BOUND
    assert abs(float(metrics.occupancy_jsd(h(3, 5, 0, 0), h(0, 0, 7, 1))) - 1.0) <= JSD_BOUND     # disjoint supports
    assert float(metrics.occupancy_jsd(h(3, 5, 7), h(6, 10, 14))) == 0.0                          # one distribution: p == q bit for bit
    for a, b in ((h(), h(1, 1)), (h(1, 1), h()), (h(), h())):
        assert np.isnan(float(metrics.occupancy_jsd(a, b)))
    one = torch.tensor([[[5]]], dtype=torch.int32).cuda()                                         # R = 1: one cell, always 0
    assert float(metrics.occupancy_jsd(one, one * 3)) == 0.0
    full = torch.full((32, 32, 32), 65535, dtype=torch.int32).cuda()                              # the totals do not fit 32 bits
    peak = torch.zeros(32, 32, 32, dtype=torch.int32)
    peak[31, 31, 31] = 2 ** 31 - 1
    assert abs(float(metrics.occupancy_jsd(full, peak.cuda())) - numpy_jsd(full.cpu().numpy(), peak.numpy())) <= JSD_BOUND


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synthetic_sets():
    """Two small sets of vertex clouds of synthetic shapes at subdivision 2 (162 points a cloud), on the CPU."""
    a = metrics.output2vertices(2, data.synthetic_batch(5, 2, seed=3)[0])
    b = metrics.output2vertices(2, data.synthetic_batch(4, 2, seed=8)[0])
    return a, b


@pytest.mark.gpu
def test_jensen_shannon_divergence_of_two_synthetic_sets_equals_the_cpu_route():
    a, b = synthetic_sets()
    for R, bounds in ((28, DEFAULT), (8, DEFAULT), (28, (-0.5, 0.5))):
        for x in (a, b):
            assert same(metrics.occupancy_counts(x.cuda(), R, bounds), metrics.occupancy_counts(x, R, bounds))
        got, want = metrics.jensen_shannon_divergence(a.cuda(), b.cuda(), R, bounds), metrics.jensen_shannon_divergence(a, b, R, bounds)
        assert got.is_cuda and got.dtype == torch.float64 and abs(float(got) - float(want)) <= JSD_BOUND
        assert 0.0 < float(got) <= 1.0 + JSD_BOUND
    assert float(metrics.jensen_shannon_divergence(a.cuda(), a.cuda())) == 0.0
    assert float(metrics.jensen_shannon_divergence(a.cuda(), b)) == float(metrics.jensen_shannon_divergence(a.cuda(), b.cuda()))   # moved over


@pytest.mark.gpu
def test_generation_metrics_carries_the_value():
    a, b = (x.cuda() for x in synthetic_sets())
    plain = metrics.generation_metrics(a, b)
    assert list(plain) == ['mmd', 'cov', 'one_nna'] and metrics.generation_metrics(a, b, jsd=0) == plain
    got = metrics.generation_metrics(a, b, jsd=8)
    assert got == dict(plain, jsd=float(metrics.jensen_shannon_divergence(a, b, 8))) and list(got) == ['mmd', 'cov', 'one_nna', 'jsd']
    assert abs(got['jsd'] - float(metrics.jensen_shannon_divergence(*synthetic_sets(), 8))) <= JSD_BOUND
    from geniconet_amd import sampling
    thinned = metrics.generation_metrics(a, b, points=50, jsd=8)
    assert thinned['jsd'] == float(metrics.jensen_shannon_divergence(sampling.farthest_points(a, 50), sampling.farthest_points(b, 50), 8))


@pytest.mark.gpu
def test_evaluate_generation_of_an_untrained_vae_with_the_jsd_column():
    torch.manual_seed(0)
    model = models.ico2ico_vae(models.default_params('ico2ico_vae', subdivisions=3)).cuda()
    reference = metrics.output2vertices(3, data.synthetic_batch(4, 3, seed=5, device='cuda')[0])
    vertices = generation.generate_vertices(model, generation.sample_prior(model, 4, seed=2))
    plain = generation.evaluate_generation(model, reference, 4, seed=2)
    assert generation.evaluate_generation(model, reference, 4, seed=2, jsd=0) == plain and list(plain) == ['mmd', 'cov', 'one_nna']
    assert generation.evaluate_generation(model, reference, 4, seed=2, jsd=8) == dict(plain, jsd=float(metrics.jensen_shannon_divergence(vertices, reference, 8)))
    sampled = generation.evaluate_generation(model, reference, 4, seed=2, samples=300, points=100, jsd=8)
    assert {k: sampled[k] for k in plain} == generation.evaluate_generation(model, reference, 4, seed=2, samples=300, points=100)
    assert 0.0 <= sampled['jsd'] <= 1.0 + JSD_BOUND
