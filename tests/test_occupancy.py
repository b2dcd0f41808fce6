"""Occupancy histograms and their Jensen-Shannon divergence by their definition in torch (metrics._torch_occupancy_counts,
metrics._torch_occupancy_jsd; include/icn_occupancy.h), on CPU tensors: the histogram against plain Python loops over numpy.float32
scalars on points built to sit on ties, one ulp either side of them, on and beyond both boundaries, where t overflows and where a
coordinate is not finite; the divergence against a float64 numpy spelling and its known answers; the options of the evaluation
entry points; the argument checks.  tests/test_occupancy_gpu.py holds the kernels to these restatements."""
import functools

import numpy as np
import pytest
import torch

from geniconet_amd import generation, metrics

INF, NAN = float('inf'), float('nan')
JSD_BOUND = 2.0 ** -44                # include/icn_occupancy.h: ten roundings a summand and R^3 / T + log2 T a sum, times 2^-53, with room
RESOLUTIONS = (1, 2, 3, 28, 32)
F32 = np.float32


def lattices(R):
    """The lattices a resolution is tested on: the default cube, the literature's unit cube, and for R >= 2 the lattice of spacing 1
    from 0, on which t = x exactly and k + 0.5 is a tie exactly."""
    return [(-1.0, 1.0), (-0.5, 0.5)] + ([(0.0, float(R - 1))] if R > 1 else [])


def lattice_numbers(R, bounds):
    """(lo, inv_spacing) as numpy.float32, computed as the public functions document it."""
    lo, hi = bounds
    return F32(lo), (F32((R - 1) / (hi - lo)) if R > 1 else F32(1.0))


def loop_axis(x, lo, inv, R):
    """The cell index of one coordinate by the header's three lines, every operation a numpy.float32 operation of its own."""
    with np.errstate(over='ignore'):
        t = F32(F32(x - lo) * inv)
        u = np.floor(F32(t + F32(0.5)))
    return int(min(max(u, F32(0.0)), F32(R - 1)))


def loop_counts(points, R, bounds, per_cloud=False):
    """(counts, dropped) of points (B, N, 3) float32 numpy by plain loops."""
    lo, inv = lattice_numbers(R, bounds)
    B = points.shape[0]
    counts, dropped = np.zeros((B, R, R, R), dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        for x, y, z in points[b]:
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(z)):
                dropped[b] += 1
                continue
            counts[b, loop_axis(x, lo, inv, R), loop_axis(y, lo, inv, R), loop_axis(z, lo, inv, R)] += 1
    return (counts, dropped) if per_cloud else (counts.sum(0, dtype=np.int32), dropped.sum(dtype=np.int32))


def edge_coordinates(R, bounds):
    """fp32 coordinates around everything the index definition decides: every tie k + 0.5 (or the nearest fp32 numbers to it) with
    two ulps either side, every lattice point, both boundaries with an ulp either side, points far outside, +-3e38 (t overflows), 0."""
    lo, inv = lattice_numbers(R, bounds)
    hi = F32(bounds[1])
    xs = [F32(0.0), F32(-0.0), F32(3e38), F32(-3e38), F32(1e30), F32(-1e30), lo - F32(7.0), hi + F32(7.0)]
    for k in range(-1, R + 1):
        for half in (0.0, 0.5):
            x = F32(float(lo) + (k + half) / float(inv))
            for _ in range(2):
                x = np.nextafter(x, F32(-INF))
            for _ in range(5):
                xs.append(F32(x))
                x = np.nextafter(x, F32(INF))
    return np.array(xs, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def edge_cloud(R, bounds, clouds=2):
    """(clouds, N, 3) float32 tensor: every edge coordinate on every axis against a few partners, then the non-finite points -- NaN,
    +inf and -inf in each position, alone and together with an edge coordinate.  Shared by the tests of both files; never modified."""
    xs = edge_coordinates(R, bounds)
    rng = np.random.RandomState(R)
    rows = []
    for axis in range(3):
        p = rng.uniform(bounds[0] - 0.3, bounds[1] + 0.3, size=(len(xs), 3)).astype(np.float32)
        p[:, axis] = xs
        rows.append(p)
    rows.append(np.stack([xs, np.roll(xs, 1), np.roll(xs, 2)], 1))
    bad = []
    for v in (NAN, INF, -INF):
        for axis in range(3):
            p = np.array([0.25, -0.25, 0.5], dtype=np.float32)
            p[axis] = v
            bad.append(p)
            q = np.array([3e38, xs[5], xs[-1]], dtype=np.float32)
            q[axis] = v
            bad.append(q)
    bad.append(np.array([NAN, INF, -INF], dtype=np.float32))
    pts = np.concatenate(rows + [np.stack(bad)]).astype(np.float32)
    pts = pts[rng.permutation(len(pts))]
    n = len(pts) // clouds
    return torch.from_numpy(pts[:n * clouds].reshape(clouds, n, 3).copy())


def numpy_jsd(a, b):
    """The divergence in float64 numpy: the header's formula, numpy's order of summation."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    A, B = int(a.sum()), int(b.sum())
    if A == 0 or B == 0:
        return NAN
    p, q = a.astype(np.float64) / float(A), b.astype(np.float64) / float(B)
    m = 0.5 * (p + q)
    tp, tq = np.zeros_like(p), np.zeros_like(q)
    tp[a > 0] = p[a > 0] * np.log2(p[a > 0] / m[a > 0])
    tq[b > 0] = q[b > 0] * np.log2(q[b > 0] / m[b > 0])
    return float((0.5 * (tp + tq)).sum())


def histogram_pairs(R):
    """Pairs of (R, R, R) int32 histograms: dense random ones of unequal totals, sparse ones of one count in a few cells (overlapping
    in some), a peaked one against a flat one."""
    g = torch.Generator().manual_seed(100 + R)
    cells = R ** 3
    dense = [torch.randint(1, 1000, (cells,), generator=g, dtype=torch.int32) for _ in range(2)]
    dense[0][3::7], dense[1] = 0, dense[1] * 3 + 1                           # empty cells on one side only, unequal totals
    few = min(cells, 5)
    sparse = [torch.zeros(cells, dtype=torch.int32) for _ in range(2)]
    sparse[0][torch.randperm(cells, generator=g)[:few]] = 1
    sparse[1][torch.randperm(cells, generator=g)[:few]] = 1
    sparse[1][sparse[0].nonzero()[0]] = 1                                    # at least one shared cell
    peaked = torch.zeros(cells, dtype=torch.int32)
    peaked[cells // 2] = 2 ** 31 - 1
    flat = torch.full((cells,), 65535, dtype=torch.int32)
    return [tuple(x.reshape(R, R, R) for x in pair) for pair in (dense, sparse, (peaked, flat), (dense[0], sparse[1]))]


def bits(x):
    return x.reshape(1).view(torch.int64)


# ---- the histogram ------------------------------------------------------------------------------------------------------------------------
def test_the_built_points_sit_exactly_on_ties_and_one_ulp_either_side():
    for R in (2, 3, 28, 32):
        lo, inv = lattice_numbers(R, (0.0, float(R - 1)))
        assert lo == 0.0 and inv == 1.0
        xs = edge_coordinates(R, (0.0, float(R - 1)))
        for k in range(R - 1):
            tie = F32(k + 0.5)
            below, above = np.nextafter(tie, F32(-INF)), np.nextafter(tie, F32(INF))
            assert {tie, below, above} <= set(xs.tolist())
            assert loop_axis(tie, lo, inv, R) == k + 1 and loop_axis(above, lo, inv, R) == k + 1                                         # up
            # one ulp below the tie stays down -- but for k = 0, where t + 0.5 = 1 - 2^-25 is itself a tie of the ADDITION and rounds
            # to 1: the definition rounds every operation on its own, and that is what it says about this point
            assert loop_axis(below, lo, inv, R) == (k if k else 1)
    lo, inv = lattice_numbers(28, (-1.0, 1.0))
    assert inv == 13.5
    for x, cell in ((-1.0, 0), (1.0, 27), (-1.5, 0), (1.5, 27), (3e38, 27), (-3e38, 0), (0.0, 14)):      # t = 13.5 at 0: a tie, up
        assert loop_axis(F32(x), lo, inv, 28) == cell
    with np.errstate(over='ignore'):
        assert np.isinf(F32(F32(3e38) - lo) * inv)                                                     # t overflows, and is clamped


@pytest.mark.parametrize('R', RESOLUTIONS)
def test_the_restatement_equals_the_loops_on_ties_boundaries_overflow_and_non_finite_points(R):
    for bounds in lattices(R):
        pts = edge_cloud(R, bounds)
        for per_cloud in (False, True):
            counts, dropped = metrics.occupancy_counts(pts, R, bounds, per_cloud=per_cloud)
            want, want_dropped = loop_counts(pts.numpy(), R, bounds, per_cloud)
            assert counts.dtype == dropped.dtype == torch.int32
            assert counts.shape == ((2, R, R, R) if per_cloud else (R, R, R)) and dropped.shape == ((2,) if per_cloud else ())
            assert np.array_equal(counts.numpy(), want) and np.array_equal(dropped.numpy(), want_dropped), (R, bounds, per_cloud)
        assert int(dropped.sum()) == int((~torch.isfinite(pts).all(-1)).sum()) >= 18
        assert int(counts.sum()) + int(dropped.sum()) == pts.shape[0] * pts.shape[1]


@pytest.mark.parametrize('R', RESOLUTIONS)
def test_per_cloud_rows_sum_to_the_set_histogram_and_equal_the_single_cloud_calls(R):
    pts = torch.cat([edge_cloud(R, (-1.0, 1.0)), torch.rand(2, edge_cloud(R, (-1.0, 1.0)).shape[1], 3, generator=torch.Generator().manual_seed(R)) * 2.4 - 1.2])
    whole, dropped = metrics.occupancy_counts(pts, R)
    rows, row_dropped = metrics.occupancy_counts(pts, R, per_cloud=True)
    assert torch.equal(rows.sum(0, dtype=torch.int32), whole) and int(row_dropped.sum()) == int(dropped)
    for b in range(pts.shape[0]):
        one, one_dropped = metrics.occupancy_counts(pts[b:b + 1], R)
        assert torch.equal(one, rows[b]) and int(one_dropped) == int(row_dropped[b])


def test_other_dtypes_are_converted_to_fp32_first_and_the_default_is_28_on_the_tanh_cube():
    pts = edge_cloud(28, (-1.0, 1.0))
    want = metrics.occupancy_counts(pts, 28, (-1.0, 1.0))
    for got in (metrics.occupancy_counts(pts), metrics.occupancy_counts(pts.double()), metrics.occupancy_counts(pts, bounds=(-1, 1))):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    half = torch.rand(2, 50, 3, generator=torch.Generator().manual_seed(3)).half()
    assert torch.equal(metrics.occupancy_counts(half)[0], metrics.occupancy_counts(half.float())[0])
    assert metrics.occupancy_counts(pts.requires_grad_(False))[0].requires_grad is False


# ---- the divergence -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('R', RESOLUTIONS)
def test_the_restated_divergence_equals_the_numpy_spelling(R):
    for a, b in histogram_pairs(R):
        got = metrics.occupancy_jsd(a, b)
        assert got.dtype == torch.float64 and got.dim() == 0
        want = numpy_jsd(a.numpy(), b.numpy())
        assert abs(float(got) - want) <= JSD_BOUND, (R, float(got), want)
        assert 0.0 <= float(got) <= 1.0 + JSD_BOUND
        assert torch.equal(bits(metrics.occupancy_jsd(b, a)), bits(got))                          # the same bits, swapped
        assert float(metrics.occupancy_jsd(a, a)) == 0.0 and float(metrics.occupancy_jsd(b, b)) == 0.0
        assert torch.equal(bits(metrics.occupancy_jsd(a.long(), b.long())), bits(got))            # any integer dtype


def test_the_known_answers_of_the_divergence():
    def h(*counts):
        x = torch.zeros(8, dtype=torch.int32)
        x[:len(counts)] = torch.tensor(counts, dtype=torch.int32)
        return x.reshape(2, 2, 2)
    assert abs(float(metrics.occupancy_jsd(h(2, 0), h(1, 1))) - 0.3112781244591328) <= JSD_BOUND
    assert abs(float(metrics.occupancy_jsd(h(3, 5, 0, 0), h(0, 0, 7, 1))) - 1.0) <= JSD_BOUND     # disjoint supports
    assert abs(float(metrics.occupancy_jsd(h(1), h(0, 0, 0, 0, 0, 0, 0, 9))) - 1.0) <= JSD_BOUND
    assert float(metrics.occupancy_jsd(h(3, 5, 7), h(3, 5, 7))) == 0.0                            # exactly
    assert float(metrics.occupancy_jsd(h(3, 5, 7), h(6, 10, 14))) == 0.0                          # the same distribution: p == q bit for bit
    empty = h()
    for a, b in ((empty, h(1, 1)), (h(1, 1), empty), (empty, empty)):
        assert np.isnan(float(metrics.occupancy_jsd(a, b))) and np.isnan(numpy_jsd(a.numpy(), b.numpy()))
    one = torch.tensor([[[5]]], dtype=torch.int32)                                                # R = 1: one cell, always 0
    assert float(metrics.occupancy_jsd(one, one * 3)) == 0.0


def test_jensen_shannon_divergence_is_the_divergence_of_the_two_set_histograms():
    g = torch.Generator().manual_seed(11)
    gen, ref = torch.rand(5, 300, 3, generator=g) * 1.6 - 0.8, torch.rand(3, 200, 3, generator=g) * 2.0 - 1.0
    for R, bounds in ((28, (-1.0, 1.0)), (8, (-0.5, 0.5)), (1, (-1.0, 1.0))):
        want = metrics.occupancy_jsd(metrics.occupancy_counts(gen, R, bounds)[0], metrics.occupancy_counts(ref, R, bounds)[0])
        got = metrics.jensen_shannon_divergence(gen, ref, R, bounds)
        assert got.dtype == torch.float64 and got.dim() == 0 and torch.equal(bits(got), bits(want))
        want_np = numpy_jsd(loop_counts(gen.numpy(), R, bounds)[0], loop_counts(ref.numpy(), R, bounds)[0])
        assert abs(float(got) - want_np) <= JSD_BOUND
    assert torch.equal(bits(metrics.jensen_shannon_divergence(gen, ref)), bits(metrics.jensen_shannon_divergence(gen, ref, 28, (-1.0, 1.0))))
    assert float(metrics.jensen_shannon_divergence(gen, gen)) == 0.0
    assert float(metrics.jensen_shannon_divergence(gen, gen[[4, 0, 2, 1, 3]])) == 0.0            # a property of the set, not of its order
    far = gen + 5.0                                                                              # everything clamped into one corner cell
    assert 0.9 < float(metrics.jensen_shannon_divergence(gen, far)) <= 1.0 + JSD_BOUND
    assert np.isnan(float(metrics.jensen_shannon_divergence(gen, torch.full_like(ref, NAN))))


# ---- the options of the evaluation entry points -------------------------------------------------------------------------------------------
def small_sets():
    g = torch.Generator().manual_seed(5)
    return torch.rand(4, 40, 3, generator=g) * 1.8 - 0.9, torch.rand(3, 50, 3, generator=g) * 1.8 - 0.9


def test_generation_metrics_adds_the_key_only_when_asked():
    gen, ref = small_sets()
    plain = metrics.generation_metrics(gen, ref)
    assert list(plain) == ['mmd', 'cov', 'one_nna']
    assert metrics.generation_metrics(gen, ref, jsd=0) == plain and list(metrics.generation_metrics(gen, ref, jsd=0)) == list(plain)
    with_jsd = metrics.generation_metrics(gen, ref, jsd=4)
    assert list(with_jsd) == ['mmd', 'cov', 'one_nna', 'jsd'] and {k: with_jsd[k] for k in plain} == plain
    assert isinstance(with_jsd['jsd'], float) and with_jsd['jsd'] == float(metrics.jensen_shannon_divergence(gen, ref, 4))
    assert 0.0 < with_jsd['jsd'] < 1.0
    thinned = metrics.generation_metrics(gen, ref, points=16, jsd=4)                              # on the sets the matrices see
    from geniconet_amd import sampling
    assert thinned['jsd'] == float(metrics.jensen_shannon_divergence(sampling.farthest_points(gen, 16), sampling.farthest_points(ref, 16), 4))
    assert {k: thinned[k] for k in plain} == metrics.generation_metrics(gen, ref, points=16)
    emd = metrics.generation_metrics(gen[:, :20], ref[:, :20], distance='emd', jsd=4)
    assert list(emd) == ['mmd', 'cov', 'one_nna', 'jsd']
    assert emd['jsd'] == float(metrics.jensen_shannon_divergence(gen[:, :20], ref[:, :20], 4))
    assert {k: emd[k] for k in plain} == metrics.generation_metrics(gen[:, :20], ref[:, :20], distance='emd')


def test_evaluate_generation_checks_the_option_before_it_draws_anything():
    for bad in (-1, 33, 2.0, True, '8'):
        with pytest.raises(ValueError, match='evaluate_generation: jsd must be an integer in \\[0, 32\\]'):
            generation.evaluate_generation(None, torch.zeros(2, 5, 3), 2, jsd=bad)


# ---- the argument checks ------------------------------------------------------------------------------------------------------------------
def test_the_argument_checks_raise_value_errors():
    pts = torch.zeros(2, 5, 3)
    for bad in (None, [[0.0, 0.0, 0.0]], torch.zeros(5, 3), torch.zeros(2, 5, 2), torch.zeros(0, 5, 3), torch.zeros(2, 0, 3),
                torch.zeros(2, 5, 3, dtype=torch.int32)):
        with pytest.raises(ValueError, match='occupancy_counts: expected the set'):
            metrics.occupancy_counts(bad)
    with pytest.raises(ValueError, match='occupancy_counts: 65536 clouds of 32768 points: B N must fit an int32'):
        metrics.occupancy_counts(torch.zeros(1, 1, 3).expand(65536, 32768, 3))                   # shapes only: nothing is materialised
    for bad in (0, 33, -1, 28.0, True, None):
        with pytest.raises(ValueError, match='occupancy_counts: resolution must be an integer in \\[1, 32\\]'):
            metrics.occupancy_counts(pts, bad)
        with pytest.raises(ValueError, match='jensen_shannon_divergence: resolution must be an integer in \\[1, 32\\]'):
            metrics.jensen_shannon_divergence(pts, pts, bad)
    for bad in ((1.0, 1.0), (1.0, -1.0), (-1.0,), (-1.0, 0.0, 1.0), (NAN, 1.0), (-INF, 1.0), (0.0, INF), ('a', 'b'), None, 1.0,
                (torch.tensor(-1.0), torch.tensor(1.0)), (False, True)):
        with pytest.raises(ValueError, match='occupancy_counts: bounds must be two finite numbers'):
            metrics.occupancy_counts(pts, 28, bad)
        with pytest.raises(ValueError, match='jensen_shannon_divergence: bounds must be two finite numbers'):
            metrics.jensen_shannon_divergence(pts, pts, 28, bad)
    for bad in ((-1e300, 1e300), (0.0, 1e-300), (1e39, 1e40)):                                    # no fp32 lattice
        with pytest.raises(ValueError, match='occupancy_counts: bounds .* give no fp32 lattice of 28 points an axis'):
            metrics.occupancy_counts(pts, 28, bad)
    with pytest.raises(ValueError, match='jensen_shannon_divergence: expected the second set'):
        metrics.jensen_shannon_divergence(pts, torch.zeros(5, 3))
    h = torch.zeros(4, 4, 4, dtype=torch.int32)
    for bad in (None, h.float(), h.bool(), h[0], h[:, :3], torch.zeros(33, 33, 33, dtype=torch.int32), torch.zeros(0, 0, 0, dtype=torch.int32)):
        with pytest.raises(ValueError, match='occupancy_jsd: expected the first histogram'):
            metrics.occupancy_jsd(bad, h)
        with pytest.raises(ValueError, match='occupancy_jsd: expected the second histogram'):
            metrics.occupancy_jsd(h, bad)
    with pytest.raises(ValueError, match='occupancy_jsd: the histograms must have one shape and one device'):
        metrics.occupancy_jsd(h, torch.zeros(5, 5, 5, dtype=torch.int32))
    for bad in (-1, 33, 4.0, True, None):
        with pytest.raises(ValueError, match='generation_metrics: jsd must be an integer in \\[0, 32\\]'):
            metrics.generation_metrics(pts, pts, jsd=bad)
