"""icn_sided_sums on the device (metrics.pairwise_sided_sums, pairwise_chamfer, generation_metrics; generation.evaluate_generation).

The kernel's distances are those of k_nn_points bit for bit, so against the shipped route -- sided_distance of every pair on the GPU,
converted to double and summed by torch -- an entry may differ by the order of a double sum alone: 2 N 2^-53 sum, N - 1 additions of
non-negative terms on either side.  Where the distances are small integers every partial sum is exact and the entries must be EQUAL;
+inf entries are equal always.  The point counts sit at the edges of the kernel's geometry, taken from the source constants and checked
against the workspace query: B queries a workgroup (one partial sum each), T targets a tile, four targets a read."""
import functools

import pytest
import torch

from geniconet_amd import _lib, data, generation, metrics, models

from test_abi_pairs import source_constants
from test_generation_metrics import INF, NAN, _lattice_clouds, nonfinite_case, within_the_summation_bound
from test_signed_distance import _profiled

B, T = source_constants()
QUERY_COUNTS = (1, 2, T - 1, T, T + 1, B - 1, B, B + 1, 2 * B + 1)
TARGET_COUNTS = (1, 6, T - 1, T, T + 1, 2 * T + 1, 2 * T + 2)               # 6 and 2 T + 2: two targets left over after the reads of four


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int64)


@functools.lru_cache(maxsize=None)
def _sets(G, R, N, M, family='random'):
    """Two sets of clouds on the CPU, seeded by their sizes; 'integer': coordinates in [-8, 8], so that every distance is an integer
    below 2^10 and every sum of them exact."""
    g = torch.Generator().manual_seed(1000003 * G + 10007 * R + 101 * N + M)
    if family == 'integer':
        return torch.randint(-8, 9, (G, N, 3), generator=g).float(), torch.randint(-8, 9, (R, M, 3), generator=g).float()
    return torch.randn(G, N, 3, generator=g), torch.randn(R, M, 3, generator=g)


def shipped_route(p1, p2):
    """(G, R) float64 on the device by what a user has without the kernel: sided_distance on the expanded copies of both sets."""
    G, R = p1.shape[0], p2.shape[0]
    dist, _ = metrics.sided_distance(p1.repeat_interleave(R, 0), p2.repeat(G, 1, 1))
    return dist.double().sum(1).view(G, R)


def test_the_geometry_constants_are_those_of_the_workspace_query():
    query = _lib.lib().icn_sided_sums_workspace_bytes
    assert query(1, 1, B, 1) == 8 and query(1, 1, B + 1, 1) == 16 and query(3, 5, 2 * B + 1, 7) == 8 * 3 * 5 * 3


@pytest.mark.gpu
def test_matrix_entries_equal_the_shipped_kernel_and_the_one_by_one_calls_bit_for_bit():
    p1, p2 = (x.cuda() for x in _sets(3, 5, 700, 300))
    got = metrics.pairwise_sided_sums(p1, p2)
    assert got.shape == (3, 5) and got.dtype == torch.float64 and got.is_cuda
    assert within_the_summation_bound(got, shipped_route(p1, p2), 700)
    for g in range(3):
        for r in range(5):
            one = metrics.pairwise_sided_sums(p1[g:g + 1], p2[r:r + 1])
            assert torch.equal(_bits(one), _bits(got[g:g + 1, r:r + 1])), (g, r)
    assert within_the_summation_bound(metrics.pairwise_sided_sums(p1, p2.cpu()), got, 0)      # the second set follows the first


@pytest.mark.gpu
@pytest.mark.parametrize('N', QUERY_COUNTS)
def test_point_counts_at_the_edges_of_the_chunks_the_tiles_and_the_reads(N):
    for M in TARGET_COUNTS:
        p1, p2 = (x.cuda() for x in _sets(2, 3, N, M))
        got, want = metrics.pairwise_sided_sums(p1, p2), shipped_route(p1, p2)
        assert within_the_summation_bound(got, want, N), (N, M)
        if N <= 2:                                                           # one addition at most: no order to differ in
            assert torch.equal(_bits(got), _bits(want)), (N, M)
        q1, q2 = (x.cuda() for x in _sets(2, 3, N, M, 'integer'))
        assert torch.equal(_bits(metrics.pairwise_sided_sums(q1, q2)), _bits(shipped_route(q1, q2))), (N, M)


@pytest.mark.gpu
@pytest.mark.parametrize('G,R', ((1, 7), (7, 1), (4, 4)))
def test_set_sizes_one_by_seven_seven_by_one_and_a_set_against_itself(G, R):
    p1, p2 = (x.cuda() for x in _sets(G, R, B + 77, T + 13))
    assert within_the_summation_bound(metrics.pairwise_sided_sums(p1, p2), shipped_route(p1, p2), B + 77)
    d = metrics.pairwise_chamfer(p1, p2, 0.25, 3.0)
    want = metrics.chamfer_distance(p1.repeat_interleave(R, 0), p2.repeat(G, 1, 1), 0.25, 3.0).view(G, R)
    assert d.dtype == torch.float32 and ((d.double() - want.double()).abs() <= 2.0 ** -23 * want.double()).all()
    rooted = metrics.pairwise_chamfer(p1, p2, squared=False)
    want = metrics.chamfer_distance(p1.repeat_interleave(R, 0), p2.repeat(G, 1, 1), squared=False).view(G, R)
    assert ((rooted.double() - want.double()).abs() <= 2.0 ** -23 * want.double()).all()          # the unfused route: chamfer_distance itself
    if G == R:                                                               # p1 is p2: the diagonal is exactly 0
        own = metrics.pairwise_sided_sums(p1, p1)
        assert (own.diagonal() == 0).all() and (own[~torch.eye(G, dtype=torch.bool, device='cuda')] > 0).all()
        both = metrics.pairwise_chamfer(p1, p1)
        assert (both.diagonal() == 0).all() and torch.equal(both, both.t())


@pytest.mark.gpu
def test_non_finite_input_on_the_device_gives_the_cpu_bits():
    p1, p2, want = nonfinite_case()
    got = metrics.pairwise_sided_sums(p1.cuda(), p2.cuda())
    assert torch.equal(_bits(got), _bits(want)) and not torch.isnan(got).any()
    assert torch.equal(_bits(metrics.pairwise_sided_sums(p2.cuda(), p1.cuda())), _bits(metrics.pairwise_sided_sums(p2, p1)))
    assert metrics.generation_metrics(p1.cuda(), p2.cuda()) == metrics.generation_metrics(p1, p2)
    # NaN, +-inf and 2^64 (its square overflows) sprinkled over both sets, at point counts past a chunk and a tile
    q1, q2 = (x.clone() for x in _sets(3, 4, B + 9, T + 6))
    values = (NAN, INF, -INF, 2.0 ** 64)
    for k in range(12):
        q2[k % 4, (37 * k) % (T + 6), k % 3] = values[k % 4]
    q2[3] = NAN
    q1[1, B + 3, 2], q1[2, 5, 0] = NAN, 2.0 ** 64
    got, want = metrics.pairwise_sided_sums(q1.cuda(), q2.cuda()), shipped_route(q1.cuda(), q2.cuda())
    assert within_the_summation_bound(got, want, B + 9)
    assert (got[:, 3] == INF).all() and (got[1] == INF).all() and (got[0, :3] < INF).all()
    assert within_the_summation_bound(got, metrics.pairwise_sided_sums(q1, q2), B + 9)             # and the torch path


@pytest.mark.gpu
def test_two_runs_are_bit_identical_and_an_entry_does_not_depend_on_its_position():
    p1, p2 = (x.cuda() for x in _sets(3, 4, 2 * B + 5, 3 * T + 2))
    first = metrics.pairwise_sided_sums(p1, p2)
    assert torch.equal(_bits(first), _bits(metrics.pairwise_sided_sums(p1, p2)))
    other1, other2 = (x.cuda() for x in _sets(2, 5, 2 * B + 5, 3 * T + 2))
    rows, cols = [4, 0, 2], [1, 8, 3, 6]                                     # where the same clouds sit in a 5 x 9 call
    big1, big2 = torch.cat([other1, other1, other1[:1]]), torch.cat([other2, other2[:4]])
    big1[rows], big2[cols] = p1, p2
    big = metrics.pairwise_sided_sums(big1, big2)
    assert big.shape == (5, 9) and torch.equal(_bits(big[rows][:, cols]), _bits(first))


@pytest.mark.gpu
def test_two_launches_a_call_and_none_on_the_unfused_route():
    p1, p2 = (x.cuda() for x in _sets(3, 5, 700, 300))
    _, kernels = _profiled(lambda: metrics.pairwise_sided_sums(p1, p2))
    assert kernels == {'k_pair_sums': 1, 'k_pair_sums_finish': 1}
    _, kernels = _profiled(lambda: metrics.pairwise_chamfer(p1, p2))
    assert kernels == {'k_pair_sums': 2, 'k_pair_sums_finish': 2}
    _, kernels = _profiled(lambda: metrics.generation_metrics(p1, p2))
    assert kernels == {'k_pair_sums': 6, 'k_pair_sums_finish': 6}
    _, kernels = _profiled(lambda: metrics.pairwise_chamfer(p1, p2, squared=False))
    assert kernels == {'k_nn_points': 6}                                     # cloud g against every cloud of p2, both ways


@pytest.mark.gpu
def test_generation_metrics_on_the_device_are_the_cpu_values():
    """Integer lattices: the sums are exact on either path, so the two distance matrices are equal and COV and 1-NNA with them; MMD is
    held to one fp32 rounding of the double result."""
    g = torch.Generator().manual_seed(77)
    gen = _lattice_clouds(6) + torch.randint(0, 3, (6, 8, 3), generator=g).float()
    ref = _lattice_clouds(5, shift=1.0) + torch.randint(0, 3, (5, 8, 3), generator=g).float()
    assert torch.equal(metrics.pairwise_chamfer(gen.cuda(), ref.cuda()).cpu(), metrics.pairwise_chamfer(gen, ref))
    got, want = metrics.generation_metrics(gen.cuda(), ref.cuda()), metrics.generation_metrics(gen, ref)
    assert got['cov'] == want['cov'] and got['one_nna'] == want['one_nna'] and 0 < want['cov'] <= 1
    assert abs(got['mmd'] - want['mmd']) <= 2.0 ** -23 * want['mmd'] and want['mmd'] > 0
    p1, p2 = _sets(4, 6, 700, 300)                                           # and on random clouds, the matrix to one rounding
    d, d_cpu = metrics.pairwise_chamfer(p1.cuda(), p2.cuda()).cpu().double(), metrics.pairwise_chamfer(p1, p2).double()
    assert ((d - d_cpu).abs() <= 2.0 ** -23 * d_cpu).all()


@pytest.mark.gpu
def test_evaluate_generation_of_an_untrained_vae():
    torch.manual_seed(0)
    model = models.ico2ico_vae(models.default_params('ico2ico_vae', subdivisions=3)).cuda()
    x, _ = data.synthetic_batch(4, 3, seed=5, device='cuda')
    reference = metrics.output2vertices(3, x)
    with torch.no_grad():
        assert tuple(model.eval().encode(x)[0].shape[1:]) == generation.latent_shape(model)
    model.train()
    z = generation.sample_prior(model, 4, seed=2)
    shape = (4,) + generation.latent_shape(model)
    assert z.is_cuda and torch.equal(z.cpu(), torch.randn(shape, generator=torch.Generator().manual_seed(2)))     # the CPU's draw
    vertices = generation.generate_vertices(model, z)
    assert vertices.shape == reference.shape == (4, 642, 3) and model.training and torch.isfinite(vertices).all()
    assert generation.generate_vertices(model, z, batch_size=3).shape == (4, 642, 3)               # three and one
    for samples in (0, 300):
        figures = generation.evaluate_generation(model, reference, 4, seed=2, samples=samples)
        assert 0 < figures['mmd'] < INF and 0.25 <= figures['cov'] <= 1 and 0 <= figures['one_nna'] <= 1
        assert figures == generation.evaluate_generation(model, reference.cpu(), 4, seed=2, samples=samples)
    assert figures != generation.evaluate_generation(model, reference, 4, seed=3, samples=300)
    assert generation.evaluate_generation(model, reference, 4, seed=2) == metrics.generation_metrics(vertices, reference)
