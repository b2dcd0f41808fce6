"""The chamfer matrix of two sets of clouds and the generation metrics on it (metrics.pairwise_sided_sums, pairwise_chamfer,
minimum_matching_distance, coverage, one_nn_accuracy, generation_metrics) on the torch path, and generation.sample_prior.

The sums are held to the shipped per-pair function: sided_distance on the pair, converted to double and summed by torch, within
2 N 2^-53 sum -- N - 1 double additions of non-negative terms on either side, each of relative error 2^-53 -- and exactly where the
sum is +inf.  The metrics are held to answers worked out by hand on small integer coordinates, where fp32 is exact."""
import pytest
import torch

from geniconet_amd import generation, metrics, models

INF, NAN = float('inf'), float('nan')


def _cloud(B, N, seed, scale=1.0):
    return torch.randn(B, N, 3, generator=torch.Generator().manual_seed(seed)) * scale


def per_pair_sums(p1, p2):
    """(G, R) float64 by the shipped per-pair route: sided_distance of cloud g against cloud r, summed in double by torch."""
    return torch.stack([torch.stack([metrics.sided_distance(p1[g:g + 1], p2[r:r + 1])[0].double().sum() for r in range(p2.shape[0])])
                        for g in range(p1.shape[0])])


def within_the_summation_bound(got, want, N):
    """+inf entries equal, the others within 2 N 2^-53 of the reference sum, and no NaN."""
    got, want = got.cpu(), want.cpu()
    assert got.dtype == torch.float64 and got.shape == want.shape and not torch.isnan(got).any()
    assert torch.equal(got == INF, want == INF)
    finite = want != INF
    assert ((got[finite] - want[finite]).abs() <= 2 * N * 2.0 ** -53 * want[finite]).all()
    return True


def points(*xyz):
    """Single-point clouds (len, 1, 3) from coordinate triples."""
    return torch.tensor(xyz, dtype=torch.float32)[:, None, :]


# ---- the torch path against the per-pair route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('G,R,N,M', ((3, 5, 40, 70), (1, 7, 33, 1), (7, 1, 1, 33), (2, 2, 64, 64)))
def test_torch_sums_equal_the_per_pair_route_within_the_summation_bound(G, R, N, M):
    p1, p2 = _cloud(G, N, 1 + N), _cloud(R, M, 2 + M)
    want = per_pair_sums(p1, p2)
    assert within_the_summation_bound(metrics.pairwise_sided_sums(p1, p2), want, N)
    # queries in slices of 7, one cloud of p2 at a time, targets in chunks: the same distances
    assert within_the_summation_bound(metrics._torch_pairwise_sided_sums(p1, p2, chunk=7), want, N)
    assert within_the_summation_bound(metrics._torch_pairwise_sided_sums(p1, p2, chunk=3 * N * M), want, N)
    assert within_the_summation_bound(metrics.pairwise_sided_sums(p1.double(), p2.double()), per_pair_sums(p1.double(), p2.double()), N)


def test_pairwise_chamfer_is_chamfer_distance_of_every_pair_rounded_once():
    p1, p2 = _cloud(3, 40, 5), _cloud(4, 25, 6)
    for kw in (dict(), dict(w1=0.25, w2=3.0), dict(squared=False), dict(w1=2.0, w2=0.5, squared=False)):
        got = metrics.pairwise_chamfer(p1, p2, **kw)
        want = torch.stack([torch.stack([metrics.chamfer_distance(p1[g:g + 1], p2[r:r + 1], **kw)[0] for r in range(4)]) for g in range(3)])
        assert got.dtype == torch.float32 and got.shape == (3, 4)
        assert ((got.double() - want.double()).abs() <= 2.0 ** -23 * want.double()).all(), kw    # equal, or neighbours
    same = metrics.pairwise_chamfer(p1, p1)
    assert (same.diagonal() == 0).all() and torch.equal(same, same.t()) and (same[~torch.eye(3, dtype=torch.bool)] > 0).all()
    assert not metrics.pairwise_chamfer(p1.requires_grad_(), p2).requires_grad


# ---- known answers on integers -------------------------------------------------------------------------------------------------------------
def test_single_point_clouds_give_twice_the_squared_distance():
    a = points((0, 0, 0), (1, 2, 3), (-4, 0, 7))
    b = points((1, 0, 0), (0, 0, 0), (5, 5, 5), (-4, 1, 7))
    want = 2 * ((a[:, None, 0] - b[None, :, 0]) ** 2).sum(-1)
    assert torch.equal(metrics.pairwise_chamfer(a, b), want)
    assert torch.equal(metrics.pairwise_sided_sums(a, b), want.double() / 2)
    assert torch.equal(metrics.pairwise_chamfer(a, b, w1=3.0, w2=0.0), 1.5 * want)


D_GR = torch.tensor([[1.0, 5.0, 9.0, 4.0],
                     [2.0, 3.0, 8.0, 7.0],
                     [6.0, 3.0, 2.0, 7.0]])
D_GG = torch.tensor([[0.0, 1.5, 10.0], [1.5, 0.0, 10.0], [10.0, 10.0, 0.0]])
D_RR = torch.tensor([[0.0, 6.0, 7.0, 0.5], [6.0, 0.0, 2.5, 9.0], [7.0, 2.5, 0.0, 9.0], [0.5, 9.0, 9.0, 0.0]])


def test_a_three_by_four_case_worked_by_hand():
    """MMD: the column minima are 1, 3, 2, 4, mean 2.5.  COV: the rows match references 0, 0, 2: two of four.  1-NNA, merged order
    g0 g1 g2 r0 r1 r2 r3: g0 -> r0 (1, wrong), g1 -> g0 (1.5, right), g2 -> r2 (2, wrong), r0 -> r3 (0.5, right), r1 -> r2 (2.5,
    right), r2 -> g2 (2, wrong), r3 -> r0 (0.5, right): four of seven."""
    assert metrics.minimum_matching_distance(D_GR).item() == 2.5
    assert metrics.coverage(D_GR).item() == 0.5
    assert metrics.one_nn_accuracy(D_GG, D_GR, D_RR).item() == 4 / 7
    assert metrics.minimum_matching_distance(D_GR.double()).dtype == torch.float64
    # the diagonal is excluded whatever it holds
    assert metrics.one_nn_accuracy(D_GG + torch.diag(torch.full((3,), -5.0)), D_GR, D_RR - torch.eye(4)).item() == 4 / 7


def _lattice_clouds(count, shift=0.0):
    """`count` distinct clouds of 8 integer points: the corners of a unit cube moved to (3 k + shift, k, 0)."""
    corners = torch.tensor([[x, y, z] for x in (0.0, 1.0) for y in (0.0, 1.0) for z in (0.0, 1.0)])
    return torch.stack([corners + torch.tensor([3.0 * k + shift, float(k), 0.0]) for k in range(count)])


def test_known_answers_of_the_three_figures_on_sets_of_clouds():
    gen = _lattice_clouds(5)
    copy = metrics.generation_metrics(gen, gen.clone())                      # every shape's nearest other element is its copy
    assert copy == dict(mmd=0.0, cov=1.0, one_nna=0.0)
    far = metrics.generation_metrics(gen, _lattice_clouds(4, shift=1000.0))  # two far-apart clusters: told apart perfectly
    assert far['one_nna'] == 1.0 and far['cov'] == 0.25 and far['mmd'] > 1e5
    identical = gen[:1].expand(6, -1, -1)                                    # all generated shapes identical: one reference is covered
    for R in (2, 3, 5):
        assert metrics.coverage(metrics.pairwise_chamfer(identical, _lattice_clouds(R, shift=1.0))).item() == 1 / R
    assert all(isinstance(v, float) for v in far.values()) and sorted(far) == ['cov', 'mmd', 'one_nna']


def test_ties_go_to_the_lowest_index():
    # two reference clouds equally far from every generated one, a third farther
    gen, ref = points((0, 0, 0), (0, 1, 0)), points((1, 0, 0), (-1, 0, 0), (5, 0, 0))
    d = metrics.pairwise_chamfer(gen, ref)
    assert torch.equal(d, torch.tensor([[2.0, 2.0, 50.0], [4.0, 4.0, 52.0]]))
    assert metrics.coverage(d).item() == 1 / 3                               # both match reference 0
    assert metrics.coverage(d.flip(1)).item() == 1 / 3                       # (50, 2, 2): both match reference 1
    assert metrics.coverage(torch.tensor([[1.0, 1.0, 5.0], [3.0, 2.0, 2.0]])).item() == 2 / 3      # references 0 and 1, not 0 and 2
    assert metrics.minimum_matching_distance(d).item() == (2 + 2 + 50) / 3
    # g0 is as far from g1 as from r0: the generated one comes first in the merged order.  g0 -> g1 right, g1 -> g0 right, r0 -> g0 wrong
    gen, ref = points((0, 0, 0), (1, 0, 0)), points((-1, 0, 0))
    assert metrics.generation_metrics(gen, ref)['one_nna'] == 2 / 3
    assert metrics.one_nn_accuracy(torch.tensor([[0.0, 2.0], [2.0, 0.0]]), torch.tensor([[2.0], [8.0]]), torch.zeros(1, 1)).item() == 2 / 3
    # r0 is as far from g0 as from r1: g0 wins, so r0 is wrong; r1 -> r0 right; g0 -> r0 wrong
    assert metrics.one_nn_accuracy(torch.zeros(1, 1), torch.tensor([[3.0, 9.0]]), torch.tensor([[0.0, 3.0], [3.0, 0.0]])).item() == 1 / 3


# ---- non-finite input --------------------------------------------------------------------------------------------------------------------
def nonfinite_case():
    """(p1 (3, 6, 3), p2 (4, 5, 3), the expected sums) on small integers: target 2 of cloud 1 of p2 has a NaN coordinate, cloud 3 of p2
    is all NaN, query 4 of cloud 2 of p1 is NaN."""
    g = torch.Generator().manual_seed(11)
    p1, p2 = torch.randint(-4, 5, (3, 6, 3), generator=g).float(), torch.randint(-4, 5, (4, 5, 3), generator=g).float()
    clean = p2.clone()
    p2[1, 2, 1] = NAN
    p2[3] = NAN
    p1[2, 4, 0] = NAN
    want = torch.empty(3, 4, dtype=torch.float64)
    for g_ in range(3):
        for r in range(4):
            targets = clean[r] if r != 1 else clean[1][[0, 1, 3, 4]]          # the NaN target is dropped, that target only
            d = ((p1[g_][:, None] - targets[None]) ** 2).sum(-1).amin(-1).double()
            want[g_, r] = INF if (r == 3 or g_ == 2) else d.sum()
    return p1, p2, want


def test_non_finite_input_answers_as_defined_and_no_nan_comes_out():
    p1, p2, want = nonfinite_case()
    got = metrics.pairwise_sided_sums(p1, p2)
    assert torch.equal(got, want) and (got[:2, :3] < INF).all()
    back = metrics.pairwise_sided_sums(p2, p1)                               # a NaN query has no acceptable target: its cloud's row is +inf
    assert (back[1] == INF).all() and (back[3] == INF).all() and (back[[0, 2]][:, :2] < INF).all() and not torch.isnan(back).any()
    d = metrics.pairwise_chamfer(p1[:2], p2)
    assert (d[:, 3] == INF).all() and (d[:, 1] == INF).all() and (d[:, [0, 2]] < INF).all()
    match = metrics._lowest_argmin(d)[1]
    assert ((match == 0) | (match == 2)).all()                               # an infinite column is never the minimum
    figures = metrics.generation_metrics(p1, p2)
    assert figures['mmd'] == INF and 0 <= figures['cov'] <= 0.5 and 0 <= figures['one_nna'] <= 1
    assert not any(v != v for v in figures.values())
    nothing = torch.full((2, 3), INF)
    nothing[0, 1] = NAN
    assert metrics.coverage(nothing).item() == 0 and metrics.minimum_matching_distance(nothing).item() == INF
    assert metrics.one_nn_accuracy(torch.full((2, 2), NAN), nothing, torch.full((3, 3), INF)).item() == 0      # no finite neighbour: wrong


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise():
    good = _cloud(2, 5, 1)
    for call in (metrics.pairwise_sided_sums, metrics.pairwise_chamfer, metrics.generation_metrics):
        for bad in (good[0], good[..., :2], good[:, :0], good[:0], good.long(), good[None], 'clouds',
                    good[:1].expand(65536, -1, -1)):                         # the shape check alone: nothing is materialised
            with pytest.raises(ValueError):
                call(bad, good)
            with pytest.raises(ValueError):
                call(good, bad)
        call(good, _cloud(3, 9, 2))                                          # the set sizes and the point counts are independent
    metrics._check_cloud_sets('pairwise_sided_sums', good[:1].expand(65535, -1, -1), good)         # the largest set is accepted
    for bad in (D_GR[0], D_GR[None], D_GR[:0], D_GR.long(), 'matrix'):
        for call in (metrics.minimum_matching_distance, metrics.coverage):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError):
            metrics.one_nn_accuracy(D_GG, bad, D_RR)
    for d_gg, d_rr in ((D_RR, D_RR), (D_GG, D_GG), (D_GG[:2], D_RR), (D_GG, D_RR[:, :3])):
        with pytest.raises(ValueError):
            metrics.one_nn_accuracy(d_gg, D_GR, d_rr)


# ---- generation.sample_prior ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def vae():
    return models.ico2ico_vae(models.default_params('ico2ico_vae', subdivisions=3))


def test_sample_prior_is_reproducible_and_follows_create_sample(vae):
    shape = (models.VAE_LATENT_CHANNELS, 5, 2)                               # level 0: a stride-2 convolution at level 1
    assert generation.latent_shape(vae) == shape
    z = generation.sample_prior(vae, 6, seed=3)
    assert z.shape == (6,) + shape and z.dtype == torch.float32
    assert torch.equal(z, generation.sample_prior(vae, 6, seed=3)) and not torch.equal(z, generation.sample_prior(vae, 6, seed=4))
    assert torch.equal(z, torch.randn((6,) + shape, generator=torch.Generator().manual_seed(3)))
    assert abs(z.mean().item()) < 0.05 and abs(z.std().item() - 1) < 0.05
    misc = [dict(trn_mean=torch.randn((6,) + shape, generator=torch.Generator().manual_seed(8)),
                 trn_logvar=torch.randn((6,) + shape, generator=torch.Generator().manual_seed(9)))]
    eps = torch.randn((6,) + shape, generator=torch.Generator().manual_seed(5))
    want = torch.add(misc[0]['trn_mean'], misc[0]['trn_logvar'] * eps)        # models.enc2ico_vae.createSample
    assert torch.equal(generation.sample_prior(vae, 6, seed=5, misc=misc), want)
    assert torch.equal(generation.sample_prior(vae, 6, seed=5, misc=misc[0]), want)
    more = generation.sample_prior(vae, 8, seed=5, misc=misc)                 # the batch's rows are cycled
    eps8 = torch.randn((8,) + shape, generator=torch.Generator().manual_seed(5))
    assert torch.equal(more[6:], misc[0]['trn_mean'][:2] + misc[0]['trn_logvar'][:2] * eps8[6:])
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError):
            generation.sample_prior(vae, bad)
    with pytest.raises(ValueError):
        generation.sample_prior(vae, 2, misc=dict(trn_mean=torch.zeros(2, 4, 5, 2), trn_logvar=torch.zeros(2, 4, 5, 2)))
    with pytest.raises(ValueError):
        generation.generate_vertices(vae, torch.zeros(2, 4, 5, 2))
