"""Farthest point sampling by its definition in torch (sampling._torch_farthest_point_sample, include/icn_fps.h), on CPU tensors: a case
checked by hand, the consequences of the definition that are EXACT in the dtype, the cases it defines (duplicates, coincident points,
non-finite and overflowing coordinates), float64 input, the gradient of farthest_points, and the `points=` option of
metrics.generation_metrics, metrics.evaluate_distance and generation.evaluate_generation.  tests/test_farthest_points_gpu.py holds the
kernel to this restatement bit for bit."""
import functools

import pytest
import torch

from geniconet_amd import generation, geometry, metrics, sampling

INF, NAN = float('inf'), float('nan')
SCALE = torch.tensor([1.0, 0.25, 3.0])


def _bits(x):
    x = x.detach().cpu().contiguous()
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int64)


@functools.lru_cache(maxsize=None)
def sphere_clouds(B, N, seed=0, anisotropic=False):
    """B clouds of N points on the unit sphere (randn normalised), seeded by their sizes; anisotropic: every axis scaled on its own."""
    p = torch.nn.functional.normalize(torch.randn(B, N, 3, generator=torch.Generator().manual_seed(7919 * N + 31 * B + seed)), dim=-1)
    return p * SCALE if anisotropic else p


def lattice_cloud():
    """The 4 x 4 x 4 integer lattice, point 16 x + 4 y + z at (x, y, z): every distance an integer, ties everywhere."""
    g = torch.arange(4.0)
    return torch.stack(torch.meshgrid(g, g, g, indexing='ij'), -1).reshape(1, 64, 3)


def duplicate_cloud():
    """Three copies of five distinct points: 15 points, five distinct."""
    return sphere_clouds(1, 5).repeat(1, 3, 1)


def coincident_cloud(N=9):
    return torch.full((1, N, 3), 0.375)


def overflow_cloud(N=64):
    """Unit vectors scaled by 3e38: the squared distance of almost every pair overflows fp32."""
    return sphere_clouds(1, N) * 3e38


def nonfinite_batch(value, N=65):
    """Three clouds, the middle one with one coordinate replaced by `value`."""
    p = sphere_clouds(3, N).clone()
    p[1, N // 2, 1] = value
    return p


def pairwise_d(q):
    """(B, S, S): the d of the definition between the points of q (B, S, 3), every product and sum an operation of its own."""
    dx, dy, dz = (q[:, :, None, :] - q[:, None, :, :]).unbind(-1)
    return (dx * dx + dy * dy) + dz * dz


def check_exact_consequences(p, idx, cover):
    """What the definition implies exactly, for clouds of distinct points: every assertion is an equality of bits."""
    (B, N, _), S = p.shape, idx.shape[1]
    assert idx.dtype == torch.int64 and cover.dtype == p.dtype and idx.shape == cover.shape == (B, S)
    assert (idx >= 0).all() and (idx < N).all() and (cover[:, 1:] <= cover[:, :-1]).all() and (cover >= 0).all()
    subset = torch.gather(p, 1, idx[..., None].expand(-1, -1, 3))
    assert torch.equal(_bits(cover[:, -1]), _bits(metrics.sided_distance(p, subset)[0].amax(-1)))
    if S >= 2:
        d = pairwise_d(subset) + torch.diag(torch.full((S,), INF, dtype=p.dtype))
        assert torch.equal(_bits(cover[:, -2]), _bits(d.amin((1, 2))))
    if S == N:
        assert torch.equal(idx.sort(1).values, torch.arange(N).expand(B, -1)) and (cover[:, -1] == 0).all()


def test_the_lattice_by_hand():
    """start = 0 = (0,0,0).  Step 0: the farthest point is the opposite corner 63 = (3,3,3), d = 27.  Step 1: dist = min(d to (0,0,0),
    d to (3,3,3)); the six other corners have min(9, 18) = 9 or min(18, 9) = 9, but (0,1,3) has min(10, 13) = 10 and nothing has more
    (10 = 0 + 1 + 9 needs coordinates {0, 1, 3} or, from the far corner, {3, 2, 0}: twelve points): the lowest is 7 = (0,1,3), cover 10.
    Step 2: of those twelve, the ones still at 10 after (0,1,3) -- 28 = (1,3,0) is at 1 + 4 + 9 = 14 from it -- the lowest is 28, cover
    10.  Step 3: 49 = (3,0,1) is at 10 from (0,0,0), 13 from (3,3,3), 9 + 1 + 4 = 14 from 7 and 4 + 9 + 1 = 14 from 28: still 10, and
    no lower index is (11 = (0,2,3) is at 1 from 7, 13 = (0,3,1) at 5 from 28, 19 = (1,0,3) at 2 from 7, ...).  Then nothing is farther
    than 5 from the five chosen: 14 = (0,3,2), 35 = (2,0,3), 56 = (3,2,0) in turn at cover 5, 5, 5, and the eighth step leaves 3."""
    idx, cover = sampling.farthest_point_sample(lattice_cloud(), 8)
    assert idx.tolist() == [[0, 63, 7, 28, 49, 14, 35, 56]]
    assert cover.tolist() == [[27.0, 10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 3.0]]
    p = lattice_cloud()[0]
    chosen = p[[0, 63, 7, 28, 49]]
    assert ((p[:, None] - chosen[None]) ** 2).sum(-1).amin(1).max() == 5                   # the claim of the fifth step, by brute force


@pytest.mark.parametrize('anisotropic', [False, True])
@pytest.mark.parametrize('N', [1, 2, 65, 642])
def test_exact_consequences_on_sphere_clouds(N, anisotropic):
    p = sphere_clouds(2, N, anisotropic=anisotropic)
    idx, cover = sampling.farthest_point_sample(p, N)
    check_exact_consequences(p, idx, cover)
    part = N // 3 + 1
    idx_part, cover_part = sampling.farthest_point_sample(p, part)
    assert torch.equal(idx_part, idx[:, :part]) and torch.equal(_bits(cover_part), _bits(cover[:, :part]))   # the loop is a prefix of itself
    check_exact_consequences(p, idx_part, cover_part)
    if N > 2:
        other, _ = sampling.farthest_point_sample(p, part, start=N - 1)
        assert (other[:, 0] == N - 1).all() and not torch.equal(other, idx_part)
        check_exact_consequences(p, *sampling.farthest_point_sample(p, part, start=N - 1))


def test_duplicates_are_defined():
    idx, cover = sampling.farthest_point_sample(duplicate_cloud(), 15)
    assert sorted(idx[0, :5].tolist()) == [0, 1, 2, 3, 4] and (cover[0, :4] > 0).all()      # the lowest index of every distinct point
    assert (cover[0, 4:] == 0).all() and (idx[0, 5:] == 0).all()
    assert not torch.signbit(cover).any()


def test_all_points_coincident():
    idx, cover = sampling.farthest_point_sample(coincident_cloud(), 6, start=3)
    assert idx.tolist() == [[3, 0, 0, 0, 0, 0]] and (cover == 0).all() and not torch.signbit(cover).any()


@pytest.mark.parametrize('value', [NAN, INF, -INF])
def test_a_non_finite_cloud_answers_minus_one_and_nan_and_leaves_the_others_alone(value):
    p = nonfinite_batch(value)
    idx, cover = sampling.farthest_point_sample(p, 20, start=2)
    assert (idx[1] == -1).all() and torch.isnan(cover[1]).all()
    for b in (0, 2):
        one_idx, one_cover = sampling.farthest_point_sample(p[b:b + 1], 20, start=2)
        assert torch.equal(idx[b:b + 1], one_idx) and torch.equal(_bits(cover[b:b + 1]), _bits(one_cover))
    sub = sampling.farthest_points(p, 20, start=2)
    assert torch.isnan(sub[1]).all() and torch.isfinite(sub[[0, 2]]).all()


def test_overflowing_distances_give_inf_and_never_nan():
    p = overflow_cloud()
    idx, cover = sampling.farthest_point_sample(p, 64)
    assert not torch.isnan(cover).any() and (cover[0, :-1] == INF).all() and cover[0, -1] == 0
    assert sorted(idx[0].tolist()) == list(range(64))


@pytest.mark.parametrize('N, S', [(65, 65), (642, 642), (2562, 256)])
def test_float64_input_runs_the_same_lines_in_double_and_picks_the_same_points(N, S):
    p = sphere_clouds(2, N)
    idx32, cover32 = sampling.farthest_point_sample(p, S)
    idx64, cover64 = sampling.farthest_point_sample(p.double(), S)
    assert cover64.dtype == torch.float64 and torch.equal(idx32, idx64)
    assert ((cover32.double() - cover64).abs() <= 6 * 2.0 ** -24 * cover64).all()          # the bound of sided_distance's docstring
    check_exact_consequences(p.double(), idx64, cover64)


def test_farthest_points_is_a_gather_with_the_gradient_of_a_gather():
    p = sphere_clouds(2, 65).clone().requires_grad_(True)
    idx, _ = sampling.farthest_point_sample(p, 10)
    assert not idx.requires_grad
    sub = sampling.farthest_points(p, 10)
    plain = torch.gather(p, 1, idx[..., None].expand(-1, -1, 3))
    assert torch.equal(sub, plain) and sub.requires_grad
    w = torch.randn(2, 10, 3, generator=torch.Generator().manual_seed(3))
    g, = torch.autograd.grad((sub * w).sum(), p)
    g_plain, = torch.autograd.grad((plain * w).sum(), p)
    assert torch.equal(g, g_plain) and (g != 0).any(-1).sum() == 20


@pytest.mark.parametrize('distance', metrics.GENERATION_DISTANCES)
def test_generation_metrics_on_subsets_is_generation_metrics_of_the_subsets(distance):
    g, r = sphere_clouds(3, 40, seed=1, anisotropic=True), sphere_clouds(3, 40, seed=2)
    want = metrics.generation_metrics(sampling.farthest_points(g, 12), sampling.farthest_points(r, 12), distance)
    assert metrics.generation_metrics(g, r, distance, points=12) == want
    assert metrics.generation_metrics(g.clone().requires_grad_(True), r, distance, points=12) == want       # under no_grad
    assert metrics.generation_metrics(g, r, distance, points=0) == metrics.generation_metrics(g, r, distance)
    assert metrics.generation_metrics(g, r, distance) != want


@pytest.mark.parametrize('mode', ['chamfer', 'f_0.3', 'hausdorff', 'emd'])
def test_evaluate_distance_on_subsets_is_evaluate_distance_of_the_subsets(mode):
    faces = torch.from_numpy(geometry.get_ico_faces(1)).long()
    V = int(faces.max()) + 1
    out, ref = sphere_clouds(1, V, seed=3)[0], sphere_clouds(1, V, seed=4, anisotropic=True)[0]
    sub = lambda x: sampling.farthest_points(x[None], 10)[0]                 # noqa: E731
    assert metrics.evaluate_distance(out, ref, faces, mode, points=10) == metrics.evaluate_distance(sub(out), sub(ref), faces, mode)
    assert metrics.evaluate_distance(out, ref, faces, mode, points=0) == metrics.evaluate_distance(out, ref, faces, mode)
    # after the surface sampling: S samples thinned to P
    u = torch.rand((2, 1, 50, 3), generator=torch.Generator().manual_seed(5))
    s_out, s_ref = (sampling.sample_points(x[None], faces, uniforms=u[k])[0][0] for k, x in enumerate((out, ref)))
    assert (metrics.evaluate_distance(out, ref, faces, mode, samples=50, seed=5, points=10)
            == metrics.evaluate_distance(sub(s_out), sub(s_ref), faces, mode))
    assert (metrics.evaluate_distance(out, ref, faces, mode, samples=50, seed=5, points=0)
            == metrics.evaluate_distance(out, ref, faces, mode, samples=50, seed=5))


def test_points_is_not_read_by_the_modes_that_pair_vertices_or_search_the_mesh():
    faces = torch.from_numpy(geometry.get_ico_faces(1)).long()
    V = int(faces.max()) + 1
    out, ref = sphere_clouds(1, V, seed=3)[0], sphere_clouds(1, V, seed=4)[0]
    for mode in ('point2point', 'point2mesh'):
        assert metrics.evaluate_distance(out, ref, faces, mode, points=5) == metrics.evaluate_distance(out, ref, faces, mode)


def test_argument_errors():
    p = sphere_clouds(2, 65)
    for fn in (sampling.farthest_point_sample, sampling.farthest_points):
        for bad in (dict(count=0), dict(count=66), dict(count=-1), dict(count=2.0), dict(count=True), dict(count=None),
                    dict(count=5, start=-1), dict(count=5, start=65), dict(count=5, start=1.0), dict(count=5, start=False)):
            with pytest.raises(ValueError, match=fn.__name__ + ': (count|start) must be an integer'):
                fn(p, **bad)
        for points in (p[0], p[..., :2], p.long(), p[:0], p[:, :0], [[0.0, 0.0, 0.0]]):
            with pytest.raises(ValueError, match='expected the point set'):
                fn(points, 1)
    for points in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match='generation_metrics: points must be a non-negative integer'):
            metrics.generation_metrics(p, p, points=points)
        with pytest.raises(ValueError, match='evaluate_distance: points must be a non-negative integer'):
            metrics.evaluate_distance(p[0], p[1], None, 'chamfer', points=points)
        with pytest.raises(ValueError, match='evaluate_generation: points must be a non-negative integer'):
            generation.evaluate_generation(None, p, 2, points=points)
    with pytest.raises(ValueError, match='generation_metrics: points=66 is more than the 65 points of a cloud'):
        metrics.generation_metrics(p, p, points=66)
    with pytest.raises(ValueError, match='generation_metrics: points=66 is more than the 65 points of a cloud'):
        metrics.generation_metrics(sphere_clouds(2, 70), p, points=66)       # the smaller of the two sets decides
    with pytest.raises(ValueError, match='evaluate_distance: points=66 is more than the 65 points of a cloud'):
        metrics.evaluate_distance(p[0], p[1], None, 'hausdorff', points=66)
