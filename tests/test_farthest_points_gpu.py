"""icn_farthest_points on the device (sampling.farthest_point_sample, farthest_points; the `points=` option of the set metrics).

The kernel is held to the restatement sampling._torch_farthest_point_sample on CPU tensors BIT FOR BIT, in idx and in cover: fminf, the
max and the lowest-index argmax are order-free, so nothing may differ however the kernel splits the scan.  Every call is one
k_farthest_points launch.  The point counts sit around a wave and around every edge between two instantiations of the kernel (512
threads times the points a thread holds, read from the source), where a thread's last slot changes from a point to padding."""
import functools
import os
import re

import pytest
import torch

from geniconet_amd import _lib, data, generation, losses, metrics, models, sampling

from test_abi import ROOT
from test_farthest_points import (INF, NAN, _bits, coincident_cloud, duplicate_cloud, lattice_cloud, nonfinite_batch, overflow_cloud,
                                  sphere_clouds)
from test_signed_distance import _profiled


def source_constants():
    """(threads of a workgroup, the points a thread may hold) as csrc/icn_fps.hip states them."""
    src = open(os.path.join(ROOT, 'geniconet_amd', 'csrc', 'icn_fps.hip')).read()
    block = int(re.search(r'constexpr int FPS_BLOCK = (\d+);', src).group(1))
    buckets = [int(x) for x in re.search(r'for \(int ppt : \{([\d, ]+)\}\)', src).group(1).split(',')]
    assert sorted(int(x) for x in re.findall(r'case (\d+): launch_bucket<\1>', src)) == buckets      # every bucket is instantiated
    assert block * buckets[-1] == int(re.search(r'constexpr int FPS_MAX_N = (\d+);', src).group(1)) == sampling._FPS_MAX_N
    return block, buckets


BLOCK, BUCKETS = source_constants()
EDGES = [BLOCK * ppt for ppt in BUCKETS]
COUNTS = sorted({1, 2, 63, 64, 65, 8193} | {e + k for e in EDGES for k in (-1, 0, 1) if e + k <= EDGES[-1]})


def test_the_point_counts_cover_every_edge_of_the_kernel_as_built():
    assert BLOCK == 512 and EDGES[0] == 512 and EDGES[-1] == 13312 and {511, 512, 513, 8193, 13311, 13312} <= set(COUNTS)
    assert all({e - 1, e} <= set(COUNTS) for e in EDGES)


def steps(N):
    return 16 if N >= 4097 else min(N, 64)


@functools.lru_cache(maxsize=None)
def restated(N, S, start, B=1):
    """The restatement on the CPU, computed once per shape and shared."""
    return sampling._torch_farthest_point_sample(sphere_clouds(B, N), S, start)


def one_launch(points, count, start=0):
    (idx, cover), kernels = _profiled(lambda: sampling.farthest_point_sample(points, count, start))
    assert kernels == {'k_farthest_points': 1}, kernels
    assert idx.is_cuda and cover.is_cuda and idx.dtype == torch.int64 and cover.dtype == torch.float32
    return idx.cpu(), cover.cpu()


def same_bits(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(_bits(got[1]), _bits(want[1]))


@pytest.mark.gpu
@pytest.mark.parametrize('N', COUNTS)
def test_the_kernel_equals_the_restatement_bit_for_bit_around_a_wave_and_every_bucket_edge(N):
    S, start = steps(N), (N - 1 if N % 2 else N // 3)                        # a nonzero start wherever there is one
    got = one_launch(sphere_clouds(1, N).cuda(), S, start)
    assert same_bits(got, restated(N, S, start))
    assert got[0][0, 0] == start and (got[0] < N).all()


@pytest.mark.gpu
def test_every_point_of_a_cloud_is_a_permutation():
    got = one_launch(sphere_clouds(2, 642).cuda(), 642)
    assert same_bits(got, restated(642, 642, 0, B=2))
    assert torch.equal(got[0].sort(1).values, torch.arange(642).expand(2, -1)) and (got[1][:, -1] == 0).all()


@pytest.mark.gpu
def test_ties_resolve_to_the_lowest_index():
    got = one_launch(lattice_cloud().cuda(), 64)
    assert same_bits(got, sampling._torch_farthest_point_sample(lattice_cloud(), 64))
    assert got[0][0, :8].tolist() == [0, 63, 7, 28, 49, 14, 35, 56] and got[1][0, :8].tolist() == [27.0, 10.0, 10.0, 10.0, 5.0, 5.0, 5.0, 3.0]


@pytest.mark.gpu
def test_the_defined_cases():
    dup = one_launch(duplicate_cloud().cuda(), 15)
    assert same_bits(dup, sampling._torch_farthest_point_sample(duplicate_cloud(), 15))
    assert sorted(dup[0][0, :5].tolist()) == [0, 1, 2, 3, 4] and (dup[0][0, 5:] == 0).all() and (_bits(dup[1][0, 4:]) == 0).all()
    same = one_launch(coincident_cloud().cuda(), 6, start=3)
    assert same[0].tolist() == [[3, 0, 0, 0, 0, 0]] and (_bits(same[1]) == 0).all()
    over = one_launch(overflow_cloud().cuda(), 64)
    assert same_bits(over, sampling._torch_farthest_point_sample(overflow_cloud(), 64))
    assert not torch.isnan(over[1]).any() and (over[1][0, :-1] == INF).all() and over[1][0, -1] == 0
    for value in (NAN, INF, -INF):
        p = nonfinite_batch(value)
        got = one_launch(p.cuda(), 20, start=2)
        assert (got[0][1] == -1).all() and torch.isnan(got[1][1]).all()
        want = sampling._torch_farthest_point_sample(p, 20, 2)
        assert torch.equal(got[0], want[0]) and torch.equal(_bits(got[1][[0, 2]]), _bits(want[1][[0, 2]]))
    sub = sampling.farthest_points(nonfinite_batch(NAN).cuda(), 20)
    assert torch.isnan(sub[1]).all() and torch.isfinite(sub[[0, 2]]).all()


@pytest.mark.gpu
def test_rows_of_a_batch_are_independent_and_slicing_changes_no_bit(monkeypatch):
    p = torch.cat([sphere_clouds(4, 700), nonfinite_batch(NAN, 700)[1:2]])[[0, 1, 4, 2, 3]].cuda()     # five clouds, the third not finite
    whole = one_launch(p, 64, start=5)
    for b in range(5):
        one = one_launch(p[b:b + 1], 64, start=5)
        assert torch.equal(one[0], whole[0][b:b + 1]) and torch.equal(_bits(one[1]), _bits(whole[1][b:b + 1])), b
    assert (whole[0][2] == -1).all() and (whole[0][[0, 1, 3, 4]] >= 0).all()
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 2)
    (idx, cover), kernels = _profiled(lambda: sampling.farthest_point_sample(p, 64, start=5))
    assert kernels == {'k_farthest_points': 3}
    assert torch.equal(idx.cpu(), whole[0]) and torch.equal(_bits(cover), _bits(whole[1]))


@pytest.mark.gpu
def test_a_null_cover_leaves_idx_unchanged():
    p = sphere_clouds(3, 1025).cuda().contiguous()
    with_cover = torch.full((3, 40), -7, dtype=torch.int32, device='cuda')
    without = torch.full((3, 40), -7, dtype=torch.int32, device='cuda')
    cover = torch.empty(3, 40, dtype=torch.float32, device='cuda')
    L = _lib.api()
    L.icn_farthest_points(p.data_ptr(), 3, 1025, 40, 7, with_cover.data_ptr(), cover.data_ptr(), _lib.stream())
    L.icn_farthest_points(p.data_ptr(), 3, 1025, 40, 7, without.data_ptr(), None, _lib.stream())
    torch.cuda.synchronize()
    assert torch.equal(with_cover, without) and (without[:, 0] == 7).all()
    assert torch.equal(without.long().cpu(), sampling._torch_farthest_point_sample(sphere_clouds(3, 1025), 40, 7)[0])


@pytest.mark.gpu
def test_the_last_cover_is_what_the_nearest_neighbour_kernel_answers_on_the_device():
    p = sphere_clouds(2, 2562).cuda()
    idx, cover = sampling.farthest_point_sample(p, 256)
    subset = sampling.farthest_points(p, 256)
    assert torch.equal(subset, torch.gather(p, 1, idx[..., None].expand(-1, -1, 3)))
    (dist, _), kernels = _profiled(lambda: metrics.sided_distance(p, subset))
    assert kernels == {'k_nn_points': 1}
    assert torch.equal(_bits(cover[:, -1]), _bits(dist.amax(-1)))
    assert (cover[:, 1:] <= cover[:, :-1]).all()


@pytest.mark.gpu
def test_other_dtypes_larger_clouds_and_the_switch_take_the_restatement(monkeypatch):
    p = sphere_clouds(1, 65).cuda()
    # float64; a cloud above the bound of the HIP path; the switch ICN_NO_HIP_LOSS=1
    for points, patch in ((p.double(), None), (p, (sampling, '_FPS_MAX_N', 64)), (p, (losses, '_NO_HIP_LOSS', True))):
        with monkeypatch.context() as m:
            if patch:
                m.setattr(*patch)
            (idx, cover), kernels = _profiled(lambda: sampling.farthest_point_sample(points, 8))
        assert kernels == {} and idx.is_cuda and cover.dtype == points.dtype
        assert torch.equal(idx.cpu(), sampling._torch_farthest_point_sample(points.cpu(), 8)[0])
    assert _profiled(lambda: sampling.farthest_point_sample(p, 8))[1] == {'k_farthest_points': 1}


@pytest.mark.gpu
def test_generation_metrics_emd_on_subsets_is_generation_metrics_of_the_subsets():
    g, r = sphere_clouds(3, 642, seed=1, anisotropic=True).cuda(), sphere_clouds(3, 642, seed=2).cuda()
    figures, kernels = _profiled(lambda: metrics.generation_metrics(g, r, distance='emd', points=64))
    assert kernels == {'k_farthest_points': 2, 'k_match_auction': 3}
    assert figures == metrics.generation_metrics(sampling.farthest_points(g, 64), sampling.farthest_points(r, 64), distance='emd')
    assert figures != metrics.generation_metrics(g, r, distance='emd')
    cpu = metrics.generation_metrics(g.cpu(), r.cpu(), points=64)            # the subsets are those of the CPU, so are the chamfer figures:
    got = metrics.generation_metrics(g, r, points=64)                        # an entry is one fp32 rounding of sums in double
    assert got['cov'] == cpu['cov'] and got['one_nna'] == cpu['one_nna'] and abs(got['mmd'] - cpu['mmd']) <= 2.0 ** -23 * cpu['mmd']


@pytest.mark.gpu
def test_evaluate_generation_on_subsets_of_an_untrained_vae():
    torch.manual_seed(0)
    model = models.ico2ico_vae(models.default_params('ico2ico_vae', subdivisions=3)).cuda()
    x, _ = data.synthetic_batch(4, 3, seed=5, device='cuda')
    reference = metrics.output2vertices(3, x)
    vertices = generation.generate_vertices(model, generation.sample_prior(model, 4, seed=2))
    want = metrics.generation_metrics(sampling.farthest_points(vertices, 100), sampling.farthest_points(reference, 100))
    assert generation.evaluate_generation(model, reference, 4, seed=2, points=100) == want
    assert generation.evaluate_generation(model, reference, 4, seed=2, points=0) == generation.evaluate_generation(model, reference, 4, seed=2)
    assert generation.evaluate_generation(model, reference, 4, seed=2, samples=300, points=100) != want
    with pytest.raises(ValueError, match='points=643 is more than the 642 points of a cloud'):
        generation.evaluate_generation(model, reference, 4, seed=2, points=643)
