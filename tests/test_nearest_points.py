"""Nearest neighbours between point sets and what is built on them (metrics.sided_distance, chamfer_distance, f_score,
hausdorff_distance, evaluate_distance; icn_nearest_points, icn_nearest_points_bwd).

The definition (metrics.sided_distance, include/icn_nn.h) is written a third time here, as plain Python loops over numpy float32
scalars (`reference`); the torch formulation must equal it bit for bit, values and indices, on ties and on non-finite input too, and
lie within 6 2^-24 of float64.  On the GPU the kernel must equal the fp32 torch formulation bit for bit over point counts chosen at
the edges of its tiles (256 staged targets, 256 threads of 2 queries: 512 queries a workgroup) and over input families, the
backward's dpoints must equal the fp32 formulation bit for bit and its dtargets must lie within a bound derived from its roundings
of float64 autograd at the device's choice, element by element."""
import functools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import metrics

from error_bounds import U, rho
from test_signed_distance import _profiled
from test_voxelize import _sphere

INF = float('inf')
NAN = float('nan')
BOUND = 6 * U                                                                 # five roundings of relative size u: (1 + u)^5 - 1 < 6 u


# ---- the reference: the definition in plain loops -----------------------------------------------------------------------------------
def reference(points, targets):
    """(dist float32 (B, N), idx int64 (B, N)) by the lines of the definition on numpy float32 scalars, one rounding an operation."""
    p, t = points.numpy().astype(np.float32), targets.numpy().astype(np.float32)
    (B, N, _), M = p.shape, t.shape[1]
    dist, idx = np.empty((B, N), np.float32), np.empty((B, N), np.int64)
    with np.errstate(all='ignore'):
        for b in range(B):
            for i in range(N):
                best, at = np.float32(INF), -1
                for j in range(M):
                    dx, dy, dz = p[b, i, 0] - t[b, j, 0], p[b, i, 1] - t[b, j, 1], p[b, i, 2] - t[b, j, 2]
                    d = (dx * dx + dy * dy) + dz * dz
                    assert d.dtype == np.float32
                    if d < best:
                        best, at = d, j
                dist[b, i], idx[b, i] = best, at
    return torch.from_numpy(dist), torch.from_numpy(idx)


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def _same(got, want, what=''):
    """dist by bit pattern, idx exactly."""
    assert got[1].dtype == torch.int64 and got[0].dtype == want[0].dtype, what
    assert torch.equal(got[1].cpu(), want[1].long()), what
    assert torch.equal(_bits(got[0]), _bits(want[0])), what
    assert not torch.isnan(got[0]).any(), what


def _cloud(B, N, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, N, 3, generator=g) * scale + shift


def _lattice(n):
    """The n^3 points of the integer lattice [0, n)^3, fp32 (n^3, 3), the last coordinate fastest."""
    a = torch.arange(n, dtype=torch.float32)
    return torch.stack(torch.meshgrid(a, a, a, indexing='ij'), -1).reshape(-1, 3)


def _cell_centres(n):
    return _lattice(n - 1) + 0.5


# ---- CPU: the formulation against the loops, against float64, on ties and on non-finite input ----------------------------------------
@pytest.mark.parametrize('M', (1, 7, 64))
@pytest.mark.parametrize('N', (1, 7, 64))
def test_torch_formulation_equals_the_definition_in_plain_loops(N, M):
    p, t = _cloud(2, N, 10 * N + M), _cloud(2, M, 1000 + 10 * N + M)
    want = reference(p, t)
    _same(metrics._torch_sided_distance(p, t), want)
    _same(metrics.sided_distance(p, t), want)
    _same(metrics._torch_sided_distance_fwd(p, t, chunk=2 * N * 3), want, 'chunks of three targets')


@pytest.mark.parametrize('scale,shift', ((2.0 ** -20, 0.0), (1.0, 0.0), (2.0 ** 20, 0.0), (1.0, 100.0)))
def test_fp32_distances_lie_within_six_roundings_of_float64(scale, shift):
    """|d32 - d64| <= 6 u d64 for EVERY pair (the distance of the chosen index among them), and the float64 distance to the chosen
    index is within the same bound of the float64 minimum; indices are not compared outright: near-ties may go either way."""
    p, t = _cloud(2, 300, 1, scale, shift * scale), _cloud(2, 400, 2, scale, shift * scale)
    dist, idx = metrics.sided_distance(p, t)
    diff = p[:, :, None].double() - t[:, None].double()
    d64 = (diff * diff).sum(-1)                                                           # (B, N, M)
    diff32 = p[:, :, None] - t[:, None]
    d32 = (diff32[..., 0] * diff32[..., 0] + diff32[..., 1] * diff32[..., 1]) + diff32[..., 2] * diff32[..., 2]
    every = ((d32.double() - d64).abs() / d64).max().item() / U
    chosen64 = torch.gather(d64, 2, idx[..., None])[..., 0]
    assert torch.equal(_bits(torch.gather(d32, 2, idx[..., None])[..., 0]), _bits(dist))
    value = ((dist.double() - chosen64).abs() / chosen64).max().item() / U
    choice = ((chosen64 - d64.amin(-1)) / d64.amin(-1)).max().item() / U
    print('scale %g shift %g: worst |d32 - d64| / (u d64) over %d pairs %.3f, of the answers %.3f; chosen against the float64 minimum %.3f u'
          % (scale, shift, d64.numel(), every, value, choice))
    assert every <= 6 and value <= 6 and choice <= 6


def test_ties_go_to_the_lowest_index_also_after_permuting_the_targets():
    """The centre of a cell of the 6^3 integer lattice is at squared distance 3/4 from its 8 corners, exactly."""
    lattice, centres = _lattice(6), _cell_centres(6)
    g = torch.Generator().manual_seed(5)
    targets = torch.stack([lattice, lattice[torch.randperm(216, generator=g)], lattice[torch.randperm(216, generator=g)]])
    points = centres[None].expand(3, -1, -1).contiguous()
    dist, idx = metrics.sided_distance(points, targets)
    assert (dist == 0.75).all()
    d = ((points[:, :, None] - targets[:, None]) ** 2).sum(-1)
    tied = d == 0.75
    assert (tied.sum(-1) == 8).all()
    lowest = torch.where(tied, torch.arange(216).expand_as(d), torch.full(d.shape, 216)).amin(-1)
    assert torch.equal(idx, lowest)
    _same((dist, idx), reference(points, targets))
    _same(metrics._torch_sided_distance_fwd(points, targets, chunk=3 * 125 * 5), (dist, idx), 'ties across chunks of five targets')


def _with_invalid(x, every=7, first=0):
    """x (B, n, 3) with every `every`-th row from `first` made non-finite: NaN, +inf, -inf in each coordinate in turn, then 2^64 (its
    square overflows) in each."""
    x = x.clone()
    values = (NAN, INF, -INF, 2.0 ** 64)
    for k, row in enumerate(range(first, x.shape[1], every)):
        x[:, row, k % 3] = values[(k // 3) % 4]
    return x


def test_non_finite_input_answers_as_defined_and_no_nan_comes_out():
    p, t = _with_invalid(_cloud(2, 90, 3), 2), _with_invalid(_cloud(2, 100, 4), 3, first=1)
    assert torch.isnan(p).any() and torch.isinf(p).any() and (p == 2.0 ** 64).any() and torch.isnan(t).any() and (t == -INF).any()
    want = reference(p, t)
    got = metrics.sided_distance(p, t)
    _same(got, want)
    bad = ~torch.isfinite(p).all(-1)
    assert (got[1][bad] == -1).all() and (got[0][bad] == INF).all()
    far = (p == 2.0 ** 64).any(-1)                                            # d overflows to +inf, which is not < +inf, except against a
    chosen = torch.gather(t, 1, got[1].clamp(0)[..., None].expand(-1, -1, 3))  # target that is as far in the same coordinate
    assert far.any() and ((got[1] == -1) | ((chosen == 2.0 ** 64) == (p == 2.0 ** 64)).all(-1))[far].all()
    good = torch.isfinite(p).all(-1) & (p.abs() < 2.0 ** 60).all(-1)
    assert (got[1][good] >= 0).all() and torch.isfinite(t[0][got[1][0][good[0]]]).all()
    one = torch.full((2, 1, 3), 0.5)
    one[0, 0, 1] = NAN
    one[1, 0, 2] = NAN
    dist, idx = metrics.sided_distance(_cloud(2, 9, 6), one)                 # M = 1 with a NaN target
    assert (dist == INF).all() and (idx == -1).all()
    _same((dist, idx), reference(_cloud(2, 9, 6), one))
    only_far = metrics.sided_distance(torch.zeros(1, 2, 3), torch.full((1, 3, 3), 2.0 ** 64))
    assert (only_far[0] == INF).all() and (only_far[1] == -1).all()


def test_gradcheck_in_float64_away_from_ties_and_the_gradients_of_empty_rows_and_coincident_points():
    p, t = _cloud(2, 5, 7).double().requires_grad_(), _cloud(2, 7, 8).double().requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: metrics.sided_distance(a, b)[0], (p, t), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, b: metrics.chamfer_distance(a, b, 0.7, 1.3), (p, t), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, b: metrics.chamfer_distance(a, b, squared=False), (p, t), eps=1e-6, atol=1e-7)
    assert torch.autograd.gradcheck(lambda a, b: metrics.hausdorff_distance(a, b), (p, t), eps=1e-6, atol=1e-7)
    for dtype in (torch.float64, torch.float32):
        q = _cloud(2, 6, 9).to(dtype)
        q[0, 2, 1], q[1, 4, 0] = NAN, INF
        q, s = q.requires_grad_(), _cloud(2, 4, 10).to(dtype).requires_grad_()
        dist, idx = metrics.sided_distance(q, s)
        assert idx[0, 2] == -1 and idx[1, 4] == -1 and (idx >= 0).sum() == 10 and not idx.requires_grad
        dist.backward(torch.ones_like(dist))
        assert (q.grad[0, 2] == 0).all() and (q.grad[1, 4] == 0).all()
        assert torch.isfinite(q.grad).all() and torch.isfinite(s.grad).all() and (q.grad != 0).any()
        assert torch.allclose(s.grad.sum(1), -q.grad.sum(1), rtol=1e-5 if dtype == torch.float32 else 1e-12)
        a = _cloud(1, 8, 11).to(dtype).requires_grad_()
        b = a.detach().clone().requires_grad_()
        value = metrics.chamfer_distance(a, b, squared=False)
        value.sum().backward()
        assert value.item() == 0 and torch.isfinite(a.grad).all() and torch.isfinite(b.grad).all()


def test_known_answers_on_lattices():
    lattice, h, eps = _lattice(4)[None], 0.25, 1e-8
    moved = lattice + torch.tensor([h, 0.0, 0.0])
    assert metrics.chamfer_distance(lattice, moved).item() == 2 * h * h
    assert metrics.chamfer_distance(lattice, moved, squared=False).item() == 2 * h
    assert metrics.chamfer_distance(lattice, moved, w1=3.0, w2=0.5).item() == 3.5 * h * h
    assert metrics.hausdorff_distance(lattice, moved).item() == h
    full = torch.tensor(2 / (2 + eps)).float().item()
    assert metrics.f_score(lattice, moved, radius=0.3).item() == full
    assert metrics.f_score(lattice, moved, radius=0.2).item() == 0
    assert metrics.chamfer_distance(lattice, lattice).item() == 0 and metrics.hausdorff_distance(lattice, lattice).item() == 0
    assert metrics.f_score(lattice, lattice).item() == full and metrics.f_score(lattice.double(), lattice.double()).item() == 2 / (2 + eps)
    # one far outlier on one side moves exactly one directed term, and sets the Hausdorff distance to its own
    outlier = torch.cat([lattice, torch.tensor([[[10.0, 0.0, 0.0]]])], 1)                  # 7 from (3, 0, 0)
    there, back = metrics.sided_distance(lattice, outlier), metrics.sided_distance(outlier, lattice)
    assert (there[0] == 0).all() and torch.equal(there[1], torch.arange(64)[None])
    assert (back[0][0, :64] == 0).all() and back[0][0, 64] == 49 and back[1][0, 64] == 48     # (3, 0, 0) is point 3 * 16
    assert metrics.chamfer_distance(lattice, outlier, w2=0.0).item() == 0
    assert metrics.chamfer_distance(lattice, outlier).item() == torch.tensor(49 / 65).float().item()
    assert metrics.hausdorff_distance(lattice, outlier).item() == 7 == metrics.hausdorff_distance(outlier, lattice).item()
    # one prediction of 65 is a false positive; no ground-truth point is missed
    want = 2 * (64 / 65) * 1.0 / (64 / 65 + 1.0 + eps)
    assert metrics.f_score(lattice.double(), outlier.double(), radius=0.5).item() == want


def test_evaluate_distance_composes_the_public_functions():
    out, faces = _sphere(2, 0.1, seed=1)
    ref, _ = _sphere(2, 0.05, seed=2)
    ev = metrics.evaluate_distance
    assert ev(out, ref, faces, 'point2point') == float(((out - ref).double() ** 2).sum(-1).mean())
    assert ev(out, ref, faces, 'point2mesh') == metrics.compute_distance(out, ref, faces)
    assert metrics.compute_distance(out, ref, faces, mode='chamfer') is None
    assert ev(out, ref, faces, 'chamfer') == float(metrics.chamfer_distance(out[None], ref[None])[0]) > 0
    assert ev(out, ref, faces, 'hausdorff') == float(metrics.hausdorff_distance(out[None], ref[None])[0]) > 0
    for radius in ('0.01', '0.05', '0.2'):
        assert ev(out, ref, faces, 'f_' + radius) == float(metrics.f_score(ref[None], out[None], radius=float(radius))[0])
    assert ev(out, ref, faces, 'f_0.01') < ev(out, ref, faces, 'f_0.05') < ev(out, ref, faces, 'f_0.2') <= 1
    for mode in ('chamfer_l1', 'f_', 'f_x', 'f_-1', 'f_inf', 'f_nan', '', None, 'Point2Mesh'):
        with pytest.raises(ValueError):
            ev(out, ref, faces, mode)
    with pytest.raises(ValueError):
        ev(out, ref, faces, 'chamfer', samples=-1)
    with pytest.raises(ValueError):
        ev(out[None], ref[None], faces, 'chamfer')
    from geniconet_amd import sampling
    u = torch.rand((2, 1, 500, 3), generator=torch.Generator().manual_seed(3))
    a, b = sampling.sample_points(out[None], faces, uniforms=u[0])[0], sampling.sample_points(ref[None], faces, uniforms=u[1])[0]
    assert ev(out, ref, faces, 'chamfer', samples=500, seed=3) == float(metrics.chamfer_distance(a, b)[0])
    assert ev(out, ref, faces, 'f_0.05', samples=500, seed=3) == float(metrics.f_score(b, a, radius=0.05)[0])
    assert ev(out, ref, faces, 'hausdorff', samples=500, seed=3) == ev(out, ref, faces, 'hausdorff', samples=500, seed=3)
    assert ev(out, ref, faces, 'chamfer', samples=500, seed=3) != ev(out, ref, faces, 'chamfer', samples=500, seed=4)
    assert ev(out, ref, faces, 'point2point', samples=500) == ev(out, ref, faces, 'point2point')


def test_the_shim_functions_are_the_metrics_functions():
    import geniconet_amd.shims.kaolin.metrics as shim
    from geniconet_amd.shims.kaolin.metrics import pointcloud
    assert shim.pointcloud is pointcloud
    assert pointcloud.sided_distance is metrics.sided_distance and pointcloud.chamfer_distance is metrics.chamfer_distance
    assert pointcloud.f_score is metrics.f_score


def test_bad_shapes_and_mismatched_batches_raise():
    good = _cloud(2, 5, 1)
    for call in (metrics.sided_distance, metrics.chamfer_distance, metrics.f_score, metrics.hausdorff_distance):
        for bad in (good[0], good[..., :2], good[:, :0], good[:0], good.long(), good[None], 'points'):
            with pytest.raises(ValueError):
                call(bad, good)
            with pytest.raises(ValueError):
                call(good, bad)
        with pytest.raises(ValueError, match='batch'):
            call(good, _cloud(3, 5, 2))
        call(good, _cloud(2, 9, 2))                                           # N and M are independent


# ---- GPU: the kernel against the fp32 formulation, bit for bit -----------------------------------------------------------------------
# 256 targets a tile, 256 threads of 2 queries a workgroup: one less, exactly, one more of each; N != M both ways
SIZES = ((1, 255), (255, 1), (255, 256), (256, 255), (256, 257), (257, 256), (257, 1000), (1000, 257), (1, 1000), (1000, 1),
         (511, 256), (512, 1000), (513, 255), (1000, 512))
FAMILIES = ('random', 'clustered', 'lattice', 'scaled down', 'scaled up', 'shifted', 'invalid', 'nan cloud')


def _cycled(x, n, generator):
    """n rows of x (k, 3): x repeated as often as needed (repeats are exact ties) and shuffled."""
    x = x.repeat(-(-n // x.shape[0]), 1)
    return x[torch.randperm(x.shape[0], generator=generator)[:n]]


@functools.lru_cache(maxsize=None)
def _case(family, N, M, B=3):
    """(points, targets, the fp32 formulation's answer) on the CPU: computed once, shared, never changed."""
    seed = 7919 * FAMILIES.index(family) + 31 * N + M
    g = torch.Generator().manual_seed(seed)
    if family == 'clustered':
        centres = torch.randn(B, 8, 3, generator=g)
        p, t = (torch.stack([centres[b][torch.randint(8, (n,), generator=g)] for b in range(B)]) + 0.01 * torch.randn(B, n, 3, generator=g)
                for n in (N, M))
    elif family == 'lattice':
        p = torch.stack([_cycled(_cell_centres(6), N, g) for _ in range(B)])
        t = torch.stack([_cycled(_lattice(6), M, g) for _ in range(B)])
    else:
        p, t = torch.randn(B, N, 3, generator=g), torch.randn(B, M, 3, generator=g)
    if family == 'scaled down':
        p, t = p * 2.0 ** -60, t * 2.0 ** -60
    if family == 'scaled up':
        p, t = p * 2.0 ** 60, t * 2.0 ** 60
    if family == 'shifted':
        p, t = p + 1000.0, t + 1000.0
    if family == 'invalid':
        p, t = _with_invalid(p, 7), _with_invalid(t, 7, first=min(3, M - 1))
    if family == 'nan cloud':
        t[1] = NAN
    return p, t, metrics._torch_sided_distance(p, t)


@pytest.mark.gpu
@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('N,M', SIZES)
def test_hip_equals_the_fp32_formulation_bit_for_bit(N, M, family):
    p, t, want = _case(family, N, M)
    got = metrics._sided_distance_unchecked(p.cuda(), t.cuda())
    _same(got, want, (family, N, M))
    if family == 'nan cloud':
        assert (got[1][1] == -1).all() and (got[0][1] == INF).all() and (got[1][0] >= 0).all()
    if family == 'lattice' and M >= 255:
        assert (want[0] == 0.75).float().mean() > 0.25                        # a corner of the cell is among the targets: up to 8-way ties, and repeats


@pytest.mark.gpu
def test_hip_through_the_checked_function():
    p, t, want = _case('random', 257, 1000)
    _same(metrics.sided_distance(p.cuda(), t.cuda()), want)
    _same(metrics.sided_distance(p.cuda(), t), want, 'the second set follows the first to its device')
    with pytest.raises(ValueError):
        metrics.sided_distance(p.cuda(), t[:2].cuda())


# ---- GPU: the backward -----------------------------------------------------------------------------------------------------------------
TARGETS = 300


def _backward_case(N, B=3):
    """fp32 inputs on the CPU for the backward: clustered points against 300 targets, a third of which lie far away so that nobody
    chooses them; an upstream with zeros on a quarter of the rows."""
    g = torch.Generator().manual_seed(N)
    t = torch.randn(B, TARGETS, 3, generator=g)
    t[:, ::3] += 50.0
    p = t[:, 1::3][:, torch.randint(100, (N,), generator=g)] + 0.3 * torch.randn(B, N, 3, generator=g)
    up = torch.randn(B, N, generator=g) * (torch.rand(B, N, generator=g) > 0.25)
    return p, t, up


@pytest.mark.gpu
@pytest.mark.parametrize('N', (257, 1000))
def test_hip_backward_bit_for_bit_in_the_points_and_within_its_roundings_in_the_targets(N):
    """dpoints is one product chain per row, the fp32 formulation's: equal bits.  dtargets[j] sums the n_j rows that chose j, each
    term -(s e) carrying two roundings (e, the product; s = 2 g is exact) against float64 on the same fp32 inputs, in n_j - 1 fp32
    additions: |got - ref| <= (n_j + 3) 2^-24 A_j, A_j the same sum on absolute values -- the form of the ray caster's backward, which
    uses the same scatter.  Exactly 0 where nobody chose j."""
    p, t, up = _backward_case(N)
    pc, tc = p.cuda().requires_grad_(), t.cuda().requires_grad_()
    dist, idx = metrics._sided_distance_unchecked(pc, tc)
    _same((dist, idx), metrics._torch_sided_distance(p, t))
    dist.backward(up.cuda())
    idx = idx.cpu()
    want_points, want_targets32 = metrics._torch_sided_distance_bwd(p, t, idx, up)
    assert torch.equal(_bits(pc.grad), _bits(want_points))
    # float64 autograd of the float64 formulation at the device's choice
    p64, t64 = p.double().requires_grad_(), t.double().requires_grad_()
    at = idx[..., None].expand(-1, -1, 3)
    e = p64 - torch.gather(t64, 1, at)
    ((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]).backward(up.double())
    terms = -(2 * up.double()[..., None] * e.detach())
    A = torch.zeros_like(t64).scatter_add_(1, at, terms.abs())
    n = torch.zeros_like(t64).scatter_add_(1, at, torch.ones_like(terms))
    assert torch.allclose(torch.zeros_like(t64).scatter_add_(1, at, terms), t64.grad, rtol=1e-12, atol=1e-300)
    assert torch.allclose(p64.grad.float(), pc.grad.cpu(), rtol=1e-6, atol=0)
    share, plain = rho(tc.grad, t64.grad, A * (n + 3)), rho(tc.grad, t64.grad, A)
    print('N = %d, M = %d, dtargets: largest |got - ref| / (2^-24 A) = %.3f, as a share of its bound (n_j + 3) %.3f; most rows on one '
          'target %d' % (N, TARGETS, plain, share, int(n.max())))
    assert n.max() >= 4 and (n == 0).any()
    assert (tc.grad[(n == 0).cuda()] == 0).all() and (tc.grad[(A == 0).cuda()] == 0).all()
    assert share <= 1.0
    assert rho(want_targets32, t64.grad, A * (n + 3)) <= 1.0                 # the fp32 formulation's own scatter keeps the bound too


def _both(pc, tc, upc, needs=(True, True)):
    args = tuple(x.detach().requires_grad_(n) for x, n in zip((pc, tc), needs))
    out = metrics._sided_distance_unchecked(*args)
    if any(needs):
        out[0].backward(upc)
    return out + tuple(x.grad for x in args)


@pytest.mark.gpu
def test_launch_counts_determinism_gradients_one_by_one_and_batch_slicing(monkeypatch):
    p, t, up = _backward_case(257, B=5)
    pc, tc, upc = p.cuda(), t.cuda(), up.cuda()
    whole, kernels = _profiled(lambda: metrics._sided_distance_unchecked(pc, tc))
    assert kernels == {'k_nn_points': 1}
    full, kernels = _profiled(lambda: _both(pc, tc, upc))
    assert kernels == {'k_nn_points': 1, 'k_nn_points_bwd_record': 1, 'k_nn_points_bwd_vertex': 1}
    only_p, kernels = _profiled(lambda: _both(pc, tc, upc, (True, False)))    # without dtargets: no scatter, no workspace
    assert kernels == {'k_nn_points': 1, 'k_nn_points_bwd_record': 1}
    assert only_p[3] is None and torch.equal(only_p[2], full[2])
    only_t, kernels = _profiled(lambda: _both(pc, tc, upc, (False, True)))
    assert kernels == {'k_nn_points': 1, 'k_nn_points_bwd_record': 1, 'k_nn_points_bwd_vertex': 1}
    assert only_t[2] is None and torch.equal(only_t[3], full[3])
    again = _both(pc, tc, upc)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(again, full))  # bit-identical run to run
    assert all(torch.equal(a, b) for a, b in zip(whole, full[:2]))
    for limit, launches in ((2, 3), (1, 5)):
        monkeypatch.setattr(metrics, '_MAX_GRID_Y', limit)
        sliced, kernels = _profiled(lambda: _both(pc, tc, upc))
        assert kernels == {'k_nn_points': launches, 'k_nn_points_bwd_record': launches, 'k_nn_points_bwd_vertex': launches}
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(sliced, full))


@pytest.mark.gpu
@pytest.mark.parametrize('with_gradient', (False, True))
def test_no_host_synchronisation_in_the_unchecked_calls(with_gradient):
    p, t, up = _backward_case(257)
    pc, tc, upc = p.cuda(), t.cuda(), up.cuda()

    def run():
        out = _both(pc, tc, upc, (with_gradient, with_gradient))
        x = pc.detach().requires_grad_(with_gradient)
        value = metrics._chamfer_unchecked(x, tc, 1.0, 0.5)
        if with_gradient:
            value.sum().backward()
        return out + (value, x.grad)
    want = run()                                                              # the allocator settles
    torch.cuda.synchronize()
    probe = torch.ones(1, device='cuda')
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            caught = False
        except RuntimeError:
            caught = True
        if caught:
            got = run()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert caught, "torch.cuda.set_sync_debug_mode('error') does not catch a deliberate .item() on this build"
    assert (got[2] is not None) == (got[3] is not None) == (got[5] is not None) == with_gradient
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, want))


# ---- GPU: the derived metrics ------------------------------------------------------------------------------------------------------------
def _one_rounding(got, want):
    """Means summed in double on either side and rounded once to fp32: equal, or neighbours."""
    got, want = got.cpu().double(), want.double()
    return bool(((got - want).abs() <= 2.0 ** -23 * want.abs()).all())


@pytest.mark.gpu
def test_derived_metrics_on_the_device_are_the_cpu_values():
    """The distances under them are equal bit for bit, so the counts of f_score are exact and the squared chamfer distance differs
    by the order of a double sum at most: one final rounding.  The unsquared figures take a device square root, held to one more."""
    p, t = _cloud(3, 1000, 21) * 0.3, _cloud(3, 700, 22) * 0.3
    pc, tc = p.cuda(), t.cuda()
    assert _one_rounding(metrics.chamfer_distance(pc, tc), metrics.chamfer_distance(p, t))
    assert _one_rounding(metrics.chamfer_distance(pc, tc, 0.25, 3.0), metrics.chamfer_distance(p, t, 0.25, 3.0))
    rooted = metrics.chamfer_distance(pc, tc, squared=False).cpu().double()
    assert ((rooted - metrics.chamfer_distance(p, t, squared=False).double()).abs() <= 2 * 2.0 ** -23 * rooted).all()
    haus = metrics.hausdorff_distance(pc, tc)
    assert _one_rounding(haus, metrics.hausdorff_distance(p, t)) and haus.shape == (3,)
    radii = (0.02, 0.05, 0.1, 0.3)
    scores = [metrics.f_score(p, t, radius=r) for r in radii]
    for r, want in zip(radii, scores):
        assert torch.equal(metrics.f_score(pc, tc, radius=r).cpu(), want), r
    assert all((a <= b).all() for a, b in zip(scores, scores[1:])) and (scores[0] < scores[-1]).all()
    out, faces = _sphere(2, 0.1, seed=1)
    ref, _ = _sphere(2, 0.05, seed=2)
    ev = metrics.evaluate_distance
    for mode in ('point2point', 'chamfer', 'hausdorff'):
        got, want = ev(out.cuda(), ref.cuda(), faces.cuda(), mode), ev(out, ref, faces, mode)
        assert abs(got - want) <= 2.0 ** -23 * want, mode
    for mode in ('f_0.01', 'f_0.05', 'f_0.2'):
        assert ev(out.cuda(), ref.cuda(), faces.cuda(), mode) == ev(out, ref, faces, mode), mode
    assert ev(out.cuda(), ref.cuda(), faces.cuda(), 'point2mesh') == metrics.compute_distance(out.cuda(), ref.cuda(), faces.cuda())
    sampled = ev(out.cuda(), ref.cuda(), faces.cuda(), 'chamfer', samples=2000, seed=5)
    assert sampled == ev(out.cuda(), ref.cuda(), faces.cuda(), 'chamfer', samples=2000, seed=5)
    assert math.isclose(sampled, ev(out, ref, faces, 'chamfer', samples=2000, seed=5), rel_tol=1e-3)
