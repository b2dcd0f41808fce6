"""Area-weighted surface sampling (geniconet_amd.sampling, icn_mesh_sample_fwd / icn_mesh_sample_bwd) and the sampled form of
losses.Surface_Loss.  Without a GPU: the new symbols and their argument checks, the torch formulation against a float64 reference,
the area shares, the loss's defaults, composition and wiring.  On the GPU: forward and backward against float64, degenerate
inputs, the sampled loss with both searches, descent, and two Trainer steps.

The float64 reference (_ref64, numpy) is computed from the same fp32 vertices and the same fp32 uniforms: areas, CDF, search, sqrt and
weights all in float64."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, data, geometry, losses, metrics, models, sampling
from geniconet_amd.train import Trainer, build_criterion

from conftest import rel_l2

U24 = 2.0 ** -24
REG = dict(factor_edge=0.1, factor_ncons=0.01, factor_smooth=0.1)
B, S = 3, 1000


def _ref64(v, f, u):
    """-> face (B, S) int64, points (B, S, 3), cdf (B, F), all float64 numpy, by the definition of sampling's docstring."""
    v, u, f = v.double().numpy(), u.double().numpy(), f.long().numpy()
    face, points, cdfs = [], [], []
    for b in range(v.shape[0]):
        tri = v[b][f]                                                        # (F, 3, 3)
        area = 0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1)
        cdf = np.cumsum(area)
        fb = np.searchsorted(cdf, u[b, :, 0] * cdf[-1], side='right')
        r = np.sqrt(u[b, :, 1])
        w = np.stack((1 - r, r * (1 - u[b, :, 2]), r * u[b, :, 2]), axis=1)
        points.append((w[:, :, None] * tri[fb]).sum(1))
        face.append(fb)
        cdfs.append(cdf)
    return np.stack(face), np.stack(points), np.stack(cdfs)


@functools.lru_cache(maxsize=None)
def _case(r):
    """Vertices perturbed as data.synthetic_batch does, (B, V, 3); the ico faces with the first five rewritten so that two of their
    vertices coincide (area exactly 0); S uniforms per mesh; the float64 reference.  Shared by the tests, never modified."""
    _, t = data.synthetic_batch(B, r, seed=5)
    v = t[:, 0:3].transpose(1, 2).contiguous()
    f = torch.from_numpy(geometry.get_ico_faces(r)).long().clone()
    f[:5, 1] = f[:5, 0]
    u = torch.rand((B, S, 3), generator=torch.Generator().manual_seed(17 + r))
    face, points, cdf = _ref64(v, f, u)
    assert face.max() < f.shape[0]
    return dict(v=v, f=f, u=u, face=face, points=points, cdf=cdf)


def _check_forward(c, points, face, weights=None, cap=0.0):
    """The forward checks of the issue: faces equal the reference's except for at most `cap` of the samples, each excepted one off by
    exactly one face with u0 T within 1e-6 T of the boundary between the two; points within 16 * 2^-24 * M where faces agree."""
    face, points = face.cpu().numpy(), points.double().cpu().numpy()
    v, f, u = c['v'].double().numpy(), c['f'].numpy(), c['u'].double().numpy()
    differ = face != c['face']
    print('faces that differ from float64: %d of %d' % (differ.sum(), differ.size))
    assert differ.mean() <= cap
    for b, s in zip(*np.nonzero(differ)):
        T = c['cdf'][b, -1]
        assert abs(int(face[b, s]) - int(c['face'][b, s])) == 1
        assert abs(u[b, s, 0] * T - c['cdf'][b, min(face[b, s], c['face'][b, s])]) <= 1e-6 * T
    assert (face >= 5).all()                                                 # no sample lands on a zero-area face
    M = np.abs(np.stack([v[b][f[face[b]]] for b in range(B)])).max(axis=(2, 3))        # (B, S): largest |coordinate| of the face
    err = np.abs(points - c['points']).max(axis=2)
    agree = ~differ
    print('points: worst error / (2^-24 M) = %.3f (bound 16)' % (err[agree] / (U24 * M[agree])).max())
    assert (err[agree] <= 16 * U24 * M[agree]).all()
    if weights is not None:
        w = weights.double().cpu().numpy()
        assert (w >= 0).all() and (np.abs(w.sum(2) - 1) <= 4 * U24).all()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_and_argument_checks_without_a_device():
    names = ('icn_mesh_sample_workspace_bytes', 'icn_mesh_sample_fwd', 'icn_mesh_sample_bwd_workspace_bytes', 'icn_mesh_sample_bwd')
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n) and n in _lib.SIGNATURES, n
    L = _lib.lib()
    assert L.icn_abi_version() == 9
    assert L.icn_mesh_sample_workspace_bytes(36, 10242, 10242, 20480) == 36 * 20480 * 8
    assert L.icn_mesh_sample_bwd_workspace_bytes(36, 10242, 10242, 20480) == 36 * 10242 * 40
    assert L.icn_mesh_sample_workspace_bytes(1, 1, 3, 1) == 16                 # rounded up to 16 bytes
    for bad in ((0, 1, 3, 1), (65536, 1, 3, 1), (1, -1, 3, 1), (1, 1, 0, 1), (1, 1, 3, 0)):
        assert L.icn_mesh_sample_workspace_bytes(*bad) == 0 and L.icn_mesh_sample_bwd_workspace_bytes(*bad) == 0
    p = 0x1000                                                               # never dereferenced: every call below fails its checks
    assert L.icn_mesh_sample_fwd(p, p, p, 1, -1, 3, 1, p, p, p, p, 1 << 20, None) != 0
    assert b'icn_mesh_sample_fwd' in L.icn_last_error() and b'sizes' in L.icn_last_error()
    assert L.icn_mesh_sample_fwd(p, None, p, 1, 4, 3, 1, p, p, p, p, 1 << 20, None) != 0
    assert b'null pointer' in L.icn_last_error()
    assert L.icn_mesh_sample_fwd(p, p, p, 1, 4, 3, 1, p, p, p, None, 0, None) != 0
    assert b'workspace' in L.icn_last_error()
    assert L.icn_mesh_sample_fwd(p, p, p, 1, 4, 3, 1, p, p, p, p + 4, 1 << 20, None) != 0
    assert b'aligned' in L.icn_last_error()
    assert L.icn_mesh_sample_bwd(p, p, p, p, 1, -1, 3, 1, p, p, 1 << 20, None) != 0
    assert b'icn_mesh_sample_bwd' in L.icn_last_error() and b'sizes' in L.icn_last_error()
    assert L.icn_mesh_sample_bwd(p, p, p, None, 1, 4, 3, 1, p, p, 1 << 20, None) != 0
    assert b'null pointer' in L.icn_last_error()
    assert L.icn_mesh_sample_bwd(p, p, p, p, 1, 4, 3, 1, p, p, 8, None) != 0
    assert b'workspace' in L.icn_last_error()


@pytest.mark.parametrize('r', (2, 3))
def test_torch_path_against_float64(r):
    c = _case(r)
    v = c['v'].clone().requires_grad_()
    points, face = sampling.sample_points(v, c['f'], uniforms=c['u'])
    assert face.dtype == torch.int64 and tuple(points.shape) == (B, S, 3) and points.dtype == torch.float32
    _check_forward(c, points.detach(), face, sampling._torch_sample(c['v'], c['f'], c['u'])[2], cap=0.0)
    # the gradient: to the vertices through the weights, face choice constant
    dp = torch.randn(points.shape, generator=torch.Generator().manual_seed(2))
    got, = torch.autograd.grad(points, v, dp)
    w = sampling._torch_sample(c['v'], c['f'], c['u'])[2]
    want = torch.zeros(B, v.shape[1], 3, dtype=torch.float64)
    for b in range(B):
        for k in range(3):
            want[b].index_add_(0, c['f'][face[b], k], (w[b, :, k:k + 1] * dp[b]).double())
    assert rel_l2(got.numpy(), want.numpy()) <= 1e-6
    # drawn uniforms: a generator reproduces them; the argument checks
    a = sampling.sample_points(c['v'], c['f'], num_samples=64, generator=torch.Generator().manual_seed(4))
    b_ = sampling.sample_points(c['v'], c['f'], uniforms=torch.rand((B, 64, 3), generator=torch.Generator().manual_seed(4)))
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])
    with pytest.raises(IndexError):
        sampling.sample_points(c['v'], c['f'] + 1, num_samples=4)
    for bad in (dict(), dict(num_samples=4, uniforms=c['u']), dict(num_samples=0), dict(num_samples=True), dict(uniforms=c['u'][:2]),
                dict(uniforms=c['u'][..., :2])):
        with pytest.raises(ValueError):
            sampling.sample_points(c['v'], c['f'], **bad)


def test_degenerate_inputs_on_the_torch_path():
    c = _case(2)
    flat = torch.zeros_like(c['f'])
    flat[:, 2] = 1
    points, face = sampling.sample_points(c['v'], flat, uniforms=c['u'])
    assert bool((face == 0).all()) and bool(torch.isfinite(points).all())
    u = c['u'][:, :8].clone()
    u[:, 0, 0], u[:, 1, 0], u[:, 2, 0], u[:, 3, 1], u[:, 4, 2], u[:, 5, 1] = 1.0, -0.5, float('nan'), float('nan'), 7.0, -1.0
    clamped = torch.nan_to_num(u, nan=0.0).clamp(0, 1)
    got, want = sampling.sample_points(c['v'], c['f'], uniforms=u), sampling.sample_points(c['v'], c['f'], uniforms=clamped)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and bool(torch.isfinite(got[0]).all())
    assert bool((got[1][:, 0] == c['f'].shape[0] - 1).all()) and bool((got[1][:, 1] == 5).all())   # last / first face with an area


def test_area_shares():
    """The r = 0 icosahedron stretched x 3 along x, S = 65 536: every face's share of the samples within five standard deviations of
    its share of the area -- for the float64 sampler alone (so the seed is a fair one) and for the torch path."""
    n = 65536
    v = torch.from_numpy(geometry.get_icosahedral_grid(0)[0]).float()[None] * torch.tensor([3.0, 1.0, 1.0])
    f = torch.from_numpy(geometry.get_ico_faces(0)).long()
    u = torch.rand((1, n, 3), generator=torch.Generator().manual_seed(23))
    face64, _, cdf = _ref64(v, f, u)
    p = np.diff(cdf[0], prepend=0.0) / cdf[0, -1]
    assert p.max() / p.min() > 1.5                                           # the stretch made the areas unequal
    tol = 5 * np.sqrt(p * (1 - p) / n)
    _, face = sampling.sample_points(v, f, uniforms=u)
    for name, got in (('float64', face64[0]), ('torch path', face[0].numpy())):
        share = np.bincount(got, minlength=20) / n
        print('%s: worst |share - p| / tol = %.3f' % (name, (np.abs(share - p) / tol).max()))
        assert (np.abs(share - p) <= tol).all(), name


def _rebuilt_uniforms(seed, batch, samples, device):
    """The loss's draw, by its contract: one torch.rand((2, B, S, 3)) per forward from a generator seeded with sample_seed."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return torch.rand((2, batch, samples, 3), generator=g, device=device)


def _composition(grid, t, r, u, search='brute'):
    """(p2m, m2p) of the sampled loss from the public pieces."""
    faces = torch.from_numpy(geometry.get_ico_faces(r)).to(grid.device)
    ref = t[:, 0:3].transpose(1, 2).contiguous()
    out = losses.grid_to_vertices(grid, r)
    p2m = metrics.point_to_mesh_distance(sampling.sample_points(out, faces, uniforms=u[0])[0], ref, faces, search=search)[0].mean()
    m2p = metrics.point_to_mesh_distance(sampling.sample_points(ref, faces, uniforms=u[1])[0], out, faces, search=search)[0].mean()
    return p2m, m2p


def test_loss_defaults_and_sampled_composition():
    r = 1
    x, t = data.synthetic_batch(2, r, seed=5)
    grid = (0.9 * x).requires_grad_()
    old, new = losses.Surface_Loss(r, 0.7, 1.3, **REG), losses.Surface_Loss(r, 0.7, 1.3, samples=0, sample_seed=9, **REG)
    a, b_ = old(grid, t), new(grid, t)
    assert torch.equal(a, b_) and torch.equal(torch.autograd.grad(a, grid)[0], torch.autograd.grad(b_, grid)[0])
    crit = losses.Surface_Loss(r, 0.7, 1.3, samples=512, sample_seed=9, **REG)
    loss = crit(grid, t)
    p2m, m2p = _composition(grid, t, r, _rebuilt_uniforms(9, 2, 512, 'cpu'))
    want = 0.7 * p2m + 1.3 * m2p + losses.Mesh_Regularizer(r, **REG)(grid)
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
    assert rel_l2(torch.autograd.grad(loss, grid)[0].numpy(), torch.autograd.grad(want, grid)[0].numpy()) <= 1e-6
    got = crit.get_last_losses()
    assert rel_l2(got[:2], [float(p2m), float(m2p)]) <= 1e-6
    assert float(crit(grid, t).detach()) != float(loss.detach())                               # the second forward draws new samples
    kld = losses.SurfaceKLD_Loss(r, 0.7, 1.3, factor_kl=0.5, samples=512, sample_seed=9, **REG)
    mu, logvar = torch.full((2, 8), 0.3), torch.full((2, 8), -0.2)
    both = float(kld((grid, mu, logvar), t).detach())
    assert abs(both - (float(want.detach()) + 0.5 * float(losses.kld(mu, logvar)))) <= 1e-6 * abs(both)
    for bad in (-1, 1.0, True, '4', None):
        with pytest.raises(ValueError):
            losses.Surface_Loss(r, samples=bad)
        with pytest.raises(ValueError):
            losses.SurfaceKLD_Loss(r, samples=bad)
    for bad in (1.5, True, None):
        with pytest.raises(ValueError):
            losses.Surface_Loss(r, samples=4, sample_seed=bad)


def test_build_criterion_and_the_kaolin_shim():
    p = models.default_params('ico2ico', subdivisions=2)
    p['ico2ico']['loss'] = 'surface'
    crit = build_criterion(p, 'cpu')
    assert crit.samples == 0 and crit.sample_seed == 0
    p['ico'].update(surface_samples=300, surface_sample_seed=12)
    crit = build_criterion(p, 'cpu')
    assert type(crit) is losses.Surface_Loss and crit.samples == 300 and crit.sample_seed == 12
    p = models.default_params('ico2ico_vae', subdivisions=2)
    p['ico2ico_vae']['loss'] = 'surfacekld'
    p['ico'].update(surface_samples=7)
    crit = build_criterion(p, 'cpu')
    assert type(crit) is losses.SurfaceKLD_Loss and crit.samples == 7 and crit.sample_seed == 0 and crit.factor_kl == 1.0
    import geniconet_amd.shims.kaolin.ops.mesh as kaolin_mesh
    c = _case(2)
    torch.manual_seed(31)
    got = kaolin_mesh.sample_points(c['v'], c['f'], 200, areas=torch.ones(B, c['f'].shape[0]))
    torch.manual_seed(31)
    want = sampling.sample_points(c['v'], c['f'], num_samples=200)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and tuple(got[0].shape) == (B, 200, 3)


def _descent(device, samples):
    """The recipe of tests/test_surface_loss.py::_descent -- r = 2, synthetic_batch(2, 2, seed=5), start 0.8 * input + 0.03 N(0, 1),
    40 Adam steps at lr 0.01 on the grid itself, factors 1 / 1 and regularisers 0.1 / 0.01 / 0.1 -- with `samples`; scored at the
    start and at the end by the samples = 0 criterion -> (p2m + m2p at the start, at the end)."""
    r = 2
    x, t = data.synthetic_batch(2, r, seed=5)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(11))
    grid = (0.8 * x + 0.03 * noise).to(device).requires_grad_()
    t = t.to(device)
    crit = losses.Surface_Loss(r, 1.0, 1.0, samples=samples, **REG).to(device)
    score = losses.Surface_Loss(r, 1.0, 1.0, **REG).to(device)
    with torch.no_grad():
        score(grid, t)
    start = float(score.last_p2m + score.last_m2p)
    opt = torch.optim.Adam([grid], lr=0.01)
    for _ in range(40):
        opt.zero_grad()
        crit(grid, t).backward()
        opt.step()
    with torch.no_grad():
        score(grid, t)
    return start, float(score.last_p2m + score.last_m2p)


def _check_descent(device):
    s0, e0 = _descent(device, 0)
    s1, e1 = _descent(device, 512)
    print('vertex-only: %.6f -> %.6f (x %.4f); samples = 512: %.6f -> %.6f (x %.4f)' % (s0, e0, e0 / s0, s1, e1, e1 / s1))
    assert math.isfinite(e1) and e1 < s1 and e1 / s1 <= 2 * (e0 / s0)


def test_descent_with_samples_on_the_torch_path():
    _check_descent('cpu')


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _gpu_forward(c):
    v, u = c['v'].cuda(), c['u'].cuda()
    return v, u, c['f'].cuda().int().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize('r', (2, 3))
def test_hip_forward_against_float64(r):
    c = _case(r)
    v, u, f32 = _gpu_forward(c)
    points, face, weights = sampling._hip_sample(v, f32, u)
    torch.cuda.synchronize()
    assert face.dtype == torch.int32
    _check_forward(c, points, face.long(), weights, cap=0.005)
    again = sampling._hip_sample(v, f32, u)
    assert all(torch.equal(a, b_) for a, b_ in zip((points, face, weights), again))
    pub = sampling.sample_points(v, c['f'].cuda(), uniforms=u)
    assert torch.equal(pub[0], points) and torch.equal(pub[1], face.long())


@pytest.mark.gpu
@pytest.mark.parametrize('r', (2, 3))
def test_hip_backward_against_float64(r):
    c = _case(r)
    v, u, f32 = _gpu_forward(c)
    V = v.shape[1]
    _, face, weights = sampling._hip_sample(v, f32, u)
    dp = torch.randn((B, S, 3), generator=torch.Generator().manual_seed(2)).cuda()
    got = sampling._hip_sample_bwd(f32, face, weights, dp, V)
    assert torch.equal(got, sampling._hip_sample_bwd(f32, face, weights, dp, V))
    want = torch.zeros(B, V, 3, dtype=torch.float64)
    mag = torch.zeros(B, V, 3, dtype=torch.float64)
    count = torch.zeros(B, V, dtype=torch.float64)
    ids = c['f'][face.long().cpu()]                                          # (B, S, 3) vertex ids of the kernel's own faces
    wd = weights.double().cpu()[..., None] * dp.double().cpu()[:, :, None, :]          # (B, S, 3 corners, 3)
    for b in range(B):
        for k in range(3):
            want[b].index_add_(0, ids[b, :, k], wd[b, :, k])
            mag[b].index_add_(0, ids[b, :, k], wd[b, :, k].abs())
            count[b].index_add_(0, ids[b, :, k], torch.ones(S, dtype=torch.float64))
    err = (got.double().cpu() - want).abs()
    bound = (count[..., None] + 2) * U24 * mag
    print('worst error / bound = %.3f; vertices no sample touches: %d' % (float((err / bound.clamp_min(1e-300)).max()), int((count == 0).sum())))
    assert bool((err <= bound).all())
    assert bool((got.cpu()[count == 0] == 0).all())
    # with 16 samples per mesh most vertices are touched by none: exactly 0 there
    few = sampling._hip_sample_bwd(f32, face[:, :16].contiguous(), weights[:, :16].contiguous(), dp[:, :16].contiguous(), V).cpu()
    untouched = torch.ones(B, V, dtype=torch.bool)
    for b in range(B):
        untouched[b, ids[b, :16].reshape(-1)] = False
    assert int(untouched.sum()) >= B * (V - 48) and bool((few[untouched] == 0).all()) and bool((few[~untouched] != 0).any())
    vg = v.clone().requires_grad_()
    points, _ = sampling.sample_points(vg, c['f'].cuda(), uniforms=u)
    assert torch.equal(torch.autograd.grad(points, vg, dp)[0], got)


@pytest.mark.gpu
def test_hip_degenerate_inputs():
    c = _case(2)
    v, u, f32 = _gpu_forward(c)
    V, F = v.shape[1], f32.shape[0]
    # every face without an area: face 0 for every sample
    flat = torch.zeros_like(f32)
    flat[:, 2] = 1
    points, face, weights = sampling._sample_points_unchecked(v, flat, u)
    assert bool((face == 0).all()) and bool(torch.isfinite(points).all()) and bool(torch.isfinite(weights).all())
    # uniforms outside [0, 1] and NaN are clamped
    bad = u[:, :8].clone()
    bad[:, 0, 0], bad[:, 1, 0], bad[:, 2, 0], bad[:, 3, 1], bad[:, 4, 2], bad[:, 5, 1] = 1.0, -0.5, float('nan'), float('nan'), 7.0, -1.0
    got = sampling._sample_points_unchecked(v, f32, bad)
    want = sampling._sample_points_unchecked(v, f32, torch.nan_to_num(bad, nan=0.0).clamp(0, 1))
    assert all(torch.equal(a, b_) for a, b_ in zip(got, want)) and bool(torch.isfinite(got[0]).all())
    assert bool((got[1][:, 0] == F - 1).all()) and bool((got[1][:, 1] == 5).all())
    # a vertex id >= V through the unchecked entry point: the face counts as area 0 and no sample takes it; handed to the backward
    # all the same, with face ids outside [0, F) beside it, those samples contribute nothing
    f_bad = f32.clone()
    f_bad[7, 2] = V + 5
    points, face, weights = sampling._sample_points_unchecked(v, f_bad, u)
    assert bool((face != 7).all()) and bool(torch.isfinite(points).all())
    forced = face.int().clone()
    forced[:, 0], forced[:, 1], forced[:, 2] = 7, F + 3, -1
    dp = torch.ones(B, S, 3, device='cuda')
    got = sampling._hip_sample_bwd(f_bad, forced, weights, dp, V)
    masked = dp.clone()
    masked[:, :3] = 0
    want = sampling._hip_sample_bwd(f32, face.int(), weights, masked, V)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    # the batch slicing: more meshes than one launch's gridDim.y
    nb = 65537
    tri = torch.rand((nb, 3, 3), generator=torch.Generator().manual_seed(8)).cuda().requires_grad_()
    one = torch.tensor([[0, 1, 2]], dtype=torch.int32, device='cuda')
    uu = torch.rand((nb, 1, 3), generator=torch.Generator().manual_seed(9)).cuda()
    points, face, weights = sampling._sample_points_unchecked(tri, one, uu)
    assert bool((face == 0).all())
    want = (weights.detach()[:, 0, :, None].double() * tri.detach().double()).sum(1)
    assert float((points.detach()[:, 0].double() - want).abs().max()) <= 16 * U24
    grad, = torch.autograd.grad(points.sum(), tri)
    assert torch.equal(grad, weights[:, 0, :, None].expand(nb, 3, 3))


def _gpu_case(r=2, batch=3):
    x, t = data.synthetic_batch(batch, r, seed=5)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    return (0.9 * x + 0.02 * noise).cuda(), t.cuda()


@pytest.mark.gpu
def test_sampled_loss_on_the_hip_path(monkeypatch):
    r = 2
    grid0, t = _gpu_case(r)
    out = {}
    for search in ('brute', 'grid'):
        crit = losses.Surface_Loss(r, 0.7, 1.3, search=search, edge_length=0.1, samples=512, sample_seed=4, **REG).cuda()
        g = grid0.clone().requires_grad_()
        loss = crit(g, t)
        loss.backward()
        out[search] = (loss.detach(), g.grad.clone(), crit.get_last_losses())
    assert torch.equal(out['brute'][0], out['grid'][0]) and torch.equal(out['brute'][1], out['grid'][1])
    g = grid0.clone().requires_grad_()
    p2m, m2p = _composition(g, t, r, _rebuilt_uniforms(4, 3, 512, 'cuda'))
    reg = losses.Mesh_Regularizer(r, edge_length=0.1, **REG)(g)
    grads = [torch.autograd.grad(term, g)[0].double() for term in (p2m, m2p, reg)]
    want_grad = 0.7 * grads[0] + 1.3 * grads[1] + grads[2]
    want = 0.7 * float(p2m) + 1.3 * float(m2p) + float(reg)
    assert abs(float(out['brute'][0]) - want) <= 1e-6 * abs(want)
    assert rel_l2(out['brute'][1].cpu().numpy(), want_grad.cpu().numpy()) <= 1e-6
    assert rel_l2(out['brute'][2][:3], [float(p2m), float(m2p), float(reg)]) <= 1e-6
    monkeypatch.setattr(losses, '_NO_HIP_LOSS', True)                       # what ICN_NO_HIP_LOSS=1 sets at import
    crit = losses.Surface_Loss(r, 0.7, 1.3, edge_length=0.1, samples=512, sample_seed=4, **REG).cuda()
    fallback = float(crit(grid0, t))
    print('hip %.8f, torch formulation on the device %.8f' % (want, fallback))
    assert abs(fallback - float(out['brute'][0])) <= 1e-5 * abs(fallback)


@pytest.mark.gpu
def test_sampled_loss_does_not_synchronise_the_host():
    r = 2
    grid0, t = _gpu_case(r)
    crit = losses.Surface_Loss(r, 1.0, 1.0, search='grid', samples=512, **REG).cuda()
    crit(grid0.clone().requires_grad_(), t).backward()                      # tables, workspaces and the allocator settle
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
            g = grid0.clone().requires_grad_()
            loss = crit(g, t)
            loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    if not caught:
        pytest.skip("torch.cuda.set_sync_debug_mode('error') does not catch a deliberate .item() on this build")
    assert math.isfinite(float(loss)) and bool(torch.isfinite(g.grad).all())


@pytest.mark.gpu
def test_descent_with_samples_on_the_hip_path():
    _check_descent('cuda')


@pytest.mark.gpu
def test_trainer_with_surface_samples():
    """Two steps with surface_samples = 256, reproduced bit for bit by a second Trainer with the same seeds.  At r = 3: the ico2ico
    model goes down three levels, so it cannot be built at r = 2 (IcoConvS2S: stride 2 needs subdivisions >= 1)."""
    r, batch = 3, 2
    x, t = data.synthetic_batch(batch, r, seed=7)
    x, t = x.cuda().contiguous(memory_format=torch.channels_last), t.cuda()

    def run():
        p = models.default_params('ico2ico', subdivisions=r)
        p['ico2ico']['loss'] = 'surface'
        p['ico'].update(REG, surface_samples=256, surface_sample_seed=3)
        tr = Trainer(p, 'cuda:0', seed=0)
        assert type(tr.criterion) is losses.Surface_Loss and tr.criterion.samples == 256 and tr.criterion.sample_seed == 3
        return [tr.step(x, t).clone() for _ in range(2)]
    first, second = run(), run()
    for a, b_ in zip(first, second):
        assert bool(torch.isfinite(a)) and torch.equal(a, b_)


# ---- the shared records -> vertices scatter and the shared scan, on dyadic inputs: every fp32 sum is exact, so equality ----------------
@pytest.mark.gpu
@pytest.mark.parametrize('samples', (1, 255, 256, 257, 513))
def test_vertex_scatter_equals_a_float64_index_add_on_dyadic_inputs(samples):
    """icn_mesh_sample_bwd alone: two meshes of 258 vertices (two blocks of vertices), faces on vertices 0, 255, 256 and 257, weights
    and dpoints multiples of 1 / 8 in [-4, 4]; the record counts straddle the tile of 256.  One record names a face out of range."""
    nb, V = 2, 258
    f = torch.tensor([[0, 255, 256], [255, 256, 257], [257, 0, 1], [2, 3, 4], [256, 257, 0], [100, 200, 255]], dtype=torch.int32)
    g = torch.Generator().manual_seed(samples)
    face = torch.randint(0, f.shape[0], (nb, samples), generator=g, dtype=torch.int32)
    face[1, samples // 2] = f.shape[0]                                       # out of range: contributes nothing
    weights = torch.randint(-32, 33, (nb, samples, 3), generator=g).float() / 8
    dp = torch.randint(-32, 33, (nb, samples, 3), generator=g).float() / 8
    got = sampling._hip_sample_bwd(f.cuda(), face.cuda(), weights.cuda(), dp.cuda(), V).cpu()
    want = torch.zeros(nb, V, 3, dtype=torch.float64)
    for b in range(nb):
        ok = face[b] < f.shape[0]
        ids = f.long()[face[b][ok].long()]
        for k in range(3):
            want[b].index_add_(0, ids[:, k], weights[b][ok][:, k:k + 1].double() * dp[b][ok].double())
    if samples >= 255:                                                       # both blocks of vertices and their edge are hit
        assert bool((want[:, [0, 255, 256, 257]] != 0).any(-1).all())
    assert torch.equal(got.double(), want)


@pytest.mark.gpu
@pytest.mark.parametrize('faces', (1, 1023, 1024, 1025, 2049))
def test_area_scan_selects_every_face_of_a_strip_of_congruent_triangles(faces):
    """F right triangles of area 1 / 8 (the second mesh: twice the size), so c_f = (f + 1) / 8 exactly; u0 = (f + 0.5) / F lies in the
    middle of face f's share and must select it, across the scan's tile of 1024 and its waves; u0 = 1 selects the last face."""
    k = torch.arange(faces, dtype=torch.float32)
    zero, half = torch.zeros(faces), torch.full((faces,), 0.5)
    v = torch.stack([torch.stack([k, zero, zero], 1), torch.stack([k + half, zero, zero], 1), torch.stack([k, half, zero], 1)], 1)
    v = torch.stack([v.reshape(-1, 3), 2 * v.reshape(-1, 3)]).cuda()         # (2, 3 F, 3)
    f32 = torch.arange(3 * faces, dtype=torch.int32).reshape(faces, 3).cuda()
    u = torch.zeros(2, faces, 3)
    u[:, :, 0] = (k + 0.5) / faces
    _, face, _ = sampling._hip_sample(v, f32, u.cuda())
    assert torch.equal(face.cpu(), torch.arange(faces, dtype=torch.int32).expand(2, faces))
    _, face, _ = sampling._hip_sample(v, f32, torch.tensor([1.0, 0.25, 0.25]).expand(2, 1, 3).contiguous().cuda())
    assert face.cpu().tolist() == [[faces - 1], [faces - 1]]


@pytest.mark.gpu
def test_batch_slicing_of_the_launch_limit_applies_to_the_sampler(monkeypatch):
    """The batch index is gridDim.y (<= 65535 per launch, metrics._MAX_GRID_Y); with the limit lowered to 1 the three meshes go through
    three launches of the forward and of the backward each, and nothing may change."""
    r, samples = 1, 64
    v = _case(r)['v'].cuda()
    f = _case(r)['f'].cuda()
    u = torch.rand((B, samples, 3), generator=torch.Generator().manual_seed(3)).cuda()
    dp = torch.randn((B, samples, 3), generator=torch.Generator().manual_seed(4)).cuda()

    def run():
        vg = v.clone().requires_grad_()
        points, face = sampling.sample_points(vg, f, uniforms=u)
        return points.detach(), face, torch.autograd.grad(points, vg, dp)[0]
    whole = run()
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 1)
    sliced = run()
    assert all(torch.equal(a, b_) for a, b_ in zip(whole, sliced))
