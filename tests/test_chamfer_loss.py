"""losses.Chamfer_Loss / ChamferKLD_Loss and the loss kinds 'chamfer' / 'chamferkld' of train.build_criterion: on the CPU the
criterion equals the formula composed from grid_to_vertices and metrics.chamfer_distance, with and without surface samples; on the
GPU its value and its gradient with respect to the grid are held against float64 at the device's own choice of neighbours."""
import pytest
import torch

from geniconet_amd import geometry, losses, metrics, sampling, train

from error_bounds import U, rho

R, B = 2, 2
N = 2 ** R
V = 10 * N * N + 2


def _inputs(seed=0):
    """A noisy sphere as the output grid (B, 3, 5n, 2n) and another as the target (B, 9, V), fp32 on the CPU."""
    g = torch.Generator().manual_seed(seed)
    v, _ = geometry.get_icosahedral_grid(R)
    v = torch.from_numpy(v).float()
    grid = (v[:V - 2] * (1 + 0.1 * torch.randn(B, V - 2, 1, generator=g))).transpose(1, 2).reshape(B, 3, 5 * N, 2 * N).contiguous()
    target = torch.randn(B, 9, V, generator=g)
    target[:, 0:3] = (v * (1 + 0.05 * torch.randn(B, V, 1, generator=g))).transpose(1, 2)
    return grid, target


def _faces():
    return torch.from_numpy(geometry.get_ico_faces(R)).long()


def test_the_criterion_is_the_formula_with_and_without_samples():
    grid, target = _inputs()
    out, ref = losses.grid_to_vertices(grid, R), target[:, 0:3].transpose(1, 2).contiguous()
    crit = losses.Chamfer_Loss(R)
    value = crit(grid, target)
    assert value.shape == () and value.item() == metrics.chamfer_distance(out, ref).mean().item() > 0
    assert crit.get_last_losses() == (value.item(), 0, 0, 0., value.item())
    weighted = losses.Chamfer_Loss(R, w1=0.25, w2=3.0)(grid, target)
    assert weighted.item() == metrics.chamfer_distance(out, ref, 0.25, 3.0).mean().item() != value.item()
    crit = losses.Chamfer_Loss(R, samples=300, sample_seed=11)
    g = torch.Generator().manual_seed(11)
    for _ in range(2):                                                        # the draw order is the contract: (2, B, S, 3) a forward
        u = torch.rand((2, B, 300, 3), generator=g)
        a, b = sampling.sample_points(out, _faces(), uniforms=u[0])[0], sampling.sample_points(ref, _faces(), uniforms=u[1])[0]
        assert crit(grid, target).item() == metrics.chamfer_distance(a, b).mean().item()
    x = grid.clone().requires_grad_()
    crit(x, target).backward()
    assert torch.isfinite(x.grad).all() and (x.grad != 0).any()
    for bad in (dict(samples=-1), dict(samples=1.5), dict(sample_seed='0'), dict(w1=float('nan')), dict(w2='1')):
        with pytest.raises(ValueError):
            losses.Chamfer_Loss(R, **bad)
    with pytest.raises(ValueError):
        losses.Chamfer_Loss(R)(grid[:, :, :-1], target)
    with pytest.raises(ValueError):
        losses.Chamfer_Loss(R)(grid, target[:, :, :-1])


def test_the_kld_form_adds_the_kld_term():
    grid, target = _inputs(1)
    mu, logvar = torch.randn(B, 16), 0.3 * torch.randn(B, 16)
    crit = losses.ChamferKLD_Loss(R, factor_kl=0.5)
    value = crit((grid, mu, logvar), target)
    recon, kld = losses.Chamfer_Loss(R)(grid, target), losses.kld(mu, logvar)
    assert value.item() == (recon + 0.5 * kld).item()
    assert crit.get_last_losses() == (recon.item(), 0, 0, -kld.item(), value.item())
    assert crit.get_factor() == 0.5


def _params(kind):
    return {'model_name': 'net', 'net': {'loss': kind}, 'ico': {'subdivisions': R, 'factor_pos': 1.0, 'factor_nor': 0.1, 'factor_lap': 0.1}}


def test_build_criterion_builds_the_new_kinds_and_still_builds_the_old_ones():
    crit = train.build_criterion(_params('chamfer'), 'cpu')
    assert type(crit) is losses.Chamfer_Loss and (crit.samples, crit.sample_seed, crit.w1, crit.w2) == (0, 0, 1.0, 1.0)
    crit = train.build_criterion(_params('chamferkld'), 'cpu')
    assert type(crit) is losses.ChamferKLD_Loss and crit.factor_kl == 1.0
    params = _params('chamfer')
    params['ico'].update(surface_samples=64, surface_sample_seed=3, chamfer_w1=2.0, chamfer_w2=0.5)
    crit = train.build_criterion(params, 'cpu')
    assert (crit.samples, crit.sample_seed, crit.w1, crit.w2) == (64, 3, 2.0, 0.5)
    for kind, cls in (('p2p', losses.P2P_Loss), ('p2pkld', losses.P2PKLD_Loss), ('surface', losses.Surface_Loss),
                      ('surfacekld', losses.SurfaceKLD_Loss)):
        assert type(train.build_criterion(_params(kind), 'cpu')) is cls
    with pytest.raises(ValueError):
        train.build_criterion(_params('chamfer_l1'), 'cpu')


@pytest.mark.gpu
def test_value_and_grid_gradient_on_the_device_against_float64():
    """The reference is float64 on the same fp32 inputs AT THE DEVICE'S CHOICE of neighbours (a float64 search may settle a near-tie
    the other way).  A vertex of the output receives its own term of sided(out, ref) and one term from every row of sided(ref, out)
    that chose it, n_v + 1 in all: each a product chain of three roundings (the upstream w / (B V) rounded to fp32, e, the product),
    summed in at most n_v fp32 additions and one more where autograd adds the two gradients -- within the (n + 3) 2^-24 A of the
    dtargets bound with n = n_v + 1.  The pole rule (a pole's gradient goes to its five corner pixels, a fifth each) is linear with
    non-negative coefficients, so it carries bound and A along, and costs a division and an addition: 2 2^-24 A more.  The float64 path
starts from the grid, so the rounding of the fp32 path's pole vertices is part of the comparison: its term is derived below."""
    grid, target = _inputs(2)
    crit = losses.Chamfer_Loss(R, w1=1.0, w2=0.75).cuda()
    x = grid.cuda().requires_grad_()
    value = crit(x, target.cuda())
    value.backward()
    again = grid.cuda().requires_grad_()
    crit(again, target.cuda()).backward()
    assert torch.equal(again.grad, x.grad)                                    # bit-identical run to run
    with torch.no_grad():
        out32, ref32 = losses.grid_to_vertices(grid.cuda(), R), target[:, 0:3].transpose(1, 2).contiguous().cuda()
        i12, i21 = metrics.sided_distance(out32, ref32)[1].cpu(), metrics.sided_distance(ref32, out32)[1].cpu()
    assert (i12 >= 0).all() and (i21 >= 0).all()
    g64 = grid.double().requires_grad_()
    out, ref = losses.grid_to_vertices(g64, R), target[:, 0:3].transpose(1, 2).double()
    out.retain_grad()
    e12 = out - torch.gather(ref, 1, i12[..., None].expand(-1, -1, 3))
    e21 = ref - torch.gather(out, 1, i21[..., None].expand(-1, -1, 3))
    want = (1.0 * (e12 * e12).sum(-1).mean(1) + 0.75 * (e21 * e21).sum(-1).mean(1)).mean()
    want.backward()
    assert abs(value.item() - want.item()) <= 1e-6 * want.item()
    assert abs(crit.get_last_losses()[0] - want.item()) <= 1e-6 * want.item()
    w = 1.0 / (B * V)
    at = i21[..., None].expand(-1, -1, 3)
    A_v = (2 * w * e12.detach()).abs() + torch.zeros_like(e12).scatter_add_(1, at, (2 * 0.75 * w * e21.detach()).abs())
    n_v = 1 + torch.zeros_like(e12).scatter_add_(1, at, torch.ones_like(e12))
    bound_v = (n_v + 3) * A_v
    # the forward's own rounding: a pole of the fp32 path is the fp32 mean of its five pixels (four additions and a division: within
    # 5 2^-24 mean|x| of the float64 mean), and that shift enters every term at the pole, 2 g each
    shift = 5 * losses.grid_to_vertices(grid.double().abs(), R)
    bound_v[:, V - 2:] += (2 * w * (1 + 0.75 * (n_v - 1)) * shift)[:, V - 2:]

    def to_pixels(field):
        """The transpose of grid_to_vertices on a vertex field (B, V, 3) -> (B, 3, 5n, 2n)."""
        probe = torch.zeros_like(g64).requires_grad_()
        return torch.autograd.grad(losses.grid_to_vertices(probe, R), probe, field)[0]
    A, bound = to_pixels(A_v), to_pixels(bound_v) + 2 * to_pixels(A_v)
    share, plain = rho(x.grad, g64.grad, bound), rho(x.grad, g64.grad, A)
    print('Chamfer_Loss at I%d / batch %d: largest |got - ref| / (2^-24 A) of the grid gradient %.3f, as a share of its bound %.3f; '
          'most rows on one vertex %d' % (R, B, plain, share, int(n_v.max()) - 1))
    assert share <= 1.0 and (g64.grad != 0).float().mean() > 0.9             # (a coordinate that is 0 on both meshes has no gradient)
