"""The normal-agreement term of losses.Surface_Loss (factor_normal, normal_oriented) on the HIP path, at r = 2, batch 2, S = 300: the
default leaves the loss bit for bit as it was, the term is the documented composition of the public pieces, its gradient is the
torch formulation's at the same faces, a sheet facing the wrong way costs l_n = 2 at zero distance, and a short descent."""
import pytest
import torch

from geniconet_amd import data, geometry, losses, metrics, sampling

from conftest import rel_l2

R, BATCH, S = 2, 2, 300
REG = dict(factor_edge=0.1, factor_ncons=0.01, factor_smooth=0.1)


def _gpu_case():
    x, t = data.synthetic_batch(BATCH, R, seed=5)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    return (0.9 * x + 0.02 * noise).cuda(), t.cuda()


def _rebuilt_uniforms(seed, forwards=1):
    """The loss's draw, by its contract: one torch.rand((2, B, S, 3)) per forward from a generator seeded with sample_seed."""
    g = torch.Generator(device='cuda')
    g.manual_seed(seed)
    return [torch.rand((2, BATCH, S, 3), generator=g, device='cuda') for _ in range(forwards)]


def _pieces(grid, t, u, search, fna=metrics.face_normal_agreement, oriented=True):
    """(p2m, m2p, l_n) from the public pieces, as the Surface_Loss docstring composes them."""
    faces = torch.from_numpy(geometry.get_ico_faces(R)).cuda()
    ref = t[:, 0:3].transpose(1, 2).contiguous()
    out = losses.grid_to_vertices(grid, R)
    p_out, on_out = sampling.sample_points(out, faces, uniforms=u[0])
    p_ref, on_ref = sampling.sample_points(ref, faces, uniforms=u[1])
    d_out, near_ref, _ = metrics.point_to_mesh_distance(p_out, ref, faces, search=search)
    d_ref, near_out, _ = metrics.point_to_mesh_distance(p_ref, out, faces, search=search)
    l_n = 0.5 * (fna(out, faces, on_out, ref, faces, near_ref, oriented).mean() + fna(ref, faces, on_ref, out, faces, near_out, oriented).mean())
    return d_out.mean(), d_ref.mean(), l_n


@pytest.mark.gpu
@pytest.mark.parametrize('search', ['brute', 'grid'])
def test_factor_normal_zero_changes_nothing(search):
    grid0, t = _gpu_case()
    kw = dict(factor_p2m=0.7, factor_m2p=1.3, search=search, samples=S, sample_seed=9, **REG)
    old, new = losses.Surface_Loss(R, **kw).cuda(), losses.Surface_Loss(R, factor_normal=0.0, normal_oriented=False, **kw).cuda()
    for _ in range(2):                                                        # the second forward: the draw order is intact
        ga, gb = grid0.clone().requires_grad_(), grid0.clone().requires_grad_()
        a, b = old(ga, t), new(gb, t)
        a.backward(), b.backward()
        assert torch.equal(a, b) and torch.equal(ga.grad, gb.grad)
        assert float(new.last_normal) == 0.0 and new.get_last_losses() == old.get_last_losses()


@pytest.mark.gpu
@pytest.mark.parametrize('search', ['brute', 'grid'])
def test_the_term_is_the_documented_composition_and_its_gradient_the_torch_formulations(search):
    grid0, t = _gpu_case()
    crit = losses.Surface_Loss(R, 0.7, 1.3, search=search, samples=S, sample_seed=9, factor_normal=0.5, **REG).cuda()
    for u in _rebuilt_uniforms(9, forwards=2):                                # the term draws nothing of its own: both forwards rebuild
        g = grid0.clone().requires_grad_()
        loss = crit(g, t)
        loss.backward()
        gw = grid0.clone().requires_grad_()
        p2m, m2p, l_n = _pieces(gw, t, u, search)
        want = 0.7 * p2m + 1.3 * m2p + losses.Mesh_Regularizer(R, **REG).cuda()(gw) + 0.5 * l_n
        assert abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
        assert abs(float(crit.last_normal) - float(l_n.detach())) <= 1e-6 * float(l_n.detach()) and float(l_n.detach()) > 0
        got = crit.get_last_losses()
        assert len(got) == 5 and rel_l2(got[:2], [float(p2m.detach()), float(m2p.detach())]) <= 1e-6
        # the same composition with the torch formulation of the normal term, evaluated at the same faces
        gt = grid0.clone().requires_grad_()
        p2m_t, m2p_t, l_n_t = _pieces(gt, t, u, search, fna=metrics._torch_face_normal_agreement)
        (0.7 * p2m_t + 1.3 * m2p_t + losses.Mesh_Regularizer(R, **REG).cuda()(gt) + 0.5 * l_n_t).backward()
        e = rel_l2(g.grad.cpu().numpy(), gt.grad.cpu().numpy())
        print('%s: loss %.8f, l_n %.8f (torch formulation %.8f), output gradient rel-L2 against the torch formulation %.3g'
              % (search, float(loss.detach()), float(l_n.detach()), float(l_n_t.detach()), e))
        assert e <= 1e-6
        # ... and the term really is in the gradient
        assert rel_l2((g.grad - torch.autograd.grad(0.5 * l_n, gw)[0]).cpu().numpy(), g.grad.cpu().numpy()) > 1e-3


def _ellipsoids():
    """Two centrally symmetric targets (the icosphere's vertex set is: -v is a vertex wherever v is) as (B, 9, V) targets, and
    the grid of the point-mirrored mesh: the same surface with every face facing inwards."""
    u = torch.from_numpy(geometry.get_icosahedral_grid(R)[0]).float()
    v = u[None] * torch.tensor([[0.9, 0.7, 0.5], [0.6, 0.8, 0.7]])[:, None]
    t = torch.cat((v, torch.zeros(BATCH, u.shape[0], 6)), dim=2).transpose(1, 2).contiguous()
    return data.target_to_input(-t, R).contiguous().cuda(), t.cuda()


@pytest.mark.gpu
def test_a_sheet_facing_the_wrong_way():
    """The case the term exists for: the distance terms see nothing (what is left, below 1e-4, is the two pole vertices, which the
    output takes as the mean of five pixels), the oriented term is at its maximum of 2 and the unoriented one at 0, up to the ten
    faces of 320 around those poles."""
    grid, t = _ellipsoids()
    seen = {}
    for oriented in (True, False):
        crit = losses.Surface_Loss(R, samples=S, sample_seed=1, factor_normal=0.5, normal_oriented=oriented).cuda()
        loss = crit(grid, t)
        p2m, m2p, _, _, total = crit.get_last_losses()
        seen[oriented] = l_n = float(crit.last_normal)
        print('oriented %s: p2m %.3g, m2p %.3g, l_n %.6f' % (oriented, p2m, m2p, l_n))
        assert 0 <= p2m < 1e-4 and 0 <= m2p < 1e-4 and abs(float(loss.detach()) - (p2m + m2p + 0.5 * l_n)) <= 1e-6 * total
    assert seen[True] > 1.99 and 0 <= seen[False] < 0.01
    # the same target against itself: nothing to pay either way
    crit = losses.Surface_Loss(R, samples=S, sample_seed=1, factor_normal=0.5).cuda()
    crit(data.target_to_input(t, R).contiguous(), t)
    assert 0 <= float(crit.last_normal) < 0.01


def _descent():
    """20 Adam steps (lr 0.003) on the grid itself from the target moved by 0.05 N(0, 1) along its tangent planes, factors 1 / 1 and
    factor_normal 0.5 -> ((p2m + m2p, l_n) before, after, the final grid); both measured on the same fresh draw (seed 77)."""
    _, t = data.synthetic_batch(BATCH, R, seed=5)
    nrm = t[:, 3:6] / t[:, 3:6].norm(dim=1, keepdim=True).clamp_min(1e-12)
    noise = torch.randn(nrm.shape, generator=torch.Generator().manual_seed(11))
    start = t.clone()
    start[:, 0:3] += 0.05 * (noise - (noise * nrm).sum(1, keepdim=True) * nrm)
    grid, t = data.target_to_input(start, R).contiguous().cuda().requires_grad_(), t.cuda()

    def measure():
        probe = losses.Surface_Loss(R, samples=S, sample_seed=77, factor_normal=1.0).cuda()
        with torch.no_grad():
            probe(grid, t)
        return float(probe.last_p2m + probe.last_m2p), float(probe.last_normal)
    crit = losses.Surface_Loss(R, 1.0, 1.0, samples=S, sample_seed=2, factor_normal=0.5).cuda()
    opt = torch.optim.Adam([grid], lr=0.003)
    before = measure()
    for _ in range(20):
        opt.zero_grad()
        crit(grid, t).backward()
        opt.step()
    return before, measure(), grid.detach().clone()


@pytest.mark.gpu
def test_descent_with_the_normal_term_is_deterministic():
    before, after, grid = _descent()
    print('p2m + m2p %.3g -> %.3g, l_n %.5f -> %.5f' % (before[0], after[0], before[1], after[1]))
    assert after[1] < before[1]                                               # l_n decreases
    assert after[0] <= 2 * before[0]                                          # the distance terms do not rise by more than they were
    again = _descent()
    assert again[0] == before and again[1] == after and torch.equal(again[2], grid)


@pytest.mark.gpu
def test_forward_and_backward_with_the_term_do_not_synchronise_the_host():
    grid0, t = _gpu_case()
    crit = losses.SurfaceKLD_Loss(R, search='grid', samples=S, factor_normal=0.5, factor_kl=0.5, **REG).cuda()
    mu, logvar = torch.full((BATCH, 8), 0.3, device='cuda'), torch.full((BATCH, 8), -0.2, device='cuda')
    crit((grid0.clone().requires_grad_(), mu, logvar), t).backward()         # tables, workspaces and the allocator settle
    torch.cuda.synchronize()
    previous = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        g = grid0.clone().requires_grad_()
        loss = crit((g, mu, logvar), t)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g.grad).all()) and float(crit.last_normal) > 0
