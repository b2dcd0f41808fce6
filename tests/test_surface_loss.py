"""losses.Surface_Loss / SurfaceKLD_Loss and their wiring into train.build_criterion / Trainer: descent on the torch path and the
constructor checks without a GPU; on the GPU the composition of the HIP pieces, both searches, the absence of host
synchronisation, descent, the torch fallback, and three Trainer steps with loss='surface'."""
import math

import pytest
import torch

from geniconet_amd import data, geometry, losses, metrics, models
from geniconet_amd.train import Trainer, build_criterion

from conftest import rel_l2

REG = dict(factor_edge=0.1, factor_ncons=0.01, factor_smooth=0.1)


def _descent(device):
    """The recipe: r = 2, synthetic_batch(2, 2, seed=5), start 0.8 * input + 0.03 N(0, 1), 40 Adam steps at lr 0.01 on the grid
    itself, factors 1 / 1 and regularisers 0.1 / 0.01 / 0.1 -> (p2m + m2p at the start, at the end)."""
    r = 2
    x, t = data.synthetic_batch(2, r, seed=5)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(11))
    grid = (0.8 * x + 0.03 * noise).to(device).requires_grad_()
    t = t.to(device)
    crit = losses.Surface_Loss(r, 1.0, 1.0, **REG).to(device)
    opt = torch.optim.Adam([grid], lr=0.01)
    trace = []
    for _ in range(40):
        opt.zero_grad()
        crit(grid, t).backward()
        opt.step()
        trace.append(crit.last_p2m + crit.last_m2p)
    with torch.no_grad():
        crit(grid, t)
    return float(trace[0]), float(crit.last_p2m + crit.last_m2p)


def test_descent_on_the_torch_path():
    start, end = _descent('cpu')
    print('p2m + m2p: %.6f -> %.6f (x %.4f)' % (start, end, end / start))
    assert math.isfinite(end) and end < 0.1 * start


def test_reporting_and_zero_factor_terms():
    r = 1
    x, t = data.synthetic_batch(2, r, seed=5)
    grid = (0.9 * x).requires_grad_()
    crit = losses.Surface_Loss(r, 1.0, 0.0, **REG)
    loss = crit(grid, t)
    p2m, m2p, reg, zero, total = crit.get_last_losses()
    assert m2p > 0 and zero == 0. and abs(total - (p2m + reg)) <= 1e-6 * total and abs(float(loss.detach()) - total) <= 1e-6 * total
    want = metrics.point_to_mesh_distance(t[:, 0:3].transpose(1, 2), losses.grid_to_vertices(grid.detach(), r),
                                          torch.from_numpy(geometry.get_ico_faces(r)))[0].mean()
    assert abs(m2p - float(want)) <= 1e-6 * m2p
    kld = losses.SurfaceKLD_Loss(r, 1.0, 1.0, factor_kl=0.5, **REG)
    mu, logvar = torch.full((2, 8), 0.3), torch.full((2, 8), -0.2)
    both = kld((grid, mu, logvar), t)
    both = float(both.detach())
    assert abs(both - (float(kld.recons_loss.detach()) + 0.5 * float(losses.kld(mu, logvar)))) <= 1e-6 * both
    assert len(kld.get_last_losses()) == 5 and kld.get_factor() == 0.5


def test_build_criterion_kinds_and_constructor_errors():
    p = models.default_params('ico2ico', subdivisions=2)
    p['ico2ico']['loss'] = 'surface'
    p['ico'].update(factor_m2p=0.5, factor_smooth=0.1, edge_length=0.2, p2m_search='grid')
    crit = build_criterion(p, 'cpu')
    assert type(crit) is losses.Surface_Loss and crit.factor_p2m == 1.0 and crit.factor_m2p == 0.5 and crit.search == 'grid'
    assert crit.regularizer.factor_smooth == 0.1 and crit.regularizer.factor_edge == 0.0 and crit.regularizer.edge_length == 0.2
    p = models.default_params('ico2ico_vae', subdivisions=2)
    p['ico2ico_vae']['loss'] = 'surfacekld'
    crit = build_criterion(p, 'cpu')
    assert type(crit) is losses.SurfaceKLD_Loss and crit.factor_kl == 1.0 and crit.search == 'brute'
    for bad in (dict(edge_length=-1.0), dict(edge_length=float('nan')), dict(factor_edge=float('inf')), dict(factor_edge='1')):
        with pytest.raises(ValueError):
            losses.Mesh_Regularizer(2, **{**dict(factor_edge=1.0, factor_ncons=1.0, factor_smooth=1.0), **bad})
    for bad in (dict(search='octree'), dict(subdivisions=-1), dict(subdivisions=2.0), dict(factor_p2m=float('nan')),
                dict(edge_length=-0.5)):
        with pytest.raises(ValueError):
            losses.Surface_Loss(**{**dict(subdivisions=2), **bad})
    with pytest.raises(ValueError):
        losses.Surface_Loss(2)(torch.zeros(2, 3, 20, 9), torch.zeros(2, 9, 162))
    with pytest.raises(ValueError):
        losses.Surface_Loss(2)(torch.zeros(2, 3, 20, 8), torch.zeros(2, 9, 160))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _gpu_case(r=2, B=3):
    x, t = data.synthetic_batch(B, r, seed=5)
    noise = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    return (0.9 * x + 0.02 * noise).cuda(), t.cuda()


@pytest.mark.gpu
def test_hip_path_is_the_sum_of_its_pieces_and_both_searches_agree():
    r = 2
    grid0, t = _gpu_case(r)
    out = {}
    for search in ('brute', 'grid'):
        crit = losses.Surface_Loss(r, 0.7, 1.3, search=search, edge_length=0.1, **REG).cuda()
        g = grid0.clone().requires_grad_()
        loss = crit(g, t)
        loss.backward()
        out[search] = (loss.detach(), g.grad.clone(), crit.get_last_losses())
    assert torch.equal(out['brute'][0], out['grid'][0]) and torch.equal(out['brute'][1], out['grid'][1])
    faces = torch.from_numpy(geometry.get_ico_faces(r)).cuda()
    ref = t[:, 0:3].transpose(1, 2).contiguous()
    g = grid0.clone().requires_grad_()
    p2m = metrics.point_to_mesh_distance(losses.grid_to_vertices(g, r), ref, faces)[0].mean()
    m2p = metrics.point_to_mesh_distance(ref, losses.grid_to_vertices(g, r), faces)[0].mean()
    reg = losses.Mesh_Regularizer(r, edge_length=0.1, **REG)(g)
    grads = [torch.autograd.grad(term, g)[0].double() for term in (p2m, m2p, reg)]
    want_grad = 0.7 * grads[0] + 1.3 * grads[1] + grads[2]
    want = 0.7 * float(p2m) + 1.3 * float(m2p) + float(reg)
    assert abs(float(out['brute'][0]) - want) <= 1e-6 * abs(want)
    assert rel_l2(out['brute'][1].cpu().numpy(), want_grad.cpu().numpy()) <= 1e-6
    got = out['brute'][2]
    assert rel_l2(got[:3], [float(p2m), float(m2p), float(reg)]) <= 1e-6 and got[3] == 0.


@pytest.mark.gpu
def test_forward_and_backward_do_not_synchronise_the_host():
    r = 2
    grid0, t = _gpu_case(r)
    crit = losses.Surface_Loss(r, 1.0, 1.0, search='grid', **REG).cuda()
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
def test_descent_on_the_hip_path():
    start, end = _descent('cuda')
    print('p2m + m2p: %.6f -> %.6f (x %.4f)' % (start, end, end / start))
    assert math.isfinite(end) and end < 0.1 * start


@pytest.mark.gpu
def test_torch_fallback_and_cpu_tensors_give_the_same_value(monkeypatch):
    r = 2
    grid0, t = _gpu_case(r)
    kw = dict(factor_p2m=0.7, factor_m2p=1.3, edge_length=0.1, **REG)
    hip = float(losses.Surface_Loss(r, **kw).cuda()(grid0, t))
    cpu = float(losses.Surface_Loss(r, **kw)(grid0.cpu(), t.cpu()))
    monkeypatch.setattr(losses, '_NO_HIP_LOSS', True)                       # what ICN_NO_HIP_LOSS=1 sets at import
    crit = losses.Surface_Loss(r, **kw).cuda()
    g = grid0.clone().requires_grad_()
    fallback = crit(g, t)
    assert not isinstance(crit.regularizer(g).grad_fn, torch.autograd.function.BackwardCFunction)
    print('hip %.8f, torch regulariser on the device %.8f, cpu %.8f' % (hip, float(fallback), cpu))
    assert abs(float(fallback) - hip) <= 1e-5 * abs(hip) and abs(cpu - hip) <= 1e-5 * abs(hip)


@pytest.mark.gpu
def test_trainer_with_the_surface_loss():
    r, B = 3, 2
    x, t = data.synthetic_batch(B, r, seed=7)
    x, t = x.cuda().contiguous(memory_format=torch.channels_last), t.cuda()

    def run():
        p = models.default_params('ico2ico', subdivisions=r)
        p['ico2ico']['loss'] = 'surface'
        p['ico'].update(REG)
        tr = Trainer(p, 'cuda:0', seed=0)
        assert type(tr.criterion) is losses.Surface_Loss
        return tr, [tr.step(x, t).clone() for _ in range(3)]
    tr, first = run()
    _, second = run()
    for a, b in zip(first, second):
        assert bool(torch.isfinite(a)) and torch.equal(a, b)
    for name, q in tr.model.named_parameters():
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
        assert bool((q.grad != 0).any()), name
    reason = tr.graph_usable()
    assert isinstance(reason, str) and reason
