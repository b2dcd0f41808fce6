"""metrics.face_normal_agreement: the torch formulation against a numpy float64 restatement, known answers, degenerate faces, gradcheck
and the argument checks without a GPU; on the GPU the HIP kernels (icn_face_normal_agree_fwd / _bwd, include/icn_ext.h) against
float64 -- values, gradients of both sides, run-to-run identity, exact zeros, bad ids and non-finite vertices.

Error model of the value checks (u = 2^-24): a cross product of rounded edge vectors has a direction error of about u / s,
s = |n| / (|e1| |e2|) the sine of the angle at vertex 0, so |t - t_64| <= K u (1 / s_a + 1 / s_b) + 16 u.  Without FMA contraction
every component of n carries at most about 4 u |e1| |e2| (one rounding per edge component, per product and for the difference): a
direction error below 4 sqrt(3) u / s < 8 u / s, so K = 8 bounds the fp32 torch formulation on the CPU.  On the GPU K is not assumed:
it is twice what the fp32 torch formulation itself shows in this form against float64 on the same inputs (the margin of
tests/test_gpu_arith.py; it covers FMA-contraction differences)."""
import functools

import numpy as np
import pytest
import torch

from geniconet_amd import data, geometry, losses, metrics, models, sampling
from geniconet_amd.train import build_criterion

from conftest import rel_l2

U = 2.0 ** -24
B = 3
SIZES = (1, 257, 600)


# ---- the definition again, in numpy float64 ------------------------------------------------------------------------------------------
def _unit64(v, f, idx):
    """(n^ (B, S, 3), resolved (B, S), s (B, S)) of faces f[idx] of float64 vertices v (B, V, 3)."""
    tri = v[np.arange(v.shape[0])[:, None, None], f[idx]]                               # (B, S, 3 corners, 3)
    e1, e2 = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
    n = np.stack((e1[..., 1] * e2[..., 2] - e1[..., 2] * e2[..., 1], e1[..., 2] * e2[..., 0] - e1[..., 0] * e2[..., 2],
                  e1[..., 0] * e2[..., 1] - e1[..., 1] * e2[..., 0]), axis=-1)
    with np.errstate(all='ignore'):
        nn, ll = (n * n).sum(-1), (e1 * e1).sum(-1) * (e2 * e2).sum(-1)
        ok = (nn * 2.0 ** 22 > ll) & np.isfinite(nn * 2.0 ** 22)
        unit = np.where(ok[..., None], n / np.sqrt(np.where(ok, nn, 1.0))[..., None], 0.0)
        s = np.where(ok, np.sqrt(nn / np.where(ll > 0, ll, 1.0)), 0.0)
    return unit, ok, s


def _ref64(va, fa, ia, vb, fb, ib, oriented=True):
    """-> (t, c, 1 / s_a + 1 / s_b) in float64."""
    (na, oka, sa), (nb, okb, sb) = _unit64(va, fa, ia), _unit64(vb, fb, ib)
    c = (na * nb).sum(-1)
    with np.errstate(all='ignore'):
        return 1.0 - (c if oriented else np.abs(c)), c, np.where(oka & okb, 1.0 / sa + 1.0 / sb, 0.0)


def _np64(*tensors):
    return [x.detach().cpu().double().numpy() if x.is_floating_point() else x.detach().cpu().numpy() for x in tensors]


# ---- known answers and degenerate faces (integer coordinates: fp32 and float64 agree exactly on what is resolved) -------------------
VERTS = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0], [3, 4, 0]]
FACES = [[0, 1, 2],      # 0: normal +z
         [0, 2, 1],      # 1: normal -z
         [0, 2, 3],      # 2: normal +x
         [1, 5, 2],      # 3: normal +z again, another triangle
         [0, 0, 1],      # 4: v1 = v0
         [1, 2, 1],      # 5: v2 = v0
         [0, 2, 2],      # 6: v1 = v2
         [0, 1, 4]]      # 7: exactly collinear
DEGENERATE = (4, 5, 6, 7)
# (face of a, face of b, t oriented, t unoriented)
KNOWN = [(0, 0, 0., 0.), (0, 3, 0., 0.), (3, 0, 0., 0.), (0, 1, 2., 0.), (1, 3, 2., 0.), (0, 2, 1., 1.), (2, 1, 1., 1.)]


def _toy(dtype, device='cpu'):
    v = torch.tensor(VERTS, dtype=dtype, device=device)[None]
    return v.clone().requires_grad_(), (v.clone() * 2 + 1).requires_grad_(), torch.tensor(FACES, device=device)


def _check_known_answers(dtype, device):
    va, vb, f = _toy(dtype, device)
    ia = torch.tensor([[k[0] for k in KNOWN]], device=device)
    ib = torch.tensor([[k[1] for k in KNOWN]], device=device)
    for oriented, col in ((True, 2), (False, 3)):
        t = metrics.face_normal_agreement(va, f, ia, vb, f, ib, oriented=oriented)
        assert t.shape == ia.shape and t.dtype == dtype
        assert t.detach().cpu().tolist() == [[k[col] for k in KNOWN]], (oriented, t)
    # perpendicular normals: t = 1 like an unresolved sample, but the gradient is there
    ga, gb = torch.autograd.grad(metrics.face_normal_agreement(va, f, ia[:, 5:6], vb, f, ib[:, 5:6]).sum(), (va, vb))
    assert float(ga.abs().max()) > 0.1 and float(gb.abs().max()) > 0.01


def _check_degenerate_faces(dtype, device, fn=metrics.face_normal_agreement):
    """t = 1 and exactly zero gradient rows on BOTH sides wherever either face is unresolved; no NaN anywhere."""
    va, vb, f = _toy(dtype, device)
    pairs = [(d, g) for d in DEGENERATE for g in (0, 2)] + [(g, d) for d in DEGENERATE for g in (0, 2)] + [(4, 7), (6, 5)]
    ia, ib = torch.tensor([[p[0] for p in pairs]], device=device), torch.tensor([[p[1] for p in pairs]], device=device)
    for oriented in (True, False):
        t = fn(va, f, ia, vb, f, ib, oriented=oriented)
        assert t.detach().cpu().tolist() == [[1.0] * len(pairs)]
        ga, gb = torch.autograd.grad((t * torch.arange(1, len(pairs) + 1, device=device, dtype=dtype)).sum(), (va, vb))
        assert torch.equal(ga, torch.zeros_like(ga)) and torch.equal(gb, torch.zeros_like(gb))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_known_answers_on_the_torch_path(dtype):
    _check_known_answers(dtype, 'cpu')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_degenerate_faces_on_the_torch_path(dtype):
    _check_degenerate_faces(dtype, 'cpu')


def _bad_id_and_nan_inputs(dtype, device):
    """Mesh a with a NaN and an infinite vertex; ids -1 and F on either side; -> (args, samples that must be unresolved)."""
    va, vb, f = _toy(dtype, device)
    with torch.no_grad():
        va[0, 5, 1] = float('nan')                                                   # face 3 of a
        vb[0, 3, 0] = float('inf')                                                   # face 2 of b
    F = f.shape[0]
    ia = torch.tensor([[0, -1, F, 0, 0, 3, 0, 0]], device=device)
    ib = torch.tensor([[0, 0, 0, -1, F, 0, 2, 1]], device=device)
    return (va, f.to(torch.int32), ia, vb, f.to(torch.int32), ib), [1, 2, 3, 4, 5, 6]


def _check_bad_ids_and_non_finite_vertices(dtype, device):
    args, bad = _bad_id_and_nan_inputs(dtype, device)
    va, vb = args[0], args[3]
    t = metrics._face_normal_agreement_unchecked(*args)
    want = [0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0]
    assert t.detach().cpu().tolist() == [want]
    for k in range(len(want)):
        ga, gb = torch.autograd.grad(t[0, k], (va, vb), retain_graph=True)
        assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all())
        if k in bad:
            assert torch.equal(ga, torch.zeros_like(ga)) and torch.equal(gb, torch.zeros_like(gb)), k
    ga, gb = torch.autograd.grad(t.sum(), (va, vb))
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all())


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_bad_ids_and_non_finite_vertices_on_the_torch_path(dtype):
    _check_bad_ids_and_non_finite_vertices(dtype, 'cpu')


# ---- perturbed icospheres ------------------------------------------------------------------------------------------------------------
def _mesh(r, seed, batch=B):
    _, t = data.synthetic_batch(batch, r, seed=seed)
    return t[:, 0:3].transpose(1, 2).contiguous(), torch.from_numpy(geometry.get_ico_faces(r)).long()


@functools.lru_cache(maxsize=None)
def _case(S):
    """B = 3 different mesh pairs: side a perturbed icospheres at r = 2 (162 / 320), side b at r = 1 (42 / 80); face_a = the faces
    of S area-weighted samples of a, face_b = the face of b closest to each sample; the float64 reference.  Shared, never modified."""
    (va, fa), (vb, fb) = _mesh(2, 5), _mesh(1, 6)
    u = torch.rand((B, S, 3), generator=torch.Generator().manual_seed(100 + S))
    points, ia = sampling.sample_points(va, fa, uniforms=u)
    ib = metrics.point_to_mesh_distance(points, vb, fb)[1]
    g = torch.rand((B, S), generator=torch.Generator().manual_seed(200 + S)) + 0.5     # the upstream gradient of the backward tests
    t64, c64, inv_s = _ref64(*_np64(va, fa, ia, vb, fb, ib))
    s_a, s_b = _unit64(*_np64(va, fa, ia))[2], _unit64(*_np64(vb, fb, ib))[2]
    assert s_a.min() > 0.1 and s_b.min() > 0.1 and np.abs(c64).min() > 0.1             # s > 0.1 throughout, c away from 0
    assert (va.shape[1], fa.shape[0], vb.shape[1], fb.shape[0]) == (162, 320, 42, 80)
    return dict(va=va, fa=fa, ia=ia, vb=vb, fb=fb, ib=ib, g=g, t64=t64, c64=c64, inv_s=inv_s)


def _args(c, device='cpu', dtype=torch.float32, grad=False):
    va, vb = (c[k].to(device=device, dtype=dtype).requires_grad_(grad) for k in ('va', 'vb'))
    return va, c['fa'].to(device), c['ia'].to(device), vb, c['fb'].to(device), c['ib'].to(device)


@pytest.mark.parametrize('S', SIZES)
def test_torch_path_against_the_numpy_restatement(S):
    c = _case(S)
    t = metrics.face_normal_agreement(*_args(c, dtype=torch.float64))
    assert np.abs(t.numpy() - c['t64']).max() <= 1e-13
    t32 = metrics.face_normal_agreement(*_args(c)).double().numpy()
    excess = np.abs(t32 - c['t64']) - (8 * U * c['inv_s'] + 16 * U)
    print('S = %d: fp32 torch formulation, worst |t - t64| = %.3g, worst excess over the bound %.3g' % (S, np.abs(t32 - c['t64']).max(), excess.max()))
    assert excess.max() <= 0
    flipped_a, flipped_b = c['fa'].clone(), c['fb'].clone()
    flipped_a[1::2], flipped_b[1::2] = c['fa'][1::2][:, [0, 2, 1]], c['fb'][1::2][:, [0, 2, 1]]
    va, _, ia, vb, _, ib = _args(c, dtype=torch.float64)
    tu = metrics.face_normal_agreement(va, flipped_a, ia, vb, flipped_b, ib, oriented=False)
    assert (c['c64'] > 0.1).all() and np.abs(tu.numpy() - c['t64']).max() <= 1e-13


def _pair_r1():
    """An r = 1 icosphere pair with Va != Vb and Fa != Fb: b has ten faces fewer and a vertex no face uses."""
    (va, fa), (vb, fb) = _mesh(1, 5, batch=2), _mesh(1, 6, batch=2)
    vb = torch.cat((vb, torch.full((2, 1, 3), 0.5)), dim=1)
    return va.double(), fa, vb.double(), fb[:-10].clone()


@pytest.mark.parametrize('oriented', [True, False])
def test_gradcheck_in_float64(oriented):
    va, fa, vb, fb = _pair_r1()
    assert (va.shape[1], fa.shape[0], vb.shape[1], fb.shape[0]) == (42, 80, 43, 70)
    gen = torch.Generator().manual_seed(3)
    ia, ib = torch.randint(0, fa.shape[0], (2, 9), generator=gen), torch.randint(0, fb.shape[0], (2, 9), generator=gen)
    c = _ref64(*_np64(va, fa, ia, vb, fb, ib))[1]
    assert np.abs(c).min() > 1e-3                                                     # |c| is differentiable at every sample
    va.requires_grad_(), vb.requires_grad_()
    assert torch.autograd.gradcheck(lambda x, y: metrics.face_normal_agreement(x, fa, ia, y, fb, ib, oriented=oriented), (va, vb),
                                    eps=1e-6, atol=1e-7, rtol=1e-5)
    ga, gb = torch.autograd.grad(metrics.face_normal_agreement(va, fa, ia, vb, fb, ib, oriented=oriented).sum(), (va, vb))
    assert torch.equal(gb[:, -1], torch.zeros(2, 3, dtype=torch.float64))              # the vertex no face uses


def test_argument_errors():
    va, fa, vb, fb = _pair_r1()
    ia, ib = torch.zeros(2, 4, dtype=torch.long), torch.zeros(2, 4, dtype=torch.long)
    fna = metrics.face_normal_agreement
    assert fna(va, fa, ia, vb, fb, ib).shape == (2, 4)
    assert fna(va, fa.int(), ia.int(), vb, fb.int(), ib.int()).shape == (2, 4)
    for bad in ((va[0], fa, ia, vb, fb, ib), (va[..., :2], fa, ia, vb, fb, ib), (va, fa, ia, vb[:1], fb, ib), (va, fa, ia, vb.float(), fb, ib),
                (va.long(), fa, ia, vb.long(), fb, ib), (va, fa[:, :2], ia, vb, fb, ib), (va, fa[:0], ia, vb, fb, ib),
                (va, fa, ia, vb, fb.double(), ib), (va, fa, ia[0], vb, fb, ib), (va, fa, ia[:1], vb, fb, ib[:1]),
                (va, fa, ia, vb, fb, ib[:, :3]), (va, fa, ia.double(), vb, fb, ib), (va, fa, ia[:, :0], vb, fb, ib[:, :0])):
        with pytest.raises(ValueError):
            fna(*bad)
    for bad in ((va, fa + 1, ia, vb, fb, ib), (va, fa, ia, vb, fb - 1, ib), (va, fa, ia + fa.shape[0], vb, fb, ib),
                (va, fa, ia - 1, vb, fb, ib), (va, fa, ia, vb, fb, ib + fb.shape[0]), (va, fa, ia, vb, fb, ib - 1)):
        with pytest.raises(IndexError):
            fna(*bad)


def test_the_loss_takes_the_term_only_with_samples_and_build_criterion_passes_the_keys():
    for cls in (losses.Surface_Loss, losses.SurfaceKLD_Loss):
        with pytest.raises(ValueError):
            cls(1, factor_normal=0.1, samples=0)
        with pytest.raises(ValueError):
            cls(1, factor_normal=float('nan'), samples=8)
        with pytest.raises(ValueError):
            cls(1, factor_normal=0.1, samples=8, normal_oriented=1)
        crit = cls(1)
        assert crit.factor_normal == 0.0 and crit.normal_oriented is True and float(crit.last_normal) == 0.0
        assert cls(1, factor_normal=0.0, samples=0).factor_normal == 0.0
    for kind, model in (('surface', 'ico2ico'), ('surfacekld', 'ico2ico_vae')):
        p = models.default_params(model, subdivisions=2)
        p[model]['loss'] = kind
        crit = build_criterion(p, 'cpu')
        assert crit.factor_normal == 0.0 and crit.normal_oriented is True
        p['ico'].update(surface_samples=64, factor_normal=0.25, normal_oriented=False)
        crit = build_criterion(p, 'cpu')
        assert crit.factor_normal == 0.25 and crit.normal_oriented is False and crit.samples == 64
        p['ico'].update(surface_samples=0)
        with pytest.raises(ValueError):
            build_criterion(p, 'cpu')


def test_the_loss_on_the_torch_path_is_the_documented_composition():
    r, S = 1, 96
    x, t = data.synthetic_batch(2, r, seed=5)
    grid = (0.9 * x).requires_grad_()
    plain = losses.Surface_Loss(r, 0.7, 1.3, samples=S, sample_seed=4)
    crit = losses.Surface_Loss(r, 0.7, 1.3, samples=S, sample_seed=4, factor_normal=0.5)
    base, loss = plain(grid, t), crit(grid, t)
    faces = torch.from_numpy(geometry.get_ico_faces(r))
    u = torch.rand((2, 2, S, 3), generator=torch.Generator().manual_seed(4))
    out, ref = losses.grid_to_vertices(grid, r), t[:, 0:3].transpose(1, 2).contiguous()
    p_out, on_out = sampling.sample_points(out, faces, uniforms=u[0])
    p_ref, on_ref = sampling.sample_points(ref, faces, uniforms=u[1])
    near_ref = metrics.point_to_mesh_distance(p_out, ref, faces)[1]
    near_out = metrics.point_to_mesh_distance(p_ref, out, faces)[1]
    l_n = 0.5 * (metrics.face_normal_agreement(out, faces, on_out, ref, faces, near_ref).mean()
                 + metrics.face_normal_agreement(ref, faces, on_ref, out, faces, near_out).mean())
    want = base + 0.5 * l_n
    assert float(l_n.detach()) > 0 and abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach()))
    assert abs(float(crit.last_normal) - float(l_n.detach())) <= 1e-6 * float(l_n.detach()) and float(plain.last_normal) == 0.0
    assert rel_l2(torch.autograd.grad(loss, grid)[0].numpy(), torch.autograd.grad(want, grid)[0].numpy()) <= 1e-6
    assert len(crit.get_last_losses()) == 5


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _ratio(t32, c):
    """What the bound's K must be for the values t32: max (|t32 - t64| - 16 u) / (u (1 / s_a + 1 / s_b)), at least 0."""
    return max(0.0, float(((np.abs(t32 - c['t64']) - 16 * U) / (U * c['inv_s'])).max()))


@functools.lru_cache(maxsize=None)
def _measured_k():
    """Twice the worst ratio of the fp32 torch formulation on the device over all cases of this file (one K for all of them)."""
    worst = 0.0
    for S in SIZES:
        c = _case(S)
        t32 = metrics._torch_face_normal_agreement(*_args(c, 'cuda')).double().cpu().numpy()
        worst = max(worst, _ratio(t32, c))
        print('S = %d: torch fp32 on the device, worst |t - t64| = %.3g (%.2f u), ratio %.3f'
              % (S, np.abs(t32 - c['t64']).max(), np.abs(t32 - c['t64']).max() / U, _ratio(t32, c)))
    return 2.0 * worst


@functools.lru_cache(maxsize=None)
def _grad64(S):
    """Gradients of sum(g t) to both sides by float64 autograd on the CPU."""
    c = _case(S)
    args = _args(c, dtype=torch.float64, grad=True)
    t = metrics.face_normal_agreement(*args)
    return [x.numpy() for x in torch.autograd.grad((t * c['g'].double()).sum(), (args[0], args[3]))]


def _hip_grads(c, sides=(True, True)):
    va, fa, ia, vb, fb, ib = _args(c, 'cuda')
    va.requires_grad_(sides[0]), vb.requires_grad_(sides[1])
    t = metrics.face_normal_agreement(va, fa, ia, vb, fb, ib)
    assert isinstance(t.grad_fn, torch.autograd.function.BackwardCFunction)          # the HIP path, not the torch formulation
    (t * c['g'].cuda()).sum().backward()
    return t.detach(), va.grad, vb.grad


@pytest.mark.gpu
@pytest.mark.parametrize('S', SIZES)
def test_hip_values_against_float64(S):
    c, K = _case(S), _measured_k()
    t = metrics.face_normal_agreement(*_args(c, 'cuda'))
    assert t.dtype == torch.float32 and t.shape == (B, S)
    err = np.abs(t.double().cpu().numpy() - c['t64'])
    print('S = %d: K = %.3f; HIP worst |t - t64| = %.3g (%.2f u), ratio %.3f' % (S, K, err.max(), err.max() / U, _ratio(t.double().cpu().numpy(), c)))
    assert (err <= K * U * c['inv_s'] + 16 * U).all()
    # every second face of both tables re-wound, unoriented: the unflipped oriented values (c > 0.1 at every sample)
    va, fa, ia, vb, fb, ib = _args(c, 'cuda')
    fa, fb = fa.clone(), fb.clone()
    fa[1::2], fb[1::2] = fa[1::2][:, [0, 2, 1]], fb[1::2][:, [0, 2, 1]]
    tu = metrics.face_normal_agreement(va, fa, ia, vb, fb, ib, oriented=False)
    assert (np.abs(tu.double().cpu().numpy() - c['t64']) <= K * U * c['inv_s'] + 16 * U).all()
    to = metrics.face_normal_agreement(va, fa, ia, vb, fb, ib, oriented=True).double().cpu().numpy()     # ... and oriented they differ
    odd = ((c['ia'] % 2) != (c['ib'] % 2)).numpy()
    assert (np.abs(to - np.where(odd, 2.0 - c['t64'], c['t64'])) <= K * U * c['inv_s'] + 16 * U).all()


@pytest.mark.gpu
@pytest.mark.parametrize('S', SIZES)
def test_hip_gradients_against_float64(S):
    c = _case(S)
    want = _grad64(S)
    args = _args(c, 'cuda', grad=True)
    torch_grads = torch.autograd.grad((metrics._torch_face_normal_agreement(*args) * c['g'].cuda()).sum(), (args[0], args[3]))
    t, ga, gb = _hip_grads(c)
    for side, got, ref32, ref64 in zip('ab', (ga, gb), torch_grads, want):
        e_hip, e_torch = rel_l2(got.cpu().numpy(), ref64), rel_l2(ref32.cpu().numpy(), ref64)
        print('S = %d side %s: rel-L2 against float64: HIP %.3g, torch fp32 %.3g' % (S, side, e_hip, e_torch))
        assert e_hip <= 2 * e_torch + 1e-6
    # bit-identical over two backward calls, and one side alone gives the same bits
    t2, ga2, gb2 = _hip_grads(c)
    assert torch.equal(t, t2) and torch.equal(ga, ga2) and torch.equal(gb, gb2)
    _, only_a, none_b = _hip_grads(c, (True, False))
    _, none_a, only_b = _hip_grads(c, (False, True))
    assert none_a is None and none_b is None and torch.equal(only_a, ga) and torch.equal(only_b, gb)
    # exact zeros at the vertices no sample touches
    for grad, f, idx in ((ga, c['fa'], c['ia']), (gb, c['fb'], c['ib'])):
        touched = torch.zeros(grad.shape[:2], dtype=torch.bool)
        for b in range(B):
            touched[b, f[idx[b]].reshape(-1)] = True
        assert bool((grad.cpu()[~touched] == 0).all()) and bool(torch.isfinite(grad).all())
        assert S > 100 or int((~touched).sum()) > 0


@pytest.mark.gpu
def test_batch_slices_give_the_bits_of_one_launch(monkeypatch):
    """B = 5 pairs of r = 1 icospheres (42 / 80 on both sides), 16 samples, in slices of 2 -- a full slice, a second full one at a
    non-zero offset and a remainder -- against the one-launch result: the forward, and a backward in which only side a requires a
    gradient."""
    (va, fa), (vb, fb) = _mesh(1, 5, batch=5), _mesh(1, 6, batch=5)
    assert (va.shape, fa.shape, vb.shape, fb.shape) == ((5, 42, 3), (80, 3), (5, 42, 3), (80, 3))
    gen = torch.Generator().manual_seed(7)
    ia, ib = torch.randint(0, 80, (5, 16), generator=gen), torch.randint(0, 80, (5, 16), generator=gen)
    c = dict(va=va, fa=fa, ia=ia, vb=vb, fb=fb, ib=ib, g=torch.rand((5, 16), generator=gen) + 0.5)
    assert metrics._MAX_GRID_Y == 65535
    t, ga, none_b = _hip_grads(c, (True, False))
    assert none_b is None and bool((ga.abs().sum((1, 2)) > 0).all()) and len({tuple(row) for row in t.tolist()}) == 5
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 2)
    assert list(metrics._batch_slices(5)) == [(0, 2), (2, 2), (4, 1)]
    t2, ga2, none_b = _hip_grads(c, (True, False))
    assert none_b is None and torch.equal(t2, t) and torch.equal(ga2, ga)


@pytest.mark.gpu
def test_hip_known_answers_degenerate_faces_bad_ids_and_non_finite_vertices():
    _check_known_answers(torch.float32, 'cuda')
    _check_degenerate_faces(torch.float32, 'cuda')
    _check_bad_ids_and_non_finite_vertices(torch.float32, 'cuda')
    args, _ = _bad_id_and_nan_inputs(torch.float32, 'cuda')
    assert isinstance(metrics._face_normal_agreement_unchecked(*args).grad_fn, torch.autograd.function.BackwardCFunction)
    with torch.no_grad():
        assert metrics._face_normal_agreement_unchecked(*args).cpu().tolist() == [[0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0]]


@pytest.mark.gpu
def test_torch_fallback_on_the_device(monkeypatch):
    c = _case(257)
    hip = metrics.face_normal_agreement(*_args(c, 'cuda'))
    monkeypatch.setattr(losses, '_NO_HIP_LOSS', True)                                 # what ICN_NO_HIP_LOSS=1 sets at import
    args = _args(c, 'cuda', grad=True)
    t = metrics.face_normal_agreement(*args)
    assert not isinstance(t.grad_fn, torch.autograd.function.BackwardCFunction)
    assert float((t.detach() - hip).abs().max()) <= 64 * U
