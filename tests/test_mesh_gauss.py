"""metrics.angle_defect / gaussian_curvature / total_curvature / curvature_error and the Gaussian-curvature term of
losses.Surface_Loss: without a GPU the torch formulation against a numpy float64 oracle that takes the angles another way (the law of
cosines), known answers (octahedron, cube, plane, cone, Gauss-Bonnet on spheres, a torus and a disc, K R^2 on spheres), invariance,
gradcheck, the documented corner formula, degenerate and hostile input and the argument checks; on the GPU the HIP kernels
(icn_mesh_angle_defect_fwd / _bwd, include/icn_gauss.h) against float64 of the same definition on the same fp32 inputs.

Bars of the device tests (u = 2^-24).  They are derived, not calibrated: the device computes in double and rounds once to fp32, so
    |defect_i - defect64_i| <= 2 u |defect64_i| + 1e-12 (resolved corners at i)
    |dv_i - dv64_i|         <= 2 u |dv64_i| + 2^-40 S_i   per component,   S_i = sum over the corners at i of
                               |g_{k+1} - g_k| / |a| + |g_k - g_{k+2}| / |b|   (every term of dv_i is such a difference times a unit vector
                               over an edge length; 2^-40 allows 2^12 double roundings for the cross product, the normalisation,
                               the division and the shape of the triangle)
    |sum_i defect_i - 4 pi| <= 2 u sum_i |defect_i| + 1e-9   summed in float64 on the host from the fp32 outputs (Gauss-Bonnet)
Worst ratio of the device to each bar over the families, the fan, the soup and the mixed mesh (MI355X, profiles/mesh_gauss.txt):
defect 0.496, gradient 0.500 -- the one rounding to fp32, u of the 2 u allowed; the double part of the bars is never reached.
Gauss-Bonnet at r = 4: the fp32 outputs miss 4 pi by 5.1e-6 against a bar of 7.0e-4, an fp32 formulation of the same angles by about
9e-5 on the device (its index_add sums in another order every run)."""
import functools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, data, geometry, losses, metrics, models
from geniconet_amd.train import build_criterion

from conftest import rel_l2
from test_mesh_curvature import (B, DEGEN_F, DEGEN_V, FAMILIES, OCTA_F, OCTA_V, U, _DropGradient, _family_vertices, _fan, _ico, _mixed,
                                 _perturbed, _profiled, _rotation, _soup, _t)

KERNELS = ('k_mesh_angle_defect_fwd', 'k_mesh_angle_defect_bwd')


# ---- an independent oracle: the angles from the three edge lengths -------------------------------------------------------------------
def _cosine_law_defect(v, f):
    """v (V, 3), f (F, 3) float64 numpy -> defect (V,), every angle as acos((|a|^2 + |b|^2 - |c|^2) / (2 |a| |b|))."""
    total = np.zeros(len(v))
    for k in range(3):
        i, j, l = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (v[j] - v[i], v[l] - v[i], v[l] - v[j]))
        np.add.at(total, i, np.arccos((la * la + lb * lb - lc * lc) / (2 * la * lb)))
    return 2 * math.pi - total


def test_torch_formulation_against_the_law_of_cosines():
    worst = 0.0
    for r in (0, 1, 2, 3):
        _, f = _ico(r)
        for amp in (0.05, 0.2):
            v = np.stack([_perturbed(r, amp, 10 * r + b) for b in range(2)])
            defect = metrics.angle_defect(_t(v, torch.float64), torch.from_numpy(f))
            assert defect.dtype == torch.float64 and defect.shape == v.shape[:2]
            for b in range(2):
                worst = max(worst, np.abs(defect[b].numpy() - _cosine_law_defect(v[b], f)).max())
    print('angle_defect against the law of cosines, worst absolute difference: %.3g' % worst)
    assert worst <= 1e-9


# ---- known answers -------------------------------------------------------------------------------------------------------------------
CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)       # vertex 4 x + 2 y + z
CUBE_QUADS = np.array([[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]])


def _planar_grid():
    ii, jj = np.meshgrid(np.arange(5), np.arange(5), indexing='ij')
    flat = np.stack([0.3 * ii.ravel() + 0.05 * jj.ravel(), 0.2 * jj.ravel(), np.zeros(25)], -1) @ _rotation(5).T + 0.5
    quad = np.array([[5 * i + j, 5 * (i + 1) + j, 5 * (i + 1) + j + 1, 5 * i + j + 1] for i in range(4) for j in range(4)])
    return flat, np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]]), np.array([5 * i + j for i in range(1, 4) for j in range(1, 4)])


def _torus(nu=8, nv=6, big=1.0, small=0.4):
    a, b = np.meshgrid(2 * math.pi * np.arange(nu) / nu, 2 * math.pi * np.arange(nv) / nv, indexing='ij')
    v = np.stack([(big + small * np.cos(b)) * np.cos(a), (big + small * np.cos(b)) * np.sin(a), small * np.sin(b)], -1).reshape(-1, 3)
    at = lambda i, j: (i % nu) * nv + j % nv                                                  # noqa: E731
    quad = np.array([[at(i, j), at(i + 1, j), at(i + 1, j + 1), at(i, j + 1)] for i in range(nu) for j in range(nv)])
    return v, np.concatenate([quad[:, [0, 1, 2]], quad[:, [0, 2, 3]]])


def _defect64(v, f):
    return metrics.angle_defect(_t(np.asarray(v)[None], torch.float64), torch.from_numpy(np.asarray(f)))[0].numpy()


def _total64(v, f):
    return float(metrics.total_curvature(_t(np.asarray(v)[None], torch.float64), torch.from_numpy(np.asarray(f))))


def test_known_answers_of_polyhedra_the_plane_and_the_cone():
    assert np.abs(_defect64(OCTA_V, OCTA_F) - 2 * math.pi / 3).max() <= 1e-12
    one = np.concatenate([CUBE_QUADS[:, [0, 1, 2]], CUBE_QUADS[:, [0, 2, 3]]])
    other = np.concatenate([CUBE_QUADS[:, [0, 1, 3]], CUBE_QUADS[:, [1, 2, 3]]])
    assert sorted(map(tuple, np.sort(one, -1))) != sorted(map(tuple, np.sort(other, -1)))
    for cube_f in (one, other):
        assert np.abs(_defect64(0.7 * CUBE_V @ _rotation(2).T - 0.3, cube_f) - math.pi / 2).max() <= 1e-12
    flat, f, inner = _planar_grid()
    assert np.abs(_defect64(flat, f)[inner]).max() <= 1e-12
    # the apex of a cone of half-angle alpha over a regular n-gon: n equal angles between neighbouring unit slant directions
    for n, alpha in ((3, 0.3), (6, 1.0), (7, 0.5 * math.pi - 1e-3), (12, 1.3)):
        phi = 2 * math.pi * np.arange(n) / n
        rim = 1.7 * np.stack([math.sin(alpha) * np.cos(phi), math.sin(alpha) * np.sin(phi), np.full(n, math.cos(alpha))], -1)
        v = np.concatenate([[[0.0, 0.0, 0.0]], rim]) @ _rotation(n).T + 0.25
        f = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)])
        want = 2 * math.pi - n * math.acos(math.sin(alpha) ** 2 * math.cos(2 * math.pi / n) + math.cos(alpha) ** 2)
        assert abs(_defect64(v, f)[0] - want) <= 1e-12, (n, alpha)


def test_gauss_bonnet_on_spheres_a_torus_and_a_disc():
    for r in (0, 1, 2, 3):
        f = _ico(r)[1]
        for amp in (0.05, 0.2):
            for b in range(2):
                assert abs(_total64(_perturbed(r, amp, 10 * r + b), f) - 4 * math.pi) <= 1e-12 * 4 * math.pi
    v, f = _torus()
    assert len(v) == 48 and len(f) == 96 and len(v) - 3 * len(f) // 2 + len(f) == 0      # chi = V - E + F = 0
    assert abs(_total64(v, f)) <= 1e-12 * 2 * math.pi * len(v)
    # An open fan, a disc.  Gauss-Bonnet with a boundary: the interior defects plus the turning pi - sum theta of the boundary
    # vertices give 2 pi chi = 2 pi; this definition gives every vertex 2 pi - sum theta, pi more at each of the nb boundary vertices.
    for n, height in ((5, 0.0), (9, 0.4)):
        phi = 1.5 * math.pi * np.arange(n + 1) / n
        v = np.concatenate([[[0.0, 0.0, height]], np.stack([(1 + 0.1 * np.arange(n + 1)) * np.cos(phi), np.sin(phi), 0 * phi], -1)])
        f = np.array([[0, 1 + k, 2 + k] for k in range(n)])
        assert abs(_total64(v, f) - math.pi * (n + 2) - 2 * math.pi) <= 1e-12 * 2 * math.pi * len(v)
    flat, f, inner = _planar_grid()
    assert abs(_total64(flat, f) - math.pi * 16 - 2 * math.pi) <= 1e-12 * 2 * math.pi * 25


def test_gaussian_curvature_of_spheres():
    """K R^2 -> 1: exactly the same for every radius, the six-valent vertices narrowing towards 1; the twelve five-valent vertices
    keep an offset, because a third of the incident area is not their Voronoi cell."""
    six, five = [], []
    for r in (1, 2, 3):
        v, f = _ico(r)
        valence = np.bincount(f.ravel(), minlength=len(v))
        assert sorted(set(valence)) == [5, 6] and (valence == 5).sum() == 12
        k = {R: metrics.gaussian_curvature(_t(R * v[None], torch.float64), torch.from_numpy(f))[0] * R * R for R in (0.5, 1.0, 2.0)}
        assert torch.equal(k[0.5], k[1.0]) and torch.equal(k[2.0], k[1.0])               # scaling by a power of two is exact
        k = k[1.0].numpy()
        six.append((k[valence == 6].min(), k[valence == 6].max()))
        five.append((k[valence == 5].min(), k[valence == 5].max()))
    print('K R^2 of the icosphere, r = 1..3: six-valent (min, max)', six, 'five-valent (min, max)', five)
    spread = [max(abs(lo - 1), abs(hi - 1)) for lo, hi in six]
    assert all(a > 2 * b for a, b in zip(spread, spread[1:])) and spread[-1] <= 5e-3
    assert all(hi - lo <= 1e-9 for lo, hi in five) and all(a[0] > b[0] > 1.14 for a, b in zip(five, five[1:]))
    assert np.allclose(six, [(1.04508, 1.04508), (1.00821, 1.01410), (1.00007, 1.00495)], atol=1e-5, rtol=0)
    assert np.allclose([lo for lo, _ in five], [1.17951, 1.15383, 1.14785], atol=1e-5, rtol=0)


# ---- invariance ----------------------------------------------------------------------------------------------------------------------
def test_defect_is_invariant_under_scaling_rotation_and_translation():
    r = 2
    v, f = _perturbed(r, 0.05, 3), _ico(r)[1]
    rot, shift = _rotation(4), np.array([6.0, -8.0, 0.0])                                  # |t| = 10
    d0 = _defect64(v, f)
    shortest = min(np.linalg.norm(v[f[:, k]] - v[f[:, (k + 1) % 3]], axis=-1).min() for k in range(3))
    for s in (0.01, 2.5):
        # the moved coordinates are rounded at size 10 + s: every edge carries up to 2 sqrt(3) eps (10 + s), which turns it by that
        # over its length; six corners of two edges each at a vertex: below 64 eps (10 + s) / (s shortest edge) with room
        assert np.abs(_defect64(s * v @ rot.T + shift, f) - d0).max() <= 64 * 2.0 ** -52 * (10 + s) / (s * shortest)
    assert np.abs(_defect64(v @ rot.T, f) - d0).max() <= 64 * 2.0 ** -52 / shortest


# ---- gradients -----------------------------------------------------------------------------------------------------------------------
def _corner_formula(v, f, g):
    """The documented backward: v (B, V, 3), g (B, V) float64 tensors, f (F, 3) long -> d sum(g defect) / d v."""
    p = [v[:, f[:, k]] for k in range(3)]
    n = torch.linalg.cross(p[1] - p[0], p[2] - p[0])
    unit = n / n.norm(dim=-1, keepdim=True)
    got = torch.zeros_like(v)
    for k in range(3):
        a, b = p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]
        g0, g1, g2 = (g[:, f[:, (k + m) % 3]][..., None] for m in range(3))
        d = (g1 - g0) * torch.linalg.cross(unit, a) / (a * a).sum(-1, keepdim=True) \
            + (g0 - g2) * torch.linalg.cross(unit, b) / (b * b).sum(-1, keepdim=True)
        got = got.index_add(1, f[:, k], d)
    return got


def test_gradcheck_the_corner_formula_and_the_constant_total():
    f = torch.from_numpy(_ico(1)[1])
    v = _t(np.stack([_perturbed(1, 0.1, 1), 0.75 * _perturbed(1, 0.2, 2) + 0.5]), torch.float64, grad=True)
    assert torch.autograd.gradcheck(lambda x: metrics.angle_defect(x, f), (v,), eps=1e-6, atol=1e-7, rtol=1e-6)
    assert torch.autograd.gradcheck(lambda x: metrics.gaussian_curvature(x, f), (v,), eps=1e-6, atol=1e-6, rtol=1e-6)
    g = torch.randn(v.shape[:2], generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    want, = torch.autograd.grad((metrics.angle_defect(v, f) * g).sum(), v)
    got = _corner_formula(v.detach(), f, g)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # Gauss-Bonnet: the total is a constant of the vertices
    total, = torch.autograd.grad(metrics.total_curvature(v, f).sum(), v)
    assert float(total.abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(_corner_formula(v.detach(), f, torch.full_like(g, 0.37)).abs().max()) == 0.0       # the difference form: exactly


# ---- degenerate and hostile input ----------------------------------------------------------------------------------------------------
def _defect_parts(v, f):
    """defect, K, the total and the gradients of a fixed linear form of the defect and of K, all detached."""
    defect = metrics.angle_defect(v, f)
    curv = metrics.gaussian_curvature(v, f)
    total = metrics.total_curvature(v, f)
    # small dyadic weights that depend on (mesh, vertex) only, not on how many vertices there are
    index = torch.arange(defect.shape[1], device=defect.device)[None] * 7 + torch.arange(defect.shape[0], device=defect.device)[:, None] * 3
    weights = ((index % 11) - 5).to(defect.dtype) / 4
    g_d, = torch.autograd.grad((defect * weights).sum(), v)
    g_k, = torch.autograd.grad((curv * weights).sum(), v)
    return defect.detach(), curv.detach(), total.detach(), g_d, g_k


def _check_degenerate(dtype, device):
    f = torch.as_tensor(DEGEN_F, device=device)
    clean_f = torch.as_tensor(OCTA_F, device=device)
    for shift in (0.0, 3.0):
        v = _t(np.stack([DEGEN_V, 2 * DEGEN_V]) + shift, dtype, device, grad=True)
        clean = _t(np.stack([OCTA_V, 2 * OCTA_V]) + shift, dtype, device, grad=True)
        parts, c_parts = _defect_parts(v, f), _defect_parts(clean, clean_f)
        for x in parts:
            assert bool(torch.isfinite(x).all())
        # the degenerate faces add exactly 0: the first six vertices are those of the clean octahedron, bit for bit
        for x, c in zip(parts, c_parts):
            assert torch.equal(x[:, :6], c) if x.dim() > 1 else torch.equal(x, c)
        # vertex 6 (all of its faces unresolved) and vertex 7 (unreferenced): defect, K and the gradients exactly 0
        for x in parts[:2] + parts[3:]:
            assert torch.equal(x[:, 6:], torch.zeros_like(x[:, 6:]))
        assert float((parts[0][:, :6].double() - 2 * math.pi / 3).abs().max()) <= 4 * torch.finfo(dtype).eps


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_degenerate_faces_on_the_torch_path(dtype):
    _check_degenerate(dtype, 'cpu')


def _check_bad_ids_and_non_finite(dtype, device):
    v = _t(np.stack([OCTA_V, OCTA_V + 0.5]), dtype, device)
    clean = torch.as_tensor(OCTA_F, device=device).int()
    want = metrics._angle_defect_unchecked(v, clean), metrics._gaussian_curvature_unchecked(v, clean)
    for bad_face in ([0, 3, -1], [6, 1, 2], [-1, -1, -1], [1, 106, 2]):
        f32 = torch.cat([clean, torch.tensor([bad_face], dtype=torch.int32, device=device)])
        for table in (None, metrics.vertex_face_table(f32, 6)):
            vg = v.clone().requires_grad_()
            defect = metrics._angle_defect_unchecked(vg, f32, table)
            curv = metrics._gaussian_curvature_unchecked(vg, f32, table)
            assert torch.equal(defect.detach(), want[0]) and torch.equal(curv.detach(), want[1])
            g, = torch.autograd.grad((defect * defect).sum() + curv.sum(), vg)
            assert bool(torch.isfinite(g).all())
    # a NaN stays in its own mesh
    v = _t(np.stack([OCTA_V, OCTA_V, OCTA_V]), dtype, device)
    v[1, 4, 1] = float('nan')
    v.requires_grad_()
    defect = metrics.angle_defect(v, clean)
    assert bool(torch.isnan(defect[1]).any()) and bool(torch.isfinite(defect[::2]).all()) and torch.equal(defect[0], defect[2])
    assert bool(torch.isnan(metrics.total_curvature(v, clean)[1]))
    g, = torch.autograd.grad((defect[0] ** 2).sum() + (defect[2] ** 2).sum(), v)
    assert bool(torch.isfinite(g[0]).all()) and torch.equal(g[0], g[2])


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_bad_ids_are_skipped_unchecked_and_non_finite_vertices_propagate(dtype):
    _check_bad_ids_and_non_finite(dtype, 'cpu')


def test_argument_checks():
    v, f = _t(OCTA_V[None]), torch.from_numpy(OCTA_F)
    table = metrics.vertex_face_table(f, 6)
    for fn in (metrics.angle_defect, metrics.gaussian_curvature, metrics.total_curvature):
        fn(v, f, table)
        fn(v, f.int(), list(table))
        for bad in ((v[0], f), (v[:, :, :2], f), (v[:0], f), (v.long(), f), (v, f[:, :2]), (v, f[:0]), (v, f.float()), (v, f.reshape(-1)),
                    (v, f, table[0]), (v, f, (table[0], table[1][:-1])), (v, f, (table[0][:-1], table[1])), (v, f, (table[0].long(), table[1]))):
            with pytest.raises(ValueError):
                fn(*bad)
        for bad in ((v, f + 1), (v, f - 1), (v[:, :5], f)):
            with pytest.raises(IndexError):
                fn(*bad)
    with pytest.raises(ValueError):
        metrics.curvature_error(v, v[0], f)
    assert metrics.curvature_error(v[0], v[0], f) == 0.0
    moved = v[0].clone()
    moved[4, 2] = 1.5
    assert 0.1 < metrics.curvature_error(moved, v[0], f) < 1.0
    assert metrics.angle_defect(v, f).dtype == torch.float32 and metrics.total_curvature(v, f).shape == (1,)


# ---- Surface_Loss on the torch path -------------------------------------------------------------------------------------------------
def test_the_loss_checks_the_factor_and_build_criterion_passes_the_key():
    for cls in (losses.Surface_Loss, losses.SurfaceKLD_Loss):
        for bad in (float('nan'), float('inf'), 'x', True, None):
            with pytest.raises(ValueError):
                cls(1, factor_gauss=bad)
        crit = cls(1)
        assert crit.factor_gauss == 0.0 and float(crit.last_gauss) == 0.0
        crit = cls(1, factor_gauss=0.3)
        assert crit.factor_gauss == 0.3 and crit.samples == 0
        assert sorted(crit.state_dict()) == sorted(cls(1).state_dict()) and not any('gauss' in k for k in crit.state_dict())
    for kind, model in (('surface', 'ico2ico'), ('surfacekld', 'ico2ico_vae')):
        p = models.default_params(model, subdivisions=2)
        p[model]['loss'] = kind
        assert build_criterion(p, 'cpu').factor_gauss == 0.0
        p['ico'].update(factor_gauss=0.3)
        assert build_criterion(p, 'cpu').factor_gauss == 0.3


@pytest.mark.parametrize('samples', [0, 48])
def test_a_zero_factor_leaves_the_loss_alone_and_a_factor_adds_its_term_exactly(samples):
    r = 1
    x, t = data.synthetic_batch(2, r, seed=5)
    kw = dict(factor_edge=0.1, factor_smooth=0.2, factor_volume=0.5, samples=samples, sample_seed=4)
    for dtype in (torch.float32, torch.float64):
        grid, tgt = (0.9 * x).to(dtype).requires_grad_(), t.to(dtype)
        base = losses.Surface_Loss(r, 0.7, 1.3, **kw)(grid, tgt)
        zero = losses.Surface_Loss(r, 0.7, 1.3, factor_gauss=0.0, **kw)
        loss = zero(grid, tgt)
        assert torch.equal(loss, base) and zero.last_gauss == 0
        assert torch.equal(torch.autograd.grad(loss, grid)[0], torch.autograd.grad(base, grid, retain_graph=True)[0])
    # float64: base + factor * l_gauss, exactly
    faces = torch.from_numpy(geometry.get_ico_faces(r))
    noisy = (grid.detach() * (1 + 0.05 * torch.randn(2, 1, 10, 4, generator=torch.Generator().manual_seed(6), dtype=dtype))).requires_grad_()
    base = losses.Surface_Loss(r, 0.7, 1.3, **kw)(noisy, tgt)
    ref = tgt[:, 0:3].transpose(1, 2)
    l_g = ((metrics.angle_defect(losses.grid_to_vertices(noisy, r), faces) - metrics.angle_defect(ref, faces)) ** 2).sum(1).mean()
    assert float(l_g.detach()) > 1e-3
    for fg in (0.3, -2.0):
        crit = losses.Surface_Loss(r, 0.7, 1.3, factor_gauss=fg, **kw)
        loss = crit(noisy, tgt)
        want = base + fg * l_g
        assert torch.equal(loss, want) and torch.equal(crit.last_gauss, l_g.detach())
        assert rel_l2(torch.autograd.grad(loss, noisy)[0].numpy(), torch.autograd.grad(want, noisy, retain_graph=True)[0].numpy()) <= 1e-14
        assert len(crit.get_last_losses()) == 5 and crit.get_last_losses()[4] == float(loss.detach())
    # the term is scale invariant: its gradient has no radial component on a mesh scaled about the origin
    crit = losses.Surface_Loss(r, 0.0, 0.0, factor_gauss=1.0)
    g, = torch.autograd.grad(crit(noisy, tgt), noisy)
    assert float(g.abs().sum()) > 1e-3 and abs(float((g * noisy.detach()).sum())) <= 1e-12 * float(g.abs().sum())
    # the KLD variant passes the factor through
    mu, logvar = torch.zeros(2, 4), torch.zeros(2, 4)
    plain = losses.SurfaceKLD_Loss(r)((noisy.detach().float(), mu, logvar), t)
    kld = losses.SurfaceKLD_Loss(r, factor_gauss=0.3)
    got = kld((noisy.detach().float(), mu, logvar), t)
    assert abs(float(got) - float(plain) - 0.3 * float(l_g.detach())) <= 1e-5 * float(got) and float(kld.last_gauss) > 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
def _corner_sums(v, f, g):
    """float64 numpy v (B, V, 3), g (B, V) -> (count (B, V) of resolved corners at a vertex, S (B, V) of the gradient bar)."""
    count, s = np.zeros(v.shape[:2]), np.zeros(v.shape[:2])
    n = np.cross(v[:, f[:, 1]] - v[:, f[:, 0]], v[:, f[:, 2]] - v[:, f[:, 0]])
    live = (n * n).sum(-1) != 0
    for k in range(3):
        i, j, l = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        la, lb = np.linalg.norm(v[:, j] - v[:, i], axis=-1), np.linalg.norm(v[:, l] - v[:, i], axis=-1)
        term = np.abs(g[:, j] - g[:, i]) / np.where(live, la, 1) + np.abs(g[:, i] - g[:, l]) / np.where(live, lb, 1)
        for b in range(len(v)):
            np.add.at(count[b], i, live[b])
            np.add.at(s[b], i, np.where(live[b], term[b], 0))
    return count, s


def _make_case(v32, f):
    """fp32 vertices (B, V, 3) and faces -> the float64 reference on those inputs: defect, a random upstream, its gradient, the bars."""
    c = dict(v=torch.from_numpy(v32), f=torch.from_numpy(f),
             g=torch.from_numpy(np.random.RandomState(23).randn(*v32.shape[:2]).astype(np.float32)))
    v64 = c['v'].double().requires_grad_()
    defect = metrics.angle_defect(v64, c['f'])
    c['defect64'] = defect.detach().numpy()
    c['grad64'] = torch.autograd.grad((defect * c['g'].double()).sum(), v64)[0].numpy()
    c['count'], c['s'] = _corner_sums(v32.astype(np.float64), f, c['g'].double().numpy())
    c['bar_defect'] = 2 * U * np.abs(c['defect64']) + 1e-12 * c['count']
    c['bar_grad'] = 2 * U * np.abs(c['grad64']) + 2.0 ** -40 * c['s'][..., None]
    return c


@functools.lru_cache(maxsize=None)
def _case(r, amp, shift):
    return _make_case(_family_vertices(r, amp, shift), _ico(r)[1])


def _hip_defect(c, table=None):
    return metrics.angle_defect(c['v'].cuda(), c['f'].cuda(), table)


def _hip_grad(c, table=None, g=None):
    v = c['v'].cuda().requires_grad_()
    out = metrics.angle_defect(v, c['f'].cuda(), table)
    assert isinstance(out.grad_fn, torch.autograd.function.BackwardCFunction)              # the HIP path, not the torch formulation
    return torch.autograd.grad((out * (c['g'] if g is None else g).cuda()).sum(), v)[0].cpu()


def _ratio(err, bar):
    return float(np.where(bar > 0, err / np.where(bar > 0, bar, 1), np.where(err > 0, np.inf, 0)).max())


def _check_within_bars(c, what):
    defect, grad = _hip_defect(c), _hip_grad(c)
    assert defect.dtype == torch.float32 and defect.is_cuda and tuple(defect.shape) == tuple(c['v'].shape[:2])
    assert bool(torch.isfinite(defect).all()) and bool(torch.isfinite(grad).all())
    d = defect.double().cpu().numpy()
    e_d, e_g = np.abs(d - c['defect64']), np.abs(grad.double().numpy() - c['grad64'])
    print('%s: HIP defect %.3g of its bar (worst absolute error %.3g), gradient %.3g of its bar (worst absolute error %.3g)'
          % (what, _ratio(e_d, c['bar_defect']), e_d.max(), _ratio(e_g, c['bar_grad']), e_g.max()))
    assert (e_d <= c['bar_defect']).all() and (e_g <= c['bar_grad']).all()
    # exact zeros where the float64 reference has none of a vertex's faces resolved
    none = torch.from_numpy(c['count'] == 0)
    assert bool((defect.cpu()[none] == 0).all()) and bool((grad[none] == 0).all())
    return d


@pytest.mark.gpu
@pytest.mark.parametrize('r,amp,shift', FAMILIES)
def test_hip_against_float64_on_the_icosphere_families(r, amp, shift):
    c = _case(r, amp, shift)
    d = _check_within_bars(c, 'r = %d, perturbed by %g, shifted by %g' % (r, amp, shift))
    # Gauss-Bonnet from the fp32 outputs, summed in float64 on the host
    miss = np.abs(d.sum(1) - 4 * math.pi)
    print('    |sum defect - 4 pi| %s, bar %s' % (miss, 2 * U * np.abs(d).sum(1) + 1e-9))
    assert (miss <= 2 * U * np.abs(d).sum(1) + 1e-9).all()
    total = metrics.total_curvature(c['v'].cuda(), c['f'].cuda())
    # total_curvature is that sum rounded once more, to fp32
    assert total.dtype == torch.float32
    assert (np.abs(total.double().cpu().numpy() - 4 * math.pi) <= 2 * U * np.abs(d).sum(1) + 1e-9 + 2 * U * 4 * math.pi).all()
    # a uniform upstream: exactly no gradient, bit for bit
    for const in (1.0, -0.37):
        assert float(_hip_grad(c, g=torch.full_like(c['g'], const)).abs().max()) == 0.0
    # one mesh of the batch alone: the same bits (a batch-stride error would show)
    one = dict(c, v=c['v'][2:3], g=c['g'][2:3])
    assert torch.equal(_hip_defect(one), _hip_defect(c)[2:3]) and torch.equal(_hip_grad(one), _hip_grad(c)[2:3])


@pytest.mark.gpu
@pytest.mark.parametrize('mesh', ['fan', 'soup', 'mixed'])
def test_hip_beyond_the_icosphere(mesh):
    v32, f = dict(fan=_fan, soup=_soup, mixed=_mixed)[mesh]()
    c = _make_case(v32, f)
    _check_within_bars(c, mesh)
    assert int((c['count'] == 0).sum()) >= (0 if mesh == 'fan' else B)
    if mesh == 'fan':
        assert c['count'][:, 0].tolist() == [200.0] * B
    k = metrics.gaussian_curvature(c['v'].cuda(), c['f'].cuda())
    assert bool(torch.isfinite(k).all()) and bool((k.cpu()[torch.from_numpy(c['count'] == 0)] == 0).all())
    if mesh == 'mixed':
        _check_degenerate(torch.float32, 'cuda')
        _check_bad_ids_and_non_finite(torch.float32, 'cuda')


@pytest.mark.gpu
def test_hip_tables_that_lie_are_safe():
    """A corners entry of -1 or 3 F is skipped, a corner filed under the wrong vertex is not used, offsets beyond 3 F are clamped."""
    c = _case(1, 0.2, 0.0)
    v, f32, V = c['v'].cuda(), c['f'].int().cuda(), 42
    F = f32.shape[0]
    offsets, corners = metrics.vertex_face_table(f32, V)

    def run(faces, table):
        vg = v.clone().requires_grad_()
        defect = metrics._angle_defect_unchecked(vg, faces, table)
        g, = torch.autograd.grad((defect * c['g'].cuda()).sum(), vg)
        return defect.detach(), g
    want = run(f32, (offsets, corners))
    less = run(f32[:-1].contiguous(), None)                                              # the mesh without its last face
    for strike in (-1, 3 * F, 3 * F + 7, -2 ** 31):
        struck = torch.where(corners >= 3 * (F - 1), torch.full_like(corners, strike), corners)
        assert int((struck != corners).sum()) == 3
        got = run(f32, (offsets, struck))
        # neither direction meets the face any more: each thread gathers over its own slice only
        assert torch.equal(got[0], less[0]) and torch.equal(got[1], less[1]), strike
    swapped = corners.clone()
    swapped[[int(offsets[1]), int(offsets[2])]] = swapped[[int(offsets[2]), int(offsets[1])]]
    got = run(f32, (offsets, swapped))
    assert all(bool(torch.isfinite(x).all()) for x in got)
    assert torch.equal(got[0][:, 3:], want[0][:, 3:]) and not torch.equal(got[0][:, 1:3], want[0][:, 1:3])
    wild = offsets.clone()
    wild[0], wild[V] = -5, 3 * F + 1000
    assert all(torch.equal(a, b) for a, b in zip(run(f32, (wild, corners)), want))


@pytest.mark.gpu
def test_hip_determinism_and_plumbing(monkeypatch):
    c = _case(3, 0.2, 10.0)
    f = c['f'].cuda()
    table = metrics.vertex_face_table(f, c['v'].shape[1])
    defect, grad = _hip_defect(c), _hip_grad(c)
    # two runs, and the table passed or built on demand: identical bits
    for tb in (None, table):
        assert torch.equal(defect, _hip_defect(c, tb)) and torch.equal(grad, _hip_grad(c, tb))
    # non-contiguous vertices and int64 / int32 faces
    wide = torch.zeros(B, c['v'].shape[1], 5, device='cuda')
    wide[..., 1:4] = c['v'].cuda()
    view = wide[..., 1:4].requires_grad_()
    assert not view.is_contiguous() and f.dtype == torch.int64
    out = metrics.angle_defect(view, f.int())
    assert torch.equal(out, defect) and torch.equal(metrics.angle_defect(view.detach(), f), defect)
    g, = torch.autograd.grad((out * c['g'].cuda()).sum(), view)
    assert torch.equal(g.cpu(), grad)
    # which kernels run: one each way; no backward when no gradient arrives
    _, ran = _profiled(lambda: _hip_grad(c, table))
    assert [ran.get(k, 0) for k in KERNELS] == [1, 1]
    _, ran = _profiled(lambda: _hip_defect(c, table))
    assert [ran.get(k, 0) for k in KERNELS] == [1, 0]

    def unused():
        v = c['v'].cuda().requires_grad_()
        (_DropGradient.apply(metrics.angle_defect(v, f, table)).sum() + (v * v).sum()).backward()
        return v.grad
    g, ran = _profiled(unused)
    assert torch.equal(g.cpu(), 2 * c['v']) and [ran.get(k, 0) for k in KERNELS] == [1, 0]
    # gaussian_curvature: both operators, one launch each per direction
    def curvature():
        v = c['v'].cuda().requires_grad_()
        metrics.gaussian_curvature(v, f, table).sum().backward()
        return v.grad
    g, ran = _profiled(curvature)
    assert bool(torch.isfinite(g).all())
    assert [ran.get(k, 0) for k in KERNELS + ('k_mesh_cotlap_fwd', 'k_mesh_cotlap_bwd')] == [1, 1, 1, 1]
    # the batch-slice path: B = 5 in slices of 2, the bits of the one-launch result
    five = dict(c, v=torch.cat([c['v'], c['v'][:2] * 0.5]), g=torch.cat([c['g'], c['g'][:2]]))
    want = _hip_defect(five), _hip_grad(five)
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 2)
    assert list(metrics._batch_slices(5)) == [(0, 2), (2, 2), (4, 1)]
    got, ran = _profiled(lambda: (_hip_defect(five), _hip_grad(five)))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert [ran.get(k, 0) for k in KERNELS] == [6, 3]


@pytest.mark.gpu
def test_no_host_synchronisation_in_the_loss_term_and_the_unchecked_calls():
    r = 2
    x, t = data.synthetic_batch(2, r, seed=7, device='cuda')
    crit = losses.Surface_Loss(r, 1.0, 1.0, search='grid', factor_gauss=0.3).cuda()
    f32 = crit.ico_faces

    def both():
        grid = (0.8 * x).requires_grad_()
        loss = crit(grid, t)
        loss.backward()
        v = losses.grid_to_vertices(0.8 * x, r).requires_grad_()
        (metrics._angle_defect_unchecked(v, f32).sum() + metrics._gaussian_curvature_unchecked(v, f32).sum()).backward()   # no table
        return loss.detach(), grid.grad, v.grad
    both()                                                                                # workspaces and the allocator settle
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
            loss, g, gv = both()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert caught, "torch.cuda.set_sync_debug_mode('error') does not catch a deliberate .item() on this build"
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g).all()) and bool(torch.isfinite(gv).all())
    assert crit.last_gauss.is_cuda and float(crit.last_gauss) > 0


@pytest.mark.gpu
def test_surface_loss_term_on_the_device():
    """r = 2, B = 2: the term alone (the distances switched off) against float64 of the torch formulation, within the bars of the
    kernels carried through the fp32 arithmetic of the term; the pole gradients reach their five corner pixels; with the factor 0
    the loss and its gradient are, bit for bit, those of a module built without the keyword, and none of the new kernels runs.

    The bars.  The device's defects d carry E_i = bar_defect(out)_i + bar_defect(ref)_i between them.  The term is
    l = fg / 2 sum_b sum_i D_i^2 with D = d(out) - d(ref): in fp32 one rounding of D (2 u on D^2), one of the square, at most V - 1 of
    the sum over the vertices, one each of the sum over the two meshes and of the factor, one spare:
        |l - l64| <= fg / 2 sum (2 |D64_i| E_i + E_i^2) + (V + 5) u l64
    The upstream on d(out) is h_i = fg D_i (2 / 2: the mean over two meshes), known to |dh_i| <= fg E_i + 3 u |h64_i|; the kernel
    then stays within its own bar for that upstream, and the upstream's own error passes through the same corner sums:
        |dv_i - dv64_i| <= 2 u |dv64_i| + 2^-40 S_i(h64) + T_i(dh),   T_i = sum over the corners at i of
                           (dh_{k+1} + dh_k) / |a| + (dh_k + dh_{k+2}) / |b|
    and the map from vertices to pixels (a pole's gradient to its five corners, a fifth each) is applied to the bar as it is to the
    gradient, with 4 u of the result for its own roundings."""
    r, n = 2, 4
    fg = 0.3
    x, t = data.synthetic_batch(2, r, seed=7)
    x = 0.8 * x * (1 + 0.05 * torch.randn(2, 1, 5 * n, 2 * n, generator=torch.Generator().manual_seed(8)))
    faces = torch.from_numpy(geometry.get_ico_faces(r))
    V = 10 * n * n + 2

    def run(crit, device):
        grid = x.clone().to(device).requires_grad_()
        loss = crit.to(device)(grid, t.to(device))
        g, = torch.autograd.grad(loss, grid)
        return loss.detach().cpu(), g.cpu(), crit

    # float64 of the torch formulation on the same fp32 inputs
    grid64 = x.double().requires_grad_()
    out64 = losses.grid_to_vertices(grid64, r)
    ref64 = t[:, 0:3].transpose(1, 2).double()
    d_out, d_ref = metrics._torch_angle_defect(out64, faces), metrics._torch_angle_defect(ref64, faces)
    l64 = fg * ((d_out - d_ref) ** 2).sum(1).mean()
    g64, gv64 = torch.autograd.grad(l64, (grid64, out64))
    l64 = float(l64.detach())
    lhip, ghip, crit = run(losses.Surface_Loss(r, 0.0, 0.0, factor_gauss=fg), 'cuda')
    assert crit.last_gauss.is_cuda and l64 > 1e-3
    # the bars
    f = faces.numpy()
    out_np, ref_np = out64.detach().numpy(), ref64.numpy()
    D = (d_out - d_ref).detach().numpy()
    count_out, _ = _corner_sums(out_np, f, np.zeros(D.shape))
    count_ref, _ = _corner_sums(ref_np, f, np.zeros(D.shape))
    E = 2 * U * (np.abs(d_out.detach().numpy()) + np.abs(d_ref.numpy())) + 1e-12 * (count_out + count_ref)
    bar_loss = fg / 2 * (2 * np.abs(D) * E + E * E).sum() + (V + 5) * U * l64
    h64 = fg * D
    dh = fg * E + 3 * U * np.abs(h64)
    _, s_h = _corner_sums(out_np, f, h64)
    t_dh = np.zeros(D.shape)
    for k in range(3):
        i, j, l = f[:, k], f[:, (k + 1) % 3], f[:, (k + 2) % 3]
        la, lb = np.linalg.norm(out_np[:, j] - out_np[:, i], axis=-1), np.linalg.norm(out_np[:, l] - out_np[:, i], axis=-1)
        term = (dh[:, j] + dh[:, i]) / la + (dh[:, i] + dh[:, l]) / lb
        for b in range(2):
            np.add.at(t_dh[b], i, term[b])
    bar_v = 2 * U * np.abs(gv64.numpy()) + (2.0 ** -40 * s_h + t_dh)[..., None]
    probe = x.double().requires_grad_()
    bar_grid, = torch.autograd.grad(losses.grid_to_vertices(probe, r), probe, grad_outputs=torch.from_numpy(bar_v))
    bar_grid = bar_grid.numpy() + 4 * U * np.abs(g64.numpy())
    e_loss, e_grad = abs(float(lhip) - l64), np.abs(ghip.double().numpy() - g64.numpy())
    print('Surface_Loss Gaussian term: loss %.6g, error %.3g, bar %.3g; gradient %.3g of its bar (rel-L2 %.3g)'
          % (l64, e_loss, bar_loss, _ratio(e_grad, bar_grid), rel_l2(ghip.numpy(), g64.numpy())))
    assert e_loss <= bar_loss and (e_grad <= bar_grid).all()
    # a pole's gradient goes to its five corner pixels, a fifth each: those pixels differ from what they get as plain vertices
    chart = 2 * n * n
    flat_hip, flat64 = ghip.reshape(2, 3, -1), g64.reshape(2, 3, -1)
    for pole, pixels in ((0, [c * chart for c in range(5)]), (1, [(c + 1) * chart - 1 for c in range(5)])):
        share = gv64[:, 10 * n * n + pole] / 5
        assert float(share.norm()) > 1e-4
        for p in pixels:
            assert float((flat64[:, :, p] - gv64[:, p] - share).norm()) <= 1e-12 * float(share.norm())
            assert float((flat_hip[:, :, p].double() - flat64[:, :, p]).norm()) <= 0.01 * float(share.norm())
    # beside the other terms, and with the factor at 0
    kw = dict(factor_edge=0.1, factor_smooth=0.2, search='grid', samples=64, sample_seed=3)
    l_plain, g_plain, _ = run(losses.Surface_Loss(r, 0.7, 1.3, **kw), 'cuda')
    (l_zero, g_zero, zero), ran = _profiled(lambda: run(losses.Surface_Loss(r, 0.7, 1.3, factor_gauss=0.0, **kw), 'cuda'))
    assert torch.equal(l_zero, l_plain) and torch.equal(g_zero, g_plain) and zero.last_gauss == 0
    assert not set(ran) & set(KERNELS) and 'k_msample_point' in ran
    (l_full, g_full, full), ran = _profiled(lambda: run(losses.Surface_Loss(r, 0.7, 1.3, factor_gauss=fg, **kw), 'cuda'))
    assert [ran.get(k, 0) for k in KERNELS] == [2, 1]                                     # forward on out and ref, backward on out only
    assert abs(float(l_full) - float(l_plain) - float(lhip)) <= 8 * U * float(l_full)
    assert rel_l2((g_full - g_plain).numpy(), ghip.numpy()) <= 1e-4 and len(full.get_last_losses()) == 5
