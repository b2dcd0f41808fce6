"""metrics.mesh_area_volume / vertex_face_table / volume_error and the volume and area terms of losses.Surface_Loss: the torch
formulation against a numpy float64 restatement, known answers, degenerate faces, gradcheck and the argument checks without a GPU; on
the GPU the HIP kernels (icn_mesh_measure_fwd / _bwd, include/icn_measure.h) against float64 -- values, gradients per term,
run-to-run identity, exact zeros, bad tables.

Error model of the value checks (u = 2^-24).  A per-face value is a sum of products of three (volume) or two (area) rounded
differences: one rounding per component of each difference vector, per product and per sum, so every component of a cross product
carries at most about 4 u |a| |b| and the vector 4 sqrt(3) u |a| |b| < 8 u |a| |b| (the argument of tests/test_normal_agreement.py);
the dot product with the third vector and the square root add less than that again only in the constant's slack, and FMA
contraction only removes roundings.  Hence
    |volume - vol64| <= 8 u sum_f |v0 - o| |v1 - o| |v2 - o| / 6 + u |vol64|
    |area - area64|  <= 8 u sum_f |e1| |e2| / 2 + u |area64|
the last terms for the final rounding to fp32 (the sums themselves run in double).  The constant is derived, not measured: numpy
fp32 on synthetic_np meshes, r = 0..5, shifts up to 1000 and scales 1e-3..37, shows at most 1.6 per face and 0.5 for a sum.
The float64 reference is taken on the fp32-rounded vertices, so both sides see the same mesh.
Gradients: rel-L2 against float64 autograd per term, bounded by twice what the fp32 torch formulation itself shows on the same
inputs (the margin of tests/test_gpu_arith.py), with a floor of 1e-6."""
import functools

import numpy as np
import pytest
import torch

from geniconet_amd import data, geometry, losses, metrics, models
from geniconet_amd.train import build_criterion
from oracle import ico_ref, make_goldens

from conftest import rel_l2

U = 2.0 ** -24
B = 3


# ---- the definition again, in numpy float64 ------------------------------------------------------------------------------------------
def _ref64(v, f):
    """v (B, V, 3) float64, f (F, 3) -> dict(area, volume, area_scale = sum |e1| |e2| / 2, volume_scale = sum |a| |b| |c| / 6), (B,)
    each; a face with a vertex id outside [0, V) takes no part."""
    f = f[((f >= 0) & (f < v.shape[1])).all(1)]
    p0, p1, p2 = v[:, f[:, 0]], v[:, f[:, 1]], v[:, f[:, 2]]
    e1, e2 = p1 - p0, p2 - p0
    o = v[:, 0:1]
    a, b, c = p0 - o, p1 - o, p2 - o
    length = lambda x: np.sqrt((x * x).sum(-1))                                         # noqa: E731
    return dict(area=0.5 * length(np.cross(e1, e2)).sum(1), volume=(a * np.cross(b, c)).sum(-1).sum(1) / 6,
                area_scale=0.5 * (length(e1) * length(e2)).sum(1), volume_scale=(length(a) * length(b) * length(c)).sum(1) / 6)


# ---- meshes --------------------------------------------------------------------------------------------------------------------------
CUBE_V = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)       # vertex 4 x + 2 y + z


def _cube_faces():
    """12 triangles, wound counter-clockwise seen from outside: each quad is split, then a triangle whose normal points towards
    the centre is reversed."""
    quads = ([0, 1, 3, 2], [4, 5, 7, 6], [0, 1, 5, 4], [2, 3, 7, 6], [0, 2, 6, 4], [1, 3, 7, 5])
    faces = []
    for q in quads:
        for tri in ([q[0], q[1], q[2]], [q[0], q[2], q[3]]):
            p = CUBE_V[tri]
            if np.dot(np.cross(p[1] - p[0], p[2] - p[0]), p.mean(0) - 0.5) < 0:
                tri = [tri[0], tri[2], tri[1]]
            faces.append(tri)
    return np.array(faces, dtype=np.int64)


CUBE_F = _cube_faces()
TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float64)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)
# the cube with a vertex 8 on the line through vertices 0 and 4, an unreferenced vertex 9, and the degenerate faces of
# tests/test_normal_agreement.py: v1 = v0, v2 = v0, v1 = v2, exactly collinear
DEGEN_V = np.concatenate([CUBE_V, [[2, 0, 0], [7, 7, 7]]])
DEGEN_F = np.concatenate([CUBE_F, [[0, 0, 1], [1, 2, 1], [0, 2, 2], [0, 4, 8]]])


def _t(v, dtype=torch.float32, device='cpu', grad=False):
    return torch.as_tensor(np.asarray(v), dtype=dtype, device=device).requires_grad_(grad)


def _av(v, f, dtype=torch.float32, device='cpu'):
    """(area, volume) of ONE mesh as Python floats."""
    a, vol = metrics.mesh_area_volume(_t(v[None], dtype, device), torch.as_tensor(f, device=device))
    assert a.shape == vol.shape == (1,) and a.dtype == vol.dtype == dtype
    return float(a), float(vol)


def _check_known_answers(dtype, device):
    assert _av(CUBE_V, CUBE_F, dtype, device) == (6.0, 1.0)
    assert _av(CUBE_V, CUBE_F[:, [0, 2, 1]], dtype, device) == (6.0, -1.0)             # every face reversed
    assert _av(CUBE_V + np.array([5.0, -7.0, 3.0]), CUBE_F, dtype, device) == (6.0, 1.0)
    assert _av(3 * CUBE_V - 1, CUBE_F, dtype, device) == (54.0, 27.0)
    a, vol = _av(TETRA_V, TETRA_F, dtype, device)
    eps = torch.finfo(dtype).eps
    assert abs(vol - 1.0 / 6) <= eps / 6 and abs(a - (1.5 + 0.5 * 3 ** 0.5)) <= 2 * eps * a
    # an open mesh: the cone over vertex 0.  Without the three faces at cube vertex 0 nothing changes (their apex is on them) ...
    away = CUBE_F[(CUBE_F != 0).all(1)]
    assert len(away) == 6 and _av(CUBE_V, away, dtype, device) == (3.0, 1.0)
    # ... and the three faces at vertex 0 alone span no volume
    assert _av(CUBE_V, CUBE_F[(CUBE_F == 0).any(1)], dtype, device) == (3.0, 0.0)
    # int32 faces and a batch
    a, vol = metrics.mesh_area_volume(_t(np.stack([CUBE_V, 2 * CUBE_V + 1]), dtype, device), torch.as_tensor(CUBE_F, device=device).int())
    assert a.tolist() == [6.0, 24.0] and vol.tolist() == [1.0, 8.0]
    assert metrics.volume_error(_t(2 * CUBE_V, dtype, device), _t(CUBE_V, dtype, device), torch.as_tensor(CUBE_F)) == 7.0
    assert metrics.volume_error(_t(CUBE_V + 3, dtype, device), _t(CUBE_V, dtype, device), torch.as_tensor(CUBE_F)) == 0.0


def _check_degenerate_faces(dtype, device):
    """The degenerate faces change no value, put no NaN into any gradient, and the unreferenced vertex gets an exact zero row."""
    f = torch.as_tensor(DEGEN_F, device=device)
    for shift in (0.0, 3.0):
        v = _t(np.stack([DEGEN_V, 2 * DEGEN_V]) + shift, dtype, device, grad=True)
        a, vol = metrics.mesh_area_volume(v, f)
        assert a.tolist() == [6.0, 24.0] and vol.tolist() == [1.0, 8.0]
        w = torch.tensor([1.0, -2.0], dtype=dtype, device=device)
        for out in (a, vol, a + 3 * vol):
            g, = torch.autograd.grad((out * w).sum(), v, retain_graph=True)
            assert bool(torch.isfinite(g).all())
            assert torch.equal(g[:, 9], torch.zeros_like(g[:, 9]))
            # ... and vertex 8, which only the collinear face references, moves neither measure to first order
            assert torch.equal(g[:, 8], torch.zeros_like(g[:, 8]))
        clean = _t(np.stack([CUBE_V, 2 * CUBE_V]) + shift, dtype, device, grad=True)
        ca, cvol = metrics.mesh_area_volume(clean, torch.as_tensor(CUBE_F, device=device))
        g, = torch.autograd.grad(((a + 3 * vol) * w).sum(), v)
        cg, = torch.autograd.grad(((ca + 3 * cvol) * w).sum(), clean)
        assert torch.equal(g[:, :8], cg)                                                # integer coordinates: exact either way


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_known_answers_on_the_torch_path(dtype):
    _check_known_answers(dtype, 'cpu')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_degenerate_faces_on_the_torch_path(dtype):
    _check_degenerate_faces(dtype, 'cpu')


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_torch_path_against_the_numpy_restatement(dtype):
    for r in (0, 1, 2):
        f = ico_ref.faces_from_lattice(r)
        for shift in (0.0, 10.0):
            v = _t(make_goldens.synthetic_np(B, r, seed=11 + r) + shift, dtype)
            want = _ref64(v.double().numpy(), f)
            a, vol = metrics.mesh_area_volume(v, torch.from_numpy(f))
            k = 8 * U if dtype == torch.float32 else 8 * 2.0 ** -53
            last = U if dtype == torch.float32 else 2.0 ** -53
            assert (np.abs(a.double().numpy() - want['area']) <= k * want['area_scale'] + last * want['area']).all()
            assert (np.abs(vol.double().numpy() - want['volume']) <= k * want['volume_scale'] + last * np.abs(want['volume'])).all()
            assert (want['volume'] > 0.5).all()                                         # wound outwards, radius about 0.75


def test_non_finite_vertices_propagate_and_bad_ids_contribute_nothing():
    v = _t(np.stack([CUBE_V, CUBE_V]))
    v[1, 6, 1] = float('nan')
    a, vol = metrics.mesh_area_volume(v, torch.from_numpy(CUBE_F))
    assert a[0] == 6 and vol[0] == 1 and bool(torch.isnan(a[1])) and bool(torch.isnan(vol[1]))
    f = torch.from_numpy(np.concatenate([CUBE_F, [[0, 3, -1], [8, 1, 2]]])).int()
    a, vol = metrics._mesh_area_volume_unchecked(_t(CUBE_V[None] * 1.0, grad=True), f)
    assert a.tolist() == [6.0] and vol.tolist() == [1.0]


def test_gradcheck_on_the_cube_and_the_closed_mesh_identities():
    f = torch.from_numpy(CUBE_F)
    g = torch.Generator().manual_seed(0)
    v = (_t(np.stack([CUBE_V, 2 * CUBE_V - 3]), torch.float64) + 0.05 * torch.randn(2, 8, 3, generator=g, dtype=torch.float64)).requires_grad_()
    assert torch.autograd.gradcheck(lambda x: metrics.mesh_area_volume(x, f), (v,), eps=1e-6, atol=1e-7, rtol=1e-6)
    # r = 1 ico meshes are closed: the volume does not move under a translation, and it is homogeneous of degree 3
    f = torch.from_numpy(ico_ref.faces_from_lattice(1))
    v = _t(make_goldens.synthetic_np(B, 1, seed=3) + 0.5, torch.float64, grad=True)
    vol = metrics.mesh_area_volume(v, f)[1]
    for b in range(B):
        gb = torch.autograd.grad(vol[b], v, retain_graph=True)[0]
        assert bool((gb[torch.arange(B) != b] == 0).all())                              # another mesh's volume
        assert float(gb[b].sum(0).abs().max()) <= 1e-14
        assert abs(float((gb[b] * v[b].detach()).sum()) - 3 * float(vol[b].detach())) <= 1e-13 * float(vol[b].detach())
    # the documented corner formulas, on one face: d volume = (b x c) / 6 about o, d area = n^ x (v2 - v1) / 2
    tri = torch.tensor([[[0.3, 0.1, -0.2], [1.0, 0.2, 0.1], [0.1, 1.1, 0.3], [0.2, 0.1, 0.9]]], dtype=torch.float64, requires_grad=True)
    a, vol = metrics.mesh_area_volume(tri, torch.tensor([[1, 2, 3]]))
    ga, gv = torch.autograd.grad(a.sum(), tri, retain_graph=True)[0][0], torch.autograd.grad(vol.sum(), tri)[0][0]
    p = tri.detach()[0]
    n = torch.linalg.cross(p[2] - p[1], p[3] - p[1])
    for k in range(3):
        k1, k2 = 1 + (k + 1) % 3, 1 + (k + 2) % 3
        assert torch.allclose(gv[1 + k], torch.linalg.cross(p[k1] - p[0], p[k2] - p[0]) / 6, rtol=1e-13, atol=1e-15)
        assert torch.allclose(ga[1 + k], torch.linalg.cross(n / n.norm(), p[k2] - p[k1]) / 2, rtol=1e-13, atol=1e-15)
    assert torch.equal(ga[0], torch.zeros(3, dtype=torch.float64)) and torch.equal(gv[0], torch.zeros(3, dtype=torch.float64))   # o is constant


def _check_table(f, V):
    offsets, corners = metrics.vertex_face_table(torch.as_tensor(f), V)
    assert offsets.dtype == corners.dtype == torch.int32 and offsets.shape == (V + 1,) and corners.shape == (3 * len(f),)
    offsets, corners, flat = offsets.numpy(), corners.numpy(), np.asarray(f).reshape(-1)
    valid = (flat >= 0) & (flat < V)
    assert offsets[0] == 0 and (np.diff(offsets) >= 0).all() and offsets[V] == valid.sum()
    assert sorted(corners.tolist()) == list(range(3 * len(f)))                          # every corner once
    for j in range(V):
        mine = corners[offsets[j]:offsets[j + 1]]
        assert (flat[mine] == j).all() and (np.diff(mine) > 0).all() and len(mine) == (flat == j).sum()
    assert not valid[corners[offsets[V]:]].any()
    return offsets, corners


def test_vertex_face_table():
    _check_table(CUBE_F, 8)
    offsets, _ = _check_table(DEGEN_F, 10)
    assert offsets[10] - offsets[9] == 0                                                # the unreferenced vertex: an empty slice
    for r in (0, 1, 2):
        f = ico_ref.faces_from_lattice(r)
        offsets, _ = _check_table(f, 10 * 4 ** r + 2)
        assert sorted(set(np.diff(offsets).tolist())) == [5, 6][:1 + (r > 0)]           # valences of an icosphere
        assert (geometry.get_ico_faces(r) == f).all()
    _check_table(np.concatenate([CUBE_F, [[0, 3, -1], [8, 1, 2]]]), 8)                  # ids out of range belong to no vertex
    _check_table(CUBE_F.astype(np.int32), 8)
    for bad in (torch.zeros(4, 2, dtype=torch.int64), torch.zeros(12, dtype=torch.int64), torch.zeros(4, 3)):
        with pytest.raises(ValueError):
            metrics.vertex_face_table(bad, 8)
    with pytest.raises(ValueError):
        metrics.vertex_face_table(torch.from_numpy(CUBE_F), 0)


def test_argument_checks():
    v, f = _t(CUBE_V[None]), torch.from_numpy(CUBE_F)
    table = metrics.vertex_face_table(f, 8)
    assert metrics.mesh_area_volume(v, f, table)[1].tolist() == [1.0]
    for bad in ((v[0], f), (v[:, :, :2], f), (v[:0], f), (v.long(), f), (v, f[:, :2]), (v, f[:0]), (v, f.float()), (v, f.reshape(-1)),
                (v, f, table[0]), (v, f, (table[0], table[1][:-1])), (v, f, (table[0][:-1], table[1])), (v, f, (table[0].long(), table[1]))):
        with pytest.raises(ValueError):
            metrics.mesh_area_volume(*bad)
    for bad in ((v, f + 1), (v, f - 1), (v[:, :7], f)):
        with pytest.raises(IndexError):
            metrics.mesh_area_volume(*bad)
    with pytest.raises(ValueError):
        metrics.volume_error(v, v, f)
    with pytest.raises(IndexError):
        metrics.volume_error(v[0], v[0], f + 1)


# ---- Surface_Loss on the torch path -------------------------------------------------------------------------------------------------
def test_the_loss_checks_the_factors_and_build_criterion_passes_the_keys():
    for cls in (losses.Surface_Loss, losses.SurfaceKLD_Loss):
        for name in ('factor_volume', 'factor_area'):
            for bad in (float('nan'), float('inf'), 'x', True, None):
                with pytest.raises(ValueError):
                    cls(1, **{name: bad})
        crit = cls(1)
        assert crit.factor_volume == 0.0 and crit.factor_area == 0.0 and float(crit.last_volume) == 0.0 and float(crit.last_area) == 0.0
        crit = cls(1, factor_volume=0.5, factor_area=0.25)
        assert crit.factor_volume == 0.5 and crit.factor_area == 0.25 and crit.samples == 0
        offsets, corners = _check_table(geometry.get_ico_faces(1), 42)
        assert crit.ico_vf_offsets.tolist() == offsets.tolist() and crit.ico_vf_corners.tolist() == corners.tolist()
        assert sorted(crit.state_dict()) == sorted(cls(1).state_dict()) and 'ico_vf_offsets' not in crit.state_dict()
    for kind, model in (('surface', 'ico2ico'), ('surfacekld', 'ico2ico_vae')):
        p = models.default_params(model, subdivisions=2)
        p[model]['loss'] = kind
        crit = build_criterion(p, 'cpu')
        assert crit.factor_volume == 0.0 and crit.factor_area == 0.0
        p['ico'].update(factor_volume=0.5, factor_area=0.25)
        crit = build_criterion(p, 'cpu')
        assert crit.factor_volume == 0.5 and crit.factor_area == 0.25


@pytest.mark.parametrize('samples', [0, 48])
def test_zero_factors_leave_the_loss_alone_and_a_factor_adds_its_term_exactly(samples):
    r = 1
    x, t = data.synthetic_batch(2, r, seed=5)
    kw = dict(factor_edge=0.1, factor_smooth=0.2, samples=samples, sample_seed=4)
    for dtype in (torch.float32, torch.float64):
        grid, tgt = (0.9 * x).to(dtype).requires_grad_(), t.to(dtype)
        base = losses.Surface_Loss(r, 0.7, 1.3, **kw)(grid, tgt)
        zero = losses.Surface_Loss(r, 0.7, 1.3, factor_volume=0.0, factor_area=0.0, **kw)
        loss = zero(grid, tgt)
        assert torch.equal(loss, base) and zero.last_volume == 0 and zero.last_area == 0
        assert torch.equal(torch.autograd.grad(loss, grid)[0], torch.autograd.grad(base, grid, retain_graph=True)[0])
    # float64: base + factor * l, exactly
    faces = torch.from_numpy(geometry.get_ico_faces(r))
    out, ref = losses.grid_to_vertices(grid, r), tgt[:, 0:3].transpose(1, 2).contiguous()
    (a_out, v_out), (a_ref, v_ref) = metrics.mesh_area_volume(out, faces), metrics.mesh_area_volume(ref, faces)
    l_vol, l_area = ((v_out - v_ref) ** 2).mean(), ((a_out - a_ref) ** 2).mean()
    assert float(l_vol.detach()) > 1e-3 and float(l_area.detach()) > 1e-3
    for fv, fa in ((0.5, 0.0), (0.0, 0.25), (-2.0, 0.0), (0.5, 0.25)):
        crit = losses.Surface_Loss(r, 0.7, 1.3, factor_volume=fv, factor_area=fa, **kw)
        loss = crit(grid, tgt)
        want = base
        if fv:
            want = want + fv * l_vol
        if fa:
            want = want + fa * l_area
        assert torch.equal(loss, want)
        assert torch.equal(torch.as_tensor(crit.last_volume, dtype=dtype), l_vol.detach() if fv else torch.zeros((), dtype=dtype))
        assert torch.equal(torch.as_tensor(crit.last_area, dtype=dtype), l_area.detach() if fa else torch.zeros((), dtype=dtype))
        assert rel_l2(torch.autograd.grad(loss, grid)[0].numpy(), torch.autograd.grad(want, grid, retain_graph=True)[0].numpy()) <= 1e-14
        assert len(crit.get_last_losses()) == 5 and crit.get_last_losses()[4] == float(loss.detach())
    # the terms pull a shrunken output back out: the volume gradient points along the inward normal while the output is too small
    crit = losses.Surface_Loss(r, 0.0, 0.0, factor_volume=1.0)
    g, = torch.autograd.grad(crit(grid, tgt), grid)
    assert float((g * grid.detach()).sum()) < 0


def test_the_kld_variant_passes_the_factors_through():
    r = 1
    x, t = data.synthetic_batch(2, r, seed=6)
    mu, logvar = torch.zeros(2, 4), torch.zeros(2, 4)
    plain = losses.SurfaceKLD_Loss(r)((0.9 * x, mu, logvar), t)
    crit = losses.SurfaceKLD_Loss(r, factor_volume=0.5, factor_area=0.25)
    loss = crit((0.9 * x, mu, logvar), t)
    assert float(loss.detach()) > float(plain.detach()) and float(crit.last_volume) > 0 and float(crit.last_area) > 0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
# (mesh, shift): the cube (V = 8, F = 12), r = 0 (F = 20: less than a wave), r = 2 (F = 320: the second pass of a thread's stride in
# the block of 1024 faces, partly filled), r = 3 (F = 1280: two blocks of faces, the second partly filled; V = 642: three blocks of
# vertices in the backward); each also translated by (10, 10, 10), where an origin-based triple product loses three digits
CASES = [(mesh, shift) for mesh in ('cube', 0, 2, 3) for shift in (0.0, 10.0)]


@functools.lru_cache(maxsize=None)
def _case(mesh, shift):
    """B = 3 different meshes, fp32-rounded; the float64 reference of the values; upstream gradients; per term ('area', 'volume',
    'both') the float64 autograd gradient and the rel-L2 error of the fp32 torch formulation on the CPU against it."""
    rs = np.random.RandomState(17)
    if mesh == 'cube':
        f = CUBE_F
        v = np.stack([CUBE_V, 1.5 * CUBE_V + 0.25, CUBE_V + 0.1 * rs.randn(8, 3)])
    else:
        f = ico_ref.faces_from_lattice(mesh)
        v = make_goldens.synthetic_np(B, mesh, seed=20 + mesh)
    v32 = (v + shift).astype(np.float32)
    c = dict(f=torch.from_numpy(f), v=torch.from_numpy(v32), ref=_ref64(v32.astype(np.float64), f),
             darea=torch.from_numpy(rs.randn(B).astype(np.float32)), dvolume=torch.from_numpy(rs.randn(B).astype(np.float32)))
    c['grad64'], c['e_torch'] = {}, {}
    for term in ('area', 'volume', 'both'):
        c['grad64'][term] = _grad(c, term, torch.float64, 'cpu').numpy()
        c['e_torch'][term] = rel_l2(_grad(c, term, torch.float32, 'cpu').numpy(), c['grad64'][term])
    return c


def _upstream(c, term, a, vol):
    return sum(((a * c['darea'].to(a)).sum(),) * (term != 'volume') + ((vol * c['dvolume'].to(a)).sum(),) * (term != 'area'))


def _grad(c, term, dtype, device, fn=metrics.mesh_area_volume):
    v = c['v'].clone().to(device=device, dtype=dtype).requires_grad_()
    a, vol = fn(v, c['f'].to(device))
    if device != 'cpu':
        assert isinstance(a.grad_fn, torch.autograd.function.BackwardCFunction)          # the HIP path, not the torch formulation
    return torch.autograd.grad(_upstream(c, term, a, vol), v)[0].cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('mesh,shift', CASES)
def test_hip_values_against_float64(mesh, shift):
    c = _case(mesh, shift)
    a, vol = metrics.mesh_area_volume(c['v'].cuda(), c['f'].cuda())
    assert a.dtype == vol.dtype == torch.float32 and a.shape == vol.shape == (B,) and a.is_cuda
    ref = c['ref']
    e_a, e_v = np.abs(a.double().cpu().numpy() - ref['area']), np.abs(vol.double().cpu().numpy() - ref['volume'])
    print('%s shift %g: |area - area64| / (u scale) = %s, |volume - vol64| / (u scale) = %s; in u of the value: %s, %s'
          % (mesh, shift, e_a / (U * ref['area_scale']), e_v / (U * ref['volume_scale']), e_a / (U * ref['area']), e_v / (U * np.abs(ref['volume']))))
    assert (e_a <= 8 * U * ref['area_scale'] + U * ref['area']).all()
    assert (e_v <= 8 * U * ref['volume_scale'] + U * np.abs(ref['volume'])).all()
    a2, vol2 = metrics.mesh_area_volume(c['v'].cuda(), c['f'].cuda())
    assert torch.equal(a, a2) and torch.equal(vol, vol2)                               # fixed order: bit-identical
    # every face reversed: the same area, the opposite volume
    ar, volr = metrics.mesh_area_volume(c['v'].cuda(), c['f'][:, [0, 2, 1]].cuda())
    assert (np.abs(ar.double().cpu().numpy() - ref['area']) <= 8 * U * ref['area_scale'] + U * ref['area']).all()
    assert (np.abs(volr.double().cpu().numpy() + ref['volume']) <= 8 * U * ref['volume_scale'] + U * np.abs(ref['volume'])).all()
    # one mesh of the batch alone: the same bits (a batch-stride error would show)
    a1, vol1 = metrics.mesh_area_volume(c['v'][2:3].cuda(), c['f'].cuda())
    assert torch.equal(a1, a[2:3]) and torch.equal(vol1, vol[2:3])


@pytest.mark.gpu
@pytest.mark.parametrize('mesh,shift', CASES)
def test_hip_gradients_against_float64(mesh, shift):
    c = _case(mesh, shift)
    got = {}
    for term in ('area', 'volume', 'both'):
        got[term] = _grad(c, term, torch.float32, 'cuda')
        e_hip, e_torch = rel_l2(got[term].numpy(), c['grad64'][term]), c['e_torch'][term]
        print('%s shift %g, %s: rel-L2 against float64: HIP %.3g, torch fp32 %.3g' % (mesh, shift, term, e_hip, e_torch))
        assert e_hip <= max(2 * e_torch, 1e-6)
        assert torch.equal(got[term], _grad(c, term, torch.float32, 'cuda'))             # bit-identical run to run
    # with one upstream gradient missing only the other term is computed: each single term met its own float64 gradient above,
    # and those lie far from each other and from their sum
    for one, other in (('area', 'volume'), ('area', 'both'), ('volume', 'both')):
        assert rel_l2(c['grad64'][one], c['grad64'][other]) > 0.1
    # a table the caller built gives the same bits as the one built on demand
    table = metrics.vertex_face_table(c['f'].cuda(), c['v'].shape[1])
    assert table[0].is_cuda and table[1].is_cuda
    assert torch.equal(got['both'], _grad(c, 'both', torch.float32, 'cuda', lambda v, f: metrics.mesh_area_volume(v, f, table)))


@pytest.mark.gpu
def test_hip_known_answers_degenerate_faces_and_non_finite_vertices():
    _check_known_answers(torch.float32, 'cuda')
    _check_degenerate_faces(torch.float32, 'cuda')
    v = _t(np.stack([CUBE_V, CUBE_V, CUBE_V]), device='cuda')
    v[1, 6, 1] = float('nan')
    v.requires_grad_()
    a, vol = metrics.mesh_area_volume(v, torch.from_numpy(CUBE_F).cuda())
    assert a.tolist()[::2] == [6.0, 6.0] and vol.tolist()[::2] == [1.0, 1.0] and bool(torch.isnan(a[1])) and bool(torch.isnan(vol[1]))
    g, = torch.autograd.grad(a[0] + vol[0] + a[2] + vol[2], v)
    assert bool(torch.isfinite(g[0]).all()) and torch.equal(g[0], g[2])                # the NaN stays in its own mesh


@pytest.mark.gpu
def test_hip_exact_zero_at_an_unreferenced_vertex():
    c = _case(2, 10.0)
    v = torch.cat([c['v'], torch.full((B, 1, 3), 3.0)], dim=1).cuda().requires_grad_()   # vertex V: no face references it
    a, vol = metrics.mesh_area_volume(v, c['f'].cuda())
    g, = torch.autograd.grad(_upstream(c, 'both', a, vol), v)
    assert torch.equal(g[:, -1], torch.zeros_like(g[:, -1])) and bool((g[:, :-1].abs().sum(-1) > 0).all())
    assert torch.equal(g[:, :-1].cpu(), _grad(c, 'both', torch.float32, 'cuda'))


@pytest.mark.gpu
def test_batch_slices_give_the_bits_of_one_launch(monkeypatch):
    """B = 5 icospheres of one subdivision (V = 42, F = 80) in slices of 2 -- a full slice, a second full one at a non-zero offset and
    a remainder -- against the one-launch result: the forward, and a backward in which only the volume is differentiated, so that the
    darea upstream is null."""
    f = torch.from_numpy(ico_ref.faces_from_lattice(1)).cuda()
    v = torch.from_numpy(make_goldens.synthetic_np(5, 1, seed=31).astype(np.float32)).cuda()
    assert v.shape == (5, 42, 3) and f.shape == (80, 3)
    dvolume = torch.tensor([0.5, -1.25, 2.0, 0.75, -3.0], device='cuda')

    def run():
        x = v.clone().requires_grad_()
        a, vol = metrics.mesh_area_volume(x, f)
        g, = torch.autograd.grad((vol * dvolume).sum(), x)
        return a.detach(), vol.detach(), g
    assert metrics._MAX_GRID_Y == 65535
    want = run()
    assert len(set(want[0].tolist())) == len(set(want[1].tolist())) == 5 and bool((want[2].abs().sum((1, 2)) > 0).all())    # five different meshes
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 2)
    assert list(metrics._batch_slices(5)) == [(0, 2), (2, 2), (4, 1)]
    for one_launch, sliced in zip(want, run()):
        assert torch.equal(one_launch, sliced)


def _unchecked(v, f32, term_weights, table=None):
    v = v.detach().clone().requires_grad_()
    a, vol = metrics._mesh_area_volume_unchecked(v, f32, table)
    g, = torch.autograd.grad((a * term_weights[0]).sum() + (vol * term_weights[1]).sum(), v)
    return a.detach(), vol.detach(), g


@pytest.mark.gpu
def test_hip_defined_behaviour_on_bad_tables():
    """A face with a vertex id of -1 or V contributes nothing; a corners entry of -1 or 3 F is skipped; offsets beyond 3 F are
    clamped.  Each against the same mesh without that face, bit for bit (the face is the last one: the order of the rest stays)."""
    c = _case('cube', 0.0)
    v, V = c['v'].cuda(), 8
    w = (c['darea'].cuda(), c['dvolume'].cuda())
    clean = c['f'].int().cuda()
    a0, vol0, g0 = _unchecked(v, clean, w)
    for bad_face in ([0, 3, -1], [V, 1, 2], [-1, -1, -1], [1, V + 100, 2]):
        f32 = torch.cat([clean, torch.tensor([bad_face], dtype=torch.int32, device='cuda')])
        for table in (None, metrics.vertex_face_table(f32, V)):
            a, vol, g = _unchecked(v, f32, w, table)
            assert torch.equal(a, a0) and torch.equal(vol, vol0) and torch.equal(g, g0), bad_face
    # the corners of the last face struck from the table: the gradient of the mesh without that face
    F = clean.shape[0]
    _, _, g_less = _unchecked(v, clean[:-1].contiguous(), w)
    offsets, corners = metrics.vertex_face_table(clean, V)
    for strike in (-1, 3 * F, 3 * F + 7, -2 ** 31):
        struck = torch.where(corners >= 3 * (F - 1), torch.full_like(corners, strike), corners)
        assert int((struck != corners).sum()) == 3
        _, _, g = _unchecked(v, clean, w, (offsets, struck))
        assert torch.equal(g, g_less), strike
    # a corner filed under the wrong vertex is not used either: faces[c] == j is checked
    swapped = corners.clone()
    swapped[[int(offsets[1]), int(offsets[2])]] = swapped[[int(offsets[2]), int(offsets[1])]]
    _, _, g = _unchecked(v, clean, w, (offsets, swapped))
    assert bool(torch.isfinite(g).all()) and torch.equal(g[:, 3:], g0[:, 3:]) and not torch.equal(g[:, 1:3], g0[:, 1:3])
    # offsets out of range are clamped into [0, 3 F]: in a correct table only the two ends can be pushed out without changing a slice
    wild = offsets.clone()
    wild[0], wild[V] = -5, 3 * F + 1000
    _, _, g = _unchecked(v, clean, w, (wild, corners))
    assert torch.equal(g, g0)


@pytest.mark.gpu
def test_no_host_synchronisation_in_the_loss_terms_and_the_unchecked_call():
    r = 2
    x, t = data.synthetic_batch(2, r, seed=7, device='cuda')
    crit = losses.Surface_Loss(r, 1.0, 1.0, search='grid', factor_volume=0.5, factor_area=0.25).cuda()
    f32 = crit.ico_faces

    def both():
        grid = (0.8 * x).requires_grad_()
        loss = crit(grid, t)
        loss.backward()
        v = losses.grid_to_vertices(0.8 * x, r).requires_grad_()
        a, vol = metrics._mesh_area_volume_unchecked(v, f32)                           # no table: built in the backward
        (a.sum() + vol.sum()).backward()
        return loss.detach(), grid.grad, v.grad
    both()                                                                              # workspaces and the allocator settle
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
    assert float(crit.last_volume) > 0 and float(crit.last_area) > 0


@pytest.mark.gpu
def test_torch_fallback_on_the_device(monkeypatch):
    c = _case(2, 0.0)
    hip = metrics.mesh_area_volume(c['v'].cuda(), c['f'].cuda())
    monkeypatch.setattr(losses, '_NO_HIP_LOSS', True)                                 # what ICN_NO_HIP_LOSS=1 sets at import
    v = c['v'].cuda().requires_grad_()
    a, vol = metrics.mesh_area_volume(v, c['f'].cuda())
    assert not isinstance(a.grad_fn, torch.autograd.function.BackwardCFunction)
    assert float(((a.detach() - hip[0]) / hip[0]).abs().max()) <= 16 * U and float(((vol.detach() - hip[1]) / hip[1]).abs().max()) <= 16 * U


@pytest.mark.gpu
def test_surface_loss_terms_on_the_device():
    """r = 2, B = 2: the two terms alone (the distances switched off, so that nothing else decides the figures) against the CPU
    float64 evaluation of the same module, at twice the error of the module in fp32 on the CPU, floor 1e-6; with both factors 0 the
    loss and its gradient are, bit for bit, those of a module built without the keywords."""
    r = 2
    x, t = data.synthetic_batch(2, r, seed=7)
    x = 0.8 * x

    def run(crit, dtype, device):
        grid = x.clone().to(device=device, dtype=dtype).requires_grad_()
        loss = crit.to(device)(grid, t.to(device=device, dtype=dtype))
        g, = torch.autograd.grad(loss, grid)
        return loss.detach().cpu(), g.cpu(), crit

    make = lambda: losses.Surface_Loss(r, 0.0, 0.0, factor_volume=0.5, factor_area=0.25)   # noqa: E731
    l64, g64, _ = run(make(), torch.float64, 'cpu')
    l32, g32, _ = run(make(), torch.float32, 'cpu')
    lhip, ghip, crit = run(make(), torch.float32, 'cuda')
    assert crit.last_volume.is_cuda and crit.last_area.is_cuda and float(l64) > 1e-2
    for name, e_hip, e_torch in (('loss', abs(float(lhip) - float(l64)) / float(l64), abs(float(l32) - float(l64)) / float(l64)),
                                 ('gradient', rel_l2(ghip.numpy(), g64.numpy()), rel_l2(g32.numpy(), g64.numpy()))):
        print('Surface_Loss volume + area, %s: relative error against float64: HIP %.3g, torch fp32 %.3g' % (name, e_hip, e_torch))
        assert e_hip <= max(2 * e_torch, 1e-6)
    want = 0.5 * float(crit.last_volume) + 0.25 * float(crit.last_area)
    assert abs(float(lhip) - want) <= 4 * U * want
    # beside the other terms, and with the factors at 0
    kw = dict(factor_edge=0.1, factor_smooth=0.2, search='grid', samples=64, sample_seed=3)
    l_plain, g_plain, _ = run(losses.Surface_Loss(r, 0.7, 1.3, **kw), torch.float32, 'cuda')
    l_zero, g_zero, zero = run(losses.Surface_Loss(r, 0.7, 1.3, factor_volume=0.0, factor_area=0.0, **kw), torch.float32, 'cuda')
    assert torch.equal(l_zero, l_plain) and torch.equal(g_zero, g_plain) and zero.last_volume == 0 and zero.last_area == 0
    l_full, g_full, full = run(losses.Surface_Loss(r, 0.7, 1.3, factor_volume=0.5, factor_area=0.25, **kw), torch.float32, 'cuda')
    assert abs(float(l_full) - float(l_plain) - want) <= 8 * U * float(l_full)
    assert rel_l2((g_full - g_plain).numpy(), ghip.numpy()) <= 1e-4 and len(full.get_last_losses()) == 5
