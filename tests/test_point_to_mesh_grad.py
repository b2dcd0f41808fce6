"""Gradient of the point-to-mesh distance (icn_point_to_mesh_bwd, metrics._PointToMeshFn) and the surface loss built on it
(losses.Point2Mesh_Loss).

Reference for every gradient: torch autograd through metrics._torch_point_to_mesh in float64 on the CPU (masked selects, not the
kernel's branch ladder; it differentiates through the weights of the closest point, the kernel uses the closed form).  Bar: 1e-4
relative L2 over the whole tensor (the project's operator bar), never per point: close to the surface p - q is at cancellation
level.

Where two DIFFERENT closest points are equally near, the gradient is discontinuous and fp32 may legitimately choose the other
one.  Such points are found from the float64 reference alone, before any GPU result exists (`_ambiguous`): some face within a
relative 1e-4 (+ 1e-12 scale^2) of the minimum whose closest point lies more than 1e-6 scale from the minimiser's.  They get
upstream weight 0 on both sides; at most 3 % of a case's points may be ambiguous (asserted).  Faces that share the winning
edge / vertex have the same closest point and do not count.
"""
import ctypes

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, geometry, metrics

CASES = ((11, 700, 2), (12, 1000, 1), (13, 1500, 3))          # (seed, points, subdivisions)
BAR = 1e-4
AMBIGUOUS_CAP = 0.03


def _case(seed, P=200, r=1):
    """The bumpy icosphere and point cloud of tests/test_metrics.py::_case: 60 points exactly on vertices, edges and faces."""
    g = np.random.default_rng(seed)
    v, f = geometry.get_icosahedral_grid(r)
    v = v * (1 + 0.2 * g.standard_normal((len(v), 1)))
    pts = g.standard_normal((P, 3)) * 0.8
    pts[:20] = v[:20]
    pts[20:40] = 0.5 * (v[f[:20, 0]] + v[f[:20, 1]])
    pts[40:60] = (v[f[:20, 0]] + v[f[:20, 1]] + v[f[:20, 2]]) / 3
    return pts.astype(np.float32), v.astype(np.float32), f


def _batch(seed, P, r):
    """Batch of 2, the second mesh scaled by 1.1: (points (2, P, 3), vertices (2, V, 3), faces (F, 3)) fp32 / int64 tensors."""
    pts, v, f = _case(seed, P, r)
    tp, tv = torch.from_numpy(pts)[None].repeat(2, 1, 1), torch.from_numpy(v)[None].repeat(2, 1, 1)
    tv[1] *= 1.1
    return tp, tv, torch.from_numpy(f)


def _closest_points(p, a, b, c):
    """float64 closest point of every triangle (a, b, c) (F, 3) to every point p (n, 3) -> (d2 (n, F), q (n, F, 3)), by the method
    of oracle/metrics_ref.py (foot of the plane projection if inside, else the nearest of the three clamped edge projections)."""
    p = p[:, None, :]
    a, b, c = a[None], b[None], c[None]
    nrm = np.cross(b - a, c - a)
    nn = (nrm * nrm).sum(-1)
    ok = nn > 0
    ns = np.where(ok[..., None], nrm, 1.0)
    foot = p - (((p - a) * ns).sum(-1) / np.where(ok, nn, 1.0))[..., None] * ns
    inside = np.broadcast_to(ok, foot.shape[:2]).copy()
    for u, w in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(w - u, foot - u) * ns).sum(-1) >= 0
    best_q, best_d = foot, np.where(inside, ((p - foot) ** 2).sum(-1), np.inf)
    for u, w in ((a, b), (b, c), (c, a)):
        uw = w - u
        den = (uw * uw).sum(-1)
        t = np.clip(((p - u) * uw).sum(-1) / np.where(den > 0, den, 1.0), 0.0, 1.0)
        q = u + uw * t[..., None]
        d = ((p - q) ** 2).sum(-1)
        take = d < best_d
        best_q, best_d = np.where(take[..., None], q, best_q), np.where(take, d, best_d)
    return best_d, best_q


def _ambiguous(points, vertices, faces):
    """(B, P) bool from float64 alone: a second, DIFFERENT closest point is as near as the nearest one (module docstring)."""
    pts, vts, f = points.double().numpy(), vertices.double().numpy(), faces.numpy()
    out = np.zeros(pts.shape[:2], dtype=bool)
    for bi in range(pts.shape[0]):
        scale = np.abs(vts[bi]).max()
        a, b, c = (vts[bi][f[:, k]] for k in range(3))
        for lo in range(0, pts.shape[1], 128):
            d2, q = _closest_points(pts[bi, lo:lo + 128], a, b, c)
            j = d2.argmin(1)
            rows = np.arange(len(j))
            dmin, qmin = d2[rows, j], q[rows, j]
            near = d2 <= (dmin * (1 + 1e-4) + 1e-12 * scale * scale)[:, None]
            apart = np.linalg.norm(q - qmin[:, None, :], axis=-1) > 1e-6 * scale
            out[bi, lo:lo + 128] = (near & apart).any(1)
    return torch.from_numpy(out)


def _weights(seed, points, vertices, faces):
    """Upstream weights in [0.5, 1.5], 0 at the ambiguous points; also the ambiguous share."""
    amb = _ambiguous(points, vertices, faces)
    g = torch.Generator().manual_seed(seed)
    w = (torch.rand(points.shape[:2], generator=g, dtype=torch.float64) + 0.5) * (~amb)
    return w, float(amb.double().mean())


def _reference_grads(points, vertices, faces, w):
    """float64 CPU autograd through the torch formulation: d sum(w dist) / d (points, vertices)."""
    p = points.double().requires_grad_(True)
    v = vertices.double().requires_grad_(True)
    d, _, _ = metrics._torch_point_to_mesh(p, v, faces)
    (d * w).sum().backward()
    return p.grad, v.grad


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _gpu_grads(fn, points, vertices, faces, w, want_points=True, want_vertices=True):
    p = points.cuda().requires_grad_(want_points)
    v = vertices.cuda().requires_grad_(want_vertices)
    d, face, kind = fn(p, v, faces.cuda())
    (d * w.float().cuda()).sum().backward()
    return d, face, kind, p.grad, v.grad


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_bound_and_versioned():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('icn_point_to_mesh_bwd', 'icn_point_to_mesh_bwd_workspace_bytes'):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION >= 8 and _lib.lib().icn_abi_version() == _lib.ABI_VERSION


def test_point_to_mesh_bwd_rejects_bad_arguments_before_touching_a_device():
    """Null pointers, bad sizes and a missing / short / misaligned workspace are refused with a message; nothing here reaches a
    kernel launch (the machine that runs this has no device)."""
    L = _lib.lib()
    x = 0x1000                                                   # never dereferenced on the host
    need = L.icn_point_to_mesh_bwd_workspace_bytes(2, 100, 50, 96)

    def call(points=x, vertices=x, faces=x, face=x, kind=x, ddist=x, B=2, P=100, V=50, F=96, dp=x, dv=x, ws=x, nbytes=need):
        return L.icn_point_to_mesh_bwd(points, vertices, faces, face, kind, ddist, B, P, V, F, dp, dv, ws, nbytes, None)
    for name in ('points', 'vertices', 'faces', 'face', 'kind', 'ddist'):
        assert call(**{name: None}) != 0 and b'null pointer' in L.icn_last_error(), name
    for bad in (dict(B=0), dict(B=65536), dict(P=0), dict(V=0), dict(F=0), dict(P=-3)):
        assert call(**bad) != 0 and b'bad sizes' in L.icn_last_error(), bad
    assert call(ws=None) != 0 and b'workspace' in L.icn_last_error()
    assert call(nbytes=need - 1) != 0 and b'workspace' in L.icn_last_error()
    assert call(ws=x + 4) != 0 and b'aligned' in L.icn_last_error()
    assert call(dp=None, dv=None, ws=None, nbytes=0) == 0         # no gradient asked for: nothing to launch


def test_point_to_mesh_bwd_workspace_query_is_host_only_and_monotonic_in_points():
    L = _lib.lib()
    q = L.icn_point_to_mesh_bwd_workspace_bytes
    assert q(0, 100, 50, 96) == 0 and q(2, 0, 50, 96) == 0 and q(2, 100, 0, 96) == 0 and q(2, 100, 50, 0) == 0 and q(65536, 1, 1, 1) == 0
    sizes = [q(4, P, 10242, 20480) for P in (1, 255, 256, 257, 1000, 10242, 50000)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert q(36, 10242, 10242, 20480) < 64 << 20                   # I5 / batch 36: a few tens of bytes per point
    assert q(8, 1000, 10, 10) >= q(4, 1000, 10, 10)


@pytest.mark.parametrize('seed,P,r', CASES)
def test_ambiguous_share_of_the_cases_is_below_the_cap(seed, P, r):
    tp, tv, tf = _batch(seed, P, r)
    _, share = _weights(seed, tp, tv, tf)
    print('case (%d, %d, %d): ambiguous share %.4f' % (seed, P, r, share))
    assert share <= AMBIGUOUS_CAP
    # the 60 points placed on the mesh itself: distance 0, gradient 0 whichever incident face wins
    gp, gv = _reference_grads(tp[:, :60], tv, tf, torch.ones(2, 60, dtype=torch.float64))
    assert float(gp[0].abs().max()) < 1e-6 and float(gv[0].abs().max()) < 1e-6


@pytest.mark.parametrize('seed,P,r', CASES)
def test_cpu_fp32_gradients_meet_the_bar_against_float64(seed, P, r):
    tp, tv, tf = _batch(seed, P, r)
    w, _ = _weights(seed, tp, tv, tf)
    want_p, want_v = _reference_grads(tp, tv, tf, w)
    p, v = tp.clone().requires_grad_(True), tv.clone().requires_grad_(True)
    d, face, kind = metrics.point_to_mesh_distance(p, v, tf)
    assert d.requires_grad and not face.requires_grad and not kind.requires_grad
    (d * w.float()).sum().backward()
    e_p, e_v = _rel(p.grad, want_p), _rel(v.grad, want_v)
    print('case (%d, %d, %d): cpu fp32 dpoints %.3g dvertices %.3g' % (seed, P, r, e_p, e_v))
    assert e_p <= BAR and e_v <= BAR


def test_point2mesh_loss_on_the_cpu_is_the_mean_of_compute_distance():
    from geniconet_amd import data
    from geniconet_amd.losses import Point2Mesh_Loss, grid_to_vertices
    R = 2
    x, _ = data.synthetic_batch(3, R, seed=5)
    _, v, f = _case(21, 60, R)
    rv = torch.from_numpy(v)[None].repeat(3, 1, 1) * torch.tensor([0.7, 0.8, 0.9])[:, None, None]
    crit = Point2Mesh_Loss(R)
    x.requires_grad_(True)
    loss = crit(x, rv, torch.from_numpy(f))
    loss.backward()
    want = np.mean([metrics.compute_distance(grid_to_vertices(x.detach(), R)[b], rv[b], torch.from_numpy(f)) for b in range(3)])
    assert float(loss.detach()) == pytest.approx(want, rel=1e-5)
    assert crit.get_last_losses() == (float(loss.detach()), 0, 0, float(loss.detach()))
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    with pytest.raises(ValueError):
        crit(x[:, :, :-1], rv, torch.from_numpy(f))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('seed,P,r', CASES)
def test_hip_gradients_match_float64_autograd(seed, P, r):
    tp, tv, tf = _batch(seed, P, r)
    w, share = _weights(seed, tp, tv, tf)                           # decided before any GPU result exists
    assert share <= AMBIGUOUS_CAP
    want_p, want_v = _reference_grads(tp, tv, tf, w)
    d, face, kind, gp, gv = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w)
    assert d.is_cuda and d.requires_grad and d.grad_fn is not None
    assert not face.requires_grad and not kind.requires_grad and face.dtype == torch.int64 and kind.dtype == torch.int32
    d0, face0, kind0 = metrics.point_to_mesh_distance(tp.cuda(), tv.cuda(), tf.cuda())
    assert not d0.requires_grad
    assert torch.equal(d.detach(), d0) and torch.equal(face, face0) and torch.equal(kind, kind0)
    with torch.no_grad():                                           # gradient tracking off: today's path even for such inputs
        d1, _, _ = metrics.point_to_mesh_distance(tp.cuda().requires_grad_(True), tv.cuda(), tf.cuda())
    assert not d1.requires_grad and torch.equal(d1, d0)
    e_p, e_v = _rel(gp, want_p), _rel(gv, want_v)
    print('case (%d, %d, %d): ambiguous %.4f, hip dpoints %.3g dvertices %.3g' % (seed, P, r, share, e_p, e_v))
    assert e_p <= BAR and e_v <= BAR
    # the points on the first mesh itself: p - q is a handful of fp32 roundings (6e-8) of coordinates below 2, times 2 w <= 3
    assert float(gp[0, :60].abs().max()) < 1e-5


@pytest.mark.gpu
def test_single_gradient_requests_equal_the_joint_run_bit_for_bit():
    for seed, P, r in CASES:
        tp, tv, tf = _batch(seed, P, r)
        w, _ = _weights(seed, tp, tv, tf)
        _, _, _, gp, gv = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w)
        _, _, _, gp1, none_v = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w, want_vertices=False)
        _, _, _, none_p, gv1 = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w, want_points=False)
        assert none_v is None and none_p is None
        assert torch.equal(gp1, gp) and torch.equal(gv1, gv)


@pytest.mark.gpu
def test_batch_slicing_of_the_launch_limit_applies_to_the_backward(monkeypatch):
    """The batch index is gridDim.y (<= 65535 per launch); with the limit lowered to 1 the two samples go through two launches of
    the forward and of the backward each, and nothing may change."""
    seed, P, r = CASES[0]
    tp, tv, tf = _batch(seed, P, r)
    w, _ = _weights(seed, tp, tv, tf)
    d, face, kind, gp, gv = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w)
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 1)
    d1, face1, kind1, gp1, gv1 = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w)
    assert torch.equal(d1.detach(), d.detach()) and torch.equal(face1, face) and torch.equal(kind1, kind)
    assert torch.equal(gp1, gp) and torch.equal(gv1, gv)


@pytest.mark.gpu
def test_backward_is_bit_deterministic_at_the_small_cases():
    for seed, P, r in CASES:
        tp, tv, tf = _batch(seed, P, r)
        w, _ = _weights(seed, tp, tv, tf)
        runs = [_gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w)[3:] for _ in range(2)]
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
        # a vertex that is on no selected face gets an exact zero
        _, face, kind, _, gv = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w)
        used = torch.zeros(tv.shape[:2], dtype=torch.bool)
        for b in range(2):
            used[b, tf[face[b].cpu()].reshape(-1)] = True
        assert bool((gv.cpu()[~used] == 0).all())


@pytest.mark.gpu
def test_full_size_backward_is_deterministic_zero_on_itself_and_balanced_on_a_shifted_copy():
    """I5: 10242 points, 20480 faces, batch 4, upstream of ones.  A mesh against itself: all-zero gradients.  Against a copy moved
    by eps along x: |dpoints| <= 2 eps per point, and since the weights of every point sum to 1 the two gradients balance:
    dvertices.sum(1) = -dpoints.sum(1) per sample."""
    from geniconet_amd import data
    from geniconet_amd.losses import grid_to_vertices
    R = 5
    x, _ = data.synthetic_batch(4, R, seed=2, device='cuda')
    v = grid_to_vertices(x, R)
    f = torch.from_numpy(geometry.get_ico_faces(R)).cuda()

    def grads(points):
        p, m = points.clone().requires_grad_(True), v.clone().requires_grad_(True)
        d, _, _ = metrics.point_to_mesh_distance(p, m, f)
        d.sum().backward()
        return p.grad, m.grad
    gp, gv = grads(v)
    assert float(gp.abs().max()) == 0 and float(gv.abs().max()) == 0
    eps = 1e-2
    shifted = v.clone()
    shifted[..., 0] += eps
    gp, gv = grads(shifted)
    gp2, gv2 = grads(shifted)
    assert torch.equal(gp, gp2) and torch.equal(gv, gv2)
    assert bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gv).all())
    assert float(gp.norm(dim=2).max()) <= 2 * eps * (1 + 1e-4) and float(gp.norm(dim=2).max()) > 0
    sp, sv = gp.double().sum(1), gv.double().sum(1)                 # (4, 3)
    balance = ((sv + sp).norm(dim=1) / sp.norm(dim=1)).cpu()
    print('full size: |sum dvertices + sum dpoints| / |sum dpoints| per sample', balance.tolist())
    assert bool((balance <= 1e-4).all())


def _unambiguous_grid(crit_r, ref_v, ref_f, seed, batch):
    """A (B, 3, 5n, 2n) fp32 input none of whose vertices (pixels and pole means) is ambiguous against the reference mesh: drawn,
    then the pixels behind ambiguous vertices are redrawn -- decided on the float64 reference alone.  Returns it with the share of
    ambiguous vertices of the first draw."""
    from geniconet_amd.losses import grid_to_vertices
    n = 2 ** crit_r
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, 3, 5 * n, 2 * n, generator=g) * 0.6
    corners = [[(c * n) * 2 * n for c in range(5)], [((c + 1) * n - 1) * 2 * n + 2 * n - 1 for c in range(5)]]
    first = None
    for _ in range(30):
        amb = _ambiguous(grid_to_vertices(x, crit_r), ref_v, ref_f)                  # (B, P + 2)
        first = float(amb.double().mean()) if first is None else first
        if not bool(amb.any()):
            return x, first
        redo = amb[:, :-2].clone()
        for k in range(2):
            redo[:, corners[k]] |= amb[:, -2 + k][:, None]
        fresh = torch.randn(batch, 3, 5 * n, 2 * n, generator=g) * 0.6
        x = torch.where(redo.view(batch, 1, 5 * n, 2 * n), fresh, x)
    raise AssertionError('no unambiguous input found')


@pytest.mark.gpu
def test_point2mesh_loss_value_and_input_gradient():
    from geniconet_amd.losses import Point2Mesh_Loss, grid_to_vertices
    R, B = 2, 3
    _, v, f = _case(31, 60, R)
    ref_v = torch.from_numpy(v)[None].repeat(B, 1, 1) * torch.tensor([0.8, 0.9, 1.0])[:, None, None]
    ref_f = torch.from_numpy(f)
    x, share = _unambiguous_grid(R, ref_v, ref_f, seed=32, batch=B)
    assert share <= AMBIGUOUS_CAP
    crit = Point2Mesh_Loss(R)
    x64 = x.double().requires_grad_(True)
    crit(x64, ref_v.double(), ref_f).backward()                       # float64 CPU evaluation of the same module
    xg = x.cuda().requires_grad_(True)
    loss = crit(xg, ref_v.cuda(), ref_f.cuda())
    assert loss.is_cuda and loss.dim() == 0
    loss.backward()
    verts = grid_to_vertices(x.cuda(), R)
    want = np.mean([metrics.compute_distance(verts[b], ref_v[b].cuda(), ref_f.cuda()) for b in range(B)])
    assert float(loss.detach()) == pytest.approx(want, rel=1e-5)
    assert crit.get_last_losses()[0] == pytest.approx(want, rel=1e-5)
    e = _rel(xg.grad, x64.grad)
    print('Point2Mesh_Loss: first-draw ambiguous share %.4f, input gradient rel-L2 %.3g' % (share, e))
    assert e <= BAR
    # pole means: each of the five corner pixels carries a fifth of its pole's gradient on top of its own
    n = 2 ** R
    gref = x64.grad.reshape(B, 3, -1)
    assert float(gref[:, :, [c * n * 2 * n for c in range(5)]].abs().min()) > 0


@pytest.mark.gpu
def test_the_kaolin_shim_is_the_differentiable_function():
    import geniconet_amd.shims.kaolin.metrics.trianglemesh as trianglemesh
    seed, P, r = CASES[0]
    tp, tv, tf = _batch(seed, P, r)
    w, _ = _weights(seed, tp, tv, tf)
    want_p, want_v = _reference_grads(tp, tv, tf, w)
    d, _, _, gp, gv = _gpu_grads(trianglemesh.point_to_mesh_distance, tp, tv, tf, w)
    assert d.requires_grad
    assert _rel(gp, want_p) <= BAR and _rel(gv, want_v) <= BAR
    _, _, _, gp1, gv1 = _gpu_grads(metrics.point_to_mesh_distance, tp, tv, tf, w)
    assert torch.equal(gp, gp1) and torch.equal(gv, gv1)


@pytest.mark.gpu
def test_vertex_gradient_has_the_sign_of_minus_the_point_gradient_exactly_on_dyadic_inputs():
    """One triangle, 257 points (two tiles of records) at (-i / 8, -j / 8, k / 8), all closest to vertex 0 (kind 1, weight exactly 1),
    upstream multiples of 1 / 4: every product and sum is exact in fp32, so dpoints = 2 ddist (p - a) and dvertices[0] =
    -2 sum ddist (p - a) hold with equality, and the other two vertices get an exact 0."""
    n = torch.arange(257)
    pts = torch.stack([-(n % 8) / 8.0, -((n // 8) % 8) / 8.0, (n // 64) / 8.0], 1).float()[None]
    vts = torch.tensor([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
    ddist = (((n % 7) - 2) / 4.0).float()[None]
    p, v = pts.cuda().requires_grad_(), vts.cuda().requires_grad_()
    d, face, kind = metrics.point_to_mesh_distance(p, v, torch.tensor([[0, 1, 2]]).cuda())
    assert bool((kind == 1).all()) and bool((face == 0).all())
    d.backward(ddist.cuda())
    want_p = 2 * ddist.double()[..., None] * pts.double()
    assert torch.equal(p.grad.double().cpu(), want_p)
    assert torch.equal(v.grad.double().cpu()[0, 0], -want_p[0].sum(0)) and bool((v.grad.cpu()[0, 1:] == 0).all())
    assert bool((v.grad.cpu()[0, 0] != 0).all())
