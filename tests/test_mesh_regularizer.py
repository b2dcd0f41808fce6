"""Mesh regularisers of the surface loss (losses.Mesh_Regularizer, icn_mesh_reg_* / icn_table_vertex_stencils in include/icn.h):
the edge stencil table against the face list, the torch formulation against an independent restatement and known answers, the
argument checks of the C ABI (all without a GPU), and the HIP kernels against the float64 torch formulation (gpu)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, data, geometry, losses

from conftest import rel_l2


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def _bumpy_vertices(r, B, seed=0):
    """(B, V, 3) float64: the unit icosphere times 1 + 0.2 N(0, 1) per vertex (the mesh of tests/test_metrics.py::_case)."""
    g = np.random.default_rng(seed)
    v, _ = geometry.get_icosahedral_grid(r)
    return torch.from_numpy(np.stack([v * (1 + 0.2 * g.standard_normal((len(v), 1))) for _ in range(B)]))


def _grid_case(r, B, mesh):
    """fp32 network-output-shaped grid (B, 3, 5n, 2n) of a 'bumpy' or 'smooth' mesh (the poles are the corner means)."""
    n = 2 ** r
    if mesh == 'smooth':
        return data.synthetic_batch(B, r, seed=5)[0].contiguous()
    v = _bumpy_vertices(r, B, seed=10 * r + B)
    return v[:, :-2].transpose(1, 2).reshape(B, 3, 5 * n, 2 * n).float().contiguous()


def _mean_edge_length(r, grid):
    f = geometry.get_ico_faces(r)
    v = losses.grid_to_vertices(grid.double(), r)
    return float((v[:, f[:, 0]] - v[:, f[:, 1]]).norm(dim=2).mean())


# ---- the restatement: explicit edge list and face pairs from the faces, with a dict ------------------------------------------
@functools.lru_cache(maxsize=None)
def _topology(r):
    faces = geometry.get_ico_faces(r)
    edge_faces, ring = {}, {}
    for fi, (a, b, c) in enumerate(faces.tolist()):
        for i, j in ((a, b), (b, c), (c, a)):
            edge_faces.setdefault((min(i, j), max(i, j)), []).append(fi)
            ring.setdefault(i, set()).add(j)
            ring.setdefault(j, set()).add(i)
    edges = sorted(edge_faces)
    assert all(len(edge_faces[e]) == 2 for e in edges)
    pairs = [edge_faces[e] for e in edges]
    return faces, torch.tensor(edges), torch.tensor(pairs), [sorted(ring[i]) for i in range(len(ring))]


def _restated_terms(v, r, L):
    """(T_e, T_n, T_s) of vertices (B, V, 3) from the definitions, on non-degenerate meshes (no clamp is active)."""
    faces, edges, pairs, ring = _topology(r)
    B, V = v.shape[:2]
    length2 = ((v[:, edges[:, 0]] - v[:, edges[:, 1]]) ** 2).sum(-1)
    t_e = ((length2.sqrt() - L) ** 2).sum() / (B * len(edges)) if L > 0 else length2.sum() / (B * len(edges))
    f = torch.from_numpy(faces)
    nrm = torch.cross(v[:, f[:, 1]] - v[:, f[:, 0]], v[:, f[:, 2]] - v[:, f[:, 0]], dim=2)
    nrm = nrm / nrm.norm(dim=2, keepdim=True).clamp_min(1e-12)
    t_n = (0.5 * ((nrm[:, pairs[:, 0]] - nrm[:, pairs[:, 1]]) ** 2).sum(-1)).sum() / (B * len(edges))
    mean_ring = torch.stack([v[:, ring[i]].mean(1) for i in range(V)], dim=1)
    t_s = ((mean_ring - v) ** 2).sum() / (3 * B * V)
    return t_e, t_n, t_s


# ---- 1. the stencil table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [0, 1, 2, 3, 4])
def test_stencil_table_against_the_faces(r):
    faces = geometry.get_ico_faces(r)
    vs = _lib.table_vertex_stencils(r)
    V = geometry.num_vertices(r)
    assert vs.shape == (V, 6, 3) and vs.dtype == np.int32
    oriented = set()
    for a, b, c in faces.tolist():
        oriented.update(((a, b, c), (b, c, a), (c, a, b)))
    valence = (vs[:, :, 0] >= 0).sum(1)
    assert sorted(set(valence.tolist())) in ([5], [5, 6]) and int((valence == 5).sum()) == 12
    seen_faces, seen_edges = {}, {}
    for i in range(V):
        k = int(valence[i])
        assert (vs[i, :k] >= 0).all() and (vs[i, k:] == -1).all()             # filled slots first, -1 padding after
        for f in range(k):
            p, q, x = (int(t) for t in vs[i, f])
            assert (i, p, q) in oriented                                        # a face, in its orientation, i first
            assert q == int(vs[i, (f + 1) % k, 0])                              # cyclic: q of slot f is p of slot f + 1
            assert (q, p, x) in oriented and x != i                             # the face across (p, q)
            key = tuple(sorted((i, p, q)))
            seen_faces[key] = seen_faces.get(key, 0) + 1
            e = (min(i, p), max(i, p))
            seen_edges[e] = seen_edges.get(e, 0) + 1
    assert len(seen_faces) == len(faces) == 20 * 4 ** r and set(seen_faces.values()) == {3}
    assert len(seen_edges) == 30 * 4 ** r and set(seen_edges.values()) == {2}


# ---- 2. torch formulation vs the restatement ------------------------------------------------------------------------------
@pytest.mark.parametrize('r', [1, 2])
@pytest.mark.parametrize('with_length', [False, True])
def test_torch_formulation_matches_the_restatement_in_float64(r, with_length):
    grid = _grid_case(r, 2, 'bumpy').double()
    L = _mean_edge_length(r, grid) if with_length else 0.0
    reg = losses.Mesh_Regularizer(r, 1.0, 1.0, 1.0, edge_length=L)
    g1, g2 = grid.clone().requires_grad_(), grid.clone().requires_grad_()
    got = reg.terms(losses.grid_to_vertices(g1, r))
    want = _restated_terms(losses.grid_to_vertices(g2, r), r, L)
    values = [float(w.detach()) for w in want]
    for k, name in enumerate(('edge', 'ncons', 'smooth')):
        assert abs(float(got[k].detach()) - values[k]) <= 1e-10 * abs(values[k]), name
        da, = torch.autograd.grad(got[k], g1, retain_graph=True)
        db, = torch.autograd.grad(want[k], g2, retain_graph=True)
        assert rel_l2(da.numpy(), db.numpy()) <= 1e-10, name
    # the module's forward is the weighted sum and reports the three terms
    reg2 = losses.Mesh_Regularizer(r, 0.3, 0.2, 0.5, edge_length=L)
    total = reg2(grid)
    assert abs(float(total) - (0.3 * values[0] + 0.2 * values[1] + 0.5 * values[2])) <= 1e-10 * abs(float(total))
    assert rel_l2(reg2.get_last_losses()[:3], values) <= 1e-10


# ---- 3. known answers ---------------------------------------------------------------------------------------------------------
def test_unit_icosahedron():
    v, f = geometry.get_icosahedral_grid(0)
    L = float(np.linalg.norm(v[f[0, 0]] - v[f[0, 1]]))
    t_e, t_n, _ = losses.Mesh_Regularizer(0, 1.0, 1.0, 1.0, edge_length=L).terms(torch.from_numpy(v)[None])
    assert abs(float(t_n) - (1 - math.sqrt(5) / 3)) < 1e-12
    assert abs(float(t_e)) < 1e-24


def test_scale_translation_rotation():
    r = 1
    v = _bumpy_vertices(r, 2, seed=3)
    reg = losses.Mesh_Regularizer(r, 1.0, 1.0, 1.0)
    e, n, s = (float(t) for t in reg.terms(v))
    e2, n2, s2 = (float(t) for t in reg.terms(2.5 * v))
    assert abs(n2 - n) < 1e-12 * n and abs(e2 - 6.25 * e) < 1e-12 * e2 and abs(s2 - 6.25 * s) < 1e-12 * s2
    a, b = 0.7, -1.9
    rot = torch.tensor([[math.cos(a), -math.sin(a), 0.], [math.sin(a), math.cos(a), 0.], [0., 0., 1.]], dtype=torch.float64) @ \
        torch.tensor([[1., 0., 0.], [0., math.cos(b), -math.sin(b)], [0., math.sin(b), math.cos(b)]], dtype=torch.float64)
    L = 0.4
    regl = losses.Mesh_Regularizer(r, 1.0, 1.0, 1.0, edge_length=L)
    want = [float(t) for t in regl.terms(v)]
    for moved in (v + torch.tensor([0.3, -1.2, 2.0], dtype=torch.float64), v @ rot.T):
        got = [float(t) for t in regl.terms(moved)]
        assert rel_l2(got, want) < 1e-12


@pytest.mark.parametrize('L', [0.0, 0.25])
def test_all_zero_grid_is_finite_with_a_zero_gradient(L):
    r = 1
    grid = torch.zeros(2, 3, 10, 4, dtype=torch.float64, requires_grad=True)
    reg = losses.Mesh_Regularizer(r, 0.3, 0.2, 0.5, edge_length=L)
    loss = reg(grid)
    loss.backward()
    e, n, s, total = reg.get_last_losses()
    assert abs(e - L * L) <= 1e-15 and n == 0.0 and s == 0.0 and math.isfinite(total)
    assert torch.equal(grid.grad, torch.zeros_like(grid))


# ---- 4. ABI -----------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ('icn_table_vertex_stencils', 'icn_mesh_reg_workspace_floats', 'icn_mesh_reg_fwd', 'icn_mesh_reg_bwd_workspace_floats',
               'icn_mesh_reg_bwd')


def test_new_symbols_are_exported_and_the_version_stays():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 9 and _lib.lib().icn_abi_version() == 9


def test_workspace_queries_are_host_only():
    L = _lib.lib()
    V = 10242
    assert L.icn_mesh_reg_workspace_floats(36, 5) == 3 * ((36 * V + 255) // 256)
    assert L.icn_mesh_reg_bwd_workspace_floats(36, 5) == 3 * 36 * V
    for B, r in ((0, 5), (36, 99), (36, -1)):
        assert L.icn_mesh_reg_workspace_floats(B, r) == 0 and L.icn_mesh_reg_bwd_workspace_floats(B, r) == 0
    assert L.icn_table_vertex_stencils(99, None, 0) < 0 and b'subdivisions' in L.icn_last_error()


def test_entry_points_reject_bad_arguments_before_touching_a_device():
    L = _lib.lib()
    p = 0x1000                                                              # never dereferenced: every call below is rejected

    def fwd(grid=p, B=2, r=2, L_=0.0, terms=p, ws=p):
        return L.icn_mesh_reg_fwd(grid, B, r, 1.0, 1.0, 1.0, L_, terms, ws, None)

    def bwd(grid=p, up=p, B=2, r=2, L_=0.0, dgrid=p, ws=p, f_smooth=1.0):
        return L.icn_mesh_reg_bwd(grid, up, B, r, 1.0, 1.0, f_smooth, L_, dgrid, ws, None)
    for call, kw, word in ((fwd, dict(grid=None), b'null'), (fwd, dict(terms=None), b'null'), (fwd, dict(ws=None), b'null'),
                           (fwd, dict(B=0), b'bad B'), (fwd, dict(r=99), b'subdivisions'), (fwd, dict(L_=-1.0), b'edge_length'),
                           (fwd, dict(L_=float('nan')), b'edge_length'), (fwd, dict(L_=float('inf')), b'edge_length'),
                           (bwd, dict(grid=None), b'null'), (bwd, dict(up=None), b'null'), (bwd, dict(dgrid=None), b'null'),
                           (bwd, dict(ws=None), b'null'), (bwd, dict(B=0), b'bad B'), (bwd, dict(r=99), b'subdivisions'),
                           (bwd, dict(L_=-1.0), b'edge_length'), (bwd, dict(L_=float('nan')), b'edge_length')):
        assert call(**kw) < 0, kw
        msg = L.icn_last_error()
        assert word in msg and b'icn_mesh_reg_' in msg, (kw, msg)


# ---- 6. HIP against the float64 torch formulation ---------------------------------------------------------------------------
FACTORS = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.3, 0.2, 0.5))
CASES = ((1, 2, 'bumpy'), (2, 3, 'bumpy'), (3, 2, 'smooth'), (5, 2, 'bumpy'))
POLE_CASES = ((0, 1, 'bumpy'), (0, 3, 'bumpy'), (1, 1, 'bumpy'), (1, 3, 'bumpy'))     # r = 0: all 10 pixels are pole corners


@functools.lru_cache(maxsize=None)
def _reference(r, B, mesh, with_length):
    """float64 torch formulation on the CPU: (fp32 grid, L, terms, {factors: gradient})."""
    grid = _grid_case(r, B, mesh)
    L = float(np.float32(_mean_edge_length(r, grid))) if with_length else 0.0
    g = grid.double().requires_grad_()
    terms = losses.Mesh_Regularizer(r, 1.0, 1.0, 1.0, edge_length=L).terms(losses.grid_to_vertices(g, r))
    per_term = [torch.autograd.grad(t, g, retain_graph=True)[0] for t in terms]
    grads = {f: f[0] * per_term[0] + f[1] * per_term[1] + f[2] * per_term[2] for f in FACTORS}
    return grid, L, [float(t) for t in terms], grads


def _pole_corner_mask(r):
    n = 2 ** r
    m = torch.zeros(5 * n, 2 * n, dtype=torch.bool)
    for c in range(5):
        m[c * n, 0] = True
        m[(c + 1) * n - 1, 2 * n - 1] = True
    assert int(m.sum()) == 10
    return m


@pytest.mark.gpu
@pytest.mark.parametrize('with_length', [False, True])
@pytest.mark.parametrize('r,B,mesh', CASES + POLE_CASES)
def test_hip_matches_float64(r, B, mesh, with_length):
    grid, L, want_terms, want_grads = _reference(r, B, mesh, with_length)
    corners = _pole_corner_mask(r)
    for f in FACTORS:
        reg = losses.Mesh_Regularizer(r, *f, edge_length=L)
        g = grid.cuda().requires_grad_()
        loss = reg(g)
        assert isinstance(loss.grad_fn, torch.autograd.function.BackwardCFunction)       # the HIP path, not the torch formulation
        loss.backward()
        got_terms = reg.get_last_losses()
        print(r, B, mesh, L, f, 'terms', got_terms[:3], want_terms)
        for k in range(3):
            assert abs(got_terms[k] - want_terms[k]) <= 1e-4 * abs(want_terms[k]), (f, k)
        total = sum(f[k] * want_terms[k] for k in range(3))
        assert abs(got_terms[3] - total) <= 1e-4 * abs(total) and abs(float(loss) - total) <= 1e-4 * abs(total)
        got, want = g.grad.cpu().double(), want_grads[f]
        e_all, e_pole = rel_l2(got.numpy(), want.numpy()), rel_l2(got[:, :, corners].numpy(), want[:, :, corners].numpy())
        print(r, B, mesh, L, f, 'gradient rel-L2 %.3g, pole corners %.3g' % (e_all, e_pole))
        assert e_all <= 1e-4, f
        assert e_pole <= 1e-4, f


# ---- 7. cross-checks ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_smoothness_is_the_p2p_laplacian_term_against_zero_rows():
    r, B = 2, 3
    grid = _grid_case(r, B, 'bumpy').cuda()
    reg = losses.Mesh_Regularizer(r, 0.0, 0.0, 1.0)
    reg(grid)
    p2p = losses.Point2Point_Loss(r, 0.0, 0.0, 1.0)
    p2p(grid, torch.zeros(B, 9, geometry.num_vertices(r), device='cuda'))
    a, b = float(reg.last_smooth), float(p2p.last_loss_lap)
    assert abs(a - b) <= 1e-6 * abs(b)


def _raw_backward(grid_bp3, r, factors, L, dgrid):
    lib = _lib.lib()
    B = grid_bp3.shape[0]
    up = torch.ones(1, device='cuda')
    ws = torch.empty(lib.icn_mesh_reg_bwd_workspace_floats(B, r), device='cuda')
    rc = lib.icn_mesh_reg_bwd(grid_bp3.data_ptr(), up.data_ptr(), B, r, factors[0], factors[1], factors[2], L, dgrid.data_ptr(),
                              ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, 'icn_mesh_reg_bwd')
    return dgrid


@pytest.mark.gpu
def test_deterministic_fully_written_and_per_sample():
    r, B, L = 2, 3, 0.3
    grid = _grid_case(r, B, 'bumpy').cuda()
    outs = []
    for _ in range(2):
        reg = losses.Mesh_Regularizer(r, 0.3, 0.2, 0.5, edge_length=L)
        g = grid.clone().requires_grad_()
        loss = reg(g)
        loss.backward()
        outs.append((loss.detach().clone(), torch.stack((reg.last_edge, reg.last_ncons, reg.last_smooth)).clone(), g.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # a dgrid pre-filled with NaN comes back fully overwritten, for every combination of active terms
    bp3 = grid.permute(0, 2, 3, 1).contiguous()
    for f in FACTORS + ((0.0, 0.0, 0.0),):
        d = _raw_backward(bp3, r, f, L, torch.full_like(bp3, float('nan')))
        assert bool(torch.isfinite(d).all()), f
    assert torch.equal(_raw_backward(bp3, r, FACTORS[3], L, torch.full_like(bp3, float('nan'))).permute(0, 3, 1, 2), outs[0][2])
    # the terms are means over the batch: sample 1 of a batch of 3, times 3, is the batch-of-1 gradient
    one = _raw_backward(bp3[1:2].contiguous(), r, FACTORS[3], L, torch.empty_like(bp3[1:2]))
    assert rel_l2((3 * outs[0][2].permute(0, 2, 3, 1)[1:2]).cpu().numpy(), one.cpu().numpy()) <= 1e-6


# ---- 8. the documented clamps on degenerate meshes: the cases, and the float64 torch formulation on them ---------------------------
# "A clamped face passes no gradient", "an edge shorter than 1e-12 adds L^2 and no gradient": on meshes that are degenerate in the
# ways a saturated or untrained network makes them.  Every case is chosen from float64 alone so that no |n| and no |d|^2 lies within
# a factor 10 of its clamp threshold (asserted), so fp32 and float64 have no excuse to take different branches.
DEGENERATE = ('zero', 'copied vertex', 'pole corners', 'collinear face', 'tiny', 'huge', 'saturated')


def _pixel_faces(r):
    """Faces (i, p, q) of the stencil table whose three vertices are grid pixels, away from the poles' corners."""
    vs = _lib.table_vertex_stencils(r)
    P = geometry.num_vertices(r) - 2
    corners = set(torch.nonzero(_pole_corner_mask(r).reshape(-1)).reshape(-1).tolist())
    return [(i, int(vs[i, 0, 0]), int(vs[i, 0, 1])) for i in range(P)
            if max(vs[i, 0, 0], vs[i, 0, 1]) < P and not {i, int(vs[i, 0, 0]), int(vs[i, 0, 1])} & corners]


def _degenerate_grid(r, case):
    n, B = 2 ** r, 2
    if case == 'zero':
        return torch.zeros(B, 3, 5 * n, 2 * n)
    if case == 'saturated':
        from test_point_to_mesh_shapes import _saturated_grid
        return _saturated_grid(B, r)
    flat = _grid_case(r, B, 'bumpy').reshape(B, 3, -1).clone()                      # (B, 3, P): column j is vertex j
    i, p, q = _pixel_faces(r)[len(_pixel_faces(r)) // 2]
    if case == 'copied vertex':                                                     # a zero-length edge, two faces without area
        flat[:, :, i] = flat[:, :, p]
    elif case == 'pole corners':                                                    # the pole and its whole ring in one lattice point
        corners = [(c * n) * 2 * n for c in range(5)]
        point = torch.round(flat[:, :, corners[0]] * 256) / 256                     # 5 x and 5 x / 5 are exact in fp32
        flat[:, :, corners] = point[:, :, None]
    elif case == 'collinear face':                                                  # area exactly zero in fp32, edges not
        a = torch.round(flat[:, :, i] * 64) / 64
        step = torch.tensor([16.0, -12.0, 8.0]) / (64 * 2 ** (r - 1))
        flat[:, :, i], flat[:, :, p], flat[:, :, q] = a, a + step, a + 2 * step
    elif case == 'tiny':                                                            # every |n| far below the 1e-12 clamp
        flat *= 1e-7
    elif case == 'huge':
        flat *= 1e6
    return flat.reshape(B, 3, 5 * n, 2 * n).contiguous()


def _clamp_margins(grid, r):
    """float64 |n| of both faces of every edge and |d|^2 of every edge; none within a factor 10 of its threshold."""
    reg = losses.Mesh_Regularizer(r, 1.0, 1.0, 1.0)
    v = losses.grid_to_vertices(grid.double(), r)
    vi, vp, vq, vm = (torch.index_select(v, 1, reg.edge_idx[c]) for c in range(4))
    d2 = ((vi - vp) ** 2).sum(-1)
    nl = torch.cat([torch.cross(vp - vi, vq - vi, dim=2).norm(dim=2), torch.cross(vm - vi, vp - vi, dim=2).norm(dim=2)], 1)
    assert not bool(((nl > 1e-13) & (nl < 1e-11)).any()) and not bool(((d2 > 1e-25) & (d2 < 1e-23)).any())
    return nl, d2


@functools.lru_cache(maxsize=None)
def _degenerate_reference(r, case, with_length):
    grid = _degenerate_grid(r, case)
    L = float(np.float32(max(_mean_edge_length(r, grid), 0.25 if case == 'zero' else 0.0))) if with_length else 0.0
    g = grid.double().requires_grad_()
    terms = losses.Mesh_Regularizer(r, 1.0, 1.0, 1.0, edge_length=L).terms(losses.grid_to_vertices(g, r))
    per_term = [torch.autograd.grad(t, g, retain_graph=True)[0] for t in terms]
    grads = {f: f[0] * per_term[0] + f[1] * per_term[1] + f[2] * per_term[2] for f in FACTORS}
    return grid, L, [float(t.detach()) for t in terms], grads


@pytest.mark.parametrize('case', DEGENERATE)
@pytest.mark.parametrize('r', [1, 2])
def test_degenerate_cases_keep_clear_of_the_clamp_thresholds(r, case):
    grid = _degenerate_grid(r, case)
    nl, d2 = _clamp_margins(grid, r)
    flat_faces, short_edges = int((nl <= 1e-13).sum()), int((d2 <= 1e-25).sum())
    print(r, case, 'clamped normals %d of %d, clamped edges %d of %d' % (flat_faces, nl.numel(), short_edges, d2.numel()))
    if case in ('zero', 'tiny'):
        assert flat_faces == nl.numel() and short_edges == (d2.numel() if case == 'zero' else 0)
    elif case == 'huge':
        assert flat_faces == 0 and short_edges == 0
    elif case == 'collinear face':
        assert flat_faces >= 2 * 3 and short_edges == 0                              # one face, seen from each of its three edges
    else:
        assert flat_faces >= 2 * 2 and short_edges >= 2
    for with_length in (False, True):                                               # the float64 formulation itself is finite
        _, _, terms, grads = _degenerate_reference(r, case, with_length)
        assert all(math.isfinite(t) for t in terms) and all(bool(torch.isfinite(g).all()) for g in grads.values())


def _check_against_float64_under_the_clamps(r, case, with_length, device):
    """Mesh_Regularizer in fp32 on `device` (cuda: k_mreg_fwd / k_mreg_bwd; cpu: the torch formulation) against the float64 torch formulation at the file's 1e-4, terms and gradient, for every FACTORS.
    Where the float64 value is 0 (a term of the all-zero grid, the normal term's gradient on a mesh whose every face is clamped)
    the bound is 0 too: the HIP value must be exactly 0.  A face with two coincident vertices has the normal 0 exactly in both
    precisions only because the kernels round both products of a cross product (face_normal in csrc/icn_mesh_device.h); contracted
    to an FMA, v x v is about 6e-8 |v|^2, far above the 1e-12 clamp, and such a face would count with a random unit normal."""
    grid, L, want_terms, want_grads = _degenerate_reference(r, case, with_length)
    _clamp_margins(grid, r)
    for f in FACTORS:
        reg = losses.Mesh_Regularizer(r, *f, edge_length=L)
        g = grid.clone().to(device).requires_grad_()
        loss = reg(g)
        assert (device == 'cuda') == isinstance(loss.grad_fn, torch.autograd.function.BackwardCFunction)       # the HIP path
        loss.backward()
        got_terms = reg.get_last_losses()
        print(r, case, L, f, 'terms', got_terms[:3], want_terms)
        assert all(math.isfinite(t) for t in got_terms) and math.isfinite(float(loss))
        for k in range(3):
            assert abs(got_terms[k] - want_terms[k]) <= 1e-4 * abs(want_terms[k]), (f, k, got_terms[k], want_terms[k])
        total = sum(f[k] * want_terms[k] for k in range(3))
        assert abs(got_terms[3] - total) <= 1e-4 * abs(total) and abs(float(loss) - total) <= 1e-4 * abs(total)
        got, want = g.grad.cpu().double(), want_grads[f]
        assert bool(torch.isfinite(got).all()), f
        if not bool(want.any()):
            assert not bool(got.any()), (f, 'gradient must be exactly zero', float(got.abs().max()))
        else:
            e = rel_l2(got.numpy(), want.numpy())
            print(r, case, L, f, 'gradient rel-L2 %.3g' % e)
            assert e <= 1e-4, (f, e)
    if case == 'zero':                                                              # T_e = L^2 and nothing else, no gradient at all
        assert want_terms == [L * L, 0.0, 0.0] and not any(bool(w.any()) for w in want_grads.values())


@pytest.mark.parametrize('with_length', [False, True])
@pytest.mark.parametrize('case', DEGENERATE)
@pytest.mark.parametrize('r', [1, 2])
def test_fp32_torch_formulation_matches_float64_under_the_clamps(r, case, with_length):
    _check_against_float64_under_the_clamps(r, case, with_length, 'cpu')


@pytest.mark.gpu
@pytest.mark.parametrize('with_length', [False, True])
@pytest.mark.parametrize('case', DEGENERATE)
@pytest.mark.parametrize('r', [1, 2])
def test_hip_matches_float64_under_the_clamps(r, case, with_length):
    _check_against_float64_under_the_clamps(r, case, with_length, 'cuda')


def _saturated_surface_case(r=2, B=2):
    from test_point_to_mesh_shapes import _saturated_grid
    output = _saturated_grid(B, r)
    target = torch.zeros(B, 9, geometry.num_vertices(r))
    target[:, 0:3] = (_bumpy_vertices(r, B, seed=7) * torch.tensor([0.9, 1.2], dtype=torch.float64)[:, None, None]).transpose(1, 2).float()
    L = float(np.float32(_mean_edge_length(r, output)))
    return output, target, dict(factor_p2m=1.0, factor_m2p=1.0, factor_edge=0.1, factor_ncons=0.01, factor_smooth=0.1, edge_length=L)


@functools.lru_cache(maxsize=None)
def _saturated_surface_reference():
    output, target, kw = _saturated_surface_case()
    crit = losses.Surface_Loss(2, **kw)
    x = output.double().requires_grad_()
    loss = crit(x, target.double())
    loss.backward()
    return float(loss.detach()), crit.get_last_losses(), x.grad.detach()


def test_surface_loss_on_the_saturated_grid_is_finite_in_float64():
    total, parts, grad = _saturated_surface_reference()
    assert math.isfinite(total) and all(math.isfinite(t) for t in parts) and bool(torch.isfinite(grad).all())
    assert parts[0] > 0 and parts[1] > 0 and parts[2] > 0 and bool(grad.any())


@pytest.mark.gpu
def test_surface_loss_on_the_saturated_grid():
    """Both directions of the distance and the regularisers with the saturated mesh as the output: in the mesh-to-points term it is
    the TRIANGLE mesh, four faces in five without area, and the vertex gradient flows into rings of coincident vertices and on to
    the grid.  Against the torch fallback in float64: the loss and its three parts at 1e-4; the gradient finite and bit-identical
    run to run and search to search.  The gradient is not compared value by value: target points with two closest points on this
    folded mesh, and the split among coincident faces and vertices, make it a matter of choice; what is well defined of it is
    checked with those points weighted out in tests/test_point_to_mesh_shapes.py::test_hip_gradients_on_whole_meshes."""
    output, target, kw = _saturated_surface_case()
    want_total, want_parts, want_grad = _saturated_surface_reference()
    runs = []
    for search in ('brute', 'brute', 'grid'):
        crit = losses.Surface_Loss(2, search=search, **kw).cuda()
        x = output.cuda().requires_grad_()
        loss = crit(x, target.cuda())
        loss.backward()
        runs.append((loss.detach().clone(), x.grad.clone(), crit.get_last_losses()))
    for other in runs[1:]:                                                          # run to run, and search to search
        assert torch.equal(runs[0][0], other[0]) and torch.equal(runs[0][1], other[1]) and runs[0][2] == other[2]
    got_total, got_grad, got_parts = float(runs[0][0]), runs[0][1].cpu(), runs[0][2]
    print('Surface_Loss on the saturated grid: got', got_parts, 'float64', want_parts)
    assert math.isfinite(got_total) and bool(torch.isfinite(got_grad).all())
    assert abs(got_total - want_total) <= 1e-4 * abs(want_total)
    for k in (0, 1, 2, 4):
        assert abs(got_parts[k] - want_parts[k]) <= 1e-4 * abs(want_parts[k]), k
