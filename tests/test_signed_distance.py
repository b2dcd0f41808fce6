"""Signed point-to-mesh distance, inside test and volumetric IoU (metrics.signed_point_to_mesh_distance, contains, volumetric_iou;
icn_point_to_mesh_sign).

The definition of the sign (metrics.signed_point_to_mesh_distance, include/icn_sdf.h) is written a third time here, as plain Python
loops over float64 values of the fp32 inputs (`reference`), and the generalised winding number (Van Oosterom & Strackee 1983, float64)
stands beside it as INDEPENDENT TRUTH: a point is inside iff w > 1/2.  Two conditions decide which points are compared, both evaluated
on the float64 reference alone and before anything is compared:
  * formulation against formulation (torch against `reference`, HIP against torch): every point whose float64 |cos angle(d, N)| >= 1e-3.
    The sides do the same arithmetic up to the last bit of an atan2 (and, on the device, fused multiply-adds), which can turn a sign
    only where d is all but orthogonal to N;
  * against the winding truth: every point with |w - 1/2| >= 0.25 (w is 0 or 1 up to rounding away from the surface).
The points either condition leaves out are counted and capped at 0.5 % per mesh.  The meshes: tetrahedron, cube (vertices of valence 4
and 5), the level-2 icosphere, the same with a non-convex radial bump and with vertex noise, and the SPIKE, a narrow cone whose apex has
sixteen faces of very different angles: the mesh on which the plain sum of the incident normals gives the wrong sign at a large share
of the points nearest the apex, and the angle-weighted sum does not."""
import functools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, geometry, metrics

from test_point_to_mesh_grad import AMBIGUOUS_CAP, BAR, CASES, _ambiguous, _batch, _rel

COS_MIN, W_MARGIN, LEFT_OUT_CAP = 1e-3, 0.25, 0.005


# ---- the reference: the definition in plain loops -----------------------------------------------------------------------------------
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _segment(up, uw):
    den = _dot(uw, uw)
    t = _dot(uw, up) / den if den != 0 else 0.0
    t = 0.0 if not t > 0 else (t if t < 1 else 1.0)
    return (up[0] - uw[0] * t, up[1] - uw[1] * t, up[2] - uw[2] * t)


def reference(points, vertices, faces, face, kind, tables, weighted=True):
    """(sign, cos) of one mesh, lists over the points: the definition on Python floats (IEEE doubles) of the fp32 inputs.  cos is
    d . N / (|d| |N|), 0 where either vanishes or the point is refused; weighted=False drops the angles (the variant the spike refutes)."""
    p_all = np.asarray(points).astype(np.float32).astype(np.float64).tolist()
    v = np.asarray(vertices).astype(np.float32).astype(np.float64).tolist()
    f = np.asarray(faces).astype(np.int64).tolist()
    adjacency, offsets, corners = (np.asarray(t).astype(np.int64).tolist() for t in tables)
    V, F = len(v), len(f)
    nc = 3 * F
    flat = [i for tri in f for i in tri]

    def usable(g):
        return 0 <= g < F and all(0 <= i < V for i in f[g])

    def normal(g):
        a, b, c = (v[i] for i in f[g])
        n = _cross(_sub(b, a), _sub(c, a))
        return n, _dot(n, n)

    def add(N, n, nn, w=1.0):
        if nn != 0:
            length = math.sqrt(nn)
            return (N[0] + w * (n[0] / length), N[1] + w * (n[1] / length), N[2] + w * (n[2] / length))
        return N
    signs, cosines = [], []
    for p, g, k in zip(p_all, np.asarray(face).tolist(), np.asarray(kind).tolist()):
        if not (usable(g) and 0 <= k <= 6):
            signs.append(1.0), cosines.append(0.0)
            continue
        a, b, c = (v[i] for i in f[g])
        n, nn = normal(g)
        N = (0.0, 0.0, 0.0)
        if k == 0:
            s = _dot(_sub(p, a), n) / nn if nn != 0 else 0.0
            d, N = (n[0] * s, n[1] * s, n[2] * s), n
        elif k >= 4:
            d = (_segment(_sub(p, a), _sub(b, a)), _segment(_sub(p, b), _sub(c, b)), _segment(_sub(p, a), _sub(c, a)))[k - 4]
            N = add(N, n, nn)
            across = adjacency[g][k - 4]
            if usable(across):
                N = add(N, *normal(across))
        else:
            j = f[g][k - 1]
            pj = v[j]
            d = _sub(p, pj)
            lo, hi = (min(max(o, 0), nc) for o in (offsets[j], offsets[j + 1]))
            for at in range(lo, hi):
                cid = corners[at]
                if not (0 <= cid < nc and flat[cid] == j and usable(cid // 3)):
                    continue
                h, kk = cid // 3, cid % 3
                m, mm = normal(h)
                if mm != 0:
                    ea, eb = _sub(v[f[h][(kk + 1) % 3]], pj), _sub(v[f[h][(kk + 2) % 3]], pj)
                    N = add(N, m, mm, math.atan2(math.sqrt(mm), _dot(ea, eb)) if weighted else 1.0)
        dn = _dot(d, N)
        signs.append(-1.0 if dn < 0 else 1.0)
        size = math.sqrt(_dot(d, d)) * math.sqrt(_dot(N, N))
        cosines.append(dn / size if size > 0 and math.isfinite(size) and math.isfinite(dn) else 0.0)
    return signs, cosines


def winding(points, vertices, faces):
    """The generalised winding number of every point about one mesh (Van Oosterom & Strackee), float64 of the fp32 inputs: 1 inside a
    closed mesh wound counter-clockwise seen from outside, 0 outside."""
    p = np.asarray(points).astype(np.float32).astype(np.float64)[:, None, :]
    tri = np.asarray(vertices).astype(np.float32).astype(np.float64)[np.asarray(faces)]
    a, b, c = tri[None, :, 0] - p, tri[None, :, 1] - p, tri[None, :, 2] - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    det = (a * np.cross(b, c)).sum(-1)
    den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
    return (2 * np.arctan2(det, den)).sum(1) / (4 * math.pi)


# ---- the meshes ---------------------------------------------------------------------------------------------------------------------
TET = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
TET_F = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
TET_ADJACENCY = [[1, 3, 2], [2, 3, 0], [0, 3, 1], [1, 2, 0]]
CUBE = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float64)     # vertex 4 x + 2 y + z
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [3, 7, 6], [3, 6, 2], [2, 6, 4], [2, 4, 0], [1, 5, 7],
                   [1, 7, 3]])
CUBE_ADJACENCY = [[5, 11, 1], [0, 7, 9], [8, 6, 3], [2, 10, 4], [9, 3, 5], [4, 10, 0], [11, 2, 7], [6, 8, 1], [7, 2, 9], [8, 4, 1],
                  [5, 3, 11], [10, 6, 0]]


def _spike():
    theta = np.sort(np.concatenate([np.linspace(0, 0.6, 13), [1.6, 3.1, 4.7]]))
    ring = np.stack([0.15 * np.cos(theta), 0.15 * np.sin(theta), -np.ones(16)], 1)
    v = np.concatenate([[[0, 0, 0]], ring, ring + [0, 0, -1], [[0, 0, -2]]])
    R, L, C = list(range(1, 17)), list(range(17, 33)), 33
    f = []
    for i in range(16):
        k = (i + 1) % 16
        f += [[0, R[i], R[k]], [R[i], L[i], L[k]], [R[i], L[k], R[k]], [C, L[k], L[i]]]
    return v, np.array(f)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    """(vertices float64 (V, 3), faces (F, 3)) of a test mesh, closed and wound counter-clockwise seen from outside."""
    if name == 'tetrahedron':
        return TET, TET_F
    if name == 'cube':
        return CUBE, CUBE_F
    if name == 'spike':
        return _spike()
    v, f = geometry.get_icosahedral_grid(2)
    if name == 'bump':
        lon, colat = np.arctan2(v[:, 1], v[:, 0]), np.arccos(np.clip(v[:, 2], -1, 1))
        v = v * (1 + 0.35 * np.sin(3 * lon) * np.cos(2 * colat))[:, None]
    elif name == 'noise':
        v = v + 0.05 * np.random.default_rng(5).standard_normal(v.shape)
    else:
        assert name == 'icosphere'
    return v, f


MESHES = ('tetrahedron', 'cube', 'icosphere', 'bump', 'noise', 'spike')


def _cloud(name, count, seed):
    """count points about a mesh: half uniform in its box padded by 0.3, half vertices with sigma 0.03 noise; for the spike
    0.15 N(0, I) about the apex."""
    v, _ = _mesh(name)
    g = np.random.default_rng(seed)
    if name == 'spike':
        return (0.15 * g.standard_normal((count, 3))).astype(np.float32)
    lo, hi = v.min(0) - 0.3, v.max(0) + 0.3
    box = lo + (hi - lo) * g.random((count // 2, 3))
    near = v[g.integers(0, len(v), count - count // 2)] + 0.03 * g.standard_normal((count - count // 2, 3))
    return np.concatenate([box, near]).astype(np.float32)


def _tensors(name):
    v, f = _mesh(name)
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f)


def _judged(points, vertices, faces, face, kind, tables):
    """What the float64 reference says about one cloud on one mesh, before anything is compared: (sign, comparable with another
    formulation, truth sign, comparable with the truth), numpy arrays over the points; the caps are asserted here."""
    sign, cos = (np.array(x) for x in reference(points, vertices, faces, face, kind, tables))
    w = winding(points, vertices, faces)
    by_cos, by_w = np.abs(cos) >= COS_MIN, np.abs(w - 0.5) >= W_MARGIN
    n = len(sign)
    assert (~by_cos).sum() <= LEFT_OUT_CAP * n, 'left out by |cos| < %g: %d of %d' % (COS_MIN, (~by_cos).sum(), n)
    assert (~by_w).sum() <= LEFT_OUT_CAP * n, 'left out by |w - 1/2| < %g: %d of %d' % (W_MARGIN, (~by_w).sum(), n)
    return sign, by_cos, np.where(w > 0.5, -1.0, 1.0), by_w


@functools.lru_cache(maxsize=None)
def _cpu_case(name):
    """One cloud (2 000 points; 2 600 about the spike's apex) through the checked function on the CPU in fp32, and the reference's
    verdict on the (face, kind) it found.  Computed once, shared, never changed."""
    v, f = _tensors(name)
    p = torch.from_numpy(_cloud(name, 2600 if name == 'spike' else 2000, seed=17))
    phi, face, kind = metrics.signed_point_to_mesh_distance(p[None], v[None], f)
    tables = metrics.signed_distance_tables(f, len(v))
    return p, v, f, tables, phi[0], face[0], kind[0], _judged(p, v, f, face[0], kind[0], tables)


# ---- CPU 1: the three statements of the definition and the truth ----------------------------------------------------------------------
@pytest.mark.parametrize('name', MESHES)
def test_meshes_are_closed_outward_wound_manifolds(name):
    v, f = _tensors(name)
    adjacency, offsets, corners = metrics.signed_distance_tables(f, len(v))
    assert int(adjacency.min()) >= 0
    assert float(metrics.mesh_area_volume(v[None], f)[1]) > 0
    assert abs(float(metrics.total_curvature(v[None].double(), f)) - 4 * math.pi) < 1e-9       # a sphere
    valence = (offsets[1:] - offsets[:-1]).tolist()
    if name == 'cube':
        assert sorted(set(valence)) == [4, 5]
    if name == 'spike':
        assert len(v) == 34 and len(f) == 64 and valence[0] == 16


@pytest.mark.parametrize('name', MESHES)
def test_torch_formulation_equals_the_reference_and_the_winding_truth(name):
    p, v, f, tables, phi, face, kind, (sign, by_cos, truth, by_w) = _cpu_case(name)
    got = metrics._torch_point_to_mesh_sign(p[None], v[None], f, face[None], kind[None], tables)[0]
    assert got.dtype == torch.float64 and set(got.tolist()) <= {-1.0, 1.0}
    got = got.numpy()
    print('%s: %d points, %d inside, left out %d by cos and %d by w, kinds %s' % (
        name, len(got), (truth < 0).sum(), (~by_cos).sum(), (~by_w).sum(), np.bincount(kind.numpy(), minlength=7).tolist()))
    assert np.array_equal(got[by_cos], sign[by_cos])
    assert np.array_equal(got[by_w], truth[by_w])
    assert (truth < 0).any() and (truth > 0).any()                           # (few points about the apex are inside the narrow spike)
    # phi is that sign on the forward's distance, exactly
    dist2 = metrics.point_to_mesh_distance(p[None], v[None], f)[0][0]
    assert torch.equal(phi.abs(), dist2.sqrt())
    assert torch.equal(phi < 0, torch.from_numpy(got < 0) & (dist2 > 0))


def test_the_spike_tells_angle_weights_from_none():
    p, v, f, tables, phi, face, kind, (sign, by_cos, truth, by_w) = _cpu_case('spike')
    at_apex = ((kind >= 1) & (kind <= 3)).numpy() & (f[face, (kind.long() - 1).clamp(0, 2)] == 0).numpy()
    assert at_apex.sum() >= 1000
    plain = np.array(reference(p, v, f, face, kind, tables, weighted=False)[0])
    use = at_apex & by_w
    wrong_plain, wrong_weighted = (plain[use] != truth[use]).mean(), (sign[use] != truth[use]).mean()
    print('spike: %d apex points, unweighted wrong at %.3f, weighted at %.3f' % (use.sum(), wrong_plain, wrong_weighted))
    assert wrong_plain > 0.10 and wrong_weighted == 0


# ---- CPU 2: the tables ---------------------------------------------------------------------------------------------------------------
def test_adjacency_of_the_tetrahedron_and_the_cube_by_hand():
    for v, f, want in ((TET, TET_F, TET_ADJACENCY), (CUBE, CUBE_F, CUBE_ADJACENCY)):
        adjacency, offsets, corners = metrics.signed_distance_tables(torch.from_numpy(f), len(v))
        assert adjacency.dtype == torch.int32 and adjacency.tolist() == want
        o, c = metrics.vertex_face_table(torch.from_numpy(f), len(v))
        assert torch.equal(offsets, o) and torch.equal(corners, c)
    adjacency = metrics.signed_distance_tables(torch.from_numpy(TET_F).int(), 4)[0]                # int32 faces alike
    assert adjacency.tolist() == TET_ADJACENCY


def test_adjacency_is_symmetric_on_the_icosphere():
    v, f = _mesh('icosphere')
    adjacency = metrics.signed_distance_tables(torch.from_numpy(f), len(v))[0].tolist()
    for g in range(len(f)):
        for e in range(3):
            h = adjacency[g][e]
            assert g in adjacency[h]
            assert {int(f[g][e]), int(f[g][(e + 1) % 3])} <= set(f[h].tolist())


def test_open_and_non_manifold_meshes_are_refused_by_the_checked_function_only():
    v, f = _tensors('cube')
    p = torch.from_numpy(_cloud('cube', 200, seed=3))[None]
    open_f = f[:-1]
    with pytest.raises(ValueError, match=r'not closed: no face holds the edge \(\d+, \d+\)'):
        metrics.signed_point_to_mesh_distance(p, v[None], open_f)
    with pytest.raises(ValueError, match='not closed'):
        metrics.contains(p, v[None], open_f)
    with pytest.raises(ValueError, match=r'not manifold: the directed edge \(0, 1\)'):
        metrics.signed_point_to_mesh_distance(p, v[None], torch.cat([f, f[:1]]))
    tables = metrics.signed_distance_tables(open_f, 8)
    assert sorted(set(tables[0].reshape(-1).tolist()))[0] == -1
    phi, face, kind = metrics._signed_point_to_mesh_distance_unchecked(p, v[None], open_f.int(), tables)
    assert set(torch.sign(phi[phi != 0]).tolist()) == {-1.0, 1.0}
    want = reference(p[0], v, open_f, face[0], kind[0], tables)
    keep = np.abs(np.array(want[1])) >= COS_MIN
    assert np.array_equal((phi[0] < 0).numpy()[keep], (np.array(want[0]) < 0)[keep])


# ---- CPU 3: degenerate and invalid input on the torch path ---------------------------------------------------------------------------
def _every_feature(f):
    """(face, kind) (1, 7 F) tensors naming every feature of every face."""
    F = len(f)
    face = torch.arange(F).repeat_interleave(7)[None]
    return face, torch.arange(7, dtype=torch.int32).repeat(F)[None]


def _both(p, v, f, face, kind, tables):
    """The torch formulation on one mesh, asserted equal to the reference wherever the reference's cosine is not marginal."""
    got = metrics._torch_point_to_mesh_sign(p[None], v[None], f, face, kind, tables)[0].numpy()
    sign, cos = (np.array(x) for x in reference(p, v, f, face[0], kind[0], tables))
    keep = (np.abs(cos) >= COS_MIN) | (cos == 0)                             # cos == 0: refused or degenerate, +1 by definition
    assert np.array_equal(got[keep], sign[keep])
    return got


def test_a_face_with_coincident_vertices_contributes_nothing():
    v = torch.from_numpy(TET.astype(np.float32))
    f = torch.cat([torch.from_numpy(TET_F), torch.tensor([[0, 0, 1], [2, 2, 2]])])                 # two faces without area
    tables = metrics.signed_distance_tables(f, 4)
    plain = metrics.signed_distance_tables(f[:4], 4)
    face, kind = _every_feature(f[:4])
    g = torch.Generator().manual_seed(2)
    p = torch.randn(face.shape[1], 3, generator=g)
    with_flat = _both(p, v, f, face, kind, tables)
    without = _both(p, v, f[:4], face, kind, plain)
    assert np.array_equal(with_flat, without)
    # on the faces without area themselves: (2, 2, 2) has no normal on its plane nor across its edges (it is its own neighbour), so
    # +1 there; its vertex kinds see the four faces around vertex 2; never a NaN
    face, kind = torch.full((1, 7), 5), torch.arange(7, dtype=torch.int32)[None]
    assert _both(p[:7], v, f, face, kind, tables)[[0, 4, 5, 6]].tolist() == [1.0] * 4
    _both(p[:7], v, f, torch.full((1, 7), 4), kind, tables)


def test_ids_out_of_range_and_lying_tables_are_refused_or_skipped_as_defined():
    v, f = _tensors('cube')
    F, V = len(f), len(v)
    tables = metrics.signed_distance_tables(f, V)
    g = torch.Generator().manual_seed(4)
    p = 0.5 + 0.6 * torch.randn(7 * F, 3, generator=g)
    face, kind = _every_feature(f)
    honest = _both(p, v, f, face, kind, tables)
    assert (honest < 0).any() and (honest > 0).any()
    # a face or a kind out of range: +1
    for bad_face, bad_kind in ((torch.full_like(face, -1), kind), (torch.full_like(face, F), kind), (face, torch.full_like(kind, 7)),
                               (face, torch.full_like(kind, -1))):
        assert _both(p, v, f, bad_face, bad_kind, tables).tolist() == [1.0] * (7 * F)
    # a vertex id out of range: that face is refused as the closest one (+1) and skipped as a neighbour
    broken = f.clone()
    broken[3, 1] = V
    got = _both(p, v, broken, face, kind, tables)
    assert got[face[0] == 3].tolist() == [1.0] * 7
    broken[3, 1] = -1
    _both(p, v, broken, face, kind, tables)
    # adjacency entries out of range add nothing; entries that name other faces are used as they stand
    adjacency, offsets, corners = tables
    for lie in (torch.full_like(adjacency, F), torch.full_like(adjacency, -7), adjacency.roll(5, 0)):
        _both(p, v, f, face, kind, (lie, offsets, corners))
    # a corner table of other vertices' corners is rejected entry by entry (+1 on the vertex kinds: N = 0); offsets beyond are clamped
    lying = _both(p, v, f, face, kind, (adjacency, offsets, corners.roll(7)))
    assert (lying[((kind[0] >= 1) & (kind[0] <= 3)).numpy()] == 1.0).all()
    _both(p, v, f, face, kind, (adjacency, offsets, torch.full_like(corners, 3 * F)))
    _both(p, v, f, face, kind, (adjacency, (offsets.long() * 1000 - 5).int(), corners))


def test_nan_points_are_outside_with_a_nan_distance():
    v, f = _tensors('tetrahedron')
    p = torch.tensor([[[0.1, 0.0, 0.0], [float('nan'), 0.0, 0.0], [5.0, 5.0, 5.0]]])
    phi, face, kind = metrics.signed_point_to_mesh_distance(p, v[None], f)
    assert phi[0, 0] < 0 and phi[0, 2] > 0 and math.isnan(float(phi[0, 1]))
    sign = metrics._torch_point_to_mesh_sign(p, v[None], f, face, kind, metrics.signed_distance_tables(f, 4))
    assert sign.tolist() == [[-1.0, 1.0, 1.0]]
    assert metrics.contains(p, v[None], f).tolist() == [[True, False, False]]


# ---- CPU 4: the gradient --------------------------------------------------------------------------------------------------------------
def test_gradcheck_away_from_the_surface_and_from_ties():
    v, f = _mesh('tetrahedron')
    v, f = torch.from_numpy(v)[None], torch.from_numpy(f)
    g = torch.Generator().manual_seed(8)
    p = (torch.rand(1, 64, 3, generator=g, dtype=torch.float64) * 2.4 - 1.2)
    phi = metrics.signed_point_to_mesh_distance(p, v, f)[0]
    keep = (phi[0].abs() >= 0.05) & ~_ambiguous(p, v, f)[0]
    p = p[:, keep][:, :12].clone().requires_grad_(True)
    assert p.shape[1] == 12 and (phi[0][keep][:12] < 0).any() and (phi[0][keep][:12] > 0).any()
    v = v.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: metrics.signed_point_to_mesh_distance(a, b, f)[0], (p, v), eps=1e-6, atol=1e-6)


def test_the_subgradient_on_the_surface_is_zero():
    v, f = _mesh('tetrahedron')
    v, f = torch.from_numpy(v)[None].clone().requires_grad_(True), torch.from_numpy(f)
    p = torch.tensor([[[1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]]], dtype=torch.float64, requires_grad=True)   # a vertex, inside, an edge
    phi, _, _ = metrics.signed_point_to_mesh_distance(p, v, f)
    assert phi[0, 0] == 0 and phi[0, 1] < 0 and phi[0, 2] == 0
    phi.sum().backward()
    assert torch.isfinite(p.grad).all() and torch.isfinite(v.grad).all()
    assert p.grad[0, 0].tolist() == [0.0] * 3 and p.grad[0, 2].tolist() == [0.0] * 3
    assert abs(float(p.grad[0, 1].norm()) - 1) < 1e-12                       # |grad phi| = 1 off the surface


# ---- CPU 5: volumetric IoU, the shim, the arguments ---------------------------------------------------------------------------------------
def test_two_unit_cubes_half_a_side_apart_overlap_by_exactly_a_third():
    v, f = _tensors('cube')
    shifted = v + torch.tensor([0.5, 0.0, 0.0])
    assert metrics.volumetric_iou(v, shifted, f, resolution=48) == 16384 / 49152
    assert metrics.volumetric_iou(v, v, f, resolution=8) == 1.0
    assert metrics.volumetric_iou(v, v + 2.0, f, resolution=12) == 0.0
    assert metrics.volumetric_iou(v.double(), shifted.double(), f.int(), resolution=24) == 1 / 3


def _occupancy(v, f, resolution, device='cpu'):
    """(count h^3, h) of one mesh on the lattice of volumetric_iou, built here a second time."""
    lo, hi = v.double().amin(0), v.double().amax(0)
    h = float((hi - lo).max()) / resolution
    axes = [float(lo[k]) + (torch.arange(max(1, math.ceil(float(hi[k] - lo[k]) / h)), dtype=torch.float64) + 0.5) * h for k in range(3)]
    centres = torch.stack(torch.meshgrid(*axes, indexing='ij'), -1).reshape(1, -1, 3).to(v.dtype)
    inside = metrics.contains(centres.to(device), v[None].to(device), f.to(device))
    return float(inside.sum()) * h ** 3, h


@pytest.mark.parametrize('r', (2, 3))
def test_lattice_occupancy_of_the_icosphere_is_its_volume_within_the_derived_bound(r):
    """A misclassified cell has its centre within h sqrt(3) / 2 of the surface: |count h^3 - volume| <= sqrt(3) area h."""
    v, f = geometry.get_icosahedral_grid(r)
    v, f = torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f)
    area, volume = (float(x) for x in metrics.mesh_area_volume(v[None], f))
    got, h = _occupancy(v, f, 16)
    print('I%d: occupancy %.4f volume %.4f, error %.2g, bound %.2g' % (r, got, volume, abs(got - volume), math.sqrt(3) * area * h))
    assert abs(got - volume) <= math.sqrt(3) * area * h


def test_kaolin_shim_is_contains():
    import geniconet_amd.shims.kaolin.ops.mesh as kaolin_mesh
    p, v, f, _, phi, _, _, _ = _cpu_case('bump')
    inside = kaolin_mesh.check_sign(v[None], f, p[None], hash_resolution=64)
    assert inside.dtype == torch.bool and inside.shape == (1, len(p))
    assert torch.equal(inside, metrics.contains(p[None], v[None], f)) and torch.equal(inside[0], phi < 0)


def test_arguments_are_checked():
    v, f = _tensors('cube')
    p = torch.zeros(1, 5, 3)
    tables = metrics.signed_distance_tables(f, 8)
    for call in (metrics.signed_point_to_mesh_distance, metrics.contains):
        for args, kwargs in (((p[0], v[None], f), {}), ((p, v, f), {}), ((p, v[None, :, :2], f), {}), ((p.repeat(2, 1, 1), v[None], f), {}),
                             ((p, v[None], f[:, :2]), {}), ((p, v[None], f[:0]), {}), ((p, v[None], f.float()), {}),
                             ((p[:, :0], v[None], f), {}), ((p.double(), v[None], f), {}), ((p, v[None], f), dict(search='tree')),
                             ((p, v[None], f), dict(tables=tables[:2])), ((p, v[None], f), dict(tables=(tables[0][:5],) + tables[1:])),
                             ((p, v[None], f), dict(tables=tuple(t.long() for t in tables)))):
            with pytest.raises(ValueError):
                call(*args, **kwargs)
        with pytest.raises(IndexError):
            call(p, v[None], f + 1)
        with pytest.raises(IndexError):
            call(p, v[None, :7], f)
        assert call(p, v[None], f, tables=tables)[0].shape[-1] == 5
    with pytest.raises(ValueError):
        metrics.signed_distance_tables(f.float(), 8)
    with pytest.raises(ValueError):
        metrics.signed_distance_tables(f, 0)
    for args, kwargs in (((v[None], v[None], f), {}), ((v, v[:7], f), {}), ((v, v, f), dict(resolution=0)), ((v * 0, v * 0, f), {}),
                         ((v, v, f), dict(search='tree'))):
        with pytest.raises(ValueError):
            metrics.volumetric_iou(*args, **kwargs)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
SCALES = (1.0, 1.1, 0.9)


@functools.lru_cache(maxsize=None)
def _gpu_batch(name, P=700):
    """A batch of three: the mesh at three scales, each with a cloud of its own seed scaled alike (fp32 CPU tensors)."""
    v, f = _tensors(name)
    p = torch.stack([torch.from_numpy(_cloud(name, P, seed=31 + b)) * s for b, s in enumerate(SCALES)])
    return p, torch.stack([v * s for s in SCALES]), f


@pytest.mark.gpu
@pytest.mark.parametrize('search', ('brute', 'grid'))
@pytest.mark.parametrize('name', MESHES)
def test_hip_sign_equals_the_torch_formulation_and_the_winding_truth(name, search):
    p, v, f = _gpu_batch(name)
    tables = metrics.signed_distance_tables(f, v.shape[1])
    phi, face, kind = metrics.signed_point_to_mesh_distance(p.cuda(), v.cuda(), f.cuda(), search=search)
    assert phi.is_cuda and phi.dtype == torch.float32 and face.dtype == torch.int64 and kind.dtype == torch.int32
    dist2, face0, kind0 = metrics.point_to_mesh_distance(p.cuda(), v.cuda(), f.cuda(), search=search)
    assert torch.equal(face, face0) and torch.equal(kind, kind0)
    assert torch.equal(phi.abs(), dist2.sqrt())                              # bit for bit
    face, kind = face.cpu(), kind.cpu()
    judged = [_judged(p[b], v[b], f, face[b], kind[b], tables) for b in range(3)]      # the caps, on the reference alone, first
    sign = torch.where(phi < 0, -1.0, 1.0).double().cpu()
    hip = metrics._hip_point_to_mesh_sign(p.cuda(), v.cuda(), f.int().cuda(), tuple(t.cuda() for t in tables), face.int().cuda(),
                                          kind.cuda()).cpu()
    assert set(hip.unique().tolist()) <= {-1.0, 1.0}
    assert torch.equal(hip.double() < 0, sign < 0) or bool((dist2 == 0).any())
    want = metrics._torch_point_to_mesh_sign(p, v, f, face, kind, tables)
    for b, (ref_sign, by_cos, truth, by_w) in enumerate(judged):
        assert np.array_equal(hip[b].numpy()[by_cos], want[b].numpy()[by_cos]), (name, search, b)
        assert np.array_equal(want[b].numpy()[by_cos], ref_sign[by_cos])
        assert np.array_equal(hip[b].numpy()[by_w], truth[by_w]), (name, search, b)


@pytest.mark.gpu
@pytest.mark.parametrize('P', (257, 1))
def test_hip_sign_one_thread_past_a_block_and_a_single_point(P):
    p, v, f = _gpu_batch('bump', 700)
    p = p[:, 350:350 + P].contiguous()                                        # from the half near the surface
    tables = metrics.signed_distance_tables(f, v.shape[1])
    for search in ('brute', 'grid'):
        phi, face, kind = metrics.signed_point_to_mesh_distance(p.cuda(), v.cuda(), f.cuda(), search=search)
        assert phi.shape == (3, P)
        want = metrics._torch_point_to_mesh_sign(p, v, f, face.cpu(), kind.cpu(), tables)
        keep = np.stack([np.abs(np.array(reference(p[b], v[b], f, face[b].cpu(), kind[b].cpu(), tables)[1])) >= COS_MIN for b in range(3)])
        assert (~keep).sum() <= LEFT_OUT_CAP * keep.size
        assert np.array_equal((phi.cpu() < 0).numpy()[keep], (want < 0).numpy()[keep])


@functools.lru_cache(maxsize=None)
def _gradient_case():
    """The first case of tests/test_point_to_mesh_grad.py (the bumpy icosphere at two scales, 700 points about it); upstream weights
    in [0.5, 1.5], 0 at the points nearer than 0.05 to the surface and at the ambiguous ones (decided in float64 on the CPU, before
    any GPU result exists)."""
    p, v, f = _batch(*CASES[0])
    amb = _ambiguous(p, v, f)
    pd, vd = p.double().requires_grad_(True), v.double().requires_grad_(True)
    phi, _, _ = metrics.signed_point_to_mesh_distance(pd, vd, f)
    near = phi.detach().abs() < 0.05
    g = torch.Generator().manual_seed(12)
    w = (torch.rand(p.shape[:2], generator=g, dtype=torch.float64) + 0.5) * ~(amb | near)
    (phi * w).sum().backward()
    return p, v, f, w, float(amb.double().mean()), pd.grad, vd.grad


@pytest.mark.gpu
@pytest.mark.parametrize('search', ('brute', 'grid'))
def test_hip_gradients_match_float64_autograd_and_the_existing_backward_bit_for_bit(search):
    p, v, f, w, share, want_p, want_v = _gradient_case()
    assert share <= AMBIGUOUS_CAP and int((w > 0).sum()) > 150
    pc, vc = p.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    phi, face, kind = metrics.signed_point_to_mesh_distance(pc, vc, f.cuda(), search=search)
    assert phi.requires_grad and not face.requires_grad and not kind.requires_grad
    (phi * w.float().cuda()).sum().backward()
    e_p, e_v = _rel(pc.grad, want_p), _rel(vc.grad, want_v)
    print('%s: ambiguous %.4f, hip dphi/dpoints %.3g dphi/dvertices %.3g' % (search, share, e_p, e_v))
    assert e_p <= BAR and e_v <= BAR
    # the same numbers from the existing backward under the rescaled upstream
    p2, v2 = p.cuda().requires_grad_(True), v.cuda().requires_grad_(True)
    dist2, _, _ = metrics._PointToMeshFn.apply(p2, v2, f.int().cuda(), search)
    root, sign, g = dist2.detach().sqrt(), torch.where(phi.detach() < 0, -1.0, 1.0), w.float().cuda()
    dist2.backward(torch.where(root == 0, torch.zeros_like(g), g * sign / (2 * root)))
    assert torch.equal(p2.grad, pc.grad) and torch.equal(v2.grad, vc.grad)
    # gradient tracking off, or nothing to differentiate: no graph
    with torch.no_grad():
        assert not metrics.signed_point_to_mesh_distance(pc, vc, f.cuda(), search=search)[0].requires_grad
    assert not metrics.signed_point_to_mesh_distance(p.cuda(), v.cuda(), f.cuda(), search=search)[0].requires_grad


def _profiled(call):
    _lib.profile_start(512)
    try:
        result = call()
        torch.cuda.synchronize()
    finally:
        kernels = {e['kernel']: e['launches'] for e in _lib.profile_stop()}
    return result, kernels


@pytest.mark.gpu
def test_batch_slicing_determinism_and_one_launch_per_slice(monkeypatch):
    p, v, f = _gpu_batch('noise')
    pc, vc, fc = p.cuda(), v.cuda(), f.int().cuda()
    tables = tuple(t.cuda() for t in metrics.signed_distance_tables(f, v.shape[1]))

    def run():
        return metrics._signed_point_to_mesh_distance_unchecked(pc, vc, fc, tables, 'grid')
    (phi, face, kind), kernels = _profiled(run)
    assert kernels['k_p2m_sign'] == 1 and kernels['k_p2m_grid_query'] == 1 and 'k_point_to_mesh' not in kernels
    again = run()
    assert torch.equal(again[0], phi) and torch.equal(again[1], face) and torch.equal(again[2], kind)       # bit-identical run to run
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 2)
    sliced, kernels = _profiled(run)
    assert kernels['k_p2m_sign'] == 2 and kernels['k_p2m_grid_query'] == 2
    assert torch.equal(sliced[0], phi) and torch.equal(sliced[1], face) and torch.equal(sliced[2], kind)
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 1)
    sliced, kernels = _profiled(run)
    assert kernels['k_p2m_sign'] == 3
    assert torch.equal(sliced[0], phi)


@pytest.mark.gpu
def test_tables_that_lie_within_range_give_what_the_torch_formulation_gives_on_them():
    """Adjacency entries that name valid but non-adjacent faces, and a corner table of other vertices' corners, which `incident`
    rejects: wrong signs, the same wrong signs as the torch formulation's, and nothing out of bounds.  (Ids out of range are guarded
    in the kernel and covered on the torch path; no GPU test feeds them.)"""
    p, v, f = _gpu_batch('noise')
    adjacency, offsets, corners = metrics.signed_distance_tables(f, v.shape[1])
    dist2, face, kind = metrics.point_to_mesh_distance(p.cuda(), v.cuda(), f.cuda())
    honest = None
    for tables in ((adjacency, offsets, corners), (adjacency.roll(37, 0), offsets, corners), (adjacency, offsets, corners.roll(11)),
                   (adjacency.flip(0), offsets, corners.flip(0))):
        got = metrics._hip_point_to_mesh_sign(p.cuda(), v.cuda(), f.int().cuda(), tuple(t.contiguous().cuda() for t in tables),
                                              face.int(), kind).cpu()
        want = metrics._torch_point_to_mesh_sign(p, v, f, face.cpu(), kind.cpu(), tables)
        cos = np.stack([np.array(reference(p[b], v[b], f, face[b].cpu(), kind[b].cpu(), tables)[1]) for b in range(3)])
        keep = (np.abs(cos) >= COS_MIN) | (cos == 0)                          # cos == 0: a vertex whose corners were all rejected, +1
        assert np.array_equal(got.numpy()[keep], want.numpy()[keep])
        if honest is None:
            honest = got
            assert (~keep).sum() <= LEFT_OUT_CAP * keep.size
        else:
            assert not torch.equal(got, honest)                               # the lie shows


@pytest.mark.gpu
def test_no_host_synchronisation_in_the_unchecked_calls():
    p, v, f = _gpu_batch('bump')
    fc = f.int().cuda()
    pc, vc = p.cuda(), v.cuda()

    def both():
        tables = metrics.signed_distance_tables(fc, v.shape[1])
        a = pc.clone().requires_grad_(True)
        b = vc.clone().requires_grad_(True)
        phi, _, _ = metrics._signed_point_to_mesh_distance_unchecked(a, b, fc, tables, 'grid')
        phi.sum().backward()
        with torch.no_grad():
            plain = metrics._signed_point_to_mesh_distance_unchecked(pc, vc, fc, tables, 'brute')[0]
        return phi.detach(), a.grad, b.grad, plain
    both()                                                                    # workspaces and the allocator settle
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
            phi, gp, gv, plain = both()
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert caught, "torch.cuda.set_sync_debug_mode('error') does not catch a deliberate .item() on this build"
    assert torch.equal(phi, plain) and bool(torch.isfinite(gp).all()) and bool(torch.isfinite(gv).all())


@pytest.mark.gpu
def test_volumetric_iou_and_check_sign_on_the_device():
    import geniconet_amd.shims.kaolin.ops.mesh as kaolin_mesh
    v, f = _tensors('cube')
    vc, fc = v.cuda(), f.cuda()
    for search in ('brute', 'grid'):
        assert metrics.volumetric_iou(vc, vc + torch.tensor([0.5, 0.0, 0.0], device='cuda'), fc, resolution=48, search=search) == 16384 / 49152
    assert metrics.volumetric_iou(vc, vc, fc, resolution=8) == 1.0 and metrics.volumetric_iou(vc, vc + 2.0, fc, resolution=12) == 0.0
    v, f = geometry.get_icosahedral_grid(2)
    v, f = torch.from_numpy(v.astype(np.float32)).cuda(), torch.from_numpy(f).cuda()
    area, volume = (float(x) for x in metrics.mesh_area_volume(v[None], f))
    resolution = 32
    h = float((v.amax(0) - v.amin(0)).max()) / resolution
    iou = metrics.volumetric_iou(0.9 * v, v, f, resolution=resolution)
    # the inner solid lies in the outer: IoU = count_inner / count_outer; a volume is off by at most sqrt(3) area h
    print('IoU %.5f against %.5f, bound %.3g' % (iou, 0.9 ** 3, math.sqrt(3) * area * h / volume))
    assert abs(iou - 0.9 ** 3) <= math.sqrt(3) * area * h / volume
    p, vb, fb = _gpu_batch('bump')
    inside = kaolin_mesh.check_sign(vb.cuda(), fb.cuda(), p.cuda())
    assert inside.dtype == torch.bool and inside.is_cuda
    assert torch.equal(inside, metrics.contains(p.cuda(), vb.cuda(), fb.cuda()))
    assert torch.equal(inside, metrics.signed_point_to_mesh_distance(p.cuda(), vb.cuda(), fb.cuda(), search='grid')[0] < 0)
