"""Self-intersection count of triangle meshes (metrics.self_intersections, self_intersection_ratio; icn_mesh_self_intersect).

The definition (metrics.self_intersections, include/icn_isect.h) is written a third time here, as plain Python loops over float64
values of the vertices rounded to fp32 (`reference`): the torch formulation must give the SAME INTEGERS, and on the GPU the HIP kernel
must give the same integers as the torch formulation evaluated in float64 on the CPU on the same fp32 vertices.  The tolerance
everywhere is zero, and it is derived, not measured: all three do the same IEEE double operations in the same order on the same inputs
(no fused multiply-add on any side), so there is no rounding to differ in."""
import functools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, geometry, losses, metrics

MAX_FACES = 1 << 20


# ---- the reference: the definition in plain loops -----------------------------------------------------------------------------------
def _orient(a, b, c, d):
    u = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    v = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    w = (d[0] - a[0], d[1] - a[1], d[2] - a[2])
    return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0])


def _crosses(p, q, a, b, c):
    sp, sq = _orient(a, b, c, p), _orient(a, b, c, q)
    if not ((sp > 0 and sq < 0) or (sp < 0 and sq > 0)):
        return False
    o = _orient(p, q, a, b), _orient(p, q, b, c), _orient(p, q, c, a)
    return all(x > 0 for x in o) or all(x < 0 for x in o)


def _intersect(A, B):
    """A is the face with the lower index."""
    return (any(_crosses(A[k], A[(k + 1) % 3], *B) for k in range(3)) or any(_crosses(B[k], B[(k + 1) % 3], *A) for k in range(3)))


def reference(v, f):
    """The boolean pair matrix (F, F) of one mesh: v (V, 3) rounded to fp32 first, then Python floats (IEEE doubles)."""
    v = np.asarray(v).astype(np.float32).astype(np.float64).tolist()
    f = np.asarray(f).astype(np.int64).tolist()
    V, F = len(v), len(f)
    valid = [all(0 <= i < V for i in face) and all(math.isfinite(x) for i in face for x in v[i]) for face in f]
    hit = np.zeros((F, F), dtype=bool)
    for i in range(F):
        for j in range(i + 1, F):
            if not (valid[i] and valid[j]) or set(f[i]) & set(f[j]):
                continue
            hit[i, j] = hit[j, i] = _intersect([v[k] for k in f[i]], [v[k] for k in f[j]])
    return hit


def _torch(v, f, unchecked=False):
    """(pairs, hits) of one mesh from the torch path as numpy arrays, and the same integers from the reference."""
    vt, ft = torch.as_tensor(np.asarray(v), dtype=torch.float32)[None], torch.as_tensor(np.asarray(f))
    call = (lambda a, b: metrics._self_intersections_unchecked(a, b.int())) if unchecked else metrics.self_intersections
    pairs, hits = call(vt, ft)
    assert pairs.dtype == torch.int64 and hits.dtype == torch.int32 and pairs.shape == (1,) and hits.shape == (1, len(f))
    want = reference(v, f).sum(1)
    assert np.array_equal(hits[0].numpy(), want), (hits[0].numpy(), want)
    assert int(pairs[0]) == want.sum() // 2 and want.sum() % 2 == 0
    return int(pairs[0]), hits[0].numpy()


# ---- the meshes ---------------------------------------------------------------------------------------------------------------------
TWO_F = np.array([[0, 1, 2], [3, 4, 5]])
PIERCE_V = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [.5, .5, -1], [.5, .5, 1], [.5, -3, 0]])
TOUCH_V = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [.5, .5, 0], [.5, .5, 1], [.5, -3, 0]])
TET = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float64)
TET_F = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]])
TETS_V = np.concatenate([TET, -0.9 * TET + np.array([.05, .02, .01])])
TETS_F = np.concatenate([TET_F, TET_F + 4])


def _pushed(r=1):
    """The icosphere with its north pole (vertex V - 2) moved to -1.5 times itself: the cap is pulled through the far side."""
    v, f = geometry.get_icosahedral_grid(r)
    v[-2] *= -1.5
    return v, f


def _crumpled(r, sigma, seed):
    """The icosphere with seeded N(0, sigma) noise on every coordinate of every vertex.  (Not along the radius alone: a mesh moved
    radially stays star-shaped about the origin, every ray from there still meets it once, and it cannot intersect itself --
    the float64 reference counts 0 pairs on the 1280-face sphere moved radially by sigma 0.2.)"""
    v, f = geometry.get_icosahedral_grid(r)
    return v + sigma * np.random.default_rng(seed).standard_normal(v.shape), f


def _soup(n, seed=11):
    """n triangles with vertices of their own, all 3 n of them standard normal: a cloud of triangles through one another."""
    return np.random.default_rng(seed).standard_normal((3 * n, 3)), np.arange(3 * n).reshape(n, 3)


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------
def test_a_piercing_pair_counts_and_a_touching_pair_does_not():
    pairs, hits = _torch(PIERCE_V, TWO_F)
    assert pairs == 1 and hits.tolist() == [1, 1]
    pairs, hits = _torch(TOUCH_V, TWO_F)                                     # the edge ends on the face: not strictly opposite
    assert pairs == 0 and hits.tolist() == [0, 0]


def test_closed_convex_meshes_do_not_intersect_themselves():
    for r in (0, 1):
        v, f = geometry.get_icosahedral_grid(r)
        assert len(f) == 20 * 4 ** r
        pairs, hits = _torch(v, f)
        assert pairs == 0 and not hits.any()


def test_the_pushed_pole_of_the_icosphere():
    v, f = _pushed()
    assert len(f) == 80
    pairs, hits = _torch(v, f)
    assert pairs == 10 and (hits > 0).sum() == 10
    at_pole = (f == len(v) - 2).any(1)
    assert at_pole.sum() == 5 and hits[at_pole].tolist() == [2] * 5
    assert metrics.self_intersection_ratio(torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f)) == 10 / 80


def test_two_interpenetrating_tetrahedra():
    pairs, hits = _torch(TETS_V, TETS_F)
    assert pairs == 12 and hits.tolist() == [3] * 8


# ---- 2. a soup ----------------------------------------------------------------------------------------------------------------------
def test_a_soup_of_triangles_is_symmetric_and_every_row_sum_is_even():
    v, f = _soup(32)
    pairs, hits = _torch(v, f)
    # "many": two such triangles, both about two units across and both around the origin, meet far more often than one time in
    # twenty-five; of the 496 pairs that would be 20
    assert pairs >= 20
    vt, ft = torch.as_tensor(v, dtype=torch.float32)[None], torch.as_tensor(f)
    matrix = metrics._torch_intersecting_pairs(vt, ft, 0, len(f))[0]
    assert matrix.dtype == torch.bool and matrix.shape == (32, 32)
    assert torch.equal(matrix, matrix.T) and not matrix.diagonal().any()
    assert np.array_equal(matrix.numpy(), reference(v, f))
    assert np.array_equal(matrix.sum(1).numpy(), hits) and hits.sum() % 2 == 0 and pairs == hits.sum() // 2
    # every chunking of the rows gives the same integers
    for chunk in (1, 5, 32, 100):
        assert np.array_equal(metrics._torch_self_intersections(vt, ft, chunk=chunk)[0].numpy(), hits)
    # a batch: each mesh on its own
    other = _soup(32, seed=12)[0]
    pairs2, hits2 = metrics.self_intersections(torch.as_tensor(np.stack([v, other]), dtype=torch.float32), ft)
    assert np.array_equal(hits2[0].numpy(), hits) and np.array_equal(hits2[1].numpy(), reference(other, f).sum(1))
    assert pairs2.tolist() == [pairs, int(hits2[1].sum()) // 2] and all(int(x) % 2 == 0 for x in hits2.sum(1))


# ---- 3. exclusions ------------------------------------------------------------------------------------------------------------------
def test_a_duplicated_face_does_not_hit_its_twin():
    assert _torch(PIERCE_V, np.array([[0, 1, 2], [0, 1, 2]]))[1].tolist() == [0, 0]
    assert _torch(PIERCE_V, np.array([[0, 1, 2], [1, 2, 0]]))[1].tolist() == [0, 0]
    # both twins are hit by the face that pierces them, and not by each other
    assert _torch(PIERCE_V, np.array([[0, 1, 2], [3, 4, 5], [0, 1, 2]]))[1].tolist() == [1, 2, 1]


def test_faces_sharing_a_vertex_are_not_tested_even_when_they_fold_through_each_other():
    # the second face starts at vertex 1 of the first and its far edge passes through the first's interior
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [.5, .5, -1], [.5, .5, 1], [2, 0, 0]])
    assert _torch(v, np.array([[0, 1, 2], [1, 3, 4]]))[1].tolist() == [0, 0]
    # the same geometry with a vertex of its own in the same place: now it is tested, and it hits
    assert _torch(v, np.array([[0, 1, 2], [5, 3, 4]]))[1].tolist() == [1, 1]


def test_a_face_with_a_bad_id_neither_hits_nor_is_hit_on_the_unchecked_path():
    for bad in (6, -1, 2 ** 31 - 1):
        # clamped into range the bad id would make the third face a copy of the second, which pierces the first
        pairs, hits = _torch(PIERCE_V, np.array([[0, 1, 2], [3, 4, 5], [3, 4, bad]]), unchecked=True)
        assert pairs == 1 and hits.tolist() == [1, 1, 0]
        pairs, hits = _torch(PIERCE_V, np.array([[0, 1, bad], [3, 4, 5]]), unchecked=True)
        assert pairs == 0 and hits.tolist() == [0, 0]


def _with_a_non_finite_vertex():
    """(vertices (3, 96, 3) fp32, faces): the soup three times, the second with a NaN and the third with an inf in one vertex."""
    v, f = _soup(32)
    batch = np.stack([v, v, v]).astype(np.float32)
    batch[1, 3 * 7 + 1, 2] = np.nan
    batch[2, 3 * 20, 0] = -np.inf
    return batch, f


def test_a_face_with_a_non_finite_coordinate_neither_hits_nor_is_hit_and_the_rest_is_unchanged():
    batch, f = _with_a_non_finite_vertex()
    pairs, hits = metrics._self_intersections_unchecked(torch.as_tensor(batch), torch.as_tensor(f).int())
    clean = reference(batch[0], f)
    assert clean[7].any() and clean[20].any()                                # the two faces did hit something
    assert np.array_equal(hits[0].numpy(), clean.sum(1))
    for b, gone in ((1, 7), (2, 20)):
        want = clean.copy()
        want[gone, :] = want[:, gone] = False
        assert np.array_equal(reference(batch[b], f), want)
        assert np.array_equal(hits[b].numpy(), want.sum(1)) and hits[b, gone] == 0
    assert pairs.tolist() == (hits.sum(1) // 2).tolist()
    assert np.array_equal(metrics.self_intersections(torch.as_tensor(batch), torch.as_tensor(f))[1].numpy(), hits.numpy())


def test_a_face_without_area_can_pierce_and_cannot_be_pierced():
    # vertices 4 and 5 coincide: the second face is the segment of the piercing pair
    v = PIERCE_V.copy()
    v[5] = v[4]
    assert _torch(v, TWO_F)[1].tolist() == [1, 1]
    # a collinear face along x, and a triangle in the plane x = 1 whose first edge passes through the point (1, 0, 0) of it
    v = np.array([[0, 0, 0], [2, 0, 0], [4, 0, 0], [1, -1, -1], [1, 1, 1], [1, 5, -5]])
    assert _torch(v, TWO_F)[1].tolist() == [0, 0]


# ---- 4. invariance of the count -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mesh', ['pushed', 'tetrahedra'])
def test_the_count_is_invariant_under_relabelling_winding_face_order_and_powers_of_two(mesh):
    v, f = _pushed() if mesh == 'pushed' else (TETS_V, TETS_F)
    pairs, hits = _torch(v, f)
    assert pairs == (10 if mesh == 'pushed' else 12)
    for g in (f[:, [1, 2, 0]], f[:, [2, 0, 1]], f[:, ::-1].copy()):          # cyclic relabelling; every winding reversed
        p, h = _torch(v, g)
        assert p == pairs and np.array_equal(h, hits)
    order = np.random.default_rng(5).permutation(len(f))
    p, h = _torch(v, f[order])
    assert p == pairs and np.array_equal(h, hits[order])
    for scale in (2.0 ** -20, 0.25, 8.0, 2.0 ** 30):
        p, h = _torch(v * scale, f)
        assert p == pairs and np.array_equal(h, hits)


# ---- 5. arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_checks_and_output_types():
    v, f = (torch.as_tensor(x) for x in _pushed())
    v = v.float()[None]
    for bad_v in (v[0], v[..., :2], v.long(), v[:0], v[:, :0]):
        with pytest.raises(ValueError):
            metrics.self_intersections(bad_v, f)
    for bad_f in (f.float(), f[:, :2], f[0], f[:0], f == 0):
        with pytest.raises(ValueError):
            metrics.self_intersections(v, bad_f)
    with pytest.raises(ValueError, match='at most 1048576'):
        metrics.self_intersections(v, torch.zeros(MAX_FACES + 1, 3, dtype=torch.int32))
    for bad_id in (v.shape[1], -1):
        g = f.clone()
        g[3, 1] = bad_id
        with pytest.raises(IndexError):
            metrics.self_intersections(v, g)
    with pytest.raises(ValueError):
        metrics.self_intersection_ratio(v, f)                                # one mesh: (V, 3)
    for dtype in (torch.float32, torch.float64, torch.float16):
        pairs, hits = metrics.self_intersections(v.to(dtype).requires_grad_(), f.int())
        assert pairs.dtype == torch.int64 and hits.dtype == torch.int32 and not pairs.requires_grad and not hits.requires_grad
        assert pairs.tolist() == [10]
    assert metrics.self_intersection_ratio(v[0], f) == 10 / 80
    assert metrics.self_intersection_ratio(torch.as_tensor(geometry.get_icosahedral_grid(1)[0]), f) == 0.0


# ---- the GPU: the kernel against the torch formulation in float64 on the CPU, integer for integer ------------------------------------
B = 3


@functools.lru_cache(maxsize=None)
def _case(name):
    """(vertices (3, V, 3) fp32, faces (F, 3) int64, hits (3, F) int32 of the torch formulation in float64 on the CPU), computed
    once and shared; three DIFFERENT meshes of one connectivity, so that a wrong batch offset cannot pass."""
    if name == 'two faces':
        v, f = np.stack([PIERCE_V, TOUCH_V, 3 * PIERCE_V]), TWO_F
    elif name == 'icosahedron':
        clean, f = geometry.get_icosahedral_grid(0)
        v = np.stack([clean, 2 * clean, _crumpled(0, 0.6, 1)[0]])
    elif name == 'icosphere 80':
        v, f = np.stack([geometry.get_icosahedral_grid(1)[0], _crumpled(1, 0.3, 2)[0], _pushed()[0]]), geometry.get_ico_faces(1)
    elif name == 'tetrahedra':
        v, f = np.stack([TETS_V, 0.5 * TETS_V, np.concatenate([TET, -0.9 * TET + 0.3])]), TETS_F
    elif name in ('soup 32', 'soup 320'):                                    # 320: one full tile of 256 faces and a partial one
        n = int(name.split()[1])
        v, f = np.stack([_soup(n, seed)[0] for seed in (11, 12, 13)]), _soup(n)[1]
    elif name == 'icosphere 1280':
        v, f = np.stack([geometry.get_icosahedral_grid(3)[0], _crumpled(3, 0.2, 3)[0], _pushed(3)[0]]), geometry.get_ico_faces(3)
    elif name == 'non-finite and bad ids':
        v, f = _with_a_non_finite_vertex()
        f = f.copy()
        f[5, 0], f[30, 2] = -1, 96
    else:
        raise KeyError(name)
    v, f = torch.as_tensor(v, dtype=torch.float32), torch.as_tensor(f)
    return v, f, metrics._torch_self_intersections(v, f)


CASES = ('two faces', 'icosahedron', 'icosphere 80', 'tetrahedra', 'soup 32', 'soup 320', 'icosphere 1280', 'non-finite and bad ids')


def _hip(v, f):
    pairs, hits = metrics._self_intersections_unchecked(v.cuda(), f.to(device='cuda', dtype=torch.int32))
    assert hits.is_cuda and hits.dtype == torch.int32 and pairs.dtype == torch.int64
    return pairs.cpu(), hits.cpu()


def _profiled(call):
    _lib.profile_start(512)
    try:
        result = call()
    finally:
        kernels = {e['kernel']: e['launches'] for e in _lib.profile_stop()}
    return result, kernels.get('k_mesh_self_intersect', 0)


@pytest.mark.gpu
@pytest.mark.parametrize('name', CASES)
def test_hip_equals_the_float64_formulation_exactly(name):
    v, f, want = _case(name)
    pairs, hits = _hip(v, f)
    assert torch.equal(hits, want), 'hits differ at %s' % (hits != want).nonzero().tolist()[:10]
    assert torch.equal(pairs, want.sum(1, dtype=torch.int64) // 2)
    if name == 'two faces':
        assert hits.tolist() == [[1, 1], [0, 0], [1, 1]]
    if name == 'icosphere 80':
        assert pairs.tolist()[0] == 0 and pairs.tolist()[2] == 10
    if name == 'tetrahedra':
        assert hits[0].tolist() == [3] * 8
    if name == 'icosphere 1280':
        assert pairs[0] == 0 and pairs[1] >= 100                             # crumpled: hundreds of hits, 2 per pair
    if name == 'non-finite and bad ids':
        assert hits[:, 5].tolist() == [0] * 3 and hits[:, 30].tolist() == [0] * 3 and hits[1, 7] == 0 and hits[2, 20] == 0
        assert hits[0, 7] > 0 and hits[0, 20] > 0


def _boxes_overlap(v, f):
    """(F, F) bool of one mesh: the fp32 bounding boxes of faces i and j overlap, lo_i <= hi_j and lo_j <= hi_i on every axis."""
    tri = v.numpy()[f.numpy()]                                               # (F, 3, 3) fp32
    lo, hi = tri.min(1), tri.max(1)
    assert lo.dtype == np.float32
    return ((lo[:, None] <= hi[None]) & (lo[None] <= hi[:, None])).all(-1)


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['soup 320', 'icosphere 1280'])
def test_the_box_filter_removes_nothing(name):
    """Every pair the float64 formulation (which has no box test) calls intersecting has overlapping fp32 boxes, and the device, which
    tests only such pairs, counts as many: the filter removed nothing."""
    v, f, want = _case(name)
    _, hits = _hip(v, f)
    for b in (range(B) if name == 'soup 320' else (1,)):                     # the three soups; the crumpled sphere
        matrix = metrics._torch_intersecting_pairs(v[b:b + 1], f, 0, len(f))[0].numpy()
        assert np.array_equal(matrix.sum(1), want[b].numpy())
        assert not (matrix & ~_boxes_overlap(v[b], f)).any()
        assert int(hits[b].sum()) == int(matrix.sum())
    assert int(want[1].sum()) > 0


@pytest.mark.gpu
def test_hip_more_meshes_than_one_launch_takes():
    n = 65537
    v = torch.as_tensor(TOUCH_V, dtype=torch.float32).repeat(n, 1, 1)
    v[-1] = torch.as_tensor(PIERCE_V, dtype=torch.float32)
    assert list(metrics._batch_slices(n)) == [(0, 65535), (65535, 2)]
    (pairs, hits), launches = _profiled(lambda: _hip(v, torch.as_tensor(TWO_F)))
    assert launches == 2
    assert int(pairs[-1]) == 1 and int(pairs[:-1].sum()) == 0 and hits[-1].tolist() == [1, 1] and int(hits.sum()) == 2


@pytest.mark.gpu
def test_hip_determinism_and_plumbing(monkeypatch):
    v, f, want = _case('icosphere 1280')
    first, second = _hip(v, f), _hip(v, f)
    assert torch.equal(first[1], second[1]) and torch.equal(first[0], second[0])
    # the public function: non-contiguous vertices, int64 / int32 faces, vertices that require grad
    wide = torch.zeros(B, v.shape[1], 5, device='cuda')
    wide[..., 1:4] = v.cuda()
    view = wide[..., 1:4].requires_grad_()
    assert not view.is_contiguous()
    for faces in (f.cuda(), f.int()):
        (pairs, hits), launches = _profiled(lambda: metrics.self_intersections(view, faces))
        assert launches == 1 and hits.is_cuda and not hits.requires_grad and not pairs.requires_grad
        assert torch.equal(hits.cpu(), want) and torch.equal(pairs.cpu(), first[0])
    assert metrics.self_intersection_ratio(v[2].cuda(), f) == float((want[2] > 0).sum()) / len(f)
    # one launch per batch slice: B = 5 in slices of 2, the integers of the one-launch result
    five = torch.cat([v, v[:2] * 0.5])
    whole = _hip(five, f)[1]
    assert torch.equal(whole[:3], want) and torch.equal(whole[3:], want[:2])
    with monkeypatch.context() as m:
        m.setattr(metrics, '_MAX_GRID_Y', 2)
        assert list(metrics._batch_slices(5)) == [(0, 2), (2, 2), (4, 1)]
        (_, sliced), launches = _profiled(lambda: _hip(five, f))
    assert launches == 3 and torch.equal(sliced, whole)
    # ICN_NO_HIP_LOSS=1: the torch formulation, on the device, the same integers
    monkeypatch.setattr(losses, '_NO_HIP_LOSS', True)                        # what ICN_NO_HIP_LOSS=1 sets at import
    small = _case('soup 320')
    (_, hits), launches = _profiled(lambda: _hip(small[0], small[1]))
    assert launches == 0 and torch.equal(hits, small[2])


@pytest.mark.gpu
def test_no_host_synchronisation_in_the_unchecked_call():
    v, f, want = _case('soup 320')
    v, f32 = v.cuda(), f.to(device='cuda', dtype=torch.int32)
    metrics._self_intersections_unchecked(v, f32)                            # the allocator settles
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
            pairs, hits = metrics._self_intersections_unchecked(v, f32)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert caught, "torch.cuda.set_sync_debug_mode('error') does not catch a deliberate .item() on this build"
    assert torch.equal(hits.cpu(), want) and torch.equal(pairs.cpu(), want.sum(1, dtype=torch.int64) // 2)
