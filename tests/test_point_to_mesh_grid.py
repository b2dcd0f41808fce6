"""Grid-accelerated closest-triangle search of the point-to-mesh distance (icn_point_to_mesh_grid, search='grid').

The central property is BIT-IDENTITY with the brute-force kernel (search='brute'): both evaluate the same point-triangle routine
and keep the lowest face index among equal distances, so dist2, face and kind must be equal as bit patterns (this also compares
NaN cases); no ambiguity allowance exists.  The cases are small on purpose, except where the issue asks for I5: every path of the
kernels is reached at these sizes (several blocks per mesh, F not a multiple of 256, G = 1 and G > 1, the always-tested list, the
no-grid mode, clamped cells, early and late stops).
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, geometry, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    pts, v, f = _case(seed, P, r)
    tp, tv = torch.from_numpy(pts)[None].repeat(2, 1, 1), torch.from_numpy(v)[None].repeat(2, 1, 1)
    tv[1] *= 1.1
    return tp, tv, torch.from_numpy(f)


def _grid_res(F):
    """G of the library (include/icn.h): round(sqrt(F / 16)) in [1, 64]."""
    return int(min(64, max(1, math.floor(math.sqrt(F / 16.0) + 0.5))))


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_grid_symbols_are_exported_bound_and_abi_is_9():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('icn_point_to_mesh_grid', 'icn_point_to_mesh_grid_workspace_bytes'):
        assert hasattr(handle, name) and name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 9 and _lib.lib().icn_abi_version() == 9
    header = open(os.path.join(ROOT, 'include', 'icn.h')).read()
    assert '#define ICN_ABI_VERSION 9' in header
    res, args = _lib.SIGNATURES['icn_point_to_mesh_grid'][:2]
    assert res is ctypes.c_int and len(args) == 13 and args[-2] is ctypes.c_size_t
    res, args = _lib.SIGNATURES['icn_point_to_mesh_grid_workspace_bytes'][:2]
    assert res is ctypes.c_size_t and args == [ctypes.c_int] * 4


def test_grid_workspace_query_is_host_only_and_monotonic():
    q = _lib.lib().icn_point_to_mesh_grid_workspace_bytes
    assert q(36, 10242, 10242, 20480) > 0
    assert q(36, 10242, 10242, 20480) < 128 << 20                     # ~1.2 MB per I5 mesh: cells + one record per triangle
    assert q(0, 100, 50, 96) == 0 and q(2, 0, 50, 96) == 0 and q(2, 100, 0, 96) == 0 and q(2, 100, 50, 0) == 0
    assert q(65536, 1, 1, 1) == 0 and q(2, -3, 50, 96) == 0
    sizes = [q(4, 100, 50, F) for F in (1, 2, 35, 36, 37, 255, 256, 257, 1000, 20480, 65535, 65536, 1 << 20, 1 << 24)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    sizes = [q(B, 100, 50, 320) for B in (1, 2, 3, 36, 65535)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert q(1, 1, 1, 1) % 16 == 0 and q(3, 5, 7, 257) % 16 == 0
    assert q(2, 1, 50, 96) == q(2, 100000, 5000, 96)                  # the index is a function of B and F alone


def test_grid_call_rejects_bad_arguments_before_touching_a_device():
    """Null pointers, bad sizes and a missing / short / misaligned workspace are refused with a message; nothing here reaches a
    device call (the machine that runs this has no device)."""
    L = _lib.lib()
    x = 0x1000                                                   # never dereferenced on the host
    need = L.icn_point_to_mesh_grid_workspace_bytes(2, 100, 50, 96)
    assert need > 0

    def call(points=x, vertices=x, faces=x, B=2, P=100, V=50, F=96, dist=x, face=x, kind=x, ws=x, nbytes=need):
        return L.icn_point_to_mesh_grid(points, vertices, faces, B, P, V, F, dist, face, kind, ws, nbytes, None)
    for name in ('points', 'vertices', 'faces', 'dist', 'face', 'kind'):
        assert call(**{name: None}) != 0 and b'null pointer' in L.icn_last_error(), name
    for bad in (dict(B=0), dict(B=65536), dict(P=0), dict(V=0), dict(F=0), dict(P=-3)):
        assert call(**bad) != 0 and b'bad sizes' in L.icn_last_error(), bad
    assert call(ws=None) != 0 and b'workspace' in L.icn_last_error()
    assert call(nbytes=need - 1) != 0 and b'workspace' in L.icn_last_error()
    assert call(nbytes=0) != 0 and b'workspace' in L.icn_last_error()
    assert call(ws=x + 4) != 0 and b'aligned' in L.icn_last_error()


def test_search_argument_on_the_cpu():
    from geniconet_amd.losses import Point2Mesh_Loss
    pts, v, f = _case(1)
    tp, tv, tf = torch.from_numpy(pts)[None], torch.from_numpy(v)[None], torch.from_numpy(f)
    with pytest.raises(ValueError):
        metrics.point_to_mesh_distance(tp, tv, tf, search='bogus')
    with pytest.raises(ValueError):
        metrics.compute_distance(tp[0], tv[0], tf, search='bogus')
    with pytest.raises(ValueError):
        Point2Mesh_Loss(2, search='bogus')
    want = metrics.point_to_mesh_distance(tp, tv, tf)
    for got in (metrics.point_to_mesh_distance(tp, tv, tf, search='grid'), metrics.point_to_mesh_distance(tp, tv, tf, search='brute')):
        assert all(torch.equal(a, b) for a, b in zip(got, want))          # CPU tensors: the torch formulation whatever `search` says
    assert metrics.compute_distance(tp[0], tv[0], tf, search='grid') == metrics.compute_distance(tp[0], tv[0], tf)
    crit = Point2Mesh_Loss(2, search='grid')
    assert crit.search == 'grid' and Point2Mesh_Loss(2).search == 'brute'


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _assert_grid_equals_brute(points, vertices, faces, label=''):
    """Both searches on the GPU; dist2 / face / kind equal as bit patterns.  Returns the grid result."""
    p, v, f = points.cuda(), vertices.cuda(), faces.cuda()
    want = metrics.point_to_mesh_distance(p, v, f, search='brute')
    got = metrics.point_to_mesh_distance(p, v, f, search='grid')
    for name, a, b in zip(('dist2', 'face', 'kind'), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        same = _bits(a) == _bits(b)
        assert bool(same.all()), '%s %s: %d of %d differ, first at %s' % (
            label, name, int((~same).sum()), same.numel(), (~same).nonzero()[0].tolist())
    return got


@pytest.mark.gpu
def test_grid_equals_brute_on_the_metric_cases_and_meets_the_oracle_tolerance():
    from oracle import metrics_ref
    for seed, P, r in ((2, 700, 2), (3, 1000, 1)):
        tp, tv, tf = _batch(seed, P, r)
        d2, face, kind = _assert_grid_equals_brute(tp, tv, tf, 'case %d' % seed)
        assert d2.is_cuda and d2.shape == (2, P) and face.dtype == torch.int64 and kind.dtype == torch.int32
        for b in range(2):
            want, _ = metrics_ref.point_to_mesh_distance(tp[b].numpy(), tv[b].numpy(), tf.numpy())
            np.testing.assert_allclose(d2[b].cpu().numpy(), want, rtol=2e-4, atol=1e-9)


def _i5(batch, seed):
    from geniconet_amd import data
    from geniconet_amd.losses import grid_to_vertices
    x, _ = data.synthetic_batch(batch, 5, seed=seed, device='cuda')
    return grid_to_vertices(x, 5), torch.from_numpy(geometry.get_ico_faces(5)).cuda()


@pytest.mark.gpu
def test_grid_equals_brute_at_full_size_on_itself_and_a_shifted_copy():
    """I5: 10242 points against 20480 triangles, batch 4."""
    v, f = _i5(4, 2)
    d2, _, _ = _assert_grid_equals_brute(v, v, f, 'self')
    assert float(d2.max()) < 1e-10
    shifted = v.clone()
    shifted[..., 0] += 1e-2
    d2, _, _ = _assert_grid_equals_brute(shifted, v, f, 'shifted')
    assert 0 < float(d2.mean()) < 1e-4


@pytest.mark.gpu
def test_grid_equals_brute_on_the_three_point_clouds_at_i5():
    """Near-surface (the loss near convergence), another synthetic shape (what tools/time_point_to_mesh.py times), and a Gaussian
    cloud mostly far outside the mesh (the hostile case: many points walk to the grid's far side)."""
    v, f = _i5(1, 2)
    g = torch.Generator().manual_seed(7)
    near = v + 0.01 * torch.randn(v.shape, generator=g).cuda()
    other, _ = _i5(1, 1)
    far = 0.8 * torch.randn(v.shape, generator=g).cuda()
    for label, pts in (('near', near), ('other shape', other), ('far gaussian', far)):
        d2, _, _ = _assert_grid_equals_brute(pts, v, f, label)
        print('%s: rms distance %.4f' % (label, float(d2.mean().sqrt())))


@pytest.mark.gpu
def test_grid_equals_brute_on_a_batch_of_meshes_of_different_scale_and_offset():
    pts, v, f = _case(5, 600, 3)
    scale = torch.tensor([1.0, 0.01, 37.0])[:, None, None]
    offset = torch.tensor([[0.0, 0.0, 0.0], [3.0, -2.0, 0.5], [-100.0, 250.0, 40.0]])[:, None, :]
    tv = torch.from_numpy(v)[None] * scale + offset
    tp = torch.from_numpy(pts)[None] * scale + offset
    _assert_grid_equals_brute(tp, tv, torch.from_numpy(f), 'scaled / offset batch')
    # a mesh far from the origin relative to its size: the index is not used for it (the bound's slack would exceed a cell)
    _assert_grid_equals_brute(tp[:1] + 5000.0, tv[:1] + 5000.0, torch.from_numpy(f), 'speck far from the origin')


@pytest.mark.gpu
def test_grid_equals_brute_at_the_smallest_sizes():
    pts, v, f = _case(6, 300, 2)                                       # 320 faces
    tp, tv, tf = torch.from_numpy(pts)[None], torch.from_numpy(v)[None], torch.from_numpy(f)
    _assert_grid_equals_brute(tp, tv, tf[:1], 'F = 1')
    _assert_grid_equals_brute(tp, tv, tf[:257], 'F = 257')
    _assert_grid_equals_brute(tp[:, 77:78], tv, tf, 'P = 1')
    _assert_grid_equals_brute(tp[:, :1], tv, tf[:1], 'P = 1, F = 1')


@pytest.mark.gpu
def test_lowest_index_wins_among_duplicate_triangles():
    pts, v, f = _case(7, 500, 2)
    tf = torch.from_numpy(f)
    F0 = tf.shape[0]
    dup = torch.cat([tf, tf.flip(0), tf])                                # every triangle three times
    tp, tv = torch.from_numpy(pts)[None], torch.from_numpy(v)[None]
    _, face, _ = _assert_grid_equals_brute(tp, tv, dup, 'duplicates')
    assert int(face.max()) < F0
    _, face1, _ = _assert_grid_equals_brute(tp, tv, tf, 'single')
    assert torch.equal(face, face1)


@pytest.mark.gpu
def test_one_giant_triangle_beside_an_icosphere_stays_exact():
    pts, v, f = _case(8, 800, 3)
    big = np.array([[-40.0, -30.0, 0.3], [50.0, -30.0, 0.3], [0.0, 60.0, 0.3]], dtype=np.float32)
    tv = torch.from_numpy(np.concatenate([v, big]))[None]
    nv = len(v)
    tf = torch.cat([torch.tensor([[nv, nv + 1, nv + 2]]), torch.from_numpy(f)])      # the giant one first: it wins ties
    tp = torch.from_numpy(pts)[None]
    _, face, _ = _assert_grid_equals_brute(tp, tv, tf, 'giant triangle')
    assert 0 < int((face == 0).sum()) < tp.shape[1]                      # some points are closest to it, not all
    # also a triangle that is only moderately over-long (a few cells): the always-tested list again
    mid = np.array([[-0.6, -0.5, 1.4], [0.7, -0.5, 1.4], [0.0, 0.8, 1.4]], dtype=np.float32)
    tv = torch.from_numpy(np.concatenate([v, mid]))[None]
    _assert_grid_equals_brute(tp, tv, torch.cat([torch.from_numpy(f), torch.tensor([[nv, nv + 1, nv + 2]])]), 'over-long triangle')


def _planar_mesh(n):
    """(n + 1)^2 vertices in the plane z = 0.25, 2 n^2 triangles."""
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing='ij')
    v = np.stack([ii / n * 2 - 1, jj / n * 3 - 1.5, np.full(ii.shape, 0.25)], -1).reshape(-1, 3).astype(np.float32)
    q = (ii[:-1, :-1] * (n + 1) + jj[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)])
    return v, f


@pytest.mark.gpu
def test_planar_and_zero_extent_meshes():
    g = torch.Generator().manual_seed(9)
    v, f = _planar_mesh(20)                                              # 800 triangles
    tp = torch.randn(1, 700, 3, generator=g)
    tp[0, :100, 2] = 0.25                                                # points in the plane itself
    _assert_grid_equals_brute(tp, torch.from_numpy(v)[None], torch.from_numpy(f), 'planar')
    _, vv, ff = _case(9, 60, 2)
    point = torch.full((1, vv.shape[0], 3), 0.375)
    d2, face, kind = _assert_grid_equals_brute(tp, point, torch.from_numpy(ff), 'zero extent')
    assert int(face.max()) == 0 and int(kind.max()) == 1                  # every triangle is that one point; the first wins
    _assert_grid_equals_brute(tp, torch.zeros(1, vv.shape[0], 3), torch.from_numpy(ff), 'zero extent at the origin')


@pytest.mark.gpu
@pytest.mark.parametrize('F', (1763, 1764))
def test_cell_counts_of_one_and_of_two_scan_tiles(F):
    """G = 10 at F = 1763 (1001 counts: one tile of the scan of 1024) and G = 11 at F = 1764 (1332 counts: two tiles, a carry)."""
    assert _grid_res(F) == (10 if F == 1763 else 11)
    v, f = _planar_mesh(30)                                              # 1800 triangles
    tv = torch.from_numpy(v)[None]
    tp = tv[:, :300] + 0.01 * torch.randn(1, 300, 3, generator=torch.Generator().manual_seed(F))
    _assert_grid_equals_brute(tp, tv, torch.from_numpy(f[:F]), 'F = %d' % F)


@pytest.mark.gpu
def test_points_on_cell_boundaries_the_bounding_box_and_far_away():
    pts, v, f = _case(10, 100, 3)                                        # 1280 faces: G = 9
    G = _grid_res(f.shape[0])
    assert G == 9
    lo, hi = v.min(0), v.max(0)
    h = np.float32((hi - lo).max()) / np.float32(G)
    ticks = [lo[c] + np.arange(G + 1, dtype=np.float32) * h for c in range(3)]         # the nominal cell boundaries per axis
    g = np.random.default_rng(10)
    on = []
    for c in range(3):                                                   # one coordinate on a boundary, the others anywhere
        q = (lo + (hi - lo) * g.random((4 * (G + 1), 3))).astype(np.float32)
        q[:, c] = np.repeat(ticks[c], 4)
        on.append(q)
    corners = np.stack(np.meshgrid(ticks[0][::3], ticks[1][::3], ticks[2][::3], indexing='ij'), -1).reshape(-1, 3)   # cell corners
    box = np.array([[lo[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]], [lo[0], hi[1], lo[2]], [hi[0], lo[1], hi[2]],
                    [np.nextafter(lo[0], -np.inf), lo[1], lo[2]], [np.nextafter(hi[0], np.inf), hi[1], hi[2]]], dtype=np.float32)
    ext = float((hi - lo).max())
    dirs = g.standard_normal((64, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    far = np.concatenate([dirs * 1e3 * ext, np.eye(3) * 1e3 * ext, -np.eye(3) * 1e3 * ext, dirs[:16] * 3 * ext]).astype(np.float32)
    cloud = np.concatenate(on + [corners.astype(np.float32), box, far, pts])
    _assert_grid_equals_brute(torch.from_numpy(cloud)[None], torch.from_numpy(v)[None], torch.from_numpy(f), 'boundaries / far')


@pytest.mark.gpu
def test_non_finite_points_and_vertices_reproduce_the_brute_force_output():
    pts, v, f = _case(11, 400, 2)
    tp, tv, tf = torch.from_numpy(pts)[None].clone(), torch.from_numpy(v)[None], torch.from_numpy(f)
    nan, inf = float('nan'), float('inf')
    tp[0, 0] = torch.tensor([nan, 0.1, 0.2])
    tp[0, 1] = torch.tensor([nan, nan, nan])
    tp[0, 2] = torch.tensor([inf, 0.0, 0.0])
    tp[0, 3] = torch.tensor([0.3, -inf, 0.0])
    tp[0, 4] = torch.tensor([inf, -inf, nan])
    tp[0, 300] = torch.tensor([0.0, 0.0, 3.0e38])
    d2, face, kind = _assert_grid_equals_brute(tp, tv, tf, 'non-finite points')
    assert float(d2[0, 0]) == float(np.float32(3.4e38)) and int(face[0, 0]) == 0 and int(kind[0, 0]) == 0
    assert float(d2[0, 1]) == float(np.float32(3.4e38)) and int(face[0, 1]) == 0 and int(kind[0, 1]) == 0
    for bad in (nan, inf, -inf):                                          # a referenced vertex, then an unreferenced one
        bv = tv.clone()
        bv[0, 5, 1] = bad
        _assert_grid_equals_brute(tp, bv, tf, 'vertex %r' % bad)
        bv = torch.cat([tv, torch.tensor([[[0.0, bad, 0.0]]])], 1)
        _assert_grid_equals_brute(tp, bv, tf, 'unreferenced vertex %r' % bad)


@pytest.mark.gpu
def test_int64_faces_and_non_contiguous_inputs():
    tp, tv, tf = _batch(12, 500, 2)
    want = _assert_grid_equals_brute(tp, tv, tf, 'int64 faces')
    assert tf.dtype == torch.int64
    got = _assert_grid_equals_brute(tp, tv, tf.int(), 'int32 faces')
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    p_nc = tp.cuda().transpose(1, 2).contiguous().transpose(1, 2)        # (B, P, 3) view of a (B, 3, P) buffer
    v_nc = torch.cat([tv, tv], 2).cuda()[:, :, :3]                       # row stride 6
    f_nc = torch.cat([tf, tf], 1).cuda()[:, :3]
    assert not p_nc.is_contiguous() and not v_nc.is_contiguous() and not f_nc.is_contiguous()
    got = metrics.point_to_mesh_distance(p_nc, v_nc, f_nc, search='grid')
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_batch_slicing_of_the_launch_limit_applies_to_the_grid_search(monkeypatch):
    tp, tv, tf = _batch(13, 400, 2)
    want = _assert_grid_equals_brute(tp, tv, tf, 'one launch')
    monkeypatch.setattr(metrics, '_MAX_GRID_Y', 1)
    got = metrics.point_to_mesh_distance(tp.cuda(), tv.cuda(), tf.cuda(), search='grid')
    assert all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_point2mesh_loss_with_the_grid_search_equals_brute_bit_for_bit_and_is_deterministic():
    from geniconet_amd import data
    from geniconet_amd.losses import Point2Mesh_Loss
    R, B = 3, 3
    x, _ = data.synthetic_batch(B, R, seed=3, device='cuda')
    _, v, f = _case(14, 60, R)
    ref_v = (torch.from_numpy(v)[None].repeat(B, 1, 1) * torch.tensor([0.8, 0.9, 1.0])[:, None, None]).cuda()
    ref_f = torch.from_numpy(f).cuda()

    def run(search):
        inp, ref = x.clone().requires_grad_(True), ref_v.clone().requires_grad_(True)
        loss = Point2Mesh_Loss(R, search=search)(inp, ref, ref_f)
        loss.backward()
        return loss.detach(), inp.grad, ref.grad
    brute, grid, again = run('brute'), run('grid'), run('grid')
    assert float(grid[1].abs().max()) > 0 and float(grid[2].abs().max()) > 0
    for a, b, c in zip(brute, grid, again):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(b), _bits(c))
    # the autograd function itself: same saved (face, kind), same outputs
    tp, tv, tf = _batch(15, 600, 2)
    pg = tp.cuda().requires_grad_(True)
    d, face, kind = metrics.point_to_mesh_distance(pg, tv.cuda(), tf.cuda(), search='grid')
    d0, face0, kind0 = metrics.point_to_mesh_distance(tp.cuda(), tv.cuda(), tf.cuda(), search='brute')
    assert d.requires_grad and not face.requires_grad
    assert torch.equal(d.detach(), d0) and torch.equal(face, face0) and torch.equal(kind, kind0)


@pytest.mark.gpu
def test_grid_forward_is_legal_inside_a_graph_capture_and_the_replay_equals_the_eager_result():
    """No allocation and no synchronisation inside the library: the forward (workspace from torch's allocator, one memset and five
    launches) is captured after an eager warm-up; replays on new inputs in the static buffers equal the eager results."""
    tp, tv, tf = _batch(16, 900, 3)
    pts, vts, f32 = tp.cuda().contiguous(), tv.cuda().contiguous(), tf.cuda().int().contiguous()
    eager = metrics._hip_point_to_mesh(pts, vts, f32, 'grid')            # warm-up: the library is loaded, the kernels are resident
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode='thread_local'):
        out = metrics._hip_point_to_mesh(pts, vts, f32, 'grid')
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, eager))
    pts.add_(0.05)                                                       # new inputs at the captured addresses
    vts.mul_(1.03)
    graph.replay()
    torch.cuda.synchronize()
    want = metrics._hip_point_to_mesh(pts, vts, f32, 'brute')
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(out, want))
    assert _lib.device_status() == 0
