"""Solid voxelisation by ray parity and the voxel IoU (metrics.voxelize, voxel_lattice, volumetric_iou(method='voxel');
icn_mesh_voxelize).

The definition (metrics.voxelize, include/icn_voxel.h) is written a third time here, as plain Python loops over float64 values of the
fp32 inputs (`reference`), and the generalised winding number of tests/test_signed_distance.py stands beside it as INDEPENDENT TRUTH: a
cell is inside iff w > 1/2 at its centre.  Everything is compared exactly -- torch.equal, every cell -- and no cell is set aside as "on
the surface": the definition decides those (the lattice-aligned cube), and the inputs compared with the winding number have no centre
there.  The one tolerance is in the comparison with `contains` on the device, whose fp32 search may turn a sign within 1e-5 of the
surface; the cells set aside that way are counted and capped.  On the GPU the kernel must equal the float64 formulation byte for
byte over meshes, lattices and batches chosen at the edges of its tiles: 16 x 16 columns, 256 staged faces, 32 parity bits a word."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import geometry, metrics

from test_signed_distance import _mesh, _profiled, winding


# ---- the reference: the definition in plain loops -----------------------------------------------------------------------------------
def _sign(x):
    return (x > 0) - (x < 0)


def _edge(iu, iw, u, w, py, pz):
    """(s, t) of the directed edge u -> w at the column (py, pz)."""
    swapped = not iu < iw
    a, b = (w, u) if swapped else (u, w)
    dy, dz = b[1] - a[1], b[2] - a[2]
    s = dy * (pz - a[2]) - dz * (py - a[1])
    t = _sign(s) or _sign(-dz) or _sign(dy)
    return (-s, -t) if swapped else (s, t)


def reference(vertices, faces, origin, h, counts):
    """bool (n0, n1, n2) of one mesh: the definition on Python floats (IEEE doubles, no fused multiply-add) of the fp32 inputs."""
    v32 = np.asarray(vertices).astype(np.float32)
    v = v32.astype(np.float64).tolist()
    n0, n1, n2 = counts
    V = len(v)
    usable = []
    for ids in np.asarray(faces).astype(np.int64).tolist():
        if all(0 <= i < V for i in ids) and all(math.isfinite(c) for i in ids for c in v[i]):
            lo, hi = v32[ids].min(0).astype(np.float64).tolist(), v32[ids].max(0).astype(np.float64).tolist()
            usable.append((ids, [v[i] for i in ids], lo, hi))
    out = np.zeros((n0, n1, n2), dtype=bool)
    for j, k in itertools.product(range(n1), range(n2)):
        py, pz = origin[1] + (j + 0.5) * h, origin[2] + (k + 0.5) * h
        flips = [0] * (n0 + 1)
        for (i0, i1, i2), (p0, p1, p2), lo, hi in usable:
            if not (lo[1] <= py <= hi[1] and lo[2] <= pz <= hi[2]):
                continue
            (s0, t0), (s1, t1), (s2, t2) = _edge(i1, i2, p1, p2, py, pz), _edge(i2, i0, p2, p0, py, pz), _edge(i0, i1, p0, p1, py, pz)
            if not (t0 > 0 and t1 > 0 and t2 > 0) and not (t0 < 0 and t1 < 0 and t2 < 0):
                continue
            den = s0 + s1 + s2
            num = s0 * p0[0] + s1 * p1[0] + s2 * p2[0]
            if den == 0:                                                      # x is infinite or NaN, and so is tau: dropped
                continue
            x = num / den
            tau = (x - origin[0]) / h - 0.5
            if math.isfinite(tau):
                flips[min(max(math.ceil(tau), 0), n0)] += 1
        crossings = 0
        for i in range(n0):
            crossings += flips[i]
            out[i, j, k] = crossings % 2 == 1
    return out


# ---- the meshes and the lattices ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sphere(r, sigma=0.0, seed=0, shift=0.0):
    """(vertices fp32 (V, 3), faces (F, 3)) tensors of the level-r icosphere with radial noise of `sigma`, moved by `shift`."""
    v, f = geometry.get_icosahedral_grid(r)
    if sigma:
        v = v * (1 + sigma * np.random.default_rng(seed).standard_normal((len(v), 1)))
    return torch.from_numpy((v + shift).astype(np.float32)), torch.from_numpy(np.asarray(f))


def _named(name):
    """A mesh of tests/test_signed_distance.py as fp32 / int64 tensors."""
    v, f = _mesh(name)
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(np.asarray(f))


def _own_lattice(v, resolution):
    return metrics.voxel_lattice(v, v, resolution)


def _centres(origin, h, counts):
    axes = [origin[k] + (np.arange(counts[k]) + 0.5) * h for k in range(3)]
    return np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3)


def _inside_by_winding(v, f, origin, h, counts):
    """bool (n0, n1, n2): w > 1/2 at every centre by `winding` of tests/test_signed_distance.py, and the smallest |w - 1/2|."""
    c = _centres(origin, h, counts)
    w = np.concatenate([winding(c[lo:lo + 2048], v.numpy(), f.numpy()) for lo in range(0, len(c), 2048)])
    return (w > 0.5).reshape(counts), float(np.abs(w - 0.5).min())


# ---- CPU 1: the three statements of the definition -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('tetrahedron', 'cube', 'spike', 'noisy I1'))
def test_torch_formulation_equals_the_definition_in_plain_loops(name):
    v, f = _sphere(1, 0.1, seed=1) if name == 'noisy I1' else _named(name)
    for resolution in ((25, 32) if name == 'spike' else (5, 8)):                          # (the spike is narrow: 0.3 across, 2 long)
        origin, h, counts = metrics.voxel_lattice(v, 1.25 * v + 0.07, resolution)         # the box of the mesh and a margin
        got = metrics._torch_voxelize(v[None], f, origin, h, counts)
        assert got.dtype == torch.bool and got.shape == (1,) + counts
        want = reference(v, f, origin, h, counts)
        assert torch.equal(got[0], torch.from_numpy(want)), name
        assert want.any() and not want.all()
        assert torch.equal(metrics.voxelize(v[None], f, origin, h, counts), got)
    # one face chunk or many: the same cells
    assert torch.equal(metrics._torch_voxelize(v[None], f, origin, h, counts, cells=1), got)


# ---- CPU 2: the lattice-aligned cube, where the tie rule decides -----------------------------------------------------------------------
ALIGNED = ((-0.375,) * 3, 0.25, (7, 7, 7))


def _cells_1_to_4():
    want = torch.zeros(7, 7, 7, dtype=torch.bool)
    want[1:5, 1:5, 1:5] = True
    return want


def test_the_aligned_cube_fills_exactly_the_cells_one_to_four_on_every_axis():
    v, f = _named('cube')
    got = metrics.voxelize(v[None], f, *ALIGNED)[0]
    assert int(got.sum()) == 64 and torch.equal(got, _cells_1_to_4())
    assert np.array_equal(reference(v, f, *ALIGNED), _cells_1_to_4().numpy())


def test_the_aligned_cube_under_relabelled_vertices_permuted_faces_and_flipped_windings():
    v, f = _named('cube')
    g = torch.Generator().manual_seed(6)
    for trial in range(6):
        label = torch.randperm(8, generator=g)                                # old id -> new id
        vv = torch.empty_like(v)
        vv[label] = v
        ff = label[f][torch.randperm(12, generator=g)]
        flip = torch.rand(12, generator=g) < (0.0, 0.5, 1.0)[trial % 3]        # none, a subset, all wound the other way
        ff = torch.where(flip[:, None], ff.flip(1), ff)
        assert torch.equal(metrics.voxelize(vv[None], ff, *ALIGNED)[0], _cells_1_to_4()), trial
    for mask in range(0, 1 << 12, 37):                                        # any subset of faces wound the other way
        flip = torch.tensor([(mask >> k) & 1 for k in range(12)], dtype=torch.bool)
        assert torch.equal(metrics.voxelize(v[None], torch.where(flip[:, None], f.flip(1), f), *ALIGNED)[0], _cells_1_to_4()), mask


# ---- CPU 3: truth by winding number ----------------------------------------------------------------------------------------------------
WINDING_CASES = {'I%d on [-1, 1]^3 at %d' % (r, n): (r, 0.0, 0, 0.0, n) for r in (0, 1, 2) for n in (7, 9, 15)}
WINDING_CASES.update({'noisy I2 at 32': (2, 0.1, 0, 0.0, 32), 'noisy shifted I3 at 24': (3, 0.05, 0, 0.3, 24), 'very noisy I2 at 17': (2, 0.3, 3, 0.0, 17)})


@pytest.mark.parametrize('case', list(WINDING_CASES))
def test_no_cell_disagrees_with_the_winding_number(case):
    r, sigma, seed, shift, resolution = WINDING_CASES[case]
    v, f = _sphere(r, sigma, seed, shift)
    origin, h, counts = _own_lattice(v, resolution) if sigma else ((-1.0,) * 3, 2.0 / resolution, (resolution,) * 3)
    truth, margin = _inside_by_winding(v, f, origin, h, counts)
    got = metrics.voxelize(v[None], f, origin, h, counts)[0].numpy()
    print('%s: %d of %d cells inside, %d disagree, smallest |w - 1/2| %.3g' % (case, truth.sum(), truth.size, (got != truth).sum(), margin))
    assert margin > 1e-6                                                      # no centre on the surface: nothing is set aside
    assert np.array_equal(got, truth)
    assert truth.any() and not truth.all()


@pytest.mark.parametrize('r', (2, 3))
def test_occupied_volume_is_the_mesh_volume_within_the_derived_bound(r):
    """A misclassified cell has its centre within h sqrt(3) / 2 of the surface: |count h^3 - volume| <= sqrt(3) area h."""
    v, f = _sphere(r)
    area, volume = (float(x) for x in metrics.mesh_area_volume(v[None], f))
    origin, h, counts = _own_lattice(v, 16)
    got = float(metrics.voxelize(v[None], f, origin, h, counts).sum()) * h ** 3
    print('I%d: occupancy %.4f volume %.4f, error %.2g, bound %.2g' % (r, got, volume, abs(got - volume), math.sqrt(3) * area * h))
    assert abs(got - volume) <= math.sqrt(3) * area * h


# ---- CPU 4: volumetric_iou ---------------------------------------------------------------------------------------------------------------
PARENT_IOU_I2_PAIR_32 = 0.7261560693641619        # volumetric_iou(0.9 v, v, f, resolution=32) of the level-2 icosphere before `method` existed


def test_voxel_iou_of_cubes_is_exact_and_the_default_method_is_unchanged():
    v, f = _named('cube')
    shifted = v + torch.tensor([0.5, 0.0, 0.0])
    assert metrics.volumetric_iou(v, shifted, f, resolution=48, method='voxel') == 16384 / 49152
    assert metrics.volumetric_iou(v, v, f, resolution=8, method='voxel') == 1.0
    assert metrics.volumetric_iou(v, v + 2.0, f, resolution=12, method='voxel') == 0.0
    assert metrics.volumetric_iou(v.double(), shifted.double(), f.int(), resolution=24, method='voxel') == 1 / 3
    # the default is today's path, and returns what it returned
    assert metrics.volumetric_iou(v, shifted, f, resolution=48) == 16384 / 49152
    for kwargs in ({}, dict(method='search')):
        assert metrics.volumetric_iou(v, v, f, resolution=8, **kwargs) == 1.0
        assert metrics.volumetric_iou(v, v + 2.0, f, resolution=12, **kwargs) == 0.0
    s, sf = _sphere(2)
    assert metrics.volumetric_iou(0.9 * s, s, sf, resolution=32) == PARENT_IOU_I2_PAIR_32
    origin, h, counts = metrics.voxel_lattice(0.9 * s, s, 32)
    voxel = metrics.volumetric_iou(0.9 * s, s, sf, resolution=32, method='voxel')
    area, volume = (float(x) for x in metrics.mesh_area_volume(s[None], sf))
    assert abs(voxel - 0.9 ** 3) <= math.sqrt(3) * area * h / volume


def test_voxel_lattice_is_the_lattice_of_volumetric_iou():
    v, f = _named('cube')
    origin, h, counts = metrics.voxel_lattice(v, v + torch.tensor([0.5, 0.0, 0.0]), 48)
    assert origin == (0.0, 0.0, 0.0) and h == 1.5 / 48 and counts == (48, 32, 32)
    assert all(isinstance(o, float) for o in origin) and all(isinstance(n, int) for n in counts)
    for args in ((v[None], v[None], 8), (v, v[:7], 8), (v, v, 0), (v * 0, v * 0, 8), (v * float('nan'), v, 8)):
        with pytest.raises(ValueError):
            metrics.voxel_lattice(*args)


def test_an_unknown_method_raises():
    v, f = _named('cube')
    for method in ('voxels', 'brute', None):
        with pytest.raises(ValueError, match='method must be one of'):
            metrics.volumetric_iou(v, v, f, method=method)
    with pytest.raises(ValueError):
        metrics.volumetric_iou(v, v, f, method='voxel', search='tree')


# ---- CPU 5: rejected input ------------------------------------------------------------------------------------------------------------------
def test_open_meshes_are_refused_by_the_checked_function_only():
    v, f = _named('cube')
    lattice = _own_lattice(v, 6)
    with pytest.raises(ValueError, match=r'not closed: the edge \(\d+, \d+\) belongs to an odd number of faces \(3 such edges\)'):
        metrics.voxelize(v[None], f[:-1], *lattice)
    with pytest.raises(ValueError, match=r'not closed: the edge \(0, 1\)'):
        metrics.voxelize(v[None], f[:1], *lattice)
    with pytest.raises(ValueError, match='not closed'):
        metrics.volumetric_iou(v, v, f[:-1], method='voxel')
    # the unchecked form gives what the definition gives: without face 0, which lies across the rays, the columns through it are wrong
    got = metrics._voxelize_unchecked(v[None], f[1:].int(), *lattice)
    assert torch.equal(got[0], torch.from_numpy(reference(v, f[1:], *lattice)))
    assert not torch.equal(got, metrics.voxelize(v[None], f, *lattice))
    # a face twice closes nothing and opens nothing: every edge stays even
    assert torch.equal(metrics.voxelize(v[None], torch.cat([f, f[:2], f[:2]]), *lattice), metrics.voxelize(v[None], f, *lattice))


def test_bad_arguments_raise():
    v, f = _named('cube')
    origin, h, counts = _own_lattice(v, 4)
    ok = (v[None], f, origin, h, counts)
    assert metrics.voxelize(*ok).shape == (1, 4, 4, 4)
    for k, bad in ((0, v), (0, v[None, :, :2]), (0, v[None].long()), (0, v[None][:0]), (1, f[:, :2]), (1, f[:0]), (1, f.float()), (1, f == 0),
                   (2, origin[:2]), (2, (0.0, float('nan'), 0.0)), (2, 'abc'), (3, 0.0), (3, -1.0), (3, float('inf')), (3, float('nan')),
                   (3, None), (4, (4, 4)), (4, (4, 0, 4)), (4, (4, 4, -1)), (4, (4, 4.5, 4)), (4, 4)):
        args = list(ok)
        args[k] = bad
        with pytest.raises(ValueError):
            metrics.voxelize(*args)
    with pytest.raises(IndexError):
        metrics.voxelize(v[None], f + 1, origin, h, counts)
    with pytest.raises(IndexError):
        metrics.voxelize(v[None, :7], f, origin, h, counts)
    assert metrics.voxelize(v[None].double(), f.int(), origin, h, (4.0, 4, 4)).shape == (1, 4, 4, 4)


def _broken_cube():
    """The cube with three faces that must contribute nothing: one at a NaN vertex, one with an id out of range, one without area
    (and, for the checked function, one with coincident ids)."""
    v, f = _named('cube')
    v = torch.cat([v, torch.tensor([[float('nan'), 0.5, 0.5], [0.5, 0.5, 0.5]])])                  # vertices 8 (NaN) and 9
    extra = torch.tensor([[0, 8, 3], [1, 2, 10], [0, 7, 7], [0, 9, 9], [5, 5, 5]])
    return v, f, extra


def test_a_nan_vertex_an_id_out_of_range_and_a_face_without_area_contribute_nothing():
    v, f, extra = _broken_cube()
    lattice = ((-0.21, -0.13, -0.17), 0.11, (13, 12, 13))
    plain = metrics._torch_voxelize(v[None], f, *lattice)
    assert plain.any() and not plain.all()
    got = metrics._voxelize_unchecked(v[None], torch.cat([extra, f, extra]).int(), *lattice)
    assert torch.equal(got, plain)
    assert torch.equal(got[0], torch.from_numpy(reference(v, torch.cat([extra, f, extra]), *lattice)))
    # the checked function lets the faces with coincident ids through (their edges close on themselves) and a NaN vertex nobody uses
    assert torch.equal(metrics.voxelize(v[None], torch.cat([f, extra[2:]]), *lattice), plain)
    assert torch.equal(metrics.voxelize(v[None], f, *ALIGNED)[0], _cells_1_to_4())
    # a face of three positions on a line, distinct ids
    v2 = torch.cat([v[:8], torch.tensor([[0.5, 0.5, 0.5], [0.25, 0.25, 0.25], [0.75, 0.75, 0.75]])])
    line = torch.tensor([[8, 9, 10], [10, 9, 8]])
    assert torch.equal(metrics.voxelize(v2[None], torch.cat([f, line]), *lattice), plain)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------
SCALES = ((1.0, 0.0), (1.1, 0.05), (0.9, -0.03))                              # the batch of three: the mesh scaled and moved


@functools.lru_cache(maxsize=None)
def _gpu_mesh(name):
    """(vertices (3, V, 3) fp32, faces (F, 3) int32) on the CPU: the mesh at SCALES.  The open meshes 'F255', 'F256', 'F257' are the
    first faces of the noisy I2 (one staging tile of the kernel, one face less and one more), 'broken' is _broken_cube."""
    if name == 'broken':
        v, f, extra = _broken_cube()
        f = torch.cat([extra, f, extra])
    elif name[0] == 'F':
        v, f = _sphere(2, 0.1)
        f = f[:int(name[1:])]
    elif name[0] == 'I':
        v, f = _sphere(int(name[1:]), 0.1, seed=int(name[1:]))
    else:
        v, f = _named(name)
    return torch.stack([v * s + t for s, t in SCALES]), f.int()


def _lattices(group, v):
    """name -> (origin, h, counts) about the first mesh of the batch (its finite vertices)."""
    p = v[0][torch.isfinite(v[0]).all(-1)].double()
    lo, hi = p.amin(0), p.amax(0)
    mid, ext = ((lo + hi) / 2).tolist(), (hi - lo).tolist()

    def centred(counts, h):
        return tuple(mid[k] - counts[k] * h / 2 for k in range(3)), h, counts

    def over_yz(counts):                                                      # covers the mesh in y and z, whatever that makes of x
        return centred(counts, 1.1 * max(ext[1] / counts[1], ext[2] / counts[2]))
    if group == 'depth':                                                      # the word boundaries of the parity bits
        out = {str(n0): centred((n0, 5, 7), 1.1 * ext[0] / n0) for n0 in (31, 32, 33, 64, 65, 512)}
        out['one cell'] = centred((1, 1, 1), 1.1 * max(ext))
        return out
    if group == 'sides':                                                      # one column past a tile of 16 x 16 in each direction
        return {'%d x %d' % (n1, n2): over_yz((3, n1, n2)) for n1 in (1, 15, 16, 17, 33) for n2 in (1, 15, 16, 17, 33)}
    assert group == 'placement'
    half = centred((8, 16, 16), 1.1 * max(ext) / 16)
    return {'many times larger': centred((20, 20, 20), 4 * max(ext) / 20),    # the mesh in a few cells in the middle
            'inside the mesh': centred((4, 9, 9), max(ext) / 16),             # every crossing clamps, at 0 or at n0
            'half the mesh': ((mid[0],) + half[0][1:],) + half[1:],           # the crossings before it clamp at 0
            'aligned': ALIGNED}                                               # on the cube every tie fires


GPU_MESHES = ('tetrahedron', 'cube', 'spike', 'I1', 'I2', 'I3', 'F255', 'F256', 'F257', 'broken')


@functools.lru_cache(maxsize=None)
def _float64_case(name, group):
    """The float64 formulation on the CPU for every lattice of the group: computed once, shared, never changed."""
    v, f = _gpu_mesh(name)
    return {key: (lattice, metrics._torch_voxelize(v, f, *lattice)) for key, lattice in _lattices(group, v).items()}


@pytest.mark.gpu
@pytest.mark.parametrize('group', ('depth', 'sides', 'placement'))
@pytest.mark.parametrize('name', GPU_MESHES)
def test_hip_equals_the_float64_formulation_byte_for_byte(name, group):
    v, f = _gpu_mesh(name)
    vc, fc = v.cuda(), f.cuda()
    filled = 0
    for key, (lattice, want) in _float64_case(name, group).items():
        for B in (1, 3):
            got = metrics._voxelize_unchecked(vc[:B], fc, *lattice)
            assert got.is_cuda and got.dtype == torch.bool and got.shape == (B,) + tuple(lattice[2])
            assert torch.equal(got.view(torch.uint8).cpu(), want[:B].to(torch.uint8)), (name, key, B)
        filled += int(want.sum())
    assert filled > 0


SEAMS = (0, 63, 64, 65, 127, 128, 255, 256, 257, 319)                         # the ends of the waves of a staging tile, and of the tile


@functools.lru_cache(maxsize=None)
def _seam_mesh():
    """(vertices (3, V, 3), faces (320, 3) int32, the indices of the faces left valid): the noisy I2 -- one full staging tile of the
    kernels that sweep all faces and a partial one -- with the faces at SEAMS made invalid, in turn by an id outside [0, V) (-1, then
    V) and by a reference to the appended vertex V - 1, which is NaN and which no other face uses."""
    v, f = _gpu_mesh('F320')
    v = torch.cat([v, torch.full((len(SCALES), 1, 3), float('nan'))], 1)
    V, f = v.shape[1], f.clone()
    assert len(f) == 320 and int(f.max()) == V - 2
    for n, i in enumerate(SEAMS):
        f[i, n % 3] = V - 1 if n % 2 else (-1, V)[n // 2 % 2]
    return v, f, torch.tensor([i for i in range(len(f)) if i not in SEAMS])


@functools.lru_cache(maxsize=None)
def _seam_case():
    """(lattice of (33, 17, 18) cells over the first mesh, the float64 formulation on the face list of _seam_mesh, the same on the list
    without its ten invalid faces): computed once, shared, never changed."""
    v, f, kept = _seam_mesh()
    counts = (33, 17, 18)
    lo, hi = (x.double() for x in v[0, :-1].aminmax(dim=0))
    h = 1.1 * float(((hi - lo)[1:] / torch.tensor(counts[1:])).max())
    lattice = (tuple(float((lo + hi)[k]) / 2 - counts[k] * h / 2 for k in range(3)), h, counts)
    return lattice, metrics._torch_voxelize(v, f, *lattice), metrics._torch_voxelize(v, f[kept], *lattice)


def test_invalid_faces_on_the_seams_of_a_staging_tile_are_faces_removed_in_the_float64_formulation():
    """An invalid face is not TESTED: by the definition alone the list with it equals the list without it."""
    lattice, want, without = _seam_case()
    assert want.shape == (3, 33, 17, 18) and want.any() and not want.all()
    assert torch.equal(want, without)


@pytest.mark.gpu
def test_hip_with_invalid_faces_on_the_seams_of_a_staging_tile():
    """The compaction of the staged tile with holes at both ends of every wave and of the tile: the float64 formulation byte for byte,
    and the bytes of the face list without those faces."""
    v, f, kept = _seam_mesh()
    lattice, want, _ = _seam_case()
    vc = v.cuda()
    got = metrics._voxelize_unchecked(vc, f.cuda(), *lattice)
    assert torch.equal(got.view(torch.uint8).cpu(), want.to(torch.uint8))
    assert torch.equal(got, metrics._voxelize_unchecked(vc, f[kept].cuda(), *lattice))


@pytest.mark.gpu
def test_hip_on_the_closed_meshes_through_the_checked_function_and_the_aligned_cube():
    v, f = _gpu_mesh('cube')
    got = metrics.voxelize(v.cuda()[:1], f.cuda(), *ALIGNED)
    assert torch.equal(got[0].cpu(), _cells_1_to_4())
    for name in ('spike', 'I2'):
        v, f = _gpu_mesh(name)
        key, (lattice, want) = next(iter(_float64_case(name, 'placement').items()))
        assert torch.equal(metrics.voxelize(v.cuda(), f.long().cuda(), *lattice).cpu(), want)
    with pytest.raises(ValueError, match='not closed'):
        metrics.voxelize(v.cuda(), f[:-1].cuda(), *lattice)
    with pytest.raises(ValueError, match='HIP path takes at most'):
        metrics.voxelize(v.cuda(), f.cuda(), lattice[0], lattice[1], (513, 4, 4))


@pytest.mark.gpu
def test_batch_slicing_determinism_and_one_launch_per_slice(monkeypatch):
    v, f = _gpu_mesh('I2')
    vc, fc = v.cuda(), f.cuda()
    lattice = _lattices('sides', v)['17 x 33']

    def run():
        return metrics._voxelize_unchecked(vc, fc, *lattice)
    whole, kernels = _profiled(run)
    assert kernels == {'k_mesh_voxelize': 1}
    assert torch.equal(run(), whole)                                          # bit-identical run to run
    for limit, launches in ((2, 2), (1, 3)):
        monkeypatch.setattr(metrics, '_MAX_GRID_Y', limit)
        sliced, kernels = _profiled(run)
        assert kernels == {'k_mesh_voxelize': launches}
        assert torch.equal(sliced, whole)


@pytest.mark.gpu
def test_no_host_synchronisation_in_the_unchecked_call():
    v, f = _gpu_mesh('I2')
    vc, fc = v.cuda(), f.cuda()
    lattice = _lattices('placement', v)['half the mesh']
    want = metrics._voxelize_unchecked(vc, fc, *lattice)                      # the allocator settles
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
            got = metrics._voxelize_unchecked(vc, fc, *lattice)
    finally:
        torch.cuda.set_sync_debug_mode(previous)
    assert caught, "torch.cuda.set_sync_debug_mode('error') does not catch a deliberate .item() on this build"
    assert torch.equal(got, want)


@pytest.mark.gpu
def test_against_contains_on_the_device():
    """Cells may differ from the fp32 signed distance only where |phi| <= 1e-5, and at most 1 % of the cells may be set aside so."""
    v, f = _sphere(2, 0.1)
    origin, h, counts = _own_lattice(v, 32)
    vc, fc = v.cuda()[None], f.cuda()
    got = metrics.voxelize(vc, fc, origin, h, counts)
    centres = torch.from_numpy(_centres(origin, h, counts)).float().cuda()[None]
    phi = metrics.signed_point_to_mesh_distance(centres, vc, fc)[0].reshape(got.shape)
    aside = phi.abs() <= 1e-5
    print('%d cells, %d inside, %d set aside, %d differ' % (got.numel(), int(got.sum()), int(aside.sum()), int((got != (phi < 0)).sum())))
    assert int(aside.sum()) <= 0.01 * got.numel()
    assert torch.equal(got[~aside], (phi < 0)[~aside])
    assert torch.equal(got.cpu(), metrics.voxelize(v[None], f, origin, h, counts))


@pytest.mark.gpu
def test_voxel_iou_on_the_device_is_the_cpu_value():
    v, f = _named('cube')
    for other, resolution in ((v + torch.tensor([0.5, 0.0, 0.0]), 48), (v, 8), (v + 2.0, 12)):
        want = metrics.volumetric_iou(v, other, f, resolution=resolution, method='voxel')
        assert metrics.volumetric_iou(v.cuda(), other.cuda(), f.cuda(), resolution=resolution, method='voxel') == want
        assert want == {48: 16384 / 49152, 8: 1.0, 12: 0.0}[resolution]
    s, sf = _sphere(2)
    want = metrics.volumetric_iou(0.9 * s, s, sf, resolution=32, method='voxel')
    assert metrics.volumetric_iou(0.9 * s.cuda(), s.cuda(), sf.cuda(), resolution=32, method='voxel') == want
