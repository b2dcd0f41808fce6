"""The area-weighted sampler (geniconet_amd.sampling, icn_mesh_sample_fwd / icn_mesh_sample_bwd) on degenerate, thin and mixed-area
meshes, against numpy float64 computed from the same fp32 vertices and uniforms.  Without a GPU the torch formulation runs on every
family; the tests marked gpu run the HIP kernels on the same cases and read the kernels' own CDF out of the caller's workspace
(include/icn.h: after icn_mesh_sample_fwd its first 8 B F bytes hold c as (B, F) doubles), `_hip_sample_cdf`.

Families, every one with B = 2 meshes of different content:
  soup        20 faces with private vertices, every kind twice in interleaved order (zero-area faces first, last and as a run in the
              middle): v1 = v0, v2 = v0, v1 = v2, all three equal (triangles of tests/test_point_to_mesh_shapes.py), collinear but
              distinct, well shaped, thin at aspect ratio 10, 1e2, 1e3, 1e4; at coordinate scales 1e-3, 1, 1e3, centred and shifted by
              scale * (3, 2, 1).  The collinear faces are built on a binary lattice of the scaled frame, so they are collinear exactly
              in fp32 at every scale and shift: a collinear face that is off the line by one rounding has an area of about 2^-25 of
              its neighbours', which would take the mesh beyond the limit 2^29 / F up to which the header promises an exact scan.
  degenerate  every face (i, j, j) or (i, i, j) on distinct positions: T = 0, every sample takes face 0
  strip       F right triangles with legs s_f / 2, s_f small integers (area s_f^2 / 8), one face padded to legs 1 / 2 and q / 2 so that
              8 T is a power of two: every c_f is an integer / 8 and u0 = c_f / T is exact in fp32.  F straddles the scan's wave (64)
              and tile (1024); the second variant has runs of s_f = 0 across f = 64, f = 1024, at the start and at the end.
  mixed       F = 64 random triangles whose areas span a ratio of 2^12 (inside the limit) and of 2^40 (beyond it: range, finiteness
              and T to F double ulps only)
  p2m shapes  every triangle family of tests/test_point_to_mesh_shapes.py as single-face meshes: areas only

Uniforms: u0 = (k + 0.5) / 4096 stratified, then hand-placed u0 = 0, 1, 1 - 2^-24 and c_f / T for at least 32 faces (on the strip: the
faces around every zero-area run), the hand-placed ones with (u1, u2) on the corners (0, x), (1, 0), (1, 1).

Checks (`_check`), on the CDF and areas OF THE PATH UNDER TEST (c_dev; A_dev from single-face meshes, which no scan touches):
  diff(c_dev) >= 0, fp32 values, equal to A_dev;  c_dev[f] == math.fsum(A_dev[: f + 1]);  A_dev == 0 on coincident vertices;
  |A_dev - A_64| <= 6 * 2^-24 |a|_64 |e|_64 otherwise (a, e the edge vectors from v0; first-order bound about 5, a float32
  restatement stays below 1.64);  face == searchsorted(c_dev, float64(u0) T, 'right') with the u0 = 1 rule, for every sample;
  the stratified samples per face within 1 of 4096 (c_f - c_{f-1}) / T;  points within 16 * 2^-24 M of float64 on the same face,
  weights >= 0, sum within 4 * 2^-24 of 1, each weight within 4 * 2^-24 of float64 (at most three roundings of numbers <= 1);
  corner uniforms give a unit weight vector and the vertex itself.

Worst |A - A_64| / (2^-24 |a||e|) and the samples checked exactly are printed per case (lines starting RECORD) and kept in
profiles/surface_sample_shapes.txt."""
import functools
import math

import numpy as np
import pytest
import torch

from geniconet_amd import _lib, data, geometry, losses, sampling

from test_point_to_mesh_shapes import _triangles
from test_surface_samples import _ref64

U24 = 2.0 ** -24
NB = 2
STRATA = 4096
AREA_BOUND = 6.0
SCALES = (1e-3, 1.0, 1e3)
STRIP_FACES = (63, 64, 65, 1023, 1024, 1025, 2049, 3073)
CORNERS = ((0.0, 0.3), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.25, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0))
KINDS = ('v1=v0', 'well', 'thin 1e1', 'v2=v0', 'collinear', 'thin 1e2', 'v1=v2', 'thin 1e3', 'all', 'thin 1e4',
         'well', 'v1=v2', 'v1=v0', 'thin 1e4', 'collinear', 'thin 1e1', 'thin 1e3', 'thin 1e2', 'v2=v0', 'all')
COINCIDENT = {'v1=v0': 0, 'v1=v2': 1, 'v2=v0': 2, 'all': 3}              # -> i % 4 of _triangles()['coincident']


# ---- float64 ---------------------------------------------------------------------------------------------------------------------
def _areas64(v, f):
    """float64 A_f (B, F) and |a| |e| (B, F) of fp32 vertices v (B, V, 3) tensor / faces f (F, 3) tensor."""
    tri = v.double().numpy()[:, f.numpy()]                                  # (B, F, 3, 3)
    a, e = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
    return 0.5 * np.linalg.norm(np.cross(a, e), axis=-1), np.linalg.norm(a, axis=-1) * np.linalg.norm(e, axis=-1)


def _coincident(v, f):
    """(B, F) bool: two or three vertices of the face are the same position."""
    tri = v.numpy()[:, f.numpy()]
    same = lambda i, j: (tri[:, :, i] == tri[:, :, j]).all(-1)
    return same(0, 1) | same(0, 2) | same(1, 2)


def _prefix_fsum(areas):
    """math.fsum(areas[: f + 1]) for every f, for fp32-valued doubles, in O(F): the prefix sums as exact integers in units of 2^-149
    (the smallest fp32 subnormal), each rounded to double once, which is what fsum returns."""
    out, total = np.empty(len(areas)), 0
    for i, a in enumerate(areas):
        scaled = math.ldexp(float(a), 149)
        assert scaled == int(scaled)
        total += int(scaled)
        out[i] = math.ldexp(float(total), -149)
    assert out[-1] == math.fsum(areas) and out[len(areas) // 2] == math.fsum(areas[:len(areas) // 2 + 1])
    return out


# ---- uniforms --------------------------------------------------------------------------------------------------------------------
def _uniforms(cdf64, picks, seed):
    """(NB, STRATA + H, 3) fp32: stratified u0 with seeded (u1, u2), then the hand-placed u0 = 0, 1, 1 - 2^-24 and c_f / T for the
    faces picks[b] (computed in float64, rounded to fp32), (u1, u2) going round CORNERS.  Meshes with T = 0 get f / F instead."""
    g = torch.Generator().manual_seed(seed)
    hand = []
    for b in range(NB):
        T, F = cdf64[b, -1], cdf64.shape[1]
        at = cdf64[b, picks[b]] / T if T > 0 else np.asarray(picks[b]) / F
        hand.append(np.concatenate([[0.0, 1.0, 1.0 - U24], at]))
    H = max(len(h) for h in hand)
    u = torch.rand((NB, STRATA + H, 3), generator=g)
    u[:, :STRATA, 0] = (torch.arange(STRATA, dtype=torch.float32) + 0.5) / STRATA
    for b in range(NB):
        h = np.concatenate([hand[b], np.full(H - len(hand[b]), 0.5)])
        u[b, STRATA:, 0] = torch.from_numpy(h).float()
        for k in range(H):
            u[b, STRATA + k, 1], u[b, STRATA + k, 2] = CORNERS[k % len(CORNERS)]
    return u


# ---- the cases: dict(name, v (NB, V, 3) fp32, f (F, 3) int64, u, zero (NB, F) bool, exact) -----------------------------------------
def _soup_faces(faces):
    return torch.arange(3 * faces).reshape(faces, 3)


def _finish(name, tri, picks, seed, exact=True, **extra):
    """tri (NB, F, 3, 3) float64 -> the case, with private vertices per face."""
    v = torch.from_numpy(tri.reshape(NB, -1, 3)).float() + 0.0            # + 0.0: no negative zero among the coordinates
    f = _soup_faces(tri.shape[1])
    cdf64 = _ref64(v, f, torch.zeros(NB, 1, 3))[2]
    return dict(name=name, v=v, f=f, u=_uniforms(cdf64, picks, seed), zero=_coincident(v, f), exact=exact, **extra)


@functools.lru_cache(maxsize=None)
def _soup(scale, shifted):
    fam = _triangles()
    g = np.random.default_rng(int(round(math.log10(scale))) + 10 + 100 * shifted)
    unit = 2.0 ** (math.floor(math.log2(scale)) - 3)                         # the lattice of the collinear faces
    shift = scale * np.array([3.0, 2.0, 1.0]) * shifted
    tri = np.zeros((NB, len(KINDS), 3, 3))
    for b in range(NB):
        seen = {}
        for i, kind in enumerate(KINDS):
            j = 2 * b + seen.setdefault(kind, 0)                            # a different triangle for every (mesh, occurrence)
            seen[kind] += 1
            if kind in COINCIDENT:
                t = fam['coincident'][4 * j + COINCIDENT[kind]] * scale + shift
            elif kind == 'collinear':
                step = np.zeros(3)
                while not step.any():
                    step = g.integers(-4, 5, 3).astype(np.float64)
                base = np.round((g.uniform(-1, 1, 3) * scale + shift) / unit) * unit
                ends = [base, base + 4 * step * unit]
                ends.insert(j % 3, base + (1.0, 3.0, 8.0, -4.0)[j] * step * unit)        # between, between, beyond, before
                t = np.stack(ends)
            else:
                t = fam['well shaped' if kind == 'well' else kind][j] * scale + shift
            tri[b, i] = t
    tri = tri.astype(np.float32).astype(np.float64)
    case = _finish('soup scale=%g %s' % (scale, 'shifted' if shifted else 'centred'), tri, [np.arange(len(KINDS))] * NB, seed=3)
    kinds = np.array([k in COINCIDENT for k in KINDS])
    assert (case['zero'] == kinds).all() and (_areas64(case['v'], case['f'])[0][:, ~kinds & (np.array(KINDS) != 'collinear')] > 0).all()
    a64, ae = _areas64(case['v'], case['f'])
    assert (a64[:, np.array(KINDS) == 'collinear'] == 0).all() and (ae[:, np.array(KINDS) == 'collinear'] > 0).all()
    return case


@functools.lru_cache(maxsize=None)
def _degenerate():
    g = np.random.default_rng(5)
    v = torch.from_numpy(g.standard_normal((NB, 8, 3))).float()
    f = torch.tensor([(i % 8, (i + 3) % 8, (i + 3) % 8) if i % 2 == 0 else (i % 8, i % 8, (i + 5) % 8) for i in range(12)])
    cdf64 = np.cumsum(_areas64(v, f)[0], axis=1)
    assert (cdf64 == 0).all()
    return dict(name='only degenerate', v=v, f=f, u=_uniforms(cdf64, [np.arange(12)] * NB, seed=4), zero=_coincident(v, f), exact=True)


def _strip_sizes(F, zero_runs):
    """-> s (NB, F) ints, pad face per mesh, the runs of zero per mesh."""
    k = np.arange(F)
    s = np.stack([1 + (5 * k) % 7, 1 + (3 * k) % 5])
    runs = ([(61, 67), (1020, 1028), (F - 3, F)], [(0, 3), (60, 64), (1024, 1031)]) if zero_runs else ([], [])
    runs = [[(lo, min(hi, F)) for lo, hi in r if lo < F] for r in runs]
    for b in range(NB):
        for lo, hi in runs[b]:
            s[b, lo:hi] = 0
    return s, (7, 5), runs


@functools.lru_cache(maxsize=None)
def _strip(F, zero_runs):
    s, pad, runs = _strip_sizes(F, zero_runs)
    eighths = s * s                                                         # 8 A_f
    tri = np.zeros((NB, F, 3, 3))
    tri[:, :, :, 0] = 8.0 * np.arange(F)[None, :, None]
    tri[:, :, 1, 0] += s / 2.0
    tri[:, :, 2, 1] = s / 2.0
    picks = []
    for b in range(NB):
        rest = int(eighths[b].sum() - eighths[b, pad[b]])
        q = (1 << rest.bit_length()) - rest                                 # 8 T = the next power of two above `rest`
        eighths[b, pad[b]] = q
        tri[b, pad[b], 1, 0] = 8.0 * pad[b] + 0.5
        tri[b, pad[b], 2, 1] = q / 2.0
        total = int(eighths[b].sum())
        assert total & (total - 1) == 0 and total < 2 ** 24 and s[b, pad[b]] > 0
        near = [f for lo, hi in runs[b] for f in (lo - 2, lo - 1, lo, hi - 1, hi, hi + 1)]
        near += [62, 63, 64, 1022, 1023, 1024, 2047, 2048, F - 2, F - 1] + list(np.linspace(0, F - 1, 40).astype(int))
        picks.append(np.unique([f for f in near if 0 <= f < F]))
        assert len(picks[-1]) >= 32
    case = _finish('strip F=%d%s' % (F, ' zero runs' if zero_runs else ''), tri, picks, seed=F, eighths=eighths)
    assert (case['zero'] == (eighths == 0)).all() and (case['v'].double().numpy().reshape(NB, F, 3, 3) == tri).all()
    # what the hand-placed samples must select, from the integers alone: 0 -> the first face with an area, 1 and 1 - 2^-24 -> the last,
    # c_f / T -> the next face with an area after f (t = c_f exactly; "smallest g with c_g > t"), the last one if there is none
    hand = []
    for b in range(NB):
        pos = np.nonzero(eighths[b] > 0)[0]
        after = lambda f: pos[np.searchsorted(pos, f, side='right')] if f < pos[-1] else pos[-1]
        want = [pos[0], pos[-1], pos[-1]] + [after(f) for f in picks[b]]
        hand.append(np.array(want))
        c8 = np.cumsum(eighths[b])
        assert (case['u'][b, STRATA + 3:STRATA + 3 + len(picks[b]), 0].double().numpy() * c8[-1] == c8[picks[b]]).all()   # exact in fp32
    case['hand'] = hand
    return case


@functools.lru_cache(maxsize=None)
def _mixed(log2_ratio):
    g = np.random.default_rng(log2_ratio)
    F = 64
    tri = g.standard_normal((NB, F, 3, 3))
    a, e = tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]
    area = 0.5 * np.linalg.norm(np.cross(a, e), axis=-1)
    size = np.stack([2.0 ** (0.5 * log2_ratio * (g.permutation(F) / (F - 1) - 0.5)) for _ in range(NB)])
    centre = tri.mean(2, keepdims=True)
    tri = centre + (tri - centre) * (size / np.sqrt(area))[:, :, None, None]
    tri = tri.astype(np.float32).astype(np.float64)
    case = _finish('mixed 2^%d' % log2_ratio, tri, [np.arange(F)] * NB, seed=log2_ratio, exact=log2_ratio <= 23)   # 2^29 / 64
    a64 = _areas64(case['v'], case['f'])[0]
    assert (np.abs(np.log2(a64.max(1) / a64.min(1)) - log2_ratio) < 0.5).all()
    return case


ALL_SOUPS = [(s, sh) for s in SCALES for sh in (False, True)]
ALL_STRIPS = [(F, z) for F in STRIP_FACES for z in (False, True)]


# ---- the two paths -> dict(points, face, weights, cdf, areas) as numpy --------------------------------------------------------------
def _run_torch(case):
    v, f, u = case['v'], case['f'], case['u']
    areas = sampling._face_areas(v, f)
    assert areas.dtype == torch.float32
    points, face, weights = sampling._torch_sample(v, f, u)
    pub = sampling.sample_points(v, f, uniforms=u)
    assert torch.equal(pub[0], points) and torch.equal(pub[1], face)
    return dict(points=points.double().numpy(), face=face.numpy(), weights=weights.double().numpy(),
                cdf=areas.double().cumsum(1).numpy(), areas=areas.double().numpy())


def _hip_sample_cdf(v, f32, u):
    """icn_mesh_sample_fwd with a workspace of the caller's own -> (points, face int32, weights, cdf (B, F) float64): the CDF is what
    include/icn.h says the first 8 B F bytes of the workspace hold after the call."""
    L = _lib.lib()
    (nb, V, _), S, F = v.shape, u.shape[1], f32.shape[0]
    points = torch.empty(nb, S, 3, dtype=torch.float32, device=v.device)
    face = torch.empty(nb, S, dtype=torch.int32, device=v.device)
    weights = torch.empty(nb, S, 3, dtype=torch.float32, device=v.device)
    ws_bytes = L.icn_mesh_sample_workspace_bytes(nb, S, V, F)
    assert ws_bytes >= 8 * nb * F and ws_bytes % 16 == 0
    ws = torch.full((ws_bytes // 8,), float('nan'), dtype=torch.float64, device=v.device)
    with torch.cuda.device(v.device):
        rc = L.icn_mesh_sample_fwd(v.data_ptr(), f32.data_ptr(), u.data_ptr(), nb, S, V, F, points.data_ptr(), face.data_ptr(),
                                   weights.data_ptr(), ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream)
        _lib.check(rc, 'icn_mesh_sample_fwd')
        torch.cuda.synchronize()
    return points, face, weights, ws[:nb * F].reshape(nb, F).clone()


def _hip_areas(v, f):
    """The device's A_f (B, F) without its scan: every face as a mesh of its own (F = 1), whose CDF is the area."""
    tri = v[:, f.to(v.device)].reshape(-1, 3, 3).contiguous()
    one = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=v.device)
    cdf = _hip_sample_cdf(tri, one, torch.zeros(tri.shape[0], 1, 3, device=v.device))[3]
    return cdf.reshape(v.shape[0], f.shape[0])


def _run_hip(case):
    v, u, f32 = case['v'].cuda(), case['u'].cuda(), case['f'].cuda().int().contiguous()
    points, face, weights, cdf = _hip_sample_cdf(v, f32, u)
    assert all(torch.equal(a, b_) for a, b_ in zip(sampling._hip_sample(v, f32, u), (points, face, weights)))
    return dict(points=points.double().cpu().numpy(), face=face.long().cpu().numpy(), weights=weights.double().cpu().numpy(),
                cdf=cdf.cpu().numpy(), areas=_hip_areas(v, case['f']).cpu().numpy())


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def _check_areas(label, name, areas, a64, ae, zero):
    assert (areas[zero] == 0.0).all(), '%s %s: %d faces with coincident vertices have an area, largest %.3g' % (
        label, name, (areas[zero] != 0).sum(), areas[zero].max())
    rest = ~zero & (ae > 0)
    assert (rest == ~zero).all()
    ratio = np.abs(areas - a64)[rest] / (U24 * ae[rest])
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= AREA_BOUND, '%s %s: |A - A_64| = %.3f * 2^-24 |a||e|' % (label, name, worst)
    return worst


def _check(case, out, label):
    name, f, zero = case['name'], case['f'].numpy(), case['zero']
    v, u = case['v'].double().numpy(), case['u'].double().numpy().clip(0.0, 1.0)
    F, S = f.shape[0], u.shape[1]
    cdf, areas, face, points, w = out['cdf'], out['areas'], out['face'], out['points'], out['weights']
    a64, ae = _areas64(case['v'], case['f'])
    worst = _check_areas(label, name, areas, a64, ae, zero)
    d = np.diff(cdf, axis=1, prepend=0.0)
    exact_samples = 0
    for b in range(NB):
        T = cdf[b, -1]
        if not case['exact']:                                               # beyond 2^29 / F: range, finiteness and T only
            assert abs(T - math.fsum(areas[b])) <= F * np.spacing(T)
            assert (face[b] >= 0).all() and (face[b] < F).all()
            continue
        assert (d[b] >= 0).all() and (d[b].astype(np.float32).astype(np.float64) == d[b]).all()
        assert (d[b][zero[b]] == 0.0).all(), '%s %s: the CDF steps on %d faces with coincident vertices' % (label, name, (d[b][zero[b]] != 0).sum())
        assert np.array_equal(d[b], areas[b])                               # the steps of the CDF are the areas, scan or no scan
        assert np.array_equal(cdf[b], _prefix_fsum(areas[b]))
        if T > 0:
            want = np.searchsorted(cdf[b], u[b, :, 0] * T, side='right')
            want = np.where(want >= F, np.searchsorted(cdf[b], T, side='left'), want)
            assert (d[b][face[b]] > 0).all()                                # never a face without area
            share = STRATA * d[b] / T
            count = np.bincount(face[b, :STRATA], minlength=F)
            assert (np.abs(count - share) <= 1).all(), '%s %s: per-face counts off by %.3f' % (label, name, np.abs(count - share).max())
        else:
            want = np.zeros(S, dtype=np.int64)
        differ = face[b] != want
        assert not differ.any(), '%s %s mesh %d: %d of %d faces differ from the search in the path\'s own CDF, first at sample %d' % (
            label, name, b, differ.sum(), S, np.argmax(differ))
        exact_samples += S
    assert np.isfinite(points).all() and np.isfinite(w).all()
    # points and weights against float64 on the SAME face
    r = np.sqrt(u[..., 1])
    w64 = np.stack((1 - r, r * (1 - u[..., 2]), r * u[..., 2]), axis=-1)
    tri = np.stack([v[b][f[face[b]]] for b in range(NB)])                   # (NB, S, 3, 3)
    p64 = (w64[..., None] * tri).sum(2)
    M = np.abs(tri).max(axis=(2, 3))
    assert (np.abs(points - p64).max(-1) <= 16 * U24 * M).all()
    assert (w >= 0).all() and (np.abs(w.sum(-1) - 1) <= 4 * U24).all() and (np.abs(w - w64) <= 4 * U24).all()
    corners = 0
    for k, hit in enumerate(((u[..., 1] == 0), (u[..., 1] == 1) & (u[..., 2] == 0), (u[..., 1] == 1) & (u[..., 2] == 1))):
        unit = np.zeros(3)
        unit[k] = 1.0
        assert hit.sum() >= NB and (w[hit] == unit).all() and np.array_equal(points[hit], tri[hit][:, k])
        corners += int(hit.sum())
    print('RECORD %-6s %-32s worst |A - A_64| / (2^-24 |a||e|) %.3f   samples with the face checked exactly %d   corner samples %d' % (
        label, name, worst, exact_samples, corners))
    return worst


def _check_strip(case, out):
    """What the integers of the strip fix on their own: 8 c_f, and the face of every hand-placed sample."""
    assert np.array_equal(out['cdf'] * 8, np.cumsum(case['eighths'], axis=1).astype(np.float64))
    for b in range(NB):
        n = len(case['hand'][b])
        assert np.array_equal(out['face'][b, STRATA:STRATA + n], case['hand'][b])
        assert (case['eighths'][b][out['face'][b]] > 0).all()


def _check_degenerate(case, out, weights_of_a_good_mesh):
    assert (out['cdf'] == 0.0).all(), 'only degenerate: T = %s' % (out['cdf'][:, -1],)
    assert (out['face'] == 0).all() and np.isfinite(out['points']).all()
    assert np.array_equal(out['weights'], weights_of_a_good_mesh)


def _collapsed_grids(r=2):
    """-> {name: grid (2, 3, 5n, 2n)}, target: the whole output at one point, and every third row of pixels equal to the row before
    it (a face's v1 and v2 are neighbours across rows: many faces with v1 = v2, others with v1 = v0)."""
    x, t = data.synthetic_batch(NB, r, seed=5)
    x = 0.9 * x
    point = x[:, :, 2:3, 3:4].expand_as(x).contiguous()
    third = x.clone()
    third[:, :, 1::3] = x[:, :, 0::3][:, :, :third[:, :, 1::3].shape[2]]
    f = torch.from_numpy(geometry.get_ico_faces(r)).long()
    vt = losses.grid_to_vertices(third, r)
    tri = vt[:, f]
    assert int((tri[:, :, 1] == tri[:, :, 2]).all(-1).sum()) >= 20 and int(_coincident(vt, f).sum()) >= f.shape[0] // 4
    assert bool(_coincident(losses.grid_to_vertices(point, r), f).all())
    return dict(point=point, third=third), t


def _surface_loss(grid, t, device):
    crit = losses.Surface_Loss(2, samples=512).to(device)
    g = grid.to(device).clone().requires_grad_()
    loss = crit(g, t.to(device))
    loss.backward()
    assert math.isfinite(float(loss.detach())) and bool(torch.isfinite(g.grad).all())
    return float(loss.detach())


# ---- CPU: the torch formulation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale,shifted', ALL_SOUPS)
def test_torch_path_on_the_soup_of_kinds(scale, shifted):
    case = _soup(scale, shifted)
    _check(case, _run_torch(case), 'torch')


def test_torch_path_on_only_degenerate_faces():
    case, good = _degenerate(), _soup(1.0, False)
    _check(case, _run_torch(case), 'torch')
    _check_degenerate(case, _run_torch(case), sampling._torch_sample(good['v'], good['f'], case['u'])[2].double().numpy())


@pytest.mark.parametrize('faces,zero_runs', ALL_STRIPS)
def test_torch_path_on_the_unequal_strip(faces, zero_runs):
    case = _strip(faces, zero_runs)
    out = _run_torch(case)
    _check(case, out, 'torch')
    _check_strip(case, out)


@pytest.mark.parametrize('log2_ratio', (12, 40))
def test_torch_path_on_mixed_areas(log2_ratio):
    case = _mixed(log2_ratio)
    _check(case, _run_torch(case), 'torch')


def _p2m_shape_meshes():
    """Every family of tests/test_point_to_mesh_shapes.py as (n, 3, 3) fp32 single-face meshes."""
    return {name: torch.from_numpy(tri).float() for name, tri in _triangles().items()}


def test_torch_areas_on_the_point_to_mesh_shapes():
    one = torch.tensor([[0, 1, 2]])
    for name, v in _p2m_shape_meshes().items():
        a64, ae = _areas64(v, one)
        worst = _check_areas('torch', name, sampling._face_areas(v, one).double().numpy(), a64, ae, _coincident(v, one))
        print('RECORD torch  p2m shapes %-21s worst |A - A_64| / (2^-24 |a||e|) %.3f' % (name, worst))


def test_torch_surface_loss_on_collapsed_meshes():
    grids, t = _collapsed_grids()
    for name, grid in grids.items():
        print('Surface_Loss(2, samples=512), %s, torch formulation: %.8f' % (name, _surface_loss(grid, t, 'cpu')))


# ---- GPU: the HIP kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('scale,shifted', ALL_SOUPS)
def test_hip_path_on_the_soup_of_kinds(scale, shifted):
    case = _soup(scale, shifted)
    _check(case, _run_hip(case), 'hip')


@pytest.mark.gpu
def test_hip_path_on_only_degenerate_faces():
    case, good = _degenerate(), _soup(1.0, False)
    out = _run_hip(case)
    _check(case, out, 'hip')
    weights = sampling._hip_sample(good['v'].cuda(), good['f'].cuda().int().contiguous(), case['u'].cuda())[2]
    _check_degenerate(case, out, weights.double().cpu().numpy())
    # the three outputs against the torch formulation's: faces exactly, points to 16 * 2^-24 M, the weights to their own bound
    ref = _run_torch(case)
    assert np.array_equal(out['face'], ref['face'])
    M = np.abs(case['v'].double().numpy()[:, case['f'].numpy()[0]]).max(axis=(1, 2))
    assert (np.abs(out['points'] - ref['points']).max(-1) <= 16 * U24 * M[:, None]).all()
    assert (np.abs(out['weights'] - ref['weights']) <= 4 * U24).all()


@pytest.mark.gpu
@pytest.mark.parametrize('faces,zero_runs', ALL_STRIPS)
def test_hip_path_on_the_unequal_strip(faces, zero_runs):
    case = _strip(faces, zero_runs)
    out = _run_hip(case)
    _check(case, out, 'hip')
    _check_strip(case, out)


@pytest.mark.gpu
@pytest.mark.parametrize('log2_ratio', (12, 40))
def test_hip_path_on_mixed_areas(log2_ratio):
    case = _mixed(log2_ratio)
    _check(case, _run_hip(case), 'hip')


@pytest.mark.gpu
def test_hip_areas_on_the_point_to_mesh_shapes():
    one = torch.tensor([[0, 1, 2]])
    for name, v in _p2m_shape_meshes().items():
        a64, ae = _areas64(v, one)
        worst = _check_areas('hip', name, _hip_areas(v.cuda(), one).cpu().numpy(), a64, ae, _coincident(v, one))
        print('RECORD hip    p2m shapes %-21s worst |A - A_64| / (2^-24 |a||e|) %.3f' % (name, worst))


@pytest.mark.gpu
@pytest.mark.parametrize('which', ('soup', 'strip'))
def test_hip_backward_on_degenerate_faces(which):
    """icn_mesh_sample_bwd with the kernel's own faces and weights against a float64 index_add, bound (count + 2) * 2^-24 * sum |w g|
    per vertex; exact zeros at every vertex that belongs only to faces without area."""
    case = _soup(1.0, True) if which == 'soup' else _strip(1025, True)
    v, u, f32 = case['v'].cuda(), case['u'].cuda(), case['f'].cuda().int().contiguous()
    V, S = v.shape[1], u.shape[1]
    _, face, weights = sampling._hip_sample(v, f32, u)
    dp = torch.randn((NB, S, 3), generator=torch.Generator().manual_seed(2)).cuda()
    got = sampling._hip_sample_bwd(f32, face, weights, dp, V)
    want, mag = torch.zeros(NB, V, 3, dtype=torch.float64), torch.zeros(NB, V, 3, dtype=torch.float64)
    count = torch.zeros(NB, V, dtype=torch.float64)
    ids = case['f'][face.long().cpu()]
    wd = weights.double().cpu()[..., None] * dp.double().cpu()[:, :, None, :]
    for b in range(NB):
        for k in range(3):
            want[b].index_add_(0, ids[b, :, k], wd[b, :, k])
            mag[b].index_add_(0, ids[b, :, k], wd[b, :, k].abs())
            count[b].index_add_(0, ids[b, :, k], torch.ones(S, dtype=torch.float64))
    err = (got.double().cpu() - want).abs()
    bound = (count[..., None] + 2) * U24 * mag
    print('%s: worst error / bound = %.3f' % (case['name'], float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    a64 = _areas64(case['v'], case['f'])[0]
    flat = torch.zeros(NB, V, dtype=torch.bool)                              # private vertices: those of the faces without area
    for b in range(NB):
        flat[b, case['f'][torch.from_numpy(a64[b] == 0)].reshape(-1)] = True
    assert int(flat.sum()) >= 3 * 8 * NB and bool((got.cpu()[flat] == 0).all()) and bool((count[flat] == 0).all())
    assert bool((got.cpu()[~flat] != 0).any())
    vg = v.clone().requires_grad_()
    points, _ = sampling.sample_points(vg, case['f'].cuda(), uniforms=u)
    assert torch.equal(torch.autograd.grad(points, vg, dp)[0], got)


@pytest.mark.gpu
def test_hip_surface_loss_on_collapsed_meshes(monkeypatch):
    grids, t = _collapsed_grids()
    hip = {name: _surface_loss(grid, t, 'cuda') for name, grid in grids.items()}
    monkeypatch.setattr(losses, '_NO_HIP_LOSS', True)                       # what ICN_NO_HIP_LOSS=1 sets at import
    for name, grid in grids.items():
        fallback = _surface_loss(grid, t, 'cuda')
        print('Surface_Loss(2, samples=512), %s: hip %.8f, torch formulation on the device %.8f' % (name, hip[name], fallback))
        assert abs(fallback - hip[name]) <= 1e-5 * abs(fallback)
