"""Test-time metric of the reference: point-to-mesh distance (ico_utils.py:26-44 computeDistance, mode 'point2mesh'), which
upstream takes from kaolin's CUDA extension (`kaolin.metrics.trianglemesh.point_to_mesh_distance`, kaolin 0.9.1; absent here).

    dist2, face, kind = point_to_mesh_distance(points (B, P, 3), vertices (B, V, 3), faces (F, 3))
    dist2 (B, P)  squared Euclidean distance of every point to the closest point of the triangle mesh
    face  (B, P)  index of a closest triangle (the lowest index among equally close ones)
    kind  (B, P)  where on that triangle the closest point lies: 0 interior, 1 / 2 / 3 at vertex 0 / 1 / 2,
                  4 / 5 / 6 on edge (0,1) / (1,2) / (2,0)
On every triangle, coincident and collinear vertices included, sqrt(dist2) is within 14 u scale + min(u scale kappa, h_min) of
float64 (u = 2^-24, scale the largest |coordinate| involved, kappa = l_max / h_min the triangle's aspect ratio); a triangle without
area never reports kind 0 (tests/test_point_to_mesh_shapes.py).
The reference consumes `torch.mean(dist2)` (ico_utils.py:41).  ROCm fp32 tensors run on a HIP kernel (icn_point_to_mesh in
include/icn.h: one thread per point, triangles staged through LDS); anything else on the chunked torch formulation below,
which is also the kernel's second check in the tests (the first is the numpy oracle, oracle/metrics_ref.py).

search='grid' (default 'brute'; ROCm fp32 tensors only, anything else behaves as before) runs the forward through a spatial index
instead (icn_point_to_mesh_grid): per mesh the triangles are binned once by centroid into a uniform grid of G^3 cells, G =
round(sqrt(F / 16)) <= 64, and each point visits shells of cells around its own until a conservative bound excludes every triangle
not yet seen.  The result is the brute-force result BIT FOR BIT (same point-triangle routine, same lowest-face tie rule, for NaN /
infinite inputs too), so the backward is the same.  When to prefer which (MI355X, I5 / batch 36, profiles/point_to_mesh_grid.txt):
  * points near the surface -- a loss near convergence, a reconstruction against its target: 'grid'.  Build 0.14 ms + query
    0.33 ms against 14.6 ms at rms distance 0.01 (31 x), 2.3 ms against 15.4 ms at rms distance 0.06 of a unit-sized mesh (6.7 x).
  * most points farther from the surface than about a quarter of the mesh's extent (a Gaussian cloud, sigma 0.8, around a unit
    mesh), or many non-finite points: 'brute'.  Such a point gives up its walk after max(2, G / 4) shells and scans all F
    triangles: 28.2 ms against 15.5 ms, 1.8 x slower.  Likewise a mesh with non-finite vertices, of extent below 1e-3 of its
    distance from the origin, or made mostly of triangles longer than two cells: exact, but a linear scan.

Like kaolin's function, dist2 is differentiable in the points and in the mesh vertices on either path: the torch formulation
through autograd, the HIP path through icn_point_to_mesh_bwd (_PointToMeshFn below) whenever one of the two requires a gradient;
face and kind never carry one.  Where two different closest points are equally near the gradient is discontinuous (either side
is a valid subgradient).

face_normal_agreement (below) compares the normals of two such surfaces sample by sample: the face a surface sample lies on against
the closest face of the other mesh, `face` of sampling.sample_points and of point_to_mesh_distance.

mesh_area_volume (below) gives the surface area and the enclosed volume of every mesh of a batch, differentiable in the vertices
(icn_mesh_measure_fwd / _bwd, include/icn_measure.h; the backward gathers over vertex_face_table, the vertex -> corner incidence
table of the face list); volume_error is the relative volume error of one mesh pair, to stand beside compute_distance.

cotangent_laplacian and willmore_energy (below) give the integrated cotangent Laplace-Beltrami operator with the barycentric vertex
areas, and the Willmore bending energy (the integral of H^2) of every mesh of a batch, differentiable in the vertices
(icn_mesh_cotlap_* / icn_mesh_willmore_*, include/icn_curvature.h; every kernel gathers over vertex_face_table): the smoothness
measure that is geometric and scale invariant, where the uniform umbrella of losses.Mesh_Regularizer shrinks the mesh.

angle_defect, gaussian_curvature and total_curvature (below) give the discrete Gaussian curvature of every mesh of a batch: the
angle defect 2 pi - sum theta per vertex, that defect over the barycentric vertex area, and its sum per mesh (2 pi chi by
Gauss-Bonnet: 4 pi for a sphere), differentiable in the vertices (icn_mesh_angle_defect_fwd / _bwd, include/icn_gauss.h; the same
gather over vertex_face_table, in double from the fp32 vertices, because the defect of a fine mesh is lost in fp32).  With
cotangent_laplacian this completes the pair (H, K); curvature_error is the relative defect error of one mesh pair, to stand beside
volume_error and compute_distance.

self_intersections (below) counts, for every face of every mesh of a batch, the other faces of the same mesh it passes through, and
the intersecting pairs per mesh (icn_mesh_self_intersect, include/icn_isect.h: all pairs of faces, fp32 boxes first, the exact
tests in double): the one figure here that is NOT unremarkable on a mesh that folds through itself -- distance, normals, area,
volume and curvature all stay finite there.  Integers, no gradient; the HIP path reproduces the float64 formulation exactly.
self_intersection_ratio is the share of self-intersecting faces of one mesh, the figure the mesh-generation literature reports, to
stand beside curvature_error, volume_error and compute_distance.

signed_point_to_mesh_distance, contains and volumetric_iou (below) add the side to the distance: phi = sign sqrt(dist2), negative
inside a closed mesh, the sign that of (p - q) . N with q the closest point the search found and N the angle-weighted pseudonormal
of the feature q lies on -- the face normal, the sum of the two unit normals at an edge, the angle-weighted sum around a vertex
(icn_point_to_mesh_sign, include/icn_sdf.h: one gather per point over signed_distance_tables, the face adjacency and
vertex_face_table, in double; no second search, and the gradient is that of dist2 under a rescaled upstream).  contains is kaolin's
check_sign; volumetric_iou is the intersection over union of the solids of one mesh pair on a lattice, to stand beside volume_error
and compute_distance.  Its lattice points lie mostly far from the surface, where 'grid' falls back to the linear scan (above).

voxel_lattice, voxelize and volumetric_iou(method='voxel') (below) fill a lattice without any search: rays along axis 0, one per
lattice column, and a cell is inside iff an odd number of faces cross its column at or before it (icn_mesh_voxelize, include/
icn_voxel.h: one thread per column against the faces of its mesh, which pass through LDS tiles culled against the workgroup's tile of
columns; double arithmetic with a symbolic perturbation, so every column crosses a closed mesh an even number of times whatever lies
on an edge or a vertex; n0 parity bits per column and one prefix XOR, no atomics).  It visits each (column, face) pair once where
contains visits each (cell, face) pair, it needs no adjacency table, and it is right for any closed mesh whatever its winding: the
occupancy grid that the reference's users otherwise take from kaolin.  Bools, no gradient; the HIP path reproduces the float64
formulation byte for byte.

ray_cast, contains_by_parity, depth_map and silhouette_iou (below) answer the general query: where a given ray first meets a mesh,
on which face, and how many faces it crosses (icn_mesh_raycast, include/icn_raycast.h: one thread per ray against the faces of its
mesh through LDS tiles, the same symbolic perturbation in double, so that exactly one of the two faces of an edge claims a ray
through it; an fp32 filter proved to change nothing in front).  The parity of the count is an inside test from any direction that
needs no consistent winding; the depth is differentiable in vertices, origins and directions (icn_mesh_raycast_bwd: one record per
ray, then the vertex scatter); depth_map renders orthographic depth images and silhouettes, and silhouette_iou is the 2-D mask IoU
of one mesh pair over seven views, to stand beside volumetric_iou.  The HIP path reproduces the float64 formulation bit for bit.

sided_distance, chamfer_distance, f_score and hausdorff_distance (below) measure two POINT SETS against each other, the figures every
mesh-reconstruction paper reports and the reference's test modes `chamfer` and `f_<radius>` (run.py:630; kaolin.metrics.pointcloud
upstream): for every point of one set the squared distance to its nearest point in the other set and which point that is
(icn_nearest_points, include/icn_nn.h: the targets through LDS tiles in ascending order, two queries per thread in registers, fp32
without contraction, the lowest index among equal distances, no atomics; the distance is differentiable in both sets through
icn_nearest_points_bwd, one record per point, then the vertex scatter).  The HIP path reproduces the fp32 formulation bit for bit.
evaluate_distance gives every test mode of the reference for one mesh pair -- point2point, point2mesh, chamfer, f_<radius> -- and
hausdorff, on the vertices or on surface samples, where compute_distance keeps the reference's answer (None but for point2mesh).

pairwise_sided_sums, pairwise_chamfer, minimum_matching_distance, coverage, one_nn_accuracy and generation_metrics (below) score a
GENERATED set of shapes, which has no targets to be paired with: the G x R matrix of chamfer distances between every generated and
every reference cloud, and the three figures the shape-generation literature reads off it (Achlioptas et al. 2018; Yang et al. 2019):
MMD-CD, COV-CD and 1-NNA-CD.  The matrix comes from icn_sided_sums (include/icn_pairs.h): a kernel that indexes the pair of clouds
itself, keeps no index, sums the distances of a pair in double inside the launch and writes one double a pair; its distances are
those of icn_nearest_points bit for bit.  No gradient.  geniconet_amd/generation.py draws the shapes of ico2ico_vae to score.

optimal_matching, pairwise_emd and earth_movers_distance (below) give the same tables their second half, the EARTH MOVER'S DISTANCE
those papers report beside chamfer because chamfer does not see uneven point density: the assignment of the points of one cloud to
the points of another that minimises the summed Euclidean distance, and its mean.  Every cloud here is the vertex set of an
icosahedral grid or S surface samples, so the two clouds of a pair have one size and EMD is a plain assignment problem, solved by a
synchronous epsilon-scaling auction (icn_match_clouds, include/icn_match.h: one workgroup owns a pair from start to finish, prices and
owners in LDS, every wave scanning the objects for one bidder at a time, bids resolved by integer LDS atomics; the mean cost is within
D 4^-phases of the optimum, D the diagonal of the joint bounding box, and the outputs prove it by epsilon-complementary slackness).
The HIP path reproduces the torch restatement on CPU tensors bit for bit in the matching, the round count and the prices.
generation_metrics(distance='emd') reads MMD-EMD, COV-EMD and 1-NNA-EMD off pairwise_emd, evaluate_distance(mode='emd') gives one mesh
pair's, and earth_movers_distance is differentiable in both sets at the matching found.

generation_metrics, evaluate_distance and generation.evaluate_generation take points = P to run on P well-spread points of every cloud
instead of the whole cloud: sampling.farthest_points (icn_farthest_points, include/icn_fps.h), the protocol those tables come from.

occupancy_counts, occupancy_jsd and jensen_shannon_divergence (below) give those tables their first column, the JENSEN-SHANNON
DIVERGENCE of the occupancy distributions of two sets: every point of every cloud of a set dropped into a lattice (28^3 in the papers),
the two normalised histograms compared -- the one figure of the four that is a property of the whole set, and the one that sees a
generator put mass where the data has none (icn_point_occupancy and icn_occupancy_jsd, include/icn_occupancy.h: every workgroup a
private histogram in LDS filled by integer LDS atomics, no global atomics; the divergence in double in a fixed order).  Integer counts
are order-free, so the HIP path reproduces the torch restatement on CPU tensors bit for bit in the counts.  generation_metrics and
generation.evaluate_generation take jsd = R to add it.
"""
import torch

from . import _lib


def _on_hip_path(vertices):
    """Whether the mesh operators on `vertices` run on the HIP kernels: ROCm fp32 tensors, unless ICN_NO_HIP_LOSS=1."""
    from . import losses
    return not losses._NO_HIP_LOSS and vertices.is_cuda and vertices.dtype == torch.float32


def _closest_on_triangles(p, a, b, c):
    """Squared distance + region of the closest point on triangles (a, b, c) for points p; all (..., 3), broadcastable.
    Region tests of Ericson, Real-Time Collision Detection 5.1.5 (Voronoi regions of the triangle's features), with the three
    edge functions taken from the normal n = ab x ac (vc = ab . (ap x n), vb = -ac . (ap x n), va = |n|^2 - vb - vc) instead of
    differences of products of dot products, and the interior distance from the plane, (ap . n)^2 / |n|^2: the error grows with
    the first power of the triangle's aspect ratio, not the second.  A triangle whose normal cannot be resolved,
    |n|^2 <= 2 eps |ab|^2 |ac|^2 (the sine of the angle at vertex 0 below about 1 / 2048 in fp32; every coincident or collinear
    triangle), is the union of its three edge segments: the nearest of three clamped projections, never kind 0.
    The same method and region tests as tri_dist2 in csrc/icn_loss.hip, not the same arithmetic: the interior distance is
    taken along n / |n| here and as n (ap . n / |n|^2) there, edge (1, 2) is the clamped projection while edges (0, 1) and
    (2, 0) divide unclamped, and the device contracts to FMAs.  The two agree to rounding, never bit for bit."""
    ab, ac, ap = b - a, c - a, p - a
    lab, lac, g = (ab * ab).sum(-1), (ac * ac).sum(-1), (ab * ac).sum(-1)
    d1, d2 = (ab * ap).sum(-1), (ac * ap).sum(-1)
    d3, d4, d5, d6 = d1 - lab, d2 - g, d1 - g, d2 - lac
    n = torch.linalg.cross(ab, ac)
    nn = (n * n).sum(-1)
    r = torch.linalg.cross(ap, n)
    vc, vb = (ab * r).sum(-1), -(ac * r).sum(-1)
    va = nn - vb - vc
    one = torch.ones_like(d1)
    tiny = torch.finfo(p.dtype).tiny

    def safe(num, den):
        return num / torch.where(den.abs() > tiny, den, one)

    def segment(u, uw, den, k_u, k_w, k_edge):
        """Clamped projection of p on the segment u + t uw -> (p - q, kind)."""
        up = p - u
        t = safe((uw * up).sum(-1), den).clamp(0, 1)
        k = torch.where(t <= 0, torch.full_like(t, k_u), torch.where(t >= 1, torch.full_like(t, k_w), torch.full_like(t, k_edge)))
        return up - uw * t[..., None], k.to(torch.int32)
    bc = c - b
    lbc = (bc * bc).sum(-1)
    seg_ab, seg_bc, seg_ac = segment(a, ab, lab, 1, 2, 4), segment(b, bc, lbc, 2, 3, 5), segment(a, ac, lac, 1, 3, 6)
    # interior (default), then the edge and vertex regions in increasing priority
    flat = ~(nn * (0.5 / torch.finfo(p.dtype).eps) > lab * lac)
    unit = n / torch.where(flat, one, nn).sqrt()[..., None]                  # |n|, not |n|^2: its square must not underflow
    d = unit * (ap * unit).sum(-1, keepdim=True)
    kind = torch.zeros_like(d1, dtype=torch.int32)

    def put(mask, vec, k):
        nonlocal d, kind
        d = torch.where(mask[..., None], vec, d)
        kind = torch.where(mask, k if torch.is_tensor(k) else torch.full_like(kind, k), kind)
    put((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), *seg_bc)                                  # edge (1, 2)
    put((vb <= 0) & (d2 >= 0) & (d6 <= 0), ap - ac * safe(d2, lac)[..., None], 6)                  # edge (2, 0)
    put((vc <= 0) & (d1 >= 0) & (d3 <= 0), ap - ab * safe(d1, lab)[..., None], 4)                  # edge (0, 1)
    put((d6 >= 0) & (d5 <= d6), (p - c).expand_as(d), 3)
    put((d3 >= 0) & (d4 <= d3), (p - b).expand_as(d), 2)
    put((d1 <= 0) & (d2 <= 0), ap.expand_as(d), 1)
    # unresolved normal: the nearest of the three segments, the first among equals in the order (0,1), (1,2), (2,0)
    # (a projection clamped to a vertex is dropped where the other segment through that vertex projects inside itself: that one
    # is nearer, by an amount that the squared distance may be too coarse to show)
    inside = [(k >= 4) for _, k in (seg_ab, seg_bc, seg_ac)]
    ends = ((1, 2, 2, 1), (2, 0, 3, 2), (1, 0, 3, 1))          # per segment: kind at t = 0, the other segment there, at t = 1, there
    fd = fk = fd2 = None
    for (vec, k), (k0, o0, k1, o1) in zip((seg_ab, seg_bc, seg_ac), ends):
        v2 = (vec * vec).sum(-1)
        v2 = torch.where(((k == k0) & inside[o0]) | ((k == k1) & inside[o1]), torch.full_like(v2, float('inf')), v2)
        if fd is None:
            fd, fk, fd2 = vec, k, v2
            continue
        take = v2 < fd2
        fd, fk, fd2 = torch.where(take[..., None], vec, fd), torch.where(take, k, fk), torch.where(take, v2, fd2)
    put(flat.expand_as(kind), fd, fk)
    return (d * d).sum(-1), kind


def _torch_point_to_mesh(points, vertices, faces, chunk=256):
    B, P, _ = points.shape
    f = faces.long()
    tri = vertices[:, f]                                           # (B, F, 3, 3)
    a, b, c = tri[:, None, :, 0], tri[:, None, :, 1], tri[:, None, :, 2]
    best = points.new_full((B, P), float('inf'))
    face = torch.zeros(B, P, dtype=torch.int64, device=points.device)
    kind = torch.zeros(B, P, dtype=torch.int32, device=points.device)
    for lo in range(0, P, chunk):
        d2, k = _closest_on_triangles(points[:, lo:lo + chunk, None, :], a, b, c)      # (B, chunk, F)
        m, j = d2.min(dim=2)
        best[:, lo:lo + chunk], face[:, lo:lo + chunk] = m, j
        kind[:, lo:lo + chunk] = torch.gather(k, 2, j[..., None])[..., 0]
    return best, face, kind


_MAX_GRID_Y = 65535


def _batch_slices(B):
    """(b0, nb) slices of a batch of B meshes: the batch index of the mesh kernels is gridDim.y, at most _MAX_GRID_Y per launch."""
    for b0 in range(0, B, _MAX_GRID_Y):
        yield b0, min(_MAX_GRID_Y, B - b0)


_NB = object()                     # in the arguments of _launch: the mesh count of the slice, where the entry takes B


class _per_mesh:
    """Marks an argument of _launch as a contiguous (B, ...) tensor with one row per mesh, or None: a slice passes the address of
    its first mesh, None stays null."""
    __slots__ = ('tensor',)

    def __init__(self, tensor):
        self.tensor = tensor


def _batch_of(args):
    """The first per-mesh tensor among the arguments of _launch: its shape[0] is the batch, its device the call's."""
    return next(a.tensor for a in args if isinstance(a, _per_mesh) and a.tensor is not None)


def _slice_arguments(L, args, workspace=None):
    """The marshalling of _launch, on tensors of any device -> (the C arguments of every slice of _batch_slices, ws_bytes).  Of args,
    a _per_mesh tensor becomes the address of the slice's first mesh, any other tensor its address (a table the batch shares), _NB
    the slice's mesh count; None is a null pointer and numbers pass as they are.  workspace = (query entry of L, its sizes after B)
    is asked once, for the largest slice, min(B, _MAX_GRID_Y); ws_bytes is None without one."""
    B = _batch_of(args).shape[0]
    ws_bytes = getattr(L, workspace[0])(min(B, _MAX_GRID_Y), *workspace[1:]) if workspace else None

    def argument(a, b0, nb):
        if isinstance(a, _per_mesh):
            t = a.tensor
            return None if t is None else (t[b0:] if b0 else t).data_ptr()
        return nb if a is _NB else a.data_ptr() if torch.is_tensor(a) else a
    return [tuple(argument(a, b0, nb) for a in args) for b0, nb in _batch_slices(B)], ws_bytes


def _launch(entry, *args, workspace=None):
    """One call into the library per slice of the batch, on the device and the current stream of the per-mesh tensors: `entry` with
    args in ABI order (see _slice_arguments), then, with workspace = (query entry, its sizes after B), a scratch buffer of that
    size and its size -- one buffer, reused by the slices in stream order -- then the stream."""
    L = _lib.api()
    device = _batch_of(args).device
    calls, ws_bytes = _slice_arguments(L, args, workspace)
    tail = ()
    if workspace:
        ws = _lib.workspace(ws_bytes, device)
        tail = (ws.data_ptr(), ws_bytes)
    fn = getattr(L, entry)
    with torch.cuda.device(device):
        for call in calls:
            fn(*call, *tail, _lib.stream())


def _upstream(grad):
    """An upstream gradient as the kernels read it (contiguous fp32); None, an output nobody differentiated, stays None."""
    return None if grad is None else grad.contiguous().to(torch.float32)


_SEARCHES = ('brute', 'grid')


def _check_search(search):
    if search not in _SEARCHES:
        raise ValueError('point_to_mesh_distance: search must be one of %s, got %r' % (_SEARCHES, search))


def _hip_point_to_mesh(pts, vts, f32, search='brute'):
    """icn_point_to_mesh (search 'brute') or icn_point_to_mesh_grid ('grid') on contiguous fp32 ROCm tensors and int32 faces
    -> (dist, face int32, kind)."""
    B, P, _ = pts.shape
    V, F = vts.shape[1], f32.shape[0]
    dist = torch.empty(B, P, dtype=torch.float32, device=pts.device)
    face = torch.empty(B, P, dtype=torch.int32, device=pts.device)
    kind = torch.empty(B, P, dtype=torch.int32, device=pts.device)
    args = (_per_mesh(pts), _per_mesh(vts), f32, _NB, P, V, F, _per_mesh(dist), _per_mesh(face), _per_mesh(kind))
    if search == 'grid':
        _launch('icn_point_to_mesh_grid', *args, workspace=('icn_point_to_mesh_grid_workspace_bytes', P, V, F))
    else:
        _launch('icn_point_to_mesh', *args)
    return dist, face, kind


class _PointToMeshFn(torch.autograd.Function):
    """point_to_mesh_distance on the HIP path with a gradient (icn_point_to_mesh / icn_point_to_mesh_bwd in include/icn.h).
    The closest point q of p minimises over the feature it lies on, so d dist / d p = 2 (p - q) and the triangle's vertices
    receive -2 w (p - q) with q's weights w; the backward recomputes q from the saved (face, kind), O(1) per point, and sums
    the vertex gradient in a fixed order (bit-identical run to run).  Only the gradients autograd asks for are computed."""

    @staticmethod
    def forward(ctx, pointclouds, vertices, f32, search='brute'):
        pts, vts = pointclouds.contiguous(), vertices.contiguous()
        dist, face, kind = _hip_point_to_mesh(pts, vts, f32, search)
        ctx.save_for_backward(pts, vts, f32, face, kind)
        face64 = face.long()
        ctx.mark_non_differentiable(face64, kind)
        return dist, face64, kind

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ddist, _gface, _gkind):
        pts, vts, f32, face, kind = ctx.saved_tensors
        P, V, F = pts.shape[1], vts.shape[1], f32.shape[0]
        dpts = torch.empty_like(pts) if ctx.needs_input_grad[0] else None
        dvts = torch.empty_like(vts) if ctx.needs_input_grad[1] else None
        args = (_per_mesh(pts), _per_mesh(vts), f32, _per_mesh(face), _per_mesh(kind), _per_mesh(_upstream(ddist)), _NB, P, V, F,
                _per_mesh(dpts), _per_mesh(dvts))
        if dvts is not None:                                                              # only the vertex gradient needs scratch
            _launch('icn_point_to_mesh_bwd', *args, workspace=('icn_point_to_mesh_bwd_workspace_bytes', P, V, F))
        else:
            _launch('icn_point_to_mesh_bwd', *args, None, 0)
        return dpts, dvts, None, None


def _point_to_mesh_unchecked(pointclouds, vertices, f32, search='brute'):
    """point_to_mesh_distance without its argument checks, for callers that validated once (losses.Surface_Loss: the face list is
    a buffer checked at construction): f32 is an int32 (F, 3) tensor on the points' device with indices in [0, V).  No host
    synchronisation -- the public function's index check reads faces.min() / max() back on every call."""
    if pointclouds.is_cuda and pointclouds.dtype == torch.float32 and vertices.dtype == torch.float32 and f32.shape[0] > 0:
        if torch.is_grad_enabled() and (pointclouds.requires_grad or vertices.requires_grad):
            return _PointToMeshFn.apply(pointclouds, vertices, f32, search)
        dist, face, kind = _hip_point_to_mesh(pointclouds.contiguous(), vertices.contiguous(), f32, search)
        return dist, face.long(), kind
    return _torch_point_to_mesh(pointclouds, vertices, f32)


def point_to_mesh_distance(pointclouds, vertices, faces, search='brute'):
    """See the module docstring.  `faces` may be int32 / int64, (F, 3), shared by the batch (as in kaolin 0.9.1).
    search: 'brute' (default) or 'grid', the forward's closest-triangle search on the HIP path; the outputs are identical."""
    _check_search(search)
    if pointclouds.dim() != 3 or vertices.dim() != 3 or pointclouds.shape[-1] != 3 or vertices.shape[-1] != 3:
        raise ValueError('point_to_mesh_distance: expected (B, P, 3) points and (B, V, 3) vertices')
    if pointclouds.shape[0] != vertices.shape[0] or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('point_to_mesh_distance: batch sizes differ or faces is not (F, 3)')
    if faces.shape[0] > 0:
        # the kernel indexes vertices[b, faces[f]] unchecked: a 1-based or mismatched face list (an OFF file read with the
        # wrong vertex set) must fail here like kaolin's / torch's IndexError, not as a device memory fault.  One host sync;
        # this is a test-time metric (ico_utils.py:26-44).
        lo, hi = int(faces.min()), int(faces.max())
        if lo < 0 or hi >= vertices.shape[1]:
            raise IndexError('point_to_mesh_distance: face indices span [%d, %d] but there are %d vertices'
                             % (lo, hi, vertices.shape[1]))
    if pointclouds.is_cuda and pointclouds.dtype == torch.float32 and vertices.dtype == torch.float32 and faces.shape[0] > 0:
        return _point_to_mesh_unchecked(pointclouds, vertices, faces.to(device=pointclouds.device, dtype=torch.int32).contiguous(),
                                        search)
    return _torch_point_to_mesh(pointclouds, vertices, faces.to(pointclouds.device))


# ---- normal agreement of two sampled surfaces ---------------------------------------------------------------------------------------
_NORMAL_FLAT = 4194304.0           # 2^22: TRI_FLAT of tri_dist2 (csrc/icn_loss.hip); a constant of the definition, in every dtype


def _resolved_unit_normals(vertices, faces, face):
    """(n^ (B, S, 3), |n| (B, S), resolved (B, S)) of faces[face] of every mesh, as face_normal_agreement defines them: n^ is 0 and
    carries no gradient where the normal is unresolved (a face id outside [0, F) and a vertex id outside [0, V) included; ids are
    clamped before they index anything)."""
    from .losses import Mesh_Regularizer
    V, F = vertices.shape[1], faces.shape[0]
    face = face.long()
    ids = faces.long()[face.clamp(0, F - 1)]                                             # (B, S, 3)
    ok = (face >= 0) & (face < F) & ((ids >= 0) & (ids < V)).all(-1)
    corners = torch.gather(vertices, 1, ids.clamp(0, V - 1).reshape(ids.shape[0], -1, 1).expand(-1, -1, 3)).view(*ids.shape, 3)
    e1, e2 = corners[:, :, 1] - corners[:, :, 0], corners[:, :, 2] - corners[:, :, 0]
    with torch.no_grad():
        n = Mesh_Regularizer._face_normal(e1, e2)
        q = (n * n).sum(-1) * _NORMAL_FLAT
        ok = ok & (q > (e1 * e1).sum(-1) * (e2 * e2).sum(-1)) & torch.isfinite(q)
    # an unresolved face enters as a zero triangle: its (possibly non-finite) vertices meet no arithmetic that autograd records
    zero = torch.zeros_like(e1)
    e1, e2 = torch.where(ok[..., None], e1, zero), torch.where(ok[..., None], e2, zero)
    n = Mesh_Regularizer._face_normal(e1, e2)
    nn = (n * n).sum(-1)
    length = torch.where(ok, nn, torch.ones_like(nn)).sqrt()
    return n / length[..., None], length, ok


def _torch_face_normal_agreement(vertices_a, faces_a, face_a, vertices_b, faces_b, face_b, oriented=True):
    """The definition of face_normal_agreement in torch, differentiable in both vertex tensors through autograd."""
    ua, _, _ = _resolved_unit_normals(vertices_a, faces_a, face_a)
    ub, _, _ = _resolved_unit_normals(vertices_b, faces_b, face_b)
    c = (ua * ub).sum(-1)                                                                # 0 where either side is unresolved
    return 1 - (c if oriented else c.abs())                                              # (abs: derivative 0 at c = 0)


def _hip_face_normal_agreement(va, fa32, face_a, vb, fb32, face_b, oriented):
    """icn_face_normal_agree_fwd on contiguous fp32 ROCm vertices, int32 face tables and int32 (B, S) face ids -> t (B, S)."""
    B, S = face_a.shape
    t = torch.empty(B, S, dtype=torch.float32, device=va.device)
    _launch('icn_face_normal_agree_fwd', _per_mesh(va), fa32, _per_mesh(face_a), va.shape[1], fa32.shape[0],
            _per_mesh(vb), fb32, _per_mesh(face_b), vb.shape[1], fb32.shape[0], _NB, S, int(oriented), _per_mesh(t))
    return t


class _FaceNormalAgreementFn(torch.autograd.Function):
    """face_normal_agreement on the HIP path (icn_face_normal_agree_fwd / _bwd in include/icn_ext.h); only the sides autograd asks
    for are computed, each summed in a fixed order (bit-identical run to run)."""

    @staticmethod
    def forward(ctx, vertices_a, fa32, face_a, vertices_b, fb32, face_b, oriented):
        va, vb = vertices_a.contiguous(), vertices_b.contiguous()
        ia, ib = face_a.to(torch.int32).contiguous(), face_b.to(torch.int32).contiguous()
        ctx.save_for_backward(va, fa32, ia, vb, fb32, ib)
        ctx.oriented = int(oriented)
        return _hip_face_normal_agreement(va, fa32, ia, vb, fb32, ib, oriented)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dt):
        va, fa32, ia, vb, fb32, ib = ctx.saved_tensors
        S, Va, Vb = ia.shape[1], va.shape[1], vb.shape[1]
        dva = torch.empty_like(va) if ctx.needs_input_grad[0] else None
        dvb = torch.empty_like(vb) if ctx.needs_input_grad[3] else None
        if dva is None and dvb is None:
            return (None,) * 7
        _launch('icn_face_normal_agree_bwd', _per_mesh(va), fa32, _per_mesh(ia), Va, fa32.shape[0], _per_mesh(vb), fb32, _per_mesh(ib),
                Vb, fb32.shape[0], _NB, S, ctx.oriented, _per_mesh(_upstream(dt)), _per_mesh(dva), _per_mesh(dvb),
                workspace=('icn_face_normal_agree_bwd_workspace_bytes', S, Va, Vb))
        return dva, None, None, dvb, None, None, None


def _face_normal_agreement_unchecked(vertices_a, fa32, face_a, vertices_b, fb32, face_b, oriented=True):
    """face_normal_agreement without its argument checks and without a host synchronisation, for callers that validated once
    (losses.Surface_Loss): fa32 / fb32 are int32 (F, 3) tensors on the vertices' device, F >= 1; face_a / face_b (B, S) integer
    tensors there.  Ids out of range are safe on either path: such a sample is unresolved (t = 1, no gradient)."""
    if _on_hip_path(vertices_a) and vertices_b.dtype == torch.float32:
        if torch.is_grad_enabled() and (vertices_a.requires_grad or vertices_b.requires_grad):
            return _FaceNormalAgreementFn.apply(vertices_a, fa32, face_a, vertices_b, fb32, face_b, bool(oriented))
        return _hip_face_normal_agreement(vertices_a.detach().contiguous(), fa32, face_a.to(torch.int32).contiguous(),
                                          vertices_b.detach().contiguous(), fb32, face_b.to(torch.int32).contiguous(), bool(oriented))
    return _torch_face_normal_agreement(vertices_a, fa32, face_a, vertices_b, fb32, face_b, oriented)


def face_normal_agreement(vertices_a, faces_a, face_a, vertices_b, faces_b, face_b, oriented=True):
    """Normal agreement of two sampled surfaces, t (B, S): for sample s of mesh pair b, face face_a[b, s] of mesh a (vertices_a
    (B, Va, 3), faces_a (Fa, 3) shared by the batch) against face face_b[b, s] of mesh b -- typically the face a surface sample lies
    on (sampling.sample_points) and the closest face of the other mesh (point_to_mesh_distance).  What pytorch3d's
    chamfer_distance(x_normals=...) adds to the distance, from face normals.

    One definition for the HIP kernels (include/icn_ext.h), the torch formulation and the tests.  For a face (i0, i1, i2):
        e1 = v1 - v0, e2 = v2 - v0, n = e1 x e2 with every product of the cross product rounded on its own
        (Mesh_Regularizer._face_normal; face_normal on the device): a face with two coincident vertices has n exactly 0
        the normal is RESOLVED iff |n|^2 2^22 > |e1|^2 |e2|^2 and all of that is finite (the constant of tri_dist2, in every dtype)
        n^ = n / |n| where resolved, else 0, and no gradient passes through that face
        c = n^_a . n^_b;   t = 1 - c (oriented, the default)  or  1 - |c| (the derivative of |c| at c = 0 is taken as 0)
    An unresolved face on either side gives t = 1 and a zero gradient on both sides; non-finite vertices are unresolved, never NaN
    in the gradient.  Differentiable in both vertex tensors: ROCm fp32 tensors run on icn_face_normal_agree_fwd / _bwd (the
    gradient of each side that requires one, summed in a fixed order without atomics: bit-identical run to run, an exact zero at a
    vertex no sample touches); ICN_NO_HIP_LOSS=1, CPU tensors and other dtypes take the torch formulation through autograd.
    Shapes are checked (ValueError); face ids against F and face tables against V with one read-back (IndexError)."""
    who = 'face_normal_agreement'
    for v, name in ((vertices_a, 'vertices_a'), (vertices_b, 'vertices_b')):
        if v.dim() != 3 or v.shape[-1] != 3 or v.shape[0] < 1 or v.shape[1] < 1 or not v.is_floating_point():
            raise ValueError('%s: expected floating-point %s (B, V, 3), got %s' % (who, name, tuple(v.shape)))
    if vertices_a.shape[0] != vertices_b.shape[0] or vertices_a.dtype != vertices_b.dtype or vertices_a.device != vertices_b.device:
        raise ValueError('%s: the two vertex tensors differ in batch size, dtype or device' % who)
    for f, name in ((faces_a, 'faces_a'), (faces_b, 'faces_b')):
        if f.dim() != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.is_floating_point():
            raise ValueError('%s: expected integer %s (F, 3) with F >= 1, got %s' % (who, name, tuple(f.shape)))
    B = vertices_a.shape[0]
    for f, name in ((face_a, 'face_a'), (face_b, 'face_b')):
        if f.dim() != 2 or f.shape[0] != B or f.shape[1] < 1 or f.is_floating_point() or f.dtype == torch.bool:
            raise ValueError('%s: expected integer %s (%d, S) with S >= 1, got %s' % (who, name, B, tuple(f.shape)))
    if face_a.shape != face_b.shape:
        raise ValueError('%s: face_a %s and face_b %s differ in shape' % (who, tuple(face_a.shape), tuple(face_b.shape)))
    dev = vertices_a.device
    fa32, fb32 = (f.to(device=dev, dtype=torch.int32).contiguous() for f in (faces_a, faces_b))
    face_a, face_b = face_a.to(dev), face_b.to(dev)
    spans = torch.stack([torch.stack(x.aminmax()).long() for x in (fa32, fb32, face_a, face_b)]).tolist()      # one read-back
    for (lo, hi), limit, what, of in zip(spans, (vertices_a.shape[1], vertices_b.shape[1], fa32.shape[0], fb32.shape[0]),
                                         ('faces_a indexes', 'faces_b indexes', 'face_a indexes', 'face_b indexes'),
                                         ('vertices', 'vertices', 'faces', 'faces')):
        if lo < 0 or hi >= limit:
            raise IndexError('%s: %s [%d, %d] but there are %d %s' % (who, what, lo, hi, limit, of))
    return _face_normal_agreement_unchecked(vertices_a, fa32, face_a, vertices_b, fb32, face_b, oriented)


# ---- surface area and enclosed volume -----------------------------------------------------------------------------------------------
def vertex_face_table(faces, num_vertices):
    """The vertex -> corner incidence table of a face list, (offsets int32 (V + 1), corners int32 (3 F)) on the faces' device: corner
    c = 3 f + k is vertex k of face f, `corners` holds them grouped by the vertex faces[f, k] and ascending in c within a vertex, and
    the corners of vertex j are corners[offsets[j] : offsets[j + 1]].  Built once per face list (a stable sort and a search of the sorted ids, no
    host synchronisation); with it a vertex gradient is a fixed-order gather of O(F) per mesh (icn_mesh_measure_bwd, include/
    icn_measure.h).  Corners whose vertex id lies outside [0, V) are sorted behind offsets[V] and belong to no vertex."""
    V = int(num_vertices)
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError('vertex_face_table: expected integer faces (F, 3), got %s %s' % (faces.dtype, tuple(faces.shape)))
    if V < 1:
        raise ValueError('vertex_face_table: num_vertices must be positive, got %r' % (num_vertices,))
    flat = faces.reshape(-1).long()
    key = torch.where((flat >= 0) & (flat < V), flat, torch.full_like(flat, V))
    ordered, corners = torch.sort(key, stable=True)
    # offsets[j] = the number of corners of the vertices before j: the cumulated bincount, read off the sorted ids (torch.bincount
    # reads its output size back from the device)
    offsets = torch.searchsorted(ordered, torch.arange(V + 1, device=key.device))
    return offsets.to(torch.int32), corners.to(torch.int32)


def _torch_mesh_area_volume(vertices, faces):
    """The definition of mesh_area_volume in torch, differentiable in the vertices through autograd; sums in float64."""
    from .losses import Mesh_Regularizer
    V = vertices.shape[1]
    ids = faces.long()
    ok = ((ids >= 0) & (ids < V)).all(-1)                                                 # (F,): the others contribute 0
    tri = vertices[:, ids.clamp(0, V - 1)]                                                # (B, F, 3 corners, 3)
    p0, p1, p2 = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
    e1, e2 = p1 - p0, p2 - p0
    with torch.no_grad():
        nn = (Mesh_Regularizer._face_normal(e1, e2) ** 2).sum(-1)
        flat = ~((nn > 0) & torch.isfinite(nn))                                           # |n|^2 zero or not finite: the subgradient 0
        a_flat = 0.5 * nn.sqrt()                                                          # ... and the value all the same (NaN stays NaN)
    # a face without a gradient enters autograd as a zero triangle: its vertices meet no arithmetic that autograd records
    zero = torch.zeros_like(e1)
    n = Mesh_Regularizer._face_normal(torch.where(flat[..., None], zero, e1), torch.where(flat[..., None], zero, e2))
    nn = (n * n).sum(-1)
    a = torch.where(flat, a_flat, 0.5 * torch.where(flat, torch.ones_like(nn), nn).sqrt())
    o = vertices[:, 0:1].detach()
    t = ((p0 - o) * Mesh_Regularizer._face_normal(p1 - o, p2 - o)).sum(-1)
    a, t = torch.where(ok, a, torch.zeros_like(a)), torch.where(ok, t, torch.zeros_like(t))
    area, volume = a.double().sum(1), t.double().sum(1) / 6
    return area.to(vertices.dtype), volume.to(vertices.dtype)


def _hip_mesh_area_volume(vts, f32):
    """icn_mesh_measure_fwd on contiguous fp32 ROCm vertices and an int32 face table -> (area (B,), volume (B,))."""
    B, V, F = vts.shape[0], vts.shape[1], f32.shape[0]
    area = torch.empty(B, dtype=torch.float32, device=vts.device)
    volume = torch.empty(B, dtype=torch.float32, device=vts.device)
    _launch('icn_mesh_measure_fwd', _per_mesh(vts), f32, _NB, V, F, _per_mesh(area), _per_mesh(volume),
            workspace=('icn_mesh_measure_workspace_bytes', V, F))
    return area, volume


class _VertexGatherFn(torch.autograd.Function):
    """mesh_area_volume, cotangent_laplacian and angle_defect on the HIP path: hip_forward(vts, f32, offsets, corners) gives the
    outputs, and the backward entries (icn_mesh_measure_bwd, icn_mesh_cotlap_bwd, icn_mesh_angle_defect_bwd) share one argument
    list -- vertices, the three tables, one upstream per output, sizes, dvertices -- and one method: a gather over the vertex -> corner
    incidence table (built in the backward when the caller passed none), summed in a fixed order: bit-identical run to run.  An
    output nobody differentiates sends no gradient and its term is skipped; when none arrives at all, nothing is launched if
    skip_unused, else the entry writes zeros."""

    @staticmethod
    def forward(ctx, vertices, f32, offsets, corners, hip_forward, backward_entry, skip_unused):
        vts = vertices.contiguous()
        ctx.save_for_backward(vts, f32, offsets, corners)
        ctx.set_materialize_grads(False)
        ctx.backward_entry, ctx.skip_unused = backward_entry, skip_unused
        return hip_forward(vts, f32, offsets, corners)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *upstreams):
        if ctx.skip_unused and all(u is None for u in upstreams):
            return (None,) * 7
        vts, f32, offsets, corners = ctx.saved_tensors
        V, F = vts.shape[1], f32.shape[0]
        if offsets is None:
            offsets, corners = vertex_face_table(f32, V)
        dvts = torch.empty_like(vts)
        _launch(ctx.backward_entry, _per_mesh(vts), f32, offsets, corners, *(_per_mesh(_upstream(u)) for u in upstreams), _NB, V, F,
                _per_mesh(dvts))
        return (dvts,) + (None,) * 6


def _mesh_area_volume_unchecked(vertices, f32, table=None):
    """mesh_area_volume without its argument checks and without a host synchronisation, for callers that validated once
    (losses.Surface_Loss): f32 is an int32 (F, 3) tensor on the vertices' device, F >= 1; table = vertex_face_table(f32, V) on that
    device, or None (built in the backward).  A vertex id out of range is safe on either path: that face contributes nothing."""
    if _on_hip_path(vertices):
        if torch.is_grad_enabled() and vertices.requires_grad:
            offsets, corners = table if table is not None else (None, None)
            return _VertexGatherFn.apply(vertices, f32, offsets, corners, lambda vts, faces, *_: _hip_mesh_area_volume(vts, faces),
                                         'icn_mesh_measure_bwd', False)
        return _hip_mesh_area_volume(vertices.detach().contiguous(), f32)
    return _torch_mesh_area_volume(vertices, f32)


def _check_mesh_arguments(who, vertices, faces, table):
    """The argument checks of the mesh operators for `who`: shapes (ValueError), face ids against V with one read-back (IndexError),
    the table's shapes -> (int32 faces on the vertices' device, the table there or None)."""
    if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1 or not vertices.is_floating_point():
        raise ValueError('%s: expected floating-point vertices (B, V, 3), got %s' % (who, tuple(vertices.shape)))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError('%s: expected integer faces (F, 3) with F >= 1, got %s' % (who, tuple(faces.shape)))
    V, F = vertices.shape[1], faces.shape[0]
    if 3 * F > 0x7fffffff:
        raise ValueError('%s: %d faces: 3 F must fit an int32' % (who, F))
    dev = vertices.device
    if table is not None:
        if (not isinstance(table, (tuple, list)) or len(table) != 2 or any(not torch.is_tensor(x) or x.dtype != torch.int32 for x in table)
                or tuple(table[0].shape) != (V + 1,) or tuple(table[1].shape) != (3 * F,)):
            raise ValueError('%s: table must be vertex_face_table(faces, %d): int32 tensors (%d,) and (%d,)' % (who, V, V + 1, 3 * F))
        table = tuple(x.to(dev).contiguous() for x in table)
    f32 = faces.to(device=dev, dtype=torch.int32).contiguous()
    lo, hi = (int(x) for x in f32.aminmax())
    if lo < 0 or hi >= V:
        raise IndexError('%s: faces index [%d, %d] but there are %d vertices' % (who, lo, hi, V))
    return f32, table


def mesh_area_volume(vertices, faces, table=None):
    """(area (B,), volume (B,)) of the triangle meshes vertices (B, V, 3), faces (F, 3) integer and shared by the batch; the two
    global measures that show a mesh shrinking (the failure edge, normal-consistency and uniform-Laplacian regularisers share).

    One definition for the HIP kernels (include/icn_measure.h), the torch formulation and the tests.  For a face (i0, i1, i2):
        A_f = 0.5 |n|, n = (v1 - v0) x (v2 - v0) with every product of the cross product rounded on its own
              (Mesh_Regularizer._face_normal; face_normal on the device): a face with two coincident vertices has area exactly 0
        T_f = (v0 - o) . ((v1 - o) x (v2 - o)),  o = vertices[b, 0], the mesh's own vertex 0, held constant in the gradient
        area[b] = sum_f A_f;   volume[b] = sum_f T_f / 6
    The volume is signed: positive for outward (counter-clockwise seen from outside) winding, which is how every mesh of this
    package is wound.  For a closed, consistently wound mesh it does not depend on o; for an OPEN mesh it is the volume of the cone
    over o = vertex 0, a number that depends on which vertex comes first.  o is not optional: in fp32 the origin-based triple
    product of an I5 mesh of radius 0.75 translated by 10 is wrong by 8.5e-4 relative, about vertex 0 by 1.4e-7.
    Per-face values are computed in the vertices' dtype, both sums run in double in a fixed order, the outputs have the vertices'
    dtype.  Non-finite vertices propagate (NaN in, NaN out).  Differentiable in the vertices:
        d volume / d v_k = ((v_{k+1} - o) x (v_{k+2} - o)) / 6;   d area / d v_k = (n^ x (v_{k+2} - v_{k+1})) / 2,  n^ = n / |n|
    for corner k of a face, the area term taken as 0 where |n|^2 is 0 or not finite (the subgradient: a face without area never
    gives NaN).  ROCm fp32 tensors run on icn_mesh_measure_fwd / _bwd: the backward is a gather over `table` =
    vertex_face_table(faces, V) -- pass it when the face list is reused, else it is built when a gradient is asked for -- in a fixed
    order without atomics (bit-identical run to run, an exact zero at a vertex no face references).  ICN_NO_HIP_LOSS=1, CPU
    tensors and other dtypes take the torch formulation through autograd.
    Shapes are checked (ValueError); face ids against V with one read-back (IndexError)."""
    f32, table = _check_mesh_arguments('mesh_area_volume', vertices, faces, table)
    return _mesh_area_volume_unchecked(vertices, f32, table)


def volume_error(outvertices, refvertices, faces):
    """|vol_out - vol_ref| / |vol_ref| of one mesh pair ((V, 3) tensors sharing `faces`) as a Python float: the standard
    reconstruction figure beside the surface distance of compute_distance.  Volumes as mesh_area_volume defines them."""
    if outvertices.dim() != 2 or refvertices.dim() != 2:
        raise ValueError('volume_error: expected (V, 3) vertices, got %s and %s' % (tuple(outvertices.shape), tuple(refvertices.shape)))
    vol_out = mesh_area_volume(outvertices[None], faces)[1]
    vol_ref = mesh_area_volume(refvertices[None], faces)[1]
    return float((vol_out - vol_ref).abs() / vol_ref.abs())


# ---- cotangent Laplacian and Willmore bending energy ------------------------------------------------------------------------------
def _torch_cotangent_laplacian(vertices, faces):
    """The definition of cotangent_laplacian in torch, differentiable in the vertices through autograd: (lap (B, V, 3), varea (B, V))
    in the vertices' dtype."""
    from .losses import Mesh_Regularizer
    V = vertices.shape[1]
    ids = faces.long()
    ok = ((ids >= 0) & (ids < V)).all(-1)                                                 # (F,): the others take no part
    ids = ids.clamp(0, V - 1)
    tri = vertices[:, ids]                                                                # (B, F, 3 corners, 3)
    with torch.no_grad():
        nn = (Mesh_Regularizer._face_normal(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]) ** 2).sum(-1)
        flat = ~((nn > 0) & torch.isfinite(nn)) | ~ok                                     # unresolved: nothing to lap, the subgradient 0
        a_flat = torch.where(ok, 0.5 * nn.sqrt(), torch.zeros_like(nn))                   # ... and its area all the same (NaN stays NaN)
    # an unresolved face enters autograd as a zero triangle: its vertices meet no arithmetic that autograd records
    tri = torch.where(flat[..., None, None], torch.zeros_like(tri), tri)
    p = [tri[:, :, k] for k in range(3)]
    n = Mesh_Regularizer._face_normal(p[1] - p[0], p[2] - p[0])
    length = torch.where(flat, torch.ones_like(nn), (n * n).sum(-1)).sqrt()
    unit = n / length[..., None]                                                          # 0 for a zero triangle
    a = torch.where(flat, a_flat, 0.5 * length)
    lap = torch.zeros_like(vertices)
    varea = torch.zeros_like(vertices[..., 0])
    for k in range(3):
        lap = lap.index_add(1, ids[:, k], -0.5 * Mesh_Regularizer._face_normal(unit, p[(k + 2) % 3] - p[(k + 1) % 3]))
        varea = varea.index_add(1, ids[:, k], a)
    return lap, varea / 3


def _willmore_from(lap, varea):
    """energy (B,) = sum_i |lap_i|^2 / (4 varea_i) over the vertices with varea_i != 0, summed in float64; no gradient passes through
    the others."""
    has = varea != 0                                                                      # NaN counts: it propagates
    lap = torch.where(has[..., None], lap, torch.zeros_like(lap))
    w = (lap * lap).sum(-1) / (4 * torch.where(has, varea, torch.ones_like(varea)))
    return w.double().sum(1).to(lap.dtype)


def _torch_willmore_energy(vertices, faces):
    """The definition of willmore_energy in torch, differentiable in the vertices through autograd."""
    return _willmore_from(*_torch_cotangent_laplacian(vertices, faces))


def _hip_cotangent_laplacian(vts, f32, offsets, corners):
    """icn_mesh_cotlap_fwd on contiguous fp32 ROCm vertices, an int32 face table and its incidence table -> (lap (B, V, 3), varea
    (B, V))."""
    B, V, F = vts.shape[0], vts.shape[1], f32.shape[0]
    lap = torch.empty_like(vts)
    varea = torch.empty(B, V, dtype=torch.float32, device=vts.device)
    _launch('icn_mesh_cotlap_fwd', _per_mesh(vts), f32, offsets, corners, _NB, V, F, _per_mesh(lap), _per_mesh(varea))
    return lap, varea


def _hip_willmore_energy(vts, f32, offsets, corners):
    """icn_mesh_willmore_fwd, arguments as _hip_cotangent_laplacian -> (lap (B, V, 3), varea (B, V), energy (B,))."""
    B, V, F = vts.shape[0], vts.shape[1], f32.shape[0]
    lap = torch.empty_like(vts)
    varea = torch.empty(B, V, dtype=torch.float32, device=vts.device)
    energy = torch.empty(B, dtype=torch.float32, device=vts.device)
    _launch('icn_mesh_willmore_fwd', _per_mesh(vts), f32, offsets, corners, _NB, V, F, _per_mesh(lap), _per_mesh(varea),
            _per_mesh(energy), workspace=('icn_mesh_willmore_workspace_bytes', V, F))
    return lap, varea, energy


class _WillmoreFn(torch.autograd.Function):
    """willmore_energy on the HIP path (icn_mesh_willmore_fwd / _bwd in include/icn_curvature.h).  The forward keeps lap and varea for
    the backward: the per-vertex upstreams, then the gather of icn_mesh_cotlap_bwd; a fixed order, bit-identical run to run.  When no
    gradient arrives nothing is launched."""

    @staticmethod
    def forward(ctx, vertices, f32, offsets, corners):
        vts = vertices.contiguous()
        lap, varea, energy = _hip_willmore_energy(vts, f32, offsets, corners)
        ctx.save_for_backward(vts, f32, offsets, corners, lap, varea)
        ctx.set_materialize_grads(False)
        return energy

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, denergy):
        if denergy is None:
            return None, None, None, None
        vts, f32, offsets, corners, lap, varea = ctx.saved_tensors
        V, F = vts.shape[1], f32.shape[0]
        dvts = torch.empty_like(vts)
        _launch('icn_mesh_willmore_bwd', _per_mesh(vts), f32, offsets, corners, _per_mesh(lap), _per_mesh(varea),
                _per_mesh(_upstream(denergy)), _NB, V, F, _per_mesh(dvts), workspace=('icn_mesh_willmore_workspace_bytes', V, F))
        return dvts, None, None, None


def _cotangent_laplacian_unchecked(vertices, f32, table=None):
    """cotangent_laplacian without its argument checks and without a host synchronisation, for callers that validated once: f32 is an
    int32 (F, 3) tensor on the vertices' device, F >= 1; table = vertex_face_table(f32, V) on that device, or None (built here: the
    forward gathers over it too).  A vertex id out of range is safe on either path: that face takes no part."""
    if _on_hip_path(vertices):
        offsets, corners = table if table is not None else vertex_face_table(f32, vertices.shape[1])
        if torch.is_grad_enabled() and vertices.requires_grad:
            return _VertexGatherFn.apply(vertices, f32, offsets, corners, _hip_cotangent_laplacian, 'icn_mesh_cotlap_bwd', True)
        return _hip_cotangent_laplacian(vertices.detach().contiguous(), f32, offsets, corners)
    return _torch_cotangent_laplacian(vertices, f32)


def _willmore_energy_unchecked(vertices, f32, table=None):
    """willmore_energy without its argument checks and without a host synchronisation (losses.Surface_Loss); arguments as
    _cotangent_laplacian_unchecked."""
    if _on_hip_path(vertices):
        offsets, corners = table if table is not None else vertex_face_table(f32, vertices.shape[1])
        if torch.is_grad_enabled() and vertices.requires_grad:
            return _WillmoreFn.apply(vertices, f32, offsets, corners)
        return _hip_willmore_energy(vertices.detach().contiguous(), f32, offsets, corners)[2]
    return _torch_willmore_energy(vertices, f32)


def cotangent_laplacian(vertices, faces, table=None):
    """(lap (B, V, 3), varea (B, V)) of the triangle meshes vertices (B, V, 3), faces (F, 3) integer and shared by the batch: the
    integrated cotangent Laplace-Beltrami operator and the barycentric vertex area -- the smoothness measure that is weighted by
    the triangles, not by vertex valence, and that does not drag vertices tangentially the way the uniform umbrella does.

    One definition for the HIP kernels (include/icn_curvature.h), the torch formulation and the tests.  For a face (i0, i1, i2):
        n = (v1 - v0) x (v2 - v0) with every product of the cross product rounded on its own (as mesh_area_volume), A_f = 0.5 |n|;
        the face is RESOLVED iff |n|^2 > 0 and |n|^2 is finite
    and for a vertex i, with k the corner of f that sits at i and corner indices taken modulo 3:
        varea_i = (sum_{f at i} A_f) / 3
        lap_i   = - sum_{f at i, resolved} 0.5 n^_f x (v_{k+2} - v_{k+1}),   n^ = n / |n|
    lap_i equals the textbook sum_j 0.5 (cot alpha_ij + cot beta_ij)(v_j - v_i) over the neighbours j of i, alpha and beta the two
    angles opposite edge (i, j), because that sum is - d area / d v_i (both to 2e-16 in float64 on icospheres); the cross product
    form divides by |n| only, never by a sine: a needle triangle costs one factor of its aspect ratio, no cotangent overflows.
    lap_i = 2 varea_i H normal with H the mean curvature.  An unresolved face adds nothing to lap (and its area, exactly 0 for
    coincident vertices, to varea); a vertex no face references has lap = 0 and varea = 0 exactly; non-finite vertices propagate.
    Differentiable in the vertices; the gradient treats an unresolved face as the subgradient 0, through lap and through varea.
    ROCm fp32 tensors run on icn_mesh_cotlap_fwd / _bwd, one thread per (mesh, vertex) gathering over `table` =
    vertex_face_table(faces, V) in a fixed order without atomics (bit-identical run to run) -- pass the table when the face list is
    reused, else it is built on entry: here the forward needs it too.  ICN_NO_HIP_LOSS=1, CPU tensors and other dtypes take the
    torch formulation through autograd.
    Shapes are checked (ValueError); face ids against V with one read-back (IndexError)."""
    f32, table = _check_mesh_arguments('cotangent_laplacian', vertices, faces, table)
    return _cotangent_laplacian_unchecked(vertices, f32, table)


def willmore_energy(vertices, faces, table=None):
    """W (B,) of the triangle meshes vertices (B, V, 3), faces (F, 3): the discrete Willmore bending energy, the integral of H^2,
        w_i = |lap_i|^2 / (4 varea_i) where varea_i != 0, else 0 (and no gradient passes through vertex i);   W[b] = sum_i w_i
    with (lap, varea) = cotangent_laplacian(vertices, faces): w_i = H^2 varea_i.  W is invariant under scaling, rotation and
    translation and is 4 pi for a sphere of any radius (W / 4 pi of the unit icosphere: 0.762, 0.931, 0.982, 0.996 for 0 .. 3
    subdivisions), so it cannot be lowered by shrinking the mesh -- the failure the edge, normal-consistency and umbrella
    regularisers share.  Summed in double in a fixed order, the output has the vertices' dtype; non-finite vertices propagate.
    Differentiable in the vertices.  ROCm fp32 tensors run on icn_mesh_willmore_fwd / _bwd (include/icn_curvature.h), which keep
    lap and varea of the forward for the backward; paths, `table` and checks as cotangent_laplacian."""
    f32, table = _check_mesh_arguments('willmore_energy', vertices, faces, table)
    return _willmore_energy_unchecked(vertices, f32, table)


# ---- Gaussian curvature by angle defect ---------------------------------------------------------------------------------------------
_TWO_PI = 6.283185307179586


def _torch_angle_defect(vertices, faces):
    """The definition of angle_defect in torch, differentiable in the vertices through autograd: float64 up to the final rounding,
    defect (B, V) in the vertices' dtype."""
    from .losses import Mesh_Regularizer
    V = vertices.shape[1]
    ids = faces.long()
    ok = ((ids >= 0) & (ids < V)).all(-1)                                                 # (F,): the others take no part
    ids = ids.clamp(0, V - 1)
    tri = vertices.double()[:, ids]                                                       # (B, F, 3 corners, 3)
    with torch.no_grad():
        nn = (Mesh_Regularizer._face_normal(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0]) ** 2).sum(-1)
        flat = ~(nn != 0) | ~ok                                                           # unresolved (NaN is not: it propagates)
        # an unresolved face enters autograd as a fixed right triangle whose angles are then dropped: its vertices meet no
        # arithmetic that autograd records, and no atan2(0, 0) or sqrt(0) gives a NaN gradient
        safe = torch.eye(3, dtype=tri.dtype, device=tri.device)
    tri = torch.where(flat[..., None, None], safe, tri)
    p = [tri[:, :, k] for k in range(3)]
    n = Mesh_Regularizer._face_normal(p[1] - p[0], p[2] - p[0])
    length = (n * n).sum(-1).sqrt()
    total = torch.zeros(vertices.shape[:2], dtype=tri.dtype, device=tri.device)
    count = torch.zeros_like(total)
    live = (~flat).to(tri.dtype)
    for k in range(3):
        a, b = p[(k + 1) % 3] - p[k], p[(k + 2) % 3] - p[k]
        theta = torch.atan2(length, (a * b).sum(-1))
        total = total.index_add(1, ids[:, k], torch.where(flat, torch.zeros_like(theta), theta))
        count = count.index_add(1, ids[:, k], live)
    return torch.where(count > 0, _TWO_PI - total, torch.zeros_like(total)).to(vertices.dtype)


def _hip_angle_defect(vts, f32, offsets, corners):
    """icn_mesh_angle_defect_fwd on contiguous fp32 ROCm vertices, an int32 face table and its incidence table -> defect (B, V)."""
    B, V, F = vts.shape[0], vts.shape[1], f32.shape[0]
    defect = torch.empty(B, V, dtype=torch.float32, device=vts.device)
    _launch('icn_mesh_angle_defect_fwd', _per_mesh(vts), f32, offsets, corners, _NB, V, F, _per_mesh(defect))
    return defect


def _angle_defect_unchecked(vertices, f32, table=None):
    """angle_defect without its argument checks and without a host synchronisation (losses.Surface_Loss); arguments as
    _cotangent_laplacian_unchecked."""
    if _on_hip_path(vertices):
        offsets, corners = table if table is not None else vertex_face_table(f32, vertices.shape[1])
        if torch.is_grad_enabled() and vertices.requires_grad:
            return _VertexGatherFn.apply(vertices, f32, offsets, corners, _hip_angle_defect, 'icn_mesh_angle_defect_bwd', True)
        return _hip_angle_defect(vertices.detach().contiguous(), f32, offsets, corners)
    return _torch_angle_defect(vertices, f32)


def _gaussian_curvature_unchecked(vertices, f32, table=None):
    """gaussian_curvature without its argument checks and without a host synchronisation; arguments as
    _cotangent_laplacian_unchecked (on the HIP path the table is built once here and serves both operators)."""
    if table is None and _on_hip_path(vertices):
        table = vertex_face_table(f32, vertices.shape[1])
    defect = _angle_defect_unchecked(vertices, f32, table)
    varea = _cotangent_laplacian_unchecked(vertices, f32, table)[1]
    has = varea != 0                                                                      # NaN counts: it propagates
    return torch.where(has, defect, torch.zeros_like(defect)) / torch.where(has, varea, torch.ones_like(varea))


def angle_defect(vertices, faces, table=None):
    """defect (B, V) of the triangle meshes vertices (B, V, 3), faces (F, 3) integer and shared by the batch: the angle defect
    2 pi - sum theta at every vertex, which is the discrete GAUSSIAN curvature integrated over the vertex's cell.  It is intrinsic
    (unchanged by bending without stretching), dimensionless (invariant under scaling, rotation and translation), and by
    Gauss-Bonnet it sums to 2 pi chi over a closed mesh: 4 pi for every sphere, whatever its shape (total_curvature).

    One definition for the HIP kernels (include/icn_gauss.h), the torch formulation and the tests.  All arithmetic up to the final
    rounding is float64, whatever the vertices' dtype; the output has the vertices' dtype.  For a face (i0, i1, i2) and its corner k,
    corner indices modulo 3:
        a = v_{k+1} - v_k,  b = v_{k+2} - v_k,  n = (v1 - v0) x (v2 - v0) with every product of the cross product rounded on its own
        theta_k = atan2(|n|, a . b)                      (|a x b| = |n| at every corner; no rounded cosine ever meets an acos)
        the face is RESOLVED iff |n|^2 != 0              (a face with two coincident vertices has n exactly 0)
        defect_i = 2 pi - sum_{resolved f at i} theta_k(f),   exactly 0 at a vertex that has no resolved face
    An unresolved face adds no angle and sends no gradient; a vertex no face references, or all of whose faces are unresolved, has
    defect 0 exactly (as lap and varea of cotangent_laplacian); non-finite vertices propagate NaN into their own mesh only.
    Why float64: written in fp32 the defect carries an absolute error of 8 - 22 units of 2^-24, about 1e-6 whatever the resolution,
    while the defect of a smooth I5 mesh is itself 1.1e-3 .. 1.5e-3; the errors do not average out (the fp32 I5 total misses 4 pi by
    1.8e-3, float64 by 2e-13).
    Differentiable in the vertices.  For L = sum_i g_i defect_i a resolved face sends to its corner k, with n^ = n / |n|,
        (g_{k+1} - g_k) (n^ x a) / |a|^2  +  (g_k - g_{k+2}) (n^ x b) / |b|^2
    and the HIP backward computes exactly this difference form: a uniform upstream gives a gradient of exactly 0 at every vertex
    (the total curvature cannot be changed), which autograd of the torch formulation reaches only to rounding.
    ROCm fp32 tensors run on icn_mesh_angle_defect_fwd / _bwd, one thread per (mesh, vertex) gathering over `table` =
    vertex_face_table(faces, V) in double in a fixed order without atomics (bit-identical run to run); paths, `table` and checks as
    cotangent_laplacian.  Cost on an MI355X: see losses.Surface_Loss (factor_gauss)."""
    f32, table = _check_mesh_arguments('angle_defect', vertices, faces, table)
    return _angle_defect_unchecked(vertices, f32, table)


def gaussian_curvature(vertices, faces, table=None):
    """K (B, V) = defect_i / varea_i, the pointwise Gaussian curvature: angle_defect over the barycentric vertex area of
    cotangent_laplacian; 0 where varea_i = 0, and no gradient passes there.  1 / R^2 on a sphere of radius R (on the icosphere the
    six-valent vertices narrow towards it, 1.045 at one subdivision and 1.0001 at three; the twelve five-valent vertices stay near
    1.146, because a third of the incident area is not their Voronoi cell).  Together with lap = 2 varea H normal this completes the
    pair (H, K).  Differentiable in the vertices, on the HIP path through the kernels of both operators; paths, `table` and checks
    as cotangent_laplacian."""
    f32, table = _check_mesh_arguments('gaussian_curvature', vertices, faces, table)
    return _gaussian_curvature_unchecked(vertices, f32, table)


def total_curvature(vertices, faces, table=None):
    """(B,): sum_i defect_i of angle_defect, summed in double, in the vertices' dtype.  By Gauss-Bonnet it is 2 pi chi for a closed
    mesh -- 4 pi for a sphere, 0 for a torus -- and 2 pi for a disc: the cheapest check that a face list is a closed sphere, and a
    constant of the vertices (its gradient vanishes)."""
    f32, table = _check_mesh_arguments('total_curvature', vertices, faces, table)
    return _angle_defect_unchecked(vertices, f32, table).double().sum(1).to(vertices.dtype)


def curvature_error(outvertices, refvertices, faces):
    """sqrt(sum_i (defect_out_i - defect_ref_i)^2 / sum_i defect_ref_i^2) of one mesh pair ((V, 3) tensors sharing `faces`) as a
    Python float, to stand beside volume_error and compute_distance: how far the output's Gaussian curvature is from the
    reference's, vertex by vertex.  Defects as angle_defect defines them."""
    if outvertices.dim() != 2 or refvertices.dim() != 2:
        raise ValueError('curvature_error: expected (V, 3) vertices, got %s and %s' % (tuple(outvertices.shape), tuple(refvertices.shape)))
    d_out = angle_defect(outvertices[None], faces).double()
    d_ref = angle_defect(refvertices[None], faces).double()
    return float(((d_out - d_ref) ** 2).sum().sqrt() / (d_ref ** 2).sum().sqrt())


# ---- self-intersection count --------------------------------------------------------------------------------------------------------
_SELF_INTERSECT_MAX_FACES = 1 << 20     # ICN_SELF_INTERSECT_MAX_FACES of include/icn_isect.h: the work is quadratic in F
_SELF_INTERSECT_CHUNK_PAIRS = 1 << 18   # pairs (mesh, i, j) the torch formulation holds at once: about 2 MiB per temporary


def _orient(a, b, c, d):
    """orient of self_intersections on (..., 3) tensors, in exactly the order of the definition (no FMA: one kernel per operation)."""
    ux, uy, uz = (b - a).unbind(-1)
    vx, vy, vz = (c - a).unbind(-1)
    wx, wy, wz = (d - a).unbind(-1)
    return ux * (vy * wz - vz * wy) - uy * (vx * wz - vz * wx) + uz * (vx * wy - vy * wx)


def _crosses(p, q, sp, sq, tri):
    """crosses of self_intersections: the segment (p, q) with plane values sp, sq against the triangle tri = (a, b, c)."""
    a, b, c = tri
    o0, o1, o2 = _orient(p, q, a, b), _orient(p, q, b, c), _orient(p, q, c, a)
    return (((sp > 0) & (sq < 0)) | ((sp < 0) & (sq > 0))) & (((o0 > 0) & (o1 > 0) & (o2 > 0)) | ((o0 < 0) & (o1 < 0) & (o2 < 0)))


def _staged_faces(vertices, faces):
    """(ids (F, 3) int64, tri (B, F, 3 corners, 3) float64, valid (B, F)) of self_intersections: a face is valid iff its ids index V
    vertices and its nine coordinates are finite; an invalid face is staged as zeros and meets no arithmetic."""
    V = vertices.shape[1]
    ids = faces.long()
    ids_ok = ((ids >= 0) & (ids < V)).all(-1)                                             # (F,)
    tri = vertices.detach().double()[:, ids.clamp(0, V - 1)]
    valid = ids_ok & torch.isfinite(tri).all(-1).all(-1)
    return ids, torch.where(valid[..., None, None], tri, torch.zeros_like(tri)), valid


def _torch_intersecting_pairs(vertices, faces, lo, hi, staged=None):
    """The definition of self_intersections in torch, float64 on the vertices as stored, for the faces i in [lo, hi) against all
    faces j -> bool (B, hi - lo, F): whether faces i and j of mesh b intersect.  staged: _staged_faces(vertices, faces), for a
    caller that walks the rows in chunks."""
    ids, tri, valid = staged if staged is not None else _staged_faces(vertices, faces)
    index = torch.arange(ids.shape[0], device=vertices.device)
    shared = (ids[lo:hi, None, :, None] == ids[None, :, None, :]).any(-1).any(-1)         # (C, F); a face shares its ids with itself
    tested = valid[:, lo:hi, None] & valid[:, None, :] & ~shared                          # (B, C, F)
    first = (index[lo:hi, None] < index[None, :])[None, :, :, None]                       # face i is A where i < j
    mine, other = tri[:, lo:hi, None], tri[:, None, :]                                    # (B, C, 1, 3, 3), (B, 1, F, 3, 3)
    A = [torch.where(first, mine[..., k, :], other[..., k, :]) for k in range(3)]
    Bt = [torch.where(first, other[..., k, :], mine[..., k, :]) for k in range(3)]
    sa = [_orient(Bt[0], Bt[1], Bt[2], A[k]) for k in range(3)]                           # the plane value of a vertex serves both
    sb = [_orient(A[0], A[1], A[2], Bt[k]) for k in range(3)]                             # edges that end in it
    hit = torch.zeros_like(tested)
    for k in range(3):
        hit = hit | _crosses(A[k], A[(k + 1) % 3], sa[k], sa[(k + 1) % 3], Bt)
    for k in range(3):
        hit = hit | _crosses(Bt[k], Bt[(k + 1) % 3], sb[k], sb[(k + 1) % 3], A)
    return hit & tested


def _torch_self_intersections(vertices, faces, chunk=None):
    """hits (B, F) int32 of self_intersections from the torch formulation, rows i in chunks against all faces j so that memory
    stays bounded: `chunk` rows at once, by default as many as keep B * chunk * F near 2^18 pairs."""
    B, F = vertices.shape[0], faces.shape[0]
    hits = torch.empty(B, F, dtype=torch.int32, device=vertices.device)
    rows = int(chunk) if chunk is not None else max(1, _SELF_INTERSECT_CHUNK_PAIRS // (B * F))
    staged = _staged_faces(vertices, faces)
    for lo in range(0, F, rows):
        hi = min(lo + rows, F)
        hits[:, lo:hi] = _torch_intersecting_pairs(vertices, faces, lo, hi, staged).sum(-1, dtype=torch.int32)
    return hits


def _hip_self_intersections(vts, f32):
    """icn_mesh_self_intersect on contiguous fp32 ROCm vertices and an int32 face table -> hits (B, F) int32."""
    B, V, F = vts.shape[0], vts.shape[1], f32.shape[0]
    hits = torch.empty(B, F, dtype=torch.int32, device=vts.device)
    _launch('icn_mesh_self_intersect', _per_mesh(vts), f32, _NB, V, F, _per_mesh(hits))
    return hits


def _self_intersections_unchecked(vertices, f32):
    """self_intersections without its argument checks and without a host synchronisation, for callers that validated once: f32 is an
    int32 (F, 3) tensor on the vertices' device, 1 <= F <= 2^20.  A vertex id out of range is safe on either path: that face
    neither hits nor is hit."""
    if _on_hip_path(vertices):
        hits = _hip_self_intersections(vertices.detach().contiguous(), f32)
    else:
        hits = _torch_self_intersections(vertices, f32)
    return hits.sum(1, dtype=torch.int64) // 2, hits


def self_intersections(vertices, faces):
    """(pairs (B,) int64, hits (B, F) int32) of the triangle meshes vertices (B, V, 3), faces (F, 3) integer and shared by the batch:
    hits[b, i] is the number of faces of mesh b that face i passes through, pairs[b] = hits[b].sum() // 2 the number of intersecting
    pairs.  What tells whether the regularisers of losses.Surface_Loss kept the output from folding over itself: every other metric
    of this module stays finite and unremarkable on a mesh that passes through itself.  Never requires grad.

    One definition for the HIP kernel (include/icn_isect.h), the torch formulation and the tests.  All arithmetic is float64 on the
    vertices as stored, every product and sum rounded on its own, in exactly the order written:
        orient(a, b, c, d) = u.x (v.y w.z - v.z w.y) - u.y (v.x w.z - v.z w.x) + u.z (v.x w.y - v.y w.x),  u = b - a, v = c - a, w = d - a
        crosses(p, q; a, b, c), a segment against a triangle:  orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs
            (signs are compared; no product that can underflow), and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0
            or all < 0
        faces i < j INTERSECT iff one of six tests holds: crosses for each edge (A_k, A_{k+1}) of A = face i against B = face j,
            then for each edge of B against A -- always with the lower face index as A, so the relation is symmetric by construction
    A pair is not tested, and does not intersect, if the two faces share a vertex id (neighbours, duplicate faces), if either has a
    vertex id outside [0, V) (only the unchecked form lets one through), or if either has a coordinate that is not finite.  The strict
    inequalities make every touching or coplanar contact a non-intersection; in general position two triangles that meet always have
    an edge piercing an interior, so the test is complete there.  A face without area can pierce another face with an edge; nothing
    can pierce it.
    ROCm fp32 tensors run on icn_mesh_self_intersect: one thread per (mesh, face) against all faces of its mesh, staged through LDS;
    pairs whose fp32 bounding boxes do not overlap are rejected before any double arithmetic (exact and conservative: no result
    changes), no atomics, bit-identical run to run -- and equal to the float64 formulation integer for integer, because both do the
    same IEEE operations in the same order.  ICN_NO_HIP_LOSS=1, CPU tensors and other dtypes take that formulation in torch
    (_torch_self_intersections), chunked over rows so that memory stays bounded.  The work is F^2 pairs per mesh: F > 2^20 is refused.
    Cost on an MI355X at I5 / batch 36 (20 480 faces, 7.5e9 pairs; profiles/self_intersect.txt from tools/time_self_intersect.py):
    8.7 ms on the unit icosphere, where all but 464 pairs per mesh end at the box test and the scan over the boxes is everything,
    and 15.4 ms with Gaussian vertex noise of sigma 0.05 (91 % of the faces hit), where 19 pairs per face reach the double
    arithmetic -- beside 29.5 and 28.0 ms for k_point_to_mesh on as many points in the same process, 0.30 and 0.55 of it.  On the
    noisy input the exact tests take 6.7 of the 15.4 ms, 44 %: they weigh as much as the scan but do not dominate it, and few
    lanes of a wave are in them at once; a grid broad phase would cut the scan, not them.  One mesh alone takes 3.8 ms (80
    workgroups do not fill the device), the torch float64 formulation on the device 1.58 s for it, 410 times as long.
    Shapes and F > 2^20 are checked (ValueError); face ids against V with one read-back (IndexError)."""
    who = 'self_intersections'
    if faces.dim() == 2 and faces.shape[0] > _SELF_INTERSECT_MAX_FACES:
        raise ValueError('%s: %d faces: at most %d (the work is quadratic in F)' % (who, faces.shape[0], _SELF_INTERSECT_MAX_FACES))
    f32, _ = _check_mesh_arguments(who, vertices, faces, None)
    return _self_intersections_unchecked(vertices, f32)


def self_intersection_ratio(vertices, faces):
    """The share of faces of one mesh ((V, 3) vertices, `faces`) that intersect another face of the same mesh, as a Python float: the
    self-intersection figure of the mesh-generation literature, to stand beside curvature_error, volume_error and compute_distance.
    Intersections as self_intersections defines them."""
    if vertices.dim() != 2:
        raise ValueError('self_intersection_ratio: expected (V, 3) vertices, got %s' % (tuple(vertices.shape),))
    hits = self_intersections(vertices[None], faces)[1]
    return float((hits > 0).sum()) / hits.shape[1]


# ---- signed distance, inside test and volumetric IoU ----------------------------------------------------------------------------------
def _edge_twins(f32, V):
    """(adjacency int32 (F, 3), report int64 (8,)) of a face list, without a host synchronisation.  Corner c = 3 f + e stands for the
    directed edge e of face f, (faces[f][e], faces[f][(e + 1) % 3]); its key is a V + b, and adjacency[f][e] is the face of the lowest
    corner whose key is the twin's, b V + a, or -1: the keys of all 3 F directed edges are sorted (stably, in int64) and the twin keys
    searched in them.  An edge with a vertex id outside [0, V) has no key and no twin.  report = (lowest id, highest id, the number of
    edges without a twin and the (a, b) of the first, the number of directed edges that occur again and the (a, b) of the first): what
    the checked functions read back in one piece."""
    f = f32.long()
    a, b = f.reshape(-1), torch.roll(f, -1, 1).reshape(-1)                                # (no index list: that would be a copy to the device)
    valid = (a >= 0) & (a < V) & (b >= 0) & (b < V)
    key = torch.where(valid, a * V + b, torch.full_like(a, V * V))
    twin = torch.where(valid, b * V + a, torch.full_like(a, -1))
    ordered, corner = torch.sort(key, stable=True)
    at = torch.searchsorted(ordered, twin).clamp(max=key.numel() - 1)
    found = ordered[at] == twin
    adjacency = torch.where(found, corner[at] // 3, torch.full_like(at, -1))
    again = torch.zeros_like(valid)
    again[1:] = (ordered[1:] == ordered[:-1]) & (ordered[1:] < V * V)
    first_open = (~found).to(torch.int8).argmax().reshape(1)
    first_again = corner.index_select(0, again.to(torch.int8).argmax().reshape(1))
    lo, hi = f.aminmax()
    report = torch.cat([lo.reshape(1), hi.reshape(1), (~found).sum().reshape(1), a.index_select(0, first_open), b.index_select(0, first_open),
                        again.sum().reshape(1), a.index_select(0, first_again), b.index_select(0, first_again)])
    return adjacency.reshape(-1, 3).to(torch.int32), report


def signed_distance_tables(faces, num_vertices):
    """(adjacency int32 (F, 3), offsets int32 (V + 1), corners int32 (3 F)) on the faces' device: what the sign of
    signed_point_to_mesh_distance reads besides the face list, built once per face list without a host synchronisation.
    adjacency[f][e] is the face that holds the directed edge opposite to edge e of f -- the face across edge (e, e + 1) of a
    consistently wound mesh -- or -1 (see _edge_twins); (offsets, corners) is vertex_face_table(faces, num_vertices)."""
    V = int(num_vertices)
    offsets, corners = vertex_face_table(faces, V)                                        # checks faces and V
    return (_edge_twins(faces, V)[0], offsets, corners)


def _torch_point_to_mesh_sign(points, vertices, faces, face, kind, tables):
    """The definition of the sign of signed_point_to_mesh_distance in torch: float64 whatever the inputs' dtype, sign (B, P) in
    float64, -1 or +1.  Vectorised: every point evaluates the plane, the three segments and the vertex sum and selects by kind;
    the vertex sum walks the incidence slices slot by slot in slice order, padded to the longest slice (one read-back of that
    length: the HIP path has none)."""
    from .losses import Mesh_Regularizer
    adjacency, offsets, corners = tables
    B, P, _ = points.shape
    V, F = vertices.shape[1], faces.shape[0]
    nc = 3 * F
    p, v, ids_all = points.detach().double(), vertices.detach().double(), faces.long()
    flat_ids = ids_all.reshape(-1)
    face, kind = face.long(), kind.long()
    rows = torch.arange(B, device=p.device)[:, None]

    def resolved_normals(fid, ok):
        """(the three vertices, n, |n|^2, usable) of faces fid (B, P) where ok: ids clamped before they index anything."""
        ids = ids_all[fid.clamp(0, F - 1)]                                                # (B, P, 3)
        ok = ok & (fid >= 0) & (fid < F) & ((ids >= 0) & (ids < V)).all(-1)
        tri = v[rows[..., None], ids.clamp(0, V - 1)]                                     # (B, P, 3 corners, 3)
        n = Mesh_Regularizer._face_normal(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0])
        return ids, tri, n, (n * n).sum(-1), ok

    def unit(n, nn, use, w=None):
        """w n / |n| where use and the normal is resolved (NaN counts), else 0."""
        use = use & (nn != 0)
        u = n / torch.where(use, nn, torch.ones_like(nn)).sqrt()[..., None]
        if w is not None:
            u = w[..., None] * u
        return torch.where(use[..., None], u, torch.zeros_like(u))

    def segment(up, uw):
        den = (uw * uw).sum(-1)
        t = torch.where(den != 0, (uw * up).sum(-1) / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(den))
        t = torch.where(t > 0, torch.where(t < 1, t, torch.ones_like(t)), torch.zeros_like(t))
        return up - uw * t[..., None]
    ids, tri, n, nn, ok = resolved_normals(face, (kind >= 0) & (kind <= 6))
    a, b, c = tri[:, :, 0], tri[:, :, 1], tri[:, :, 2]
    ab, ac, ap = b - a, c - a, p - a
    # kind 0: the plane
    s = torch.where(nn != 0, (ap * n).sum(-1) / torch.where(nn != 0, nn, torch.ones_like(nn)), torch.zeros_like(nn))
    d, N = n * s[..., None], n
    # kind 4 / 5 / 6: the edge's segment, this face and the one across
    edge = (kind - 4).clamp(0, 2)
    g = torch.gather(adjacency.long()[face.clamp(0, F - 1)], 2, edge[..., None])[..., 0]
    _, _, m, mm, g_ok = resolved_normals(g, kind >= 4)
    N_edge = unit(n, nn, ok) + unit(m, mm, g_ok)
    for k, dk in ((4, segment(ap, ab)), (5, segment(p - b, c - b)), (6, segment(ap, ac))):
        d = torch.where((kind == k)[..., None], dk, d)
    N = torch.where((kind >= 4)[..., None], N_edge, N)
    # kind 1 / 2 / 3: the vertex, every resolved face of its slice by its angle
    at_vertex = ok & (kind >= 1) & (kind <= 3)
    local = (kind - 1).clamp(0, 2)
    j = torch.gather(ids, 2, local[..., None])[..., 0].clamp(0, V - 1)                    # (B, P)
    pj = torch.gather(tri, 2, local[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
    lo, hi = offsets.long()[j].clamp(0, nc), offsets.long()[j + 1].clamp(0, nc)
    longest = int(torch.where(at_vertex, hi - lo, torch.zeros_like(lo)).max()) if at_vertex.numel() else 0
    N_vertex = torch.zeros_like(d)
    for slot in range(longest):
        entry = lo + slot
        cid = corners.long()[entry.clamp(0, nc - 1)]
        use = at_vertex & (entry < hi) & (cid >= 0) & (cid < nc)
        use = use & (flat_ids[cid.clamp(0, nc - 1)] == j)
        fid, k = cid.clamp(0, nc - 1) // 3, cid.clamp(0, nc - 1) % 3
        fids, ftri, fn, fnn, use = resolved_normals(fid, use)
        q1 = torch.gather(ftri, 2, ((k + 1) % 3)[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
        q2 = torch.gather(ftri, 2, ((k + 2) % 3)[..., None, None].expand(-1, -1, 1, 3))[:, :, 0]
        ea, eb = q1 - pj, q2 - pj
        live = use & (fnn != 0)
        theta = torch.atan2(torch.where(live, fnn, torch.ones_like(fnn)).sqrt(), (ea * eb).sum(-1))
        N_vertex = N_vertex + unit(fn, fnn, use, theta)
    d = torch.where(at_vertex[..., None], p - pj, d)
    N = torch.where(at_vertex[..., None], N_vertex, N)
    inside = ok & ((d * N).sum(-1) < 0)
    return torch.where(inside, -torch.ones_like(nn), torch.ones_like(nn))


def _hip_point_to_mesh_sign(pts, vts, f32, tables, face, kind):
    """icn_point_to_mesh_sign on contiguous fp32 ROCm points and vertices, int32 faces, tables and (face, kind) -> sign (B, P) fp32."""
    B, P, _ = pts.shape
    V, F = vts.shape[1], f32.shape[0]
    adjacency, offsets, corners = tables
    sign = torch.empty(B, P, dtype=torch.float32, device=pts.device)
    _launch('icn_point_to_mesh_sign', _per_mesh(pts), _per_mesh(vts), f32, adjacency, offsets, corners, _per_mesh(face), _per_mesh(kind),
            _NB, P, V, F, _per_mesh(sign))
    return sign


class _SignedRootFn(torch.autograd.Function):
    """phi = sign sqrt(dist2), differentiable in dist2 alone: the upstream g becomes g sign / (2 sqrt(dist2)), and 0 where dist2 == 0
    (the subgradient on the surface, where the root has no derivative)."""

    @staticmethod
    def forward(ctx, dist2, sign):
        root = dist2.sqrt()
        ctx.save_for_backward(root, sign)
        return sign * root

    @staticmethod
    def backward(ctx, g):
        root, sign = ctx.saved_tensors
        return torch.where(root == 0, torch.zeros_like(g), g * sign / (2 * root)), None


def _signed_point_to_mesh_distance_unchecked(pointclouds, vertices, f32, tables, search='brute'):
    """signed_point_to_mesh_distance without its argument checks, for callers that validated once: f32 is an int32 (F, 3) tensor on
    the points' device, F >= 1, tables = signed_distance_tables(f32, V) there.  On the HIP path (ROCm fp32 points and vertices, unless
    ICN_NO_HIP_LOSS=1) no host synchronisation; ids out of range in f32, the tables or (face, kind) are safe on either path (+1 or
    skipped, as defined)."""
    dist2, face, kind = _point_to_mesh_unchecked(pointclouds, vertices, f32, search)
    with torch.no_grad():
        if _on_hip_path(vertices) and pointclouds.is_cuda and pointclouds.dtype == torch.float32:
            sign = _hip_point_to_mesh_sign(pointclouds.detach().contiguous(), vertices.detach().contiguous(), f32, tables,
                                           face.to(torch.int32), kind)
        else:
            sign = _torch_point_to_mesh_sign(pointclouds, vertices, f32, face, kind, tables).to(dist2.dtype)
    return _SignedRootFn.apply(dist2, sign), face, kind


def _check_signed_distance_arguments(who, pointclouds, vertices, faces, search, tables):
    """The argument checks of point_to_mesh_distance for `who`, F >= 1, and -- with the one read-back of the face ids -- that the
    mesh is closed and manifold -> (int32 faces on the points' device, the tables there)."""
    _check_search(search)
    if pointclouds.dim() != 3 or vertices.dim() != 3 or pointclouds.shape[-1] != 3 or vertices.shape[-1] != 3:
        raise ValueError('%s: expected (B, P, 3) points and (B, V, 3) vertices' % who)
    if pointclouds.shape[0] != vertices.shape[0] or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError('%s: batch sizes differ or faces is not (F, 3)' % who)
    if (pointclouds.shape[0] < 1 or pointclouds.shape[1] < 1 or vertices.shape[1] < 1 or faces.shape[0] < 1 or faces.is_floating_point()
            or faces.dtype == torch.bool or pointclouds.dtype != vertices.dtype or pointclouds.device != vertices.device):
        raise ValueError('%s: expected at least one mesh, point, vertex and face, integer faces, and points and vertices of one dtype '
                         'and device' % who)
    V, F = vertices.shape[1], faces.shape[0]
    if 3 * F > 0x7fffffff:
        raise ValueError('%s: %d faces: 3 F must fit an int32' % (who, F))
    dev = pointclouds.device
    f32 = faces.to(device=dev, dtype=torch.int32).contiguous()
    if tables is not None:
        if (not isinstance(tables, (tuple, list)) or len(tables) != 3 or any(not torch.is_tensor(x) or x.dtype != torch.int32 for x in tables)
                or tuple(tables[0].shape) != (F, 3) or tuple(tables[1].shape) != (V + 1,) or tuple(tables[2].shape) != (3 * F,)):
            raise ValueError('%s: tables must be signed_distance_tables(faces, %d): int32 tensors (%d, 3), (%d,) and (%d,)'
                             % (who, V, F, V + 1, 3 * F))
        tables = tuple(x.to(dev).contiguous() for x in tables)
    adjacency, report = _edge_twins(f32, V)
    lo, hi, n_open, a_open, b_open, n_again, a_again, b_again = report.tolist()           # the one read-back
    if lo < 0 or hi >= V:
        raise IndexError('%s: face indices span [%d, %d] but there are %d vertices' % (who, lo, hi, V))
    if n_again:
        raise ValueError('%s: the mesh is not manifold: the directed edge (%d, %d) belongs to more than one face (%d such edges); '
                         'the sign needs a closed, consistently wound manifold' % (who, a_again, b_again, n_again))
    if n_open:
        raise ValueError('%s: the mesh is not closed: no face holds the edge (%d, %d), opposite to (%d, %d) (%d such edges); the sign '
                         'needs a closed, consistently wound manifold' % (who, b_open, a_open, a_open, b_open, n_open))
    if tables is None:
        tables = (adjacency,) + vertex_face_table(f32, V)
    return f32, tables


def signed_point_to_mesh_distance(pointclouds, vertices, faces, search='brute', tables=None):
    """(phi (B, P), face (B, P), kind (B, P)): the SIGNED distance of every point to the closed triangle mesh vertices (B, V, 3), faces
    (F, 3) integer and shared by the batch -- negative inside, positive outside, |phi| = sqrt(dist2) of point_to_mesh_distance exactly,
    with its (face, kind).  The sign is that of (p - q) . N, q the closest point the forward found and N the ANGLE-WEIGHTED
    PSEUDONORMAL of the feature q lies on (Baerentzen & Aanaes 2005): for a closed mesh wound counter-clockwise seen from outside --
    every mesh of this package -- it is exact for every point, whichever feature is the closest, at O(valence) per point on top of
    the search (MI355X, I5 / batch 36, one point per vertex: k_p2m_sign 0.017 - 0.027 ms beside 0.023 ms for the angle-defect gather;
    with search='grid' the whole signed distance of points 0.01 from the surface takes 0.55 ms, profiles/signed_distance.txt).

    One definition for the HIP kernel (include/icn_sdf.h), the torch formulation and the tests.  All arithmetic from the inputs to the
    one comparison is float64, whatever the dtype.  A face has n = (v1 - v0) x (v2 - v0) with every product of the cross product rounded
    on its own, is RESOLVED iff |n|^2 != 0, and n^ = n / |n|.  For a point p with its face f and kind:
        d = p - q, q recomputed from (f, kind) as the backward of point_to_mesh_distance does: the vertex; the clamped projection on
            the edge's segment; the plane, d = n (ap . n / |n|^2)
        N = n                    kind 0
            n^_f + n^_g          kind 4 / 5 / 6, g = adjacency[f][kind - 4] the face across that edge (an unresolved face adds nothing;
                                 without a g the edge takes n^_f alone)
            sum theta n^         kind 1 / 2 / 3, over the resolved faces at vertex j = faces[f][kind - 1] in the order of j's slice of
                                 vertex_face_table, theta = atan2(|n|, a . b) the face's angle at j (the corner of angle_defect)
        sign = -1 iff d . N < 0, else +1;   phi = sign sqrt(dist2)
    A point on the surface, a feature all of whose faces are unresolved and a NaN point give sign +1 (phi = NaN for the last).  Without
    the angles -- the plain sum of the incident normals -- the sign is wrong near a vertex whose faces differ much in their angles
    (tests/test_signed_distance.py: the spike).  Topology goes by vertex id: two vertices at one position are two vertices.
    The sign means "inside" only for a CLOSED, consistently wound manifold whose closest feature was found correctly, so this function
    checks, with the read-back that checks the face ids, that every directed edge has its opposite and none occurs twice, and raises
    ValueError naming the first offending edge otherwise.  On a mesh that passes through itself (self_intersections) the sign is still
    the one defined above, the side of the nearest sheet: a point in a fold-over counts as outside where the nearest sheet shows it
    its front -- use it there as a local, not a global, statement.
    tables = signed_distance_tables(faces, V): pass them when the face list is reused, else they are built here.  ROCm fp32 tensors run
    the search on icn_point_to_mesh / icn_point_to_mesh_grid (`search`, as point_to_mesh_distance) and the sign on icn_point_to_mesh_sign,
    one thread per point; CPU tensors, other dtypes and ICN_NO_HIP_LOSS=1 take the sign from the torch formulation.
    Differentiable in the points and the vertices by composition: the sign is piecewise constant and carries no gradient, so the
    gradient of phi is that of dist2 (icn_point_to_mesh_bwd on the HIP path) under the upstream g sign / (2 sqrt(dist2)), taken as 0
    where dist2 == 0.  face and kind never carry one."""
    f32, tables = _check_signed_distance_arguments('signed_point_to_mesh_distance', pointclouds, vertices, faces, search, tables)
    return _signed_point_to_mesh_distance_unchecked(pointclouds, vertices, f32, tables, search)


def contains(points, vertices, faces, search='brute', tables=None):
    """bool (B, P): whether each point lies strictly inside its closed mesh, phi < 0 of signed_point_to_mesh_distance (arguments,
    checks and paths as there; a NaN point is not inside).  Never requires grad."""
    f32, tables = _check_signed_distance_arguments('contains', points, vertices, faces, search, tables)
    with torch.no_grad():
        return _signed_point_to_mesh_distance_unchecked(points, vertices, f32, tables, search)[0] < 0


def voxel_lattice(outvertices, refvertices, resolution):
    """(origin, spacing, counts) of the lattice volumetric_iou counts on, for two (V, 3) vertex tensors of one shape: [lo, hi] the joint
    bounding box of both meshes (one read-back), origin = lo as three Python floats, spacing h = largest extent / resolution,
    counts n_k = max(1, ceil(extent_k / h)), all evaluated in float64 on the host.  Cell (i, j, k) has its centre at
    origin + ((i, j, k) + 1/2) h.  ValueError for other shapes, resolution < 1 or a box that is not finite or has no extent."""
    who = 'volumetric_iou'
    if outvertices.dim() != 2 or refvertices.dim() != 2 or outvertices.shape != refvertices.shape or outvertices.shape[-1] != 3:
        raise ValueError('%s: expected two (V, 3) vertex tensors of one shape, got %s and %s'
                         % (who, tuple(outvertices.shape), tuple(refvertices.shape)))
    if int(resolution) < 1:
        raise ValueError('%s: resolution must be positive, got %r' % (who, resolution))
    both = torch.stack([outvertices, refvertices.to(device=outvertices.device, dtype=outvertices.dtype)]).detach()
    lo, hi = (x.double() for x in (both.amin((0, 1)), both.amax((0, 1))))
    box = torch.stack([lo, hi]).tolist()                                                  # one read-back
    extent = [box[1][k] - box[0][k] for k in range(3)]
    if not all(e == e and abs(e) != float('inf') for e in extent) or max(extent) <= 0:
        raise ValueError('%s: the meshes have no finite bounding box of positive extent' % who)
    import math
    h = max(extent) / int(resolution)
    return tuple(box[0]), h, tuple(max(1, math.ceil(e / h)) for e in extent)


# ---- solid voxelisation by ray parity --------------------------------------------------------------------------------------------------
_VOXEL_MAX_DEPTH, _VOXEL_MAX_SIDE = 512, 4096                                             # ICN_VOXEL_MAX_DEPTH / _SIDE of include/icn_voxel.h


def _torch_voxelize(vertices, faces, origin, spacing, counts, cells=1 << 20):
    """The definition of voxelize in torch: float64 on the vertices as stored, every product and sum an operation of its own, in the
    order of include/icn_voxel.h -> bool (B, n0, n1, n2).  Chunked over the faces so that one intermediate holds about `cells`
    (mesh, column, face) triples; ids are clamped before they index anything and non-finite values meet only masked arithmetic."""
    B, V = vertices.shape[0], vertices.shape[1]
    n0, n1, n2 = (int(n) for n in counts)
    (ox, oy, oz), h = (float(o) for o in origin), float(spacing)
    dev = vertices.device
    v, ids = vertices.detach().double(), faces.long()
    F, C = ids.shape[0], n1 * n2
    py = (oy + (torch.arange(n1, dtype=torch.float64, device=dev) + 0.5) * h)[:, None].expand(n1, n2).reshape(1, C, 1)
    pz = (oz + (torch.arange(n2, dtype=torch.float64, device=dev) + 0.5) * h)[None, :].expand(n1, n2).reshape(1, C, 1)
    flips = torch.zeros(B, C, n0 + 1, dtype=torch.int32, device=dev)                      # crossings by k0; slot n0 is behind the lattice
    step = max(1, cells // (B * C))
    for lo in range(0, F, step):
        f = ids[lo:lo + step]                                                             # (c, 3)
        tri = v[:, f.clamp(0, V - 1)]                                                     # (B, c, 3 corners, 3)
        ok = ((f >= 0) & (f < V)).all(-1)[None] & torch.isfinite(tri).all(-1).all(-1)     # (B, c)
        x, y, z = (tri[..., k][:, None] for k in range(3))                                # (B, 1, c, 3 corners)
        covered = (ok[:, None] & (y.amin(-1) <= py) & (py <= y.amax(-1)) & (z.amin(-1) <= pz) & (pz <= z.amax(-1)))      # (B, C, c): tested
        s, positive, negative = [], covered, covered
        for e in range(3):                                                                # the edge opposite vertex e: u -> w
            u, w = (e + 1) % 3, (e + 2) % 3
            as_given = f[:, u] < f[:, w]                                                  # (c,): else the ends are swapped
            ay, az = torch.where(as_given, y[..., u], y[..., w]), torch.where(as_given, z[..., u], z[..., w])
            by, bz = torch.where(as_given, y[..., w], y[..., u]), torch.where(as_given, z[..., w], z[..., u])
            dy, dz = by - ay, bz - az
            value = dy * (pz - az) - dz * (py - ay)                                       # (B, C, c)
            t = torch.sign(value)
            t = torch.where(t == 0, torch.sign(-dz), t)
            t = torch.where(t == 0, torch.sign(dy), t)
            s.append(torch.where(as_given, value, -value))
            t = torch.where(as_given, t, -t)
            positive, negative = positive & (t > 0), negative & (t < 0)
        covered = positive | negative
        depth = (s[0] * x[..., 0] + s[1] * x[..., 1] + s[2] * x[..., 2]) / (s[0] + s[1] + s[2])
        tau = (depth - ox) / h - 0.5
        covered = covered & torch.isfinite(tau)
        k0 = torch.where(covered, torch.ceil(tau).clamp(0, n0), torch.full_like(tau, n0)).long()
        flips.scatter_add_(2, k0, covered.to(torch.int32))
    inside = (flips[..., :n0].cumsum(2) & 1).bool()                                       # (B, C, n0)
    return inside.permute(0, 2, 1).reshape(B, n0, n1, n2)


def _hip_voxelize(vts, f32, origin, spacing, counts):
    """icn_mesh_voxelize on contiguous fp32 ROCm vertices and an int32 face table -> bool (B, n0, n1, n2)."""
    B, V, F = vts.shape[0], vts.shape[1], f32.shape[0]
    n0, n1, n2 = (int(n) for n in counts)
    occupancy = torch.empty(B, n0, n1, n2, dtype=torch.uint8, device=vts.device)
    _launch('icn_mesh_voxelize', _per_mesh(vts), f32, _NB, V, F, *(float(o) for o in origin), float(spacing), n0, n1, n2,
            _per_mesh(occupancy))
    return occupancy.view(torch.bool)                                                     # bytes 0 / 1, each written once


def _voxelize_unchecked(vertices, f32, origin, spacing, counts):
    """voxelize without its argument checks and without a host synchronisation, for callers that validated once: f32 is an int32
    (F, 3) tensor on the vertices' device, F >= 1; origin three floats, spacing a positive float, counts three positive ints -- on the
    HIP path within (512, 4096, 4096), else the entry refuses them.  A vertex id out of range or a non-finite vertex is safe on either
    path: that face is not tested.  A mesh that is not closed gives what the definition gives: whole columns wrong."""
    if _on_hip_path(vertices):
        return _hip_voxelize(vertices.detach().contiguous(), f32, origin, spacing, counts)
    return _torch_voxelize(vertices, f32, origin, spacing, counts)


def _odd_edges(f32, V):
    """report int64 (5,) of a face list, without a host synchronisation: (lowest id, highest id, the number of undirected edges that
    belong to an odd number of faces, the (a, b), a < b, of the first of them in the order of a V + b).  The three edges of every
    face are keyed by their sorted ends and the keys sorted; an edge from a vertex to itself has no extent and is left out."""
    f = f32.long()
    a, b = f.reshape(-1), torch.roll(f, -1, 1).reshape(-1)
    low, high = torch.minimum(a, b), torch.maximum(a, b)
    key = torch.where(low != high, low * V + high, torch.full_like(low, -1))              # -1: left out, sorted to the front
    ordered, _ = torch.sort(key)
    at = torch.arange(ordered.numel(), device=ordered.device)
    first = torch.ones_like(ordered, dtype=torch.bool)
    first[1:] = ordered[1:] != ordered[:-1]
    last = torch.ones_like(first)
    last[:-1] = first[1:]
    start = torch.where(first, at, torch.zeros_like(at)).cummax(0)[0]                      # where each element's run begins
    odd = last & ((at - start) % 2 == 0) & (ordered >= 0)                                 # the run's last element has an even rank
    where = ordered.index_select(0, odd.to(torch.int8).argmax().reshape(1))
    lo, hi = f.aminmax()
    return torch.cat([lo.reshape(1), hi.reshape(1), odd.sum().reshape(1), where // V, where % V])


def voxelize(vertices, faces, origin, spacing, counts):
    """bool (B, n0, n1, n2): for every cell of a lattice whether its centre lies inside the closed triangle mesh vertices (B, V, 3),
    faces (F, 3) integer and shared by the batch.  Cell (i, j, k) has its centre at origin + ((i, j, k) + 1/2) spacing; origin is
    three floats, spacing a positive float, counts = (n0, n1, n2) (voxel_lattice gives all three for a mesh pair).  kaolin's
    trianglemeshes_to_voxelgrids followed by a fill, as one exact operation.  Never requires grad.

    One definition for the HIP kernel (include/icn_voxel.h), the torch formulation and the tests.  Rays run along axis 0 and the mesh
    is projected onto (y, z); a column is (j, k) with p = (py, pz), py = origin[1] + (j + 0.5) h, pz likewise.  All arithmetic is
    float64 on the vertices as stored, every product and sum rounded on its own, in exactly the order written:
        a face is TESTED for a column iff its ids lie in [0, V), its nine coordinates are finite, and lo_y <= py <= hi_y and
            lo_z <= pz <= hi_z against the minimum / maximum of its vertices -- part of the definition, not a filter
        the value of a directed edge u -> w, on (a, b) = (u, w) if id_u < id_w, else (w, u):
            s = (b.y - a.y) (pz - a.z) - (b.z - a.z) (py - a.y);  t = sign(s), if 0 sign(-(b.z - a.z)), if still 0 sign(b.y - a.y)
            (the symbolic perturbation p + (eps, eps^2)), both negated if the ends were swapped: the two faces of an edge evaluate one
            expression and get opposite values
        the face COVERS the column iff t > 0 for its three edges or t < 0 for all three
        its crossing, from the raw values s0, s1, s2 of the edges opposite vertices 0, 1, 2:
            x = (s0 v0.x + s1 v1.x + s2 v2.x) / (s0 + s1 + s2),  tau = (x - origin[0]) / h - 0.5, dropped if not finite,
            k0 = clamp(ceil(tau), 0, n0)
        cell i of the column is occupied iff the number of crossings with k0 <= i is odd.
    So a centre exactly on the surface counts the low side as inside ([0, 1) on every axis), the winding of the faces plays no part
    (where contains needs a consistently wound mesh), a mesh that passes through itself gets the XOR fill, and a face with
    coincident vertices, a non-finite vertex or (in the unchecked form) an id out of range contributes nothing.  On a mesh that is NOT
    CLOSED a column through the hole is wrong for its whole length, so this function checks, with the read-back that checks the face
    ids, that every undirected edge belongs to an even number of faces and raises ValueError naming the first that does not.
    ROCm fp32 tensors run on icn_mesh_voxelize: one thread per (mesh, column) in 16 x 16 tiles of columns, the faces staged through
    LDS and culled against the tile's box while they are staged, n0 <= 512 parity bits per column, n1, n2 <= 4096; no atomics,
    bit-identical run to run and equal to the float64 formulation byte for byte.  ICN_NO_HIP_LOSS=1, CPU tensors and other dtypes
    take that formulation in torch (_torch_voxelize), chunked over the faces.
    Shapes, the lattice and the closedness are checked (ValueError); face ids against V in the same read-back (IndexError)."""
    who = 'voxelize'
    if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1 or not vertices.is_floating_point():
        raise ValueError('%s: expected floating-point vertices (B, V, 3), got %s' % (who, tuple(vertices.shape)))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError('%s: expected integer faces (F, 3) with F >= 1, got %s' % (who, tuple(faces.shape)))
    V, F = vertices.shape[1], faces.shape[0]
    if 3 * F > 0x7fffffff:
        raise ValueError('%s: %d faces: 3 F must fit an int32' % (who, F))
    try:
        origin, spacing = tuple(float(o) for o in origin), float(spacing)
        if any(int(n) != n for n in counts):
            raise ValueError
        counts = tuple(int(n) for n in counts)
    except (TypeError, ValueError):
        raise ValueError('%s: origin must be three numbers, spacing a number and counts three integers' % who)
    finite = all(x == x and abs(x) != float('inf') for x in origin + (spacing,))
    if len(origin) != 3 or len(counts) != 3 or not finite or not spacing > 0 or min(counts) < 1:
        raise ValueError('%s: expected a finite origin of three numbers, a finite spacing > 0 and three counts >= 1, got %r, %r, %r'
                         % (who, origin, spacing, counts))
    if _on_hip_path(vertices) and (counts[0] > _VOXEL_MAX_DEPTH or max(counts[1:]) > _VOXEL_MAX_SIDE):
        raise ValueError('%s: counts %r: the HIP path takes at most (%d, %d, %d)'
                         % (who, counts, _VOXEL_MAX_DEPTH, _VOXEL_MAX_SIDE, _VOXEL_MAX_SIDE))
    f32 = faces.to(device=vertices.device, dtype=torch.int32).contiguous()
    lo, hi, n_odd, a, b = _odd_edges(f32, V).tolist()                                     # the one read-back
    if lo < 0 or hi >= V:
        raise IndexError('%s: faces index [%d, %d] but there are %d vertices' % (who, lo, hi, V))
    if n_odd:
        raise ValueError('%s: the mesh is not closed: the edge (%d, %d) belongs to an odd number of faces (%d such edges); a ray '
                         'through the hole would be wrong for its whole length' % (who, a, b, n_odd))
    with torch.no_grad():
        return _voxelize_unchecked(vertices, f32, origin, spacing, counts)


_IOU_METHODS = ('search', 'voxel')


def volumetric_iou(outvertices, refvertices, faces, resolution=32, search='brute', method='search'):
    """|A and B| / |A or B| of the solids two closed meshes enclose ((V, 3) tensors sharing `faces`), counted on a lattice, as a Python
    float: the standard volumetric figure of a reconstruction, to stand beside volume_error, curvature_error, self_intersection_ratio
    and compute_distance.  0 when no lattice point lies in either.
    The lattice is voxel_lattice(outvertices, refvertices, resolution): [lo, hi] the joint bounding box of both meshes (one
    read-back), h = largest extent / resolution, n_k = max(1, ceil(extent_k / h)) evaluated in float64 on the host, cell centres
    lo_k + (i + 1/2) h.  A cell is misclassified only if its centre is within h sqrt(3) / 2 of the surface, so each volume is off by
    at most sqrt(3) area h.
    method='search' (the default): both meshes go through `contains` as one batch of two; the counts are taken on the device.  That is
    n_0 n_1 n_2 points per mesh, up to resolution^3, each through the closest-triangle search -- and the lattice points deep inside or
    far outside are exactly the regime where search='grid' gives up its walk and scans all triangles (module docstring), so 'brute'
    is the default `search`: on an MI355X one I5 pair (20 480 faces) takes 11 ms at resolution 32 and 21 ms at 64 with 'brute', 20
    and 23 ms with 'grid' (profiles/signed_distance.txt from tools/time_signed_distance.py).  The sign needs a consistently wound
    mesh.
    method='voxel': both meshes go through `voxelize` on that lattice as one batch of two, the counts are taken on the device with
    one read-back; `search` plays no part.  One ray per lattice column instead of one search per cell, right for any closed mesh
    whatever its winding, and resolution up to 512 on the HIP path.  On an MI355X the same I5 pair takes 1.4 ms at resolution 32 and
    1.2 ms at 64, 7.5 and 17.6 times faster than 'search' with 'brute' in the same process and the same IoU to every printed digit,
    and 0.94 / 0.88 ms at 128 / 256 -- host time throughout: the kernel fills 128^3 cells for a batch of 36 in 1.10 ms, beside 8.55 ms
    for k_mesh_self_intersect on the same meshes, and 7.61 ms without its tile culling (profiles/voxelize.txt from
    tools/time_voxelize.py).  The default stays 'search'."""
    who = 'volumetric_iou'
    if method not in _IOU_METHODS:
        raise ValueError('%s: method must be one of %s, got %r' % (who, _IOU_METHODS, method))
    _check_search(search)
    origin, h, counts = voxel_lattice(outvertices, refvertices, resolution)
    both = torch.stack([outvertices, refvertices.to(device=outvertices.device, dtype=outvertices.dtype)]).detach()
    if method == 'voxel':
        inside = voxelize(both, faces, origin, h, counts).reshape(2, -1)
    else:
        axes = [origin[k] + (torch.arange(counts[k], dtype=torch.float64, device=both.device) + 0.5) * h for k in range(3)]
        centres = torch.stack(torch.meshgrid(*axes, indexing='ij'), -1).reshape(1, -1, 3).to(both.dtype)
        inside = contains(centres.expand(2, -1, -1).contiguous(), both, faces, search=search)
    n_and, n_or = torch.stack([(inside[0] & inside[1]).sum(), (inside[0] | inside[1]).sum()]).tolist()
    return n_and / n_or if n_or else 0.0


# ---- ray casting ------------------------------------------------------------------------------------------------------------------------
_RAY_CAST_CHUNK = 1 << 18          # (mesh, ray, face) triples the torch formulation holds at once: about 2 MiB per temporary


def _ray_edge(swapped, pu, pw, d):
    """(s, tau) of the directed edge u -> w of include/icn_raycast.h: pu, pw (..., 3) the ends less the origin, d (..., 3) the
    direction, `swapped` where id_u < id_w does not hold.  Every product and sum is a torch operation of its own."""
    a, b = torch.where(swapped[..., None], pw, pu), torch.where(swapped[..., None], pu, pw)
    ax, ay, az = a.unbind(-1)
    bx, by, bz = b.unbind(-1)
    nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
    s = (d[..., 0] * nx + d[..., 1] * ny) + d[..., 2] * nz
    tau = torch.sign(s)
    for n in (nx, ny, nz):
        tau = torch.where(tau == 0, torch.sign(n), tau)
    return torch.where(swapped, -s, s), torch.where(swapped, -tau, tau)


def _ray_parameter(ids, tri, o, d):
    """(t, covers) of rays against faces by the definition: ids (..., 3) integer, tri (..., 3 corners, 3) float64, o and d (..., 3)
    float64, all broadcastable."""
    p = tri - o[..., None, :]
    s, positive, negative = [], True, True
    for e in range(3):                                                                    # the edge opposite vertex e: u -> w
        u, w = (e + 1) % 3, (e + 2) % 3
        value, tau = _ray_edge(~(ids[..., u] < ids[..., w]), p[..., u, :], p[..., w, :], d)
        s.append(value)
        positive, negative = (tau > 0) & positive, (tau < 0) & negative
    c = [(p[..., k, 0] * d[..., 0] + p[..., k, 1] * d[..., 1]) + p[..., k, 2] * d[..., 2] for k in range(3)]
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return ((s[0] * c[0] + s[1] * c[1]) + s[2] * c[2]) / (((s[0] + s[1]) + s[2]) * dd), positive | negative


def _torch_ray_cast(origins, directions, vertices, faces, chunk=_RAY_CAST_CHUNK):
    """The definition of ray_cast in torch: float64 on the values as stored, every product and sum an operation of its own, in the
    order of include/icn_raycast.h -> (depth (B, R) in the vertices' dtype, face int64, count int32).  Chunked over the faces so that
    one intermediate holds about `chunk` (mesh, ray, face) triples; ids are clamped before they index anything and non-finite values
    meet only masked arithmetic.  Differentiable in vertices, origins and directions by evaluating t once more on the chosen face."""
    B, V = vertices.shape[0], vertices.shape[1]
    R, dev = origins.shape[1], vertices.device
    ids_all = faces.long()
    F = ids_all.shape[0]
    with torch.no_grad():
        v, o, d = vertices.detach().double(), origins.detach().double(), directions.detach().double()
        live = torch.isfinite(o).all(-1) & torch.isfinite(d).all(-1) & (d != 0).any(-1)                                  # (B, R)
        o, d = (torch.where(live[..., None], x, torch.zeros_like(x))[:, :, None] for x in (o, d))                        # (B, R, 1, 3)
        best = torch.full((B, R), float('inf'), dtype=torch.float64, device=dev)
        face = torch.full((B, R), -1, dtype=torch.int64, device=dev)
        count = torch.zeros(B, R, dtype=torch.int32, device=dev)
        step = max(1, chunk // (B * R))
        for lo in range(0, F, step):
            ids = ids_all[lo:lo + step]                                                                                   # (c, 3)
            tri = v[:, ids.clamp(0, V - 1)]                                                                               # (B, c, 3, 3)
            tested = ((ids >= 0) & (ids < V)).all(-1)[None] & torch.isfinite(tri).all(-1).all(-1)                         # (B, c)
            tri = torch.where(tested[..., None, None], tri, torch.zeros_like(tri))
            t, covers = _ray_parameter(ids, tri[:, None], o, d)                                                           # (B, R, c)
            hit = covers & tested[:, None] & live[..., None] & torch.isfinite(t) & (t > 0)
            count += hit.sum(-1, dtype=torch.int32)
            t = torch.where(hit, t, torch.full_like(t, float('inf')))
            nearest = t.amin(-1)                                                                                          # (B, R)
            index = torch.arange(lo, lo + ids.shape[0], device=dev).expand_as(t)
            first = torch.where(hit & (t == nearest[..., None]), index, torch.full_like(index, F)).amin(-1)              # the lowest index
            take = (first < F) & (nearest < best)                                                                         # earlier chunks win ties
            best, face = torch.where(take, nearest, best), torch.where(take, first, face)
    found = face >= 0
    if not (torch.is_grad_enabled() and (vertices.requires_grad or origins.requires_grad or directions.requires_grad)):
        return torch.where(found, best, torch.full_like(best, float('inf'))).to(vertices.dtype), face, count
    # once more on the chosen face, with autograd: the same operations on the same values, so the same t; rays without a hit run on
    # harmless constants and are masked out on either side, so that neither they nor their gradients can be NaN
    ids = ids_all[face.clamp(0)]                                                                                          # (B, R, 3)
    tri = torch.gather(vertices.double(), 1, ids.reshape(B, R * 3, 1).expand(-1, -1, 3)).reshape(B, R, 3, 3)
    tri = torch.where(found[..., None, None], tri, torch.eye(3, dtype=torch.float64, device=dev))
    o = torch.where(found[..., None], origins.double(), torch.zeros(3, dtype=torch.float64, device=dev))
    d = torch.where(found[..., None], directions.double(), torch.ones(3, dtype=torch.float64, device=dev))
    t, _ = _ray_parameter(ids, tri, o, d)
    return torch.where(found, t, torch.full_like(t, float('inf'))).to(vertices.dtype), face, count


def _hip_ray_cast(org, dirs, vts, f32):
    """icn_mesh_raycast on contiguous fp32 ROCm tensors and an int32 face table -> (depth fp32, face int32, count int32)."""
    B, R = org.shape[0], org.shape[1]
    V, F = vts.shape[1], f32.shape[0]
    depth = torch.empty(B, R, dtype=torch.float32, device=vts.device)
    face = torch.empty(B, R, dtype=torch.int32, device=vts.device)
    count = torch.empty(B, R, dtype=torch.int32, device=vts.device)
    _launch('icn_mesh_raycast', _per_mesh(org), _per_mesh(dirs), _per_mesh(vts), f32, _NB, R, V, F, _per_mesh(depth), _per_mesh(face),
            _per_mesh(count))
    return depth, face, count


class _RayCastFn(torch.autograd.Function):
    """ray_cast on the HIP path with a gradient (icn_mesh_raycast / icn_mesh_raycast_bwd in include/icn_raycast.h): the gradient of the
    depth at the forward's face choice, G = ddepth n / (n . d), w_k G to the face's vertices, -G to the origin, -t G to the direction;
    the vertex gradient is summed in a fixed order (bit-identical run to run).  Only the gradients autograd asks for are computed."""

    @staticmethod
    def forward(ctx, origins, directions, vertices, f32):
        org, dirs, vts = origins.contiguous(), directions.contiguous(), vertices.contiguous()
        depth, face, count = _hip_ray_cast(org, dirs, vts, f32)
        ctx.save_for_backward(org, dirs, vts, f32, face)
        face64 = face.long()
        ctx.mark_non_differentiable(face64, count)
        return depth, face64, count

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ddepth, _gface, _gcount):
        org, dirs, vts, f32, face = ctx.saved_tensors
        R, V, F = org.shape[1], vts.shape[1], f32.shape[0]
        dorg = torch.empty_like(org) if ctx.needs_input_grad[0] else None
        ddir = torch.empty_like(dirs) if ctx.needs_input_grad[1] else None
        dvts = torch.empty_like(vts) if ctx.needs_input_grad[2] else None
        args = (_per_mesh(org), _per_mesh(dirs), _per_mesh(vts), f32, _per_mesh(face), _per_mesh(_upstream(ddepth)), _NB, R, V, F,
                _per_mesh(dorg), _per_mesh(ddir), _per_mesh(dvts))
        if dvts is not None:                                                              # only the vertex gradient needs scratch
            _launch('icn_mesh_raycast_bwd', *args, workspace=('icn_mesh_raycast_bwd_workspace_bytes', R, V))
        else:
            _launch('icn_mesh_raycast_bwd', *args, None, 0)
        return dorg, ddir, dvts, None


def _ray_cast_unchecked(origins, directions, vertices, f32):
    """ray_cast without its argument checks and without a host synchronisation, for callers that validated once: origins and
    directions (B, R, 3) of the vertices' dtype and device, f32 an int32 (F, 3) tensor there, F >= 1.  A vertex id out of range or a
    non-finite vertex is safe on either path: that face is not tested."""
    if _on_hip_path(vertices) and origins.dtype == torch.float32 and directions.dtype == torch.float32:
        if torch.is_grad_enabled() and (origins.requires_grad or directions.requires_grad or vertices.requires_grad):
            return _RayCastFn.apply(origins, directions, vertices, f32)
        depth, face, count = _hip_ray_cast(origins.detach().contiguous(), directions.detach().contiguous(), vertices.detach().contiguous(), f32)
        return depth, face.long(), count
    return _torch_ray_cast(origins, directions, vertices, f32)


def _check_ray_mesh(who, vertices, faces):
    """The shape checks of a mesh batch for ray_cast and its callers -> the int32 face table on the vertices' device.  ValueError."""
    if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1 or not vertices.is_floating_point():
        raise ValueError('%s: expected floating-point vertices (B, V, 3), got %s' % (who, tuple(vertices.shape)))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1 or faces.is_floating_point() or faces.dtype == torch.bool:
        raise ValueError('%s: expected integer faces (F, 3) with F >= 1, got %s' % (who, tuple(faces.shape)))
    if 3 * faces.shape[0] > 0x7fffffff:
        raise ValueError('%s: %d faces: 3 F must fit an int32' % (who, faces.shape[0]))
    return faces.to(device=vertices.device, dtype=torch.int32).contiguous()


def _check_face_ids(who, f32, V):
    """IndexError unless the ids of the face table lie in [0, V): one read-back."""
    lo, hi = torch.stack(f32.aminmax()).tolist()
    if lo < 0 or hi >= V:
        raise IndexError('%s: faces index [%d, %d] but there are %d vertices' % (who, lo, hi, V))


def _check_ray_arguments(who, rays, vertices, faces, names):
    """The shape checks of ray_cast and its callers -> the rays as (B, R, 3) tensors of the vertices' dtype and device (rays (R, 3)
    are shared by the batch), the int32 face table and V.  ValueError."""
    f32, B = _check_ray_mesh(who, vertices, faces), vertices.shape[0]
    out = []
    for name, x in zip(names, rays):
        if not torch.is_tensor(x) or not x.is_floating_point() or x.dim() not in (2, 3) or x.shape[-1] != 3 or x.shape[-2] < 1 or \
                (x.dim() == 3 and x.shape[0] != B):
            raise ValueError('%s: expected floating-point %s (R, 3) or (%d, R, 3) with R >= 1, got %s'
                             % (who, name, B, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        x = x.to(device=vertices.device, dtype=vertices.dtype)
        out.append(x if x.dim() == 3 else x[None].expand(B, -1, -1))
    if len({x.shape[1] for x in out}) != 1:
        raise ValueError('%s: %s differ in their ray counts: %s' % (who, ' and '.join(names), [tuple(x.shape) for x in out]))
    if 3 * out[0].shape[1] > 0x7fffffff:
        raise ValueError('%s: %d rays: 3 R must fit an int32' % (who, out[0].shape[1]))
    return out, f32, vertices.shape[1]


def ray_cast(origins, directions, vertices, faces):
    """(depth (B, R), face (B, R) int64, count (B, R) int32): where each ray origins + t directions, t > 0, first meets the triangle
    mesh vertices (B, V, 3), faces (F, 3) integer and shared by the batch, which face that is (-1: none) and how many faces the ray
    crosses.  origins and directions are (B, R, 3), or (R, 3) shared by the batch; a direction need not be a unit vector and depth
    is in units of its length, +inf for a miss.  The query under depth maps and silhouettes (depth_map, silhouette_iou), visibility
    tests and an inside test from any direction (contains_by_parity).  depth is differentiable in vertices, origins and directions
    at the face it chose; face and count never carry a gradient.

    One definition for the HIP kernel (include/icn_raycast.h), the torch formulation and the tests.  All arithmetic is float64 on the
    values as stored, every product and sum rounded on its own, in exactly the order written:
        a ray is LIVE iff its six values are finite and d != (0, 0, 0); a ray that is not answers a miss (+inf, -1, 0)
        a face is TESTED iff its ids lie in [0, V) and its nine coordinates are finite; p_k = v_k - o
        the value of a directed edge u -> w, on (a, b) = (p_u, p_w) if id_u < id_w, else (p_w, p_u):
            N = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x);  s = (d.x N.x + d.y N.y) + d.z N.z;
            tau = sign(s), if 0 sign(N.x), if still 0 sign(N.y), if still 0 sign(N.z) (the symbolic perturbation
            d + (eps, eps^2, eps^3)), both negated if the ends were swapped: the two faces of an edge evaluate one expression and get
            opposite values; a face with a repeated id gets tau = 0 on that edge
        the face COVERS the ray iff tau > 0 for its three edges or tau < 0 for all three
        its parameter, from the raw values s0, s1, s2 of the edges opposite vertices 0, 1, 2:
            c_k = (p_k.x d.x + p_k.y d.y) + p_k.z d.z,  S = (s0 + s1) + s2,  dd = (d.x d.x + d.y d.y) + d.z d.z,
            t = ((s0 c0 + s1 c1) + s2 c2) / (S dd)
        a HIT is a covering face whose t is finite and > 0
        count = the number of hits; face = the hit of smallest t, the lowest face index among equal t; depth = that t rounded once to
        the vertices' dtype.  A t beyond that dtype rounds to +inf while face >= 0: the face is what tells a hit.
    So on a closed mesh the parity of count is the inside test of the origin whatever the winding of the faces (where contains needs a
    consistently wound mesh), a mesh that passes through itself gets the XOR, an origin exactly on the surface does not count that
    surface, and a face with coincident vertices, a non-finite vertex or (in the unchecked form) an id out of range is never hit.  A
    NaN never comes out.
    The gradient, at the chosen face: with n = (v1 - v0) x (v2 - v0), G = ddepth n / (n . d), d/dv_k = (s_k / S) G, d/do = -G,
    d/dd = -t G; nothing where there is no hit.
    ROCm fp32 tensors run on icn_mesh_raycast: one thread per (mesh, ray), the faces staged through LDS, an fp32 filter that skips a
    face only where it is proved not to cover the ray (csrc/icn_raycast.hip) in front of the double arithmetic, no atomics,
    bit-identical run to run and equal to the float64 formulation bit for bit; the backward is
    icn_mesh_raycast_bwd, one record per ray and a vertex scatter in a fixed order.  ICN_NO_HIP_LOSS=1, CPU tensors and other dtypes
    take the definition in torch (_torch_ray_cast), chunked over the faces, with autograd.
    Shapes are checked (ValueError) and the face ids against V with one read-back (IndexError)."""
    who = 'ray_cast'
    (origins, directions), f32, V = _check_ray_arguments(who, (origins, directions), vertices, faces, ('origins', 'directions'))
    _check_face_ids(who, f32, V)                                                          # the one read-back
    return _ray_cast_unchecked(origins, directions, vertices, f32)


def contains_by_parity(points, vertices, faces, direction=(1.0, 0.0, 0.0)):
    """bool (B, P): whether each point of points (B, P, 3) or (P, 3) lies inside its closed mesh, by the parity of ray_cast's count
    along `direction` (three numbers, not all zero; one ray per point).  Right whatever the winding of the faces, where `contains`
    needs a consistent one, and needs no table; a point exactly on the surface does not count that surface, and a NaN point is not
    inside.  On a mesh that is NOT CLOSED a ray through the hole is wrong, so this function checks, with the read-back that checks the
    face ids, that every undirected edge belongs to an even number of faces (ValueError, as voxelize).  Never requires grad."""
    who = 'contains_by_parity'
    try:
        direction = tuple(float(x) for x in direction)
    except (TypeError, ValueError):
        raise ValueError('%s: direction must be three numbers' % who)
    if len(direction) != 3 or not all(x == x and abs(x) != float('inf') for x in direction) or not any(direction):
        raise ValueError('%s: direction must be three finite numbers, not all zero, got %r' % (who, direction))
    (points,), f32, V = _check_ray_arguments(who, (points,), vertices, faces, ('points',))
    lo, hi, n_odd, a, b = _odd_edges(f32, V).tolist()                                     # the one read-back
    if lo < 0 or hi >= V:
        raise IndexError('%s: faces index [%d, %d] but there are %d vertices' % (who, lo, hi, V))
    if n_odd:
        raise ValueError('%s: the mesh is not closed: the edge (%d, %d) belongs to an odd number of faces (%d such edges); a ray '
                         'through the hole would be wrong' % (who, a, b, n_odd))
    with torch.no_grad():
        d = torch.tensor(direction, dtype=torch.float64).to(device=points.device, dtype=points.dtype).expand_as(points)
        return (_ray_cast_unchecked(points.detach(), d, vertices, f32)[2] & 1).bool()


_AXES = ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def _view_basis(view, who='depth_map'):
    """(w, e1, e2) of an orthographic view as tuples of Python floats: w the unit view direction, e1 = normalize(w x a) with a the
    coordinate axis of w's smallest |component| (the first on ties), e2 = w x e1.  ValueError unless view is three finite numbers
    with a length."""
    import math
    try:
        w = tuple(float(x) for x in view)
    except (TypeError, ValueError):
        raise ValueError('%s: a view must be three numbers, got %r' % (who, view))
    length = math.sqrt(sum(x * x for x in w)) if len(w) == 3 else 0.0
    if len(w) != 3 or not (length > 0 and length != float('inf')):
        raise ValueError('%s: a view must be three finite numbers, not all zero, got %r' % (who, view))
    w = tuple(x / length for x in w)
    a = _AXES[min(range(3), key=lambda k: (abs(w[k]), k))]

    def cross(p, q):
        return (p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0])
    e1 = cross(w, a)
    length = math.sqrt(sum(x * x for x in e1))
    e1 = tuple(x / length for x in e1)
    return w, e1, cross(w, e1)


def _frame_of_box(who, lo, hi):
    """(centre, rho) of a bounding box given as two lists of three Python floats: its midpoint and its half-diagonal, in float64 on the
    host.  ValueError unless the box is finite and has an extent."""
    import math
    centre = tuple((lo[k] + hi[k]) / 2 for k in range(3))
    rho = math.sqrt(sum((hi[k] - lo[k]) ** 2 for k in range(3))) / 2
    if not all(c == c and abs(c) != float('inf') for c in centre + (rho,)) or rho <= 0:
        raise ValueError('%s: the meshes have no finite bounding box of positive extent' % who)
    return centre, rho


def _joint_frame(vertices, who='depth_map'):
    """(centre, rho) of a batch of meshes: the midpoint and the half-diagonal of their joint bounding box (one read-back)."""
    v = vertices.detach()
    lo, hi = torch.stack([v.amin((0, 1)).double(), v.amax((0, 1)).double()]).tolist()     # one read-back
    return _frame_of_box(who, lo, hi)


def _pixel_rays(view, resolution, frame, like):
    """(origins (H W, 3), direction (3,)) of depth_map's pixels as tensors of like's dtype and device: evaluated in float64 on the
    host's values, rounded once."""
    w, e1, e2 = _view_basis(view)
    (centre, rho), n = frame, int(resolution)
    h = 2 * rho / n
    at = (torch.arange(n, dtype=torch.float64) + 0.5) * h - rho                            # (i + 1/2) h - rho
    base = torch.tensor(centre, dtype=torch.float64) - 2 * rho * torch.tensor(w, dtype=torch.float64)
    origins = (base + at[:, None, None] * torch.tensor(e1, dtype=torch.float64)) + at[None, :, None] * torch.tensor(e2, dtype=torch.float64)
    return origins.reshape(n * n, 3).to(device=like.device, dtype=like.dtype), torch.tensor(w, dtype=torch.float64).to(device=like.device, dtype=like.dtype)


def _check_view_arguments(resolution, frame, who='depth_map'):
    try:
        whole = int(resolution) == resolution and int(resolution) >= 1
    except (TypeError, ValueError):
        whole = False
    if not whole:
        raise ValueError('%s: resolution must be a positive integer, got %r' % (who, resolution))
    if frame is not None:
        try:
            centre, rho = frame
            frame = tuple(float(c) for c in centre), float(rho)
        except (TypeError, ValueError):
            raise ValueError('%s: frame must be (centre of three numbers, rho), got %r' % (who, frame))
        if len(frame[0]) != 3 or not all(c == c and abs(c) != float('inf') for c in frame[0] + (frame[1],)) or frame[1] <= 0:
            raise ValueError('%s: frame must be a finite centre of three numbers and a finite rho > 0, got %r' % (who, frame))
    return frame


def depth_map(vertices, faces, view, resolution, frame=None):
    """(depth (B, H, W), mask (B, H, W) bool), H = W = resolution: the orthographic depth image of every mesh of vertices (B, V, 3),
    faces (F, 3), seen along `view` (three numbers; w is its unit vector).  The image plane is spanned by e1 = normalize(w x a), a the
    coordinate axis of w's smallest |component| (the first on ties), and e2 = w x e1.  frame = (centre, rho) places it: a square of
    side 2 rho about centre; the default is the midpoint and the half-diagonal of the joint bounding box of the batch (one read-back),
    which holds every mesh from every view.  Pixel (i, j) casts the ray of direction w from
        centre + ((i + 1/2) h - rho) e1 + ((j + 1/2) h - rho) e2 - 2 rho w,    h = 2 rho / resolution
    -- evaluated in float64 on the host's values and rounded once to the vertices' dtype -- through ray_cast: depth is its depth (the
    distance from that plane, 2 rho in front of centre; +inf where nothing is hit), mask = face >= 0, the silhouette.  depth is
    differentiable in the vertices.  Checks as ray_cast, with its read-back."""
    frame = _check_view_arguments(resolution, frame)
    f32 = _check_ray_mesh('depth_map', vertices, faces)
    _check_face_ids('depth_map', f32, vertices.shape[1])
    return _depth_map_unchecked(vertices, f32, view, int(resolution), frame if frame is not None else _joint_frame(vertices))


def _depth_map_unchecked(vertices, f32, view, resolution, frame):
    """depth_map after its checks: no read-back of its own."""
    B = vertices.shape[0]
    origins, w = _pixel_rays(view, resolution, frame, vertices)
    depth, face, _ = _ray_cast_unchecked(origins[None].expand(B, -1, -1), w.expand(B, origins.shape[0], 3), vertices, f32)
    return depth.reshape(B, resolution, resolution), (face >= 0).reshape(B, resolution, resolution)


SILHOUETTE_VIEWS = _AXES + ((1.0, 1.0, 1.0), (1.0, 1.0, -1.0), (1.0, -1.0, 1.0), (1.0, -1.0, -1.0))


def silhouette_iou(outvertices, refvertices, faces, resolution=64, views=None):
    """The mean over `views` of |A and B| / |A or B| of the silhouettes of two meshes ((V, 3) tensors sharing `faces`), as a Python
    float: the standard image-space figure of a reconstruction, to stand beside volumetric_iou, and the one that can be compared with
    a photograph.  Each view is an orthographic depth_map of both meshes as one batch of two on a shared frame, the midpoint and
    half-diagonal of their joint bounding box (one read-back for the frame and the face ids); the masks are counted on the device and
    all counts come back in one read-back.  A view in which neither mesh is seen counts 0.  The default views are the three coordinate
    axes and the four body diagonals; the opposite directions would give the mirror images and the same figures.  The meshes need not
    be closed and their winding plays no part."""
    who = 'silhouette_iou'
    if outvertices.dim() != 2 or refvertices.dim() != 2 or outvertices.shape != refvertices.shape or outvertices.shape[-1] != 3:
        raise ValueError('%s: expected two (V, 3) vertex tensors of one shape, got %s and %s'
                         % (who, tuple(outvertices.shape), tuple(refvertices.shape)))
    _check_view_arguments(resolution, None, who)
    views = SILHOUETTE_VIEWS if views is None else tuple(views)
    if not views:
        raise ValueError('%s: no views' % who)
    for view in views:
        _view_basis(view, who)                                                            # raises on a bad view before any work
    both = torch.stack([outvertices, refvertices.to(device=outvertices.device, dtype=outvertices.dtype)]).detach()
    f32, V = _check_ray_mesh(who, both, faces), both.shape[1]
    box = torch.cat([torch.stack(f32.aminmax()).double(), both.amin((0, 1)).double(), both.amax((0, 1)).double()]).tolist()
    if box[0] < 0 or box[1] >= V:                                                         # (one read-back: the face ids and the box)
        raise IndexError('%s: faces index [%d, %d] but there are %d vertices' % (who, box[0], box[1], V))
    frame = _frame_of_box(who, box[2:5], box[5:8])
    counts = []
    with torch.no_grad():
        for view in views:
            _, mask = _depth_map_unchecked(both, f32, view, int(resolution), frame)
            counts += [(mask[0] & mask[1]).sum(), (mask[0] | mask[1]).sum()]
        counts = torch.stack(counts).tolist()                                             # one read-back
    return sum(a / o if o else 0.0 for a, o in zip(counts[::2], counts[1::2])) / len(views)


# ---- nearest neighbours between point sets: sided distance, chamfer, F-score, Hausdorff ------------------------------------------------
_SIDED_CHUNK = 1 << 22             # (cloud, query, target) triples the torch formulation holds at once: 16 MiB per fp32 temporary


def _torch_sided_distance_fwd(points, targets, chunk=_SIDED_CHUNK):
    """The forward of the definition of sided_distance in torch, in the dtype of `points`: every difference, product and sum a torch
    operation of its own, in the order of include/icn_nn.h -> (dist (B, N), idx (B, N) int64); no graph.  Chunked over the targets; the
    lowest index among equal distances is picked explicitly, inside a chunk and between chunks."""
    B, N, _ = points.shape
    M, dev = targets.shape[1], points.device
    with torch.no_grad():
        p, t = points.detach(), targets.detach()
        px, py, pz = p[:, :, None, 0], p[:, :, None, 1], p[:, :, None, 2]                                                # (B, N, 1)
        best = torch.full((B, N), float('inf'), dtype=p.dtype, device=dev)
        idx = torch.full((B, N), -1, dtype=torch.int64, device=dev)
        step = max(1, chunk // (B * N))
        for lo in range(0, M, step):
            q = t[:, None, lo:lo + step]                                                                                  # (B, 1, c, 3)
            dx, dy, dz = px - q[..., 0], py - q[..., 1], pz - q[..., 2]
            d = (dx * dx + dy * dy) + dz * dz                                                                             # (B, N, c)
            ok = d < float('inf')                                                          # what can ever be `< best`: no NaN, no +inf
            d = torch.where(ok, d, torch.full_like(d, float('inf')))
            nearest = d.amin(-1)
            index = torch.arange(lo, lo + q.shape[2], device=dev).expand_as(d)
            first = torch.where(ok & (d == nearest[..., None]), index, torch.full_like(index, M)).amin(-1)               # the lowest index
            take = (first < M) & (nearest < best)                                                                         # earlier chunks win ties
            best, idx = torch.where(take, nearest, best), torch.where(take, first, idx)
    return best, idx


def _torch_sided_distance_bwd(points, targets, idx, ddist, need_points=True, need_targets=True):
    """The backward of the definition in torch, in the dtype of `points`, at the fixed choice idx (B, N) integer under the upstream
    ddist (B, N): e = p - q_idx, s = 2 g, dpoints = s e, dtargets[idx] += -(s e); a row whose idx is outside [0, M) or whose e or g is
    not finite is an exact zero and contributes nothing -> (dpoints or None, dtargets or None)."""
    M = targets.shape[1]
    idx = idx.long()
    ok = (idx >= 0) & (idx < M)
    at = idx.clamp(0, M - 1)[..., None].expand(-1, -1, 3)
    e = points - torch.gather(targets, 1, at)
    s = 2 * ddist
    ok = ok & torch.isfinite(e).all(-1) & torch.isfinite(ddist)
    d = torch.where(ok[..., None], s[..., None] * e, torch.zeros_like(e))
    dtargets = torch.zeros_like(targets).scatter_add_(1, at, -d) if need_targets else None
    return (d if need_points else None), dtargets


class _TorchSidedDistanceFn(torch.autograd.Function):
    """The definition with its own backward (not autograd's of the forward's lines: the rows that contribute nothing are part of the
    definition), in any floating dtype on any device."""

    @staticmethod
    def forward(ctx, points, targets):
        dist, idx = _torch_sided_distance_fwd(points, targets)
        ctx.save_for_backward(points, targets, idx)
        ctx.mark_non_differentiable(idx)
        return dist, idx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ddist, _gidx):
        points, targets, idx = ctx.saved_tensors
        return _torch_sided_distance_bwd(points, targets, idx, ddist.to(points.dtype), *ctx.needs_input_grad)


def _torch_sided_distance(points, targets):
    """sided_distance by the definition in torch: fp32 in, the definition; float64 in, the same lines in double; differentiable in
    both point sets."""
    if torch.is_grad_enabled() and (points.requires_grad or targets.requires_grad):
        return _TorchSidedDistanceFn.apply(points, targets)
    return _torch_sided_distance_fwd(points, targets)


def _hip_sided_distance(pts, tgt):
    """icn_nearest_points on contiguous fp32 ROCm tensors -> (dist fp32, idx int32)."""
    B, N, M = pts.shape[0], pts.shape[1], tgt.shape[1]
    dist = torch.empty(B, N, dtype=torch.float32, device=pts.device)
    idx = torch.empty(B, N, dtype=torch.int32, device=pts.device)
    _launch('icn_nearest_points', _per_mesh(pts), _per_mesh(tgt), _NB, N, M, _per_mesh(dist), _per_mesh(idx))
    return dist, idx


class _SidedDistanceFn(torch.autograd.Function):
    """sided_distance on the HIP path with a gradient (icn_nearest_points / icn_nearest_points_bwd in include/icn_nn.h): at the
    forward's choice, 2 g (p - q) to the point and its negative to the chosen target, summed per target in a fixed order (bit-identical
    run to run).  Only the gradients autograd asks for are computed."""

    @staticmethod
    def forward(ctx, points, targets):
        pts, tgt = points.contiguous(), targets.contiguous()
        dist, idx = _hip_sided_distance(pts, tgt)
        ctx.save_for_backward(pts, tgt, idx)
        idx64 = idx.long()
        ctx.mark_non_differentiable(idx64)
        return dist, idx64

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, ddist, _gidx):
        pts, tgt, idx = ctx.saved_tensors
        N, M = pts.shape[1], tgt.shape[1]
        dpts = torch.empty_like(pts) if ctx.needs_input_grad[0] else None
        dtgt = torch.empty_like(tgt) if ctx.needs_input_grad[1] else None
        args = (_per_mesh(pts), _per_mesh(tgt), _per_mesh(idx), _per_mesh(_upstream(ddist)), _NB, N, M, _per_mesh(dpts), _per_mesh(dtgt))
        if dtgt is not None:                                                              # only the targets' gradient needs scratch
            _launch('icn_nearest_points_bwd', *args, workspace=('icn_nearest_points_bwd_workspace_bytes', N, M))
        else:
            _launch('icn_nearest_points_bwd', *args, None, 0)
        return dpts, dtgt


def _sided_distance_unchecked(p1, p2):
    """sided_distance without its argument checks and without a host synchronisation, for callers that validated once: p1 (B, N, 3)
    and p2 (B, M, 3) floating-point tensors of one dtype on one device, N, M >= 1."""
    if _on_hip_path(p1) and p2.dtype == torch.float32:
        if torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad):
            return _SidedDistanceFn.apply(p1, p2)
        dist, idx = _hip_sided_distance(p1.detach().contiguous(), p2.detach().contiguous())
        return dist, idx.long()
    return _torch_sided_distance(p1, p2)


def _check_point_sets(who, p1, p2):
    """The shape checks of two batched point sets -> (p1, p2 in p1's dtype and on its device).  ValueError."""
    for name, x in (('the first', p1), ('the second', p2)):
        if not torch.is_tensor(x) or not x.is_floating_point() or x.dim() != 3 or x.shape[-1] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError('%s: expected %s point set as a floating-point (B, N, 3) tensor with B, N >= 1, got %s'
                             % (who, name, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if 3 * x.shape[1] > 0x7fffffff:
            raise ValueError('%s: %d points: 3 N must fit an int32' % (who, x.shape[1]))
    if p1.shape[0] != p2.shape[0]:
        raise ValueError('%s: the batch sizes differ: %s and %s' % (who, tuple(p1.shape), tuple(p2.shape)))
    return p1, p2.to(device=p1.device, dtype=p1.dtype)


def sided_distance(p1, p2):
    """(dist (B, N), idx (B, N) int64): for every point of p1 (B, N, 3) the SQUARED distance to its nearest point in p2 (B, M, 3) and
    the index of that point (-1: none) -- kaolin.metrics.pointcloud.sided_distance, and the primitive under chamfer_distance, f_score
    and hausdorff_distance.  dist is differentiable in both point sets at the choice it made; idx carries no gradient.

    One definition for the HIP kernel (include/icn_nn.h), the torch formulation and the tests.  All arithmetic is in the dtype of p1
    (fp32 on the device) on the values as stored, every product and sum rounded on its own, in exactly the order written:
        dx = p.x - q_j.x;  dy = p.y - q_j.y;  dz = p.z - q_j.z;   d_j = (dx dx + dy dy) + dz dz
        best = +inf, idx = -1;  for j = 0 ... M - 1 ascending: if d_j < best then best = d_j, idx = j
    so among equal distances the lowest index wins, a NaN anywhere makes d_j NaN, which is never <, an infinite coordinate or an
    overflowing d_j gives +inf, which is not < +inf, and a point with no acceptable target answers (+inf, -1).  A NaN never comes out.
    Against float64 on the same values |d32 - d64| <= 6 2^-24 d64 while nothing underflows.
    The gradient, at the chosen index under the upstream g: e = p - q_idx, s = 2 g, s e to the point and -(s e) to target idx; a row
    with idx = -1, or with a non-finite e or g, is an exact zero and contributes nothing.
    ROCm fp32 tensors run on icn_nearest_points: the targets pass through LDS tiles in ascending order, every thread holds two
    queries in registers, no atomics, bit-identical run to run and equal to the fp32 formulation bit for bit; the backward is
    icn_nearest_points_bwd, one record per point and the vertex scatter in a fixed order.  ICN_NO_HIP_LOSS=1, CPU tensors and other
    dtypes take the definition in torch (_torch_sided_distance), chunked over the targets.  Shapes are checked (ValueError); nothing
    is read back."""
    return _sided_distance_unchecked(*_check_point_sets('sided_distance', p1, p2))


def _rooted(d):
    """sqrt of squared distances whose gradient at 0 is 0, not NaN."""
    positive = d > 0
    return torch.where(positive, torch.where(positive, d, torch.ones_like(d)).sqrt(), torch.zeros_like(d))


def _per_cloud_mean(d):
    """The mean over the points of every cloud, summed in double; still a double."""
    return d.double().mean(1)


def _chamfer_unchecked(p1, p2, w1=1.0, w2=1.0, squared=True):
    """chamfer_distance after its checks: no host synchronisation."""
    d12, d21 = _sided_distance_unchecked(p1, p2)[0], _sided_distance_unchecked(p2, p1)[0]
    if not squared:
        d12, d21 = _rooted(d12), _rooted(d21)
    return (w1 * _per_cloud_mean(d12) + w2 * _per_cloud_mean(d21)).to(p1.dtype)


def chamfer_distance(p1, p2, w1=1.0, w2=1.0, squared=True):
    """(B,): w1 mean_i sided(p1, p2)_i + w2 mean_j sided(p2, p1)_j of two batched point sets (B, N, 3) and (B, M, 3) --
    kaolin.metrics.pointcloud.chamfer_distance.  squared=False takes the root of each distance first (its gradient at a zero distance
    is 0, not NaN).  The means are summed in double and the result is rounded once to the dtype of p1.  Differentiable in both sets
    through sided_distance; nothing is read back."""
    p1, p2 = _check_point_sets('chamfer_distance', p1, p2)
    return _chamfer_unchecked(p1, p2, w1, w2, squared)


def f_score(gt_points, pred_points, radius=0.01, eps=1e-8):
    """(B,): the F-score of pred_points (B, N_pred, 3) against gt_points (B, N_gt, 3) at `radius` -- kaolin 0.9.1's
    kaolin.metrics.pointcloud.f_score:
        d_gt = sqrt(sided(pred, gt));  d_pred = sqrt(sided(gt, pred))
        fp = #(d_gt > radius);  fn = #(d_pred > radius);  tp = N_pred - fp
        precision = tp / (tp + fp);  recall = tp / (tp + fn);  F = 2 precision recall / (precision + recall + eps)
    The counts are exact integers; the ratios are taken in double and F is rounded once to the dtype of gt_points.  No gradient;
    nothing is read back."""
    gt, pred = _check_point_sets('f_score', gt_points, pred_points)
    with torch.no_grad():
        d_gt, d_pred = _sided_distance_unchecked(pred, gt)[0].sqrt(), _sided_distance_unchecked(gt, pred)[0].sqrt()
        fp, fn = (d_gt > radius).sum(1).double(), (d_pred > radius).sum(1).double()
        tp = pred.shape[1] - fp
        precision, recall = tp / (tp + fp), tp / (tp + fn)
        return (2 * precision * recall / (precision + recall + eps)).to(gt.dtype)


def hausdorff_distance(p1, p2):
    """(B,): the point-set Hausdorff distance of two batched point sets, the larger of the two directed maxima of the (unsquared)
    distances: max(max_i sqrt sided(p1, p2)_i, max_j sqrt sided(p2, p1)_j).  Differentiable through the one pair that attains it."""
    p1, p2 = _check_point_sets('hausdorff_distance', p1, p2)
    d12, d21 = _rooted(_sided_distance_unchecked(p1, p2)[0]), _rooted(_sided_distance_unchecked(p2, p1)[0])
    return torch.maximum(d12.amax(1), d21.amax(1))


# ---- every pair of clouds of two sets: the chamfer matrix, and the generation metrics on it -------------------------------------------
_MAX_CLOUDS = 65535                # clouds a set of the pairwise functions may hold: both set sizes are grid dimensions of k_pair_sums


def _check_cloud_sets(who, p1, p2):
    """The shape checks of two SETS of clouds, whose sizes are independent -> (p1, p2 in p1's dtype and on its device), detached.
    ValueError.  Shapes only: a zero-stride view of 65536 clouds is rejected without being materialised."""
    for name, x in (('the first', p1), ('the second', p2)):
        if not torch.is_tensor(x) or not x.is_floating_point() or x.dim() != 3 or x.shape[-1] != 3 or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError('%s: expected %s set as a floating-point (clouds, points, 3) tensor with clouds, points >= 1, got %s'
                             % (who, name, tuple(x.shape) if torch.is_tensor(x) else type(x).__name__))
        if x.shape[0] > _MAX_CLOUDS:
            raise ValueError('%s: %d clouds in %s set: at most %d' % (who, x.shape[0], name, _MAX_CLOUDS))
        if 3 * x.shape[1] > 0x7fffffff:
            raise ValueError('%s: %d points: 3 N must fit an int32' % (who, x.shape[1]))
    return p1.detach(), p2.detach().to(device=p1.device, dtype=p1.dtype)


def _torch_pairwise_sided_sums(p1, p2, chunk=_SIDED_CHUNK):
    """pairwise_sided_sums by the definition in torch, in the dtype of p1: cloud g against a few clouds of p2 at a time through
    _torch_sided_distance_fwd, the distances converted to double and summed per pair.  Never more than `chunk` (cloud, query, target)
    triples at once: the queries go in slices of at most `chunk`, as many clouds of p2 at a time as then fit, and the targets are
    chunked by _torch_sided_distance_fwd itself."""
    (G, N, _), (R, M, _) = p1.shape, p2.shape
    sums = torch.zeros(G, R, dtype=torch.float64, device=p1.device)
    queries = min(N, chunk)
    clouds = max(1, min(R, chunk // (queries * M)))                                        # 1: the targets are chunked instead
    for g in range(G):
        for lo in range(0, N, queries):
            q = p1[g:g + 1, lo:lo + queries]
            for r0 in range(0, R, clouds):
                t = p2[r0:r0 + clouds]
                dist, _ = _torch_sided_distance_fwd(q.expand(t.shape[0], -1, -1), t, chunk)
                sums[g, r0:r0 + clouds] += dist.double().sum(1)
    return sums


def _hip_pairwise_sided_sums(qry, tgt):
    """icn_sided_sums on contiguous fp32 ROCm tensors -> sums (G, R) float64."""
    (G, N, _), (R, M, _) = qry.shape, tgt.shape
    L = _lib.api()
    sums = torch.empty(G, R, dtype=torch.float64, device=qry.device)
    ws_bytes = L.icn_sided_sums_workspace_bytes(G, R, N, M)
    ws = _lib.workspace(ws_bytes, qry.device)
    with torch.cuda.device(qry.device):
        L.icn_sided_sums(qry.data_ptr(), tgt.data_ptr(), G, R, N, M, sums.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream())
    return sums


def _pairwise_sided_sums_unchecked(p1, p2):
    """pairwise_sided_sums after its checks: detached tensors of one dtype on one device; no host synchronisation."""
    if _on_hip_path(p1) and p2.dtype == torch.float32:
        return _hip_pairwise_sided_sums(p1.contiguous(), p2.contiguous())
    return _torch_pairwise_sided_sums(p1, p2)


def pairwise_sided_sums(p1, p2):
    """sums (G, R) float64 of two SETS of clouds p1 (G, N, 3) and p2 (R, M, 3): sums[g, r] = sum_i sided_distance(p1[g], p2[r])_i, the
    sum over the points of cloud g of the squared distance to the nearest point of cloud r, for EVERY pair -- where sided_distance pairs
    cloud b with cloud b.  G, R, N and M are independent; G, R <= 65535.  No gradient: the inputs are detached.

    Every distance is the `dist` of sided_distance, bit for bit (fp32 on the device, every product and sum rounded on its own, a NaN
    distance passed over, +inf where a point has no acceptable target); the distances of a pair are converted to double, which is
    exact, and summed in double in a fixed order.  Every term is >= 0, so no NaN comes out, and a single +inf distance makes the
    entry exactly +inf.  Against the same distances summed in another order, |difference| <= N 2^-53 sum on either side.
    ROCm fp32 tensors run on icn_sided_sums (include/icn_pairs.h): the kernel indexes the pair itself, keeps no index, reduces in the
    launch and writes one double a pair -- nothing of size G R N is ever held, where sided_distance on repeat_interleave / repeat copies
    reads G R (N + M) 12 bytes and writes G R N 8; two launches, no atomics, bit-identical run to run, and entry (g, r) does not depend
    on G, R or the position of the two clouds.  ICN_NO_HIP_LOSS=1, CPU tensors and other dtypes take _torch_pairwise_sided_sums, which
    never holds more than _SIDED_CHUNK (cloud, query, target) triples.  Shapes are checked (ValueError); nothing is read back."""
    return _pairwise_sided_sums_unchecked(*_check_cloud_sets('pairwise_sided_sums', p1, p2))


def pairwise_chamfer(p1, p2, w1=1.0, w2=1.0, squared=True):
    """(G, R) in the dtype of p1: the chamfer distance of EVERY pair of clouds of p1 (G, N, 3) and p2 (R, M, 3),
        d[g, r] = w1 pairwise_sided_sums(p1, p2)[g, r] / N + w2 pairwise_sided_sums(p2, p1)[r, g] / M,
    computed in double and rounded once: chamfer_distance(p1[g:g+1], p2[r:r+1]) for all g and r.  The distance matrix that
    minimum_matching_distance, coverage and one_nn_accuracy take.  No gradient.
    squared=False (the root of every distance before the mean) is NOT SUPPORTED on the fused path, because the root has to be taken
    per point before the sum: it is defined, and computed by chamfer_distance(squared=False) of cloud g against every cloud of p2, one
    g at a time -- G calls that each hold R copies of one cloud."""
    p1, p2 = _check_cloud_sets('pairwise_chamfer', p1, p2)
    if not squared:
        with torch.no_grad():
            return torch.stack([_chamfer_unchecked(p1[g:g + 1].expand(p2.shape[0], -1, -1), p2, w1, w2, False) for g in range(p1.shape[0])])
    d = w1 * _pairwise_sided_sums_unchecked(p1, p2) / p1.shape[1] + w2 * _pairwise_sided_sums_unchecked(p2, p1).t() / p2.shape[1]
    return d.to(p1.dtype)


def _check_distance_matrix(who, d, name='d', shape=None):
    if not torch.is_tensor(d) or not d.is_floating_point() or d.dim() != 2 or d.shape[0] < 1 or d.shape[1] < 1:
        raise ValueError('%s: expected %s as a floating-point (G, R) distance matrix with G, R >= 1, got %s'
                         % (who, name, tuple(d.shape) if torch.is_tensor(d) else type(d).__name__))
    if shape is not None and tuple(d.shape) != tuple(shape):
        raise ValueError('%s: expected %s of shape %s, got %s' % (who, name, tuple(shape), tuple(d.shape)))
    return d.detach()


def _lowest_argmin(d):
    """(minimum, index) along the last dimension of d over its acceptable entries -- those < +inf: no NaN, no +inf -- THE LOWEST INDEX
    AMONG EQUAL MINIMA, written out with the masked amin of _torch_sided_distance_fwd (argmin on the device promises no tie rule).
    A row without an acceptable entry answers (+inf, n), n its length."""
    n = d.shape[-1]
    ok = d < float('inf')
    d = torch.where(ok, d, torch.full_like(d, float('inf')))
    nearest = d.amin(-1)
    index = torch.arange(n, device=d.device).expand_as(d)
    return nearest, torch.where(ok & (d == nearest[..., None]), index, torch.full_like(index, n)).amin(-1)


def minimum_matching_distance(d):
    """MMD of a distance matrix d (G, R), generated shapes by reference shapes (Achlioptas et al. 2018): the mean over the reference
    shapes r of min_g d[g, r], how far the nearest generated shape is from each reference shape.  A 0-dim tensor in the dtype of d,
    the mean taken in double.  NaN and +inf entries are never a minimum; a reference shape without a finite distance contributes +inf."""
    d = _check_distance_matrix('minimum_matching_distance', d)
    return _lowest_argmin(d.t())[0].double().mean().to(d.dtype)


def coverage(d):
    """COV of a distance matrix d (G, R): #unique{argmin_r d[g, r] : g} / R, the share of the reference shapes that are the nearest
    reference shape of some generated shape.  Among equally near reference shapes the lowest index is the match; a generated shape
    without a finite distance matches none.  A 0-dim float64 tensor; nothing is read back."""
    d = _check_distance_matrix('coverage', d)
    R = d.shape[1]
    match = _lowest_argmin(d)[1]                                                           # R: no match
    hit = torch.zeros(R + 1, dtype=torch.bool, device=d.device)
    hit[match] = True
    return hit[:R].sum().double() / R


def one_nn_accuracy(d_gg, d_gr, d_rr):
    """1-NNA of the distance matrices generated x generated (G, G), generated x reference (G, R) and reference x reference (R, R): the
    accuracy of the leave-one-out 1-nearest-neighbour classifier on the merged set, generated shapes first, then reference shapes
    (Yang et al. 2019).  Every element looks for its nearest OTHER element (the diagonal is excluded; the lowest merged index among
    equally near ones) and is right when that neighbour carries its own label; an element without a finite distance to anyone
    counts as wrong.  0.5 is the ideal (the sets cannot be told apart), 1 the worst.  Row g of the merged matrix is
    (d_gg[g], d_gr[g]), row G + r is (d_gr[:, r], d_rr[r]).  A 0-dim float64 tensor; nothing is read back."""
    who = 'one_nn_accuracy'
    d_gr = _check_distance_matrix(who, d_gr, 'd_gr')
    G, R = d_gr.shape
    d_gg, d_rr = _check_distance_matrix(who, d_gg, 'd_gg', (G, G)), _check_distance_matrix(who, d_rr, 'd_rr', (R, R))
    d_gg, d_rr = d_gg.to(device=d_gr.device, dtype=d_gr.dtype), d_rr.to(device=d_gr.device, dtype=d_gr.dtype)
    merged = torch.cat([torch.cat([d_gg, d_gr], 1), torch.cat([d_gr.t(), d_rr], 1)], 0)
    own = torch.eye(G + R, dtype=torch.bool, device=merged.device)
    neighbour = _lowest_argmin(torch.where(own, torch.full_like(merged, float('inf')), merged))[1]      # G + R: none
    generated = torch.arange(G + R, device=merged.device) < G
    right = torch.where(generated, neighbour < G, (neighbour >= G) & (neighbour < G + R))
    return right.sum().double() / (G + R)


# ---- optimal matching of two clouds of one size: the earth mover's distance ------------------------------------------------------------
_MATCH_PHASES = 26                 # eps_k = D 4^-k stays a normal step of the prices up to here
_MATCH_PAIRS = 1024                # pairs one launch of k_match_auction takes: bounds the workspace and the length of a launch
_MATCH_MAX_N = 13312               # points a cloud may hold on the HIP path: prices and owners in LDS (include/icn_match.h)


def _rounded_root(d):
    """sqrt(d) CORRECTLY ROUNDED for fp32 d, whatever the device's sqrt does: torch's vectorised fp32 sqrt is one unit off on some CPUs
    (for d = 0x40450D2E an AVX-512 build answers 0x3FE0999D where IEEE, numpy and the GPU say 0x3FE0999C), and one unit in a cost moves the prices.
    The neighbour s' of s = d.sqrt() is the right answer iff d lies beyond the midpoint m of s and s'; m has 25 significant bits, so
    m m is exact in double and the comparison with d is exact (the root of an fp32 number is never a midpoint).  Other dtypes: d.sqrt()."""
    s = d.sqrt()
    if d.dtype != torch.float32:
        return s
    inf, d64 = torch.full_like(s, float('inf')), d.double()
    for _ in range(2):                                                                    # a sqrt up to two units off is put right
        up, down = torch.nextafter(s, inf), torch.nextafter(s, -inf)
        m_up, m_down = (s.double() + up.double()) / 2, (s.double() + down.double()) / 2
        moved = torch.where(d64 > m_up * m_up, up, torch.where(d64 < m_down * m_down, down, s))
        s = torch.where((d > 0) & (d < float('inf')), moved, s)
    return s


def _torch_optimal_matching(p, q, phases=6, max_rounds=None, bidders=None):
    """THE DEFINITION of optimal_matching for one pair of clouds p, q (N, 3), restated in torch -> (match int64 (N,), cost 0-dim
    double, rounds int, prices double (N,)): the synchronous epsilon-scaling auction of include/icn_match.h, every step in the order
    written there.  The cost matrix is held whole, N^2 doubles.  Max, the argmax with the lowest index (written out: torch's own
    promises no tie rule on every device) and the second maximum are order-free, so with the root of _rounded_root this fixes
    every bit of match, rounds and prices.  bidders: a list that receives the number of bidders of every round (for measurements)."""
    import math
    N, dev = p.shape[0], p.device
    max_rounds = 64 * N + 4096 if max_rounds is None else max_rounds
    both = torch.cat([p, q])
    ex, ey, ez = (both.amax(0).double() - both.amin(0).double()).tolist()
    D = math.sqrt((ex * ex + ey * ey) + ez * ez)
    if not math.isfinite(D) or not bool(torch.isfinite(both).all()):
        return (torch.full((N,), -1, dtype=torch.int64, device=dev), torch.tensor(float('nan'), dtype=torch.float64, device=dev), 0,
                torch.full((N,), float('nan'), dtype=torch.float64, device=dev))
    dx, dy, dz = (p[:, None, :] - q[None, :, :]).unbind(-1)
    c = _rounded_root((dx * dx + dy * dy) + dz * dz).double()                             # c_ij: rounded in the clouds' dtype
    price = torch.zeros(N, dtype=torch.float64, device=dev)
    everyone = torch.arange(N, device=dev)
    if D == 0 or N == 1:
        return everyone, (c[0, 0] if D != 0 else torch.zeros((), dtype=torch.float64, device=dev)), 0, price
    negc, rounds, capped = -c, 0, False
    p2o = torch.full((N,), -1, dtype=torch.int64, device=dev)
    for k in range(1, phases + 1):
        eps = D * 4.0 ** -k
        owner = torch.full((N,), -1, dtype=torch.int64, device=dev)
        p2o = torch.full((N,), -1, dtype=torch.int64, device=dev)
        while True:
            U = (p2o < 0).nonzero()[:, 0]
            if U.numel() == 0:
                break
            if rounds == max_rounds:
                capped = True
                break
            rounds += 1
            if bidders is not None:
                bidders.append(U.numel())
            v = negc[U] - price[None]
            v1 = v.amax(1)
            j1 = torch.where(v == v1[:, None], everyone[None], torch.full_like(everyone, N)[None]).amin(1)
            j1 = torch.where(j1 < N, j1, torch.zeros_like(j1))                            # values that are no number: object 0
            v2 = v.scatter(1, j1[:, None], float('-inf')).amax(1)
            bid = ((v1 - v2) + eps) + price[j1]
            # per object: the highest bid, the lowest person among equals; the previous owner becomes unassigned
            best = torch.full((N,), float('-inf'), dtype=torch.float64, device=dev).scatter_reduce(0, j1, bid, 'amax')
            top = bid == best[j1]
            winner = torch.full((N,), N, dtype=torch.int64, device=dev).scatter_reduce(0, j1[top], U[top], 'amin')
            objects = (winner < N).nonzero()[:, 0]
            previous = owner[objects]
            p2o[previous[previous >= 0]] = -1
            owner[objects] = winner[objects]
            p2o[winner[objects]] = objects
            price[objects] = best[objects]
        if capped:
            break
    if capped:
        return p2o, torch.tensor(float('nan'), dtype=torch.float64, device=dev), rounds, price
    return p2o, c[everyone, p2o].sum(), rounds, price


def _check_match_arguments(who, p1, p2, phases, max_rounds, paired):
    """The checks of the matching functions -> (p1, p2 detached, in p1's dtype and on its device, max_rounds).  ValueError."""
    p1, p2 = _check_cloud_sets(who, p1, p2)
    if p1.shape[1] != p2.shape[1]:
        raise ValueError('%s: the two clouds of a pair must have one size, got %d and %d points: unequal sizes are not supported'
                         % (who, p1.shape[1], p2.shape[1]))
    if paired and p1.shape[0] != p2.shape[0]:
        raise ValueError('%s: paired sets must hold equally many clouds, got %d and %d' % (who, p1.shape[0], p2.shape[0]))
    if isinstance(phases, bool) or not isinstance(phases, int) or not 1 <= phases <= _MATCH_PHASES:
        raise ValueError('%s: phases must be an integer in [1, %d], got %r' % (who, _MATCH_PHASES, phases))
    if max_rounds is None:
        max_rounds = 64 * p1.shape[1] + 4096
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, int) or not 1 <= max_rounds <= 0x7fffffff:
        raise ValueError('%s: max_rounds must be a positive integer that fits an int32, got %r' % (who, max_rounds))
    return p1, p2, max_rounds


def _optimal_matching_unchecked(p1, p2, phases, max_rounds, paired, want_match=True, want_prices=True):
    """optimal_matching after its checks -> (match int64 or None, cost, rounds, prices or None).  On the HIP path one call of
    icn_match_clouds per slice of at most _MATCH_PAIRS pairs: whole rows of g, or pieces of one row where R alone exceeds that; every
    slice of the outputs is contiguous and, entry (g, r) being the 1 x 1 call bit for bit, slicing changes nothing."""
    (G, N, _), R = p1.shape, p2.shape[0]
    shape = (G,) if paired else (G, R)
    dev = p1.device
    if _on_hip_path(p1) and p2.dtype == torch.float32:
        if N > _MATCH_MAX_N:
            raise ValueError('optimal_matching: %d points: at most %d on the HIP path' % (N, _MATCH_MAX_N))
        qry, tgt = p1.contiguous(), p2.contiguous()
        L = _lib.api()
        match = torch.empty(shape + (N,), dtype=torch.int32, device=dev) if want_match else None
        prices = torch.empty(shape + (N,), dtype=torch.float64, device=dev) if want_prices else None
        cost = torch.empty(shape, dtype=torch.float64, device=dev)
        rounds = torch.empty(shape, dtype=torch.int32, device=dev)
        if paired:
            slices = [(g0, min(_MATCH_PAIRS, G - g0), g0, min(_MATCH_PAIRS, G - g0)) for g0 in range(0, G, _MATCH_PAIRS)]
        elif R <= _MATCH_PAIRS:
            rows = _MATCH_PAIRS // R
            slices = [(g0, min(rows, G - g0), 0, R) for g0 in range(0, G, rows)]
        else:
            slices = [(g, 1, r0, min(_MATCH_PAIRS, R - r0)) for g in range(G) for r0 in range(0, R, _MATCH_PAIRS)]
        ws_bytes = max(L.icn_match_clouds_workspace_bytes(ng, nr, N, int(paired)) for _, ng, _, nr in slices)
        ws = _lib.workspace(ws_bytes, dev)

        def at(t, g0, r0):                                                                # the slice's first entry; None stays null
            return None if t is None else (t[g0:] if paired or not r0 else t[g0, r0:]).data_ptr()
        with torch.cuda.device(dev):
            for g0, ng, r0, nr in slices:
                L.icn_match_clouds(qry[g0:].data_ptr(), tgt[r0:].data_ptr(), ng, nr, N, int(paired), phases, max_rounds,
                                   at(match, g0, r0), at(prices, g0, r0), at(cost, g0, r0), at(rounds, g0, r0), ws.data_ptr(), ws_bytes,
                                   _lib.stream())
        return (match.long() if want_match else None), cost, rounds, prices
    pairs = [(b, b) for b in range(G)] if paired else [(g, r) for g in range(G) for r in range(R)]
    results = [_torch_optimal_matching(p1[g], p2[r], phases, max_rounds) for g, r in pairs]
    match = torch.stack([m for m, _, _, _ in results]).view(shape + (N,)) if want_match else None
    prices = torch.stack([x for _, _, _, x in results]).view(shape + (N,)) if want_prices else None
    cost = torch.stack([c.double() for _, c, _, _ in results]).view(shape)
    rounds = torch.tensor([n for _, _, n, _ in results], dtype=torch.int32, device=dev).view(shape)
    return match, cost, rounds, prices


def optimal_matching(p1, p2, phases=6, max_rounds=None, paired=True):
    """(match int64, cost float64, rounds int32, prices float64): the assignment of the points of one cloud to the points of another
    of THE SAME SIZE that minimises the sum of Euclidean distances, by a synchronous epsilon-scaling auction (Bertsekas's forward
    auction, every unassigned person bidding at once).  p1 (G, N, 3), p2 (R, N, 3).  paired=True (default) needs G == R and matches
    cloud b with cloud b: match and prices (G, N), cost and rounds (G,).  paired=False matches every pair: (G, R, N) and (G, R).
    Unequal sizes are not supported.  No gradient: the inputs are detached.

    One definition for the HIP kernel (include/icn_match.h, where it is written out), the torch restatement
    (_torch_optimal_matching) and the tests.  c_ij = sqrt(d_ij), d_ij the squared distance of sided_distance in the clouds' dtype;
    everything after it is double.  D is the diagonal of the joint bounding box, eps_k = D 4^-k for the phases k = 1 ... phases;
    prices start at 0 and carry over, every phase starts with everybody unassigned; in a round every unassigned person i bids
    ((v_ij1 - v2) + eps_k) + price_j1 for its best object j1 (v_ij = (-c_ij) - price_j; the lowest j among equals), and every object
    goes to its highest bid (the lowest person among equals) at that price.  match[i] is the object person i owns, cost the sum of
    c_{i, match[i]} in double, rounds the total number of rounds, prices the final prices.  The cost is within N D 4^-phases of the
    optimum -- the mean within D / 4096 at the default phases = 6 -- and (match, prices) prove it by epsilon-complementary slackness.
    Decided before any round: a non-finite coordinate gives (all -1, NaN, 0, NaN); D == 0 the identity at cost 0; N == 1 match [0].
    max_rounds (default 64 N + 4096, seven times the most any measured pair took) keeps a call finite and is no tuning knob: a pair that
    reaches it reports rounds == max_rounds, cost NaN and -1 for its unassigned persons.
    ROCm fp32 tensors run on icn_match_clouds: one workgroup of 1024 threads owns a pair from start to finish, prices and owners in
    LDS (hence N <= 13312 there), every wave scanning the objects for one bidder at a time, bids resolved by integer LDS atomics; match,
    rounds and prices equal the restatement on CPU tensors bit for bit, cost within N 2^-53 cost.  Sets of many pairs go in launches
    of at most 1024 pairs, which changes no bit.  ICN_NO_HIP_LOSS=1, CPU tensors and other dtypes take the restatement pair by
    pair, which holds N^2 doubles.  Shapes and arguments are checked (ValueError); nothing is read back."""
    p1, p2, max_rounds = _check_match_arguments('optimal_matching', p1, p2, phases, max_rounds, paired)
    return _optimal_matching_unchecked(p1, p2, phases, max_rounds, bool(paired))


def _raise_if_capped(who, cost, rounds, max_rounds):
    """One read-back: RuntimeError naming the first pair that stopped at the round cap (its cost is NaN and rounds == max_rounds)."""
    capped = (torch.isnan(cost) & (rounds == max_rounds)).reshape(-1)
    hit = capped.nonzero()[:1, 0].tolist()
    if hit:
        where = hit[0] if cost.dim() == 1 else divmod(hit[0], cost.shape[1])
        raise RuntimeError('%s: the auction of pair %s stopped at the cap of %d rounds: no distance for it' % (who, where, max_rounds))


def pairwise_emd(p1, p2, phases=6):
    """(G, R) float64: the earth mover's distance of EVERY pair of clouds of p1 (G, N, 3) and p2 (R, N, 3) -- cost / N of
    optimal_matching(paired=False), the mean distance of a point to its partner under the optimal assignment, within D 4^-phases of the
    optimum.  The distance matrix that minimum_matching_distance, coverage and one_nn_accuracy take (MMD-EMD, COV-EMD, 1-NNA-EMD).
    Neither the matching nor the prices are asked for or stored.  One read-back of `rounds`: a pair that stopped at the round cap
    raises RuntimeError -- minimum_matching_distance passes over unacceptable entries, so a silent NaN would be dropped, not seen.  A
    pair with a non-finite coordinate is NaN, as in the chamfer matrix.  No gradient."""
    p1, p2, max_rounds = _check_match_arguments('pairwise_emd', p1, p2, phases, None, False)
    _, cost, rounds, _ = _optimal_matching_unchecked(p1, p2, phases, max_rounds, False, want_match=False, want_prices=False)
    _raise_if_capped('pairwise_emd', cost, rounds, max_rounds)
    return cost / p1.shape[1]


def earth_movers_distance(p1, p2, phases=6):
    """(B,) in the dtype of p1: the earth mover's distance of cloud b of p1 (B, N, 3) against cloud b of p2 (B, N, 3), the mean of
    |p1_i - p2[match_i]| under optimal_matching's assignment.  The matching is found without a gradient; the value is recomputed in
    torch at that matching (the root through the zero-safe _rooted, the mean in double), so it is differentiable in both sets by
    autograd at the fixed matching -- the gradient almost everywhere, as the matching is piecewise constant.  One read-back: a pair
    that stopped at the round cap raises RuntimeError; a pair with a non-finite coordinate is NaN."""
    who = 'earth_movers_distance'
    _check_point_sets(who, p1, p2)
    q1, q2, max_rounds = _check_match_arguments(who, p1, p2, phases, None, True)
    match, cost, rounds, _ = _optimal_matching_unchecked(q1, q2, phases, max_rounds, True, want_prices=False)
    _raise_if_capped(who, cost, rounds, max_rounds)
    p2 = p2.to(device=p1.device, dtype=p1.dtype)
    diff = p1 - torch.gather(p2, 1, match.clamp(min=0)[..., None].expand(-1, -1, 3))
    value = _per_cloud_mean(_rooted((diff * diff).sum(-1)))
    return torch.where(torch.isnan(cost), cost, value).to(p1.dtype)


# ---- occupancy histograms of point sets on a lattice, and their Jensen-Shannon divergence ------------------------------------------------
_OCCUPANCY_MAX_R = 32              # lattice points per axis at most: the 32^3 cells of a workgroup's histogram fill 128 KiB of LDS
_OCCUPANCY_BOUNDS = (-1.0, 1.0)    # the cube of the tanh head's range: the default lattice needs no read-back of the data


def _fp32(value):
    """The fp32 number nearest to the Python number `value`, as a Python float (inf where it overflows; no warning)."""
    return torch.tensor(float(value), dtype=torch.float64).to(torch.float32).item()


def _check_lattice(who, resolution, bounds, name='resolution'):
    """The checks of a lattice -> (lo, inv_spacing), the two fp32 numbers of include/icn_occupancy.h as Python floats.  ValueError."""
    if isinstance(resolution, bool) or not isinstance(resolution, int) or not 1 <= resolution <= _OCCUPANCY_MAX_R:
        raise ValueError('%s: %s must be an integer in [1, %d], got %r' % (who, name, _OCCUPANCY_MAX_R, resolution))
    if not isinstance(bounds, (tuple, list)) or len(bounds) != 2 \
            or any(isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v in (float('inf'), -float('inf')) for v in bounds) \
            or not bounds[0] < bounds[1]:
        raise ValueError('%s: bounds must be two finite numbers (lo, hi) with lo < hi, got %r' % (who, bounds))
    lo = _fp32(bounds[0])
    inv_spacing = _fp32((resolution - 1) / (float(bounds[1]) - float(bounds[0]))) if resolution > 1 else 1.0
    if lo in (float('inf'), -float('inf')) or inv_spacing == float('inf') or not inv_spacing > 0.0:
        raise ValueError('%s: bounds %r give no fp32 lattice of %d points an axis' % (who, bounds, resolution))
    return lo, inv_spacing


def _check_clouds(who, clouds):
    """The shape checks of one set of clouds.  ValueError."""
    if not torch.is_tensor(clouds) or not clouds.is_floating_point() or clouds.dim() != 3 or clouds.shape[-1] != 3 or clouds.shape[0] < 1 \
            or clouds.shape[1] < 1:
        raise ValueError('%s: expected the set as a floating-point (clouds, points, 3) tensor with clouds, points >= 1, got %s'
                         % (who, tuple(clouds.shape) if torch.is_tensor(clouds) else type(clouds).__name__))
    if clouds.shape[0] * clouds.shape[1] > 0x7fffffff:
        raise ValueError('%s: %d clouds of %d points: B N must fit an int32' % (who, clouds.shape[0], clouds.shape[1]))


def _torch_occupancy_counts(clouds, resolution, lo, inv_spacing, per_cloud=False):
    """THE DEFINITION of occupancy_counts restated in torch (include/icn_occupancy.h, where it is written out), on any device ->
    (counts int32 (R, R, R) or (B, R, R, R), dropped int32 () or (B,)).  fp32 whatever the dtype of `clouds` (they are converted first:
    exact for the narrower types, to the nearest for float64), every operation a torch operation of its own in the header's order:
    t = (x - lo) * inv_spacing, u = floor(t + 0.5), i = clamp(u, 0, R - 1), c = (ix R + iy) R + iz, then one bincount.  A point with a
    non-finite coordinate is masked before the arithmetic (it runs on zeros and lands in a bin of its own that is cut off)."""
    B, N, _ = clouds.shape
    R = resolution
    cells = R * R * R
    with torch.no_grad():
        p = clouds.detach().to(torch.float32)
        dev = p.device
        finite = torch.isfinite(p).all(-1)                                                 # (B, N)
        p = torch.where(finite[..., None], p, torch.zeros_like(p))
        t = (p - torch.tensor(lo, dtype=torch.float32, device=dev)) * torch.tensor(inv_spacing, dtype=torch.float32, device=dev)
        u = torch.floor(t + torch.tensor(0.5, dtype=torch.float32, device=dev))
        i = u.clamp(0.0, float(R - 1)).to(torch.int64)
        c = (i[..., 0] * R + i[..., 1]) * R + i[..., 2]
        rows = B if per_cloud else 1
        if per_cloud:
            c = c + cells * torch.arange(B, device=dev)[:, None]
        c = torch.where(finite, c, torch.full_like(c, rows * cells))
        counts = torch.bincount(c.reshape(-1), minlength=rows * cells + 1)[:rows * cells].to(torch.int32)
        dropped = (~finite).sum(-1) if per_cloud else (~finite).sum()
    return counts.reshape((B, R, R, R) if per_cloud else (R, R, R)), dropped.to(torch.int32)


def _hip_occupancy_counts(pts, resolution, lo, inv_spacing, per_cloud):
    """icn_point_occupancy on a contiguous fp32 ROCm tensor -> (counts, dropped) int32."""
    B, N, _ = pts.shape
    R = resolution
    L = _lib.api()
    if per_cloud:
        counts = torch.empty(B, R, R, R, dtype=torch.int32, device=pts.device)
        dropped = torch.empty(B, dtype=torch.int32, device=pts.device)
        with torch.cuda.device(pts.device):
            for b0, nb in _batch_slices(B):                                  # (the workspace is asked per slice: fewer clouds may take more pieces)
                ws_bytes = L.icn_point_occupancy_workspace_bytes(nb, N, R, 1)
                ws = _lib.workspace(ws_bytes, pts.device)
                L.icn_point_occupancy(pts[b0:].data_ptr(), nb, N, R, lo, inv_spacing, 1, counts[b0:].data_ptr(), dropped[b0:].data_ptr(),
                                      ws.data_ptr(), ws_bytes, _lib.stream())
        return counts, dropped
    if B > _MAX_GRID_Y:                                                      # the set's histogram does not see where a cloud ends
        B, N = 1, B * N
    counts = torch.empty(R, R, R, dtype=torch.int32, device=pts.device)
    dropped = torch.empty((), dtype=torch.int32, device=pts.device)
    ws_bytes = L.icn_point_occupancy_workspace_bytes(B, N, R, 0)
    ws = _lib.workspace(ws_bytes, pts.device)
    with torch.cuda.device(pts.device):
        L.icn_point_occupancy(pts.data_ptr(), B, N, R, lo, inv_spacing, 0, counts.data_ptr(), dropped.data_ptr(), ws.data_ptr(), ws_bytes,
                              _lib.stream())
    return counts, dropped


def _occupancy_counts_unchecked(clouds, resolution, lo, inv_spacing, per_cloud=False):
    """occupancy_counts after its checks; no host synchronisation on the HIP path."""
    if _on_hip_path(clouds):
        return _hip_occupancy_counts(clouds.detach().contiguous(), resolution, lo, inv_spacing, per_cloud)
    return _torch_occupancy_counts(clouds, resolution, lo, inv_spacing, per_cloud)


def occupancy_counts(clouds, resolution=28, bounds=_OCCUPANCY_BOUNDS, per_cloud=False):
    """(counts, dropped) int32: the occupancy histogram of a SET of clouds (B, N, 3) on a lattice of R = `resolution` lattice points an
    axis from bounds[0] to bounds[1] on every axis -- counts (R, R, R), the number of points of the whole set nearest to each lattice
    point, and dropped (), the number of points with a non-finite coordinate, which are counted in no cell.  per_cloud=True gives one
    histogram a cloud: counts (B, R, R, R), dropped (B,).  No gradient.

    One definition for the HIP kernel (include/icn_occupancy.h), the torch restatement (_torch_occupancy_counts) and the tests, in
    fp32 with every operation rounded on its own: with lo = float32(bounds[0]) and inv_spacing = float32((R - 1) / (hi - lo)) (1.0 for
    R = 1), computed here so that both routes use the same bits,
        t = (x - lo) * inv_spacing,  u = floor(t + 0.5),  i = clamp(u, 0, R - 1)  per axis;   cell (ix, iy, iz)
    -- the nearest lattice point, a tie goes up, anything outside the cube is clamped onto the boundary lattice point (a t that
    overflows included).  Integer counts are order-free, so the result is fixed bit for bit: row b of a per-cloud call equals the
    call on that cloud alone, the set histogram equals the sum of the rows, counts.sum() + dropped.sum() == B N.
    The default bounds (-1, 1) are the cube of the tanh head's range, so nothing is read back to place the lattice; (-0.5, 0.5) is the
    literature's unit cube.  The lattice is the whole cube: the variant of some code bases that keeps only the lattice points inside
    the inscribed sphere is not offered.
    ROCm fp32 tensors run on icn_point_occupancy: every workgroup a private histogram of R^3 words in LDS, integer LDS atomics, one
    workgroup per 16 384 points up to one a CU and a second launch that adds their histograms; no global atomics.  CPU tensors, other
    dtypes (converted to fp32 first) and ICN_NO_HIP_LOSS=1 take the restatement.  Arguments are checked (ValueError): resolution an
    integer in [1, 32], bounds two finite Python numbers lo < hi, B N <= 2^31 - 1."""
    _check_clouds('occupancy_counts', clouds)
    lo, inv_spacing = _check_lattice('occupancy_counts', resolution, bounds)
    return _occupancy_counts_unchecked(clouds, resolution, lo, inv_spacing, bool(per_cloud))


def _torch_occupancy_jsd(counts_a, counts_b):
    """THE DEFINITION of occupancy_jsd restated in torch (include/icn_occupancy.h), in float64 on any device -> 0-dim float64.  The
    totals are integer sums; p = a / A, q = b / B, m = 0.5 (p + q), s = 0.5 (p log2(p / m) + q log2(q / m)) with a term of an empty
    cell exactly 0, summed by torch (the header's order is the kernel's: the two agree within 2^-44); NaN if a histogram is empty."""
    a, b = counts_a.reshape(-1).to(torch.int64), counts_b.reshape(-1).to(torch.int64)
    A, B = a.sum(), b.sum()
    p, q = a.double() / A.double(), b.double() / B.double()
    m = 0.5 * (p + q)
    one, zero = torch.ones_like(p), torch.zeros_like(p)
    tp = torch.where(a > 0, p * torch.log2(torch.where(a > 0, p / m, one)), zero)
    tq = torch.where(b > 0, q * torch.log2(torch.where(b > 0, q / m, one)), zero)
    jsd = (0.5 * (tp + tq)).sum()
    return torch.where((A == 0) | (B == 0), torch.full_like(jsd, float('nan')), jsd)


def _occupancy_jsd_unchecked(counts_a, counts_b):
    """occupancy_jsd after its checks; no host synchronisation."""
    from . import losses
    if not losses._NO_HIP_LOSS and counts_a.is_cuda and counts_a.dtype == torch.int32 and counts_b.dtype == torch.int32:
        a, b = counts_a.contiguous(), counts_b.contiguous()
        jsd = torch.empty((), dtype=torch.float64, device=a.device)
        with torch.cuda.device(a.device):
            _lib.api().icn_occupancy_jsd(a.data_ptr(), b.data_ptr(), a.shape[0], jsd.data_ptr(), _lib.stream())
        return jsd
    return _torch_occupancy_jsd(counts_a, counts_b)


def occupancy_jsd(counts_a, counts_b):
    """0-dim float64: the Jensen-Shannon divergence, base 2, of two occupancy histograms (R, R, R) of non-negative integers, as
    occupancy_counts gives them -- for callers who keep histograms.  All in double (include/icn_occupancy.h): with the totals A and B
    as integers, p = a / A, q = b / B, m = 0.5 (p + q), jsd = sum over the cells of 0.5 (p log2(p / m) + q log2(q / m)), a term of an
    empty cell 0; in [0, 1]; NaN if either histogram is empty.  Identical histograms give exactly 0.0 and swapping the two gives the
    same bits.  ROCm int32 tensors run on icn_occupancy_jsd (one workgroup, a fixed order: bit-identical run to run), anything else
    on the restatement _torch_occupancy_jsd; the two agree within 2^-44.  Shapes are checked (ValueError); nothing is read back."""
    for name, x in (('the first', counts_a), ('the second', counts_b)):
        if not torch.is_tensor(x) or x.is_floating_point() or x.is_complex() or x.dtype == torch.bool or x.dim() != 3 \
                or not 1 <= x.shape[0] <= _OCCUPANCY_MAX_R or x.shape != (x.shape[0],) * 3:
            raise ValueError('occupancy_jsd: expected %s histogram as an integer (R, R, R) tensor with 1 <= R <= %d, got %s'
                             % (name, _OCCUPANCY_MAX_R, '%s %s' % (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__))
    if counts_a.shape != counts_b.shape or counts_a.device != counts_b.device:
        raise ValueError('occupancy_jsd: the histograms must have one shape and one device, got %s on %s and %s on %s'
                         % (tuple(counts_a.shape), counts_a.device, tuple(counts_b.shape), counts_b.device))
    return _occupancy_jsd_unchecked(counts_a, counts_b)


def jensen_shannon_divergence(generated, reference, resolution=28, bounds=_OCCUPANCY_BOUNDS):
    """0-dim float64: the Jensen-Shannon divergence (base 2, in [0, 1]) between the occupancy distributions of a set of generated
    clouds (G, N, 3) and a set of reference clouds (R, M, 3) -- the JSD column of the shape-generation tables (Achlioptas et al. 2018):
    occupancy_jsd of the two occupancy_counts(., resolution, bounds), which see each set as one heap of points, so the sets need
    neither one size nor one point count.  0 for two sets that fill the lattice alike, 1 for two sets that share no cell.  The
    papers use resolution 28 on the unit cube, bounds=(-0.5, 0.5), of shapes normalised into it; the default bounds (-1, 1) are the
    cube of the tanh head's range.  The lattice is the whole cube: the variant that keeps only the lattice points inside the
    inscribed sphere is not offered.  NaN if every point of a set is non-finite.  No gradient; nothing is read back."""
    generated, reference = _check_cloud_sets('jensen_shannon_divergence', generated, reference)
    for x in (generated, reference):
        _check_clouds('jensen_shannon_divergence', x)
    lo, inv_spacing = _check_lattice('jensen_shannon_divergence', resolution, bounds)
    return _jsd_unchecked(generated, reference, resolution, lo, inv_spacing)


def _jsd_unchecked(generated, reference, resolution, lo, inv_spacing):
    """jensen_shannon_divergence after its checks."""
    a, b = (_occupancy_counts_unchecked(x, resolution, lo, inv_spacing)[0] for x in (generated, reference))
    return _occupancy_jsd_unchecked(a, b)


def _check_jsd_resolution(who, jsd):
    """The check of the `jsd=` option -> jsd.  ValueError."""
    if isinstance(jsd, bool) or not isinstance(jsd, int) or not 0 <= jsd <= _OCCUPANCY_MAX_R:
        raise ValueError('%s: jsd must be an integer in [0, %d], the lattice points an axis (0: no JSD), got %r' % (who, _OCCUPANCY_MAX_R, jsd))
    return jsd


GENERATION_DISTANCES = ('chamfer', 'emd')


def _check_subset_size(who, points):
    """The check of the `points=` option -> points.  ValueError."""
    if isinstance(points, bool) or not isinstance(points, int) or points < 0:
        raise ValueError('%s: points must be a non-negative integer, got %r' % (who, points))
    return points


def _farthest_subsets(who, clouds, points):
    """The `points=` option: every cloud of `clouds` (B, N, 3) thinned to its `points` farthest points (sampling.farthest_points from
    index 0), without a gradient.  A cloud smaller than that raises ValueError."""
    if points > clouds.shape[1]:
        raise ValueError('%s: points=%d is more than the %d points of a cloud' % (who, points, clouds.shape[1]))
    from .sampling import farthest_points
    with torch.no_grad():
        return farthest_points(clouds.detach(), points)


def generation_metrics(generated, reference, distance='chamfer', points=0, jsd=0):
    """dict(mmd=, cov=, one_nna=) of Python floats for a set of generated clouds (G, N, 3) against a set of reference clouds (R, M, 3):
    minimum_matching_distance and coverage of pairwise_chamfer(generated, reference), one_nn_accuracy with the two within-set matrices
    as well.  Three pairwise_chamfer calls (squared distances, unit weights) and one read-back at the end.
    distance='emd' takes the three matrices from pairwise_emd instead (MMD-EMD, COV-EMD, 1-NNA-EMD; M == N then).
    points = P > 0 replaces both sets by sampling.farthest_points(., P) first -- the protocol of the shape-generation tables, P
    well-spread points a shape (2 048 there), which is what makes the EMD matrices affordable; P larger than a cloud raises
    ValueError.  points=0 (default) matches whole clouds.
    jsd = R > 0 adds the key 'jsd', the first column of those tables: jensen_shannon_divergence of the two sets on a lattice of R
    lattice points an axis (28 there; at most 32) over the default bounds (-1, 1), on exactly the point sets the matrices see (after
    points=), in the same read-back.  The lattice is the whole cube; the variant that keeps only the lattice points inside the
    inscribed sphere is not offered.  jsd=0 (default) returns the three keys alone."""
    if distance not in GENERATION_DISTANCES:
        raise ValueError('generation_metrics: distance must be one of %s, got %r' % (GENERATION_DISTANCES, distance))
    _check_subset_size('generation_metrics', points)
    _check_jsd_resolution('generation_metrics', jsd)
    generated, reference = _check_cloud_sets('generation_metrics', generated, reference)
    if points:
        generated, reference = (_farthest_subsets('generation_metrics', x, points) for x in (generated, reference))
    if distance == 'emd':
        d_gr, d_gg, d_rr = pairwise_emd(generated, reference), pairwise_emd(generated, generated), pairwise_emd(reference, reference)
        figures = [minimum_matching_distance(d_gr), coverage(d_gr), one_nn_accuracy(d_gg, d_gr, d_rr)]
    else:
        d_gr = pairwise_chamfer(generated, reference)
        d_gg, d_rr = pairwise_chamfer(generated, generated), pairwise_chamfer(reference, reference)
        figures = [minimum_matching_distance(d_gr).double(), coverage(d_gr), one_nn_accuracy(d_gg, d_gr, d_rr)]
    if jsd:
        _check_clouds('generation_metrics', generated), _check_clouds('generation_metrics', reference)
        figures.append(_jsd_unchecked(generated, reference, jsd, *_check_lattice('generation_metrics', jsd, _OCCUPANCY_BOUNDS, 'jsd')))
    return dict(zip(('mmd', 'cov', 'one_nna', 'jsd'), torch.stack(figures).tolist()))


def output2vertices(subdivisions, output):
    """Grid -> vertex list incl. the two pole means (reference ico_utils.py:10-24)."""
    from .losses import grid_to_vertices
    return grid_to_vertices(output, subdivisions)


def compute_distance(outvertices, refvertices, reffaces, mode='point2mesh', search='brute'):
    """ico_utils.py:26-44 computeDistance for one mesh pair ((N, 3) tensors): mean squared point-to-mesh distance of the
    output's vertices to the reference mesh, as a Python float; None for other modes (as the reference).  `search` as in
    point_to_mesh_distance."""
    _check_search(search)
    if mode != 'point2mesh':
        return None
    dist, _, _ = point_to_mesh_distance(outvertices[None], refvertices[None], reffaces, search=search)
    return float(dist.mean())


EVALUATION_MODES = ('point2point', 'point2mesh', 'chamfer', 'f_<radius>', 'hausdorff', 'emd')


def evaluate_distance(outvertices, refvertices, reffaces, mode, samples=0, seed=0, points=0):
    """The test modes the reference names (run.py:630: point2point, point2mesh, chamfer, f_<radius>) and 'hausdorff', for one mesh
    pair ((V, 3) tensors; `reffaces` (F, 3) is the face table of both, as everywhere in the reference), as a Python float.
    compute_distance itself keeps answering None to every mode but 'point2mesh', as the reference's computeDistance does.
        'point2point'  the mean squared distance of corresponding vertices (the two meshes have one shape)
        'point2mesh'   exactly compute_distance(outvertices, refvertices, reffaces)
        'chamfer'      chamfer_distance of the two point sets
        'f_<radius>'   f_score of the output's points against the reference's at that radius, for example 'f_0.01'
        'hausdorff'    hausdorff_distance of the two point sets
        'emd'          earth_movers_distance of the two point sets, which have one size (the vertices, or S samples each)
    The point sets of the last four are the vertices, or with samples = S > 0 sampling.sample_points of the two surfaces from
    uniforms torch.rand((2, S, 3), generator=g), g a CPU generator seeded with `seed` (the output's surface takes the first S): the
    same samples on every device.  points = P > 0 then thins both point sets of those four modes to their P farthest points
    (sampling.farthest_points; after the surface sampling, so samples=S, points=P is "S surface samples thinned to P"); P larger than a
    point set raises ValueError, and points=0 (default) keeps the sets whole.  An unknown mode raises ValueError."""
    who = 'evaluate_distance'
    radius = None
    if isinstance(mode, str) and mode.startswith('f_'):
        try:
            radius = float(mode[2:])
        except ValueError:
            radius = None
        if radius is None or not radius >= 0 or radius == float('inf'):
            raise ValueError("%s: mode 'f_<radius>' needs a finite radius >= 0, got %r" % (who, mode))
    elif mode not in ('point2point', 'point2mesh', 'chamfer', 'hausdorff', 'emd'):
        raise ValueError('%s: mode must be one of %s, got %r' % (who, EVALUATION_MODES, mode))
    if isinstance(samples, bool) or not isinstance(samples, int) or samples < 0:
        raise ValueError('%s: samples must be a non-negative integer, got %r' % (who, samples))
    _check_subset_size(who, points)
    if outvertices.dim() != 2 or refvertices.dim() != 2 or outvertices.shape[-1] != 3 or refvertices.shape[-1] != 3:
        raise ValueError('%s: expected two (V, 3) vertex tensors, got %s and %s' % (who, tuple(outvertices.shape), tuple(refvertices.shape)))
    if mode == 'point2mesh':
        return compute_distance(outvertices, refvertices, reffaces)
    with torch.no_grad():
        out, ref = outvertices.detach()[None], refvertices.detach().to(device=outvertices.device, dtype=outvertices.dtype)[None]
        if mode == 'point2point':
            if out.shape != ref.shape:
                raise ValueError('%s: point2point needs two meshes of one shape, got %s and %s' % (who, tuple(out.shape[1:]), tuple(ref.shape[1:])))
            diff = (out - ref).double()
            return float((diff * diff).sum(-1).mean())
        if samples:
            from .sampling import sample_points
            u = torch.rand((2, 1, samples, 3), generator=torch.Generator().manual_seed(seed)).to(device=out.device, dtype=out.dtype)
            out, ref = sample_points(out, reffaces, uniforms=u[0])[0], sample_points(ref, reffaces, uniforms=u[1])[0]
        if points:
            out, ref = _farthest_subsets(who, out, points), _farthest_subsets(who, ref, points)
        if mode == 'chamfer':
            return float(chamfer_distance(out, ref)[0])
        if mode == 'hausdorff':
            return float(hausdorff_distance(out, ref)[0])
        if mode == 'emd':
            return float(earth_movers_distance(out, ref)[0])
        return float(f_score(ref, out, radius=radius)[0])
