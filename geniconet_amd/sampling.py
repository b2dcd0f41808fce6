"""Area-weighted surface sampling of triangle meshes: what kaolin.ops.mesh.sample_points and pytorch3d's
sample_points_from_meshes draw, from uniforms the caller can supply (the kernels draw no random numbers: a pure function).

    points (B, S, 3), face (B, S) int64 = sample_points(vertices (B, V, 3), faces (F, 3), num_samples=S)        # or uniforms=(B, S, 3)

One definition for the HIP kernels (icn_mesh_sample_fwd / icn_mesh_sample_bwd in include/icn.h), the torch formulation and the tests.
Per mesh, with u (S, 3) uniforms in [0, 1):
    A_f    = 0.5 |(v1 - v0) x (v2 - v0)| with every product of the cross product rounded on its own (Mesh_Regularizer._face_normal;
             face_normal in k_msample_area), so a face with two or three coincident vertices has area exactly 0
    c_f    = A_0 + ... + A_f in float64, T = c_{F-1}
    face_s = the smallest f with c_f > u[s,0] T (in float64): a zero-area face is never chosen while T > 0; for u[s,0] = 1, where no such
             f exists, the last face of positive area; face 0 for every sample if T is not a positive finite number
    r      = sqrt(u[s,1]);  weights_s = (1 - r, r (1 - u[s,2]), r u[s,2]);  points_s = sum_k weights[s,k] v_k of face_s
Components of u outside [0, 1] are clamped and NaN counts as 0.  The gradient goes to `vertices` only, through the weights with the
face choice held constant (as kaolin and pytorch3d differentiate): dvertices[b, faces[face_s, k]] += weights[s,k] dpoints[s]; on the
HIP path it is summed in a fixed order without floating-point atomics (bit-identical run to run, an untouched vertex gets an exact 0).

ROCm fp32 tensors run on the HIP kernels; CPU tensors, other dtypes and ICN_NO_HIP_LOSS=1 take the torch formulation (cumsum in
float64, searchsorted(..., right=True)), which computes areas, weights and points in the dtype of `vertices`.

farthest_point_sample and farthest_points (below) thin a cloud -- the vertices, or such surface samples -- to a fixed number of
WELL-SPREAD points: farthest point sampling, the subset the shape-generation tables (MMD / COV / 1-NNA on 2 048 points a shape) are
computed on, where random surface samples have clumps and holes (icn_farthest_points, include/icn_fps.h: one workgroup a cloud, every
point in a register, one barrier a step)."""
import torch

from . import metrics
from .metrics import _NB, _launch, _per_mesh


def _face_areas(vertices, f):
    """(B, F) areas in the dtype of vertices; f (F, 3) int64."""
    v0, v1, v2 = vertices[:, f[:, 0]], vertices[:, f[:, 1]], vertices[:, f[:, 2]]
    ax, ay, az = (v1 - v0).unbind(-1)
    bx, by, bz = (v2 - v0).unbind(-1)
    nx, ny, nz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx      # every product rounded on its own: a x a = 0 exactly (as the HIP kernel's face_normal)
    return 0.5 * (nx * nx + ny * ny + nz * nz).sqrt()


def _torch_sample(vertices, faces, u):
    """The definition of the module docstring in torch -> (points, face int64, weights); differentiable in vertices."""
    B, S, _ = u.shape
    f = faces.long()
    F = f.shape[0]
    u = torch.nan_to_num(u.detach().to(vertices.dtype), nan=0.0).clamp(0.0, 1.0)
    with torch.no_grad():
        cdf = _face_areas(vertices.detach(), f).double().cumsum(1)
        total = cdf[:, -1:]
        usable = (total > 0) & torch.isfinite(total)
        cdf = torch.where(usable, cdf, torch.zeros_like(cdf))                  # keeps searchsorted's input sorted (no NaN)
        total = torch.where(usable, total, torch.zeros_like(total))
        face = torch.searchsorted(cdf, u[..., 0].double() * total, right=True)
        last = torch.searchsorted(cdf, total, right=False)                     # the last face of positive area (u0 = 1)
        face = torch.where(face >= F, last.expand_as(face), face)
        face = torch.where(usable, face, torch.zeros_like(face)).clamp_(0, F - 1)
        r = u[..., 1].sqrt()
        weights = torch.stack((1 - r, r * (1 - u[..., 2]), r * u[..., 2]), dim=-1)
    corners = vertices[torch.arange(B, device=vertices.device)[:, None, None], f[face]]      # (B, S, 3 corners, 3)
    points = (weights[..., 0:1] * corners[:, :, 0] + weights[..., 1:2] * corners[:, :, 1]) + weights[..., 2:3] * corners[:, :, 2]
    return points, face, weights


def _hip_sample(vts, f32, u):
    """icn_mesh_sample_fwd on contiguous fp32 ROCm tensors and int32 faces -> (points, face int32, weights)."""
    (B, V, _), S, F = vts.shape, u.shape[1], f32.shape[0]
    points = torch.empty(B, S, 3, dtype=torch.float32, device=vts.device)
    face = torch.empty(B, S, dtype=torch.int32, device=vts.device)
    weights = torch.empty(B, S, 3, dtype=torch.float32, device=vts.device)
    _launch('icn_mesh_sample_fwd', _per_mesh(vts), f32, _per_mesh(u), _NB, S, V, F, _per_mesh(points), _per_mesh(face),
            _per_mesh(weights), workspace=('icn_mesh_sample_workspace_bytes', S, V, F))
    return points, face, weights


def _hip_sample_bwd(f32, face, weights, dpoints, V):
    """icn_mesh_sample_bwd -> dvertices (B, V, 3); face int32 (B, S), weights / dpoints contiguous fp32 (B, S, 3)."""
    (B, S), F = face.shape, f32.shape[0]
    dvts = torch.empty(B, V, 3, dtype=torch.float32, device=face.device)
    _launch('icn_mesh_sample_bwd', f32, _per_mesh(face), _per_mesh(weights), _per_mesh(dpoints), _NB, S, V, F, _per_mesh(dvts),
            workspace=('icn_mesh_sample_bwd_workspace_bytes', S, V, F))
    return dvts


class _SamplePointsFn(torch.autograd.Function):
    """sample_points on the HIP path with its gradient to the vertices (face choice and weights constant)."""

    @staticmethod
    def forward(ctx, vertices, f32, u):
        points, face, weights = _hip_sample(vertices.contiguous(), f32, u.contiguous())
        ctx.save_for_backward(f32, face, weights)
        ctx.num_vertices = vertices.shape[1]
        face64 = face.long()
        ctx.mark_non_differentiable(face64, weights)
        return points, face64, weights

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dpoints, _gface, _gweights):
        f32, face, weights = ctx.saved_tensors
        return _hip_sample_bwd(f32, face, weights, dpoints.contiguous().to(torch.float32), ctx.num_vertices), None, None


def _sample_points_unchecked(vertices, f32, uniforms):
    """sample_points without its argument checks and without a host synchronisation, for callers that validated once
    (losses.Surface_Loss): f32 is an int32 (F, 3) tensor on the vertices' device, F >= 1, with indices in [0, V); uniforms (B, S, 3)
    on the same device.  -> (points, face int64, weights)."""
    if metrics._on_hip_path(vertices) and uniforms.dtype == torch.float32:
        if torch.is_grad_enabled() and vertices.requires_grad:
            return _SamplePointsFn.apply(vertices, f32, uniforms)
        points, face, weights = _hip_sample(vertices.detach().contiguous(), f32, uniforms.detach().contiguous())
        return points, face.long(), weights
    return _torch_sample(vertices, f32, uniforms)


def sample_points(vertices, faces, num_samples=None, uniforms=None, generator=None):
    """See the module docstring.  `faces` may be int32 / int64, (F, 3), shared by the batch.  Either `uniforms` (B, S, 3) is given, or
    `num_samples` and the uniforms are drawn with torch.rand((B, S, 3), generator=generator) on the vertices' device.
    -> (points (B, S, 3), face (B, S) int64).  Face indices are checked against V (IndexError, one host synchronisation)."""
    if vertices.dim() != 3 or vertices.shape[-1] != 3 or vertices.shape[0] < 1 or not vertices.is_floating_point():
        raise ValueError('sample_points: expected floating-point vertices (B, V, 3), got %s' % (tuple(vertices.shape),))
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError('sample_points: expected faces (F, 3) with F >= 1, got %s' % (tuple(faces.shape),))
    if (uniforms is None) == (num_samples is None):
        raise ValueError('sample_points: give either num_samples or uniforms')
    B = vertices.shape[0]
    if uniforms is None:
        if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 1:
            raise ValueError('sample_points: num_samples must be a positive integer, got %r' % (num_samples,))
        uniforms = torch.rand((B, num_samples, 3), generator=generator, device=vertices.device, dtype=torch.float32)
    elif uniforms.dim() != 3 or tuple(uniforms.shape[::2]) != (B, 3) or uniforms.shape[1] < 1 or not uniforms.is_floating_point():
        raise ValueError('sample_points: expected floating-point uniforms (%d, S, 3) with S >= 1, got %s' % (B, tuple(uniforms.shape)))
    lo, hi = torch.stack(faces.aminmax()).tolist()                            # one read-back
    if lo < 0 or hi >= vertices.shape[1]:
        raise IndexError('sample_points: face indices span [%d, %d] but there are %d vertices' % (lo, hi, vertices.shape[1]))
    f32 = faces.to(device=vertices.device, dtype=torch.int32).contiguous()
    uniforms = uniforms.to(vertices.device)
    if vertices.dtype == torch.float32:
        uniforms = uniforms.to(torch.float32)                                  # uniforms of another dtype must not leave the HIP path
    points, face, _ = _sample_points_unchecked(vertices, f32, uniforms)
    return points, face


# ---- farthest point sampling: a fixed number of well-spread points of every cloud ---------------------------------------------------------
_FPS_MAX_N = 13312                 # points a cloud may hold on the HIP path: every point in a register of its workgroup (include/icn_fps.h)


def _torch_farthest_point_sample(points, count, start=0):
    """THE DEFINITION of farthest_point_sample restated in torch (include/icn_fps.h, where it is written out), in the dtype of `points`
    on any device -> (idx (B, count) int64, cover (B, count)); no graph, nothing read back.  Every difference, product and sum is a
    torch operation of its own, in the order of the header; the lowest index among equal distances is picked explicitly (torch's own
    argmax promises no tie rule on every device).  A cloud with a non-finite coordinate is masked BEFORE the loop (it runs on zeros
    and its rows are overwritten with -1 / NaN), so no NaN ever enters the loop.  `count` dependent steps of about eight small
    operations each: the restatement, not the fast path."""
    B, N, _ = points.shape
    dev = points.device
    with torch.no_grad():
        p = points.detach()
        finite = torch.isfinite(p).all(-1).all(-1)                                        # (B,)
        x, y, z = torch.where(finite[:, None, None], p, torch.zeros_like(p)).unbind(-1)   # (B, N) each
        dist = torch.full((B, N), float('inf'), dtype=p.dtype, device=dev)
        idx = torch.empty((B, count), dtype=torch.int64, device=dev)
        cover = torch.empty((B, count), dtype=p.dtype, device=dev)
        everyone = torch.arange(N, device=dev)[None]
        nobody = torch.full_like(everyone, N)
        cur = torch.full((B, 1), start, dtype=torch.int64, device=dev)
        for s in range(count):
            idx[:, s] = cur[:, 0]
            dx, dy, dz = x - x.gather(1, cur), y - y.gather(1, cur), z - z.gather(1, cur)
            dist = torch.minimum(dist, (dx * dx + dy * dy) + dz * dz)
            top = dist.amax(1, keepdim=True)
            cover[:, s] = top[:, 0]
            cur = torch.where(dist == top, everyone, nobody).amin(1, keepdim=True)       # the lowest index among equals
        idx = torch.where(finite[:, None], idx, torch.full_like(idx, -1))
        cover = torch.where(finite[:, None], cover, torch.full_like(cover, float('nan')))
    return idx, cover


def _hip_farthest_point_sample(pts, count, start):
    """icn_farthest_points on a contiguous fp32 ROCm tensor of at most _FPS_MAX_N points a cloud -> (idx int32, cover fp32)."""
    B, N, _ = pts.shape
    idx = torch.empty(B, count, dtype=torch.int32, device=pts.device)
    cover = torch.empty(B, count, dtype=torch.float32, device=pts.device)
    _launch('icn_farthest_points', _per_mesh(pts), _NB, N, count, start, _per_mesh(idx), _per_mesh(cover))
    return idx, cover


def _check_farthest_arguments(who, points, count, start):
    """The checks of the farthest-point functions.  ValueError."""
    if not torch.is_tensor(points) or not points.is_floating_point() or points.dim() != 3 or points.shape[-1] != 3 or points.shape[0] < 1 \
            or points.shape[1] < 1:
        raise ValueError('%s: expected the point set as a floating-point (B, N, 3) tensor with B, N >= 1, got %s'
                         % (who, tuple(points.shape) if torch.is_tensor(points) else type(points).__name__))
    N = points.shape[1]
    if 3 * N > 0x7fffffff:
        raise ValueError('%s: %d points: 3 N must fit an int32' % (who, N))
    if isinstance(count, bool) or not isinstance(count, int) or not 1 <= count <= N:
        raise ValueError('%s: count must be an integer in [1, %d], the size of a cloud, got %r' % (who, N, count))
    if isinstance(start, bool) or not isinstance(start, int) or not 0 <= start < N:
        raise ValueError('%s: start must be an integer in [0, %d), got %r' % (who, N, start))


def _farthest_point_sample_unchecked(points, count, start):
    """farthest_point_sample after its checks."""
    if metrics._on_hip_path(points) and points.shape[1] <= _FPS_MAX_N:
        idx, cover = _hip_farthest_point_sample(points.detach().contiguous(), count, start)
        return idx.long(), cover
    return _torch_farthest_point_sample(points, count, start)


def farthest_point_sample(points, count, start=0):
    """(idx (B, count) int64, cover (B, count) in the dtype of points): farthest point sampling of every cloud of points (B, N, 3) --
    `count` indices of well-spread points, beginning with `start`, each next one the point farthest from all chosen so far; cover[b, s]
    is the largest squared distance of a point of the cloud to its nearest chosen point after s + 1 choices (the covering radius,
    squared).  The subset that the shape-generation tables match instead of whole clouds.  No gradient; farthest_points gathers the
    points themselves.

    One definition for the HIP kernel (include/icn_fps.h), the torch restatement (_torch_farthest_point_sample) and the tests.  All
    arithmetic is in the dtype of points (fp32 on the device), every product and sum rounded on its own:
        d(i, c) = (dx dx + dy dy) + dz dz,  dx = p_i.x - p_c.x, dy and dz likewise     (the d_j of sided_distance; symmetric bit for bit)
        dist_i = +inf, cur = start;  for s = 0 ... count - 1:
            idx[b, s] = cur;  dist_i = fminf(dist_i, d(i, cur)) for every i;  cover[b, s] = max_i dist_i;
            cur = the LOWEST i with dist_i == cover[b, s]
    Decided before the loop: a cloud with a non-finite coordinate gives idx -1 and cover NaN in its rows and leaves the other clouds of
    the batch alone.  fminf, max and the lowest-index argmax are order-free, so idx and cover are fixed bit for bit; with finite
    coordinates no NaN arises (an overflowing d is +inf).  Exactly, in the dtype: cover is non-increasing; cover[:, -1] is
    sided_distance(points, points[idx])[0].amax(-1); for count >= 2 the smallest d between two chosen points is cover[:, -2];
    count == N with distinct points gives a permutation with final cover 0; once the distinct points are used up cover is 0 and idx
    repeats index 0 -- duplicates are defined, not an error.
    ROCm fp32 tensors of at most 13312 points a cloud run on icn_farthest_points: one workgroup of 512 threads owns a cloud from
    start to finish, every point and its dist in registers, one 64-bit key (dist bits, ~index) a thread reduced over the wave and
    through one LDS slot a wave, one barrier a step; a batch costs about what one cloud does until there are more clouds than compute
    units, and idx and cover equal the restatement on CPU tensors bit for bit.  Batches beyond 65535 clouds go in several launches.
    CPU tensors, other dtypes, ICN_NO_HIP_LOSS=1 and ROCm clouds of MORE than 13312 points take the restatement: `count` dependent
    steps of about eight small operations each, so subsampling 100 000 surface samples stays possible, slowly.  Arguments are checked
    (ValueError): count and start integers with 1 <= count <= N and 0 <= start < N.  Nothing is read back."""
    _check_farthest_arguments('farthest_point_sample', points, count, start)
    return _farthest_point_sample_unchecked(points, count, start)


def farthest_points(points, count, start=0):
    """(B, count, 3): the points farthest_point_sample(points, count, start) chooses, by torch.gather -- differentiable in `points` at
    the fixed choice (the choice itself carries no gradient).  A cloud with a non-finite coordinate (idx -1) gives NaN rows."""
    _check_farthest_arguments('farthest_points', points, count, start)
    idx, _ = _farthest_point_sample_unchecked(points, count, start)
    chosen = torch.gather(points, 1, idx.clamp(min=0)[..., None].expand(-1, -1, 3))
    return torch.where((idx < 0)[..., None], torch.full_like(chosen, float('nan')), chosen)
