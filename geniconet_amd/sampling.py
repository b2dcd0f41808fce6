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
float64, searchsorted(..., right=True)), which computes areas, weights and points in the dtype of `vertices`."""
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
