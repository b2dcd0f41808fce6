"""Losses of the ico2ico / ico2ico_vae training step (reference losses.py:10-145).

Same classes, constructor arguments and reporting methods as the reference.  The mesh helpers the reference
imports from the absent `PythonFunctions/mesh/utils.py` (losses.py:7) are restated here:
  * vertex normals: area-weighted face-normal accumulation, normalised -- the formula the reference itself
    ships for its preprocessing, generate.py:20-43;
  * Laplacian: uniform umbrella operator  mean(1-ring) - v  by default.  Upstream's sign / normalisation is unpinned
    (generate.py:197 writes target rows 6:9 with the absent mesh.utils.compute_laplacian), so the convention is a
    constructor option `laplacian` in LAPLACIAN_MODES -- 'mean-v', 'v-mean', 'sum-kv' (sum(ring) - k v), 'kv-sum' -- and
    data.IcoDataset checks the rows 6:9 of a dataset against it (data.detect_laplacian_convention), failing loudly on a
    mismatch instead of silently training towards the wrong curvature.
Loss values are kept as device tensors; `.item()` (a host sync in the reference on every iteration,
losses.py:72,81,129) only happens when get_last_losses() is called.

On ROCm fp32 tensors Point2Point_Loss runs on HIP kernels (libicn's icn_p2p_loss_*), forward and backward, for any
factors; the torch formulation below is what runs for other dtypes and for CPU tensors (as used by the CPU restatement in
bench.py), and it is what the HIP kernels are tested against besides the numpy oracle.  The KLD term (losses.py:105) runs
on icn_kld_fwd / icn_kld_bwd under the same conditions.

Point2Mesh_Loss is not in the reference: the surface distance it reports at test time (ico_utils.py:26-44) as a loss term.
Surface_Loss / SurfaceKLD_Loss (train.build_criterion: 'surface' / 'surfacekld') make a training criterion of it: the distance in
both directions plus Mesh_Regularizer (edge length, normal consistency, Laplacian smoothness; HIP kernels icn_mesh_reg_*); from
surface samples (samples > 0) optionally with the normal agreement of the two surfaces (factor_normal; icn_face_normal_agree_*),
and optionally with the enclosed volume and the surface area held to the target's (factor_volume / factor_area; icn_mesh_measure_*)
and with the Willmore bending energy of the output (factor_willmore; icn_mesh_willmore_*), the smoothness term that does not shrink,
and with the Gaussian curvature of the output held to the target's vertex by vertex (factor_gauss; icn_mesh_angle_defect_*).
"""
import math
import os

import torch

from . import _lib, geometry

_NO_HIP_LOSS = os.environ.get('ICN_NO_HIP_LOSS', '') == '1'
LAPLACIAN_MODES = _lib.LAP_MODES          # name -> ICN_LAP_* code of include/icn.h


def laplacian_code(laplacian):
    try:
        return LAPLACIAN_MODES[laplacian]
    except KeyError:
        raise ValueError('laplacian must be one of %s, got %r' % (sorted(LAPLACIAN_MODES), laplacian))


class _P2PLossFn(torch.autograd.Function):
    """Point2Point_Loss on the HIP path (icn_p2p_loss_* in include/icn.h): one kernel evaluates the three terms; the
    gradient is one kernel for the auto-encoder's factors 1/0/0 (run.py:690-692) and two for factors that weigh the normal
    and Laplacian terms (the VAE's 0.6/0.2/0.2, run.py:694-696)."""

    @staticmethod
    def forward(ctx, inputs, target, r, f_pos, f_nor, f_lap, lap_mode=0):
        L = _lib.api()
        B = inputs.shape[0]
        grid = inputs.permute(0, 2, 3, 1).contiguous()            # (B, 5n, 2n, 3) = (B, P, 3); free for channels_last
        tgt = target.contiguous()
        terms = torch.empty(4, dtype=torch.float32, device=inputs.device)
        ws = _lib.workspace(L.icn_p2p_loss_workspace_floats(B, r), inputs.device, torch.float32)
        with torch.cuda.device(inputs.device):
            L.icn_p2p_loss_fwd(grid.data_ptr(), tgt.data_ptr(), B, r, f_pos, f_nor, f_lap, lap_mode, terms.data_ptr(),
                               ws.data_ptr(), _lib.stream())
        ctx.save_for_backward(grid, tgt)
        ctx.cfg = (B, r, f_pos, f_nor, f_lap, lap_mode)
        total = terms[3].clone()
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gtotal, _gterms):
        B, r, f_pos, f_nor, f_lap, lap_mode = ctx.cfg
        L = _lib.api()
        grid, tgt = ctx.saved_tensors
        dgrid = torch.empty_like(grid)
        up = gtotal.contiguous().to(torch.float32)
        ws = None
        if f_nor != 0 or f_lap != 0:
            ws = _lib.workspace(L.icn_p2p_loss_bwd_workspace_floats(B, r), grid.device, torch.float32)
        with torch.cuda.device(grid.device):
            L.icn_p2p_loss_bwd(grid.data_ptr(), tgt.data_ptr(), up.data_ptr(), B, r, f_pos, f_nor, f_lap, lap_mode,
                               dgrid.data_ptr(), ws.data_ptr() if ws is not None else None, _lib.stream())
        return dgrid.permute(0, 3, 1, 2), None, None, None, None, None, None


class _KLDFn(torch.autograd.Function):
    """mean_b(-0.5 * mean_d(1 + logvar - mu^2 - exp(logvar))) on the HIP path (icn_kld_fwd / icn_kld_bwd): one
    deterministic two-level sum forward, one elementwise kernel backward -- reference losses.py:105."""

    @staticmethod
    def forward(ctx, mu, logvar):
        L = _lib.api()
        # elementwise + a full sum: any common element order will do; (B, H, W, C) storage is free for channels_last
        m, lv = (t.permute(0, 2, 3, 1).contiguous() if t.dim() == 4 else t.contiguous() for t in (mu, logvar))
        n = m.numel()
        out = torch.empty(1, dtype=torch.float32, device=m.device)
        ws = _lib.workspace(L.icn_kld_workspace_floats(n), m.device, torch.float32)
        with torch.cuda.device(m.device):
            L.icn_kld_fwd(m.data_ptr(), lv.data_ptr(), n, out.data_ptr(), ws.data_ptr(), _lib.stream())
        ctx.save_for_backward(m, lv)
        ctx.dim4 = mu.dim() == 4
        return out[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        L = _lib.api()
        m, lv = ctx.saved_tensors
        dm, dlv = torch.empty_like(m), torch.empty_like(lv)
        up = g.contiguous().to(torch.float32)
        with torch.cuda.device(m.device):
            L.icn_kld_bwd(m.data_ptr(), lv.data_ptr(), up.data_ptr(), m.numel(), dm.data_ptr(), dlv.data_ptr(), _lib.stream())
        if ctx.dim4:
            return dm.permute(0, 3, 1, 2), dlv.permute(0, 3, 1, 2)
        return dm, dlv


def kld(mu, logvar):
    """The KL term of losses.py:105 for (B, ...) tensors: HIP kernels for ROCm fp32 tensors of equal shape, torch otherwise."""
    if (not _NO_HIP_LOSS and mu.is_cuda and logvar.is_cuda and mu.dtype == torch.float32 and logvar.dtype == torch.float32
            and mu.shape == logvar.shape and mu.numel() > 0):
        return _KLDFn.apply(mu, logvar)
    mu, logvar = torch.flatten(mu, start_dim=1), torch.flatten(logvar, start_dim=1)
    return torch.mean(-0.5 * torch.mean(1 + logvar - mu.pow(2) - logvar.exp(), dim=1), dim=0)


def grid_to_vertices(x, subdivisions):
    """(B, C, 5n, 2n) -> (B, 10*4^r + 2, C): row-major grid then N, S poles (mean of the 5 corner pixels);
    reference losses.py:47-51, ico_utils.py:10-24."""
    n = 2 ** subdivisions
    B, C = x.shape[:2]
    x5 = x.reshape(B, C, 5, n, 2 * n)
    poles = torch.stack((x5[:, :, :, 0, 0].mean(-1), x5[:, :, :, n - 1, 2 * n - 1].mean(-1)), dim=2)
    return torch.cat((x.reshape(B, C, -1), poles), dim=2).transpose(1, 2).contiguous()


def compute_vertex_normals(v, faces, eps=1e-10):
    """v (B, N, 3), faces (F, 3) int64 -> unit vertex normals (B, N, 3), face-area weighted (generate.py:20-43)."""
    # index_select (backward = index_add) instead of advanced indexing (backward = sort-based scatter)
    v0, v1, v2 = (torch.index_select(v, 1, faces[:, k]) for k in range(3))
    fn = torch.cross(v1 - v0, v2 - v0, dim=2)
    vn = torch.zeros_like(v)
    for k in range(3):
        vn = vn.index_add(1, faces[:, k], fn)
    return vn / vn.norm(dim=2, keepdim=True).clamp_min(eps)


def compute_laplacian_batch(v, nbr_idx, nbr_w, laplacian='mean-v'):
    """Uniform Laplacian: mean of the 1-ring minus the vertex.  nbr_idx (N, 6) int64 (padding entries point at
    vertex 0 with weight 0), nbr_w (N, 6) = 1/valence or 0.  `laplacian` (LAPLACIAN_MODES): 'v-mean' flips the sign,
    'sum-kv' / 'kv-sum' multiply by the valence (sum(ring) - k v and its negative)."""
    mode = laplacian_code(laplacian)
    ring = torch.index_select(v, 1, nbr_idx.reshape(-1)).view(v.shape[0], nbr_idx.shape[0], 6, 3)
    lap = (ring * nbr_w[None, :, :, None]).sum(2) - v
    if mode & 2:
        lap = lap * (nbr_w > 0).sum(1).to(lap.dtype)[None, :, None]
    return -lap if mode & 1 else lap


class Point2Point_Loss(torch.nn.Module):
    """factor_pos * MSE(v) + factor_nor * mean(1 - cos(normals)) + factor_lap * MSE(laplacian)
    against target rows [0:3], [3:6], [6:9]  -- reference losses.py:10-85.  `laplacian` (keyword, not in the reference's
    signature): the convention of the Laplacian rows, see the module docstring."""

    def __init__(self, subdivisions, factor_pos, factor_nor, factor_lap, laplacian='mean-v'):
        super().__init__()
        self.subdivisions = subdivisions
        self.laplacian, self._lap_mode = laplacian, laplacian_code(laplacian)
        self.factor_pos, self.factor_nor, self.factor_lap = factor_pos, factor_nor, factor_lap
        self.register_buffer('ico_faces', torch.from_numpy(geometry.get_ico_faces(subdivisions)))
        nbr = torch.from_numpy(geometry.vertex_neighbours(subdivisions).copy())
        valid = nbr >= 0
        self.register_buffer('nbr_idx', nbr.clamp_min(0))
        self.register_buffer('nbr_w', valid.float() / valid.sum(1, keepdim=True).float())
        self.last_loss_mse = self.last_loss_cos = self.last_loss_lap = self.last_loss_total = 0

    def _hip_path(self, inputs, target):
        """HIP kernels for ROCm fp32 tensors of the expected shapes."""
        if _NO_HIP_LOSS or not (inputs.is_cuda and target.is_cuda) or inputs.dtype != torch.float32 or target.dtype != torch.float32:
            return False
        n = 2 ** self.subdivisions
        if inputs.dim() != 4 or tuple(inputs.shape[1:]) != (3, 5 * n, 2 * n):
            return False
        if tuple(target.shape) != (inputs.shape[0], 9, 10 * n * n + 2):
            return False
        return True

    def forward(self, inputs, target):
        if self._hip_path(inputs, target):
            loss, terms = _P2PLossFn.apply(inputs, target, self.subdivisions, float(self.factor_pos), float(self.factor_nor),
                                           float(self.factor_lap), self._lap_mode)
            self.last_loss_mse, self.last_loss_cos, self.last_loss_lap = terms[0], terms[1], terms[2]
            self.last_loss_total = terms[3]
            return loss
        v = grid_to_vertices(inputs, self.subdivisions)
        tgt = target.transpose(1, 2)
        l_pos = torch.nn.functional.mse_loss(v, tgt[:, :, :3])
        # The normal and Laplacian terms are evaluated (and reported) even when their factor is 0, as the reference
        # does (losses.py:54,57,74-80); a zero-weighted term contributes exactly zero gradient, so it is evaluated
        # without recording a backward graph.
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.factor_nor != 0):
            normals = compute_vertex_normals(v, self.ico_faces)
            l_nor = torch.mean(1 - torch.nn.functional.cosine_similarity(normals, tgt[:, :, 3:6], dim=2))
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.factor_lap != 0):
            lap = compute_laplacian_batch(v, self.nbr_idx, self.nbr_w, self.laplacian)
            l_lap = torch.nn.functional.mse_loss(lap, tgt[:, :, 6:9])
        loss = self.factor_pos * l_pos + self.factor_nor * l_nor + self.factor_lap * l_lap
        self.last_loss_mse, self.last_loss_cos, self.last_loss_lap = l_pos.detach(), l_nor.detach(), l_lap.detach()
        self.last_loss_total = loss.detach()
        return loss

    def get_last_losses(self):
        return float(self.last_loss_mse), self.last_loss_cos, self.last_loss_lap, float(self.last_loss_total)


class Point2Mesh_Loss(torch.nn.Module):
    """Mean squared distance of the output's vertices (grid pixels, then the two pole means) to a reference SURFACE:
    point_to_mesh_distance(grid_to_vertices(inputs), ref_vertices, ref_faces)[0].mean() -- the number the reference reports at
    test time (ico_utils.py:26-44, metrics.compute_distance), averaged over the batch, as a differentiable reconstruction term:
    vertices may slide along the target surface instead of being tied to target vertex i as in Point2Point_Loss.  Not in the
    reference (it has no surface loss); a stand-alone module, not part of Trainer / build_criterion.  Surface_Loss below is the
    criterion(output, target) form for training: both directions of the distance plus shape regularisers.

        forward(inputs (B, 3, 5n, 2n), ref_vertices (B, V, 3), ref_faces (F, 3)) -> scalar tensor

    ROCm fp32 tensors run on icn_point_to_mesh and, for the gradient (to inputs and / or ref_vertices), icn_point_to_mesh_bwd.
    Cost: the forward is a brute-force search, P * F triangle tests per mesh (2.1e8 at I5); the backward is O(1) geometry per
    point plus P * V integer compares per mesh.  Measured on an MI355X at I5 / batch 36 (10 242 points against 20 480 triangles
    per mesh, HIP events, median of 10, profiles/point_to_mesh_bwd.txt): k_point_to_mesh 15.1 ms, the two backward kernels
    1.05 ms together, the whole term forward + backward 16.5 ms, beside a training step of 6.3 ms (python bench.py, same
    batch) -- 2.6 training steps' worth per evaluation, nearly all of it the forward search.
    search='grid' replaces that search by an exact grid-accelerated one (icn_point_to_mesh_grid; same value and gradients bit for
    bit).  Same machine and sizes, both searches alternating in one process (profiles/point_to_mesh_grid.txt): with the output
    near its target (rms distance 0.01) the forward takes 0.46 ms (index build 0.14 + query 0.33) against 14.6 ms and the whole
    term 1.8 ms against 15.9 ms, a third of a training step; against a different shape (rms 0.06) 2.3 ms against 15.4 ms, the term
    3.7 ms.  Far from the surface (Gaussian cloud, rms 0.75) it is 1.8 x SLOWER than 'brute' (28.2 against 15.5 ms): an untrained
    network's output may be such a cloud, so start with 'brute' or a point-to-point term if the output is nowhere near the surface."""

    def __init__(self, subdivisions, search='brute'):
        super().__init__()
        from .metrics import _check_search
        _check_search(search)
        self.subdivisions = subdivisions
        self.search = search
        self.last_loss_total = 0

    def forward(self, inputs, ref_vertices, ref_faces):
        from .metrics import point_to_mesh_distance
        n = 2 ** self.subdivisions
        if inputs.dim() != 4 or tuple(inputs.shape[1:]) != (3, 5 * n, 2 * n):
            raise ValueError('Point2Mesh_Loss: expected inputs (B, 3, %d, %d), got %s' % (5 * n, 2 * n, tuple(inputs.shape)))
        dist, _, _ = point_to_mesh_distance(grid_to_vertices(inputs, self.subdivisions), ref_vertices, ref_faces,
                                            search=self.search)
        loss = dist.mean()
        self.last_loss_total = loss.detach()
        return loss

    def get_last_losses(self):
        """(the loss, 0, 0, the loss): position-like term, no normal / Laplacian term, total -- the tuple of Point2Point_Loss."""
        return float(self.last_loss_total), 0, 0, float(self.last_loss_total)


class _MeshRegFn(torch.autograd.Function):
    """Mesh_Regularizer on the HIP path (icn_mesh_reg_* in include/icn.h): one kernel evaluates the three terms; the gradient is
    one gather kernel, preceded by a small per-vertex pass when the smoothness term has a weight."""

    @staticmethod
    def forward(ctx, inputs, r, f_edge, f_ncons, f_smooth, edge_length):
        L = _lib.api()
        B = inputs.shape[0]
        grid = inputs.permute(0, 2, 3, 1).contiguous()            # (B, P, 3); free for channels_last
        terms = torch.empty(4, dtype=torch.float32, device=inputs.device)
        ws = _lib.workspace(L.icn_mesh_reg_workspace_floats(B, r), inputs.device, torch.float32)
        with torch.cuda.device(inputs.device):
            L.icn_mesh_reg_fwd(grid.data_ptr(), B, r, f_edge, f_ncons, f_smooth, edge_length, terms.data_ptr(), ws.data_ptr(),
                               _lib.stream())

        ctx.save_for_backward(grid)
        ctx.cfg = (B, r, f_edge, f_ncons, f_smooth, edge_length)
        total = terms[3].clone()
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gtotal, _gterms):
        B, r, f_edge, f_ncons, f_smooth, edge_length = ctx.cfg
        L = _lib.api()
        grid, = ctx.saved_tensors
        dgrid = torch.empty_like(grid)
        up = gtotal.contiguous().to(torch.float32)
        ws = None
        if f_smooth != 0:
            ws = _lib.workspace(L.icn_mesh_reg_bwd_workspace_floats(B, r), grid.device, torch.float32)
        with torch.cuda.device(grid.device):
            L.icn_mesh_reg_bwd(grid.data_ptr(), up.data_ptr(), B, r, f_edge, f_ncons, f_smooth, edge_length, dgrid.data_ptr(),
                               ws.data_ptr() if ws is not None else None, _lib.stream())
        return dgrid.permute(0, 3, 1, 2), None, None, None, None, None


def _check_factors(who, **factors):
    for name, f in factors.items():
        if isinstance(f, bool) or not isinstance(f, (int, float)) or not math.isfinite(f):
            raise ValueError('%s: %s must be a finite number, got %r' % (who, name, f))


def _check_subdivisions(who, subdivisions):
    if isinstance(subdivisions, bool) or not isinstance(subdivisions, int) or not 0 <= subdivisions <= 10:
        raise ValueError('%s: subdivisions must be an integer in [0, 10], got %r' % (who, subdivisions))


class Mesh_Regularizer(torch.nn.Module):
    """Shape regularisers of the output mesh on the static icosahedral topology (V = 10 * 4^r + 2 vertices = grid pixels then the
    two pole means, E = 30 * 4^r edges); not in the reference.

        forward(inputs (B, 3, 5n, 2n)) -> factor_edge * T_e + factor_ncons * T_n + factor_smooth * T_s

        T_e = 1 / (B E)   sum_b sum_{(i,j) in E} (|v_i - v_j| - edge_length)^2     edge_length = 0: |v_i - v_j|^2 without a square root;
                          edge_length > 0: an edge with |v_i - v_j| <= 1e-12 contributes edge_length^2 and a zero gradient
        T_n = 1 / (B E)   sum_b sum_edges 1/2 |n^_F0 - n^_F1|^2 over the two faces of each edge, n_F = (v_b - v_a) x (v_c - v_a),
                          n^ = n / max(|n|, 1e-12): 1 - cos of the dihedral angle, in the difference form (in fp32 its gradient is
                          several times more accurate than that of 1 - n^ . n^ on smooth meshes); a face whose clamp is active
                          passes no gradient through its normal
        T_s = 1 / (3 B V) sum_b sum_i |mean(ring_i) - v_i|^2                        (uniform umbrella operator)

    All three are evaluated and reported whatever their factors (last_edge / last_ncons / last_smooth / last_total: device tensors,
    no .item() until get_last_losses()).  ROCm fp32 tensors of the expected shape run on icn_mesh_reg_fwd / icn_mesh_reg_bwd (gather
    kernels over the library's edge stencil table, no atomics, bit-identical run to run); ICN_NO_HIP_LOSS=1, CPU tensors and other
    dtypes take the torch formulation of the same definitions over the same table (_lib.table_vertex_stencils)."""

    def __init__(self, subdivisions, factor_edge, factor_ncons, factor_smooth, edge_length=0.0):
        super().__init__()
        _check_subdivisions('Mesh_Regularizer', subdivisions)
        _check_factors('Mesh_Regularizer', factor_edge=factor_edge, factor_ncons=factor_ncons, factor_smooth=factor_smooth,
                       edge_length=edge_length)
        if edge_length < 0:
            raise ValueError('Mesh_Regularizer: edge_length must be >= 0, got %r' % (edge_length,))
        self.subdivisions = subdivisions
        self.factor_edge, self.factor_ncons, self.factor_smooth = factor_edge, factor_ncons, factor_smooth
        self.edge_length = float(edge_length)
        vs = torch.from_numpy(_lib.table_vertex_stencils(subdivisions)).long()           # (V, 6, 3) of (p, q, x)
        p, valid = vs[:, :, 0], vs[:, :, 0] >= 0
        k = valid.sum(1, keepdim=True)
        slot = torch.arange(6)[None, :].expand_as(p)
        p_prev = torch.gather(p, 1, (slot - 1) % k)                                      # p of slot f - 1, wrapping at the valence
        i = torch.arange(p.shape[0])[:, None].expand_as(p)
        once = valid & (i < p)                                                            # every undirected edge from its lower end
        # edge (i, p) and the third vertices of its two faces: slot f = (i, p, q), slot f - 1 = (i, p_prev, p)
        self.register_buffer('edge_idx', torch.stack((i[once], p[once], vs[:, :, 1][once], p_prev[once]), dim=0))
        self.register_buffer('nbr_idx', p.clamp_min(0))
        self.register_buffer('nbr_w', valid.double() / k.double())                       # cast to the input's dtype at use
        self.last_edge = self.last_ncons = self.last_smooth = self.last_total = 0

    def _hip_path(self, inputs):
        return not _NO_HIP_LOSS and inputs.is_cuda and inputs.dtype == torch.float32

    @staticmethod
    def _face_normal(a, b):
        """a x b with every product rounded on its own.  torch.cross (and a contracting compiler) evaluates a component as
        fma(a_y, b_z, -(a_z b_y)), which makes a x a the rounding error of one product: about 6e-8 |a|^2 in fp32, far above the
        1e-12 clamp, so a face with two coincident vertices would count with a random unit normal.  Here a x a is exactly 0."""
        ax, ay, az = a.unbind(-1)
        bx, by, bz = b.unbind(-1)
        return torch.stack((ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx), dim=-1)

    @staticmethod
    def _unit(nrm):
        """n / max(|n|, 1e-12); where the clamp is active the value is kept and no gradient passes."""
        d2 = (nrm * nrm).sum(-1, keepdim=True)
        ok = d2.sqrt() > 1e-12
        return torch.where(ok, nrm / torch.where(ok, d2, torch.ones_like(d2)).sqrt(), nrm.detach() / 1e-12)

    def terms(self, v):
        """(T_e, T_n, T_s) of vertices v (B, V, 3) in torch; a term whose factor is 0 records no backward graph."""
        grad = torch.is_grad_enabled()
        vi, vp, vq, vm = (torch.index_select(v, 1, self.edge_idx[c]) for c in range(4))
        with torch.set_grad_enabled(grad and self.factor_edge != 0):
            d2 = ((vi - vp) ** 2).sum(-1)
            if self.edge_length > 0:
                ok = d2 > 1e-24
                length = torch.where(ok, d2, torch.ones_like(d2)).sqrt()
                t_e = torch.where(ok, (length - self.edge_length) ** 2, torch.full_like(d2, self.edge_length ** 2)).mean()
            else:
                t_e = d2.mean()
        with torch.set_grad_enabled(grad and self.factor_ncons != 0):
            n0 = self._unit(self._face_normal(vp - vi, vq - vi))
            n1 = self._unit(self._face_normal(vm - vi, vp - vi))
            t_n = 0.5 * ((n0 - n1) ** 2).sum(-1).mean()
        with torch.set_grad_enabled(grad and self.factor_smooth != 0):
            ring = torch.index_select(v, 1, self.nbr_idx.reshape(-1)).view(v.shape[0], -1, 6, 3)
            u = (ring * self.nbr_w.to(v.dtype)[None, :, :, None]).sum(2) - v
            t_s = (u ** 2).mean()
        return t_e, t_n, t_s

    def forward(self, inputs):
        n = 2 ** self.subdivisions
        if inputs.dim() != 4 or tuple(inputs.shape[1:]) != (3, 5 * n, 2 * n) or inputs.shape[0] < 1:
            raise ValueError('Mesh_Regularizer: expected inputs (B, 3, %d, %d), got %s' % (5 * n, 2 * n, tuple(inputs.shape)))
        if self._hip_path(inputs):
            loss, terms = _MeshRegFn.apply(inputs, self.subdivisions, float(self.factor_edge), float(self.factor_ncons),
                                           float(self.factor_smooth), self.edge_length)
            self.last_edge, self.last_ncons, self.last_smooth, self.last_total = terms[0], terms[1], terms[2], terms[3]
            return loss
        t_e, t_n, t_s = self.terms(grid_to_vertices(inputs, self.subdivisions))
        loss = self.factor_edge * t_e + self.factor_ncons * t_n + self.factor_smooth * t_s
        self.last_edge, self.last_ncons, self.last_smooth = t_e.detach(), t_n.detach(), t_s.detach()
        self.last_total = loss.detach()
        return loss

    def get_last_losses(self):
        """(edge, normal consistency, smoothness, weighted total) as floats."""
        return float(self.last_edge), float(self.last_ncons), float(self.last_smooth), float(self.last_total)


class Surface_Loss(torch.nn.Module):
    """Surface training criterion, criterion(output (B, 3, 5n, 2n), target (B, 9, V)) as Trainer.step calls it; not in the reference.

        out = grid_to_vertices(output);  ref = target[:, 0:3] as (B, V, 3)              (the target mesh shares the ico faces)
        loss = factor_p2m * mean(p2m(out, ref, ico_faces)) + factor_m2p * mean(p2m(ref, out, ico_faces)) + Mesh_Regularizer(output)

    with p2m = metrics.point_to_mesh_distance.  The first term alone (Point2Mesh_Loss) is zero for an output bunched on one patch of the
    target; the second, the reference's vertices against the OUTPUT surface (differentiable in the output through the mesh-vertex
    gradient of icn_point_to_mesh_bwd), pulls the output surface over all of the target; the regularisers keep a mesh that may slide
    along the surface from folding.  A term with factor 0 is still evaluated for reporting, without a backward graph.  The face
    list is an int32 buffer validated at construction, so forward + backward never synchronise the host (the public
    point_to_mesh_distance reads faces.min() back on every call).  search: 'brute' / 'grid' as in point_to_mesh_distance (same
    values bit for bit; see Point2Mesh_Loss for when 'grid' pays).
    Cost on an MI355X at I5 / batch 36: NOT MEASURED yet -- `python tools/time_mesh_regularizer.py 10` records the regulariser kernels
    beside icn_p2p_loss_fwd / _bwd, the torch formulation on the device and this whole term for both searches into
    profiles/mesh_regularizer.txt; whether the HIP regulariser beats the torch formulation on the device is therefore not known.

    samples = S > 0 measures surfaces instead of vertices: with samples = 0 (the default: vertices only) the interior of a
    face is never tested, so a surface that cuts a corner or bulges between its vertices goes unseen.  With S > 0 every forward draws
    u = torch.rand((2, B, S, 3), generator=g, device=output.device) once, g a torch.Generator made on the first forward's device and
    seeded with sample_seed (this draw order is the contract: a caller can rebuild the uniforms), and
        l_p2m = mean p2m(sample_points(out mesh, u[0]), ref mesh)     gradient to the output through icn_mesh_sample_bwd
        l_m2p = mean p2m(sample_points(ref mesh, u[1]), out mesh)     gradient through the mesh-vertex gradient of icn_point_to_mesh_bwd
    with sampling.sample_points (area-weighted, HIP kernels icn_mesh_sample_*).  The regularisers, the reporting, the zero-factor rule
    and the absence of host synchronisation are unchanged.  The loss is then a stochastic estimate: two forwards differ.  The
    generator is a plain attribute: its state is not in state_dict, so a resumed run starts again from sample_seed.
    Cost of samples > 0 on an MI355X at I5 / batch 36 with S = 10 242 (HIP events, median of 10, profiles/surface_samples.txt, from
    `python tools/time_surface_samples.py 10`): the three forward kernels 0.07 ms together (area 0.008, scan 0.033, search + point
    0.028), the backward 1.04 ms, nearly all of it k_msample_bwd_vertex (S V integer compares per mesh).  The torch formulation on the
    device takes 0.36 ms forward and 1.04 ms forward + backward against 0.09 / 1.24 ms on the HIP path: the HIP forward is 4 x
    faster, the fixed-order HIP backward is what buys run-to-run identity and is no faster than torch's atomic index_put.  This whole
    term, forward + backward: samples = 0 33.2 ms ('brute') / 2.8 ms ('grid'); samples = S 38.4 / 4.2 ms, beside a training step of
    6.6 ms.

    factor_normal != 0 (needs samples > 0: a vertex has no face of its own; ValueError otherwise) adds what the distances cannot
    see -- a sheet that lies on the target but faces the wrong way, wrinkles across the surface below the sample scale -- from the
    faces the forward already has, with fna = metrics.face_normal_agreement (1 - n^_a . n^_b per sample, or 1 - |n^_a . n^_b| with
    normal_oriented=False; an unresolved face gives 1 and no gradient):
        l_n = 0.5 * ( mean fna(out mesh, face of sample_points(out mesh, u[0]),   ref mesh, closest ref face of those points)
                    + mean fna(ref mesh, face of sample_points(ref mesh, u[1]),   out mesh, closest out face of those points) )
        loss += factor_normal * l_n                                      gradient to the output through icn_face_normal_agree_bwd
    The term draws no random numbers of its own (the draw order above stays the contract) and never synchronises the host; last_normal
    holds l_n (a device tensor; 0 while the term is off) and get_last_losses() keeps its five-tuple.  With factor_normal = 0 (the
    default) the term is not evaluated: the same kernels, the same draw, the same results bit for bit.
    Cost of factor_normal != 0 on an MI355X at I5 / batch 36 with S = 10 242 (HIP events, median of 10, profiles/normal_agreement.txt,
    from `python tools/time_normal_agreement.py 10`): k_fnormal_agree 0.02 ms, k_fnormal_agree_bwd_record 0.02 ms,
    k_fnormal_agree_bwd_vertex 2.04 ms per side (2 S V integer compares per mesh: twice the sampler's scatter).  The torch formulation on
    the device takes 0.69 ms forward and 1.89 ms forward + backward of both sides against 0.05 / 4.33 ms on the HIP path: the HIP forward
    is 15 x faster, the fixed-order HIP backward is again what buys run-to-run identity and does not beat torch's atomic index_put.
    This whole term, forward + backward, samples = S: 38.2 -> 42.3 ms ('brute'), 4.2 -> 8.4 ms ('grid') with the normal term (the
    output's side of both halves: two record passes and two scatters).

    factor_volume / factor_area != 0 hold the two global measures of the output mesh to the target's.  The three regularisers are
    local and share one global failure -- they shrink the mesh (the umbrella operator is the textbook case) -- which nothing else
    here measures.  With (area, vol) = metrics.mesh_area_volume(., ico_faces) (every ico mesh is closed and wound outwards, so the
    signed volume is well defined and positive):
        l_vol = mean_b (vol(out) - vol(ref))^2;   l_area = mean_b (area(out) - area(ref))^2       absolute: the data are normalised
        loss += factor_volume * l_vol + factor_area * l_area                                       to the unit sphere
    The gradient to the output runs through icn_mesh_measure_bwd, one gather over the vertex -> corner incidence table of the ico
    faces (a buffer built at construction), O(F) per mesh, fixed order, no atomics.  The terms need no samples (they work with
    samples = 0), draw no random numbers and never synchronise the host; a term is evaluated only when its factor is non-zero.
    last_volume / last_area hold l_vol / l_area (device tensors; 0 while the term is off), get_last_losses() keeps its five-tuple.
    With both factors 0 (the default) nothing new is launched and the loss is bit for bit what it was.
    Cost on an MI355X at I5 / batch 36 (HIP events, median of 10, profiles/mesh_measure.txt, from `python tools/time_mesh_measure.py
    10`): k_mesh_measure_face 0.008 ms, k_mesh_measure_finish 0.007 ms, k_mesh_measure_bwd 0.017 ms -- the incidence gather
    against 1.04 ms (k_msample_bwd_vertex) and 2.04 ms per side (k_fnormal_agree_bwd_vertex) for the record scatters above, whose callers
    could move to the same table.  Through autograd the HIP path takes 0.04 ms forward and 0.34 ms forward + backward (the three kernels
    are 0.03 ms of that; the rest is launch and autograd overhead on the host, 0.22 ms in another run) against 0.43 / 3.3 ms (1.87 ms in
    that other run) for the torch formulation on the device: 10 x either way; building the table on demand instead adds 0.10 - 0.13 ms
    per backward.  This whole term, forward + backward, search='grid': samples = 0 6.07 -> 6.14 ms, samples = 10 242 7.83 -> 7.98 ms with
    both factors.

    factor_willmore != 0 adds the remedy for the cause: a smoothness measure that is geometric -- weighted by the triangles, not by
    vertex valence -- and that does not shrink the mesh.  W = metrics.willmore_energy(out, ico_faces) is the discrete integral of
    H^2 from the cotangent Laplace-Beltrami operator (metrics.cotangent_laplacian): invariant under scaling, rotation and
    translation, 4 pi for a sphere of any radius, so it cannot be lowered by shrinking and does not drag vertices tangentially the
    way the umbrella of factor_smooth does:
        loss += factor_willmore * mean_b W(out mesh)
    The gradient to the output runs through icn_mesh_willmore_bwd over the same incidence table (the ico_vf_* buffers).  The term
    needs no samples, draws no random numbers and never synchronises the host; last_willmore holds mean_b W (a device tensor; 0
    while the term is off), get_last_losses() keeps its five-tuple and state_dict is unchanged.  With the factor 0 (the default)
    nothing new is launched and the loss is bit for bit what it was.
    Cost on an MI355X at I5 / batch 36 (HIP events, median of 10, profiles/mesh_curvature.txt, from `python
    tools/time_mesh_curvature.py 10`): k_mesh_cotlap_fwd 0.018 ms, k_mesh_willmore_finish 0.007 ms, k_mesh_willmore_upstream
    0.007 ms, k_mesh_cotlap_bwd 0.026 ms.  Through autograd the HIP path takes 0.04 ms forward and 0.21 ms forward + backward
    (the four kernels are 0.06 ms of that; the rest is launch and autograd overhead on the host) against 0.80 / 2.6 ms for the
    torch formulation on the device: 21 x and 13 x, and here the fixed-order HIP backward does beat torch's atomic index_add.
    Building the table on entry instead adds 0.12 ms.  This whole term, forward + backward, search='grid': samples = 0
    6.01 -> 6.01 ms, samples = 10 242 7.75 -> 7.81 ms with the factor.

    factor_gauss != 0 compares the CURVATURE of the output with that of the target, which none of the terms above does: W penalises
    mean curvature everywhere, pulls every mesh towards the round sphere and erases the target's own creases and bumps as readily as
    noise.  Output and target share the ico faces, so the comparison is vertex by vertex.  With defect = metrics.angle_defect(.,
    ico_faces), the angle defect 2 pi - sum theta, which is the Gaussian curvature integrated over a vertex's cell:
        l_gauss = mean_b sum_i (defect(out)_i - defect(ref)_i)^2;   loss += factor_gauss * l_gauss
    The term holds the output to the TARGET's features where W flattens them.  The defect is intrinsic and dimensionless, so the
    term is invariant under scaling of either mesh and shrinking cannot lower it; by Gauss-Bonnet sum_i defect_i = 4 pi on both
    sides, so the differences sum to zero and cannot all be driven one way.  defect(ref) is computed without a graph; both sides
    gather over the ico_vf_* buffers; the gradient to the output runs through icn_mesh_angle_defect_bwd.  The kernels compute in
    double from the fp32 vertices and round once (in fp32 the defect of an I5 mesh, 1e-3, carries an error of 1e-6).  The term needs
    no samples, draws no random numbers and never synchronises the host; last_gauss holds l_gauss (a device tensor; 0 while the
    term is off), get_last_losses() keeps its five-tuple and state_dict is unchanged.  With the factor 0 (the default) nothing new
    is launched and the loss is bit for bit what it was.
    Cost on an MI355X at I5 / batch 36 (HIP events, median of 10, profiles/mesh_gauss.txt, from `python tools/time_mesh_gauss.py
    10`): k_mesh_angle_defect_fwd 0.024 ms, k_mesh_angle_defect_bwd 0.026 ms, beside k_mesh_cotlap_fwd 0.017 ms and
    k_mesh_cotlap_bwd 0.024 ms in the same run -- the same gathers in fp32 -- so the double arithmetic costs 1.4 x forward (six
    atan2 per vertex) and 1.06 x backward (1.04 - 1.05 in two other runs).  Through autograd the HIP path takes 0.03 ms forward and
    0.23 ms forward + backward (the rest is launch and autograd overhead on the host: 0.11 and 0.18 ms in the other runs) against
    0.80 / 2.31 ms for the float64 torch formulation on the device: 25 x and 10 x.  Building the table on entry instead adds
    0.11 ms.  This whole term, forward + backward, search='grid': samples = 0 6.00 -> 6.13 ms, samples = 10 242 7.81 -> 7.92 ms
    with the factor (two forwards and one backward)."""

    def __init__(self, subdivisions, factor_p2m=1.0, factor_m2p=1.0, factor_edge=0.0, factor_ncons=0.0, factor_smooth=0.0,
                 edge_length=0.0, search='brute', samples=0, sample_seed=0, factor_normal=0.0, normal_oriented=True,
                 factor_volume=0.0, factor_area=0.0, factor_willmore=0.0, factor_gauss=0.0):
        super().__init__()
        from .metrics import _check_search
        _check_search(search)
        _check_subdivisions('Surface_Loss', subdivisions)
        _check_factors('Surface_Loss', factor_p2m=factor_p2m, factor_m2p=factor_m2p, factor_normal=factor_normal,
                       factor_volume=factor_volume, factor_area=factor_area, factor_willmore=factor_willmore, factor_gauss=factor_gauss)
        if isinstance(samples, bool) or not isinstance(samples, int) or samples < 0:
            raise ValueError('%s: samples must be a non-negative integer, got %r' % (type(self).__name__, samples))
        if isinstance(sample_seed, bool) or not isinstance(sample_seed, int):
            raise ValueError('%s: sample_seed must be an integer, got %r' % (type(self).__name__, sample_seed))
        if factor_normal != 0 and samples == 0:
            raise ValueError('%s: factor_normal needs samples > 0 (a vertex has no face of its own), got samples = 0'
                             % type(self).__name__)
        if not isinstance(normal_oriented, bool):
            raise ValueError('%s: normal_oriented must be a bool, got %r' % (type(self).__name__, normal_oriented))
        self.samples, self.sample_seed, self._sample_generator = samples, sample_seed, None
        self.factor_normal, self.normal_oriented = factor_normal, normal_oriented
        self.factor_volume, self.factor_area = factor_volume, factor_area
        self.factor_willmore, self.factor_gauss = factor_willmore, factor_gauss
        self.subdivisions, self.search = subdivisions, search
        self.factor_p2m, self.factor_m2p = factor_p2m, factor_m2p
        self.regularizer = Mesh_Regularizer(subdivisions, factor_edge, factor_ncons, factor_smooth, edge_length)
        faces = geometry.get_ico_faces(subdivisions)
        nv = geometry.num_vertices(subdivisions)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.min() < 0 or faces.max() >= nv:
            raise ValueError('Surface_Loss: the face table does not index %d vertices' % nv)
        self.register_buffer('ico_faces', torch.from_numpy(faces).to(torch.int32))
        # vertex -> corner incidence table of the ico faces (the gather of icn_mesh_measure_bwd and icn_mesh_willmore_*); derived from the subdivisions, so
        # not part of state_dict
        from .metrics import vertex_face_table
        offsets, corners = vertex_face_table(self.ico_faces, nv)
        self.register_buffer('ico_vf_offsets', offsets, persistent=False)
        self.register_buffer('ico_vf_corners', corners, persistent=False)
        self.last_p2m = self.last_m2p = self.last_reg = self.last_loss_total = self.last_normal = 0
        self.last_volume = self.last_area = self.last_willmore = self.last_gauss = 0

    def _vertex_face_table(self, device):
        """The incidence table of the ico faces (the ico_vf_* buffers) on `device`."""
        return tuple(t if t.device == device else t.to(device) for t in (self.ico_vf_offsets, self.ico_vf_corners))

    def _draw_uniforms(self, B, device):
        """The (2, B, S, 3) uniforms of one forward, from the generator seeded with sample_seed on the first forward's device."""
        if self._sample_generator is None or self._sample_generator.device != device:
            self._sample_generator = torch.Generator(device=device)
            self._sample_generator.manual_seed(self.sample_seed)
        return torch.rand((2, B, self.samples, 3), generator=self._sample_generator, device=device)

    def forward(self, output, target):
        from .metrics import _point_to_mesh_unchecked
        from .sampling import _sample_points_unchecked
        n = 2 ** self.subdivisions
        if output.dim() != 4 or tuple(output.shape[1:]) != (3, 5 * n, 2 * n) or output.shape[0] < 1:
            raise ValueError('Surface_Loss: expected output (B, 3, %d, %d), got %s' % (5 * n, 2 * n, tuple(output.shape)))
        if tuple(target.shape) != (output.shape[0], 9, 10 * n * n + 2):
            raise ValueError('Surface_Loss: expected target (%d, 9, %d), got %s'
                             % (output.shape[0], 10 * n * n + 2, tuple(target.shape)))
        grad = torch.is_grad_enabled()
        out = grid_to_vertices(output, self.subdivisions)
        ref = target[:, 0:3].transpose(1, 2).contiguous().to(out.dtype)
        faces = self.ico_faces if self.ico_faces.device == out.device else self.ico_faces.to(out.device)
        p_out, p_ref = out, ref                                               # the points measured against the other surface
        u = self._draw_uniforms(out.shape[0], out.device) if self.samples else None
        normal = self.factor_normal != 0                                      # (then samples > 0: checked at construction)
        with torch.set_grad_enabled(grad and self.factor_p2m != 0):
            if u is not None:
                p_out, on_out, _ = _sample_points_unchecked(out, faces, u[0])
            l_p2m, near_ref, _ = _point_to_mesh_unchecked(p_out, ref, faces, self.search)
            l_p2m = l_p2m.mean()
        with torch.set_grad_enabled(grad and self.factor_m2p != 0):
            if u is not None:
                p_ref, on_ref, _ = _sample_points_unchecked(ref, faces, u[1])
            l_m2p, near_out, _ = _point_to_mesh_unchecked(p_ref, out, faces, self.search)
            l_m2p = l_m2p.mean()
        l_reg = self.regularizer(output)
        loss = self.factor_p2m * l_p2m + self.factor_m2p * l_m2p + l_reg
        if normal:                                                            # no further draw: the faces the forward already has
            from .metrics import _face_normal_agreement_unchecked as fna
            l_n = 0.5 * (fna(out, faces, on_out, ref, faces, near_ref, self.normal_oriented).mean()
                         + fna(ref, faces, on_ref, out, faces, near_out, self.normal_oriented).mean())
            loss = loss + self.factor_normal * l_n
            self.last_normal = l_n.detach()
        else:
            self.last_normal = 0                                              # (not a tensor: the default path launches nothing new)
        self.last_volume = self.last_area = 0
        if self.factor_volume != 0 or self.factor_area != 0:                  # one forward serves both; a backward term per factor
            from .metrics import _mesh_area_volume_unchecked
            table = self._vertex_face_table(out.device)
            area_out, vol_out = _mesh_area_volume_unchecked(out, faces, table)
            with torch.no_grad():
                area_ref, vol_ref = _mesh_area_volume_unchecked(ref, faces)
            if self.factor_volume != 0:
                l_vol = ((vol_out - vol_ref) ** 2).mean()
                loss = loss + self.factor_volume * l_vol
                self.last_volume = l_vol.detach()
            if self.factor_area != 0:
                l_area = ((area_out - area_ref) ** 2).mean()
                loss = loss + self.factor_area * l_area
                self.last_area = l_area.detach()
        self.last_willmore = 0
        if self.factor_willmore != 0:
            from .metrics import _willmore_energy_unchecked
            table = self._vertex_face_table(out.device)
            l_w = _willmore_energy_unchecked(out, faces, table).mean()
            loss = loss + self.factor_willmore * l_w
            self.last_willmore = l_w.detach()
        self.last_gauss = 0
        if self.factor_gauss != 0:
            from .metrics import _angle_defect_unchecked
            table = self._vertex_face_table(out.device)
            defect_out = _angle_defect_unchecked(out, faces, table)
            with torch.no_grad():
                defect_ref = _angle_defect_unchecked(ref, faces, table)
            l_g = ((defect_out - defect_ref) ** 2).sum(1).mean()
            loss = loss + self.factor_gauss * l_g
            self.last_gauss = l_g.detach()
        self.last_p2m, self.last_m2p, self.last_reg = l_p2m.detach(), l_m2p.detach(), l_reg.detach()
        self.last_loss_total = loss.detach()
        return loss

    def get_last_losses(self):
        """(p2m, m2p, regulariser, 0., total) -- the five-tuple of P2P_Loss."""
        return float(self.last_p2m), float(self.last_m2p), float(self.last_reg), 0., float(self.last_loss_total)


class KLD_Loss(torch.nn.Module):
    """mean_b( -0.5 * mean_d(1 + logvar - mu^2 - exp(logvar)) )   -- reference losses.py:87-118."""

    def forward(self, output, target):
        _, mu, logvar = output
        if self.factor_kl:
            self.loss = kld(mu, logvar)
        else:
            self.loss = torch.tensor(0.)
        return self.loss

    def get_last_losses(self):
        return 0, 0, 0, 0, -float(self.loss.detach())

    def get_factor(self):
        return self.factor_kl

    def update_factor(self, epoch, factor_step_size, factor_gamma):
        if epoch % factor_step_size == 0:
            self.factor_kl *= factor_gamma


class P2P_Loss(Point2Point_Loss):
    """reference losses.py:121-130."""

    def get_last_losses(self):
        return (float(self.last_loss_mse), float(self.last_loss_cos), float(self.last_loss_lap), 0.,
                float(self.last_loss_total))


class P2PKLD_Loss(P2P_Loss, KLD_Loss):
    """reconstruction + factor_kl * KLD   -- reference losses.py:132-145."""

    def __init__(self, subdivisions, factor_pos, factor_nor, factor_lap, factor_kl, laplacian='mean-v'):
        super().__init__(subdivisions, factor_pos, factor_nor, factor_lap, laplacian=laplacian)
        self.factor_kl = factor_kl

    def forward(self, output, target):
        self.kld_loss = KLD_Loss.forward(self, output, target)
        self.recons_loss = P2P_Loss.forward(self, output[0], target)
        self.loss = self.recons_loss + self.factor_kl * self.kld_loss
        return self.loss

    def get_last_losses(self):
        return float(self.recons_loss.detach()), 0, 0, -float(self.kld_loss.detach()), float(self.loss.detach())


class SurfaceKLD_Loss(Surface_Loss, KLD_Loss):
    """Surface_Loss of the reconstruction + factor_kl * KLD, for (recon, mu, logvar) outputs -- as P2PKLD_Loss is to P2P_Loss."""

    def __init__(self, subdivisions, factor_p2m=1.0, factor_m2p=1.0, factor_edge=0.0, factor_ncons=0.0, factor_smooth=0.0,
                 edge_length=0.0, search='brute', factor_kl=1.0, samples=0, sample_seed=0, factor_normal=0.0, normal_oriented=True,
                 factor_volume=0.0, factor_area=0.0, factor_willmore=0.0, factor_gauss=0.0):
        super().__init__(subdivisions, factor_p2m, factor_m2p, factor_edge, factor_ncons, factor_smooth, edge_length, search,
                         samples=samples, sample_seed=sample_seed, factor_normal=factor_normal, normal_oriented=normal_oriented,
                         factor_volume=factor_volume, factor_area=factor_area, factor_willmore=factor_willmore,
                         factor_gauss=factor_gauss)
        _check_factors('SurfaceKLD_Loss', factor_kl=factor_kl)
        self.factor_kl = factor_kl

    def forward(self, output, target):
        self.kld_loss = KLD_Loss.forward(self, output, target)
        self.recons_loss = Surface_Loss.forward(self, output[0], target)
        self.loss = self.recons_loss + self.factor_kl * self.kld_loss
        return self.loss

    def get_last_losses(self):
        return float(self.recons_loss.detach()), 0, 0, -float(self.kld_loss.detach()), float(self.loss.detach())


class Chamfer_Loss(torch.nn.Module):
    """Chamfer training criterion, criterion(output (B, 3, 5n, 2n), target (B, 9, V)) as Trainer.step calls it: the CustomChamfer loss
    the reference names beside its others (run.py:629) and does not ship.

        out = grid_to_vertices(output);  ref = target[:, 0:3] as (B, V, 3)
        loss = mean_b ( w1 mean_i sided(out, ref)_i + w2 mean_j sided(ref, out)_j )          = mean_b metrics.chamfer_distance(out, ref)

    with metrics.sided_distance, the squared distance of every point to its nearest point in the other set (HIP kernels
    icn_nearest_points / icn_nearest_points_bwd on ROCm fp32 tensors, fixed summation order: bit-identical run to run).  Both terms
    are differentiable in the output: the first through the points, the second through the chosen targets.
    samples = S > 0 measures surfaces instead of vertices, as in Surface_Loss and with its sampler and its draw order: every forward
    draws u = torch.rand((2, B, S, 3), generator=g, device=output.device), g seeded with sample_seed on the first forward's device,
    and the two point sets are sampling.sample_points(out mesh, u[0]) and sampling.sample_points(ref mesh, u[1]) over the ico faces
    (gradient to the output through icn_mesh_sample_bwd).  The loss is then a stochastic estimate.  The face list is a buffer
    validated at construction and nothing is read back: forward + backward never synchronise the host.
    Cost on an MI355X: profiles/nearest_neighbour.txt (tools/time_nearest.py)."""

    _draw_uniforms = Surface_Loss._draw_uniforms

    def __init__(self, subdivisions, samples=0, sample_seed=0, w1=1.0, w2=1.0):
        super().__init__()
        who = type(self).__name__
        _check_subdivisions(who, subdivisions)
        _check_factors(who, w1=w1, w2=w2)
        if isinstance(samples, bool) or not isinstance(samples, int) or samples < 0:
            raise ValueError('%s: samples must be a non-negative integer, got %r' % (who, samples))
        if isinstance(sample_seed, bool) or not isinstance(sample_seed, int):
            raise ValueError('%s: sample_seed must be an integer, got %r' % (who, sample_seed))
        self.subdivisions, self.w1, self.w2 = subdivisions, w1, w2
        self.samples, self.sample_seed, self._sample_generator = samples, sample_seed, None
        faces = geometry.get_ico_faces(subdivisions)
        nv = geometry.num_vertices(subdivisions)
        if faces.ndim != 2 or faces.shape[1] != 3 or faces.min() < 0 or faces.max() >= nv:
            raise ValueError('%s: the face table does not index %d vertices' % (who, nv))
        self.register_buffer('ico_faces', torch.from_numpy(faces).to(torch.int32))
        self.last_chamfer = 0

    def forward(self, output, target):
        from .metrics import _chamfer_unchecked
        from .sampling import _sample_points_unchecked
        n, who = 2 ** self.subdivisions, type(self).__name__
        if output.dim() != 4 or tuple(output.shape[1:]) != (3, 5 * n, 2 * n) or output.shape[0] < 1:
            raise ValueError('%s: expected output (B, 3, %d, %d), got %s' % (who, 5 * n, 2 * n, tuple(output.shape)))
        if tuple(target.shape) != (output.shape[0], 9, 10 * n * n + 2):
            raise ValueError('%s: expected target (%d, 9, %d), got %s' % (who, output.shape[0], 10 * n * n + 2, tuple(target.shape)))
        out = grid_to_vertices(output, self.subdivisions)
        ref = target[:, 0:3].transpose(1, 2).contiguous().to(out.dtype)
        if self.samples:
            faces = self.ico_faces if self.ico_faces.device == out.device else self.ico_faces.to(out.device)
            u = self._draw_uniforms(out.shape[0], out.device)
            out, ref = _sample_points_unchecked(out, faces, u[0])[0], _sample_points_unchecked(ref, faces, u[1])[0]
        loss = _chamfer_unchecked(out, ref, self.w1, self.w2).mean()
        self.last_chamfer = loss.detach()
        return loss

    def get_last_losses(self):
        """(chamfer, 0, 0, 0., total) -- the five-tuple of P2P_Loss."""
        return float(self.last_chamfer), 0, 0, 0., float(self.last_chamfer)


class ChamferKLD_Loss(Chamfer_Loss, KLD_Loss):
    """Chamfer_Loss of the reconstruction + factor_kl * KLD, for (recon, mu, logvar) outputs -- as SurfaceKLD_Loss is to Surface_Loss."""

    def __init__(self, subdivisions, samples=0, sample_seed=0, w1=1.0, w2=1.0, factor_kl=1.0):
        super().__init__(subdivisions, samples=samples, sample_seed=sample_seed, w1=w1, w2=w2)
        _check_factors('ChamferKLD_Loss', factor_kl=factor_kl)
        self.factor_kl = factor_kl

    def forward(self, output, target):
        self.kld_loss = KLD_Loss.forward(self, output, target)
        self.recons_loss = Chamfer_Loss.forward(self, output[0], target)
        self.loss = self.recons_loss + self.factor_kl * self.kld_loss
        return self.loss

    def get_last_losses(self):
        return float(self.recons_loss.detach()), 0, 0, -float(self.kld_loss.detach()), float(self.loss.detach())
