"""Test helper: element-wise error bars against the float64 oracle, and the operator calls of a production training step.

A rel-L2 over a whole tensor dilutes a single wrong element by the norm of everything else: at 6 M elements one output pixel
that misses one tap's term moves the rel-L2 by ~1e-7.  The bar here is per element instead.  For an operator that is linear in
each of its inputs with NON-NEGATIVE structural coefficients (the convolution, the pair, the upsample, the upconv composite, the
head's 1x1 part) the same oracle evaluated on |x|, |w|, |b| with |gy| gives, per output element,

    A = sum over the element's terms of |term|          (y, dx, dw and db alike; the pole mean and the 0.5 of the upsample are >= 0)

and any fp32 evaluation of the sum -- in any order, with or without the three-way bf16 split -- is off by at most a small
multiple of u * A, u = 2^-24.  The bar is  rho = |got - ref| / (u * A) <= bar(output)  for every element (RHO_MAX, or
RHO_MAX_WGRAD for parameter gradients), and got == 0 exactly where A == 0.  A dropped term of typical size |term| ~ A / n is
flagged as long as 1 / (n u) >= 4 bar (`detectable`).

BatchNorm is not of that form (a square root, a division, the ReLU mask); its bars are per channel: the statistics against
u * mean|x| resp. u * var, y and dx as per-channel rel-L2 in units of u, dgamma / dbeta element-wise against sum |g| (|xhat| + 1).
Its statistics are summed in double over row chunks (icn_bn.hip), the per-element arithmetic is a handful of fp32 operations.

Off the production shapes (tests/test_gpu_streaming_edges.py) BatchNorm, KLD and the reparameterisation are held element by element
too, against condition-aware bounds A (bn_edge_measure, kld_oracle, reparam_oracle); each comes with an fp32 restatement of the
kernel's arithmetic in numpy, which tests/test_error_bounds.py keeps well inside the bar before any GPU run.  Adam's restatement
(adam_reference_f32) is exact: the kernel is compared with it bit for bit.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
RHO_MAX = 16.0              # element-wise bar of y and dx (and the head's y), every case, both arithmetics
RHO_MAX_WGRAD = 2.0         # the same for weight / bias / BatchNorm-affine gradients: their sums (up to B P = 368 640 terms) are
                            # split into many partial sums, the measured maxima are 0.6; 16 would leave one dropped term of the
                            # longest sums (1 / (n u) = 45) without a 4x margin (`detectable`)
BN_STAT_MAX = 8.0           # |mean - ref| / (u mean|x|),  |var - ref| / (u var),  running statistics likewise
BN_RL2_MAX = 8.0            # per-channel rel-L2 of y and dx, in units of u
BN_EPS = 1e-5


# ---- linear operators ----------------------------------------------------------------------------------------------------------
def rho(got, ref, A):
    """max over elements of |got - ref| / (u A); inf if an element with A == 0 is not exactly zero."""
    got = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float64)
    ref = np.asarray(ref.detach().cpu() if torch.is_tensor(ref) else ref, dtype=np.float64)
    A = np.asarray(A.detach().cpu() if torch.is_tensor(A) else A, dtype=np.float64)
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    if not np.isfinite(got).all():
        return math.inf
    zero = A == 0
    if (got[zero] != 0).any():
        return math.inf
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / (U * A[~zero])).max())


def oracle_and_bound(op, inputs, gys):
    """op(**tensors) -> tuple of outputs, linear in each tensor with non-negative structural coefficients.
    inputs: dict name -> (fp32 CPU tensor or None, needs gradient).  Returns (ref, A): dicts with 'y<i>' and 'd<name>' for every
    input that needs a gradient; ref in float64 from the fp32 values, A = the same on absolute values (float32 is enough for a
    sum of non-negative terms: its own error is ~1e-6 of A)."""
    def run(dtype, absolute):
        ts = {}
        for k, (t, grad) in inputs.items():
            if t is None:
                ts[k] = None
                continue
            v = t.to(dtype)
            ts[k] = (v.abs() if absolute else v).requires_grad_(grad)
        ys = op(**ts)
        torch.autograd.backward(ys, [(g.abs() if absolute else g).to(dtype) for g in gys])
        out = {'y%d' % i: y.detach() for i, y in enumerate(ys)}
        for k, (t, grad) in inputs.items():
            if grad:
                out['d' + k] = ts[k].grad
        return out
    return run(torch.float64, False), run(torch.float32, True)


def n_terms(kind, r, stride, cin, cout, B):
    """Terms behind one output element of a production call, per output: y = 7 Cin, dx = 7 Cout (a pair: both branches, 14 Cout),
    dw = B P_out (one term per output pixel).  The upconv composite reads two coarse values per tap (y: 14 Cin) and a coarse pixel
    reaches the gradients of up to 7 fine pixels (dx: 49 per output channel of either branch).  The 1x1 head: Cin, Cout, B P."""
    n_out = 2 ** (r + 1) if kind == 'upconv' else 2 ** r // stride
    P_out = 10 * n_out * n_out
    if kind == 'head':
        return {'y': cin, 'dx': cout, 'dw': B * P_out}
    branches = 2 if kind in ('pair', 'upconv') else 1
    return {'y': (14 if kind == 'upconv' else 7) * cin, 'dx': (49 if kind == 'upconv' else 7) * branches * cout, 'dw': B * P_out}


def bar(key):
    """RHO_MAX_WGRAD for parameter gradients ('dw*', 'db*', 'dgamma*', 'dbeta*'), RHO_MAX for everything else."""
    return RHO_MAX_WGRAD if key.startswith(('dw', 'db', 'dgamma', 'dbeta')) else RHO_MAX


def detectable(n, key):
    """A single dropped term of typical size (A / n) in output `key` is flagged at 4 x its bar."""
    return 1.0 / (n * U) >= 4.0 * bar(key)


# ---- BatchNorm (+ residual) + ReLU in float64 ----------------------------------------------------------------------------------
def bn_stats(x):
    """x (M, C) float64 -> (mean, biased var) per channel."""
    m = x.mean(0)
    return m, ((x - m) ** 2).mean(0)


def bn_relu_ref(xs, gammas, betas, gy, mask=None, stats=None):
    """relu(sum_i bn_i(x_i)) with batch statistics, and its backward under `mask` (the GPU's own ReLU pattern, y_gpu > 0; the
    float64 forward's own pattern when None).  xs, gy: (M, C) float64.  Returns dict: y, the pre-activation z, per input i
    mean_i, var_i, dx_i, dgamma_i, dbeta_i and the bounds A_dgamma_i, A_dbeta_i."""
    stats = stats or [bn_stats(x) for x in xs]
    z, xhs = 0, []
    for x, g_, b_, (m, v) in zip(xs, gammas, betas, stats):
        xh = (x - m) / torch.sqrt(v + BN_EPS)
        xhs.append(xh)
        z = z + g_ * xh + b_
    y = torch.relu(z)
    g = gy * (mask if mask is not None else (z > 0)).to(gy.dtype)
    out = {'y': y, 'z': z}
    for i, (x, g_, (m, v), xh) in enumerate(zip(xs, gammas, stats, xhs)):
        inv = 1.0 / torch.sqrt(v + BN_EPS)
        out['mean%d' % i], out['var%d' % i] = m, v
        out['dbeta%d' % i], out['dgamma%d' % i] = g.sum(0), (g * xh).sum(0)
        out['A_dbeta%d' % i], out['A_dgamma%d' % i] = g.abs().sum(0), (g.abs() * (xh.abs() + 1)).sum(0)
        out['dx%d' % i] = g_ * inv * (g - g.mean(0) - xh * (g * xh).mean(0))
    return out


def per_channel_rel_l2(got, ref):
    """(M, C) -> (C,) ||got - ref|| / ||ref|| per channel, in units of u (a channel whose reference is all zero must be zero)."""
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    num, den = (got - ref).norm(dim=0), ref.norm(dim=0)
    return torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, math.inf, 0.0)) / U


def stat_rho(got, ref, scale):
    """per channel |got - ref| / (u scale)."""
    return (torch.as_tensor(got).double() - ref).abs() / (U * scale)


# ---- the operator calls of one training step, read off the models ---------------------------------------------------------------
CONFIGS = (('ico2ico', 5, 36), ('ico2ico_vae', 5, 36), ('ico2ico', 6, 8))   # bench.py's headline, --config vae and i6


def step_calls(name, R, B):
    """Every operator call a Trainer step of models.<name> at level R and batch B makes, as tuples:
    ('stem' | 'single' | 'pair' | 'upconv' | 'head', r, stride, cin, cout, B) for the convolution-type operators (r: level of the
    input; 'upconv': the decoder block's upsample + conv pair over the coarse tensor), ('bn', M, C, dual) for every fused
    BatchNorm + ReLU, ('p2p', R, B) for the loss."""
    from geniconet_amd import models
    from geniconet_amd.models import BasicIcoS2SDownBlock, BasicIcoS2SUpBlock
    net = getattr(models, name)(models.default_params(name, subdivisions=R))
    rows = lambda r: B * 10 * 4 ** r
    stem = net.encoder[0]
    calls = [('stem', stem.subdivisions, stem.stride, stem.in_features, stem.out_features, B),
             ('bn', rows(stem.subdivisions), stem.out_features, False)]
    for m in net.modules():
        if isinstance(m, BasicIcoS2SDownBlock):
            c0, c1 = m.conv00, m.conv01
            calls += [('pair', c0.subdivisions, c0.stride, c0.in_features, c0.out_features, B),
                      ('bn', rows(c1.subdivisions), c1.out_features, False),
                      ('single', c1.subdivisions, c1.stride, c1.in_features, c1.out_features, B),
                      ('bn', rows(c1.subdivisions), c1.out_features, True)]
        elif isinstance(m, BasicIcoS2SUpBlock):
            up, c1 = m.upsample00, m.conv01
            calls += [('upconv', up.subdivisions, 1, m.conv00.in_features, m.conv00.out_features, B),
                      ('bn', rows(c1.subdivisions), c1.out_features, False),
                      ('single', c1.subdivisions, c1.stride, c1.in_features, c1.out_features, B),
                      ('bn', rows(c1.subdivisions), c1.out_features, True)]
    if name == 'ico2ico_vae':                   # mu / logvar: one pair (their BatchNorm(512) runs on the torch module)
        c = net.mu[0]
        calls.append(('pair', c.subdivisions, c.stride, c.in_features, c.out_features, B))
    head = (net.enc2icoConv if name == 'ico2ico' else net.final_layer)[0]
    calls += [('head', R, 1, head.in_channels, head.out_channels, B), ('p2p', R, B)]
    return calls


def production_cases():
    """step_calls of every configuration in CONFIGS, de-duplicated, in first-seen order."""
    seen = []
    for cfg in CONFIGS:
        for c in step_calls(*cfg):
            if c not in seen:
                seen.append(c)
    return seen


# ---- GPU entry points shared by the parity tests ---------------------------------------------------------------------------------
CL = torch.channels_last


def _rows4(t):
    """(M, C) CPU rows -> (1, C, M, 1) channels_last on the device: the kernels' (M, C) rows."""
    M, C = t.shape
    return t.t().reshape(1, C, M, 1).cuda().contiguous(memory_format=CL)


def _bn_modules(gammas, betas, rms, rvs, momentum, train):
    bns = []
    for g_, b_, m_, v_ in zip(gammas, betas, rms, rvs):
        bn = torch.nn.BatchNorm2d(g_.numel(), momentum=momentum).cuda().train(train)
        with torch.no_grad():
            bn.weight.copy_(g_); bn.bias.copy_(b_); bn.running_mean.copy_(m_); bn.running_var.copy_(v_)
        bns.append(bn)
    return bns


def bn_run(xs, gammas, betas, rm0, rv0, gy, momentum):
    """fused.bn_relu / bn_add_relu on (1, C, M, 1) channels_last tensors, i.e. the kernels' (M, C) rows."""
    from geniconet_amd import fused
    M, C = gy.shape
    bns = _bn_modules(gammas, betas, rm0, rv0, momentum, True)
    ins = [_rows4(x).requires_grad_() for x in xs]
    assert fused.can_fuse(ins[0], *bns)
    y = fused.bn_relu(ins[0], bns[0]) if len(xs) == 1 else fused.bn_add_relu(ins[0], bns[0], ins[1], bns[1])
    y.backward(_rows4(gy))
    rows = lambda t: t.detach().reshape(C, M).t().cpu().double()
    out = {'y': rows(y)}
    for i, (a, bn) in enumerate(zip(ins, bns)):
        out['dx%d' % i] = rows(a.grad)
        out['dgamma%d' % i], out['dbeta%d' % i] = bn.weight.grad.cpu().double(), bn.bias.grad.cpu().double()
        out['rm%d' % i], out['rv%d' % i] = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    return out


def bn_run_eval(xs, gammas, betas, rms, rvs):
    """fused.bn_relu_eval / bn_add_relu_eval (running statistics, inference forward) on the same rows -> y (M, C) float64."""
    from geniconet_amd import fused
    M, C = xs[0].shape
    bns = _bn_modules(gammas, betas, rms, rvs, 0.1, False)
    ins = [_rows4(x) for x in xs]
    with torch.no_grad():
        assert fused.can_fuse_eval(ins[0], *bns)
        y = fused.bn_relu_eval(ins[0], bns[0]) if len(xs) == 1 else fused.bn_add_relu_eval(ins[0], bns[0], ins[1], bns[1])
    return y.reshape(C, M).t().cpu().double()


def head_run(x, w, b, gy, x_grad=True):
    """fused.head on Sequential(Conv2d(Cin, Cout, 1), Tanh), forward + backward.  x (B, Cin, H, W), w (Cout, Cin, 1), b (Cout),
    gy (B, Cout, H, W), fp32 on the CPU.  Returns y0, dw0, db0 and, when the input takes a gradient, dx."""
    from geniconet_amd import fused
    cout, cin = w.shape[:2]
    xg = x.cuda().contiguous(memory_format=CL).requires_grad_(x_grad)
    seq = torch.nn.Sequential(torch.nn.Conv2d(cin, cout, kernel_size=1), torch.nn.Tanh()).cuda()
    seq[0].weight, seq[0].bias = torch.nn.Parameter(w.cuda()[..., None]), torch.nn.Parameter(b.cuda())
    assert fused.can_fuse_head(xg, seq)
    y = fused.head(xg, seq)
    y.backward(gy.cuda())
    out = {'y0': y.detach().cpu()}
    if x_grad:
        out['dx'] = xg.grad.cpu()
    out['dw0'] = seq[0].weight.grad.detach().cpu().reshape(w.shape)
    out['db0'] = seq[0].bias.grad.detach().cpu()
    return out


def head_chunking(M):
    """(chunks, rows per chunk) of the head's backward: head_chunks() and launch_head_bwd of icn_bn.hip."""
    chunks = min(1024, -(-M // 64))
    return chunks, -(-M // chunks)


def head_oracle(x, w, b, gy, y_got, x_grad=True):
    """(ref, A) of the head for eb.rho: y0 = tanh(z) in float64 with A = (1 - t^2) A_lin + |t| (A_lin: the 1x1 convolution on
    absolute values); dx, dw0, db0 through the linear oracle with the kernel's own dz = gy (1 - y_got^2)."""
    y = y_got.double()
    gz = gy.double() * (1 - y * y)
    op = lambda x, w0, b0: (torch.nn.functional.conv2d(x, w0[..., None], b0),)
    ref, A = oracle_and_bound(op, {'x': (x, x_grad), 'w0': (w, True), 'b0': (b, True)}, [gz])
    t = torch.tanh(ref['y0'])
    ref['y0'], A['y0'] = t, (1 - t * t) * A['y0'].double() + t.abs()
    return ref, A


# ---- BatchNorm (+ residual) + ReLU off the production shapes, element by element ---------------------------------------------
# k_bn_partial splits the rows into bn_chunks(M) chunks and strides 256 / (C / 4) row stripes over each: at C = 4 / 8 / 32 the
# stripes (256 / 128 / 32) times the rows per iteration exceed a chunk's rows, at C = 1024 there is one stripe, and above
# M = 64 * 512 the rounded-up chunk length leaves trailing chunks without rows.
BN_FAMILIES = ((0.3, 2.0), (1e3, 1e-2), (-300.0, 1.0))      # (mean, std) of the first input; the second: mean -0.3, std 1
BN_EDGE_C = (4, 8, 32, 64, 1024)                            # 64: the control (a production width)
BN_EDGE_M = (7, 63, 64, 65, 257, 1000)
BN_EMPTY_CHUNK_M = 33469                                    # 512 chunks of 66 rows: chunks 508..511 start past the last row
BN_FLIP_SHARE_MAX = 0.01


def bn_chunking(M):
    """(chunks, rows per chunk) of the BatchNorm passes: bn_chunks() and the launchers of icn_bn.hip."""
    chunks = min(512, -(-M // 64))
    return chunks, -(-M // chunks)


def bn_edge_cases():
    """(M, C, dual, family): every C against every M with the family and the form cycling, so that every C sees each family and
    both forms; M = 33 469 with C = 4 / 32; and four more for the extreme stripe counts under the ill-conditioned families."""
    cases = []
    for ci, C in enumerate(BN_EDGE_C):
        for mi, M in enumerate(BN_EDGE_M):
            cases.append((M, C, (mi + ci) % 2 == 1, (mi + ci // 2 + mi // 3) % 3))
    cases += [(BN_EMPTY_CHUNK_M, 4, False, 0), (BN_EMPTY_CHUNK_M, 4, True, 1), (BN_EMPTY_CHUNK_M, 4, False, 2),
              (BN_EMPTY_CHUNK_M, 32, True, 0), (BN_EMPTY_CHUNK_M, 32, False, 1), (BN_EMPTY_CHUNK_M, 32, True, 2)]
    cases += [(1000, 4, True, 1), (1000, 1024, False, 2), (65, 8, True, 2), (257, 1024, True, 1)]
    assert len(set(cases)) == len(cases)
    return cases


def bn_edge_inputs(case):
    """Seeded fp32 inputs of a bn_edge_cases() entry: xs, gammas in U(0.5, 1.5), betas in U(-0.5, 0.5), gy ~ N(0, 1)."""
    import zlib
    M, C, dual, fam = case
    g = torch.Generator().manual_seed(zlib.crc32(repr(case).encode()))
    mean, std = BN_FAMILIES[fam]
    xs = [torch.randn(M, C, generator=g) * std + mean]
    if dual:
        xs.append(torch.randn(M, C, generator=g) - 0.3)
    gammas = [torch.rand(C, generator=g) + 0.5 for _ in xs]
    betas = [torch.rand(C, generator=g) - 0.5 for _ in xs]
    gy = torch.randn(M, C, generator=g)
    return xs, gammas, betas, gy


def bn_restatement_f32(xs, gammas, betas, gy):
    """The arithmetic of icn_bn.hip in numpy, operation by operation: statistics summed in double from the fp32 differences to
    row 0 and rounded to fp32 (k_bn_partial<0/3>, k_bn_finalize_fwd at momentum 1 from zero running statistics), then the fp32
    expressions of bn_pre4 and of the backward (sums of g and g xhat in double, rounded to fp32).  Without FMA contraction and
    without the chunking: what it says about a bound is its size, not the last bit.  Returns the dict of bn_run plus 'z'."""
    f, M = np.float32, gy.shape[0]
    xs, gammas, betas = [x.numpy() for x in xs], [g.numpy() for g in gammas], [b.numpy() for b in betas]
    gy = gy.numpy()
    out, st = {}, []
    for i, x in enumerate(xs):
        d = (x - x[0]).astype(np.float64)
        ms = d.sum(0) / M
        mean = x[0].astype(np.float64) + ms
        var = np.maximum((d * d).sum(0) / M - ms * ms, 0.0)
        st.append((mean.astype(f), (1.0 / np.sqrt(var + np.float64(f(BN_EPS)))).astype(f)))
        out['rm%d' % i], out['rv%d' % i] = mean.astype(f), (var * M / (M - 1)).astype(f)
    v = None
    for x, (m, inv), g_, b_ in zip(xs, st, gammas, betas):
        t = (x - m) * (inv * g_) + b_
        v = t if v is None else v + t
    out['z'], out['y'] = v, np.maximum(v, f(0))
    g = np.where(v > 0, gy, f(0))
    gd = g.astype(np.float64)
    inv_m = f(1.0) / f(M)
    for i, (x, (m, inv), g_) in enumerate(zip(xs, st, gammas)):
        xh = (x - m) * inv
        sg, sgx = gd.sum(0).astype(f), (gd * xh.astype(np.float64)).sum(0).astype(f)
        out['dbeta%d' % i], out['dgamma%d' % i] = sg, sgx
        out['dx%d' % i] = g_ * inv * (g - sg * inv_m - xh * (sgx * inv_m))
    return {k: torch.from_numpy(np.ascontiguousarray(a)).double() for k, a in out.items()}


def bn_edge_measure(got, xs, gammas, betas, gy):
    """Element-wise rho of a bn_run-style result against float64 on the fp32 inputs, the backward under got's own ReLU pattern.
    With inv = 1 / sqrt(var + eps), ax = |x| + mean_c |x| (the scale of the mean's error: |mean| would be too small for a channel
    whose mean is near zero), ah = ax inv, ag = |g|:
        y (and 'z' if present)  A = sum_i |gamma_i| inv_i ax_i + |beta_i|
        dx_i                    A = |gamma| inv (ag + mean(ag) + ah mean(ag |xhat|) + |xhat| mean(ag ah))
        dgamma_i, dbeta_i       A = sum ag ah,  sum ag
        mean_i, var_i           A = mean |x|,  var        (momentum-1 running statistics: the mean, the unbiased variance)
    Also 'flip_share', the share of elements whose ReLU pattern differs from float64's, and 'flips_inside': every one of them has
    |z_ref| <= RHO_MAX u A_y."""
    M = gy.shape[0]
    x64, g64, b64 = [x.double() for x in xs], [g.double() for g in gammas], [b.double() for b in betas]
    mask = got['y'] > 0
    ref = bn_relu_ref(x64, g64, b64, gy.double(), mask=mask)
    invs = [1.0 / torch.sqrt(ref['var%d' % i] + BN_EPS) for i in range(len(xs))]
    axs = [x.abs() + x.abs().mean(0) for x in x64]
    A_y = sum(g_.abs() * inv * ax + b_.abs() for g_, b_, inv, ax in zip(g64, b64, invs, axs))
    z = ref['z']
    out = {'y': rho(got['y'], ref['y'], A_y)}
    if 'z' in got:
        out['z'] = rho(got['z'], z, A_y)
    flips = mask != (z > 0)
    out['flip_share'] = float(flips.double().mean())
    out['flips_inside'] = bool((z.abs()[flips] <= RHO_MAX * U * A_y[flips]).all())
    ag = (gy.double() * mask.double()).abs()
    for i, (x, g_, inv, ax) in enumerate(zip(x64, g64, invs, axs)):
        mean, var = ref['mean%d' % i], ref['var%d' % i]
        xh, ah = ((x - mean) * inv).abs(), ax * inv
        A_dx = g_.abs() * inv * (ag + ag.mean(0) + ah * (ag * xh).mean(0) + xh * (ag * ah).mean(0))
        unb = var * M / (M - 1)
        out['dx%d' % i] = rho(got['dx%d' % i], ref['dx%d' % i], A_dx)
        out['dgamma%d' % i] = rho(got['dgamma%d' % i], ref['dgamma%d' % i], (ag * ah).sum(0))
        out['dbeta%d' % i] = rho(got['dbeta%d' % i], ref['dbeta%d' % i], ag.sum(0))
        out['mean%d' % i] = rho(got['rm%d' % i], mean, x.abs().mean(0))
        out['var%d' % i] = rho(got['rv%d' % i], unb, unb)
    return out


def bn_edge_bar(name):
    """RHO_MAX for y / z / dx, BN_STAT_MAX for the statistics and the affine gradients."""
    return RHO_MAX if name[0] in 'yz' or name.startswith('dx') else BN_STAT_MAX


def bn_eval_oracle(xs, gammas, betas, rms, rvs):
    """relu(sum_i gamma_i (x_i - rm_i) / sqrt(rv_i + eps) + beta_i) in float64 and its bound: the running statistics are inputs
    here, so the cancellation of x - rm is u (|x| + |rm|)."""
    z = A = 0
    for x, g_, b_, m_, v_ in zip(xs, gammas, betas, rms, rvs):
        x, g_, b_, m_, v_ = (t.double() for t in (x, g_, b_, m_, v_))
        inv = 1.0 / torch.sqrt(v_ + BN_EPS)
        z = z + g_ * (x - m_) * inv + b_
        A = A + g_.abs() * inv * (x.abs() + m_.abs()) + b_.abs()
    return torch.relu(z), A


# ---- KLD and the reparameterisation --------------------------------------------------------------------------------------------
# The only non-elementary step of these kernels is __expf(l): a multiply by log2(e), then the hardware exp2.  The rounding of
# the product moves the result by |l| u, the exp2 itself by about one more: relative error (|l| + 2) u.
LOG2E_F32 = np.float32(1.4426950408889634)


def expf_restatement(l):
    """float32(exp2(float32(l * log2e))) for an fp32 array."""
    t = (np.asarray(l, dtype=np.float32) * LOG2E_F32).astype(np.float32)
    with np.errstate(over='ignore'):
        return np.exp2(t.astype(np.float64)).astype(np.float32)


def kld_oracle(mu, lv, up):
    """float64 value and gradients of up * kld(mu, lv), kld = -0.5 / n sum(1 + l - m^2 - e^l), with their bounds (value: of kld)."""
    m, l = mu.double().numpy().ravel(), lv.double().numpy().ravel()
    n, w = m.size, float(up) / m.size
    e = np.exp(l)
    ref = {'value': -0.5 / n * (1 + l - m * m - e).sum(), 'dmu': w * m, 'dlogvar': 0.5 * w * (e - 1)}
    A = {'value': 0.5 / n * (1 + np.abs(l) + m * m + (np.abs(l) + 2) * e).sum(), 'dmu': np.abs(w * m),
         'dlogvar': 0.5 * abs(w) * ((np.abs(l) + 2) * e + 1)}
    return ref, A


def kld_restatement_f32(mu, lv, up):
    """k_kld_partial / k_kld_finalize / k_kld_bwd in numpy fp32 with expf_restatement: a thread's elements in grid-stride order,
    256 threads of a block in a pairwise fp32 tree, the blocks in double."""
    f = np.float32
    m, l = mu.numpy().ravel(), lv.numpy().ravel()
    n = m.size
    e = expf_restatement(l)
    term = f(1) + l - m * m - e
    threads = min(1024, -(-n // 256)) * 256
    padded = np.zeros(-(-n // threads) * threads, f)
    padded[:n] = term
    acc = np.zeros(threads, f)
    for row in padded.reshape(-1, threads):
        acc = acc + row
    blk = acc.reshape(-1, 256)
    while blk.shape[1] > 1:
        blk = blk[:, 0::2] + blk[:, 1::2]
    w = f(up) * f(1.0 / n)
    return {'value': f(blk.astype(np.float64).sum() * (-0.5 / n)), 'dmu': w * m, 'dlogvar': f(0.5) * w * (e - f(1))}


def reparam_oracle(mu, lv, eps, g):
    """float64 z = eps e^{l / 2} + mu and the gradient of logvar under the output gradient g, with their bounds."""
    m, l, e, g = (t.double().numpy().ravel() for t in (mu, lv, eps, g))
    s = np.exp(0.5 * l)
    k = np.abs(l) / 2 + 2
    return ({'z': e * s + m, 'dlogvar': g * e * 0.5 * s},
            {'z': np.abs(e) * s * k + np.abs(m), 'dlogvar': np.abs(g * e) * 0.5 * s * k})


def reparam_restatement_f32(mu, lv, eps, g):
    f = np.float32
    m, l, e, g = (t.numpy().ravel() for t in (mu, lv, eps, g))
    s = expf_restatement(f(0.5) * l)
    return {'z': e * s + m, 'dlogvar': g * e * f(0.5) * s}


KLD_EDGE_SHAPES = ((1, 1, 1, 1), (1, 5, 3, 17), (2, 8, 4, 4), (1, 257, 1, 1), (5, 13, 37, 109))   # n = 1, 255, 256, 257, 1024 * 256 + 1
KLD_FAMILIES = ('randn', 'uniform30')
KLD_UPSTREAM = 1.7


def kld_edge_inputs(shape, family):
    """Seeded fp32 mu ~ N(0, 1), logvar (0.7 randn, or uniform in [-30, 30]), eps ~ N(0, 1) and an output gradient g ~ N(0, 1)."""
    import zlib
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, family)).encode()))
    mu = torch.randn(shape, generator=g)
    lv = 0.7 * torch.randn(shape, generator=g) if family == 'randn' else torch.rand(shape, generator=g) * 60 - 30
    return mu, lv, torch.randn(shape, generator=g), torch.randn(shape, generator=g)


# ---- Adam, bit for bit ---------------------------------------------------------------------------------------------------------
def adam_reference_f32(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    """adam_one of icn_optim.hip in numpy float32, every operation rounded on its own in the kernel's order (the kernel has
    contraction off; fp32 sqrt and division are correctly rounded on the device and in numpy).  The scalars as the kernel receives
    them: step_size and bc2_sqrt computed in double as optim.Adam.step does and rounded to fp32, the rest cast from double.
    p, g, m, v: float32 arrays; returns the new (p, m, v)."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1c, b2, b2c, eps, wd = f(1.0 - beta1), f(beta2), f(1.0 - beta2), f(eps), f(wd)
    step_size, bc2_sqrt = f(lr / (1.0 - beta1 ** step)), f((1.0 - beta2 ** step) ** 0.5)
    if wd != 0:
        g = g + wd * p
    m = m + (g - m) * b1c
    v = v * b2 + b2c * g * g
    denom = np.sqrt(v) / bc2_sqrt + eps
    return p - step_size * (m / denom), m, v
