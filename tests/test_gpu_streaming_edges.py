"""The streaming kernels of every training step -- BatchNorm (+ residual) + ReLU, the head, KLD / reparameterisation, Adam -- off the
step's own shapes, element by element against float64 (Adam: bit for bit against its fp32 restatement).

fused.can_fuse / can_fuse_head admit C = 4 .. 1024, Cin = 16 .. 256, Cout <= 4 and any M; the production tests run C >= 64,
Cin = 64, Cout = 3 and row counts the chunking divides.  The cases here reach what those leave out:
  k_bn_partial   C = 4 / 8 / 32 (256 / 128 / 32 row stripes: more than a chunk has rows, the clamped loads and the skips do the
                 work), C = 1024 (one stripe), M = 33 469 (512 chunks of 66 rows, the last four without a row)
  k_head_*       every lanes-per-row instantiation, every Cout and dx == NULL, each in the fp32 pass (M >= 1024) and the
                 double one (below), M below and just past one block pass, M = 66 000
                 (1024 chunks of 65 rows, eight of them empty: k_head_reduce sums their zero partials)
  k_kld_*, k_reparam_*   n = 1, 255, 256, 257 and 1024 * 256 + 1 (the grid-stride wrap), |logvar| up to 30, special values
  k_adam         180 non-empty tensors in one call with one step count (the flush at 96), empty tensors, n % 4 tails, two step counts interleaved in one call,
                 weight decay, device scalars, and each of p, g, m, v on a 4-byte offset (the scalar path) with canaries
The bars are those of error_bounds.py: |got - ref| <= bar u A per element with the bounds A stated there, validated on the CPU by
tests/test_error_bounds.py (an fp32 restatement of each kernel stays under a quarter of RHO_MAX, half of BN_STAT_MAX).

Measured maxima of rho over all cases (MI355X | the CPU restatement), a value above half its bar is a finding:
  BatchNorm      y 2.2 | 2.6, dx 2.8 | 2.8 (bar 16); dgamma 1.0 | 1.0, dbeta 1.0 | 1.0, mean 1.1 | 1.1, var 2.4 | 2.4 (bar 8);
                 flipped ReLU share 0.22 % | 0.22 % (cap 1 %), every flip inside RHO_MAX u A_y; eval-mode y 2.7
  head           y 1.5, dx 3.5 (bar 16); dw 1.0, db 0.8 (bar 2); in the fp32 pass (M >= 1024) dw 0.35, db 0.14
  KLD            value 0.6 | 0.7, dmu 2.0 | 2.5, dlogvar 1.8 | 2.3;  reparam z 1.1 | 1.2, dlogvar 1.4 | 1.3 (bar 16)
  Adam           p, m, v equal the restatement in every bit, every case
The finding: k_head_bwd summed dw and db in fp32, and the cases of M <= 17 rows gave dw 2.2 - 3.1 against the bar of 2 (ten cases;
M = 63 / 65: 1.8 - 2.0; every term carries the roundings of y^2, 1 - y^2, dy (.) and g x, which only long sums average out).  Below
1024 rows its sums are in double since, as BatchNorm's are, and dw is rounded once: 1.0 at most.  From 1024 rows on the pass is
unchanged (fp32: dw 0.3 at M = 1024, 0.04 at M = 66 000), so a training step computes what it did.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import error_bounds as eb

pytestmark = pytest.mark.gpu
CL = torch.channels_last


def _cid(c):
    return '_'.join(str(v) for v in c)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# ---- BatchNorm (+ residual) + ReLU --------------------------------------------------------------------------------------------
def test_the_large_m_really_leaves_trailing_chunks_empty():
    """From the library's own formulas (bn_chunks / head_chunks, rows = ceil(M / chunks)): a later change of the chunking cannot
    silently stop covering the chunks that start past the last row."""
    chunks, rows = eb.bn_chunking(eb.BN_EMPTY_CHUNK_M)
    assert (chunks, rows) == (512, 66) and -(-eb.BN_EMPTY_CHUNK_M // rows) == 508
    chunks, rows = eb.head_chunking(HEAD_EMPTY_CHUNK_M)
    assert (chunks, rows) == (1024, 65) and -(-HEAD_EMPTY_CHUNK_M // rows) == 1016
    from geniconet_amd import _lib
    L = _lib.api()
    for C in (4, 32):                                       # the workspace the library sizes: chunks x 4 sums x C doubles
        assert L.icn_bn_workspace_floats(eb.BN_EMPTY_CHUNK_M, C) == 512 * 4 * C * 2
    assert L.icn_head_workspace_floats(HEAD_EMPTY_CHUNK_M, 16) == 1024 * 4 * (16 + 4)
    for M in HEAD_F64_ROWS - 1, HEAD_F64_ROWS:              # double partials below HEAD_F64_ROWS rows, float from there on
        assert L.icn_head_workspace_floats(M, 64) == 16 * 4 * (64 + 4) * (2 if M < HEAD_F64_ROWS else 1)


@pytest.mark.parametrize('case', eb.bn_edge_cases(), ids=_cid)
def test_batchnorm_relu_element_by_element(case):
    M, C, dual, fam = case
    xs, gammas, betas, gy = eb.bn_edge_inputs(case)
    zeros = [torch.zeros(C)] * len(xs)
    got = eb.bn_run(xs, gammas, betas, zeros, zeros, gy, 1.0)
    m = eb.bn_edge_measure(got, xs, gammas, betas, gy)
    print('\nBN-EDGE %s %s' % (_cid(case), ' '.join('%s=%.3g' % kv for kv in m.items())))
    assert m.pop('flips_inside')
    assert m.pop('flip_share') <= eb.BN_FLIP_SHARE_MAX
    for name, v in m.items():
        assert v <= eb.bn_edge_bar(name), (name, v)


@pytest.mark.parametrize('C', eb.BN_EDGE_C)
@pytest.mark.parametrize('dual', [False, True], ids=['single', 'dual'])
def test_batchnorm_relu_eval_element_by_element(C, dual):
    M = 257
    g = _gen('bn-eval', C, dual)
    k = 2 if dual else 1
    xs = [torch.randn(M, C, generator=g) * 2 + 0.3 for _ in range(k)]
    gammas = [torch.rand(C, generator=g) + 0.5 for _ in range(k)]
    betas = [torch.rand(C, generator=g) - 0.5 for _ in range(k)]
    rms = [torch.randn(C, generator=g) * 0.1 + 0.3 for _ in range(k)]
    rvs = [(torch.rand(C, generator=g) + 0.5) * 4 for _ in range(k)]
    y = eb.bn_run_eval(xs, gammas, betas, rms, rvs)
    ref, A = eb.bn_eval_oracle(xs, gammas, betas, rms, rvs)
    r = eb.rho(y, ref, A)
    print('\nBN-EVAL C=%d dual=%d y=%.3g' % (C, dual, r))
    assert r <= eb.RHO_MAX


# ---- head ---------------------------------------------------------------------------------------------------------------------
HEAD_EMPTY_CHUNK_M = 66000
HEAD_CHANNELS = [(cin, 3) for cin in (16, 32, 64, 128, 256)] + [(cin, cout) for cin in (16, 256) for cout in (1, 2, 4)]
HEAD_CASES = [(cin, cout, M, True) for cin, cout in HEAD_CHANNELS for M in (1, 1024 // cin - 1, 1024 // cin + 1, 1000)]
HEAD_CASES += [(16, 3, HEAD_EMPTY_CHUNK_M, True), (32, 2, 1000, False)]        # ..., False: the input takes no gradient, dx == NULL
HEAD_F64_ROWS = 1024                  # k_head_bwd sums dw / db in double below that many rows, in fp32 from there on: both sides
HEAD_CASES += [(64, 3, HEAD_F64_ROWS - 1, True), (64, 3, HEAD_F64_ROWS, True), (16, 4, HEAD_F64_ROWS, True)]
# ... and the fp32 pass, the one a training step runs, for every width, every Cout and dx == NULL too (M = 1025: one row past 16 chunks)
HEAD_CASES += [(cin, cout, HEAD_F64_ROWS + 1, True) for cin, cout in HEAD_CHANNELS if (cin, cout) != (64, 3)]
HEAD_CASES += [(128, 1, HEAD_F64_ROWS + 1, False)]


@pytest.mark.parametrize('case', HEAD_CASES, ids=_cid)
def test_head_element_by_element(case):
    """256 / LPR = 1024 / Cin rows make one block pass.  Reference and bars: those of the production head
    (test_gpu_production_parity.py), through the same code."""
    cin, cout, M, x_grad = case
    g = _gen('head', case)
    bound = 1.0 / cin ** 0.5
    x = torch.randn(1, cin, M, 1, generator=g)
    w = (torch.rand(cout, cin, 1, generator=g) * 2 - 1) * bound
    b = (torch.rand(cout, generator=g) * 2 - 1) * bound
    gy = torch.randn(1, cout, M, 1, generator=g)
    got = eb.head_run(x, w, b, gy, x_grad)
    assert ('dx' in got) == x_grad
    ref, A = eb.head_oracle(x, w, b, gy, got['y0'], x_grad)
    assert set(ref) == set(got)
    m = {k: eb.rho(got[k], ref[k], A[k]) for k in ref}
    print('\nHEAD-EDGE %s %s' % (_cid(case), ' '.join('%s=%.3g' % kv for kv in m.items())))
    for k, v in m.items():
        assert v <= eb.bar(k), (k, v)


# ---- KLD and the reparameterisation --------------------------------------------------------------------------------------------
def _layouts(ts, fmt):
    return [t.cuda().contiguous(memory_format=CL) if fmt == 'channels_last' else t.cuda().contiguous() for t in ts]


def _kld_gpu(mu, lv, fmt):
    from geniconet_amd import losses
    m, l = (t.requires_grad_() for t in _layouts((mu, lv), fmt))
    val = losses.kld(m, l)
    assert val.grad_fn is not None and type(val.grad_fn).__name__.startswith('_KLDFn')
    (val * eb.KLD_UPSTREAM).backward()
    return {'value': val.detach().cpu().numpy().reshape(()), 'dmu': m.grad.cpu().numpy().ravel(),
            'dlogvar': l.grad.cpu().numpy().ravel()}


def _reparam_gpu(mu, lv, eps, g, fmt):
    from geniconet_amd import fused
    m, l, e, gz = _layouts((mu, lv, eps, g), fmt)
    m.requires_grad_()
    l.requires_grad_()
    z = fused._ReparamFn.apply(m, l, e)
    z.backward(gz)
    return {'z': z.detach().cpu().numpy().ravel(), 'dlogvar': l.grad.cpu().numpy().ravel(), 'dmu': m.grad.cpu().numpy().ravel()}


@pytest.mark.parametrize('fmt', ['contiguous', 'channels_last'])
@pytest.mark.parametrize('family', eb.KLD_FAMILIES)
@pytest.mark.parametrize('shape', eb.KLD_EDGE_SHAPES, ids=_cid)
def test_kld_and_reparam_element_by_element(shape, family, fmt):
    mu, lv, eps, g = eb.kld_edge_inputs(shape, family)
    got = _kld_gpu(mu, lv, fmt)
    ref, A = eb.kld_oracle(mu, lv, float(np.float32(eb.KLD_UPSTREAM)))
    m = {'kld_' + k: eb.rho(got[k], np.asarray(ref[k]), np.asarray(A[k])) for k in ref}
    again = _kld_gpu(mu, lv, fmt)
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k         # deterministic: equal bits
    got = _reparam_gpu(mu, lv, eps, g, fmt)
    ref, A = eb.reparam_oracle(mu, lv, eps, g)
    m.update({'reparam_' + k: eb.rho(got[k], ref[k], A[k]) for k in ref})
    assert np.array_equal(got['dmu'].view(np.int32), g.numpy().ravel().view(np.int32))   # dmu = g, bit for bit
    again = _reparam_gpu(mu, lv, eps, g, fmt)
    for k in got:
        assert np.array_equal(got[k].view(np.int32), again[k].view(np.int32)), k
    print('\nKLD-EDGE %s %s %s %s' % (_cid(shape), family, fmt, ' '.join('%s=%.3g' % kv for kv in m.items())))
    for k, v in m.items():
        assert v <= eb.RHO_MAX, (k, v)


def _classes(a):
    """NaN -> 'nan', +-inf -> '+inf' / '-inf', finite -> the value itself."""
    a = np.asarray(a, dtype=np.float32).ravel()
    return ['nan' if np.isnan(v) else ('+inf' if v > 0 else '-inf') if np.isinf(v) else float(v) for v in a]


def test_kld_and_reparam_special_values():
    """logvar in {-inf, +inf, NaN} against eps in {0, 1}, padded with logvar = 0 to n = 8 (1 / n, the small integer mu and the
    gradient 2 make every finite result exact): every output is of the class of torch's fp32 CPU evaluation of the reference
    expression, and equal to it where finite.  The KLD value once per special value alone, the gradients with all of them."""
    inf, nan = float('inf'), float('nan')
    lv = torch.tensor([-inf, -inf, inf, inf, nan, nan, 0.0, 0.0]).reshape(1, 8, 1, 1)
    eps = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0]).reshape(1, 8, 1, 1)
    mu = torch.tensor([1.0, -2.0, 3.0, -1.0, 2.0, -3.0, 1.0, 2.0]).reshape(1, 8, 1, 1)
    g = torch.full((1, 8, 1, 1), 2.0)

    def cpu(mu, lv):
        m, l = mu.clone().requires_grad_(), lv.clone().requires_grad_()
        val = torch.mean(-0.5 * torch.mean(1 + l.flatten(1) - m.flatten(1).pow(2) - l.flatten(1).exp(), dim=1), dim=0)
        (val * eb.KLD_UPSTREAM).backward()
        return {'value': val.detach().numpy(), 'dmu': m.grad.numpy(), 'dlogvar': l.grad.numpy()}
    got, want = _kld_gpu(mu, lv, 'contiguous'), cpu(mu, lv)
    for k in ('dmu', 'dlogvar', 'value'):
        assert _classes(got[k]) == _classes(want[k]), (k, got[k], want[k])
    for special in (-inf, inf, nan):
        one = torch.zeros(1, 8, 1, 1)
        one[0, 3] = special
        got, want = _kld_gpu(mu, one, 'contiguous'), cpu(mu, one)
        assert _classes(got['value']) == _classes(want['value']), (special, got['value'], want['value'])
    m, l = mu.clone().requires_grad_(), lv.clone().requires_grad_()
    z = eps * torch.exp(0.5 * l) + m
    z.backward(g)
    got = _reparam_gpu(mu, lv, eps, g, 'contiguous')
    for k, w in (('z', z.detach()), ('dmu', m.grad), ('dlogvar', l.grad)):
        assert _classes(got[k]) == _classes(w.numpy()), (k, got[k], w)


# ---- Adam, bit for bit ---------------------------------------------------------------------------------------------------------
ADAM_SIZES = (1, 3, 4, 5, 2047, 2048, 2049, 4097, 0, 1023)
ADAM_TENSORS = 200
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
ADAM_MAX_TENSORS = 96                 # icn_launch.h: tensors per launch table


def _adam_values(tag):
    g = _gen('adam', tag)
    return [torch.randn(ADAM_SIZES[i % len(ADAM_SIZES)], generator=g) for i in range(ADAM_TENSORS)]


def _adam_grads(step):
    g = _gen('adam-grad', step)
    return [torch.randn(ADAM_SIZES[i % len(ADAM_SIZES)], generator=g) * 10.0 ** (step - 2) for i in range(ADAM_TENSORS)]


def _bits_equal(got, want):
    return torch.equal(got.detach().cpu().view(torch.int32), torch.as_tensor(want).view(torch.int32))


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_many_tensors_two_groups_unequal_steps_bit_for_bit(wd):
    """200 tensors (every tenth empty, sizes with every n % 4), four steps, the learning rate changing each step.  Every third
    tensor of the first group has no gradient in the first step, so from the second step on one icn_adam_step call carries two
    step counts interleaved.  The second group, added after two steps, is only a second call with a learning rate of its own
    (optim.Adam.step makes one call per group).  No table here reaches ADAM_MAX_TENSORS (at most 72 non-empty tensors share a
    call and a step count): the flush is the next test's."""
    from geniconet_amd import optim
    ps = [t.cuda().requires_grad_() for t in _adam_values('p')]
    first, late = list(range(120)), list(range(120, ADAM_TENSORS))
    P = [t.numpy().copy() for t in _adam_values('p')]
    Mo, V = [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P]
    steps = [0] * ADAM_TENSORS
    o = optim.Adam([ps[i] for i in first], lr=1e-3, betas=BETAS, eps=ADAM_EPS, weight_decay=wd)
    for step in range(4):
        if step == 2:
            o.add_param_group({'params': [ps[i] for i in late]})
        lrs = [1e-3 * (1 + step), 3e-4 * (4 - step)]
        for group, lr in zip(o.param_groups, lrs):
            group['lr'] = lr
        grads = _adam_grads(step)
        live = [i for i in (first if step < 2 else first + late) if not (step == 0 and i % 3 == 1)]
        for i, p in enumerate(ps):
            p.grad = grads[i].cuda() if i in live else None
        assert o._hip_groups() is not None
        o.step()
        for i in live:
            steps[i] += 1
            lr = lrs[0] if i < 120 else lrs[1]
            P[i], Mo[i], V[i] = eb.adam_reference_f32(P[i], grads[i].numpy(), Mo[i], V[i], lr, *BETAS, ADAM_EPS, wd, steps[i])
        if step >= 1:
            assert len({steps[i] for i in first if ps[i].numel()}) == 2          # two step counts in the first group's call
        for i in live:
            st = o.state[ps[i]]
            assert float(st['step']) == steps[i]
            assert _bits_equal(ps[i], P[i]), (step, i, 'p')
            assert _bits_equal(st['exp_avg'], Mo[i]), (step, i, 'm')
            assert _bits_equal(st['exp_avg_sq'], V[i]), (step, i, 'v')
    torch.cuda.synchronize()


@pytest.mark.parametrize('wd', [0.0, 0.01])
def test_adam_device_scalars_give_the_bits_of_step(wd):
    """All 200 tensors in one group with one step count: 180 non-empty ones in one call, so launch_adam flushes a full table of
    ADAM_MAX_TENSORS = 96 and launches the other 84 from a second one.  step() against the restatement bit for bit, and
    step_captured / advance_host (the step of a captured training graph, here launched directly) against step()."""
    from geniconet_amd import optim
    assert sum(1 for i in range(ADAM_TENSORS) if ADAM_SIZES[i % len(ADAM_SIZES)]) > ADAM_MAX_TENSORS
    P = [t.numpy().copy() for t in _adam_values('p')]
    Mo, V = [np.zeros_like(p) for p in P], [np.zeros_like(p) for p in P]
    a = [t.cuda().requires_grad_() for t in _adam_values('p')]
    b = [t.cuda().requires_grad_() for t in _adam_values('p')]
    oa = optim.Adam(a, lr=1e-3, betas=BETAS, eps=ADAM_EPS, weight_decay=wd)
    ob = optim.Adam(b, lr=1e-3, betas=BETAS, eps=ADAM_EPS, weight_decay=wd)
    scal = torch.zeros(2, dtype=torch.float32, device='cuda')
    for step in range(4):
        lr = 1e-3 * (1 + step)
        oa.param_groups[0]['lr'] = ob.param_groups[0]['lr'] = lr
        grads = _adam_grads(step)
        for x, y, g in zip(a, b, grads):
            x.grad, y.grad = g.cuda(), g.cuda()
        oa.step()
        for i, x in enumerate(a):
            P[i], Mo[i], V[i] = eb.adam_reference_f32(P[i], grads[i].numpy(), Mo[i], V[i], lr, *BETAS, ADAM_EPS, wd, step + 1)
            assert _bits_equal(x, P[i]), (step, i, 'p')
            assert _bits_equal(oa.state[x]['exp_avg'], Mo[i]), (step, i, 'm')
            assert _bits_equal(oa.state[x]['exp_avg_sq'], V[i]), (step, i, 'v')
        assert ob.graph_ready()
        if step == 0:       # the first launch precedes the first advance_host, as in a capture: its scalars by hand
            scal.copy_(torch.tensor([lr / (1.0 - BETAS[0]), (1.0 - BETAS[1]) ** 0.5], dtype=torch.float32))
            ob.step_captured(scal)
            ss, bc = ob.advance_host()
            assert torch.equal(scal.cpu(), torch.tensor([ss, bc], dtype=torch.float32))
        else:
            scal.copy_(torch.tensor(ob.advance_host(), dtype=torch.float32))
            ob.step_captured(scal)
        for i, (x, y) in enumerate(zip(a, b)):
            assert float(ob.state[y]['step']) == step + 1
            assert _bits_equal(y, x.detach().cpu()), (step, i, 'p')
            for k in ('exp_avg', 'exp_avg_sq'):
                assert _bits_equal(ob.state[y][k], oa.state[x][k].cpu()), (step, i, k)


CANARY = 12345.0


def _raw_adam(n, offset, wd, step):
    """One icn_adam_step call on views into canary-filled buffers; `offset`: which of p, g, m, v start 4 bytes past a 16-byte
    boundary (buf[1:1 + n]; the others buf[4:4 + n]).  Returns (p, m, v) as CPU tensors after checking every canary and g."""
    from geniconet_amd import _lib
    vals = {}
    g = _gen('adam-raw', n)
    vals['p'], vals['g'] = torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1
    vals['m'], vals['v'] = torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.01 + 1e-4
    bufs, views = {}, {}
    for k in 'pgmv':
        bufs[k] = torch.full((n + 8,), CANARY, dtype=torch.float32, device='cuda')
        lo = 1 if k in offset else 4
        views[k] = bufs[k][lo:lo + n]
        views[k].copy_(vals[k])
        assert views[k].data_ptr() % 16 == (4 if k in offset else 0)
    lr = 2e-3
    one = lambda ctype, v: (ctype * 1)(v)
    ptr = lambda k: one(ctypes.c_void_p, views[k].data_ptr())
    _lib.api().icn_adam_step(1, ptr('p'), ptr('g'), ptr('m'), ptr('v'), one(ctypes.c_size_t, n),
                             one(ctypes.c_float, lr / (1.0 - BETAS[0] ** step)), one(ctypes.c_float, (1.0 - BETAS[1] ** step) ** 0.5),
                             BETAS[0], BETAS[1], ADAM_EPS, wd, _lib.stream())
    torch.cuda.synchronize()
    for k in 'pgmv':
        lo = 1 if k in offset else 4
        full = bufs[k].cpu()
        assert bool((full[:lo] == CANARY).all()) and bool((full[lo + n:] == CANARY).all()), (k, offset)
    assert _bits_equal(views['g'], vals['g'])
    want = eb.adam_reference_f32(vals['p'].numpy(), vals['g'].numpy(), vals['m'].numpy(), vals['v'].numpy(), lr, *BETAS, ADAM_EPS,
                                 wd, step)
    return [views[k].cpu() for k in 'pmv'], want


@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('n', [5, 2049])
def test_adam_scalar_path_equals_the_vector_path_bit_for_bit(n, wd):
    """The kernel promises that a tensor on a 4-byte offset (the scalar path) rounds as a 16-byte aligned one (the vector path):
    each of p, g, m, v offset in turn, then all four; nothing outside a view is written."""
    aligned, want = _raw_adam(n, '', wd, 3)
    for got, w, k in zip(aligned, want, 'pmv'):
        assert _bits_equal(got, w), ('aligned', k)
    for offset in ('p', 'g', 'm', 'v', 'pgmv'):
        res, _ = _raw_adam(n, offset, wd, 3)
        for got, ref, k in zip(res, aligned, 'pmv'):
            assert _bits_equal(got, ref), (offset, k)
