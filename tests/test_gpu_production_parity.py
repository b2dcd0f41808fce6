"""Every operator of the training step against the float64 oracle at the shapes the step runs them at.

The case list is read off the models (error_bounds.step_calls): ico2ico I5 / batch 36, ico2ico_vae I5 / batch 36 and ico2ico I6 /
batch 8, de-duplicated.  At these shapes the launches run hundreds of tiles, stream-K splits and weight-gradient sums of up to
B P = 368 640 terms -- what the small-shape tests elsewhere never reach.  The bars are element-wise (error_bounds.rho <= RHO_MAX)
beside the rel-L2 bars of tests/test_gpu_arith.py, in both arithmetics; BatchNorm per channel; the loss per sample.

Measured maxima on the MI355X over all cases (a value above half its bar is a finding, not a reason to raise the bar):
  y, dx     rho 7.4 (f32) / 7.0 (bf16x3), bar RHO_MAX = 16: the sequential fp32 accumulation, the same in both arithmetics;
            per case 0.7-1.3 (upconv y), 0.9-2.7 (upconv dx), 1.7-2.2 (r2/r3 singles), 3.0-7.4 (the rest); head y 1.2, dx 3.8
  dw, db    rho 0.63 / 0.59, bar RHO_MAX_WGRAD = 2
  BatchNorm mean 1.0, var 1.6, running statistics 2.1, y 2.6, dx 1.9 (units of u), bar 8; dgamma / dbeta 0.06, bar 2
  p2p loss  value 8e-8 relative, per-sample gradient rel-L2 3e-6 (r5 / B36), bars 2e-5 / 5e-5
"""
import zlib

import numpy as np
import pytest
import torch

import error_bounds as eb
from conftest import rel_l2
from oracle import ico_ref

pytestmark = pytest.mark.gpu
TOL = 1e-4
CASES = eb.production_cases()
CONV = [c for c in CASES if c[0] in ('stem', 'single', 'pair', 'upconv', 'head')]
BNS = [c for c in CASES if c[0] == 'bn']
LOSS = [c for c in CASES if c[0] == 'p2p']
CL = torch.channels_last


def _cid(c):
    return '_'.join(str(v) for v in c)


def _seed(case):
    return zlib.crc32(repr(case).encode())


@pytest.fixture
def arith():
    from geniconet_amd import _lib
    prev = _lib.get_arith()
    yield _lib
    _lib.set_arith(prev)


def _kernels_of(fn):
    from geniconet_amd import _lib
    _lib.profile_start(4096)
    out = fn()
    torch.cuda.synchronize()
    return out, {e['kernel'] for e in _lib.profile_stop()}


def _is_split(kernel):
    return 'b3' in kernel or kernel.endswith(', 1>')


# ---- convolution-type operators -------------------------------------------------------------------------------------------------
def _inputs(case):
    """Seeded Gaussian input and output gradients, weights and biases at the model's init scale (IcoConvS2S / nn.Conv2d)."""
    kind, r, stride, cin, cout, B = case
    g = torch.Generator().manual_seed(_seed(case))
    n = 2 ** r
    n_out = 2 * n if kind == 'upconv' else n // stride
    k = 2 if kind in ('pair', 'upconv') else 1
    taps = 1 if kind == 'head' else 7
    bound = 1.0 / (taps * cin) ** 0.5
    x = torch.randn(B, cin, 5 * n, 2 * n, generator=g)
    ws = [(torch.rand(cout, cin, taps, generator=g) * 2 - 1) * bound for _ in range(k)]
    bs = [(torch.rand(cout, generator=g) * 2 - 1) * bound for _ in range(k)]
    gys = [torch.randn(B, cout, 5 * n_out, 2 * n_out, generator=g) for _ in range(k)]
    return x, ws, bs, gys


def _op(case):
    kind, r, stride = case[:3]
    if kind in ('stem', 'single'):
        return lambda x, w0, b0: (ico_ref.ico_conv(x, w0, b0, r, stride, 'average'),)
    if kind == 'pair':
        return lambda x, w0, b0, w1, b1: (ico_ref.ico_conv(x, w0, b0, r, stride, 'average'),
                                          ico_ref.ico_conv(x, w1, b1, r, stride, 'average'))
    assert kind == 'upconv', kind                       # (the head: error_bounds.head_oracle)

    def up(x, w0, b0, w1, b1):
        u = ico_ref.ico_upsample(x, r, 'average')
        return ico_ref.ico_conv(u, w0, b0, r + 1, 1, 'average'), ico_ref.ico_conv(u, w1, b1, r + 1, 1, 'average')
    return up


def _named(case, x, ws, bs):
    d = {'x': (x, case[0] != 'stem')}                   # the stem's input needs no gradient in the step
    for i, (w, b) in enumerate(zip(ws, bs)):
        d['w%d' % i], d['b%d' % i] = (w, True), (b, True)
    return d


def _run_gpu(case, x, ws, bs, gys):
    """The step's own entry point for this operator, forward + backward; the head returns tanh(z) as 'y0'."""
    from geniconet_amd.ico_conv import (ico_conv, ico_conv_pair, ico_conv_pair_supported, ico_upconv_pair,
                                        ico_upconv_pair_supported)
    kind, r, stride = case[:3]
    if kind == 'head':
        return eb.head_run(x, ws[0], bs[0], gys[0])
    xg = x.cuda().contiguous(memory_format=CL).requires_grad_(kind != 'stem')
    wg = [w.cuda().requires_grad_() for w in ws]
    bg = [b.cuda().requires_grad_() for b in bs]
    if kind in ('stem', 'single'):
        ys = (ico_conv(xg, wg[0], bg[0], r, stride, 'average'),)
    elif kind == 'pair':
        assert ico_conv_pair_supported(xg, wg[0], wg[1], r, stride)
        ys = ico_conv_pair(xg, wg[0], bg[0], wg[1], bg[1], r, stride, 'average')
    else:
        assert ico_upconv_pair_supported(xg, wg[0], wg[1], r)
        ys = ico_upconv_pair(xg, wg[0], bg[0], wg[1], bg[1], r, 'average')
    torch.autograd.backward(ys, [g.cuda() for g in gys])
    out = {'y%d' % i: y.detach().cpu() for i, y in enumerate(ys)}
    if kind != 'stem':
        out['dx'] = xg.grad.cpu()
    for i in range(len(wg)):
        out['dw%d' % i] = wg[i].grad.detach().cpu().reshape(ws[i].shape)
        out['db%d' % i] = bg[i].grad.detach().cpu()
    return out


def _measure(case, got, gys, oracle):
    """{output: (rho, rel-L2)} against the oracle (ref, A); for the head: y = tanh(z) in float64, its gradients through the linear
    oracle with the kernel's own dz = gy (1 - y^2)."""
    if case[0] == 'head':
        x, ws, bs, _ = _inputs(case)
        ref, A = eb.head_oracle(x, ws[0], bs[0], gys[0], got['y0'])
    else:
        ref, A = oracle
    return {k: (eb.rho(got[k], ref[k], A[k]), rel_l2(got[k].numpy(), ref[k].numpy())) for k in ref}


@pytest.mark.parametrize('case', CONV, ids=_cid)
def test_production_operator_against_the_float64_oracle(case, arith):
    x, ws, bs, gys = _inputs(case)
    arith.set_arith('f32')
    got_e, k_e = _kernels_of(lambda: _run_gpu(case, x, ws, bs, gys))
    arith.set_arith('bf16x3')
    got_s, k_s = _kernels_of(lambda: _run_gpu(case, x, ws, bs, gys))
    assert not any(_is_split(k) for k in k_e), k_e
    if case[0] in ('single', 'pair', 'upconv'):
        assert any(_is_split(k) for k in k_s), k_s
    oracle = None if case[0] == 'head' else eb.oracle_and_bound(_op(case), _named(case, x, ws, bs), gys)
    exact, split = _measure(case, got_e, gys, oracle), _measure(case, got_s, gys, oracle)
    print('\nRHO %s  f32 %s  bf16x3 %s' % (_cid(case), ' '.join('%s=%.2f' % (k, v[0]) for k, v in exact.items()),
                                          ' '.join('%s=%.2f' % (k, v[0]) for k, v in split.items())))
    for k in exact:
        for mode, m in (('f32', exact), ('bf16x3', split)):
            assert m[k][0] <= eb.bar(k), (mode, k, m[k])
            assert m[k][1] < TOL, (mode, k, m[k])
        assert split[k][1] <= 2.0 * exact[k][1] + 1e-9, (k, split[k], exact[k])


# ---- BatchNorm (+ residual) + ReLU --------------------------------------------------------------------------------------------
def _bn_inputs(case, dual):
    _, M, C, _ = case
    g = torch.Generator().manual_seed(_seed(case))
    k = 2 if dual else 1
    xs = [torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) * 1.5 + 0.5) + (torch.rand(C, generator=g) * 2 - 1)
          for _ in range(k)]
    gammas = [torch.rand(C, generator=g) + 0.5 for _ in range(k)]
    betas = [torch.rand(C, generator=g) - 0.5 for _ in range(k)]
    rm0 = [torch.randn(C, generator=g) for _ in range(k)]
    rv0 = [torch.rand(C, generator=g) + 0.5 for _ in range(k)]
    gy = torch.randn(M, C, generator=g)
    return xs, gammas, betas, rm0, rv0, gy


_bn_run = eb.bn_run


@pytest.mark.parametrize('case', BNS, ids=_cid)
def test_production_batchnorm_per_channel(case):
    """Statistics from a momentum-1 pass (running mean / var = the batch's mean / unbiased variance), the running statistics at
    the step's momentum 0.1, y and the gradients against the float64 restatement under the kernel's own ReLU pattern."""
    _, M, C, dual = case
    xs, gammas, betas, rm0, rv0, gy = _bn_inputs(case, dual)
    k = len(xs)
    zeros = [torch.zeros(C)] * k
    got = _bn_run(xs, gammas, betas, zeros, zeros, gy, 1.0)
    run = _bn_run(xs, gammas, betas, rm0, rv0, gy, 0.1)
    x64 = [x.double() for x in xs]
    ref = eb.bn_relu_ref(x64, [g.double() for g in gammas], [b.double() for b in betas], gy.double(), mask=got['y'] > 0)
    m32 = float(np.float32(0.1))
    worst = {}
    for i in range(k):
        mean, var = ref['mean%d' % i], ref['var%d' % i]
        unb = var * M / (M - 1)
        meas = {'mean': eb.stat_rho(got['rm%d' % i], mean, x64[i].abs().mean(0)),
                'var': eb.stat_rho(got['rv%d' % i], unb, unb),
                'running_mean': eb.stat_rho(run['rm%d' % i], (1 - m32) * rm0[i].double() + m32 * mean,
                                            (1 - m32) * rm0[i].double().abs() + m32 * x64[i].abs().mean(0)),
                'running_var': eb.stat_rho(run['rv%d' % i], (1 - m32) * rv0[i].double() + m32 * unb,
                                           (1 - m32) * rv0[i].double() + m32 * unb),
                'dx': eb.per_channel_rel_l2(got['dx%d' % i], ref['dx%d' % i]),
                'dgamma': eb.stat_rho(got['dgamma%d' % i], ref['dgamma%d' % i], ref['A_dgamma%d' % i]),
                'dbeta': eb.stat_rho(got['dbeta%d' % i], ref['dbeta%d' % i], ref['A_dbeta%d' % i])}
        for name, v in meas.items():
            worst['%s%d' % (name, i)] = float(v.max())
    worst['y'] = float(eb.per_channel_rel_l2(got['y'], ref['y']).max())
    print('\nBN %s %s' % (_cid(case), ' '.join('%s=%.2f' % kv for kv in worst.items())))
    for name, v in worst.items():
        bar = eb.BN_RL2_MAX if name[:2] in ('y', 'dx') else (eb.bar(name) if name.startswith('d') else eb.BN_STAT_MAX)
        assert v <= bar, (name, v, bar)


# ---- loss --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('factors', [(1.0, 0.0, 0.0), (0.6, 0.2, 0.2)], ids=['ae', 'vae'])
@pytest.mark.parametrize('case', LOSS, ids=_cid)
def test_production_p2p_loss_value_and_per_sample_gradient(case, factors):
    """P2P_Loss with the autoencoder's factors (position only: its own backward kernel) and the VAE's 0.6 / 0.2 / 0.2 against
    oracle/loss_ref.py; the gradient per sample, so that one item's chunk cannot hide among the batch."""
    from geniconet_amd.losses import P2P_Loss
    from oracle import loss_ref
    _, r, B = case
    g = torch.Generator().manual_seed(_seed(case))
    n = 2 ** r
    pred = torch.randn(B, 3, 5 * n, 2 * n, generator=g)
    target = torch.randn(B, 9, 10 * n * n + 2, generator=g)
    crit = P2P_Loss(r, *factors).cuda()
    x = pred.cuda().contiguous(memory_format=CL).requires_grad_()
    loss = crit(x, target.cuda())
    loss.backward()
    want = loss_ref.p2p_loss(pred.numpy(), target.numpy(), r, *factors)
    assert abs(float(loss) - want) <= 2e-5 * abs(want), (float(loss), want)
    gw = loss_ref.p2p_grad(pred.numpy(), target.numpy(), r, *factors)
    gg = x.grad.cpu().numpy()
    per = [rel_l2(gg[b], gw[b]) for b in range(B)]
    print('\nP2P %s %s value %.2e  worst per-sample grad rel-L2 %.2e' % (_cid(case), factors, abs(float(loss) - want) / abs(want), max(per)))
    assert max(per) < 5e-5, per


# ---- the list covers the step ---------------------------------------------------------------------------------------------------
def test_the_case_list_launches_every_mfma_kernel_kind_of_the_step():
    """One Trainer step per configuration and the convolution-type cases above, forward + backward without the oracle, in the
    default arithmetic: every MFMA kernel kind the step launches must be launched by the list."""
    from geniconet_amd import data, models
    from geniconet_amd.train import Trainer
    step = set()
    for name, R, B in eb.CONFIGS:
        tr = Trainer(models.default_params(name, subdivisions=R), 'cuda', seed=0)
        x, t = data.synthetic_batch(B, R, seed=1, device='cuda')
        tr.step(x, t)
        _, kinds = _kernels_of(lambda: tr.step(x, t))
        step |= kinds
        del tr
    listed = set()
    for case in CONV:
        _, kinds = _kernels_of(lambda: _run_gpu(case, *_inputs(case)))
        listed |= kinds
    assert step, 'the profiler saw no MFMA launch in the step'
    assert step <= listed, sorted(step - listed)
