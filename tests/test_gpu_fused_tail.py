"""The decoder's tail as one operator (include/icn_fused.h; fused.bn_add_relu_head): y = tanh(W relu(bn_a(a) + bn_b(b)) + bias) and its
backward, which store neither the ReLU output nor the head's input gradient.

C ABI: against float64 on the CPU, evaluated at the GPU's ReLU pattern (tests/test_relu_pattern.py), with the rule of
tests/test_gpu_arith.py: the error of every output is at most twice the error of the unfused entry points on the same inputs
(icn_bn_stats2 + icn_bn_relu_fwd + icn_head_fwd, icn_head_bwd + icn_bn_relu_bwd -- the yardstick), and inside the project's 1e-4.
Shapes: one row; one row less / more than a chunk of 64 (65 rows are two chunks of 33 and 32); C = 16 with one output; 1000 rows (16
chunks, ragged row groups); level 1 at batch 3 with four outputs; 2050 rows, the first count whose 33 chunks of 63 rows leave a ragged
last chunk (34 rows).  Some channels of either input have |mean| = 100 std.
Module level: one Trainer.step of both models at level 3, batch 2, with the operator on and off, and with hooks that must switch it
off."""
import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu

TOL = 1e-4                # the project's bar (tests/test_gpu_arith.py, tests/test_gpu_training_parity.py)
GRAD_TOL = 1e-3           # tests/test_gpu_training_parity.py: network gradients at a fixed activation pattern
EPS, MOMENTUM = 1e-5, 0.1
CASES = [(1, 64, 3), (63, 64, 3), (65, 16, 1), (1000, 64, 3), (40 * 3, 64, 4), (2050, 64, 3)]
KEYS = ('y', 'da', 'db', 'dw', 'dbias', 'dgamma_a', 'dbeta_a', 'dgamma_b', 'dbeta_b')


def _inputs(M, C, Cout, seed=5):
    g = torch.Generator().manual_seed(seed + M)
    c = torch.arange(C)
    mean_a, std_a = torch.where(c % 4 == 1, 50.0, 0.3), torch.where(c % 4 == 1, 0.5, 2.0)       # |mean| = 100 std in a quarter of
    mean_b, std_b = torch.where(c % 4 == 2, -30.0, -0.3), torch.where(c % 4 == 2, 0.3, 1.0)     # the channels of either input
    t = {'a': torch.randn(M, C, generator=g) * std_a + mean_a, 'b': torch.randn(M, C, generator=g) * std_b + mean_b,
         'ga': 1 + 0.3 * torch.randn(C, generator=g), 'ba': 0.2 * torch.randn(C, generator=g),
         'gb': 1 + 0.3 * torch.randn(C, generator=g), 'bb': 0.2 * torch.randn(C, generator=g),
         'w': torch.randn(Cout, C, generator=g) / C ** 0.5, 'bias': 0.1 * torch.randn(Cout, generator=g),
         'dy': torch.randn(M, Cout, generator=g)}
    return {k: v.float().contiguous() for k, v in t.items()}


def _reference(t, mask):
    """float64 on the CPU at the ReLU pattern `mask` (M, C); also gx = g3 W, the head's input gradient before the mask."""
    d = {k: v.double() for k, v in t.items()}
    out, xh, inv = {}, {}, {}
    z = 0
    for i in 'ab':
        m = d[i].mean(0)
        inv[i] = 1.0 / torch.sqrt(((d[i] - m) ** 2).mean(0) + EPS)
        xh[i] = (d[i] - m) * inv[i]
        z = z + d['g' + i] * xh[i] + d['b' + i]
    x = z * mask
    out['y'] = torch.tanh(x @ d['w'].T + d['bias'])
    g3 = d['dy'] * (1 - out['y'] ** 2)
    out['dw'], out['dbias'] = g3.T @ x, g3.sum(0)
    out['gx'] = g3 @ d['w']
    g = out['gx'] * mask
    for i in 'ab':
        out['dbeta_' + i], out['dgamma_' + i] = g.sum(0), (g * xh[i]).sum(0)
        out['d' + i] = d['g' + i] * inv[i] * (g - g.mean(0) - xh[i] * (g * xh[i]).mean(0))
        out['scale_' + i] = d['g' + i] * inv[i]
    return out


def _run(t, fused):
    """One forward and backward through the C ABI on the GPU -> dict of CPU tensors (and the ReLU output x of the unfused path)."""
    from geniconet_amd import _lib
    L = _lib.api()
    M, C = t['a'].shape
    Cout = t['w'].shape[0]
    dev = torch.device('cuda', 0)
    d = {k: v.to(dev) for k, v in t.items()}
    new = lambda *shape: torch.full(shape, float('nan'), device=dev)           # noqa: E731
    st = {i: new(2 * C) for i in 'ab'}
    rm, rv = {i: torch.zeros(C, device=dev) for i in 'ab'}, {i: torch.ones(C, device=dev) for i in 'ab'}
    ws = _lib.workspace(L.icn_bn_workspace_floats(M, C), dev, torch.float32)
    o = {'y': new(M, Cout), 'da': new(M, C), 'db': new(M, C), 'dw': new(Cout, C), 'dbias': new(Cout), 'sums': new(3 * C)}
    for k in ('dgamma_a', 'dbeta_a', 'dgamma_b', 'dbeta_b'):
        o[k] = new(C)
    p = lambda x: x.data_ptr()                                                 # noqa: E731
    bn = [p(d['a']), p(d['b']), p(st['a']), p(st['b']), p(d['ga']), p(d['ba']), p(d['gb']), p(d['bb'])]
    with torch.cuda.device(dev):
        s = _lib.stream()
        L.icn_bn_stats2(p(d['a']), p(d['b']), M, C, EPS, MOMENTUM, p(rm['a']), p(rv['a']), p(st['a']), EPS, MOMENTUM, p(rm['b']),
                        p(rv['b']), p(st['b']), p(ws), s)
        if fused:
            need = L.icn_bn_head_workspace_bytes(M, C, Cout)
            ws2 = _lib.workspace(need, dev)
            L.icn_bn_head_fwd(*bn, p(d['w']), p(d['bias']), p(o['y']), M, C, Cout, s)
            L.icn_bn_head_bwd(p(d['dy']), p(o['y']), *bn, p(d['w']), p(o['da']), p(o['db']), p(o['sums']), p(o['dw']), p(o['dbias']),
                              p(o['dbeta_a']), p(o['dgamma_a']), p(o['dbeta_b']), p(o['dgamma_b']), M, C, Cout, p(ws2), need, s)
        else:
            o['x'], dx = new(M, C), new(M, C)
            ws2 = _lib.workspace(L.icn_head_workspace_floats(M, C), dev, torch.float32)
            L.icn_bn_relu_fwd(*bn, p(o['x']), M, C, s)
            L.icn_head_fwd(p(o['x']), p(d['w']), p(d['bias']), p(o['y']), M, C, Cout, s)
            L.icn_head_bwd(p(d['dy']), p(o['y']), p(o['x']), p(d['w']), p(dx), p(o['dw']), p(o['dbias']), p(ws2), M, C, Cout, s)
            L.icn_bn_relu_bwd(p(dx), *bn, p(o['da']), p(o['db']), p(o['sums']), p(ws), M, C, p(o['dbeta_a']), p(o['dgamma_a']),
                              p(o['dbeta_b']), p(o['dgamma_b']), s)
        torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'M%d_C%d_o%d' % c)
def test_fused_tail_against_float64_within_twice_the_unfused_error(case):
    t = _inputs(*case)
    unfused, fused = _run(t, False), _run(t, True)
    again = _run(t, True)
    mask = (unfused['x'] > 0).double()
    ref = _reference(t, mask)
    for k in KEYS:
        assert torch.isfinite(fused[k]).all(), k
        e_fused, e_unfused = rel_l2(fused[k].numpy(), ref[k].numpy()), rel_l2(unfused[k].numpy(), ref[k].numpy())
        print('%-9s fused %.3e unfused %.3e' % (k, e_fused, e_unfused))
        assert e_fused < TOL, (k, e_fused)
        assert e_fused <= 2.0 * e_unfused + 1e-9, (k, e_fused, e_unfused)
        assert torch.equal(fused[k], again[k]), k                                 # run to run, bit for bit
        # the same expressions, the head's sums in the unfused operator's type and order, the BatchNorm sums exact doubles regrouped
        # before their one rounding: the unfused entries' bits
        assert torch.equal(fused[k], unfused[k]), k
    # the ReLU mask of the fused backward is the unfused path's.  Where da (db) is exactly zero the sets agree; and as BatchNorm's
    # backward leaves -sum g / M - xhat sum g xhat / M at a masked element, a flipped element shows as a difference of the whole
    # scale * gx there, against rounding differences seven orders smaller: no element may differ by half of that.
    for i in 'ab':
        assert torch.equal(fused['d' + i] == 0, unfused['d' + i] == 0)
        whole = (ref['scale_' + i] * ref['gx']).abs()
        diff = (fused['d' + i].double() - unfused['d' + i].double()).abs()
        flipped = (diff > 0.5 * whole) & (whole > 1e-3 * ref['d' + i].abs().max())
        assert int(flipped.sum()) == 0, (i, int(flipped.sum()))


def _trainer_step(name, tail, monkeypatch, hook=None, seed=21):
    from geniconet_amd import data, fused, models
    from geniconet_amd.train import Trainer
    dev = torch.device('cuda', 0)
    R, B = 3, 2
    calls = {'n': 0}
    real = fused.bn_add_relu_head

    def counted(*args):
        calls['n'] += 1
        return real(*args)
    monkeypatch.setattr(fused, '_NO_TAIL', not tail)
    monkeypatch.setattr(fused, 'bn_add_relu_head', counted)
    p = models.default_params(name, subdivisions=R)
    p[name].update(lr=1e-4, lr_base=1e-4, lr_max=1e-3)
    tr = Trainer(p, dev, seed=seed)
    handle = hook(tr.model) if hook else None
    x, t = data.synthetic_batch(B, R, seed=70, device=dev)
    torch.manual_seed(300)                                                     # the VAE draws its noise from the default generator
    loss = tr.step(x.contiguous(memory_format=torch.channels_last), t)
    if handle:
        handle.remove()
    grads = {k: q.grad.detach().cpu().clone() for k, q in tr.model.named_parameters()}
    stats = {k: v.detach().cpu().clone() for k, v in tr.model.state_dict().items() if 'running' in k or 'tracked' in k}
    return float(loss), grads, stats, calls['n']


def _head_of(net):
    return net.enc2icoConv if hasattr(net, 'enc2icoConv') else net.final_layer


HOOKS = {'head_conv': lambda net: _head_of(net)[0].register_forward_hook(lambda m, i, o: None),
         'head': lambda net: _head_of(net).register_forward_hook(lambda m, i, o: None),
         'last_block': lambda net: net.decoder[-1].register_forward_hook(lambda m, i, o: None)}


@pytest.mark.parametrize('name', ['ico2ico', 'ico2ico_vae'])
def test_one_training_step_with_the_fused_tail_on_and_off(name, monkeypatch):
    """Same weights, same batch, same ReLU pattern (the pre-activation is the same expression): the loss within TOL and every
    parameter gradient within GRAD_TOL (relative L2; gradients whose true value is zero -- conv biases in front of a BatchNorm -- on
    the floor smoke() uses), the running statistics bit for bit.  A hooked head, head conv or last block takes the
    module-by-module path: the same hooked model with the operator switched off gives the same loss and running statistics bit for bit and
    the same gradients: bit for bit in the decoder and the head where every operator there is the library's (the hooked block), within
    GRAD_TOL elsewhere (a hooked head runs torch's Conv2d, whose backward is not deterministic run to run; two identical steps of the
    VAE on the module-by-module path gave equal losses and statistics but gradients that differ in the last bits, on either setting)."""
    loss_on, g_on, s_on, n_on = _trainer_step(name, True, monkeypatch)
    loss_off, g_off, s_off, n_off = _trainer_step(name, False, monkeypatch)
    assert n_on == 1 and n_off == 0
    assert abs(loss_on - loss_off) <= TOL * abs(loss_off), (loss_on, loss_off)
    floor = 1e-3 * max(float(g.norm()) for g in g_off.values())
    for k in g_off:
        err = float((g_on[k].double() - g_off[k].double()).norm()) / max(float(g_off[k].double().norm()), floor)
        assert err < GRAD_TOL, (k, err)
    assert sorted(s_on) == sorted(s_off) and all(torch.equal(s_on[k], s_off[k]) for k in s_off)
    for which, hook in HOOKS.items():
        loss_h, g_h, s_h, n_h = _trainer_step(name, True, monkeypatch, hook=hook)
        loss_o, g_o, s_o, n_o = _trainer_step(name, False, monkeypatch, hook=hook)
        assert n_h == 0 and n_o == 0, which
        assert loss_h == loss_o and all(torch.equal(s_h[k], s_o[k]) for k in s_o), which
        if which == 'last_block' and name == 'ico2ico':   # decoder and head run the library's operators only: deterministic
            exact = [k for k in g_o if k.startswith(('decoder.', 'enc2icoConv.', 'final_layer.'))]
            assert len(exact) == 38 and [k for k in exact if not torch.equal(g_h[k], g_o[k])] == [], which
        for k in g_o:                                                          # (a hooked head runs torch's Conv2d, whose backward is not)
            err = float((g_h[k].double() - g_o[k].double()).norm()) / max(float(g_o[k].double().norm()), floor)
            assert err < GRAD_TOL, (which, k, err)
