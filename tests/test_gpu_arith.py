"""The three-way bf16 split of the channel-mixing contraction (ICN_ARITH=bf16x3; include/icn.h icn_set_arith) is fp32-GRADE arithmetic:
its error against the float64 oracle must stay within 2 x the exact fp32 kernel's on the same inputs -- not merely under the 1e-4 bar
(VERDICT r5 item 1 acceptance).  The reference computes in plain fp32 (models.py / run.py: no autocast), so this is the bar a drop-in has
to hold.  Every case also checks that the split kernels really ran (HIP-event profile of the launch names).
"""
import numpy as np
import pytest
import torch

from conftest import rel_l2
from oracle import ico_ref
from test_gpu_parity import MFMA_CASES, PAIR_CASES

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture
def arith():
    from geniconet_amd import _lib
    prev = _lib.get_arith()
    yield _lib
    _lib.set_arith(prev)


def _kernels_of(fn):
    from geniconet_amd import _lib
    _lib.profile_start(256)
    out = fn()
    torch.cuda.synchronize()
    return out, {e['kernel'] for e in _lib.profile_stop()}


def _conv_case(case, seed, pair, bias=True):
    """Inputs + the float64 oracle's outputs and gradients for a single convolution or a pair sharing its input."""
    r, stride, cin, cout, B, mode = case[:6]
    g = torch.Generator().manual_seed(seed)
    n = 2 ** r
    k = 2 if pair else 1
    x = torch.randn(B, cin, 5 * n, 2 * n, generator=g)
    ws = [torch.randn(cout, cin, 7, generator=g) / (7 * cin) ** 0.5 for _ in range(k)]
    bs = [torch.randn(cout, generator=g) if bias else None for _ in range(k)]
    xr = x.double().requires_grad_()
    wr = [w.double().requires_grad_() for w in ws]
    yr = [ico_ref.ico_conv(xr, wr[i], bs[i].double() if bias else None, r, stride, mode) for i in range(k)]
    gys = [torch.randn(y.shape, generator=g) for y in yr]
    torch.autograd.backward(yr, [gy.double() for gy in gys])
    ref = {'y%d' % i: yr[i].detach() for i in range(k)}
    ref['dx'] = xr.grad
    for i in range(k):
        ref['dw%d' % i] = wr[i].grad
    return (r, stride, mode, x, ws, bs, gys), ref


def _run(inputs, pair):
    from geniconet_amd.ico_conv import ico_conv, ico_conv_pair
    r, stride, mode, x, ws, bs, gys = inputs
    xg = x.cuda().requires_grad_()
    wg = [w.cuda().requires_grad_() for w in ws]
    bg = [b.cuda() if b is not None else None for b in bs]
    if pair:
        ys = ico_conv_pair(xg, wg[0], bg[0], wg[1], bg[1], r, stride, mode)
    else:
        ys = (ico_conv(xg, wg[0], bg[0], r, stride, mode),)
    torch.autograd.backward(ys, [gy.cuda() for gy in gys])
    out = {'y%d' % i: ys[i].detach() for i in range(len(ys))}
    out['dx'] = xg.grad
    for i in range(len(ys)):
        out['dw%d' % i] = wg[i].grad
    return out


def _errors(got, ref):
    return {k: rel_l2(got[k].cpu().numpy(), ref[k].numpy()) for k in ref}


# stride-1 cases run the split kernels in forward, data gradient and weight gradient (k_wgrad7<.., 1>); stride-2 cases too: their data
# gradients are the masked launches (k_conv_b3<128, BN, NW>), their weight gradients the per-tap kernel (k_wgrad_dma<.., 1>)
SINGLE = [c for c in MFMA_CASES if c[2] % 32 == 0 and c[3] % 64 == 0]
PAIRS = [c for c in PAIR_CASES if c[2] % 32 == 0 and c[3] % 64 == 0]


@pytest.mark.parametrize('case', SINGLE, ids=lambda c: 'r%d_s%d_%dx%d_b%d_%s' % c)
def test_split_arithmetic_is_fp32_grade_single(case, arith):
    inputs, ref = _conv_case(case, 11, False)
    arith.set_arith('f32')
    exact = _errors(_run(inputs, False), ref)
    arith.set_arith('bf16x3')
    got, kernels = _kernels_of(lambda: _run(inputs, False))
    split = _errors(got, ref)
    assert any(k.startswith('k_conv_b3') for k in kernels), kernels
    if case[1] == 1 and case[0] >= 2 and case[2] % 64 == 0 and case[3] % 64 == 0:
        assert 'k_wgrad7<.., 1>' in kernels, kernels
    for k in ref:
        assert split[k] < TOL, (k, split[k])
        assert split[k] <= 2.0 * exact[k] + 1e-9, (k, split[k], exact[k])


@pytest.mark.parametrize('case', PAIRS, ids=lambda c: 'r%d_s%d_%dx2x%d_b%d_%s_bias%d' % c)
def test_split_arithmetic_is_fp32_grade_pair(case, arith):
    inputs, ref = _conv_case(case, 23, True, bias=case[6])
    arith.set_arith('f32')
    exact = _errors(_run(inputs, True), ref)
    arith.set_arith('bf16x3')
    got, kernels = _kernels_of(lambda: _run(inputs, True))
    split = _errors(got, ref)
    assert any(k.startswith('k_conv_b3') for k in kernels), kernels
    if case[1] == 2:
        assert 'k_conv_b3<128, BN, NW>' in kernels and 'k_wgrad_dma<.., 1>' in kernels, kernels
    for k in ref:
        assert split[k] < TOL, (k, split[k])
        assert split[k] <= 2.0 * exact[k] + 1e-9, (k, split[k], exact[k])


@pytest.mark.parametrize('r,cin,cout,B', [(2, 256, 256, 5), (3, 256, 128, 3), (4, 128, 64, 2)])
def test_split_arithmetic_in_the_decoder_heads_dense_gemms(r, cin, cout, B, arith):
    """conv(upsample(x)) pair (models.py:58-60): z = x W and dx = g W are dense one-tap GEMMs -- both on the split kernels, against
    the float64 oracle's upsample-then-convolve."""
    from geniconet_amd import fused
    from geniconet_amd.ico_conv import IcoConvS2S, IcoUpsampleS2S
    torch.manual_seed(5)
    n = 2 ** r
    x = torch.randn(B, cin, 5 * n, 2 * n)
    convs = [IcoConvS2S(cin, cout, subdivisions=r + 1, corner_mode='average') for _ in range(2)]
    xr = x.double().requires_grad_()
    up = ico_ref.ico_upsample(xr, r, 'average')
    yr = [ico_ref.ico_conv(up, c.weight.detach().double(), c.bias.detach().double(), r + 1, 1, 'average') for c in convs]
    gys = [torch.randn(y.shape) for y in yr]
    torch.autograd.backward(yr, [g.double() for g in gys])
    ref = {'y0': yr[0].detach(), 'y1': yr[1].detach(), 'dx': xr.grad}
    ups = [IcoUpsampleS2S(cin, r, 'average').cuda() for _ in range(2)]
    cg = [c.cuda() for c in convs]

    def run():
        xg = x.cuda().requires_grad_()
        ys = fused.upconv_pair(xg, ups[0], ups[1], cg[0], cg[1])
        torch.autograd.backward(ys, [g.cuda() for g in gys])
        return {'y0': ys[0].detach(), 'y1': ys[1].detach(), 'dx': xg.grad}
    arith.set_arith('f32')
    exact = _errors(run(), ref)
    arith.set_arith('bf16x3')
    got, kernels = _kernels_of(run)
    split = _errors(got, ref)
    assert any(k.startswith('k_conv_b3_dense') for k in kernels), kernels
    for k in ref:
        assert split[k] < TOL, (k, split[k])
        assert split[k] <= 2.0 * exact[k] + 1e-9, (k, split[k], exact[k])


def test_split_arithmetic_is_deterministic_and_the_exact_path_is_untouched(arith):
    """Two runs under bf16x3 are bit-identical (stream-K adds its partial tiles in a fixed order there too); switching back to f32
    gives bit-for-bit what f32 gave before the switch."""
    inputs, _ = _conv_case((3, 1, 256, 256, 36, 'average'), 3, False)
    arith.set_arith('f32')
    a0 = _run(inputs, False)
    arith.set_arith('bf16x3')
    b0, b1 = _run(inputs, False), _run(inputs, False)
    arith.set_arith('f32')
    a1 = _run(inputs, False)
    for k in a0:
        assert torch.equal(b0[k], b1[k]), k
        assert torch.equal(a0[k], a1[k]), k
        assert not torch.equal(a0[k], b0[k]), k                       # (the modes really differ)
        assert rel_l2(b0[k].cpu().numpy(), a0[k].cpu().numpy()) < 5e-6, k


def test_special_values_survive_the_split(arith):
    """Zeros stay zero rows, huge and tiny magnitudes keep fp32's range (bf16 has fp32's exponent), a NaN input poisons its outputs."""
    from geniconet_amd.ico_conv import ico_conv
    torch.manual_seed(9)
    r, cin, cout, B = 2, 64, 128, 2
    n = 2 ** r
    x = torch.randn(B, cin, 5 * n, 2 * n, device='cuda')
    w = torch.randn(cout, cin, 7, device='cuda') / (7 * cin) ** 0.5
    arith.set_arith('bf16x3')
    assert torch.count_nonzero(ico_conv(torch.zeros_like(x), w, None, r, 1, 'average')) == 0
    for scale in (1e30, 1e-30):
        y = ico_conv(x * scale, w, None, r, 1, 'average')
        arith.set_arith('f32')
        ye = ico_conv(x * scale, w, None, r, 1, 'average')
        arith.set_arith('bf16x3')
        assert torch.isfinite(y).all()
        assert rel_l2(y.cpu().numpy(), ye.cpu().numpy()) < 5e-6, scale
    xn = x.clone()
    xn[0, 3, 5, 2] = float('nan')
    reach = ico_ref.ico_conv(torch.zeros(B, cin, 5 * n, 2 * n, dtype=torch.float64).index_put_(
        (torch.tensor([0]), torch.tensor([3]), torch.tensor([5]), torch.tensor([2])), torch.tensor([1.0], dtype=torch.float64)),
        w.abs().double().cpu(), None, r, 1, 'average') > 0                    # the outputs whose sums read the NaN
    for mode in ('bf16x3', 'f32'):
        arith.set_arith(mode)
        y = ico_conv(xn, w, None, r, 1, 'average')
        assert torch.equal(torch.isnan(y).cpu(), reach), mode
        assert torch.isfinite(y.cpu()[~reach]).all(), mode


# ---- non-finite values through the split: the exact kernel's footprint ------------------------------------------------------
# (kind, r, stride, cin, cout, B): a single convolution at stride 1 and 2, a pair, the decoder block's upsample + conv pair
NONFINITE_CASES = [('single', 2, 1, 64, 64, 2), ('single', 3, 2, 64, 128, 2), ('pair', 2, 1, 64, 64, 2), ('upconv', 2, 1, 64, 64, 2)]


def _positions(r):
    """(item, row, column) of an interior pixel, a chart-seam pixel, a chart corner that feeds the north pole mean and a pixel of
    the second item, at level r (n = 2^r)."""
    n = 2 ** r
    return {'interior': (0, n + 1, 2), 'seam': (0, 2 * n, 3), 'pole_corner': (0, 3 * n, 0), 'second_item': (1, 4 * n + 1, 2)}


def _classes(t):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    t = t.detach().cpu()
    c = torch.zeros(t.shape, dtype=torch.int8)
    c[torch.isposinf(t)], c[torch.isneginf(t)], c[torch.isnan(t)] = 1, 2, 3
    return c


def _expected(pos_reach, neg_reach, value):
    """Footprint of one special value from the oracle on indicators: pos_reach / neg_reach = sums of the positive / negative
    coefficients with which it reaches each output.  +inf lands as +inf where only positive ones reach, -inf where only negative
    ones do, NaN where both do; a NaN wherever anything reaches."""
    p, q = pos_reach > 0, neg_reach > 0
    if value != value:
        return (p | q).to(torch.int8) * 3
    if value < 0:
        p, q = q, p
    c = torch.zeros(p.shape, dtype=torch.int8)
    c[p & ~q], c[q & ~p], c[p & q] = 1, 2, 3
    return c


def _reach(case, x, ws, gys, which, at):
    """{output: (pos_reach, neg_reach)} of a unit at `at` in x (which='x') or in gy of the first branch (which='gy'), float64."""
    from test_gpu_production_parity import _op
    op = _op(case)
    k = len(ws)
    plus = lambda t: t.double().clamp_min(0)
    minus = lambda t: (-t.double()).clamp_min(0)
    b, i, j = at
    nob = [torch.zeros(w.shape[0], dtype=torch.float64) for w in ws]

    def args(xv, wv):
        d = {'x': xv}
        for m in range(k):
            d['w%d' % m], d['b%d' % m] = wv[m], nob[m]
        return d
    out = {}
    if which == 'x':
        e = torch.zeros(x.shape, dtype=torch.float64)
        e[b, 3, i, j] = 1
        for sgn, f in ((0, plus), (1, minus)):
            ys = op(**args(e, [f(w) for w in ws]))
            for m, y in enumerate(ys):
                out.setdefault('y%d' % m, [None, None])[sgn] = y
            wr = [w.double().requires_grad_() for w in ws]
            torch.autograd.backward(op(**args(e, wr)), [f(g) for g in gys])
            for m in range(k):
                out.setdefault('dw%d' % m, [None, None])[sgn] = wr[m].grad
    else:
        e = torch.zeros(gys[0].shape, dtype=torch.float64)
        e[b, 3, i, j] = 1
        ge = [e] + [torch.zeros_like(e) for _ in range(k - 1)]
        for sgn, f in ((0, plus), (1, minus)):
            xr = torch.zeros(x.shape, dtype=torch.float64, requires_grad=True)
            torch.autograd.backward(op(**args(xr, [f(w) for w in ws])), ge)
            out.setdefault('dx', [None, None])[sgn] = xr.grad
            wr = [w.double().requires_grad_() for w in ws]
            torch.autograd.backward(op(**args(f(x), wr)), ge)
            out.setdefault('dw0', [None, None])[sgn] = wr[0].grad
        db = torch.zeros(ws[0].shape[0], dtype=torch.float64)
        db[3] = 1
        out['db0'] = [db, torch.zeros_like(db)]
    return out


@pytest.mark.xfail(strict=True, reason='the split cuts +-inf activations into NaN residual pieces (inf - inf): the fix in split_bf16x3 '
                                       '(pieces of +-FLT_MAX and a +-inf third piece) costs 5.4 % of the headline step (DESIGN 4.0)')
@pytest.mark.parametrize('which', ['x', 'gy'])
@pytest.mark.parametrize('case', NONFINITE_CASES, ids=lambda c: '%s_r%d_s%d_%dx%d_b%d' % c)
def test_non_finite_activations_give_the_exact_footprint_in_both_arithmetics(case, which, arith):
    """+-inf and NaN in x, or in the output gradient, at an interior, a chart-seam, a pole-corner and a second item's pixel: the
    split's outputs are +inf, -inf, NaN or finite exactly where the exact kernel's are, and what stays finite holds the
    element-wise bar.  The exact kernel's forward of a single convolution or a pair is the oracle's indicator footprint; the
    upconv composite and the gradient kernels regroup coefficients before they meet the special value (virtual taps, aggregated
    output gradients, zero rows), so there the exact kernel is the reference."""
    import error_bounds as eb
    from test_gpu_production_parity import _inputs, _named, _op, _run_gpu
    kind, r, stride = case[:3]
    x, ws, bs, gys = _inputs(case)
    lvl = r if which == 'x' else (r + 1 if kind == 'upconv' else r - (stride == 2))
    for pos, at in _positions(lvl).items():
        b, i, j = at
        x0, g0 = x.clone(), [g.clone() for g in gys]
        (x0 if which == 'x' else g0[0])[b, 3, i, j] = 0.0
        ref, A = eb.oracle_and_bound(_op(case), _named(case, x0, ws, bs), g0)
        reach = _reach(case, x, ws, gys, which, at)
        for value in (float('inf'), -float('inf'), float('nan')):
            xs, gs = x0.clone(), [g.clone() for g in g0]
            (xs if which == 'x' else gs[0])[b, 3, i, j] = value
            have = {}
            for mode in ('f32', 'bf16x3'):
                arith.set_arith(mode)
                got = _run_gpu(case, xs, ws, bs, gs)
                have[mode] = {k: _classes(v) for k, v in got.items()}
                for k in ref:
                    fin = have[mode][k] == 0
                    rho = eb.rho(got[k][fin], ref[k][fin], A[k][fin])
                    assert rho <= eb.bar(k), (mode, pos, value, k, rho)
            for k in ref:
                if which == 'x' and kind in ('single', 'pair') and k.startswith('y'):
                    assert torch.equal(have['f32'][k], _expected(*reach[k], value)), (pos, value, k)
                elif k not in reach:
                    assert (have['f32'][k] == 0).all(), (pos, value, k)
                assert torch.equal(have['bf16x3'][k], have['f32'][k]), (pos, value, k, int((have['bf16x3'][k] != have['f32'][k]).sum()))


@pytest.mark.parametrize('case', NONFINITE_CASES, ids=lambda c: '%s_r%d_s%d_%dx%d_b%d' % c)
def test_an_infinite_weight_gives_the_exact_kernels_footprint_under_the_split(case, arith):
    """+-inf in one weight: the split's non-finite outputs, and their signs, are the exact kernel's (a zero row of the operand it
    meets makes 0 * inf = NaN in both).  The one exception: the stride-2 data gradient under the split runs the masked launches,
    whose zero rows (input pixels no output reads through that tap) meet the weight too -- there the split may add NaNs, but
    never a finite value or an infinity the exact kernel does not give."""
    from test_gpu_production_parity import _inputs, _run_gpu
    x, ws, bs, gys = _inputs(case)
    for value in (float('inf'), -float('inf')):
        for t in (0, 4):
            wv = [w.clone() for w in ws]
            wv[0][5, 3, t] = value
            have = {}
            for mode in ('f32', 'bf16x3'):
                arith.set_arith(mode)
                have[mode] = {k: _classes(v) for k, v in _run_gpu(case, x, wv, bs, gys).items()}
            for k in have['f32']:
                e, s = have['f32'][k], have['bf16x3'][k]
                if k in ('y0', 'dx'):
                    assert (e != 0).any(), (value, t, k)
                if case[2] == 2 and k == 'dx':
                    assert ((s == e) | (s == 3)).all(), (value, t, k)
                    continue
                assert torch.equal(s, e), (value, t, k, int((s != e).sum()))


def test_the_mode_is_part_of_the_abi(arith):
    assert arith.set_arith('bf16x3') in ('f32', 'bf16x3')
    assert arith.get_arith() == 'bf16x3'
    with pytest.raises(KeyError):
        arith.set_arith('bf16')
    assert arith.lib().icn_set_arith(7) == -1 and b'arithmetic mode' in arith.lib().icn_last_error()
    assert arith.get_arith() == 'bf16x3'
