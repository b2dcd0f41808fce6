"""The element-wise and per-channel error bars of tests/error_bounds.py have teeth (no GPU needed).

Exact results rounded to fp32 pass them; each of the defects a kernel could plausibly have -- one output element missing one
tap's term, one weight-gradient entry missing one pixel, one 128 x 64 tile missing one K-step, one pole pixel on the wrong corner
rule, one BatchNorm row chunk left out of a statistic -- is flagged at 4 x the margin or more.  And at every production call of
the step the longest sum is still short enough for a single dropped term of typical size to be flagged at 4 x the margin.
"""
import pytest
import torch

import error_bounds as eb
from oracle import ico_ref

R, STRIDE, CIN, COUT, B = 2, 1, 64, 64, 2


def _fp32(d):
    return {k: v.float().double() for k, v in d.items()}


@pytest.fixture(scope='module')
def conv():
    g = torch.Generator().manual_seed(7)
    n = 2 ** R
    x = torch.randn(B, CIN, 5 * n, 2 * n, generator=g)
    w = (torch.rand(COUT, CIN, 7, generator=g) * 2 - 1) / (7 * CIN) ** 0.5
    b = (torch.rand(COUT, generator=g) * 2 - 1) / (7 * CIN) ** 0.5
    gy = torch.randn(B, COUT, 5 * n, 2 * n, generator=g)
    op = lambda x, w, b: (ico_ref.ico_conv(x, w, b, R, STRIDE, 'average'),)
    ref, A = eb.oracle_and_bound(op, {'x': (x, True), 'w': (w, True), 'b': (b, True)}, [gy])
    return dict(x=x.double(), w=w.double(), b=b.double(), gy=gy.double(), ref=ref, A=A)


def test_exact_results_rounded_to_fp32_pass(conv):
    got = _fp32(conv['ref'])
    for k in conv['ref']:
        assert eb.rho(got[k], conv['ref'][k], conv['A'][k]) <= 1.0, k       # one rounding: <= u |v| <= u A


def test_a_nonzero_where_the_bound_is_zero_is_flagged(conv):
    A = conv['A']['y0'].clone()
    A[0, 0, 0, 0] = 0
    got = conv['ref']['y0'].clone()
    assert eb.rho(got, conv['ref']['y0'], A) == float('inf')
    got[0, 0, 0, 0] = 0
    ref = conv['ref']['y0'].clone()
    ref[0, 0, 0, 0] = 0
    assert eb.rho(got, ref, A) < 1.0


def _flagged(got, conv, key):
    rho = eb.rho(got, conv['ref'][key], conv['A'][key])
    assert rho >= 4 * eb.bar(key), (key, rho)
    return rho


def test_one_output_element_missing_one_taps_term(conv):
    t, bi, co, p = 3, 1, 17, 29                                       # an interior output pixel, tap (-1, 1)
    only_t = torch.zeros(7, dtype=torch.float64)
    only_t[t] = 1
    tap = ico_ref.ico_conv(conv['x'], conv['w'] * only_t, None, R, STRIDE, 'average')
    got = _fp32(conv['ref'])['y0']
    flat = got.view(B, COUT, -1)
    flat[bi, co, p] -= tap.view(B, COUT, -1)[bi, co, p].float().double()
    _flagged(got, conv, 'y0')


def test_weight_gradient_missing_one_pixels_contribution(conv):
    """dw[co, ci, t] = sum over (b, p) of gy[b, co, p] x[b, ci, tap_t(p)]: leave out one (b, p)."""
    co, ci, t, bi, p = 5, 11, 2, 0, 77
    src = int(ico_ref.tap_table(R, STRIDE)[t, p])
    assert src < 10 * 4 ** R                                          # an ordinary pixel, not a pole mean
    term = conv['gy'].view(B, COUT, -1)[bi, co, p] * conv['x'].view(B, CIN, -1)[bi, ci, src]
    got = _fp32(conv['ref'])['dw']
    got[co, ci, t] -= term
    _flagged(got, conv, 'dw')


def test_one_tile_missing_one_k_step(conv):
    """Rows 128..255 of the (B P) x Cout GEMM, columns 0..63: tap 4, input channels 32..63 left out."""
    t, k0, rows, cols = 4, 32, slice(128, 256), slice(0, 64)
    only = torch.zeros(COUT, CIN, 7, dtype=torch.float64)
    only[:, k0:k0 + 32, t] = 1
    part = ico_ref.ico_conv(conv['x'], conv['w'] * only, None, R, STRIDE, 'average')
    as_gemm = lambda y: y.permute(0, 2, 3, 1).reshape(-1, COUT)           # (B P, Cout), row = b * P + p
    got = _fp32(conv['ref'])['y0']
    g2 = as_gemm(got).clone()
    g2[rows, cols] -= as_gemm(part)[rows, cols]
    got = g2.view(B, 5 * 2 ** R, 2 ** (R + 1), COUT).permute(0, 3, 1, 2)
    _flagged(got, conv, 'y0')


def test_one_pole_pixel_on_the_zeros_rule(conv):
    """Output pixel 0 (chart 0, row 0, column 0) reads the north pole through tap (0, -1)."""
    bi, co = 1, 40
    zeros = ico_ref.ico_conv(conv['x'], conv['w'], conv['b'], R, STRIDE, 'zeros')
    got = _fp32(conv['ref'])['y0']
    assert zeros[bi, co, 0, 0] != conv['ref']['y0'][bi, co, 0, 0]
    got[bi, co, 0, 0] = float(zeros[bi, co, 0, 0])
    _flagged(got, conv, 'y0')


# ---- BatchNorm -----------------------------------------------------------------------------------------------------------------
M, C, CHUNK = 4 * 640, 32, 128


@pytest.fixture(scope='module')
def bn():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(M, C, generator=g) * 2 + 0.3).double()
    gamma = (torch.rand(C, generator=g) + 0.5).double()
    beta = (torch.rand(C, generator=g) - 0.5).double()
    gy = torch.randn(M, C, generator=g).double()
    return dict(x=x, gamma=gamma, beta=beta, gy=gy, ref=eb.bn_relu_ref([x], [gamma], [beta], gy))


def _bn_measures(got, ref, x):
    """the per-channel bars of tests/test_gpu_production_parity.py, each as its worst channel"""
    return {'mean': float(eb.stat_rho(got['mean0'], ref['mean0'], x.abs().mean(0)).max()),
            'var': float(eb.stat_rho(got['var0'], ref['var0'], ref['var0']).max()),
            'y': float(eb.per_channel_rel_l2(got['y'], ref['y']).max()),
            'dx': float(eb.per_channel_rel_l2(got['dx0'], ref['dx0']).max()),
            'dgamma': float(eb.stat_rho(got['dgamma0'], ref['dgamma0'], ref['A_dgamma0']).max()),
            'dbeta': float(eb.stat_rho(got['dbeta0'], ref['dbeta0'], ref['A_dbeta0']).max())}


def test_batchnorm_rounded_to_fp32_passes(bn):
    got = _fp32(bn['ref'])
    m = _bn_measures(got, bn['ref'], bn['x'])
    for k, v in m.items():
        assert v <= 1.0, (k, v)


def test_batchnorm_missing_one_row_chunk_of_one_channel_is_flagged(bn):
    c, k = 9, 7
    x = bn['x']
    keep = torch.ones(M, dtype=torch.bool)
    keep[k * CHUNK:(k + 1) * CHUNK] = False
    stats = list(eb.bn_stats(x))
    stats[0], stats[1] = stats[0].clone(), stats[1].clone()
    stats[0][c] = x[keep, c].mean()
    stats[1][c] = ((x[keep, c] - stats[0][c]) ** 2).mean()
    mask = bn['ref']['y'] > 0
    wrong = _fp32(eb.bn_relu_ref([x], [bn['gamma']], [bn['beta']], bn['gy'], mask=mask, stats=[tuple(stats)]))
    m = _bn_measures(wrong, bn['ref'], x)
    assert m['mean'] >= 4 * eb.BN_STAT_MAX and m['var'] >= 4 * eb.BN_STAT_MAX, m
    assert m['y'] >= 4 * eb.BN_RL2_MAX and m['dx'] >= 4 * eb.BN_RL2_MAX, m
    assert m['dgamma'] >= 4 * eb.bar('dgamma'), m


# ---- production sums -----------------------------------------------------------------------------------------------------------
def test_production_case_list_covers_the_three_configurations():
    cases = eb.production_cases()
    kinds = {c[0] for c in cases}
    assert kinds == {'stem', 'single', 'pair', 'upconv', 'head', 'bn', 'p2p'}
    assert ('stem', 5, 1, 3, 64, 36) in cases and ('stem', 6, 1, 3, 64, 8) in cases
    assert ('pair', 3, 2, 256, 512, 36) in cases                       # the VAE's latent pair
    assert ('upconv', 2, 1, 512, 256, 36) in cases                     # the VAE decoder's first block
    assert ('bn', 36 * 10240, 64, True) in cases                       # the last decoder block at I5 / B36
    assert len(eb.step_calls('ico2ico', 5, 36)) == 2 + 4 * 6 + 2       # stem + BN, six blocks, head, loss


@pytest.mark.parametrize('case', [c for c in eb.production_cases() if c[0] not in ('bn', 'p2p')], ids=str)
def test_a_dropped_term_stays_detectable_at_production_sum_lengths(case):
    for out, n in eb.n_terms(*case).items():
        assert eb.detectable(n, out), (out, n, 1.0 / (n * eb.U), 4 * eb.bar(out))


# ---- the streaming kernels off the production shapes (tests/test_gpu_streaming_edges.py) ------------------------------------------
# Each bound A is validated before any GPU run: an fp32 restatement of the kernel's arithmetic must stay under a quarter of RHO_MAX
# (y, dx, KLD, reparameterisation) or half of BN_STAT_MAX (statistics, affine gradients).  Measured here: BatchNorm y 2.6, dx 2.8,
# dgamma 1.0, dbeta 1.0, mean 1.1, var 2.4, at most 0.22 % of the ReLU pattern flipped; KLD value 0.7, dmu 2.5, dlogvar 2.3;
# reparameterisation z 1.2, dlogvar 1.3.
def test_batchnorm_edge_case_list_covers_every_width_family_and_form():
    cases = eb.bn_edge_cases()
    assert 36 <= len(cases) <= 44
    for C in eb.BN_EDGE_C:
        mine = [c for c in cases if c[1] == C]
        assert {c[0] for c in mine} >= set(eb.BN_EDGE_M)
        assert {c[3] for c in mine} == {0, 1, 2} and {c[2] for c in mine} == {False, True}
    for C in (4, 32):
        assert {c[2] for c in cases if c[:2] == (eb.BN_EMPTY_CHUNK_M, C)} == {False, True}
    assert max(c[0] * c[1] for c in cases) <= 1.1e6
    chunks, rows = eb.bn_chunking(eb.BN_EMPTY_CHUNK_M)
    assert chunks == 512 and (chunks - 1) * rows >= eb.BN_EMPTY_CHUNK_M          # the last chunk starts past the last row
    for M, C, _, _ in cases:                        # C < 64: the forward's 4 rows per iteration x stripes exceed a chunk's rows
        if C <= 32:
            assert 4 * 256 // (C // 4) > eb.bn_chunking(M)[1]


@pytest.mark.parametrize('case', eb.bn_edge_cases(), ids=str)
def test_batchnorm_fp32_restatement_stays_well_inside_the_edge_bars(case):
    xs, gammas, betas, gy = eb.bn_edge_inputs(case)
    m = eb.bn_edge_measure(eb.bn_restatement_f32(xs, gammas, betas, gy), xs, gammas, betas, gy)
    assert m.pop('flips_inside')
    assert m.pop('flip_share') <= eb.BN_FLIP_SHARE_MAX / 2
    for name, v in m.items():
        bar = eb.bn_edge_bar(name)
        assert v <= (bar / 4 if bar == eb.RHO_MAX else bar / 2), (name, v)


def test_batchnorm_edge_bars_flag_a_row_added_twice():
    """What a broken row clamp of the statistics pass would do: the last row of a chunk enters the sums a second time."""
    case = (63, 8, False, 0)
    xs, gammas, betas, gy = eb.bn_edge_inputs(case)
    twice = [torch.cat([xs[0], xs[0][-1:]])]
    good = eb.bn_restatement_f32(xs, gammas, betas, gy)
    bad = eb.bn_restatement_f32(twice, gammas, betas, torch.cat([gy, gy[-1:]]))
    for k in ('rm0', 'rv0'):
        good[k] = bad[k]
    m = eb.bn_edge_measure(good, xs, gammas, betas, gy)
    assert m['mean0'] >= 4 * eb.BN_STAT_MAX and m['var0'] >= 4 * eb.BN_STAT_MAX, m


@pytest.mark.parametrize('family', eb.KLD_FAMILIES)
@pytest.mark.parametrize('shape', eb.KLD_EDGE_SHAPES, ids=str)
def test_kld_and_reparam_fp32_restatement_stays_under_a_quarter_of_the_bar(shape, family):
    import numpy as np
    mu, lv, eps, g = eb.kld_edge_inputs(shape, family)
    up = float(np.float32(eb.KLD_UPSTREAM))
    for (ref, A), got in ((eb.kld_oracle(mu, lv, up), eb.kld_restatement_f32(mu, lv, up)),
                          (eb.reparam_oracle(mu, lv, eps, g), eb.reparam_restatement_f32(mu, lv, eps, g))):
        for k in ref:
            assert eb.rho(np.asarray(got[k]), np.asarray(ref[k]), np.asarray(A[k])) <= eb.RHO_MAX / 4, k


def test_kld_edge_shapes_have_the_element_counts_of_the_kernel_edges():
    import math
    assert [math.prod(s) for s in eb.KLD_EDGE_SHAPES] == [1, 255, 256, 257, 1024 * 256 + 1]


def test_adam_restatement_is_adam():
    """Three steps of adam_reference_f32 against torch's Adam in float64, within the tolerances of tests/test_optim.py."""
    import numpy as np
    for wd in (0.0, 0.01):
        g = torch.Generator().manual_seed(11)
        p = torch.randn(4099, generator=g)
        ref = p.double().clone().requires_grad_()
        oref = torch.optim.Adam([ref], lr=1e-3, weight_decay=wd)
        P, Mo, V = p.numpy().copy(), np.zeros(4099, np.float32), np.zeros(4099, np.float32)
        for step in range(3):
            lr = 1e-3 * (1 + step)
            oref.param_groups[0]['lr'] = lr
            grad = (torch.randn(4099, generator=g) * 10.0 ** (step - 2))
            ref.grad = grad.double()
            oref.step()
            P, Mo, V = eb.adam_reference_f32(P, grad.numpy(), Mo, V, lr, 0.9, 0.999, 1e-8, wd, step + 1)
            assert P.dtype == Mo.dtype == V.dtype == np.float32
            assert torch.allclose(torch.from_numpy(P).double(), ref.detach(), rtol=2e-6, atol=1e-7), step
            for got, k in ((Mo, 'exp_avg'), (V, 'exp_avg_sq')):
                want = oref.state[ref][k]
                assert torch.allclose(torch.from_numpy(got).double(), want, rtol=2e-6, atol=3e-7 * float(want.abs().max())), (step, k)
