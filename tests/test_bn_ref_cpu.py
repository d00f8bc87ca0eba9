"""CPU tests of the BatchNorm + ReLU yardstick (tests/bn_ref.py): the float64 formulas against torch autograd, the float32 restatement
of the kernels' chains against float64, and the planted variants that the bit-for-bit GPU tests must be able to see."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref as B

BAR = 1e-4
SHAPES = [(2, 16), (3, 16), (65, 32), (1025, 48), (2049, 16)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('n,c', SHAPES[:4])
def test_float64_formulas_are_torch_autograd(n, c):
    r = B.case(n, c)
    x = torch.from_numpy(np.array(r['x'])).double().requires_grad_(True)
    gamma = torch.from_numpy(np.array(r['gamma'])).double().requires_grad_(True)
    beta = torch.from_numpy(np.array(r['beta'])).double().requires_grad_(True)
    y = torch.relu(F.batch_norm(x, None, None, gamma, beta, training=True, eps=B.EPS))
    y.backward(torch.from_numpy(np.array(r['dy'])).double())
    for got, want, what in ((r['f64']['y'], y, 'y'), (r['dx64'], x.grad, 'dx'), (r['dgamma64'], gamma.grad, 'dgamma'), (r['dbeta64'], beta.grad, 'dbeta')):
        err = B.rel_err(got, want.detach().numpy())
        assert err <= 1e-12, (what, err)
    # a given mask is used as it is
    mask = r['f64']['z'] > 0
    for a, b in zip(B.backward64(r['x'], r['dy'], r['gamma'], mask=mask), (r['dx64'], r['dgamma64'], r['dbeta64'])):
        assert np.array_equal(a, b)


@pytest.mark.parametrize('n,c', SHAPES)
def test_float32_restatement_is_within_the_bar_of_float64(n, c):
    r = B.case(n, c)
    assert np.abs(r['f64']['z']).min() >= B.MARGIN
    for k in ('y', 'mean', 'var', 'invstd', 'scale', 'shift'):
        assert B.rel_err(r['f32'][k], r['f64'][k]) <= BAR, k
    for k in ('dx', 'dgamma', 'dbeta'):
        assert B.rel_err(r[k + '32'], r[k + '64']) <= BAR, k


def test_column_sum_is_the_stated_tree():
    """Against a scalar loop written from the header's words, on a column whose partial sums round."""
    n = 2 * B.ROWS + 70
    t = (np.random.default_rng(3).uniform(0, 1, (n, 2)) * [1.0, 1e4]).astype(np.float32)
    u = np.random.default_rng(4).uniform(-1, 1, (n, 2)).astype(np.float32)
    for second in (None, u):
        total = None
        for lo in range(0, n, B.ROWS):
            chunk = None
            for s in range(lo, min(lo + B.ROWS, n), B.SEG):
                p = np.zeros(2, np.float32)
                for i in range(s, min(s + B.SEG, n)):
                    p = p + t[i] if second is None else B.fmaf(t[i], second[i], p)
                chunk = p if chunk is None else chunk + p
            total = chunk if total is None else total + chunk
        assert np.array_equal(_bits(B.column_sum(t, second)), _bits(total))


def test_planted_variants_change_bits():
    n, c = 2049, 16
    r = B.case(n, c)
    x, gamma, beta, dy = r['x'], r['gamma'], r['beta'], r['dy']
    base = r['f32']
    for kw in (dict(flat=True), dict(descending=True), dict(one_pass=True)):
        other = B.forward32(x, gamma, beta, **kw)
        assert (_bits(other['mean']) != _bits(base['mean'])).any() or (_bits(other['var']) != _bits(base['var'])).any(), kw
        assert (_bits(other['y']) != _bits(base['y'])).mean() > 0.01, kw
    fused = B.forward32(x, gamma, beta, contract=True)
    assert np.array_equal(_bits(fused['scale']), _bits(base['scale'])) and (_bits(fused['y']) != _bits(base['y'])).mean() > 0.01
    for kw in (dict(flat=True), dict(descending=True)):
        dx, dgamma, dbeta = B.backward32(x, dy, base, **kw)
        assert (_bits(dgamma) != _bits(r['dgamma32'])).any() and (_bits(dbeta) != _bits(r['dbeta32'])).any(), kw
        assert (_bits(dx) != _bits(r['dx32'])).mean() > 0.01, kw


def test_two_pass_variance_holds_the_bar_on_an_offset_column_and_one_pass_does_not():
    """Column 0 has mean 1e3 and deviation 1.  What the variance formula decides -- var, invstd, scale -- and mean, shift and every
    gradient hold the bar with two passes.  The activation of that one column is reported, not asserted: float32's spacing at 1e3 is
    6.1e-5, the chain that sums 300 such values leaves the mean 8.7e-5 off, and y = x*scale + shift carries that error times |scale|
    plus two roundings of its own at magnitude 1e3, whichever way the variance is formed (measured here: 2.9e-4 against the bar of
    1e-4).  The other columns hold the bar."""
    n, c = 300, 16
    r = B.case(n, c, offset=1e3)
    assert abs(r['f64']['mean'][0] - 1e3) < 0.5 and 0.5 < r['f64']['var'][0] < 2.0
    for k in ('mean', 'var', 'invstd', 'scale', 'shift'):
        assert B.rel_err(r['f32'][k], r['f64'][k]) <= BAR, k
    for k in ('dx', 'dgamma', 'dbeta'):
        assert B.rel_err(r[k + '32'], r[k + '64']) <= BAR, k
    assert B.rel_err(r['f32']['y'][:, 1:], r['f64']['y'][:, 1:]) <= BAR
    print('y of the offset column, two-pass:', B.rel_err(r['f32']['y'][:, 0], r['f64']['y'][:, 0]),
          'mean:', abs(float(r['f32']['mean'][0]) - r['f64']['mean'][0]))
    one = B.forward32(r['x'], r['gamma'], r['beta'], one_pass=True)
    errs = {k: B.rel_err(one[k][:1], r['f64'][k][:1]) for k in ('var', 'invstd')}
    print('one-pass variance on a column of mean 1e3, deviation 1:', errs)
    assert errs['var'] > BAR and B.rel_err(one['y'][:, 0], r['f64']['y'][:, 0]) > BAR


def test_constant_column_is_finite():
    r = B.case(65, 32, constant=True)
    assert r['f32']['var'][1] < 1e-12 and all(np.isfinite(v).all() for v in r['f32'].values())
    assert np.isfinite(r['dx32']).all() and np.isfinite(r['dgamma32']).all()
