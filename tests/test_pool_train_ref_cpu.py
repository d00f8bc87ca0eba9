"""CPU proof (no GPU) of tests/pool_train_ref.py: the closed form of the pooled layer equals torch autograd in float64, the exact side has
the stated chains and tie rule, and every planted variant is rejected."""
import numpy as np
import pytest

import pool_train_ref as P
from dense_ref import fma_chain

TIGHT = 1e-11          # float64 against float64: rounding only (measured worst 1.3e-15 on unit-scale data; offset 8 costs two digits)
SHAPES = [(3, 33, 16, 32, True, 0.0), (3, 33, 16, 32, False, 0.0), (2, 65, 8, 64, True, 8.0)]


@pytest.mark.parametrize('B,N,cin,c,relu,offset', SHAPES)
def test_closed_form_equals_autograd_in_float64(B, N, cin, c, relu, offset):
    k = P.case(B, N, cin, c, relu, offset)
    out, grads = P.autograd64(k['x'], k['w'], k['b'], k['gamma'], k['beta'], relu, k['dout'])
    r = P.forward64(k['x'], k['w'], k['b'], k['gamma'], k['beta'], relu)
    # the planted copies tie: torch may route to either; the reference's own index is judged only where the point is unique
    pair = k['pair']
    same = r['idx'] == k['idx']
    assert same.sum() >= same.size - (same.shape[1] if pair else 0)
    assert P.rel_err(out, r['out']) <= TIGHT
    g = P.backward64(P.forward64(k['x'], k['w'], k['b'], k['gamma'], k['beta'], relu, idx=k['idx']), k['dout'])
    # torch's gradient to x splits between / picks one of the tied copies: compare the SUM over the two planted rows there
    gx, tx = g['x'].copy(), grads['x'].copy()
    if pair:
        for a in (gx, tx):
            a[0, pair[1]] += a[0, pair[2]]
            a[0, pair[2]] = 0
    assert P.rel_err(gx, tx) <= TIGHT
    # gamma[1] == 0 makes every point of a cloud tie in y: torch routes dgamma[1] through whichever it picks, the closed form through
    # the maximum of z (the issue's rule).  Every other gradient of that channel is zero either way (scale = 0) and is compared.
    keep = np.arange(c) != 1
    assert not g['w'][1].any()
    for name in ('w', 'gamma', 'beta'):
        sel = keep if name == 'gamma' else slice(None)
        assert P.rel_err(g[name][sel], grads[name][sel]) <= TIGHT, name
    assert np.abs(grads['b']).max() <= 1e-12 and not g['b'].any()            # torch: rounding noise; the closed form: exactly 0
    assert P.rel_err(k['grads']['w'], grads['w']) <= TIGHT


def test_planted_variants_are_rejected():
    k = P.case(3, 33, 16, 32, True)
    args = (k['x'], k['w'], k['b'], k['gamma'], k['beta'], True)
    out, grads = P.autograd64(*args, k['dout'])
    assert P.rel_err(P.forward64(*args, wrong_sign=True)['out'], out) > P.BAR          # max taken where gamma < 0
    r = P.forward64(*args, idx=k['idx'])
    assert P.rel_err(P.backward64(r, k['dout'], drop_zhat=True)['w'], grads['w']) > P.BAR
    assert P.rel_err(P.backward64(r, k['dout'], bias_grad=True)['b'], grads['b']) > P.BAR
    _, last = P.extrema_exact(k['z32'], k['gamma'], last=True)
    pair = k['pair']
    assert k['idx'][0, 2] == pair[1] and last[0, 2] == pair[2] and (last >= k['idx']).all()


def test_exact_side_has_the_stated_chains_and_tie_rule():
    k = P.case(3, 33, 16, 32, True)
    B, N, cin = k['x'].shape
    z = fma_chain(k['x'].reshape(B * N, cin), k['w']) + k['b'][None, :]       # dense_ref's own chain + the bias once
    assert z.dtype == np.float32 and np.array_equal(z.reshape(B, N, -1), k['z32'])
    zsel, idx = k['zsel32'], k['idx']
    for b in range(B):
        for c in range(32):
            col = k['z32'][b, :, c]
            want = col.max() if k['gamma'][c] >= 0 else col.min()
            assert zsel[b, c] == want and idx[b, c] == np.nonzero(col == want)[0][0]
    assert k['gamma'][1] == 0 and (k['gamma'] < 0).any() and idx.dtype == np.int32
    coef = (k['dout'] * k['f64']['scale']).astype(np.float32)
    t = P.gather_exact(k['x'], coef, idx)
    p = np.zeros(cin, np.float32)
    for b in range(B):                                                       # channel 5, spelled out
        p = np.float32(coef[b, 5]) * k['x'][b, idx[b, 5]].astype(np.float64) + p.astype(np.float64)
        p = p.astype(np.float32)                                            # one rounding per step: a * b is exact in float64, and the
    assert P.rel_err(t[5], p) <= 1e-6                                        # double rounding differs from fmaf by at most an ulp
    want = P.backward64(k['f64'], k['dout'], mask=np.ones_like(k['mask']))
    assert P.rel_err(t, np.einsum('bc,bck->ck', coef.astype(np.float64), k['x'].astype(np.float64)[np.arange(B)[:, None], idx])) <= 1e-5
    dx0 = np.zeros_like(k['x'])
    dx = P.scatter_exact(dx0, coef, idx, k['w'])
    ref = np.zeros(k['x'].shape)
    for b in range(B):
        np.add.at(ref[b], idx[b], coef[b].astype(np.float64)[:, None] * k['w'].astype(np.float64))
    assert P.rel_err(dx, ref) <= 1e-5 and not dx0.any() and want['x'].shape == dx.shape
    rows = [(b, r) for b in range(B) for r in np.unique(idx[b]) if (idx[b] == r).sum() > 1]
    assert rows, 'two channels of a cloud select the same row somewhere'


def test_gram_route_holds_the_bar_at_offset_8_and_the_one_pass_route_does_not():
    k = P.case(2, 65, 8, 64, True, 8.0)
    var = k['f64']['var']
    gram = np.abs(P.var_gram32(k['x'], k['w']) - var) / var
    one = np.abs(P.var_onepass32(k['x'], k['w'], k['b']) - var) / var
    print(f'relative error of var at offset 8: Gram route {gram.max():.2e}, E[z^2] - mean^2 {one.max():.2e}')
    sweep = np.abs(P.var_sweep32(k['x'], k['w'], k['b']) - var) / var
    assert gram.max() <= P.BAR and sweep.max() <= P.BAR          # the Gram route and the sweep stay within the bar
    assert one.max() > P.BAR              # the one-pass route does not


def test_two_rows_are_where_the_gram_route_loses_the_variance_and_the_sweep_keeps_it():
    """(2, 1, 8, 32), unconditioned: S has rank one and some W[c] is nearly orthogonal to the two points' difference."""
    k = P.case(2, 1, 8, 32, False)
    var = k['f64']['var']
    kap = P.kappa(k['f64'])
    gram = np.abs(P.var_gram32(k['x'], k['w']) - var) / var
    sweep = np.abs(P.var_sweep32(k['x'], k['w'], k['b']) - var) / var
    print(f'(2, 1, 8, 32): kappa up to {kap.max():.3g}, relative error of var: Gram route {gram.max():.2e}, sweep {sweep.max():.2e}')
    assert kap.max() > 1e3                                      # the case is the hard one
    u = 2.0 ** -24
    assert sweep.max() <= 16 * u * np.sqrt(kap.max()) * 8       # sqrt(kappa) times the roundoff of a chain of Cin = 8, with slack 16
    assert gram.max() > sweep.max()
