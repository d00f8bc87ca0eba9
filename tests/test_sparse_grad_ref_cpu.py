"""Pins the yardstick tests/sparse_grad_ref.py.  No GPU, no kernel of catgrasp_amd.

Its float64 gradients equal torch autograd through dense float64 conv3d / conv_transpose3d to 1e-12 * max(1, |ref|) on the full299
scene, for the submanifold 3x3x3, strided, inverse and 1x1x1 layers.  The transposed rule books of the input gradient hold
nbr[i, k] = j  <=>  nbr_t[j, k'] = i on full299 and every small edge scene.  The float32 restatements of the kernels' chains
(wgrad_exact, dgrad_exact) stay within float32 rounding of the float64 gradients and change bits under each planted variant:
descending rows, one flat chain without chunks, a submanifold weight that is transposed but not flipped."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_grad_ref as gref
import sparse_ref as ref
from dense_ref import gamma

CIN, COUT = 6, 5


def _close(got, want, what):
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert got.shape == want.shape and err.max(initial=0.0) <= 1e-12, (what, err.max(initial=0.0))


def _dense(idx, x, shape):
    out = torch.zeros((ref.BATCH,) + tuple(shape) + (x.shape[1],), dtype=torch.float64)
    i = torch.from_numpy(idx.astype(np.int64))
    return out.index_put((i[:, 0], i[:, 1], i[:, 2], i[:, 3]), x).permute(0, 4, 1, 2, 3)


def _at(dense_out, idx):
    i = torch.from_numpy(idx.astype(np.int64))
    return dense_out[i[:, 0], :, i[:, 1], i[:, 2], i[:, 3]]


@pytest.mark.parametrize('kind', ['subm', 'down', 'inverse', 'k1'])
def test_float64_gradients_equal_autograd_through_dense_convolutions(kind):
    idx = ref.scene()
    out_idx, _, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
    nbr, _, _, n_in, n_out = gref.books(idx, ref.SHAPE)[kind]
    k = {'subm': 3, 'down': 2, 'inverse': 2, 'k1': 1}[kind]
    w, b = ref.weights(k, CIN, COUT)
    x = np.random.default_rng(1).uniform(-1, 1, (n_in, CIN))
    dy = np.random.default_rng(7).uniform(-1, 1, (n_out, COUT))
    X, W, B = (torch.from_numpy(np.asarray(a, dtype=np.float64)).requires_grad_() for a in (x, w, b))
    if kind == 'subm':
        out = _at(F.conv3d(_dense(idx, X, ref.SHAPE), W.permute(4, 3, 0, 1, 2), B, padding=1), idx)
    elif kind == 'down':
        out = _at(F.conv3d(_dense(idx, X, ref.SHAPE), W.permute(4, 3, 0, 1, 2), B, stride=2), out_idx)
    elif kind == 'inverse':
        up = F.conv_transpose3d(_dense(out_idx, X, out_shape), W.permute(3, 4, 0, 1, 2), None, stride=2)
        full = F.pad(up, (0, ref.SHAPE[2] - up.shape[4], 0, ref.SHAPE[1] - up.shape[3], 0, ref.SHAPE[0] - up.shape[2]))
        out = _at(full, idx) + B
        assert dropped.sum() >= 6
    else:
        out = X @ W.reshape(CIN, COUT) + B
    np.testing.assert_allclose(out.detach().numpy(), ref.conv(x, nbr, w, b), rtol=0, atol=1e-12)
    (out * torch.from_numpy(dy)).sum().backward()
    dw, dx, db = gref.grads(x, nbr, w, dy)
    _close(dw, W.grad.numpy().reshape(dw.shape), f'{kind} dW')
    _close(dx, X.grad.numpy(), f'{kind} dx')
    _close(db, B.grad.numpy(), f'{kind} db')
    assert np.abs(dw).max() > 0.1 and np.abs(dx).max() > 0.1


def _scenes():
    yield 'full299', ref.scene(), ref.SHAPE
    for name in ref.EDGE_SCENES:
        if name != 'large':
            idx, shape, _ = ref.edge_scene(name)
            yield name, idx, shape


def test_transposed_books_hold_the_identity():
    seen = 0
    for name, idx, shape in _scenes():
        bk = gref.books(idx, shape)
        assert ('down' in bk) == (min(shape) >= 2)
        for kind, (nbr, nbr_t, flip, n_in, n_out) in bk.items():
            K = nbr.shape[1]
            assert nbr.shape == (n_out, K) and nbr_t.shape == (n_in, K) and flip == (kind == 'subm')
            assert nbr.max(initial=-1) < n_in and nbr_t.max(initial=-1) < n_out
            forward = {(i, k, int(nbr[i, k])) for i in range(n_out) for k in range(K) if nbr[i, k] >= 0}
            back = {(int(nbr_t[j, k]), (K - 1 - k) if flip else k, j) for j in range(n_in) for k in range(K) if nbr_t[j, k] >= 0}
            assert forward == back, (name, kind)
            seen += len(forward)
    assert seen > 5000


def _share(a, b):
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


def test_the_exact_restatements_are_within_rounding_and_see_each_planted_variant():
    idx, shape, _ = gref.big_scene()
    n = len(idx)
    assert n == 2 * gref.ROWS + 1
    nbr, nbr_t, flip, _, _ = gref.books(idx, shape)['subm']
    cin = cout = 16
    x, dy = ref.features(n, cin), gref.dy_for(n, cout)
    w = ref.weights(3, cin, cout)[0].reshape(27, cin, cout)
    dw64, dx64, db64 = gref.grads(x, nbr, w, dy)
    dw, db = gref.wgrad_exact(x, nbr, dy)
    dx = gref.dgrad_exact(dy, nbr_t, w, flip)
    # n fmaf roundings per chain (+ the chunk adds) on sums of magnitude <= n * max|x| * max|dy|, resp. 27*cout products
    assert np.abs(dw - dw64).max() <= gamma(n + 3) * n * np.abs(dy).max() and np.abs(db - db64).max() <= gamma(n + 3) * np.abs(dy.astype(np.float64)).sum(0).max()
    assert np.abs(dx - dx64).max() <= gamma(27 * cout) * 27 * cout * np.abs(dy).max() * np.abs(w).max()
    for what, (pw, pb) in (('descending rows', gref.wgrad_exact(x, nbr, dy, descending=True)), ('one flat chain', gref.wgrad_exact(x, nbr, dy, rows=n))):
        share_w, share_b = _share(dw, pw), _share(db, pb)
        print(f'{what}: {100 * share_w:.1f} % of dW and {100 * share_b:.1f} % of db change bits')
        assert share_w > 0.05 and share_b > 0, what
        assert np.abs(pw - dw64).max() <= 1e-5 and np.abs(pb - db64).max() <= 1e-5            # and yet the same values
    unflipped = gref.dgrad_exact(dy, nbr_t, w, False)
    assert _share(dx, unflipped) > 0.5 and np.abs(unflipped - dx64).max() > 1e-3              # a wrong gradient, not a reordering
    assert _share(dx, gref.dgrad_exact(dy, nbr_t, w, flip)) == 0
    again = gref.wgrad_exact(x, nbr, dy)
    assert _share(dw, again[0]) == 0 and _share(db, again[1]) == 0


def test_the_exact_weight_gradient_of_no_rows_is_zero():
    dw, db = gref.wgrad_exact(np.zeros((5, 16), np.float32), np.zeros((0, 8), np.int32), np.zeros((0, 32), np.float32))
    assert dw.shape == (8, 16, 32) and not dw.any() and db.shape == (32,) and not db.any()
