"""Yardstick of the sparse convolution layers' gradients (catgrasp_amd/spconv_autograd.py, csrc/sparse_conv_grad.hip).  CPU only: numpy,
tests/sparse_ref.py for the rule books and the forward chain, tests/dense_ref.py for the emulated fmaf.
tests/test_sparse_grad_ref_cpu.py pins it against torch autograd through dense float64 convolutions.

grads        float64 gradients of sparse_ref.conv (no prologue, no residual) for dy = dL/dout:
               dW[k] = x[nbr[rows, k]]^T @ dy[rows] over the rows with a neighbour at k, dx by np.add.at of dy[rows] @ W[k]^T onto
               the rows nbr[rows, k], db = dy.sum(0).
books        the four (nbr, transposed nbr, flip) of a scene.  nbr_t[j, k'] = i exactly when nbr[i, k] = j, with k' = 26 - k for the
               submanifold 3x3x3 layer (flip) and k' = k for the others (include/catgrasp_amd_sparse_grad.h has the table).
wgrad_exact  float32, the bits of cg_sparse_conv_wgrad: the rows in chunks of CG_SPARSE_GRAD_ROWS; per chunk and element a chain of
               fmaf from +0 over the chunk's rows in ascending order (rows without a neighbour at k skipped; the bias: fmaf(1, dy, p)
               over every row); then the partial of chunk 0 and the others added to it in ascending order.
dgrad_exact  float32, the bits of cg_sparse_conv_dgrad: sparse_ref.conv_exact over the transposed book with the transposed weight
               (k ascending, the channels of dy in the order of the MFMA steps, no bias).
"""
import re

import numpy as np

import sparse_ref as ref
from catgrasp_amd import _lib
from dense_ref import fmaf

with open(_lib.SPARSE_GRAD_HEADER_PATH) as _f:
    ROWS = int(re.search(r'^#define CG_SPARSE_GRAD_ROWS (\d+)$', _f.read(), flags=re.M).group(1))


def grads(x, nbr, w, dy):
    """float64 -> (dW (K, Cin, Cout), dx (n_in, Cin), db (Cout,)).  w: (k0, k1, k2, Cin, Cout) or (K, Cin, Cout)."""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1, w.shape[-2], w.shape[-1])
    assert w.shape[0] == nbr.shape[1] and w.shape[1] == x.shape[1] and dy.shape == (nbr.shape[0], w.shape[2])
    dw, dx = np.zeros_like(w), np.zeros_like(x)
    for k in range(w.shape[0]):
        rows = np.nonzero(nbr[:, k] >= 0)[0]
        dw[k] = x[nbr[rows, k]].T @ dy[rows]
        np.add.at(dx, nbr[rows, k], dy[rows] @ w[k].T)
    return dw, dx, dy.sum(0)


def books(idx, shape):
    """{kind: (nbr (n_out, K), nbr_t (n_in, K), flip, n_in, n_out)} of a scene, from the restatement."""
    n = len(idx)
    subm = ref.subm_rules(idx, shape)
    one = np.arange(n, dtype=np.int32).reshape(n, 1)
    out = {'subm': (subm, subm, True, n, n), 'k1': (one, one, False, n, n)}
    if min(shape) >= 2:
        out_idx, down, _, _ = ref.down_rules(idx, shape)
        inv = ref.inverse_rules(idx, out_idx, shape)
        out['down'] = (down, inv, False, n, len(out_idx))
        out['inverse'] = (inv, down, False, len(out_idx), n)
    return out


def transposed_weight(w, flip):
    """(K, Cin, Cout) -> (K, Cout, Cin): Wt[k] = W[k]^T, with flip W[K - 1 - k]^T."""
    w = np.asarray(w).reshape(-1, w.shape[-2], w.shape[-1])
    return np.ascontiguousarray(np.swapaxes(w[::-1] if flip else w, 1, 2))


def dy_for(n_out, cout, seed=7):
    """Uniform in +-sqrt(3 / n_out): weight gradients of order one."""
    a = np.sqrt(3.0 / max(n_out, 1))
    return np.random.default_rng(seed).uniform(-a, a, (n_out, cout)).astype(np.float32)


def wgrad_exact(x, nbr, dy, rows=ROWS, descending=False):
    """float32 (dW (K, Cin, Cout), db (Cout,)) with the bits of cg_sparse_conv_wgrad.  Planted variants: rows = n_out is one flat
    chain without chunks, descending runs every chunk's rows from the last to the first."""
    f32 = np.float32
    x, dy = np.asarray(x, dtype=f32), np.asarray(dy, dtype=f32)
    (n_out, K), cin, cout = nbr.shape, x.shape[1], dy.shape[1]
    dw, db = np.zeros((K, cin, cout), f32), np.zeros(cout, f32)
    for lo in range(0, n_out, max(rows, 1)):
        p, pb = np.zeros((K, cin, cout), f32), np.zeros(cout, f32)
        chunk = range(lo, min(lo + rows, n_out))
        for i in (reversed(chunk) if descending else chunk):
            pb = fmaf(f32(1), dy[i], pb)
            ks = np.nonzero(nbr[i] >= 0)[0]
            if len(ks):
                p[ks] = fmaf(x[nbr[i, ks]][:, :, None], dy[i][None, None, :], p[ks])
        dw, db = (p, pb) if lo == 0 else (dw + p, db + pb)
    assert dw.dtype == f32 and db.dtype == f32
    return dw, db


def dgrad_exact(dy, nbr_t, w, flip):
    """float32 dx (n_in, Cin) with the bits of cg_sparse_conv_dgrad.  flip = False on a submanifold 3x3x3 book is the planted
    wrong weight permutation."""
    return ref.conv_exact(np.asarray(dy, dtype=np.float32), nbr_t, transposed_weight(np.asarray(w, dtype=np.float32), flip))


BIG_SHAPE = (9, 40, 41)


def big_scene():
    """-> (indices, spatial shape, batch size) with n = 2*ROWS + 1 sites: two whole chunks and a last chunk of one row."""
    return ref.scene(n=2 * ROWS + 1, seed=11, shape=BIG_SHAPE), BIG_SHAPE, ref.BATCH
