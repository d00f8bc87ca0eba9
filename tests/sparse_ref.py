"""Yardstick of the sparse 3-D convolution layers (catgrasp_amd/spconv.py): a seeded scene maker and a float64 restatement of the
layers' rules with dictionary lookups.  numpy only, CPU only.  tests/test_sparse_ref_cpu.py pins the restatement against dense
torch.nn.functional.conv3d / conv_transpose3d.

Rules restated (weights (k0, k1, k2, Cin, Cout), correlation, offsets in row-major (k0, k1, k2) order):
  subm     k = 3, padding 1: output i is input site i; offset kk reads the site at d + kk - 1.
  down     kernel 2, stride 2: out_shape = (s - 2)//2 + 1; inputs with a coordinate >= 2*out_shape are dropped; outputs are the
           distinct [b, d//2] of the rest in ascending linear key ((b*S0 + d0)*S1 + d1)*S2 + d2; offset kk reads the site at 2*o + kk.
  inverse  outputs are the strided layer's input sites; site x reads its parent x//2 through offset x % 2; dropped sites read nothing.
  conv     out[i] = bias + residual[i] + sum_k pro(x[nbr[i, k]]) @ W[k] over the entries that exist, pro(x) = max(x*scale + shift, 0).
"""
import functools

import numpy as np

SHAPE = (9, 12, 17)          # non-cubic, two odd axes
BATCH = 2


def _special_sites():
    """The sites every full scene must hold (tests/test_sparse_conv_gpu.py lists why)."""
    s = [[0, 0, 0, 0], [1, 8, 11, 16],                          # the two corners
         [0, 3, 4, 16], [0, 3, 5, 0],                            # end of one row, start of the next: not neighbours
         [0, 5, 6, 7], [1, 5, 6, 7],                             # the same position in both batch items: not neighbours
         [1, 2, 9, 3]]                                           # isolated (the random fill keeps away from it)
    s += [[0, 1 + a, 1 + b, 10 + c] for a in range(3) for b in range(3) for c in range(3)]           # a full 3x3x3 block
    s += [[1, 8, 2, 5], [1, 8, 3, 5], [0, 4, 7, 16], [0, 4, 6, 16], [1, 8, 10, 16], [0, 8, 0, 16]]   # odd last coordinates: dropped by `down`
    return s


@functools.lru_cache(maxsize=None)
def scene(n=299, seed=0, batch=BATCH, shape=SHAPE, special=True, only_item=None):
    """-> indices (n, 4) int32, distinct sites in a seeded random row order.  special: includes _special_sites() (n >= their count).
    The random fill is a surface-like sheet (a noisy plane per batch item) so most 3x3x3 offsets are absent, as on real scenes.
    only_item: every site in that batch item (the other one stays empty)."""
    rng = np.random.default_rng(seed)
    sites = {tuple(s) for s in _special_sites()} if special else set()
    assert len(sites) <= n
    iso = np.array([1, 2, 9, 3])
    while len(sites) < n:
        b = only_item if only_item is not None else int(rng.integers(batch))
        d1, d2 = int(rng.integers(shape[1])), int(rng.integers(shape[2]))
        d0 = int(np.clip(round(shape[0] / 2 + 1.5 * np.sin(d1 / 3.0 + b) + 1.5 * np.cos(d2 / 4.0) + rng.normal(0, 0.8)), 0, shape[0] - 1))
        c = (b, d0, d1, d2)
        if special and b == iso[0] and max(abs(np.array(c[1:]) - iso[1:])) <= 1:
            continue
        sites.add(c)
    out = np.array(sorted(sites), dtype=np.int32)
    return out[rng.permutation(len(out))]


def features(n, c, seed=1):
    return np.random.default_rng(seed).uniform(-1, 1, (n, c)).astype(np.float32)


def weights(k, cin, cout, seed=2):
    """Uniform in +-sqrt(3/Cin): outputs of order one; and a bias of order one."""
    rng = np.random.default_rng(seed)
    a = np.sqrt(3.0 / cin)
    return rng.uniform(-a, a, (k, k, k, cin, cout)).astype(np.float32), rng.uniform(-1, 1, (cout,)).astype(np.float32)


def bn_params(c, seed=3):
    """(scale, shift) of order one with both signs, so the ReLU cuts about half of the values."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, c).astype(np.float32) * rng.choice([-1, 1], c).astype(np.float32), rng.uniform(-0.5, 0.5, c).astype(np.float32)


def linear_key(idx, shape):
    idx = np.asarray(idx, dtype=np.int64)
    return ((idx[:, 0] * shape[0] + idx[:, 1]) * shape[1] + idx[:, 2]) * shape[2] + idx[:, 3]


def _table(indices):
    t = {tuple(int(v) for v in row): i for i, row in enumerate(indices)}
    assert len(t) == len(indices), 'duplicate site'
    return t


def subm_rules(indices, shape):
    """-> nbr (n, 27) int32"""
    t = _table(indices)
    nbr = np.full((len(indices), 27), -1, dtype=np.int32)
    for i, (b, d0, d1, d2) in enumerate(indices.tolist()):
        for k in range(27):
            nbr[i, k] = t.get((b, d0 + k // 9 - 1, d1 + (k // 3) % 3 - 1, d2 + k % 3 - 1), -1)       # a site outside the grid is not in the table
    return nbr


def down_rules(indices, shape):
    """-> (out_indices (m, 4) int32 in key order, nbr (m, 8) int32, out_shape, dropped (n,) bool)"""
    out_shape = tuple((s - 2) // 2 + 1 for s in shape)
    dropped = (indices[:, 1:] >= 2 * np.array(out_shape)).any(1)
    parents = {(int(r[0]), int(r[1]) // 2, int(r[2]) // 2, int(r[3]) // 2) for r, d in zip(indices, dropped) if not d}
    out = np.array(sorted(parents), dtype=np.int32).reshape(-1, 4)
    out = out[np.argsort(linear_key(out, out_shape), kind='stable')]
    t = _table(indices)
    nbr = np.full((len(out), 8), -1, dtype=np.int32)
    for o, (b, p0, p1, p2) in enumerate(out.tolist()):
        for k in range(8):
            nbr[o, k] = t.get((b, 2 * p0 + (k >> 2), 2 * p1 + ((k >> 1) & 1), 2 * p2 + (k & 1)), -1)
    return out, nbr, out_shape, dropped


def inverse_rules(indices, out_indices, shape):
    """-> nbr (n, 8) int32: the parent's row at offset (d0%2, d1%2, d2%2), -1 elsewhere and for dropped sites"""
    t = _table(out_indices)
    nbr = np.full((len(indices), 8), -1, dtype=np.int32)
    for i, (b, d0, d1, d2) in enumerate(indices.tolist()):
        nbr[i, ((d0 & 1) << 2) | ((d1 & 1) << 1) | (d2 & 1)] = t.get((b, d0 // 2, d1 // 2, d2 // 2), -1)
    return nbr


def conv(x, nbr, w, bias=None, scale=None, shift=None, residual=None):
    """float64.  w: (k0, k1, k2, Cin, Cout) or (K, Cin, Cout)."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64).reshape(-1, w.shape[-2], w.shape[-1])
    assert w.shape[0] == nbr.shape[1] and w.shape[1] == x.shape[1]
    if scale is not None:
        x = np.maximum(x * np.asarray(scale, dtype=np.float64) + np.asarray(shift, dtype=np.float64), 0.0)
    out = np.zeros((nbr.shape[0], w.shape[2]))
    for k in range(w.shape[0]):
        rows = np.nonzero(nbr[:, k] >= 0)[0]
        out[rows] += x[nbr[rows, k]] @ w[k]
    if bias is not None:
        out += np.asarray(bias, dtype=np.float64)
    if residual is not None:
        out += np.asarray(residual, dtype=np.float64)
    return out


def dense(indices, x, batch, shape):
    """(batch, C, s0, s1, s2) float64, zeros at inactive sites"""
    out = np.zeros((batch,) + tuple(shape) + (x.shape[1],))
    out[indices[:, 0], indices[:, 1], indices[:, 2], indices[:, 3]] = x
    return np.moveaxis(out, -1, 1)
