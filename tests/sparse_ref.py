"""Yardstick of the sparse 3-D convolution layers (catgrasp_amd/spconv.py): a seeded scene maker and a float64 restatement of the
layers' rules with dictionary lookups.  CPU only; numpy, and from tests/dense_ref.py the emulated fmaf and chain_order that conv_exact
is built on (that module imports torch and catgrasp_amd.folding, host code).
tests/test_sparse_ref_cpu.py pins the restatement against dense torch.nn.functional.conv3d / conv_transpose3d.

Rules restated (weights (k0, k1, k2, Cin, Cout), correlation, offsets in row-major (k0, k1, k2) order):
  subm     k = 3, padding 1: output i is input site i; offset kk reads the site at d + kk - 1.
  down     kernel 2, stride 2: out_shape = (s - 2)//2 + 1; inputs with a coordinate >= 2*out_shape are dropped; outputs are the
           distinct [b, d//2] of the rest in ascending linear key ((b*S0 + d0)*S1 + d1)*S2 + d2; offset kk reads the site at 2*o + kk.
  inverse  outputs are the strided layer's input sites; site x reads its parent x//2 through offset x % 2; dropped sites read nothing.
  conv     out[i] = bias + residual[i] + sum_k pro(x[nbr[i, k]]) @ W[k] over the entries that exist, pro(x) = max(x*scale + shift, 0).

conv_exact restates the kernel (csrc/sparse_conv.hip) itself, in float32, bit for bit: the contract of include/catgrasp_amd_sparse.h
("k ascending, absent entries skipped, one wave's fixed-order f32 sum") with the one order the kernel's MFMA steps fix.  Per output
element:
  prologue     p = fmax(f32(f32(x*scale) + shift), 0): two roundings (the library is built with -ffp-contract=off), and C's fmaxf, which
               returns 0 for a NaN argument;
  accumulator  starts at +0; for k = 0 .. K-1, for the rows whose nbr[:, k] >= 0, for c in dense_ref.chain_order(cin rounded up
               to 8) with c < cin: acc = fmaf(p[nbr[:, k], c], w[k, c, :], acc).  Step (q, j) of the kernel's v_mfma_f32_32x32x2_f32
               chain takes channel 8q + j from lanes 0..31 and then 8q + 4 + j from lanes 32..63, which is chain_order;
  epilogue     f32(f32(acc + bias_or_0) + residual_or_0).
"Rows skipped" and "rows gathered as zeros" give the same bits.  The kernel skips an offset only when no row of its 32-row tile has a
neighbour there; otherwise a row without one is gathered as zeros and runs through the chain, and so do the padded channels 6 and 7
of cin = 6 (against a clamped, finite weight).  The accumulator starts at +0, and round-to-nearest never produces -0 from it: a sum
that cancels exactly is +0, and x*w + acc is -0 only if both x*w and acc are (the inputs stay in the normal range: no product
underflows to -0).  fmaf(0, w, acc) is acc + (+-0), which is acc for every acc but -0.  So a zero row or channel leaves every bit of
the accumulator as it was, for finite w, and the model may skip what the kernel multiplies by zero.
"""
import functools

import numpy as np

from dense_ref import chain_order, fmaf

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


def prologue_f32(x, scale, shift, contract=False):
    """The kernel's prologue on float32: fmax(f32(f32(x*scale) + shift), 0), fmaxf's 0 for a NaN.  contract: one rounding (planted)."""
    x, scale, shift = (np.asarray(v, dtype=np.float32) for v in (x, scale, shift))
    with np.errstate(invalid='ignore'):
        return np.fmax(fmaf(x, scale, shift) if contract else (x * scale).astype(np.float32) + shift, np.float32(0))


def _chain(x, nbr, w, bias, scale, shift, residual, channels='mfma', contract=False, right_epilogue=False, k_descending=False):
    """conv_exact and its planted variants (tests/test_sparse_ref_cpu.py shows that each one changes bits)."""
    f32 = np.float32
    x = np.asarray(x, dtype=f32)
    w = np.asarray(w, dtype=f32).reshape(-1, w.shape[-2], w.shape[-1])
    K, cin, cout = w.shape
    assert K == nbr.shape[1] and cin == x.shape[1] and (scale is None) == (shift is None)
    with np.errstate(invalid='ignore'):
        if scale is not None:
            x = prologue_f32(x, scale, shift, contract)
        order = [c for c in chain_order((cin + 7) & ~7) if c < cin] if channels == 'mfma' else list(range(cin))
        acc = np.zeros((nbr.shape[0], cout), dtype=f32)
        for k in (range(K - 1, -1, -1) if k_descending else range(K)):
            rows = np.nonzero(nbr[:, k] >= 0)[0]
            if not len(rows):
                continue
            g, a = x[nbr[rows, k]], acc[rows]
            for c in order:
                a = fmaf(g[:, c, None], w[k, c][None, :], a)
            acc[rows] = a
        b = np.zeros(cout, dtype=f32) if bias is None else np.asarray(bias, dtype=f32)
        r = np.zeros_like(acc) if residual is None else np.asarray(residual, dtype=f32)
        out = acc + (b[None, :] + r) if right_epilogue else (acc + b[None, :]) + r
    assert out.dtype == f32
    return out


def conv_exact(x, nbr, w, bias=None, scale=None, shift=None, residual=None):
    """float32 (n_out, cout) with the bits of cg_sparse_conv (the module docstring states the chain)."""
    return _chain(x, nbr, w, bias, scale, shift, residual)


# ------------------------------------------------------------------------------------------------- grids at the edges
LARGE_SHAPE, LARGE_BATCH = (1201, 1301, 1401), 9          # 2,189,063,901 cells per item: item 0 crosses 2^31, item 1 crosses 2^32
LARGE_ITEMS = (0, 1, 8)                                   # coarse grid (600, 650, 700): every key of item 8 is above 2^31


def site_of_key(key, shape):
    """[b, d0, d1, d2] of a linear key"""
    r, d2 = divmod(int(key), shape[2])
    r, d1 = divmod(r, shape[1])
    b, d0 = divmod(r, shape[0])
    return [b, d0, d1, d2]


def _block(centre, shape):
    """The 3x3x3 block round a site, clipped to the grid."""
    b, c = centre[0], centre[1:]
    return {(b, d0, d1, d2) for d0 in range(max(c[0] - 1, 0), min(c[0] + 2, shape[0])) for d1 in range(max(c[1] - 1, 0), min(c[1] + 2, shape[1]))
            for d2 in range(max(c[2] - 1, 0), min(c[2] + 2, shape[2]))}


def large_centres():
    """The four block centres of large_scene(): the sites of the largest fine keys below 2^31 and 2^32, the far corner of the last
    item and the origin."""
    return [site_of_key(2 ** 31 - 1, LARGE_SHAPE), site_of_key(2 ** 32 - 1, LARGE_SHAPE), [LARGE_BATCH - 1] + [s - 1 for s in LARGE_SHAPE], [0, 0, 0, 0]]


@functools.lru_cache(maxsize=None)
def large_scene(seed=0, pairs=100):
    """-> indices (n, 4) int32 in batch LARGE_BATCH x LARGE_SHAPE, sites in items LARGE_ITEMS only, in a seeded random row order:
    a full 3x3x3 block round each of large_centres() and `pairs` random sites, each with one random neighbour."""
    rng = np.random.default_rng(seed)
    sites = set()
    for c in large_centres():
        sites |= _block(c, LARGE_SHAPE)
    for _ in range(pairs):
        b = int(rng.choice(LARGE_ITEMS))
        c = [int(rng.integers(s)) for s in LARGE_SHAPE]
        d = [int(np.clip(v + rng.integers(-1, 2), 0, s - 1)) for v, s in zip(c, LARGE_SHAPE)]
        sites |= {(b, *c), (b, *d)}
    out = np.array(sorted(sites), dtype=np.int32)
    return out[rng.permutation(len(out))]


def _shuffled(sites, seed):
    out = np.array(sorted(sites), dtype=np.int32).reshape(-1, 4)
    return out[np.random.default_rng(seed).permutation(len(out))]


def full_grid(batch, shape, seed=0):
    """Every site of the grid, in a seeded random row order."""
    return _shuffled([(b, d0, d1, d2) for b in range(batch) for d0 in range(shape[0]) for d1 in range(shape[1]) for d2 in range(shape[2])], seed)


# name -> (indices, spatial shape, batch size)
@functools.lru_cache(maxsize=None)
def edge_scene(name):
    if name == 'unit':                      # an axis of 1 everywhere: one site per item, no neighbour but itself, no strided layer
        return full_grid(3, (1, 1, 1)), (1, 1, 1), 3
    if name == 'two':                       # one strided output per item, every offset present
        return full_grid(2, (2, 2, 2)), (2, 2, 2), 2
    if name == 'three_two_five':            # item 0 full, item 1 a random half; d0 = 2 and d2 = 4 are dropped
        idx = full_grid(2, (3, 2, 5), seed=1)
        keep = (idx[:, 0] == 0) | (np.random.default_rng(2).random(len(idx)) < 0.5)
        return np.ascontiguousarray(idx[keep]), (3, 2, 5), 2
    if name == 'dense':                     # 240 rows, 2*3*4 interior sites per item with 27 of 27 neighbours
        return full_grid(2, (4, 5, 6), seed=3), (4, 5, 6), 2
    if name == 'all_dropped':               # every site has a coordinate equal to 2 = 2*out_shape: n_out = 0 with n_in = 38
        idx = full_grid(2, (3, 3, 3), seed=4)
        return np.ascontiguousarray(idx[(idx[:, 1:] == 2).any(1)]), (3, 3, 3), 2
    if name == 'mostly_dropped':            # 27 sites, one strided output: n_out*8 < n_in
        return full_grid(1, (3, 3, 3), seed=5), (3, 3, 3), 1
    if name == 'mostly_dropped_x20':        # 540 sites, 20 outputs: the 160 table threads fit one workgroup, the sites need three
        return full_grid(20, (3, 3, 3), seed=6), (3, 3, 3), 20
    if name == 'large':
        return large_scene(), LARGE_SHAPE, LARGE_BATCH
    raise KeyError(name)


EDGE_SCENES = ('unit', 'two', 'three_two_five', 'dense', 'all_dropped', 'mostly_dropped', 'mostly_dropped_x20', 'large')


def with_dropped_duplicate(name):
    """-> (indices, position): the scene with the row of the last site in key order overwritten by the site before it (both dropped
    by the strided layer in the mostly_dropped scenes), and the position of that pair among the sorted keys."""
    idx, shape, _ = edge_scene(name)
    order = np.argsort(linear_key(idx, shape))
    out = idx.copy()
    out[order[-1]] = out[order[-2]]
    return out, len(idx) - 2
