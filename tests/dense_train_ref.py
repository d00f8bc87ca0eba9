"""Yardstick of the dense layers' gradients and of PointNetSeg's per-point head in training mode (catgrasp_amd/dense_autograd.py,
csrc/dense_train.hip).  CPU only: numpy, tests/dense_ref.py for the emulated fmaf and the MFMA k order, tests/bn_ref.py for BatchNorm.
tests/test_dense_train_ref_cpu.py pins it against torch autograd in float64.

linear_grads64      float64 (dW, db, dX) of y = x W^T + b, and group_sums64 for the gradient of row_bias.
head_forward64 /    the head  conv1 (split: g Wg^T + b1 per cloud, pointfeat Wp^T per point) - bn - relu - conv2 - bn - relu - conv3 -
head_backward64     bn - relu - conv4  in float64 with bn_ref's batch-statistics formulas, and every gradient of it.
wgrad_exact         float32, the bits of cg_dense_wgrad: the rows in chunks of CG_DENSE_GRAD_ROWS; per chunk and element one fmaf chain
                    from +0 over the chunk's rows ascending (the bias: fmaf(1, dy, p)); the partial of chunk 0, then the others added
                    in ascending order.  Planted: rows = n is one flat chain, descending runs every chunk from its last row.
group_sums_exact    float32, the bits of cg_dense_group_sums: bn_ref.column_sum (64-row segments, 1024-row chunks) over each group's
                    own rows.  Planted: global_tree cuts the segments and chunks from row 0 of the whole array, not of the group.
dgrad_exact         float32, the bits of cg_dense_dgrad: per element one fmaf chain from +0 over the columns of dy in dgrad_order:
                    dense_ref.chain_order of cout rounded up to 8, columns >= cout left out (cout = 300: a tail of four).
"""
import functools
import re

import numpy as np

import bn_ref
from catgrasp_amd import _lib
from dense_ref import chain_order, fma_chain, fmaf, gemm_f32_epilogue  # noqa: F401  (gemm_f32_epilogue: the forward's epilogue)

with open(_lib.DENSE_HEADER_PATH) as _f:
    ROWS = int(re.search(r'^#define CG_DENSE_GRAD_ROWS (\d+)$', _f.read(), flags=re.M).group(1))
f32 = np.float32
rel_err = bn_ref.rel_err
BAR = 1e-4          # the suite's per-element bar: |got - ref| <= BAR * max(1, |ref|)


# ------------------------------------------------------------------------------------------------------------------ float64
def linear_grads64(x, w, dy):
    x, w, dy = (np.asarray(a, dtype=np.float64) for a in (x, w, dy))
    return dy.T @ x, dy.sum(0), dy @ w


def group_sums64(dy, rows_per_group):
    dy = np.asarray(dy, dtype=np.float64)
    return dy.reshape(-1, rows_per_group, dy.shape[1]).sum(1)


def head_forward64(g, pf, P):
    """g (B, Cg), pf (B, N, Cp), P: w1..w4, b1..b4, gamma1..3, beta1..3 -> record with 'logits' (B, N, n_out), the layer inputs h0..h3
    (rows) and the BatchNorm inputs z1..z3."""
    g, pf = np.asarray(g, dtype=np.float64), np.asarray(pf, dtype=np.float64)
    P = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}
    B, N, cp = pf.shape
    cg = g.shape[1]
    rec = dict(B=B, N=N, cg=cg, g=g, h0=pf.reshape(B * N, cp))
    r = g @ P['w1'][:, :cg].T + P['b1']
    z = rec['h0'] @ P['w1'][:, cg:].T + np.repeat(r, N, axis=0)
    for i in (1, 2, 3):
        rec[f'z{i}'] = z
        fw = bn_ref.forward64(z, P[f'gamma{i}'], P[f'beta{i}'])
        rec[f'pre{i}'], rec[f'h{i}'], rec[f'mean{i}'], rec[f'var{i}'] = fw['z'], fw['y'], fw['mean'], fw['var']
        z = fw['y'] @ P[f'w{i + 1}'].T + P[f'b{i + 1}']
    rec['logits'] = z.reshape(B, N, -1)
    return rec


def head_backward64(rec, P, dlogits):
    """-> dict of float64 gradients: g, pf, w1..w4, b1..b4, gamma1..3, beta1..3."""
    P = {k: np.asarray(v, dtype=np.float64) for k, v in P.items()}
    B, N, cg = rec['B'], rec['N'], rec['cg']
    G = {}
    d = np.asarray(dlogits, dtype=np.float64).reshape(B * N, -1)
    for i in (3, 2, 1):
        G[f'w{i + 1}'], G[f'b{i + 1}'], dh = linear_grads64(rec[f'h{i}'], P[f'w{i + 1}'], d)
        d, G[f'gamma{i}'], G[f'beta{i}'] = bn_ref.backward64(rec[f'z{i}'], dh, P[f'gamma{i}'], mask=rec[f'pre{i}'] > 0)
    dwp, _, dpf = linear_grads64(rec['h0'], P['w1'][:, cg:], d)
    dr = group_sums64(d, N)
    dwg, G['b1'], G['g'] = linear_grads64(rec['g'], P['w1'][:, :cg], dr)
    G['w1'] = np.concatenate([dwg, dwp], axis=1)
    G['pf'] = dpf.reshape(B, N, -1)
    return G


# ------------------------------------------------------------------------------------------------------------------ float32
_LOW29, _HALF29, _ABS = np.int64(0x1FFFFFFF), np.int64(0x10000000), np.int64(0x7FFFFFFFFFFFFFFF)
_TINY, _HUGE = np.float64(2.0 ** -120).view(np.int64), np.float64(2.0 ** 127).view(np.int64)


def fmaf_step(a, b, acc):
    """dense_ref.fmaf(a, b, acc) for float32 VALUES held in float64 arrays (the chains below run thousands of steps, and the casts
    are most of fmaf's cost).  a * b is exact; s = fl64(a * b + acc) rounded once more to float32 is the correctly rounded fma unless s
    sits exactly on a float32 midpoint (its low 29 mantissa bits are 1 0 ... 0), or in the range where float32 is subnormal or
    overflows; a step with any such element is recomputed by dense_ref.fmaf itself."""
    s = a * b + acc
    bits = s.view(np.int64)
    mag = bits & _ABS
    if ((bits & _LOW29) == _HALF29).any() or ((mag < _TINY) & (mag != 0)).any() or (mag >= _HUGE).any():
        return fmaf(a.astype(f32), b.astype(f32), acc.astype(f32)).astype(np.float64)
    return s.astype(f32).astype(np.float64)


def wgrad_exact(x, dy, rows=ROWS, descending=False):
    """float32 (dW (Cout, Cin), db (Cout,)) with the bits of cg_dense_wgrad."""
    x, dy = np.asarray(x, dtype=f32).astype(np.float64), np.asarray(dy, dtype=f32).astype(np.float64)
    n, cin = x.shape
    cout = dy.shape[1]
    one = np.ones(cout)
    dw = db = None
    for lo in range(0, n, max(rows, 1)):
        p, pb = np.zeros((cout, cin)), np.zeros(cout)
        chunk = range(lo, min(lo + rows, n))
        for i in (reversed(chunk) if descending else chunk):
            pb = fmaf_step(one, dy[i], pb)
            p = fmaf_step(dy[i][:, None], x[i][None, :], p)
        p, pb = p.astype(f32), pb.astype(f32)
        dw, db = (p, pb) if lo == 0 else (dw + p, db + pb)
    assert dw.dtype == f32 and db.dtype == f32
    return dw, db


def group_sums_exact(dy, rows_per_group, global_tree=False):
    """float32 (G, C) with the bits of cg_dense_group_sums."""
    dy = np.asarray(dy, dtype=f32)
    n, c = dy.shape
    out = np.zeros((n // rows_per_group, c), f32)
    for gi in range(n // rows_per_group):
        lo, hi = gi * rows_per_group, (gi + 1) * rows_per_group
        if not global_tree:
            out[gi] = bn_ref.column_sum(dy[lo:hi])
            continue
        # planted: segments and chunks of the whole array's rows, each clipped to the group
        total = None
        for c0 in range(lo - lo % bn_ref.ROWS, hi, bn_ref.ROWS):
            chunk = None
            for s0 in range(c0, min(c0 + bn_ref.ROWS, hi), bn_ref.SEG):
                a, b = max(s0, lo), min(s0 + bn_ref.SEG, hi)
                if a >= b:
                    continue
                p = np.zeros(c, f32)
                for i in range(a, b):
                    p = p + dy[i]
                chunk = p if chunk is None else chunk + p
            if chunk is not None:
                total = chunk if total is None else total + chunk
        out[gi] = total
    return out


def dgrad_order(cout):
    """Column order of one element's chain in cg_dense_dgrad."""
    return [k for k in chain_order((cout + 7) // 8 * 8) if k < cout]


def dgrad_exact(dy, w, order=None):
    """float32 dX (n, Cin) with the bits of cg_dense_dgrad; w (Cout, Cin)."""
    dy, w = np.asarray(dy, dtype=f32).astype(np.float64), np.asarray(w, dtype=f32).astype(np.float64)
    acc = np.zeros((dy.shape[0], w.shape[1]))
    for k in (dgrad_order(w.shape[0]) if order is None else order):          # dense_ref.fma_chain(dy, w.T, order), on fmaf_step
        acc = fmaf_step(dy[:, k, None], w[None, k, :], acc)
    return acc.astype(f32)


# ------------------------------------------------------------------------------------------------------------------ inputs
def dy_for(n, cout, seed=7):
    """Uniform in +-sqrt(3 / n): weight gradients of order one (sparse_grad_ref.dy_for's scale)."""
    a = np.sqrt(3.0 / max(n, 1))
    return np.random.default_rng(seed).uniform(-a, a, (n, cout)).astype(f32)


@functools.lru_cache(maxsize=None)
def dense_case(n, cin, cout, seed=0):
    """Inputs, float64 gradients and the float32 restatements of one shape, computed once and shared, read-only."""
    rng = np.random.default_rng(100003 * cin + 1009 * cout + n + seed)
    x = rng.uniform(-1, 1, (n, cin)).astype(f32)
    w = rng.uniform(-1, 1, (cout, cin)).astype(f32) * f32(np.sqrt(3.0 / cout))
    dy = dy_for(n, cout, seed=seed + 7)
    dw64, db64, dx64 = linear_grads64(x, w, dy)
    dw32, db32 = wgrad_exact(x, dy)
    out = dict(x=x, w=w, dy=dy, dw64=dw64, db64=db64, dx64=dx64, dw32=dw32, db32=db32, dx32=dgrad_exact(dy, w))
    for a in out.values():
        a.setflags(write=False)
    return out


HEAD_WIDTHS = dict(cg=32, cp=16, hidden=(32, 16, 16), n_out=12)


def head_params(cg, cp, hidden, n_out, seed=0):
    rng = np.random.default_rng(seed)
    widths = [cg + cp, *hidden, n_out]
    P = {}
    for i in range(4):
        a = np.sqrt(3.0 / widths[i])
        P[f'w{i + 1}'] = rng.uniform(-a, a, (widths[i + 1], widths[i])).astype(f32)
        P[f'b{i + 1}'] = rng.uniform(-0.5, 0.5, widths[i + 1]).astype(f32)
    for i in range(3):
        P[f'gamma{i + 1}'] = (rng.uniform(0.5, 1.5, hidden[i]) * rng.choice([-1.0, 1.0], hidden[i])).astype(f32)
        P[f'beta{i + 1}'] = rng.uniform(-0.5, 0.5, hidden[i]).astype(f32)
    return P


@functools.lru_cache(maxsize=None)
def head_case(B, N, seed=0, margin=bn_ref.MARGIN):
    """-> dict(g, pf, P, dlogits, rec, grads): a head of HEAD_WIDTHS whose float64 pre-activations (all three BatchNorm outputs) lie at
    least `margin` from zero, so that float32 and float64 agree on every ReLU mask: as bn_ref.nudge, the per-point features of the rows
    that own a near-zero pre-activation are moved until there is none."""
    W = HEAD_WIDTHS
    rng = np.random.default_rng(7919 * B + N + seed)
    P = head_params(W['cg'], W['cp'], W['hidden'], W['n_out'], seed=seed)
    g = rng.normal(0, 1, (B, W['cg'])).astype(f32)
    pf = rng.normal(0, 1, (B, N, W['cp'])).astype(f32)
    for _ in range(200):
        rec = head_forward64(g, pf, P)
        near = np.zeros(B * N, bool)
        for i in (1, 2, 3):
            near |= (np.abs(rec[f'pre{i}']) < margin).any(axis=1)
        if not near.any():
            break
        pf.reshape(B * N, -1)[near] += rng.normal(0, 0.05, (int(near.sum()), W['cp'])).astype(f32)
    else:
        raise AssertionError('the inputs cannot be moved off the ReLU edges')
    dlogits = dy_for(B * N, W['n_out'], seed=seed + 11).reshape(B, N, -1)
    grads = head_backward64(rec, P, dlogits)
    for a in (g, pf, dlogits, *P.values()):
        a.setflags(write=False)
    return dict(g=g, pf=pf, P=P, dlogits=dlogits, rec=rec, grads=grads)
