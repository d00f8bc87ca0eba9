"""Yardstick of BatchNorm in batch-statistics mode + ReLU (catgrasp_amd/batchnorm.py, csrc/batchnorm_train.hip).  CPU only, numpy.
tests/test_bn_ref_cpu.py pins it against torch autograd in float64.

forward64, backward64   the explicit formulas in float64.
column_sum              float32, the tree of include/catgrasp_amd_bn.h: 64-row segments (one chain each, from +0, ascending rows), the
                        segments of a 1024-row chunk added in ascending order, the chunks added in ascending order.  Vectorised over
                        channels and segments: 64 loop steps.
forward32, backward32   float32, every operation of the header's contract rounded separately: the bits of the kernels.  Planted
                        variants: flat (one chain over all rows), descending (rows of a segment from the last to the first),
                        one_pass (var = E[x^2] - mean^2), contract (the activation as one fmaf).
inputs                  seeded (x, gamma, beta, dy), x nudged until no float64 pre-activation lies within MARGIN of zero.
"""
import functools
import re

import numpy as np

from catgrasp_amd import _lib
from dense_ref import fmaf

with open(_lib.BN_HEADER_PATH) as _f:
    _text = _f.read()
SEG = int(re.search(r'^#define CG_BN_SEG (\d+)$', _text, flags=re.M).group(1))
ROWS = int(re.search(r'^#define CG_BN_ROWS (\d+)$', _text, flags=re.M).group(1))
EPS = 1e-5
MARGIN = 1e-3
f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ float64
def forward64(x, gamma, beta, eps=EPS):
    x, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (x, gamma, beta))
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    z = (x - mean) * invstd * gamma + beta
    return dict(y=np.maximum(z, 0.0), z=z, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift)


def backward64(x, dy, gamma, eps=EPS, mask=None, beta=None):
    """-> (dx, dgamma, dbeta).  mask: the ReLU's (n, c) bool; by default float64's own (needs beta)."""
    x, dy, gamma = (np.asarray(a, dtype=np.float64) for a in (x, dy, gamma))
    n = x.shape[0]
    mean = x.mean(0)
    invstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(0) + eps)
    xhat = (x - mean) * invstd
    if mask is None:
        mask = xhat * gamma + np.asarray(beta, dtype=np.float64) > 0
    g = np.where(mask, dy, 0.0)
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    return gamma * invstd * (g - dbeta / n - xhat * dgamma / n), dgamma, dbeta


# ------------------------------------------------------------------------------------------------------------------ float32
def column_sum(t, u=None, seg=SEG, rows=ROWS, descending=False):
    """S over the rows of t (n, c) float32 with the chain step p + t, or, with u, fmaf(t, u, p)."""
    t = np.asarray(t)
    assert t.dtype == f32 and (u is None or (u.dtype == f32 and u.shape == t.shape)) and rows % seg == 0
    n, c = t.shape
    nseg = -(-n // seg)
    pad = lambda a: np.concatenate([a, np.zeros((nseg * seg - n, c), f32)]).reshape(nseg, seg, c)
    T, U = pad(t), None if u is None else pad(u)
    valid = (np.arange(nseg * seg) < n).reshape(nseg, seg)
    p = np.zeros((nseg, c), f32)
    for i in (reversed(range(seg)) if descending else range(seg)):
        new = p + T[:, i] if U is None else fmaf(T[:, i], U[:, i], p)
        p = np.where(valid[:, i, None], new, p)
    per = rows // seg
    total = None
    for k in range(0, nseg, per):
        chunk = p[k]
        for s in range(k + 1, min(k + per, nseg)):
            chunk = chunk + p[s]
        total = chunk if total is None else total + chunk
    assert total.dtype == f32
    return total


def forward32(x, gamma, beta, eps=EPS, flat=False, descending=False, one_pass=False, contract=False):
    x, gamma, beta = (np.asarray(a, dtype=f32) for a in (x, gamma, beta))
    n = x.shape[0]
    tree = dict(seg=n, rows=n) if flat else dict(descending=descending)
    nf = f32(n)
    mean = column_sum(x, **tree) / nf
    if one_pass:
        var = column_sum(x, x, **tree) / nf - mean * mean
    else:
        d = x - mean
        var = column_sum(d, d, **tree) / nf
    invstd = f32(1) / np.sqrt(var + f32(eps))
    scale = gamma * invstd
    shift = beta - mean * scale
    z = fmaf(x, scale, shift) if contract else x * scale + shift
    out = dict(y=np.maximum(z, f32(0)), z=z, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift)
    assert all(v.dtype == f32 for v in out.values())
    return out


def backward32(x, dy, fwd, flat=False, descending=False):
    """fwd: forward32's record (mean, invstd, scale, shift).  -> (dx, dgamma, dbeta) float32."""
    x, dy = np.asarray(x, dtype=f32), np.asarray(dy, dtype=f32)
    n = x.shape[0]
    tree = dict(seg=n, rows=n) if flat else dict(descending=descending)
    z = x * fwd['scale'] + fwd['shift']
    g = np.where(z > 0, dy, f32(0))
    xhat = (x - fwd['mean']) * fwd['invstd']
    dbeta = column_sum(g, **tree)
    dgamma = column_sum(g, xhat, **tree)
    k1, k2 = dbeta / f32(n), dgamma / f32(n)
    dx = fwd['scale'] * ((g - k1) - xhat * k2)
    assert dx.dtype == f32 and dgamma.dtype == f32 and dbeta.dtype == f32
    return dx, dgamma, dbeta


# ------------------------------------------------------------------------------------------------------------------ inputs
def nudge(x, gamma, beta, eps=EPS, margin=MARGIN):
    """Moves the entries of x (float32) whose float64 pre-activation lies within `margin` of zero until there is none."""
    x = np.array(x, dtype=f32)
    for _ in range(100):
        near = np.abs(forward64(x, gamma, beta, eps)['z']) < margin
        if not near.any():
            return x
        x[near] += f32(0.02)
    raise AssertionError('the inputs cannot be moved off the ReLU edge')


@functools.lru_cache(maxsize=None)
def inputs(n, c, seed=0, offset=0.0, constant=False):
    """-> (x (n, c), gamma, beta, dy) float32, read-only.  Channel means within +-2, deviations 0.5 .. 2, gamma of both signs in
    0.5 .. 1.5, beta within 0.5, dy uniform in +-1.  offset: column 0 gets mean `offset` and deviation 1.  constant: column 1 is constant
    (it is left out of the nudge: its pre-activation is beta)."""
    rng = np.random.default_rng(1000 * c + n + seed)
    x = (rng.normal(0, 1, (n, c)) * rng.uniform(0.5, 2.0, c) + rng.uniform(-2, 2, c)).astype(f32)
    if offset:
        x[:, 0] = (offset + rng.normal(0, 1, n)).astype(f32)
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(f32)
    beta = rng.uniform(-0.5, 0.5, c).astype(f32)
    if constant:
        x[:, 1] = f32(0.75)
        beta[1] = f32(0.25)
    x = nudge(x, gamma, beta)
    dy = rng.uniform(-1, 1, (n, c)).astype(f32)
    for a in (x, gamma, beta, dy):
        a.setflags(write=False)
    return x, gamma, beta, dy


@functools.lru_cache(maxsize=None)
def case(n, c, **kw):
    """Inputs, the float64 results and the float32 restatement of one shape, computed once and shared: dict(x, gamma, beta, dy, f64, dx64,
    dgamma64, dbeta64, f32, dx32, dgamma32, dbeta32)."""
    x, gamma, beta, dy = inputs(n, c, **kw)
    f64 = forward64(x, gamma, beta)
    assert np.abs(f64['z']).min() >= MARGIN                        # float32 and float64 agree on every mask
    dx64, dgamma64, dbeta64 = backward64(x, dy, gamma, beta=beta)
    r32 = forward32(x, gamma, beta)
    assert np.array_equal(r32['z'] > 0, f64['z'] > 0)
    dx32, dgamma32, dbeta32 = backward32(x, dy, r32)
    return dict(x=x, gamma=gamma, beta=beta, dy=dy, f64=f64, dx64=dx64, dgamma64=dgamma64, dbeta64=dbeta64, f32=r32, dx32=dx32,
                dgamma32=dgamma32, dbeta32=dbeta32)


def rel_err(got, want):
    """max |got - want| / max(1, |want|), the project's per-element measure."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max(initial=0.0))
