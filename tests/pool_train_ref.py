"""Yardstick of the closed-form training of PointNet's pooled layer conv(k = 1) + BatchNorm (batch statistics) + [ReLU] + max over the points
(catgrasp_amd/pool_autograd.py, csrc/pool_train.hip).  CPU only: numpy, tests/dense_ref.py for the MFMA k order, tests/dense_train_ref.py
for the fast emulated fmaf.  tests/test_pool_train_ref_cpu.py pins it against torch autograd in float64.

forward64 / backward64   the closed form in float64: statistics from xbar and the centred Gram matrix S, the extremum by the sign of
                         gamma, the gradients without any (M, C) gradient tensor.  backward64 takes idx and the ReLU mask as arguments:
                         the tests pass the exact side's, so that the yardstick does not depend on sub-rounding near-ties.
                         Planted: wrong_sign (max where gamma < 0), drop_zhat (the zhat term of dW left out), bias_grad (a conv-bias
                         gradient sum_b e scale instead of 0).
autograd64               torch autograd in float64 through conv -> batch_norm -> [relu] -> max, what forward64 / backward64 are proved on.
z_exact                  float32, the bits of cg_gemm_bias_act: dense_ref.chain_order's fmaf chain, the bias added once after it.
extrema_exact            max / min by the sign of gamma and the FIRST index that attains it.  Planted: last (ties to the larger index).
gather_exact             the bits of cg_pool_wgrad_gather: one fmaf chain over b ascending.
scatter_exact            the bits of cg_pool_dgrad_scatter: per row fmaf(coef, W[c], dx) in ascending c.
var_gram32 / var_sweep32 / var_onepass32   float32 emulations of the routes to the variance (from S; the sum of (z - mean)^2;
                         E[z^2] - mean^2), for the offset case and the two-row case.
case                     inputs with gamma of both signs and one exact zero, one planted tie (two identical points in cloud 0), the
                         runner-up gaps and the ReLU pre-activations of the un-planted pairs at least MARGIN from the edge.
"""
import functools

import numpy as np

import bn_ref
from dense_ref import chain_order
from dense_train_ref import BAR, fmaf_step, rel_err  # noqa: F401  (BAR, rel_err: the bar of the GPU tests)

f32 = np.float32
EPS = 1e-5
MARGIN = bn_ref.MARGIN


# ------------------------------------------------------------------------------------------------------------------ float64
def stats64(x, w, b, gamma, beta, eps=EPS):
    x, w, b, gamma, beta = (np.asarray(a, dtype=np.float64) for a in (x, w, b, gamma, beta))
    B, N, cin = x.shape
    m = B * N
    x2 = x.reshape(m, cin)
    xbar = x2.mean(0)
    xc = x2 - xbar
    s = xc.T @ xc
    mean = w @ xbar + b
    var = np.maximum(np.einsum('ck,kj,cj->c', w, s, w) / m, 0.0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    return dict(x=x, w=w, b=b, gamma=gamma, beta=beta, m=m, xbar=xbar, s=s, mean=mean, var=var, invstd=invstd, scale=scale,
                shift=beta - mean * scale, z=(x2 @ w.T + b).reshape(B, N, -1))


def forward64(x, w, b, gamma, beta, relu, eps=EPS, idx=None, wrong_sign=False):
    """-> record with out (B, C), pre (before the ReLU), zsel, idx and the statistics.  idx: take z at these indices instead of float64's
    own extremum."""
    r = stats64(x, w, b, gamma, beta, eps)
    z = r['z']
    if idx is None:
        take_max = np.ones_like(r['gamma'], bool) if wrong_sign else r['gamma'] >= 0
        idx = np.where(take_max[None, :], z.argmax(1), z.argmin(1))
    r['idx'] = np.asarray(idx)
    r['zsel'] = np.take_along_axis(z, r['idx'][:, None, :], axis=1)[:, 0, :]
    r['pre'] = r['zsel'] * r['scale'] + r['shift']
    r['out'] = np.maximum(r['pre'], 0.0) if relu else r['pre']
    r['relu'] = relu
    return r


def backward64(r, dout, mask=None, drop_zhat=False, bias_grad=False):
    """-> dict(x, w, b, gamma, beta) of float64 gradients for the record r of forward64; mask: the ReLU's (B, C) bool (default r's own)."""
    dout = np.asarray(dout, dtype=np.float64)
    x, w, m, idx = r['x'], r['w'], r['m'], r['idx']
    B, N, cin = x.shape
    if mask is None:
        mask = r['pre'] > 0
    e = np.where(mask, dout, 0.0) if r['relu'] else dout
    zhat = (r['zsel'] - r['mean']) * r['invstd']
    dbeta = e.sum(0)
    dgamma = (e * zhat).sum(0)
    u = r['scale'] * r['invstd'] * dgamma / m
    coef = e * r['scale']
    xsel = x[np.arange(B)[:, None], idx]                                    # (B, C, cin)
    dw = np.einsum('bc,bck->ck', coef, xsel) - (r['scale'] * dbeta)[:, None] * r['xbar'][None, :]
    if not drop_zhat:
        dw = dw - u[:, None] * (w @ r['s'])
    g = w.T @ (u[:, None] * w)
    v = (r['scale'] * dbeta / m) @ w
    dx = (-(x.reshape(m, cin) - r['xbar']) @ g - v).reshape(B, N, cin).copy()
    for bi in range(B):
        np.add.at(dx[bi], idx[bi], coef[bi][:, None] * w)
    db = coef.sum(0) if bias_grad else np.zeros_like(dbeta)
    return dict(x=dx, w=dw, b=db, gamma=dgamma, beta=dbeta)


def autograd64(x, w, b, gamma, beta, relu, dout, eps=EPS):
    """torch autograd in float64 through conv1d -> batch_norm (training) -> [relu] -> max over the points."""
    import torch
    import torch.nn.functional as F
    t = {k: torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for k, v in dict(x=x, w=w, b=b, gamma=gamma, beta=beta).items()}
    y = F.conv1d(t['x'].transpose(1, 2), t['w'][:, :, None], t['b'])
    y = F.batch_norm(y, None, None, t['gamma'], t['beta'], True, 0.1, eps)
    out = (F.relu(y) if relu else y).max(dim=2)[0]
    out.backward(torch.tensor(np.asarray(dout, dtype=np.float64)))
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in t.items()}


# ------------------------------------------------------------------------------------------------------------------ float32
def z_exact(x, w, b):
    """(B, N, Cin), (C, Cin), (C) or None -> float32 (B, N, C) with the bits of cg_gemm_bias_act."""
    x, w = np.asarray(x, dtype=f32), np.asarray(w, dtype=f32)
    B, N, cin = x.shape
    x2, w64 = x.reshape(B * N, cin).astype(np.float64), w.astype(np.float64)
    acc = np.zeros((B * N, w.shape[0]))
    for k in chain_order(cin):
        acc = fmaf_step(x2[:, k, None], w64[None, :, k], acc)
    bias = np.zeros(w.shape[0], f32) if b is None else np.asarray(b, dtype=f32)
    return (acc.astype(f32) + bias[None, :]).astype(f32).reshape(B, N, -1)


def extrema_exact(z, sign, last=False):
    """z (B, N, C) float32, sign (C) -> (zsel (B, C) float32, idx (B, C) int32): max where sign >= 0, min otherwise, first occurrence."""
    z = np.asarray(z)
    N = z.shape[1]
    take_max = np.asarray(sign) >= 0
    if last:
        imax, imin = N - 1 - z[:, ::-1].argmax(1), N - 1 - z[:, ::-1].argmin(1)
    else:
        imax, imin = z.argmax(1), z.argmin(1)
    idx = np.where(take_max[None, :], imax, imin).astype(np.int32)
    return np.take_along_axis(z, idx[:, None, :].astype(np.int64), axis=1)[:, 0, :], idx


def gather_exact(x, coef, idx):
    x, coef = np.asarray(x, dtype=f32).astype(np.float64), np.asarray(coef, dtype=f32).astype(np.float64)
    B, N, cin = x.shape
    p = np.zeros((coef.shape[1], cin))
    for b in range(B):
        p = fmaf_step(coef[b][:, None], x[b][idx[b]], p)
    return p.astype(f32)


def scatter_exact(dx, coef, idx, w):
    dx = np.array(dx, dtype=f32).astype(np.float64)
    coef, w = np.asarray(coef, dtype=f32).astype(np.float64), np.asarray(w, dtype=f32).astype(np.float64)
    for b in range(dx.shape[0]):
        for c in range(coef.shape[1]):
            row = idx[b, c]
            dx[b, row] = fmaf_step(np.full(w.shape[1], coef[b, c]), w[c], dx[b, row])
    return dx.astype(f32)


def _chain32(a, b):
    """sum_k a[..., k] * b[..., k] as one float32 fmaf chain over k ascending (values in float64 arrays)."""
    p = np.zeros(np.broadcast(a[..., 0], b[..., 0]).shape)
    for k in range(a.shape[-1]):
        p = fmaf_step(np.broadcast_to(a[..., k], p.shape), np.broadcast_to(b[..., k], p.shape), p)
    return p


def var_gram32(x, w):
    """float32 emulation of the Gram route: xbar and S as float32 sums (plain float32 accumulation per row chunk order is not
    restated here: numpy's float32 pairwise sums stand in, the error model is the same), var = W S W^T / M by ascending fmaf chains."""
    x, w = np.asarray(x, dtype=f32), np.asarray(w, dtype=f32)
    x2 = x.reshape(-1, x.shape[-1])
    m = x2.shape[0]
    xbar = (x2.sum(0, dtype=f32) / f32(m)).astype(f32)
    xc = (x2 - xbar).astype(f32)
    s = (xc.T @ xc).astype(f32)
    w64 = w.astype(np.float64)
    t = _chain32(w64[:, None, :], s.astype(np.float64).T[None, :, :])      # t[c, j] = sum_k W[c, k] S[k, j]
    q = _chain32(t, w64)
    return np.maximum((q.astype(f32) / f32(m)).astype(f32), f32(0))


def var_sweep32(x, w, b):
    """float32 emulation of the sweep: mean = W xbar + b in float32, then the sum of (z - mean)^2 over the float32 z (numpy's float32
    sums stand in for the kernel's chains: the error model is the same)."""
    x, w = np.asarray(x, dtype=f32), np.asarray(w, dtype=f32)
    z = z_exact(x, w, b).reshape(-1, w.shape[0])
    x2 = x.reshape(-1, x.shape[-1])
    m = f32(z.shape[0])
    xbar = (x2.sum(0, dtype=f32) / m).astype(f32)
    mean = (_chain32(w.astype(np.float64), xbar.astype(np.float64)[None, :]).astype(f32) + np.asarray(b, dtype=f32)).astype(f32)
    d = (z - mean).astype(f32)
    return ((d * d).astype(f32).sum(0, dtype=f32) / m).astype(f32)


def var_onepass32(x, w, b):
    """float32 E[z^2] - mean^2 over the float32 z."""
    z = z_exact(x, w, b).reshape(-1, np.asarray(w).shape[0])
    m = f32(z.shape[0])
    mean = (z.sum(0, dtype=f32) / m).astype(f32)
    return ((z * z).astype(f32).sum(0, dtype=f32) / m - mean * mean).astype(f32)


# ------------------------------------------------------------------------------------------------------------------ inputs
def kappa(r):
    """Per channel |W[c]|^2 lambda_max(S) / (M var[c]) >= 1: how far W[c] leans out of the data's widest direction.  The variance from
    the Gram matrix, var = W S W^T / M, is a sum of terms of size |W|^2 |S| / M: its relative error in float32 is kappa times the unit
    roundoff times the chain's length, against kappa^(1/2) for a sum of (z - mean)^2, and BatchNorm's weight gradient, a difference of
    two terms that cancel to eps / (var + eps) of their size, passes that relative error on undamped.  With many rows S is full and
    kappa is a small number; with M = 2 rows S has rank one and kappa = 1 / cos^2 of the angle between W[c] and the two points'
    difference, unbounded: at (2, 1, 8, 32) one channel of case() has var = 7.8e-4 and kappa = 9.5e3, the Gram route's variance is
    off by 3.3e-5 relative there and dW by 1.2e-4 of the bar's 1e-4 (on an MI355X and in var_gram32 here), the sweep's by 3.4e-6 and
    2e-5.  That is why the layer takes its variance from the sweep; case() does not condition on kappa."""
    lam = np.linalg.eigvalsh(r['s']).max()
    return (r['w'] ** 2).sum(1) * lam / (r['m'] * np.maximum(r['var'], 1e-300))


def planted_pair(B, N):
    """(cloud, n1, n2) of the two identical points, or None when a cloud has one point."""
    return (0, N // 3, N - 1) if N >= 2 else None


@functools.lru_cache(maxsize=None)
def case(B, N, cin, c, relu, offset=0.0, seed=0):
    """-> dict(x, w, b, gamma, beta, dout, z32, zsel32, idx, mask, f64 (forward64's record at idx), grads (backward64 at idx, mask)),
    arrays read-only.  gamma[0] < 0, gamma[1] == 0 exactly, gamma[2] > 0, the rest of both signs.  Cloud 0 holds the same point at
    planted_pair's two indices, moved so that it IS the extremum of channel 2 (a planted tie).  For every (cloud, channel) the float64
    gap between the selected value and the best point that is not a copy of the selected one is >= MARGIN, and every ReLU
    pre-activation is >= MARGIN from zero: both are asserted."""
    rng = np.random.default_rng(100003 * cin + 1009 * c + 31 * N + B + seed)
    x = (rng.normal(0, 1, (B, N, cin)) + offset).astype(f32)
    w = (rng.uniform(-1, 1, (c, cin)) * np.sqrt(3.0 / cin)).astype(f32)
    b = rng.uniform(-0.5, 0.5, c).astype(f32)
    gamma = (rng.uniform(0.5, 1.5, c) * rng.choice([-1.0, 1.0], c)).astype(f32)
    gamma[0], gamma[1], gamma[2] = -abs(gamma[0]), 0.0, abs(gamma[2])
    beta = rng.uniform(-0.5, 0.5, c).astype(f32)
    beta[1] = f32(0.25)
    dout = rng.uniform(-1, 1, (B, c)).astype(f32)
    pair = planted_pair(B, N)
    if pair:
        x[0, pair[1]] += (6.0 * w[2] / np.linalg.norm(w[2])).astype(f32)     # far out along channel 2's weight: its maximum
        x[0, pair[2]] = x[0, pair[1]]
    for _ in range(300):
        r = forward64(x, w, b, gamma, beta, relu)
        z, idx = r['z'], r['idx']
        zs = np.where(r['gamma'] >= 0, z, -z)                                # the selected value is the maximum of zs
        other = zs.copy()
        np.put_along_axis(other, idx[:, None, :], -np.inf, axis=1)
        if pair:                                                            # the copy of a selected planted point is no runner-up
            for k1, k2 in (pair[1:], pair[:0:-1]):
                other[0, k2, idx[0] == k1] = -np.inf
        run = other.argmax(1)
        gap = np.take_along_axis(zs, idx[:, None, :], axis=1)[:, 0] - np.take_along_axis(other, run[:, None, :], axis=1)[:, 0]
        near = (gap < MARGIN) & np.isfinite(gap)
        edge = (np.abs(r['pre']) < MARGIN).any(0) if relu else np.zeros(c, bool)
        if not near.any() and not edge.any():
            break
        for bi, ci in zip(*np.nonzero(near)):
            k = run[bi, ci]
            if pair and bi == 0 and k in pair[1:]:
                k = idx[bi, ci]
            if not (pair and bi == 0 and k in pair[1:]):
                x[bi, k] += rng.normal(0, 0.05, cin).astype(f32)
        beta[edge] += f32(0.01)
    else:
        raise AssertionError('the inputs cannot be moved off the near-ties and the ReLU edges')
    if pair:
        assert np.array_equal(x[0, pair[1]], x[0, pair[2]]) and r['idx'][0, 2] in pair[1:]
    z32 = z_exact(x, w, b)
    zsel32, idx32 = extrema_exact(z32, gamma)
    if pair:
        assert idx32[0, 2] == pair[1]
    f64 = forward64(x, w, b, gamma, beta, relu, idx=idx32)
    mask = f64['pre'] > 0
    assert not relu or np.abs(f64['pre']).min() >= MARGIN / 2
    grads = backward64(f64, dout, mask=mask)
    out = dict(x=x, w=w, b=b, gamma=gamma, beta=beta, dout=dout, z32=z32, zsel32=zsel32, idx=idx32, mask=mask)
    for a in out.values():
        a.setflags(write=False)
    out.update(f64=f64, grads=grads, relu=relu, pair=pair)
    return out
