"""PointNet's pooled layer `Conv1d(k=1) -> BatchNorm1d (batch statistics) -> [ReLU] -> max over the points` trained on HIP in closed form
(csrc/pool_train.hip, catgrasp_amd/include/catgrasp_amd_pool.h), and the training-mode walk of PointNet's encoder built on it.

    out = conv_bn_max_train(x, conv, bn, relu)       # x (B, N, Cin) point-major -> (B, C)
    trans = tnet_train(tnet, rows, B, N)             # STN3d / STNkd on point-major rows (B * N, cin) -> (B, k, k)
    g, pointfeat, trans_feat = encoder_train(enc, x) # PointNetEncoder on x (B, N, D)

The (B * N, C) activation z = x W^T + b is never stored, forward or backward.  With M = B N, xbar the column mean of x and
S = sum_r (x[r] - xbar)^T (x[r] - xbar) the centred Gram matrix (Cin x Cin):

  forward    mean = W xbar + b, var = sum_r (z[r] - mean)^2 / M per channel by a second sweep of the extrema tiles (cg_pool_var), invstd =
             1 / sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale.  (var = W S W^T / M is exact algebra too, z - mean =
             (x - xbar) W^T, and costs no sweep, but in float32 it loses |W[c]|^2 lambda_max(S) / (M var[c]) where the sweep loses the
             square root of that: pool_stats keeps that route for callers who know their inputs, the layer does not take it.)  BatchNorm [+ ReLU] is monotone in z per channel, so
             zsel[b, c] = max_n z (gamma[c] >= 0) or min_n z (gamma[c] < 0), idx[b, c] the smallest n that attains it, and
             out = act(zsel * scale + shift).
  backward   e = dout * (out > 0) with ReLU, dout without; zhat = (zsel - mean) * invstd; dbeta = sum_b e; dgamma = sum_b e * zhat;
             u = scale * invstd * dgamma / M; dbias = 0 exactly (BatchNorm removes the mean);
             dW = T - (scale * dbeta)[:, None] * xbar[None, :] - u[:, None] * (W S)      with T[c] = sum_b (e scale)[b, c] x[b, idx[b, c]];
             G = W^T diag(u) W, v = sum_c (scale dbeta / M)[c] W[c];   dx[r] = -(x[r] - xbar) G - v, then
             dx[b, idx[b, c]] += (e scale)[b, c] W[c] for every (b, c).

Launch list.  Forward: cg_dense_group_sums (xbar, one group), x - xbar (torch, a temporary freed before the forward returns),
cg_dense_wgrad on the centred rows (S, which the backward needs), cg_pool_extrema (two launches), cg_pool_stats for the mean alone,
cg_pool_var (two launches), cg_pool_stats.  Backward: cg_dense_group_sums twice (dbeta,
dgamma, one group of B rows), cg_pool_wgrad_gather and cg_gemm_bias_act (W S) for dW; cg_dense_wgrad(x = W, dy = u * W) for G and
cg_dense_wgrad(dy = (scale dbeta / M) * W) for v (its bias output), cg_gemm_bias_act for xbar G and for the dense part
x (-G) + (xbar G - v), cg_pool_dgrad_scatter on top.  Every sum is one of those entry points' stated chains; the elementwise
combinations are torch ops, each one rounding, in the order written above, left to right, brackets first.

Only the gradients that autograd asks for are computed.  Saved for backward: x, W, xbar, S, zsel, idx, out (B, C) and the (5, C)
statistics; nothing of size M x C.  Once differentiable.  float32, HIP device tensors only; Cin a multiple of 8 in 8 .. 128, C a multiple
of 32 in 32 .. 1024, 2 <= B N <= 2^24.
"""
import ctypes

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from . import dense_autograd as D
from ._lib import _p, _stream, check
from .batchnorm import bn_relu_train
from .dense_autograd import _raw, linear

MAX_CIN = 128
MAX_C = 1024
MAX_ROWS = 1 << 24


def _rawi(t, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise NotImplementedError(f'{what} must be an int32 tensor, got {getattr(t, "dtype", type(t).__name__)}')
    if not t.is_contiguous():
        raise ValueError(f'{what} must be contiguous, got strides {t.stride()} for shape {tuple(t.shape)}')
    if not t.is_cuda:
        raise NotImplementedError(f'{what} must be on a HIP device (there is no CPU fallback), got {t.device}')
    return t


def pool_extrema(x, weight, bias=None, sign=None):
    """x (B, N, Cin), weight (C, Cin), bias (C) or None, sign (C) or None -> (zsel (B, C) float32, idx (B, C) int32): per cloud and channel
    the max (sign >= 0 or None) or min (sign < 0) over the points of the bits dense_forward(x, weight, bias) holds, and its first index."""
    _raw(x, 'x'), _raw(weight, 'weight')
    if x.dim() != 3 or weight.dim() != 2 or x.shape[2] != weight.shape[1]:
        raise ValueError(f'expected x (B, N, Cin) and weight (C, Cin), got {tuple(x.shape)} and {tuple(weight.shape)}')
    B, N, cin = x.shape
    c = weight.shape[0]
    _shape(bias, (c,), 'bias'), _shape(sign, (c,), 'sign')
    size = int(L.lib().cg_pool_extrema_workspace(B, N, c))
    check(min(size, 0), 'cg_pool_extrema_workspace')
    ws = torch.empty((size,), dtype=torch.float32, device=x.device)
    zsel = torch.empty((B, c), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, c), dtype=torch.int32, device=x.device)
    check(L.lib().cg_pool_extrema(_p(x), B, N, cin, _p(D.pack_b(weight)), _p(None if bias is None else _raw(bias, 'bias')), c,
                                  _p(None if sign is None else _raw(sign, 'sign')), _p(ws), _p(zsel), _p(idx), _stream()), 'cg_pool_extrema')
    return zsel, idx


def _shape(t, shape, what):
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f'expected {what} {tuple(shape)}, got {tuple(t.shape)}')


def pool_mean(weight, bias, xbar, B, n):
    """-> mean (C) = weight xbar + bias, cg_pool_stats' chain alone (B clouds of n points: the shapes it is judged by)."""
    _raw(weight, 'weight'), _raw(xbar, 'xbar')
    c, cin = weight.shape
    _shape(xbar, (cin,), 'xbar'), _shape(bias, (c,), 'bias')
    mean = torch.empty((c,), dtype=torch.float32, device=weight.device)
    nul = _p(None)
    check(L.lib().cg_pool_stats(_p(weight), _p(None if bias is None else _raw(bias, 'bias')), _p(xbar), nul, nul, nul, nul, 0.0, B, int(n), cin, c,
                                nul, 0, _p(mean), nul, nul, nul, nul, nul, _stream()), 'cg_pool_stats')
    return mean


def pool_var(x, weight, bias, mean):
    """-> var (C): the biased variance of z = x weight^T + bias about `mean` by a second sweep of the extrema tiles (cg_pool_var)."""
    _raw(x, 'x'), _raw(weight, 'weight'), _raw(mean, 'mean')
    if x.dim() != 3 or weight.dim() != 2 or x.shape[2] != weight.shape[1]:
        raise ValueError(f'expected x (B, N, Cin) and weight (C, Cin), got {tuple(x.shape)} and {tuple(weight.shape)}')
    B, N, cin = x.shape
    c = weight.shape[0]
    _shape(mean, (c,), 'mean'), _shape(bias, (c,), 'bias')
    size = int(L.lib().cg_pool_var_workspace(B, N, c))
    check(min(size, 0), 'cg_pool_var_workspace')
    ws = torch.empty((size,), dtype=torch.float32, device=x.device)
    var = torch.empty((c,), dtype=torch.float32, device=x.device)
    check(L.lib().cg_pool_var(_p(x), B, N, cin, _p(D.pack_b(weight)), _p(None if bias is None else _raw(bias, 'bias')), c, _p(mean), _p(ws), _p(var),
                              _stream()), 'cg_pool_var')
    return var


def pool_stats(weight, bias, xbar, s, gamma, beta, eps, n, zsel, relu, var=None):
    """-> (stats (5, C): the rows mean, var (biased), invstd, scale, shift; out (B, C)) for n points per cloud.  var (C): pool_var's
    result; None: the variance from the Gram matrix s."""
    for t, what in ((weight, 'weight'), (xbar, 'xbar'), (gamma, 'gamma'), (beta, 'beta'), (zsel, 'zsel')):
        _raw(t, what)
    if var is None:
        _raw(s, 's')
    else:
        _raw(var, 'var')
    if weight.dim() != 2 or zsel.dim() != 2 or zsel.shape[1] != weight.shape[0]:
        raise ValueError(f'expected weight (C, Cin) and zsel (B, C), got {tuple(weight.shape)} and {tuple(zsel.shape)}')
    c, cin = weight.shape
    B = zsel.shape[0]
    _shape(xbar, (cin,), 'xbar'), _shape(bias, (c,), 'bias'), _shape(gamma, (c,), 'gamma'), _shape(beta, (c,), 'beta'), _shape(var, (c,), 'var')
    if var is None:
        _shape(s, (cin, cin), 's')
    stats = torch.empty((5, c), dtype=torch.float32, device=weight.device)
    out = torch.empty((B, c), dtype=torch.float32, device=weight.device)
    rows = [ctypes.c_void_p(stats.data_ptr() + 4 * c * i) for i in range(5)]
    check(L.lib().cg_pool_stats(_p(weight), _p(None if bias is None else _raw(bias, 'bias')), _p(xbar), _p(s if var is None else None), _p(var),
                                _p(gamma), _p(beta), float(eps),
                                B, int(n), cin, c, _p(zsel), int(bool(relu)), *rows, _p(out), _stream()), 'cg_pool_stats')
    return stats, out


def pool_wgrad_gather(x, coef, idx):
    """-> T (C, Cin)[c] = sum_b coef[b, c] x[b, idx[b, c]], one fmaf chain over b ascending."""
    _raw(x, 'x'), _raw(coef, 'coef'), _rawi(idx, 'idx')
    if x.dim() != 3 or coef.dim() != 2 or coef.shape[0] != x.shape[0]:
        raise ValueError(f'expected x (B, N, Cin) and coef (B, C), got {tuple(x.shape)} and {tuple(coef.shape)}')
    B, N, cin = x.shape
    c = coef.shape[1]
    _shape(idx, (B, c), 'idx')
    t = torch.empty((c, cin), dtype=torch.float32, device=x.device)
    check(L.lib().cg_pool_wgrad_gather(_p(x), B, N, cin, _p(coef), _p(idx), c, _p(t), _stream()), 'cg_pool_wgrad_gather')
    return t


def pool_dgrad_scatter(dx, coef, idx, weight):
    """dx (B, N, Cin), in place: dx[b, idx[b, c]] = fmaf(coef[b, c], weight[c], dx[b, idx[b, c]]) for every (b, c), ascending c per row."""
    _raw(dx, 'dx'), _raw(coef, 'coef'), _rawi(idx, 'idx'), _raw(weight, 'weight')
    if dx.dim() != 3 or coef.dim() != 2 or coef.shape[0] != dx.shape[0]:
        raise ValueError(f'expected dx (B, N, Cin) and coef (B, C), got {tuple(dx.shape)} and {tuple(coef.shape)}')
    B, N, cin = dx.shape
    c = coef.shape[1]
    _shape(idx, (B, c), 'idx'), _shape(weight, (c, cin), 'weight')
    check(L.lib().cg_pool_dgrad_scatter(_p(coef), _p(idx), _p(weight), B, N, cin, c, _p(dx), _stream()), 'cg_pool_dgrad_scatter')
    return dx


def centred_gram(x2):
    """x2 (M, Cin) -> (xbar (Cin), S (Cin, Cin)): the column mean (cg_dense_group_sums with one group, / M) and the Gram matrix of the
    centred rows (cg_dense_wgrad of x - xbar with itself; bitwise symmetric, the products commute)."""
    m = x2.shape[0]
    xbar = D.group_sums(x2, m)[0] / m
    xc = x2 - xbar
    s = D.dense_wgrad(xc, xc, need_bias=False)[0]
    return xbar, s


class ConvBnMaxFunction(torch.autograd.Function):
    """(x (B, N, Cin), weight (C, Cin), bias (C) or None, gamma, beta, eps, relu) -> (out (B, C), stats (5, C)); stats carries no gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, eps, relu):
        x = x.detach().contiguous()
        weight = weight.detach().contiguous()
        gamma = gamma.detach().contiguous()
        bias = None if bias is None else bias.detach().contiguous()
        B, N, cin = x.shape
        xbar, s = centred_gram(x.view(B * N, cin))
        zsel, idx = pool_extrema(x, weight, bias, gamma)
        var = pool_var(x, weight, bias, pool_mean(weight, bias, xbar, B, N))
        stats, out = pool_stats(weight, bias, xbar, None, gamma, beta.detach().contiguous(), eps, N, zsel, relu, var=var)
        ctx.save_for_backward(x, weight, xbar, s, zsel, idx, stats, out)
        ctx.relu = bool(relu)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dstats):
        x, weight, xbar, s, zsel, idx, stats, out = ctx.saved_tensors
        need_x, need_w, need_b, need_gamma, need_beta = ctx.needs_input_grad[:5]
        if dout.dtype != torch.float32 or not dout.is_cuda:
            raise NotImplementedError(f'the gradient of conv_bn_max_train must be a float32 device tensor, got {dout.dtype} on {dout.device}')
        dx = dw = db = dgamma = dbeta = None
        if need_b:
            db = torch.zeros(weight.shape[0], dtype=torch.float32, device=x.device)
        if not (need_x or need_w or need_gamma or need_beta):
            return None, None, db, None, None, None, None
        B, N, cin = x.shape
        m = B * N
        mean, _, invstd, scale, _ = stats
        e = (dout * (out > 0)).contiguous() if ctx.relu else dout.contiguous()
        dbeta = D.group_sums(e, B)[0]
        dgamma = D.group_sums(e * ((zsel - mean) * invstd), B)[0]
        u = scale * invstd * dgamma / m
        coef = e * scale
        if need_w:
            ws = D.dense_forward(weight, s)                                   # W S^T = W S: S is symmetric to the bit
            dw = pool_wgrad_gather(x, coef, idx) - (scale * dbeta)[:, None] * xbar[None, :] - u[:, None] * ws
        if need_x:
            g = D.dense_wgrad(weight, u[:, None] * weight, need_bias=False)[0]                              # (u W)^T W = G
            v = D.dense_wgrad(weight, (scale * dbeta / m)[:, None] * weight, need_weight=False)[1]          # column sums
            gt = g.t().contiguous()
            row = D.dense_forward(xbar.view(1, cin), gt)[0] - v                # xbar G - v
            dx = D.dense_forward(x.view(m, cin), -gt, row).view(B, N, cin)
            pool_dgrad_scatter(dx, coef, idx, weight)
        return dx, dw, db, dgamma if need_gamma else None, dbeta if need_beta else None, None, None


def _conv_weight(conv, who='conv_bn_max_train'):
    if not isinstance(conv, nn.Conv1d) or conv.kernel_size != (1,) or conv.stride != (1,) or conv.padding != (0,) or conv.groups != 1:
        raise ValueError(f'{who} takes an nn.Conv1d of kernel size 1')
    return conv.weight.squeeze(2)          # a view: its gradient flows to conv.weight


def conv_bn_max_train(x, conv, bn, relu):
    """max over the points of [relu](bn(conv(x))) for x (B, N, Cin) contiguous float32 on the device, conv an nn.Conv1d(k = 1), bn an
    nn.BatchNorm1d in training mode -> (B, C); bn's running statistics are updated as torch does (running_var with the unbiased
    var * M / (M - 1), num_batches_tracked + 1)."""
    w = _conv_weight(conv)
    if not isinstance(bn, nn.BatchNorm1d) or not bn.training:
        raise ValueError('conv_bn_max_train takes an nn.BatchNorm1d in training mode')
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError('conv_bn_max_train is built for momentum given, affine=True and track_running_stats=True')
    for t, what in ((x, 'x'), (w, 'weight'), (conv.bias, 'bias'), (bn.weight, 'gamma'), (bn.bias, 'beta'), (bn.running_mean, 'running_mean'),
                    (bn.running_var, 'running_var')):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda):
            raise NotImplementedError(f'catgrasp_amd.pool_autograd is float32 on a HIP device only (there is no CPU fallback): {what} is '
                                      f'{getattr(t, "dtype", type(t).__name__)} on {getattr(t, "device", "the host")}')
    if x.dim() != 3 or x.shape[2] != w.shape[1] or bn.num_features != w.shape[0]:
        raise ValueError(f'expected x (B, N, {w.shape[1]}) and {w.shape[0]} BatchNorm features, got {tuple(x.shape)} and {bn.num_features}')
    B, N, cin = x.shape
    c = w.shape[0]
    m = B * N
    if m <= 1:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size((B, c, N))}')
    if m > MAX_ROWS:
        raise ValueError(f'a pooled layer takes 2 .. {MAX_ROWS} rows, got {m}')
    if cin % 8 or c % 32 or cin > MAX_CIN or c > MAX_C or cin < 8 or c < 32:
        raise NotImplementedError(f'the pooled layer is built for Cin a multiple of 8 up to {MAX_CIN} and C a multiple of 32 up to {MAX_C}; got '
                                  f'Cin = {cin}, C = {c}')
    out, stats = ConvBnMaxFunction.apply(x, w, conv.bias, bn.weight, bn.bias, bn.eps, bool(relu))
    with torch.no_grad():
        mo = bn.momentum
        bn.running_mean.mul_(1 - mo).add_(stats[0], alpha=mo)
        bn.running_var.mul_(1 - mo).add_(stats[1], alpha=mo * m / (m - 1))
        bn.num_batches_tracked += 1
    return out


def rows_layer(rows, conv, bn):
    """relu(bn(conv(rows))) on point-major rows (M, cin) through dense_autograd.linear + bn_relu_train.  A width that is no multiple of 8
    (the 6 input channels) takes rows and the weight zero-padded to the next multiple with F.pad: a zero column adds fmaf(0, 0, p) = p."""
    w = _conv_weight(conv, 'rows_layer')
    pad = -w.shape[1] % 8
    if pad:
        rows, w = F.pad(rows, (0, pad)), F.pad(w, (0, pad))
    return bn_relu_train(linear(rows.contiguous(), w, conv.bias), bn)


def tnet_train(tnet, rows, B, N):
    """pointnet2.STN3d / STNkd in training mode on point-major rows (B * N, cin) -> (B, k, k).  conv1 and conv2 with their BatchNorms
    through rows_layer, conv3 / bn3 / ReLU / max through conv_bn_max_train; every width is read from the modules.  The FC tail on B rows
    (fc1 .. fc3, bn4, bn5) stays on torch ops."""
    h = rows_layer(rows, tnet.conv1, tnet.bn1)
    h = rows_layer(h, tnet.conv2, tnet.bn2)
    g = conv_bn_max_train(h.view(B, N, -1), tnet.conv3, tnet.bn3, relu=True)
    g = F.relu(tnet.bn4(tnet.fc1(g)))
    g = F.relu(tnet.bn5(tnet.fc2(g)))
    k = tnet._k
    return (tnet.fc3(g) + torch.eye(k, device=g.device, dtype=g.dtype).reshape(1, -1)).view(-1, k, k)


def encoder_train(enc, x):
    """pointnet2.PointNetEncoder (with its feature transform) in training mode on x (B, N, D) -> (g (B, C3), pointfeat (B, N, C1)
    point-major, trans_feat).  The per-point layers through rows_layer, the three pooled layers (stn.conv3, fstn.conv3 with ReLU, conv3
    without) through conv_bn_max_train.  On torch ops: the two bmm's and the FC tails of the two transform nets."""
    B, N, Dn = x.shape
    trans = tnet_train(enc.stn, x.reshape(B * N, Dn), B, N)
    xyz = torch.bmm(x[:, :, :3], trans)
    pts = torch.cat([xyz, x[:, :, 3:]], dim=2) if Dn > 3 else xyz
    h = rows_layer(pts.reshape(B * N, Dn), enc.conv1, enc.bn1)
    trans_feat = tnet_train(enc.fstn, h, B, N)
    pointfeat = torch.bmm(h.view(B, N, -1), trans_feat)
    h = rows_layer(pointfeat.reshape(B * N, -1), enc.conv2, enc.bn2)
    g = conv_bn_max_train(h.view(B, N, -1), enc.conv3, enc.bn3, relu=False)
    return g, pointfeat, trans_feat
