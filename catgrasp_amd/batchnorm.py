"""BatchNorm1d in batch-statistics mode fused with ReLU, with its gradient, on HIP (csrc/batchnorm_train.hip,
include/catgrasp_amd_bn.h): the training-time form of the `BatchNorm1d, ReLU` run that the inference layers fold into a convolution's
prologue.

    y = bn_relu_train(x, bn)          # x (n, c) float32 on the device, bn an nn.BatchNorm1d in training mode

The statistics are two-pass (mean, then the biased variance of x - mean); every per-channel sum, forward and backward, is a stated tree
of f32 chains that depends on n alone (the header has it), there are no atomics, so a result is the same bits on any run and any
stream.  The activation is fmaxf(x*scale + shift, 0), the inference kernel's prologue with the batch's constants; the backward
recomputes the ReLU mask from x, scale and shift, so nothing but x and five (c) vectors is kept (one (5, c) tensor).

c is a multiple of 16 up to 1024, 2 <= n <= 2^24, float32, HIP device tensors only; there is no CPU implementation and no double
backward.  Widths up to 224 (the sparse networks') run through the entry points of include/catgrasp_amd_bn.h, wider ones (the 512 /
256 / 128 of PointNetSeg's head) through the `_wide` ones of catgrasp_amd/include/catgrasp_amd_dense.h: the same kernels and the same
tree, only the limit differs, and at c <= 224 both give the same bits."""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from ._lib import _p, _stream, check

MAX_C = 224            # the entry points of catgrasp_amd_bn.h
WIDE_MAX_C = 1024      # the `_wide` entry points of catgrasp_amd_dense.h


def _entry(c, wide):
    """(workspace, forward, backward) symbol names for width c; wide=None: by the width."""
    if wide or (wide is None and c > MAX_C):
        return 'cg_bn_wide_workspace', 'cg_bn_relu_train_forward_wide', 'cg_bn_relu_train_backward_wide'
    return 'cg_bn_workspace', 'cg_bn_relu_train_forward', 'cg_bn_relu_train_backward'


def _workspace(n, c, dev, wide=None):
    name = _entry(c, wide)[0]
    size = int(getattr(L.lib(), name)(n, c))
    check(min(size, 0), name)
    return torch.empty((size,), dtype=torch.float32, device=dev)


def bn_relu_forward(x, gamma, beta, eps, wide=None):
    """-> (y (n, c), stats (5, c): the rows mean, var (biased), invstd, scale, shift) of a contiguous float32 device x.
    wide: True / False forces the `_wide` / the catgrasp_amd_bn.h entry points, None takes them by the width."""
    n, c = x.shape
    name = _entry(c, wide)[1]
    y = torch.empty_like(x)
    stats = torch.empty((5, c), dtype=torch.float32, device=x.device)
    rows = [ctypes.c_void_p(stats.data_ptr() + 4 * c * i) for i in range(5)]
    check(getattr(L.lib(), name)(_p(L.f32c(x)), n, c, _p(L.f32c(gamma)), _p(L.f32c(beta)), float(eps), _p(_workspace(n, c, x.device, wide)),
                                 *rows, _p(y), _stream()), name)
    return y, stats


def bn_relu_backward(x, dy, stats, need_dx=True, wide=None):
    """-> (dx (n, c) or None, dgamma (c), dbeta (c)) for dy = dL/dy and the forward's stats.  wide: as in bn_relu_forward."""
    n, c = x.shape
    name = _entry(c, wide)[2]
    dx = torch.empty_like(x) if need_dx else None
    dgamma, dbeta = (torch.empty((c,), dtype=torch.float32, device=x.device) for _ in range(2))
    mean, _, invstd, scale, shift = (ctypes.c_void_p(stats.data_ptr() + 4 * c * i) for i in range(5))
    check(getattr(L.lib(), name)(_p(L.f32c(x)), _p(L.f32c(dy)), n, c, mean, invstd, scale, shift,
                                 _p(_workspace(n, c, x.device, wide)), _p(dgamma), _p(dbeta), _p(dx), _stream()), name)
    return dx, dgamma, dbeta


class BatchNormReLUFunction(torch.autograd.Function):
    """(x, gamma, beta, eps) -> (y, stats): y = relu(batch_norm(x)) with the batch's statistics; stats (5, c) holds mean, the biased
    var, invstd, scale and shift, is returned for the running statistics and carries no gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        x = x.detach().contiguous()
        y, stats = bn_relu_forward(x, gamma.detach().contiguous(), beta.detach().contiguous(), eps)
        ctx.save_for_backward(x, stats)
        ctx.mark_non_differentiable(stats)
        return y, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y, _grad_stats):
        x, stats = ctx.saved_tensors
        need_x, need_gamma, need_beta = ctx.needs_input_grad[:3]
        if grad_y.dtype != torch.float32 or not grad_y.is_cuda:
            raise NotImplementedError(f'the gradient of bn_relu_train must be a float32 device tensor, got {grad_y.dtype} on {grad_y.device}')
        if not (need_x or need_gamma or need_beta):
            return None, None, None, None
        dx, dgamma, dbeta = bn_relu_backward(x, grad_y.contiguous(), stats, need_dx=need_x)
        return dx, dgamma if need_gamma else None, dbeta if need_beta else None, None


def bn_relu_train(x, bn):
    """relu(bn(x)) for an nn.BatchNorm1d in training mode and x (n, c), and the update of bn's running statistics that torch makes:
    running_mean <- (1 - momentum) running_mean + momentum mean, running_var likewise with the unbiased var * n / (n - 1),
    num_batches_tracked + 1."""
    if not isinstance(bn, nn.BatchNorm1d) or not bn.training:
        raise ValueError('bn_relu_train takes an nn.BatchNorm1d in training mode')
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise NotImplementedError('bn_relu_train is built for momentum given, affine=True and track_running_stats=True')
    if x.dim() != 2 or x.shape[1] != bn.num_features:
        raise ValueError(f'expected (n, {bn.num_features}) features, got {tuple(x.shape)}')
    tensors = (x, bn.weight, bn.bias, bn.running_mean, bn.running_var)
    if any(t.dtype != torch.float32 or not t.is_cuda for t in tensors):
        raise NotImplementedError('bn_relu_train is float32 on a HIP device only (there is no CPU fallback)')
    n, c = x.shape
    if n <= 1:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {x.size()}')
    if c % 16 or c > WIDE_MAX_C:
        raise NotImplementedError(f'bn_relu_train takes widths that are multiples of 16 up to {WIDE_MAX_C}, got {c}')
    y, stats = BatchNormReLUFunction.apply(x, bn.weight, bn.bias, bn.eps)
    with torch.no_grad():
        m = bn.momentum
        bn.running_mean.mul_(1 - m).add_(stats[0], alpha=m)
        bn.running_var.mul_(1 - m).add_(stats[1], alpha=m * n / (n - 1))
        bn.num_batches_tracked += 1
    return y
