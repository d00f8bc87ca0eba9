"""Dense per-row layers (`nn.Linear`, `Conv1d(k=1)` on point-major rows) with gradients on HIP, and the per-point head of PointNetSeg
built from them (csrc/dense_train.hip, catgrasp_amd/include/catgrasp_amd_dense.h).

    y = linear(x, weight, bias)                                          # x (n, Cin), weight (Cout, Cin) -> (n, Cout)
    y = linear_group_bias(x, weight, bias, row_bias, rows_per_group)     # ... + row_bias[row // rows_per_group]
    logits = seg_head_train(g, pointfeat, convs, bns)                    # (B, Cg), (B, N, Cp) -> (B, N, n_out)

  forward    cg_gemm_bias_act (csrc/gemm.hip) as it is, `row_bias` in its epilogue; the weight is packed into the MFMA's B-fragment
             order on the device (pack_b: folding.pack_b's permutation as torch ops), every step, because it changes every step.
  backward   cg_dense_wgrad for the weight and the bias (row chunks of CG_DENSE_GRAD_ROWS, one fmaf chain per chunk and element, the
             chunks added in ascending order through a workspace that torch allocates per call), cg_dense_dgrad for the input (the
             forward operator with the weight read transposed, the contraction padded with zeros to whole steps of 8) and
             cg_dense_group_sums for row_bias (the column-sum tree of catgrasp_amd_bn.h per group).  Exact f32 on
             v_mfma_f32_32x32x2_f32; every sum has a stated order, so a step gives the same bits on any run and any stream.
             Only the gradients that autograd asks for are computed.  Once differentiable: there is no double backward.

The head's first layer is split: the reference multiplies the (B, Cg + Cp, N) concatenation of the global feature, repeated over
the N points, and the per-point feature by conv1's weight.  Here  z1[b, n] = pointfeat[b, n] . Wp^T + (g[b] . Wg^T + bias)  with
Wg = conv1.weight[:, :Cg] and Wp = conv1.weight[:, Cg:]: the bracket is one product per cloud, added per row group by the GEMM's
epilogue, and neither the concatenation nor its gradient is ever formed.

float32, HIP device tensors only; there is no CPU implementation.  Cin a multiple of 8, Cout a multiple of 4, both up to 1024; BatchNorm
widths multiples of 16 up to 1024.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from ._lib import _p, _stream, check
from .batchnorm import bn_relu_train

MAX_C = 1024
MAX_ROWS = 1 << 24


def grad_rows():
    """CG_DENSE_GRAD_ROWS of catgrasp_amd_dense.h: rows per chunk of the weight gradient's reduction."""
    with open(L.DENSE_HEADER_PATH) as f:
        for line in f:
            if line.startswith('#define CG_DENSE_GRAD_ROWS'):
                return int(line.split()[2])
    raise L.CatgraspAmdError('catgrasp_amd_dense.h does not define CG_DENSE_GRAD_ROWS')


def _raw(t, what):
    """The argument rule of the raw wrappers: a contiguous float32 device tensor; dtype, strides and device are judged, in that order,
    before any device work."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise NotImplementedError(f'{what} must be a float32 tensor, got {getattr(t, "dtype", type(t).__name__)}')
    if not t.is_contiguous():
        raise ValueError(f'{what} must be contiguous, got strides {t.stride()} for shape {tuple(t.shape)}')
    if not t.is_cuda:
        raise NotImplementedError(f'{what} must be on a HIP device (there is no CPU fallback), got {t.device}')
    return t


def pack_b(weight):
    """W (N, K) on the device, K % 8 == 0 -> the flat B-fragment image cg_gemm_bias_act reads: folding.pack_b's permutation
    Wp[nb][ks][lane >> 5][lane & 31][j] = W[32 nb + (lane & 31)][8 ks + 4 (lane >> 5) + j], rows zero padded to 32, as torch ops."""
    n, k = weight.shape
    nb = (n + 31) // 32
    w = weight.detach()
    if nb * 32 != n:
        w = torch.cat([w, w.new_zeros((nb * 32 - n, k))])
    return w.reshape(nb, 32, k // 8, 2, 4).permute(0, 2, 3, 1, 4).contiguous().reshape(-1)


def dense_forward(x, weight, bias=None, row_bias=None, rows_per_group=1):
    """-> y (n, Cout) = x . weight^T + bias + row_bias[row // rows_per_group] through cg_gemm_bias_act."""
    _raw(x, 'x'), _raw(weight, 'weight')
    n, cin = x.shape
    cout = weight.shape[0]
    y = torch.empty((n, cout), dtype=torch.float32, device=x.device)
    ld_rb = row_bias.shape[1] if row_bias is not None else 0
    check(L.lib().cg_gemm_bias_act(_p(x), n, cin, cin, _p(pack_b(weight)), cout, _p(None if bias is None else _raw(bias, 'bias')),
                                   _p(None if row_bias is None else _raw(row_bias, 'row_bias')), rows_per_group, ld_rb, 0, 0, _p(y), cout,
                                   _stream()), 'cg_gemm_bias_act')
    return y


def dense_wgrad(x, grad_out, need_weight=True, need_bias=True):
    """-> (dW (Cout, Cin) or None, db (Cout,) or None) of y = x . W^T + b for grad_out = dL/dy (n, Cout)."""
    _raw(x, 'x'), _raw(grad_out, 'grad_out')
    (n, cin), cout = x.shape, grad_out.shape[1]
    if grad_out.shape[0] != n:
        raise ValueError(f'x has {n} rows, grad_out {grad_out.shape[0]}')
    size = int(L.lib().cg_dense_wgrad_workspace(n, cin, cout))
    check(min(size, 0), 'cg_dense_wgrad_workspace')
    dev = x.device
    ws = torch.empty((size,), dtype=torch.float32, device=dev)
    dw = torch.empty((cout, cin), dtype=torch.float32, device=dev) if need_weight else None
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if need_bias else None
    check(L.lib().cg_dense_wgrad(_p(x), _p(grad_out), n, cin, cout, _p(ws), _p(dw), _p(db), _stream()), 'cg_dense_wgrad')
    return dw, db


def dense_dgrad(grad_out, weight):
    """-> dx (n, Cin) = grad_out . weight for grad_out (n, Cout) and weight (Cout, Cin) as it is stored."""
    _raw(grad_out, 'grad_out'), _raw(weight, 'weight')
    n, cout = grad_out.shape
    if weight.shape[0] != cout:
        raise ValueError(f'grad_out has {cout} columns, weight {weight.shape[0]} rows')
    cin = weight.shape[1]
    dx = torch.empty((n, cin), dtype=torch.float32, device=grad_out.device)
    check(L.lib().cg_dense_dgrad(_p(grad_out), n, cout, _p(weight), cin, _p(dx), _stream()), 'cg_dense_dgrad')
    return dx


def group_sums(grad_out, rows_per_group):
    """-> (G, C): the sums of grad_out (G * rows_per_group, C) over the rows of every group."""
    _raw(grad_out, 'grad_out')
    n, c = grad_out.shape
    groups = n // max(int(rows_per_group), 1)
    if rows_per_group < 1 or groups * rows_per_group != n or groups < 1:
        raise ValueError(f'{n} rows are not a whole number of groups of {rows_per_group}')
    size = int(L.lib().cg_dense_group_sums_workspace(groups, rows_per_group, c))
    check(min(size, 0), 'cg_dense_group_sums_workspace')
    ws = torch.empty((size,), dtype=torch.float32, device=grad_out.device)
    out = torch.empty((groups, c), dtype=torch.float32, device=grad_out.device)
    check(L.lib().cg_dense_group_sums(_p(grad_out), groups, rows_per_group, c, _p(ws), _p(out), _stream()), 'cg_dense_group_sums')
    return out


class DenseFunction(torch.autograd.Function):
    """y = x . weight^T [+ bias] [+ row_bias[row // rows_per_group]].  x (n, Cin), weight (Cout, Cin), bias (Cout,) or None, row_bias
    (n / rows_per_group, Cout) or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, row_bias, rows_per_group):
        x = x.detach().contiguous()
        weight = weight.detach().contiguous()
        ctx.save_for_backward(x, weight)
        ctx.rows_per_group = int(rows_per_group)
        return dense_forward(x, weight, None if bias is None else bias.detach().contiguous(),
                             None if row_bias is None else row_bias.detach().contiguous(), int(rows_per_group))

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        if grad_out.dtype != torch.float32 or not grad_out.is_cuda:
            raise NotImplementedError(f'the gradient of a dense layer must be a float32 device tensor, got {grad_out.dtype} on {grad_out.device}')
        grad_out = grad_out.contiguous()
        dx = dw = db = dr = None
        if need_x:
            dx = dense_dgrad(grad_out, weight)
        if need_w or need_b:
            dw, db = dense_wgrad(x, grad_out, need_w, need_b)
        if need_r:
            dr = group_sums(grad_out, ctx.rows_per_group)
        return dx, dw, db, dr, None


def _check(x, weight, bias, row_bias=None, rows_per_group=1):
    for t, what in ((x, 'x'), (weight, 'weight'), (bias, 'bias'), (row_bias, 'row_bias')):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda):
            raise NotImplementedError(f'catgrasp_amd.dense_autograd is float32 on a HIP device only (there is no CPU fallback): {what} is '
                                      f'{getattr(t, "dtype", type(t).__name__)} on {getattr(t, "device", "the host")}')
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f'expected x (n, Cin) and weight (Cout, Cin), got {tuple(x.shape)} and {tuple(weight.shape)}')
    n, cin = x.shape
    cout = weight.shape[0]
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f'expected bias ({cout},), got {tuple(bias.shape)}')
    if not 1 <= n <= MAX_ROWS:
        raise ValueError(f'a dense layer takes 1 .. {MAX_ROWS} rows, got {n}')
    if cin % 8 or cout % 4 or cin > MAX_C or cout > MAX_C or cin < 8 or cout < 4:
        raise NotImplementedError(f'the dense layers are built for Cin a multiple of 8 and Cout a multiple of 4, both up to {MAX_C}; got '
                                  f'Cin = {cin}, Cout = {cout}')
    if row_bias is not None:
        if rows_per_group < 1 or n % rows_per_group or tuple(row_bias.shape) != (n // rows_per_group, cout):
            raise ValueError(f'expected row_bias ({n} / rows_per_group, {cout}) for whole groups of rows, got {tuple(row_bias.shape)} with '
                             f'rows_per_group = {rows_per_group}')


def linear(x, weight, bias=None):
    """x . weight^T + bias on rows: nn.Linear, or Conv1d(k=1) on point-major rows.  x (n, Cin), weight (Cout, Cin), bias (Cout,)."""
    _check(x, weight, bias)
    return DenseFunction.apply(x, weight, bias, None, 1)


def linear_group_bias(x, weight, bias, row_bias, rows_per_group):
    """linear(x, weight, bias) + row_bias[row // rows_per_group]; row_bias (n / rows_per_group, Cout) gets the per-group column sums of
    the output's gradient."""
    rows_per_group = int(rows_per_group)
    _check(x, weight, bias, row_bias, rows_per_group)
    return DenseFunction.apply(x, weight, bias, row_bias, rows_per_group)


def _conv_weight(conv):
    if not isinstance(conv, nn.Conv1d) or conv.kernel_size != (1,) or conv.stride != (1,) or conv.padding != (0,) or conv.groups != 1:
        raise ValueError('seg_head_train takes nn.Conv1d layers of kernel size 1')
    return conv.weight.squeeze(2)          # a view: its gradient flows to conv.weight


def seg_head_train(g, pointfeat, convs, bns):
    """The per-point head of PointNetSeg in training mode: conv1 (on [g repeated over the points | pointfeat], split as above), bn1,
    ReLU, conv2, bn2, ReLU, conv3, bn3, ReLU, conv4.  g (B, Cg) the global feature, pointfeat (B, N, Cp) point-major contiguous,
    convs four nn.Conv1d(k=1) with convs[0].in_channels = Cg + Cp, bns three nn.BatchNorm1d in training mode.
    -> logits (B, N, n_out) contiguous; the running statistics of bns are updated as torch does."""
    if len(convs) != 4 or len(bns) != 3:
        raise ValueError('seg_head_train takes four convolutions and three batch norms')
    for t, what in ((g, 'g'), (pointfeat, 'pointfeat')):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda:
            raise NotImplementedError(f'seg_head_train is float32 on a HIP device only (there is no CPU fallback): {what} is '
                                      f'{getattr(t, "dtype", type(t).__name__)} on {getattr(t, "device", "the host")}')
    if g.dim() != 2 or pointfeat.dim() != 3 or g.shape[0] != pointfeat.shape[0]:
        raise ValueError(f'expected g (B, Cg) and pointfeat (B, N, Cp), got {tuple(g.shape)} and {tuple(pointfeat.shape)}')
    B, N, cp = pointfeat.shape
    cg = g.shape[1]
    w = [_conv_weight(c) for c in convs]
    if w[0].shape[1] != cg + cp:
        raise ValueError(f'conv1 takes {w[0].shape[1]} channels, g and pointfeat have {cg} + {cp}')
    if B * N <= 1:
        raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size((B, w[0].shape[0], N))}')
    r = linear(g, w[0][:, :cg], convs[0].bias)
    h = linear_group_bias(pointfeat.contiguous().view(B * N, cp), w[0][:, cg:], None, r, N)
    for i in range(3):
        h = bn_relu_train(h, bns[i])
        h = linear(h, w[i + 1], convs[i + 1].bias)
    return h.view(B, N, -1)
