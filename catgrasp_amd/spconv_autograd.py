"""The layers of `catgrasp_amd.spconv` with gradients: a drop-in for the part of `spconv` that the reference's PointGroup model code
trains with (PointGroup/model/pointgroup/pointgroup.py; its backward is spconv/functional.py).

    import catgrasp_amd.spconv_autograd as spconv

SparseConvTensor, SparseModule, SparseSequential, RuleBook and the rule-book functions are `catgrasp_amd.spconv`'s own.  SubMConv3d,
SparseConv3d and SparseInverseConv3d are subclasses of its layers: same constructor arguments, same state_dict keys, same
initialisation, so a state_dict trained here loads strictly into `catgrasp_amd.spconv` layers and `pointgroup.PointGroup`.

When nothing asks for a gradient (torch.no_grad(), or no input and no parameter requires one) a layer's forward IS the base class's:
prologue, residual and features_b in the one launch, identical bits.  When a gradient is needed the layer runs SparseConvFunction:

  forward    spconv.sparse_conv (csrc/sparse_conv.hip) without prologue and residual: the bits of the inference layer.  An eval-mode
             folded prologue (scale, shift) is applied beforehand as relu(x*scale + shift) with torch ops (equivalent, because an
             absent neighbour contributes nothing either way), the residual afterwards with a torch add; both are differentiable
             through torch.  features_b raises NotImplementedError.
  backward   csrc/sparse_conv_grad.hip (include/catgrasp_amd_sparse_grad.h), exact f32 on v_mfma_f32_32x32x2_f32, no atomics:
             cg_sparse_conv_wgrad for the weight and the bias (row chunks of CG_SPARSE_GRAD_ROWS reduced in a fixed order through
             a workspace that torch allocates per call) and cg_sparse_conv_dgrad for the input, which is the forward operator over
             the transposed rule book with transposed weights:

               layer                  transposed book                      transposed weight
               SubM 3x3x3             nbr itself                           Wt[k] = W[26 - k]^T
               SparseConv3d           inverse_rules(book)                  Wt[k] = W[k]^T
               SparseInverseConv3d    the strided layer's book.nbr         Wt[k] = W[k]^T
               SubM 1x1x1             the identity column                  Wt = W^T

             Only the gradients that autograd asks for are computed.  Once differentiable: there is no double backward.

float32, HIP device tensors only; there is no CPU implementation.  Not differentiated: cg_sparse_conv_cat (features_b), the
prologue inside the kernel, anything but f32.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L
from . import spconv as _S
from ._lib import _p, _stream, check
from .spconv import (MAX_CIN, MAX_COUT, RuleBook, SparseConvTensor, SparseConvolution, SparseModule, SparseSequential,  # noqa: F401
                     bn_relu_prologue, down_rules, identity_rules, inverse_rules, sparse_conv, subm_rules)


def grad_rows():
    """CG_SPARSE_GRAD_ROWS of include/catgrasp_amd_sparse_grad.h: rows per chunk of the weight gradient's reduction."""
    with open(L.SPARSE_GRAD_HEADER_PATH) as f:
        for line in f:
            if line.startswith('#define CG_SPARSE_GRAD_ROWS'):
                return int(line.split()[2])
    raise L.CatgraspAmdError('include/catgrasp_amd_sparse_grad.h does not define CG_SPARSE_GRAD_ROWS')


def sparse_conv_wgrad(features, nbr, grad_out, cin, need_weight=True, need_bias=True):
    """-> (dW (K, Cin, Cout) or None, db (Cout,) or None) of out[i] = bias + sum_k features[nbr[i, k]] @ W[k] for grad_out = dL/dout."""
    n_out, K = nbr.shape
    cout = grad_out.shape[1]
    dev = grad_out.device
    size = int(L.lib().cg_sparse_wgrad_workspace(n_out, K, cin, cout))
    check(min(size, 0), 'cg_sparse_wgrad_workspace')
    ws = torch.empty((size,), dtype=torch.float32, device=dev)
    dw = torch.empty((K, cin, cout), dtype=torch.float32, device=dev) if need_weight else None
    db = torch.empty((cout,), dtype=torch.float32, device=dev) if need_bias else None
    check(L.lib().cg_sparse_conv_wgrad(_p(L.f32c(features)), features.shape[0], _p(L.i32c(nbr)), n_out, K, _p(L.f32c(grad_out)), cin, cout,
                                       _p(ws), _p(dw), _p(db), _stream()), 'cg_sparse_conv_wgrad')
    return dw, db


def sparse_conv_dgrad(grad_out, nbr_t, weight_t):
    """-> dx (n_in, Cin) = sum_k grad_out[nbr_t[:, k]] @ weight_t[k]; nbr_t (n_in, K) the transposed book, weight_t (K, Cout, Cin)."""
    n_in, K = nbr_t.shape
    cout, cin = weight_t.shape[1:]
    dx = torch.empty((n_in, cin), dtype=torch.float32, device=grad_out.device)
    check(L.lib().cg_sparse_conv_dgrad(_p(L.f32c(grad_out)), grad_out.shape[0], _p(L.i32c(nbr_t)), n_in, K, _p(L.f32c(weight_t)), cin, cout,
                                       _p(dx), _stream()), 'cg_sparse_conv_dgrad')
    return dx


def transposed_weight(weight, flip):
    """(K, Cin, Cout) -> (K, Cout, Cin) contiguous: Wt[k] = W[k]^T, or W[K - 1 - k]^T with flip (the submanifold 3x3x3 layer, whose
    offset k seen from the other end is 26 - k)."""
    w = weight.detach()
    if flip:
        w = w.flip(0)
    return w.transpose(1, 2).contiguous()


class SparseConvFunction(torch.autograd.Function):
    """out = bias + sum_k features[nbr[:, k]] @ weight[k].  features (n_in, Cin), weight (K, Cin, Cout), bias (Cout,) or None,
    nbr (n_out, K) int32, nbr_t (n_in, K) int32 the transposed book, flip: the weight permutation that goes with it
    (transposed_weight)."""

    @staticmethod
    def forward(ctx, features, weight, bias, nbr, nbr_t, flip):
        features = features.detach().contiguous()
        ctx.save_for_backward(features, weight, nbr, nbr_t)
        ctx.flip = bool(flip)
        return sparse_conv(features, nbr, weight.detach(), None if bias is None else bias.detach())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        features, weight, nbr, nbr_t = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        if grad_out.dtype != torch.float32 or not grad_out.is_cuda:
            raise NotImplementedError(f'the gradient of a sparse convolution must be a float32 device tensor, got {grad_out.dtype} on {grad_out.device}')
        grad_out = grad_out.contiguous()
        dx = dw = db = None
        if need_x:
            dx = sparse_conv_dgrad(grad_out, nbr_t, transposed_weight(weight, ctx.flip))
        if need_w or need_b:
            dw, db = sparse_conv_wgrad(features, nbr, grad_out, weight.shape[1], need_w, need_b)
        return dx, dw, db, None, None, None


class _Differentiable:
    """Mixed in before a `catgrasp_amd.spconv` layer class: forward with gradients."""

    def _books(self, input):
        """-> (nbr, transposed nbr, flip, output indices, output spatial shape)"""
        if not (self.conv1x1 or self.subm or self.inverse) and self.indice_key is None:
            book = down_rules(input.indices, input.spatial_shape, input.batch_size)        # a strided layer that keeps no book
            return book.nbr, inverse_rules(book), False, book.out_indices, book.out_spatial_shape
        nbr, out_indices, out_shape = self._rule_book(input)
        if self.conv1x1:
            return nbr, nbr, False, out_indices, out_shape
        if self.subm:
            return nbr, nbr, True, out_indices, out_shape
        book = input.find_indice_pair(self.indice_key)
        return nbr, (book.nbr if self.inverse else inverse_rules(book)), False, out_indices, out_shape

    def forward(self, input, prologue=None, residual=None, features_b=None):
        if not isinstance(input, SparseConvTensor):
            raise TypeError(f'expected a SparseConvTensor, got {type(input).__name__}')
        scale, shift = prologue if prologue is not None else (None, None)
        wanted = (input.features, self.weight, self.bias, scale, shift, residual, features_b)
        if not (torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in wanted)):
            return super().forward(input, prologue=prologue, residual=residual, features_b=features_b)
        if not torch.cuda.is_available() or not input.features.is_cuda or not input.indices.is_cuda:
            raise L.CatgraspAmdError('catgrasp_amd.spconv_autograd needs HIP device tensors (there is no CPU fallback)')
        if features_b is not None:
            raise NotImplementedError('catgrasp_amd.spconv_autograd: the two-source layer (features_b) has no gradient')
        feats = input.features
        if feats.dtype != torch.float32:
            raise NotImplementedError(f'catgrasp_amd.spconv_autograd is float32 only, got {feats.dtype}')
        if feats.shape[0] != input.indices.shape[0]:
            raise ValueError(f'features has {feats.shape[0]} rows, indices {input.indices.shape[0]}')
        if feats.shape[1] != self.in_channels:
            raise ValueError(f'features have {feats.shape[1]} channels, the layer takes {self.in_channels}')
        if scale is not None:
            feats = torch.relu(feats * scale + shift)
        nbr, nbr_t, flip, out_indices, out_shape = self._books(input)
        out = SparseConvFunction.apply(feats, self.weight.reshape(nbr.shape[1], self.in_channels, self.out_channels), self.bias, nbr, nbr_t, flip)
        if residual is not None:
            out = out + residual
        return input.replace_feature(out, out_indices, out_shape)


class SubMConv3d(_Differentiable, _S.SubMConv3d):
    pass


class SparseConv3d(_Differentiable, _S.SparseConv3d):
    pass


class SparseInverseConv3d(_Differentiable, _S.SparseInverseConv3d):
    pass
