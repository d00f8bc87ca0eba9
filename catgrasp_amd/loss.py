"""The NUNOCS training objective on HIP (csrc/nocs_loss.hip, include/catgrasp_amd_loss.h): the cross-entropy over coordinate bins,
minimised per sample over the category's symmetries, with its gradient -- the reference's NocsMinSymmetryCELoss (loss.py:16-45), which
trainer_nunocs.py:52,81 calls on every training and validation step.

    crit = NocsMinSymmetryCELoss({'nocs_class_name': 'screw', 'ce_loss_bins': 100})
    loss = crit(pred, target)                      # pred (B, N, 3*bins) logits, target (B, N, 3) in [0, 1]; a 0-d tensor
    loss.backward()
    loss = nocs_symce(pred, target, tfs, bins)     # the functional form, for any (S, 4, 4) set of transforms

The reference expands the logits to (B, N, 3, bins, n_sym) and runs CrossEntropyLoss on the expansion.  Here nothing of that size
exists: the forward reads the logits once (one log-sum-exp per point and axis, one gathered logit per point, axis and symmetry), the
backward reads them once and writes softmax minus the one-hot at the winning symmetry's bins.  Every sum is a stated f32 chain (the
header has them), so a result is the same bits on any run and any stream.

`pred` is used where it lies, in one of two storages, told apart by its strides: contiguous (B, N, 3*bins), which the HIP inference
forward returns, or a (B, 3*bins, N) tensor seen through .permute(0, 2, 1), which the training forward's last convolution hands over
(pointnet2.py:231).  Anything else raises: there is no hidden copy.  The gradient has the strides of `pred`.

bins <= 128, at most 128 symmetries, float32, HIP device tensors only; there is no CPU implementation and no double backward.  No
gradient flows to `target`."""
import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib as L
from ._lib import CatgraspAmdError, _p, _stream, check
from .transforms import get_symmetry_tfs

CHANNEL_MAJOR, POINT_MAJOR = 0, 1
MAX_BINS = MAX_SYM = 128

# what the last forward call handed to the kernel: the address of the logits and their storage (tests assert that it is pred's own)
last_pred_ptr = None
last_layout = None


def layouts_of(pred):
    """The storages that the strides of a (B, N, C) tensor fit: both when N or C is 1, none for a striding that would need a copy."""
    if pred.dim() != 3:
        raise ValueError(f'expected (B, N, 3*bins) logits, got {tuple(pred.shape)}')
    return ((POINT_MAJOR,) if pred.is_contiguous() else ()) + ((CHANNEL_MAJOR,) if pred.transpose(1, 2).is_contiguous() else ())


def layout_of(pred, layout=None):
    """CHANNEL_MAJOR or POINT_MAJOR for a (B, N, C) tensor, from its strides; any other striding raises.  Where the strides fit both
    (one point: the same bytes either way) point-major is taken unless `layout` names the other; a `layout` the strides do not fit raises."""
    fits = layouts_of(pred)
    if not fits or (layout is not None and layout not in fits):
        raise ValueError(f'logits of shape {tuple(pred.shape)} with strides {pred.stride()} are neither contiguous (B, N, C) nor a permuted '
                         'contiguous (B, C, N)' + ('' if layout is None else f', or not of the storage {layout} asked for') + ': the loss does not copy them')
    return fits[0] if layout is None else layout


def _check_inputs(pred, target, tfs, bins, layout=None):
    L.require_cuda(pred, target, tfs)
    if any(t.dtype != torch.float32 for t in (pred, target, tfs)):
        raise CatgraspAmdError('the NUNOCS loss is float32 only')
    layout = layout_of(pred, layout)
    B, N, C = pred.shape
    if C != 3 * bins or tuple(target.shape) != (B, N, 3) or tfs.dim() != 3 or tuple(tfs.shape[1:]) != (4, 4):
        raise ValueError(f'expected pred (B, N, {3 * bins}), target (B, N, 3), tfs (S, 4, 4); got {tuple(pred.shape)}, {tuple(target.shape)}, '
                         f'{tuple(tfs.shape)}')
    return layout, B, N, tfs.shape[0]


def _forward(pred, target, tfs, bins, keep_lse, layout=None):
    """-> (loss (1), ids (B) int32, L (B, S), lse (B, N, 3) or None) of detached inputs."""
    global last_pred_ptr, last_layout
    layout, B, N, S = _check_inputs(pred, target, tfs, bins, layout)
    size = int(L.lib().cg_nocs_symce_workspace_floats(B, N, bins, S))
    check(min(size, 0), 'cg_nocs_symce_workspace_floats')
    dev = pred.device
    ws = torch.empty((size,), dtype=torch.float32, device=dev)
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    ids = torch.empty((B,), dtype=torch.int32, device=dev)
    per_sym = torch.empty((B, S), dtype=torch.float32, device=dev)
    lse = torch.empty((B, N, 3), dtype=torch.float32, device=dev) if keep_lse else None
    last_pred_ptr, last_layout = pred.data_ptr(), layout
    check(L.lib().cg_nocs_symce_forward(_p(pred), layout, _p(target), _p(tfs), B, N, bins, S, _p(ws), _p(loss), _p(ids), _p(per_sym), _p(lse),
                                        _stream()), 'cg_nocs_symce_forward')
    return loss, ids, per_sym, lse


class NocsSymCEFunction(torch.autograd.Function):
    """(pred, target, tfs, bins, layout) -> (loss 0-d, ids (B) int32, L (B, S)); ids and L carry no gradient, and neither do target and
    tfs."""

    @staticmethod
    def forward(ctx, pred, target, tfs, bins, layout):
        layout = layout_of(pred, layout)
        loss, ids, per_sym, lse = _forward(pred.detach(), target, tfs, bins, True, layout)
        ctx.save_for_backward(pred, target, tfs, lse, ids)
        ctx.bins, ctx.layout = bins, layout
        ctx.mark_non_differentiable(ids, per_sym)
        return loss.reshape(()), ids, per_sym

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss, _grad_ids, _grad_per_sym):
        pred, target, tfs, lse, ids = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if grad_loss.dtype != torch.float32 or not grad_loss.is_cuda:
            raise NotImplementedError(f'the gradient of the NUNOCS loss must be a float32 device tensor, got {grad_loss.dtype} on {grad_loss.device}')
        B, N, _ = pred.shape
        grad = torch.empty_strided(pred.shape, pred.stride(), dtype=torch.float32, device=pred.device)
        g = grad_loss.contiguous()
        check(L.lib().cg_nocs_symce_backward(_p(pred), ctx.layout, _p(target), _p(tfs), _p(lse), _p(ids), _p(g), B, N, ctx.bins, tfs.shape[0],
                                             _p(grad), _stream()), 'cg_nocs_symce_backward')
        return grad, None, None, None, None


def nocs_symce_all(pred, target, tfs, bins, layout=None):
    """-> (loss 0-d, ids (B) int32, L (B, S)): the loss, the winning symmetry of every sample and the per-symmetry table it was taken
    from.  Where no gradient is asked for (torch.no_grad(), or a pred that needs none) the call is forward-only and keeps no lse.
    `layout` says which storage to take where the strides fit both (layout_of)."""
    bins = int(bins)
    target, tfs = target.detach().contiguous(), tfs.detach().contiguous()
    if torch.is_grad_enabled() and pred.requires_grad:
        return NocsSymCEFunction.apply(pred, target, tfs, bins, layout)
    loss, ids, per_sym, _ = _forward(pred.detach(), target, tfs, bins, False, layout)
    return loss.reshape(()), ids, per_sym


def nocs_symce(pred, target, tfs, bins):
    """The loss alone (a 0-d tensor) for the symmetry transforms tfs (S, 4, 4)."""
    return nocs_symce_all(pred, target, tfs, bins)[0]


class NocsMinSymmetryCELoss(nn.Module):
    """loss.py:16-45 with the reference's constructor and forward(pred, target).  After a call, `last_ids` (B) holds the winning
    symmetry of every sample and `last_per_symmetry` (B, S) the table of per-symmetry losses."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.bins = int(cfg['ce_loss_bins'])
        self.bin_resolution = 1 / self.bins
        tfs = torch.from_numpy(np.stack(get_symmetry_tfs(cfg['nocs_class_name'])).astype(np.float32))
        self.n_sym = len(tfs)
        self._tfs = {tfs.device: tfs}               # per device, filled on first use: the module holds no parameter to follow .to()
        self.last_ids = self.last_per_symmetry = None

    def symmetry_tfs(self, device=torch.device('cpu')):
        """The (n_sym, 4, 4) float32 transforms on `device`."""
        if device not in self._tfs:
            self._tfs[device] = self._tfs[torch.device('cpu')].to(device)
        return self._tfs[device]

    def forward(self, pred, target):
        L.require_cuda(pred, target)
        loss, self.last_ids, self.last_per_symmetry = nocs_symce_all(pred, target, self.symmetry_tfs(pred.device), self.bins)
        return loss
