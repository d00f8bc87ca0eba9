"""The PointGroup offset network in training mode (the reference's PointGroup/model/pointgroup/pointgroup.py:20-110, 223-233 and its
offset loss and model_fn, :310-389), so that the checkpoints `PointGroupPredictor` loads can be made on this hardware.

`PointGroup(cfg)` is `pointgroup.PointGroup` with the sparse layers of `spconv_autograd`: same module tree, same state_dict keys, order
and shapes, same initial tensors under the same torch.manual_seed, so `pointgroup.load_model` loads what it saves, strictly.

  eval mode       the base class's fused forward, bit for bit.
  training mode   the base class's walk of the U-Net (UBlock.forward and the blocks') with _train_run in place of the fused launch:
                  every `BatchNorm1d, ReLU, conv` run is bn_relu_train (batch statistics, csrc/batchnorm_train.hip) followed by the
                  layer's SparseConvFunction; residuals are torch adds, skips torch.cat.  The head runs per point after the gather, as
                  the reference's does: the batch statistics of offset.1 run over the N points, not over the M voxels.  The two
                  nn.Linear are K = 1 SparseConvFunction calls, the gather is GatherRows, whose backward is the sum-mode voxelization
                  (members in ascending point order).  Every sum of a step, forward and backward, is therefore a fixed-order f32
                  chain and nothing uses atomics: a training step is a pure function of its inputs, bit for bit, on any run and any
                  stream.  A BatchNorm that sees a single row (a level with one voxel) raises torch's ValueError.

The score branch (epoch > prepare_epochs) is not built.  loss_fn is the offset loss alone; fix_module / pretrain_module, the optimiser
and the data loader belong to the training loop.

USE_TORCH_OPS wires the same network from nn.BatchNorm1d + nn.ReLU + torch indexing instead of the fused functions.  It exists as the
baseline of scripts/pointgroup_train_time.py and of one equality-within-bar test; torch states no summation order for it."""
import torch
from torch import nn

from . import pointgroup, pointgroup_ops
from . import spconv_autograd as spconv
from .batchnorm import bn_relu_train

USE_TORCH_OPS = False


def v2p_from_input_map(input_map, n_voxels):
    """(N) voxel row of every point -> (n_voxels, 1 + max members) int32 rows [count, member point ids ascending, 0 ...]: the
    output_map of pointgroup_ops.voxelization_idx, rebuilt with a stable sort."""
    rows = input_map.long()
    n, dev = rows.shape[0], rows.device
    order = torch.sort(rows, stable=True).indices                   # points by voxel, ascending point id inside a voxel
    counts = torch.bincount(rows, minlength=n_voxels)
    width = int(counts.max().item()) if n else 0
    voxel = rows[order]
    slot = torch.arange(n, device=dev) - (torch.cumsum(counts, 0) - counts)[voxel]
    out = torch.zeros((n_voxels, width + 1), dtype=torch.int32, device=dev)
    out[:, 0] = counts.int()
    out[voxel, slot + 1] = order.int()
    return out


class GatherRows(torch.autograd.Function):
    """features[input_map].  Backward: the rows of the gradient summed per voxel by pointgroup_ops.voxelization in sum mode over
    v2p_map -- one f32 chain from +0 over the voxel's points in ascending order, no atomics (torch's index_put would use them)."""

    @staticmethod
    def forward(ctx, features, input_map, v2p_map):
        ctx.save_for_backward(v2p_map)
        return features[input_map.long()]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        v2p_map, = ctx.saved_tensors
        return pointgroup_ops.voxelization(grad.contiguous(), v2p_map, mode=3), None, None


def gather_rows(features, input_map, v2p_map=None):
    if v2p_map is None:
        v2p_map = v2p_from_input_map(input_map, features.shape[0])
    return GatherRows.apply(features, input_map, v2p_map.int())


def _linear(x, lin):
    """nn.Linear as a K = 1 layer, so that its gradients are cg_sparse_conv_wgrad's and cg_sparse_conv_dgrad's chains."""
    rows = spconv.identity_rules(x.shape[0], x.device)
    return spconv.SparseConvFunction.apply(x, lin.weight.t().unsqueeze(0), lin.bias, rows, rows, False)


def _bn_relu(x, bn, relu):
    if USE_TORCH_OPS:
        return relu(bn(x))
    return bn_relu_train(x, bn)


def _train_run(input, bn, relu, conv, residual=None, features_b=None):
    """One `BatchNorm1d, ReLU, conv` run in training mode: the `run` of pointgroup's walk (pointgroup._fused is the eval-mode one).
    The walk is asked for torch.cat skips, so features_b stays None; a layer with gradients refuses anything else."""
    return conv(input.replace_feature(_bn_relu(input.features, bn, relu)), residual=residual, features_b=features_b)


class PointGroup(pointgroup.PointGroup):
    def __init__(self, cfg):
        super().__init__(cfg, layers=spconv)

    def forward(self, input_tensor, input_map, coords, batch_idxs, batch_offsets, epoch, v2p_map=None):
        """The reference's positional signature; v2p_map (M, 1 + maxActive) int32, the voxelization's output_map, spares rebuilding
        it from input_map for the gather's backward.  -> {'pt_offsets': (N, 3)}."""
        if not self.training:
            return super().forward(input_tensor, input_map, coords, batch_idxs, batch_offsets, epoch)
        if epoch > self.prepare_epochs:
            raise NotImplementedError('the score branch (epoch > prepare_epochs) is not built')
        output = self.unet(self.input_conv[0](input_tensor), run=_train_run, cat_skip=True)
        bn, relu = self.output_layer
        lin0, head_bn, head_relu, lin1 = self.offset
        voxel_feats = _bn_relu(output.features, bn, relu)
        if USE_TORCH_OPS:
            return {'pt_offsets': self.offset(voxel_feats[input_map.long()])}
        point_feats = gather_rows(voxel_feats, input_map, v2p_map)
        return {'pt_offsets': _linear(_bn_relu(_linear(point_feats, lin0), head_bn, head_relu), lin1)}


def loss_fn(loss_inp, epoch, cfg):
    """-> (loss, loss_out, infos).  The offset loss: the mean squared error between pt_offsets and instance_info[:, :3] - coords_float
    (the vector from every point to its instance's centre); the direction term is zero."""
    if epoch > cfg.prepare_epochs:
        raise NotImplementedError('the score loss (epoch > prepare_epochs) is not built')
    pt_offsets, coords_float, instance_info, instance_labels = loss_inp['pt_offsets']
    gt_offsets = instance_info[:, :3] - coords_float
    offset_norm_loss = nn.functional.mse_loss(pt_offsets, gt_offsets)
    offset_dir_loss = torch.zeros((), dtype=torch.float32, device=pt_offsets.device)
    loss_out = {'offset_norm_loss': (offset_norm_loss.item(), len(gt_offsets)), 'offset_dir_loss': (offset_dir_loss.item(), len(gt_offsets))}
    loss = cfg.loss_weight[1] * offset_norm_loss + cfg.loss_weight[2] * offset_dir_loss
    return loss, loss_out, {}


def model_fn_decorator(cfg, test=False):
    """-> model_fn(batch, model, epoch).  batch: the reference's keys (locs, voxel_locs, p2v_map, v2p_map, locs_float, feats, offsets,
    spatial_shape and, for training, instance_labels, instance_info, instance_pointnum).  Training: (loss, preds, visual_dict,
    meter_dict); test=True: preds."""
    def forward(batch, model, epoch):
        dev = torch.device('cuda', torch.cuda.current_device())
        coords = batch['locs'].to(dev)
        v2p_map = batch['v2p_map'].to(dev)
        coords_float = batch['locs_float'].to(dev)
        feats = batch['feats'].to(dev)
        if cfg.use_coords:
            feats = torch.cat((feats, coords_float), 1)
        voxel_feats = pointgroup_ops.voxelization(feats, v2p_map, cfg.mode)
        input_ = spconv.SparseConvTensor(voxel_feats, batch['voxel_locs'].to(dev).int(), batch['spatial_shape'], cfg.batch_size)
        extra = {'v2p_map': v2p_map} if isinstance(model, PointGroup) else {}
        ret = model(input_, batch['p2v_map'].to(dev), coords_float, coords[:, 0].int(), batch['offsets'].to(dev), epoch, **extra)
        return ret, coords_float

    def test_model_fn(batch, model, epoch):
        with torch.no_grad():
            ret, _ = forward(batch, model, epoch)
        return {'pt_offsets': ret['pt_offsets']}

    def model_fn(batch, model, epoch):
        ret, coords_float = forward(batch, model, epoch)
        dev = coords_float.device
        pt_offsets = ret['pt_offsets']
        loss_inp = {'pt_offsets': (pt_offsets, coords_float, batch['instance_info'].to(dev), batch['instance_labels'].to(dev))}
        loss, loss_out, _ = loss_fn(loss_inp, epoch, cfg)
        preds = {'pt_offsets': pt_offsets.detach()}
        visual_dict = {'loss': loss.item()}
        for k, v in loss_out.items():
            visual_dict[k] = v[0]
        return loss, preds, visual_dict, {}

    return test_model_fn if test else model_fn
