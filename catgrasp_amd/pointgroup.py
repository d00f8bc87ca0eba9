"""The reference's PointGroup network (PointGroup/model/pointgroup/pointgroup.py:20-263) assembled from the sparse layers of
`catgrasp_amd.spconv`: ResidualBlock, VGGBlock, UBlock and PointGroup(cfg), with the reference's module tree, constructor arguments and
state_dict keys and shapes, so that its checkpoints load strictly.

Inference only.  The predictor calls the model with epoch = prepare_epochs - 1, so a forward runs input_conv, the 7-level U-Net,
output_layer, the gather by the point-to-voxel map and the offset head.  The eval-mode forward is written against the fused launches
instead of through SparseSequential:

  ResidualBlock n -> n     2 launches: BatchNorm + ReLU is the prologue of each convolution, the block's input the residual of the second.
  ResidualBlock 2n -> n    3 launches, after the skip: the k = 3 convolution and the k = 1 i_branch read [skip | decoder] -- through the
                           two-source kernel (cg_sparse_conv_cat, no torch.cat) with USE_TWO_SOURCE_KERNEL, else from one torch.cat per
                           skip; the n -> n convolution takes the i_branch result as its residual.
  conv, deconv             1 launch each, prologue folded.
  head                     offset(output_layer(x).features[input_map]) is the head applied per voxel and then gathered: two K = 1
                           launches on the voxel rows (16 -> 16 with output_layer's BatchNorm + ReLU as prologue, 16 -> 3 with the head's
                           own), then one 3-float row gather by input_map.

The blocks' and UBlock's forward are the only walk of the module tree (block order, skip, residual, recursion).  They take `run`,
how one `BatchNorm1d, ReLU, conv` is executed: `_fused` by default, `pointgroup_train._train_run` for a training step.

At the shipped configuration (m = 16, block_reps = 2, residual blocks) that is 71 + 2 launches and 19 rule-book builds (7 submanifold,
6 strided, 6 inverse).  The score branch (epoch > prepare_epochs) draws torch.rand and is training-time only: it is constructed, for the
checkpoint's keys, and not run."""
import argparse
import functools
from collections import OrderedDict

import torch
import yaml
from torch import nn

from . import spconv
from .spconv import SparseModule


# Whether the skip's 2n -> n block reads its two sources through cg_sparse_conv_cat or through torch.cat + cg_sparse_conv: the same
# bits either way.  Measured (profiles/pointgroup_time.json): the two-source pair of launches wins at n = 16 and
# is not faster than torch.cat + cg_sparse_conv at n = 96, so the forward concatenates.
USE_TWO_SOURCE_KERNEL = False

_FOLDED = '_cg_folded'


def _prologue(bn):
    """(scale, shift) of an eval-mode BatchNorm1d, kept on the module and remade when one of its four tensors has been replaced or
    written in place (load_state_dict, .to(), copy_, fill_ ...: torch's version counters).  A write through `.data` moves no counter
    and is NOT seen: call model.eval() (or .train()) afterwards, which drops every kept pair."""
    ts = (bn.running_mean, bn.running_var, bn.weight, bn.bias)
    stamp = tuple((t.data_ptr(), t._version) for t in ts) + (bn.eps,)
    kept = bn.__dict__.get(_FOLDED)
    if kept is None or kept[0] != stamp:
        kept = (stamp, spconv.bn_relu_prologue(bn))
        bn.__dict__[_FOLDED] = kept
    return kept[1]


def _fused(input, bn, relu, conv, residual=None, features_b=None):
    """How the walk (the blocks' and UBlock's forward) runs one `BatchNorm1d, ReLU, conv`: the one decision in which the eval-mode
    and the training forward differ, taken as the walk's `run` argument.  This is the eval-mode run, one launch; the training
    one is pointgroup_train._train_run."""
    return conv(input, prologue=_prologue(bn), residual=residual, features_b=features_b)


def _subm3(cin, cout, key, layers=spconv):
    """layers: the module that supplies the three sparse layer classes -- `spconv`, or its drop-in with gradients."""
    return layers.SubMConv3d(cin, cout, kernel_size=3, padding=1, bias=True, indice_key=key)


def _pre_activated(norm_fn, width, conv):
    """BatchNorm, ReLU, convolution: the run that becomes one launch (the convolution with a prologue)."""
    return [norm_fn(width), nn.ReLU(), conv]


class ResidualBlock(SparseModule):
    """i_branch (identity, or a k = 1 convolution when the widths differ) + conv_branch (two pre-activated k = 3 convolutions).
    Eval mode: 2 launches, 3 with an i_branch."""

    def __init__(self, in_channels, out_channels, norm_fn, indice_key=None, layers=spconv):
        super().__init__()
        shortcut = nn.Identity() if in_channels == out_channels else layers.SubMConv3d(in_channels, out_channels, kernel_size=1, bias=True)
        self.i_branch = spconv.SparseSequential(shortcut)
        self.conv_branch = spconv.SparseSequential(*_pre_activated(norm_fn, in_channels, _subm3(in_channels, out_channels, indice_key, layers)),
                                                   *_pre_activated(norm_fn, out_channels, _subm3(out_channels, out_channels, indice_key, layers)))

    def forward(self, input, features_b=None, run=_fused):
        """features_b: the block reads [input.features | features_b] (the block behind a skip).  run: see _fused."""
        bn0, relu0, conv0, bn1, relu1, conv1 = self.conv_branch
        shortcut = self.i_branch[0]
        if isinstance(shortcut, nn.Identity):
            if features_b is not None:
                raise ValueError('a block of equal widths has one source')
            residual = input.features
        else:
            residual = shortcut(input, features_b=features_b).features
        hidden = run(input, bn0, relu0, conv0, features_b=features_b)
        return run(hidden, bn1, relu1, conv1, residual=residual)


class VGGBlock(SparseModule):
    """One pre-activated k = 3 convolution: 1 launch."""

    def __init__(self, in_channels, out_channels, norm_fn, indice_key=None, layers=spconv):
        super().__init__()
        self.conv_layers = spconv.SparseSequential(*_pre_activated(norm_fn, in_channels, _subm3(in_channels, out_channels, indice_key, layers)))

    def forward(self, input, features_b=None, run=_fused):
        return run(input, *self.conv_layers, features_b=features_b)


class UBlock(nn.Module):
    """One U-Net level of width nPlanes[0]: `blocks`; then, unless it is the last level, `conv` (strided, to nPlanes[1]), the next
    level `u`, `deconv` (its inverse) and `blocks_tail`, whose first block reads [this level's output | the decoder's] and narrows
    the doubled width back.  Rule books: 'subm<id>' for every block of the level, 'spconv<id>' for conv and deconv."""

    def __init__(self, nPlanes, norm_fn, block_reps, block, indice_key_id=1, layers=spconv):
        super().__init__()
        self.nPlanes = nPlanes
        width, subm, strided = nPlanes[0], f'subm{indice_key_id}', f'spconv{indice_key_id}'

        def group(first_in):
            return spconv.SparseSequential(OrderedDict(
                (f'block{i}', block(first_in if i == 0 else width, width, norm_fn, indice_key=subm, layers=layers)) for i in range(block_reps)))
        self.blocks = group(width)
        if len(nPlanes) > 1:
            below = nPlanes[1]
            self.conv = spconv.SparseSequential(*_pre_activated(
                norm_fn, width, layers.SparseConv3d(width, below, kernel_size=2, stride=2, bias=True, indice_key=strided)))
            self.u = UBlock(nPlanes[1:], norm_fn, block_reps, block, indice_key_id=indice_key_id + 1, layers=layers)
            self.deconv = spconv.SparseSequential(*_pre_activated(
                norm_fn, below, layers.SparseInverseConv3d(below, width, kernel_size=2, bias=True, indice_key=strided)))
            self.blocks_tail = group(2 * width)

    def forward(self, input, run=_fused, cat_skip=False):
        """run: see _fused.  cat_skip: the skip is one torch.cat whatever USE_TWO_SOURCE_KERNEL says (the two-source kernel has
        no gradient)."""
        output = input
        for blk in self.blocks:
            output = blk(output, run=run)
        if len(self.nPlanes) > 1:
            decoder = run(self.u(run(output, *self.conv), run, cat_skip), *self.deconv)
            first, *rest = self.blocks_tail
            if USE_TWO_SOURCE_KERNEL and not cat_skip:
                output = first(output, features_b=decoder.features, run=run)
            else:
                output = first(output.replace_feature(torch.cat((output.features, decoder.features), dim=1)), run=run)
            for blk in rest:
                output = blk(output, run=run)
        return output


# cfg attributes the model keeps under its own names, as the reference's model does (its training loop reads them there)
_KEPT = {'cluster_radius': 'cluster_radius', 'cluster_meanActive': 'cluster_meanActive', 'cluster_shift_meanActive': 'cluster_shift_meanActive',
         'cluster_npoint_thre': 'cluster_npoint_thre', 'score_fullscale': 'score_fullscale', 'mode': 'score_mode',
         'prepare_epochs': 'prepare_epochs', 'pretrain_module': 'pretrain_module', 'fix_module': 'fix_module'}


class PointGroup(nn.Module):
    def __init__(self, cfg, layers=spconv):
        """layers: see _subm3; `pointgroup_train.PointGroup` passes the layers with gradients."""
        super().__init__()
        self.cfg = cfg
        for own, theirs in _KEPT.items():
            setattr(self, own, getattr(cfg, theirs))
        m = cfg.m
        channels = cfg.input_channel + (3 if cfg.use_coords else 0)
        if 14 * m > spconv.MAX_CIN or 7 * m > spconv.MAX_COUT or m % 16 or channels != 6:
            raise NotImplementedError(f'the layer kernel takes 6 input channels and widths that are multiples of 16 up to {spconv.MAX_COUT} '
                                      f'({spconv.MAX_CIN} after a skip): m = {m} with {channels} input channels is not built')
        norm_fn = functools.partial(nn.BatchNorm1d, eps=1e-5, momentum=0.1)
        block = ResidualBlock if cfg.block_residual else VGGBlock

        self.input_conv = spconv.SparseSequential(_subm3(channels, m, 'subm1', layers))
        self.unet = UBlock([m * level for level in range(1, 8)], norm_fn, cfg.block_reps, block, indice_key_id=1, layers=layers)
        self.output_layer = spconv.SparseSequential(norm_fn(m), nn.ReLU())
        self.offset = nn.Sequential(nn.Linear(m, m), norm_fn(m), nn.ReLU(), nn.Linear(m, 3))
        # the score branch: never run here (forward), constructed because checkpoints hold its tensors and load strictly
        self.score_unet = UBlock([m, 2 * m], norm_fn, 2, block, indice_key_id=1, layers=layers)
        self.score_outputlayer = spconv.SparseSequential(norm_fn(m), nn.ReLU())
        self.score_linear = nn.Linear(m, 1)
        self.apply(self.set_bn_init)

    @staticmethod
    def set_bn_init(module):
        """Every BatchNorm starts at gamma = 1, beta = 0."""
        if 'BatchNorm' in type(module).__name__:
            nn.init.ones_(module.weight)
            nn.init.zeros_(module.bias)

    def train(self, mode=True):
        for module in self.modules():               # a mode switch drops the folded BatchNorm constants (_prologue)
            module.__dict__.pop(_FOLDED, None)
        return super().train(mode)

    def _refuse_training(self):
        if self.training:
            raise NotImplementedError('catgrasp_amd.pointgroup is inference only: call model.eval() first')

    def unet_features(self, input_tensor):
        """input_conv and the U-Net on the fused launches -> SparseConvTensor with the input's sites and row order, m channels."""
        self._refuse_training()
        with torch.no_grad():
            return self.unet(self.input_conv[0](input_tensor))

    def head(self, voxel_features):
        """offset(output_layer(.)) per voxel row: (M, m) -> (M, 3) in two K = 1 launches."""
        self._refuse_training()
        with torch.no_grad():
            rows = spconv.identity_rules(voxel_features.shape[0], voxel_features.device)
            lin0, bn, lin1 = self.offset[0], self.offset[1], self.offset[3]
            scale, shift = _prologue(self.output_layer[0])
            hidden = spconv.sparse_conv(voxel_features, rows, lin0.weight.detach().t().unsqueeze(0), lin0.bias.detach(), scale, shift)
            scale, shift = _prologue(bn)
            return spconv.sparse_conv(hidden, rows, lin1.weight.detach().t().unsqueeze(0), lin1.bias.detach(), scale, shift)

    def forward(self, input_tensor, input_map, coords, batch_idxs, batch_offsets, epoch):
        """input_tensor: the voxel SparseConvTensor; input_map (N) the voxel row of every point.  coords, batch_idxs and batch_offsets
        feed the score branch alone and are not read.  -> {'pt_offsets': (N, 3)}."""
        self._refuse_training()
        if epoch > self.prepare_epochs:
            raise NotImplementedError('the score branch (epoch > prepare_epochs) is training-time only and is not built')
        voxel_offsets = self.head(self.unet_features(input_tensor).features)
        return {'pt_offsets': voxel_offsets[input_map.long()]}


def config_from_yaml(path):
    """The reference's util/config.py: every leaf of the YAML file, whatever section it sits in, becomes an attribute."""
    with open(path, 'r') as f:
        config = yaml.safe_load(f)
    args = argparse.Namespace(config=path)

    def key_to_attr(section):
        for k, v in section.items():
            if isinstance(v, dict):
                key_to_attr(v)
            else:
                setattr(args, k, v)
    key_to_attr(config)
    return args


def load_model(model, ckpt_path):
    """Utils.load_model: the 'state_dict' entry of the checkpoint if it has one, 'module.' stripped from the key names, loaded
    strictly (a missing or unexpected key raises)."""
    state_dict = torch.load(ckpt_path, map_location=torch.device('cpu'), weights_only=False)
    if 'state_dict' in state_dict:
        state_dict = state_dict['state_dict']
    state_dict = OrderedDict((name.replace('module.', ''), v) for name, v in state_dict.items())
    if len(state_dict) == 0:
        raise ValueError(f'{ckpt_path} holds no tensors')
    model.load_state_dict(state_dict)
    return model
