"""PointNetSeg, the NUNOCS per-point classifier, with its per-point head trained on HIP (the reference's pointnet2.py:302-329 under
trainer_nunocs.py), so that the checkpoints the NUNOCS predicter loads can be made on this hardware.

`PointNetSeg(n_in, n_out)` is `pointnet2.PointNetSeg`: same module tree, same state_dict keys, order and shapes, same initial tensors
under the same torch.manual_seed, so a state_dict saved here loads strictly into `pointnet2.PointNetSeg` and back.

  eval mode       the base class's forward, bit for bit.
  training mode   the encoder (STN3d, STNkd, conv1 .. conv3 with their BatchNorms, the three max-pools) on torch ops, walked here so that
                  the global feature g (B, 1024) and the per-point feature (B, N, 64) -- point-major straight out of the bmm with
                  the feature transform -- stay separate; then dense_autograd.seg_head_train: the first layer split into one product
                  per cloud and one per point, BatchNorm + ReLU with batch statistics on csrc/batchnorm_train.hip, every weight,
                  bias and input gradient a stated f32 chain (csrc/dense_train.hip).  The (B, 1088, N) concatenation and its gradient
                  are never formed.  Returns (logits (B, N, n_out) contiguous, trans_feat), the storage loss.py takes without a copy.

Refused in training mode: anything but float32, host tensors, B * N < 2 (torch's ValueError), a second backward through the same
graph and double backward (the functions are once differentiable).  n_out must be a multiple of 4.

USE_TORCH_OPS runs the head on torch ops over the same walk (the concatenation, Conv1d, BatchNorm1d, relu: the arithmetic of
`pointnet2.PointNetSeg`'s training forward).  It is the baseline of scripts/pointnet_seg_train_time.py and of one
equality-within-bar test; torch states no summation order for it.

ENCODER_ON_HIP (opt-in, False by default: the default training forward keeps its bits) walks the encoder on HIP as well
(pool_autograd.encoder_train): the 64- and 128-wide per-point layers through dense_autograd.linear + bn_relu_train (the 6 -> 64 layers
on rows and weights zero-padded to 8 columns), the three conv + BatchNorm + max-pool layers (stn.conv3, fstn.conv3 with ReLU, conv3
without) through pool_autograd.conv_bn_max_train, whose closed form stores no (B N, 1024) tensor forward or backward.  What stays on
torch ops with the switch set: the two bmm's and the FC tails of the two transform nets on B rows.  USE_TORCH_OPS keeps precedence;
eval mode is untouched."""
import torch
import torch.nn.functional as F

from . import pointnet2
from .dense_autograd import seg_head_train
from .pool_autograd import encoder_train

USE_TORCH_OPS = False
ENCODER_ON_HIP = False


class PointNetSeg(pointnet2.PointNetSeg):
    """forward(x (B, N, D)) -> ((B, N, n_out), trans_feat (B, 64, 64))."""

    def _encode(self, x):
        """The training-mode encoder on torch ops (PointNetEncoder._torch_forward without the concatenation), or, with ENCODER_ON_HIP,
        pool_autograd.encoder_train: -> (g (B, 1024), pointfeat (B, N, 64) point-major, trans_feat)."""
        enc = self.feat
        if ENCODER_ON_HIP and not USE_TORCH_OPS:
            return encoder_train(enc, x)
        D = x.shape[2]
        trans = enc.stn._torch_forward(x.transpose(2, 1))
        xyz = torch.bmm(x[:, :, :3], trans)
        pts = torch.cat([xyz, x[:, :, 3:]], dim=2) if D > 3 else xyz
        h = F.relu(enc.bn1(enc.conv1(pts.transpose(2, 1))))
        trans_feat = enc.fstn._torch_forward(h)
        pointfeat = torch.bmm(h.transpose(2, 1), trans_feat)
        h = F.relu(enc.bn2(enc.conv2(pointfeat.transpose(2, 1))))
        h = enc.bn3(enc.conv3(h))
        return h.max(dim=2)[0], pointfeat, trans_feat

    def _torch_head(self, g, pointfeat):
        N = pointfeat.shape[1]
        f = torch.cat([g.unsqueeze(2).expand(-1, -1, N), pointfeat.transpose(2, 1)], 1)
        h = F.relu(self.bn1(self.conv1(f)))
        h = F.relu(self.bn2(self.conv2(h)))
        h = F.relu(self.bn3(self.conv3(h)))
        return self.conv4(h).permute(0, 2, 1)

    def forward(self, x):
        if not self.training:
            return super().forward(x)
        if USE_TORCH_OPS:
            g, pointfeat, trans_feat = self._encode(x)
            return self._torch_head(g, pointfeat), trans_feat
        if x.dtype != torch.float32 or not x.is_cuda:
            raise NotImplementedError(f'pointnet2_train.PointNetSeg trains in float32 on a HIP device only (there is no CPU fallback), got '
                                      f'{x.dtype} on {x.device}')
        if x.dim() != 3:
            raise ValueError(f'expected points (B, N, D), got {tuple(x.shape)}')
        if x.shape[0] * x.shape[1] < 2:
            raise ValueError(f'Expected more than 1 value per channel when training, got input size {torch.Size((x.shape[0], 64, x.shape[1]))}')
        if self.conv4.out_channels % 4:
            raise NotImplementedError(f'the head trains with n_out a multiple of 4, got {self.conv4.out_channels}')
        g, pointfeat, trans_feat = self._encode(x)
        logits = seg_head_train(g, pointfeat, (self.conv1, self.conv2, self.conv3, self.conv4), (self.bn1, self.bn2, self.bn3))
        return logits, trans_feat
