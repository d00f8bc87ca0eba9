"""Yardstick of the PointGroup network in training mode (catgrasp_amd/pointgroup_train.py): the training forward and the offset loss in
torch on the CPU, float64 (or float32, to measure that precision's own noise), over the rule books of tests/sparse_ref.py, on the
scenes, test weights and point map of tests/pointgroup_ref.py.  Gradients are torch autograd's.

conv       one index_select / mm / index_add per kernel offset; pinned against sparse_ref.conv and sparse_grad_ref.grads by
           tests/test_pointgroup_train_ref_cpu.py.
BatchNorm  the explicit batch-statistics formulas.  `masks`: an optional list of ReLU masks, one per BatchNorm in the order the forward
           meets them (Run.keys), used as where(mask, z, 0).  With given masks the function is smooth around the device's evaluation:
           a mask that float32 flips at a pre-activation of 1e-6 changes a gradient by far more than any bar, and among 640k
           pre-activations there always is one.
"""
import functools

import numpy as np
import torch

import pointgroup_ref as P

EPS = P.EPS
MOMENTUM = 0.1
BAND = 1e-4                     # |float64 pre-activation| below this: the sign is float32's to decide
WEIGHT_SEED = 7                 # pointgroup_ref.make_params' default


def conv(x, nbr, w, b):
    """x (n_in, Cin) tensor, nbr (n_out, K) numpy, w (K, Cin, Cout) tensor, b (Cout) -> (n_out, Cout)."""
    out = b.expand(nbr.shape[0], w.shape[2])
    for k in range(nbr.shape[1]):
        rows = np.nonzero(nbr[:, k] >= 0)[0]
        if len(rows):
            out = out.index_add(0, torch.from_numpy(rows), x.index_select(0, torch.from_numpy(nbr[rows, k].astype(np.int64))) @ w[k])
    return out


@functools.lru_cache(maxsize=None)
def points(kind):
    """-> (input_map (N) int32, coords_float (N, 3) float32, instance_info (N, 9) float32, v2p_map (M, 1 + width) int32) of a scene:
    every point sits in its voxel (2 cm voxels, a seeded jitter inside), and its instance centre is the centroid of its batch item's
    points, so the offset targets point there."""
    idx = P.scene(kind)
    imap = P.point_map(len(idx))
    rng = np.random.default_rng(8)
    coords = ((idx[imap, 1:].astype(np.float64) + rng.uniform(0, 1, (len(imap), 3))) * 0.02).astype(np.float32)
    item = idx[imap, 0]
    info = np.zeros((len(imap), 9), np.float32)
    for b in np.unique(item):
        info[item == b, :3] = coords[item == b].astype(np.float64).mean(0).astype(np.float32)
    members = [np.nonzero(imap == v)[0] for v in range(len(idx))]
    v2p = np.zeros((len(idx), 1 + max(len(m) for m in members)), np.int32)
    for v, m in enumerate(members):
        v2p[v, 0] = len(m)
        v2p[v, 1:1 + len(m)] = m
    for a in (coords, info, v2p):
        a.setflags(write=False)
    return imap, coords, info, v2p


@functools.lru_cache(maxsize=None)
def params(seed=WEIGHT_SEED):
    """The test weights: pointgroup_ref.params() at the shipped seed."""
    if seed == WEIGHT_SEED:
        return P.params()
    lv = P.scene_levels('full')
    return P.make_params(lv, P.features(len(lv.indices)), seed=seed)


class Run(object):
    """One training forward + loss + backward.  After it: loss (float), pt_offsets (N, 3) numpy, grads {key: numpy}, keys (the
    BatchNorms in forward order), pre {key: (n, c) numpy pre-activations}, running {key + '.running_mean' / '.running_var': numpy}
    after the step."""

    def __init__(self, kind, dtype=torch.float64, masks=None, weights=None):
        weights = params() if weights is None else weights
        self.p = {k: torch.from_numpy(np.array(v)).to(dtype) for k, v in weights.items()}
        for k, t in self.p.items():
            if 'running' not in k:
                w = t.reshape(-1, t.shape[-2], t.shape[-1]) if t.dim() == 5 else t
                self.p[k] = w.clone().requires_grad_(True)
        self.dtype, self.masks = dtype, masks
        self.keys, self.pre, self.running = [], {}, {}
        lv = P.scene_levels(kind)
        imap, coords, info, _ = points(kind)
        x = conv(torch.from_numpy(P.features(len(lv.indices))).to(dtype), lv.subm, self.p['input_conv.0.weight'], self.p['input_conv.0.bias'])
        x = self.ublock(x, lv, 'unet', P.PLANES)
        y = self.bn_relu(x, 'output_layer.0')[torch.from_numpy(imap.astype(np.int64))]
        y = self.bn_relu(y @ self.p['offset.0.weight'].t() + self.p['offset.0.bias'], 'offset.1')
        pt = y @ self.p['offset.3.weight'].t() + self.p['offset.3.bias']
        gt = torch.from_numpy(np.array(info[:, :3])).to(dtype) - torch.from_numpy(np.array(coords)).to(dtype)
        loss = ((pt - gt) ** 2).mean()
        loss.backward()
        self.loss, self.pt_offsets = float(loss.detach()), pt.detach().numpy()
        self.grads = {k: t.grad.numpy().reshape(weights[k].shape) for k, t in self.p.items() if t.requires_grad and t.grad is not None}

    def bn_relu(self, x, key):
        n = x.shape[0]
        if n < 2:
            raise ValueError('Expected more than 1 value per channel when training')
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
        z = (x - mean) / torch.sqrt(var + EPS) * self.p[key + '.weight'] + self.p[key + '.bias']
        mask = z > 0 if self.masks is None else torch.from_numpy(np.asarray(self.masks[len(self.keys)]))
        assert mask.shape == z.shape, (key, mask.shape, z.shape)
        self.keys.append(key)
        self.pre[key] = z.detach().numpy()
        self.running[key + '.running_mean'] = ((1 - MOMENTUM) * self.p[key + '.running_mean'] + MOMENTUM * mean.detach()).numpy()
        self.running[key + '.running_var'] = ((1 - MOMENTUM) * self.p[key + '.running_var'] + MOMENTUM * var.detach() * n / (n - 1)).numpy()
        return torch.where(mask, z, torch.zeros((), dtype=self.dtype))

    def pre_conv(self, x, nbr, key, bn, cv):
        return conv(self.bn_relu(x, f'{key}.{bn}'), nbr, self.p[f'{key}.{cv}.weight'], self.p[f'{key}.{cv}.bias'])

    def block(self, x, nbr, key, cin, cout):
        if cin == cout:
            residual = x
        else:
            own = np.arange(x.shape[0], dtype=np.int32).reshape(-1, 1)
            residual = conv(x, own, self.p[key + '.i_branch.0.weight'], self.p[key + '.i_branch.0.bias'])
        h = self.pre_conv(x, nbr, key + '.conv_branch', 0, 2)
        return self.pre_conv(h, nbr, key + '.conv_branch', 3, 5) + residual

    def ublock(self, x, lv, key, planes):
        n = planes[0]
        for i in range(2):
            x = self.block(x, lv.subm, f'{key}.blocks.block{i}', n, n)
        if len(planes) > 1:
            d = self.pre_conv(x, lv.down_nbr, key + '.conv', 0, 2)
            d = self.ublock(d, lv.down, key + '.u', planes[1:])
            d = self.pre_conv(d, lv.inverse_nbr, key + '.deconv', 0, 2)
            x = torch.cat([x, d], dim=1)
            x = self.block(x, lv.subm, key + '.blocks_tail.block0', 2 * n, n)
            x = self.block(x, lv.subm, key + '.blocks_tail.block1', n, n)
        return x


@functools.lru_cache(maxsize=None)
def own(kind):
    """The float64 run under its own masks; computed once, shared, not to be written to."""
    return Run(kind)


def zero_by_mathematics(grads):
    """The biases whose gradient is zero by mathematics, read off the float64 gradients alone (below 1e-12, where the others are of
    order 1e-3): a constant added to every row in front of a BatchNorm in batch-statistics mode changes nothing.  These are
    input_conv.0.bias, offset.0.bias and every conv_branch.2.bias (directly in front of one), and every other convolution bias of the
    U-Net, which reaches a BatchNorm through identity, concatenation and 1x1x1 paths only: they hand a constant row on as one.  They have no scale
    of their own to be held to: a test asserts that they are small."""
    zero = sorted(k for k, g in grads.items() if float(np.abs(g).max()) < 1e-12)
    assert all(k.endswith('.bias') for k in zero)
    direct = [k for k in grads if k in ('input_conv.0.bias', 'offset.0.bias') or k.endswith('conv_branch.2.bias')]
    assert len(direct) == 28 and set(direct) <= set(zero), sorted(set(direct) - set(zero))
    return zero


def errors(got, want):
    """-> (max |got - want| / max(1, |want|), max |got - want| / max |want|)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want)
    top = float(np.abs(want).max(initial=0.0))
    return float((d / np.maximum(1.0, np.abs(want))).max(initial=0.0)), (float(d.max(initial=0.0)) / top if top > 0 else float('inf'))
