"""GPU tests of PointNet's encoder trained on HIP (catgrasp_amd/pool_autograd.py: tnet_train, encoder_train; the opt-in switch
pointnet2_train.ENCODER_ON_HIP) against float64 on the CPU and the torch-op path on the same device.

The whole encoder is ill-conditioned in float32 under ANY summation order (the FC tails of the two transform nets run BatchNorm over the
B rows; see test_pointnet_seg_train_gpu.py), so the torch-op path itself misses the suite's bar against float64 and the two paths'
errors are independent draws of the same magnitude.  Every tensor is therefore held to max(BAR, K * the torch-op path's error on the same
inputs), measured on the spot.  K is the smallest power of two >= twice the worst ratio (HIP error / torch-op error, over the tensors
where the HIP error is above BAR) measured at three seeds on an MI355X:

    model (B, N) = (6, 40)    seed  worst HIP vs f64  worst torch ops vs f64  worst ratio (tensor)                  logits HIP / torch ops
    PointNetSeg(6, 12)        0     2.21e-01          2.21e-01                1.36 (feat.stn.bn1.weight)            3.49e-05 / 2.35e-05
    PointNetSeg(6, 12)        1     3.77e-01          3.77e-01                1.00 (feat.stn.conv2.weight, others)  3.22e-05 / 2.14e-05
    PointNetSeg(6, 12)        2     4.44e-04          3.21e-01                0.002                                 2.25e-05 / 2.12e-05
    small 8 -> 16 -> 32 -> 64  0, 1, 2   2.53e-05, 5.34e-05, 1.49e-05 against 1.21e-05, 4.02e-05, 2.75e-05: every tensor inside the bar

Twice the worst ratio is 2.73, so K = 4.  No ratio came near 8; at seed 2 the torch-op path drew an error 700 times the HIP path's.
Outputs and buffers are inside the plain bar in both paths at every seed (trans_feat at most 1.32e-05, running statistics at most
2.7e-06); only gradients leave it.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import dense_train_ref as R
from catgrasp_amd import dense_autograd as D, pointnet2, pointnet2_train, pool_autograd as PA

pytestmark = pytest.mark.gpu

K = 4
B, N = 6, 40


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _perturb(model, seed):
    """BatchNorm weights and biases off their 1 / 0 start (some weights of the pooled layers negative: the min branch)."""
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'bn' in name and name.endswith('weight'):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
                if name.endswith('bn3.weight') and p.numel() >= 64:
                    p[::7].neg_()
            if 'bn' in name and name.endswith('bias'):
                p.add_(0.2 * torch.randn(p.shape, generator=g))


def _step(fn, model, x, weights):
    model.zero_grad(set_to_none=True)
    outs = fn(model, x)
    sum((o * w).sum() for o, w in zip(outs, weights)).backward()
    return [o.detach() for o in outs], {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _compare(fn_hip, fn_torch, model, x, weights, names):
    """-> rows {tensor: (HIP vs float64, torch ops vs float64)} over the outputs `names`, every parameter gradient and every buffer."""
    ref64 = copy.deepcopy(model).cpu().double().train()
    o64, g64 = _step(fn_torch, ref64, x.cpu().double(), [w.cpu().double() for w in weights])
    tor, hip = copy.deepcopy(model).train(), copy.deepcopy(model).train()
    ot, gt = _step(fn_torch, tor, x, weights)
    oh, gh = _step(fn_hip, hip, x, weights)
    assert set(gh) == set(g64) == set(gt) and len(gh) == len(list(model.parameters()))
    cpu = lambda t: t.double().cpu().numpy()
    rows = {n: (R.rel_err(cpu(a), cpu(r)), R.rel_err(cpu(b), cpu(r))) for n, a, b, r in zip(names, oh, ot, o64)}
    for k in gh:
        assert gh[k].shape == g64[k].shape and torch.isfinite(gh[k]).all(), k
        rows[k] = (R.rel_err(cpu(gh[k]), cpu(g64[k])), R.rel_err(cpu(gt[k]), cpu(g64[k])))
    want = dict(ref64.named_buffers())
    for k, b in hip.named_buffers():
        rows['buffer ' + k] = (R.rel_err(cpu(b), cpu(want[k])), R.rel_err(cpu(dict(tor.named_buffers())[k]), cpu(want[k])))
    return rows, gh


def _report(rows, what):
    ratios = {k: eh / et for k, (eh, et) in rows.items() if eh > R.BAR and et > 0}
    worst = max(ratios.values(), default=0.0)
    print(f'{what}: {len(rows)} tensors, worst HIP vs float64 {max(r[0] for r in rows.values()):.2e}, worst torch ops vs float64 '
          f'{max(r[1] for r in rows.values()):.2e}, worst ratio above the bar {worst:.2f}')
    for k, (eh, et) in rows.items():
        print(f'  {k}: HIP {eh:.2e}, torch ops {et:.2e}' + (f', ratio {ratios[k]:.2f}' if k in ratios else ''))
    return worst


# ------------------------------------------------------------------------------------------------------------- A: real widths
def _seg_inputs(seed, device, n_out=12):
    torch.manual_seed(seed)
    model = pointnet2_train.PointNetSeg(6, n_out)
    _perturb(model, seed)
    rng = np.random.default_rng(seed)
    x = _dev(rng.normal(0, 0.5, (B, N, 6)).astype(np.float32), device)
    wl = _dev(R.dy_for(B * N, n_out, seed=seed + 3).reshape(B, N, n_out), device)
    wt = _dev(rng.uniform(-1, 1, (B, 64, 64)).astype(np.float32) / 64, device)
    return model.to(device), x, (wl, wt)


def _seg_hip(model, x):
    old = pointnet2_train.ENCODER_ON_HIP
    pointnet2_train.ENCODER_ON_HIP = True
    try:
        return model(x)
    finally:
        pointnet2_train.ENCODER_ON_HIP = old


def _seg_torch(model, x):
    """The torch-op arithmetic of the whole model (pointnet2.PointNetSeg's training forward), in the model's own dtype and device."""
    return pointnet2.PointNetSeg.forward(model, x) if x.dtype == torch.float64 else _with(pointnet2_train, 'USE_TORCH_OPS', True, lambda: model(x))


def _with(mod, name, value, fn):
    old = getattr(mod, name)
    setattr(mod, name, value)
    try:
        return fn()
    finally:
        setattr(mod, name, old)


def seg_rows(seed, device):
    model, x, weights = _seg_inputs(seed, device)
    return _compare(_seg_hip, _seg_torch, model, x, weights, ('logits', 'trans_feat'))


def test_real_widths_with_the_switch_on(cuda_device):
    model, x, _ = _seg_inputs(0, cuda_device)
    base = pointnet2.PointNetSeg(6, 12).to(cuda_device)
    base.load_state_dict(model.state_dict(), strict=True)
    assert list(model.state_dict()) == list(base.state_dict())
    model.eval(); base.eval()
    with torch.no_grad():
        (ya, ta), (yb, tb) = _seg_hip(model, x), base(x)
    assert torch.equal(ya, yb) and torch.equal(ta, tb)              # eval mode is untouched by the switch
    rows, gh = seg_rows(0, cuda_device)
    assert len(gh) == 70
    _report(rows, f'PointNetSeg, encoder on HIP, (B, N) = {(B, N)}')
    for k, (eh, et) in rows.items():
        assert eh <= max(R.BAR, K * et), (k, eh, et)


# ------------------------------------------------------------------------------------------------------- B: small, width-agnostic
class _SmallTNet(nn.Module):
    def __init__(self, cin, k, widths=(16, 32, 64), fc=(32, 16)):
        super().__init__()
        w = [cin, *widths]
        for i in range(3):
            setattr(self, f'conv{i + 1}', nn.Conv1d(w[i], w[i + 1], 1))
        self.fc1, self.fc2, self.fc3 = nn.Linear(widths[2], fc[0]), nn.Linear(fc[0], fc[1]), nn.Linear(fc[1], k * k)
        for i, c in enumerate([*widths, *fc]):
            setattr(self, f'bn{i + 1}', nn.BatchNorm1d(c))
        self._k = k


class _SmallEncoder(nn.Module):
    """The module tree encoder_train walks, at widths 8 -> 16 -> 32 -> pooled 64 (none of them PointNet's)."""

    def __init__(self, channel=8):
        super().__init__()
        self.stn = _SmallTNet(channel, 3)
        self.conv1, self.conv2, self.conv3 = nn.Conv1d(channel, 16, 1), nn.Conv1d(16, 32, 1), nn.Conv1d(32, 64, 1)
        self.bn1, self.bn2, self.bn3 = nn.BatchNorm1d(16), nn.BatchNorm1d(32), nn.BatchNorm1d(64)
        self.fstn = _SmallTNet(16, 16)


def _torch_tnet(t, h):
    for i in (1, 2, 3):
        h = F.relu(getattr(t, f'bn{i}')(getattr(t, f'conv{i}')(h)))
    g = h.max(dim=2)[0]
    g = F.relu(t.bn4(t.fc1(g)))
    g = F.relu(t.bn5(t.fc2(g)))
    return (t.fc3(g) + torch.eye(t._k, device=g.device, dtype=g.dtype).reshape(1, -1)).view(-1, t._k, t._k)


def _torch_encoder(enc, x):
    """pointnet2_train.PointNetSeg._encode's torch-op walk, for any widths."""
    trans = _torch_tnet(enc.stn, x.transpose(2, 1))
    xyz = torch.bmm(x[:, :, :3], trans)
    pts = torch.cat([xyz, x[:, :, 3:]], dim=2) if x.shape[2] > 3 else xyz
    h = F.relu(enc.bn1(enc.conv1(pts.transpose(2, 1))))
    trans_feat = _torch_tnet(enc.fstn, h)
    pointfeat = torch.bmm(h.transpose(2, 1), trans_feat)
    h = F.relu(enc.bn2(enc.conv2(pointfeat.transpose(2, 1))))
    h = enc.bn3(enc.conv3(h))
    return h.max(dim=2)[0], pointfeat, trans_feat


def small_rows(seed, device):
    torch.manual_seed(seed)
    enc = _SmallEncoder()
    _perturb(enc, seed)
    rng = np.random.default_rng(seed)
    x = _dev(rng.normal(0, 0.5, (B, N, 8)).astype(np.float32), device)
    weights = [_dev(rng.uniform(-1, 1, s).astype(np.float32) / np.sqrt(np.prod(s)), device) for s in ((B, 64), (B, N, 16), (B, 16, 16))]
    return _compare(PA.encoder_train, _torch_encoder, enc.to(device), x, weights, ('g', 'pointfeat', 'trans_feat'))


def test_the_walk_reads_every_width_from_the_modules(cuda_device):
    rows, gh = small_rows(0, cuda_device)
    assert len(gh) == len(list(_SmallEncoder().parameters()))
    _report(rows, 'small encoder 8 -> 16 -> 32 -> 64')
    for k, (eh, et) in rows.items():
        assert eh <= max(R.BAR, K * et), (k, eh, et)


# ------------------------------------------------------------------------------------------------------- C: unchanged behaviour
def test_the_default_training_forward_is_the_torch_op_encoder_and_the_hip_head(cuda_device, monkeypatch):
    """With the switch off (the default) the training forward is the parent's: the encoder on torch ops, restated here, and
    seg_head_train, bit for bit on the same seed."""
    assert pointnet2_train.ENCODER_ON_HIP is False
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    model, x, _ = _seg_inputs(1, cuda_device)
    twin = copy.deepcopy(model)
    model.train(); twin.train()
    logits, trans_feat = model(x)
    g, pointfeat, tf = _torch_encoder(twin.feat, x)
    want = D.seg_head_train(g, pointfeat, (twin.conv1, twin.conv2, twin.conv3, twin.conv4), (twin.bn1, twin.bn2, twin.bn3))
    assert torch.equal(logits, want) and torch.equal(trans_feat, tf)
    for (k, a), (_, b) in zip(model.named_buffers(), twin.named_buffers()):
        assert torch.equal(a, b), k
