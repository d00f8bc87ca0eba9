"""GPU tests of PointNetSeg's per-point head in training mode (catgrasp_amd/dense_autograd.py: seg_head_train) and of the trainable model
(catgrasp_amd/pointnet2_train.py) against the float64 yardstick of tests/dense_train_ref.py, torch autograd in float64 on the CPU and
the torch-op path on the same device."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

import dense_train_ref as R
from catgrasp_amd import dense_autograd as D, loss as nl, pointnet2, pointnet2_train

pytestmark = pytest.mark.gpu


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _head_modules(P, device, dtype=torch.float32):
    W = R.HEAD_WIDTHS
    widths = [W['cg'] + W['cp'], *W['hidden'], W['n_out']]
    convs = [nn.Conv1d(widths[i], widths[i + 1], 1) for i in range(4)]
    bns = [nn.BatchNorm1d(c, eps=R.bn_ref.EPS) for c in W['hidden']]
    with torch.no_grad():
        for i, c in enumerate(convs):
            c.weight.copy_(torch.from_numpy(P[f'w{i + 1}']).unsqueeze(2)); c.bias.copy_(torch.from_numpy(P[f'b{i + 1}']))
        for i, b in enumerate(bns):
            b.weight.copy_(torch.from_numpy(P[f'gamma{i + 1}'])); b.bias.copy_(torch.from_numpy(P[f'beta{i + 1}']))
            b.running_mean.normal_(generator=torch.Generator().manual_seed(i)); b.running_var.uniform_(0.5, 2, generator=torch.Generator().manual_seed(i))
    return [m.to(device=device, dtype=dtype).train() for m in convs], [m.to(device=device, dtype=dtype).train() for m in bns]


@pytest.mark.parametrize('B,N', [(1, 2), (2, 33), (3, 65)])
def test_head_logits_and_every_gradient_match_float64(B, N, cuda_device):
    c = R.head_case(B, N)
    convs, bns = _head_modules(c['P'], cuda_device)
    g, pf = _dev(c['g'], cuda_device).requires_grad_(True), _dev(c['pf'], cuda_device).requires_grad_(True)
    logits = D.seg_head_train(g, pf, convs, bns)
    assert logits.shape == (B, N, R.HEAD_WIDTHS['n_out']) and logits.is_contiguous()
    logits.backward(_dev(c['dlogits'], cuda_device))
    got = dict(g=g.grad, pf=pf.grad)
    for i, m in enumerate(convs):
        got[f'w{i + 1}'], got[f'b{i + 1}'] = m.weight.grad.squeeze(2), m.bias.grad
    for i, m in enumerate(bns):
        got[f'gamma{i + 1}'], got[f'beta{i + 1}'] = m.weight.grad, m.bias.grad
    assert set(got) == set(c['grads'])
    worst = {'logits': R.rel_err(logits.detach().cpu().numpy(), c['rec']['logits'])}
    for k, v in got.items():
        assert v is not None and v.shape == c['grads'][k].shape, k
        worst[k] = R.rel_err(v.cpu().numpy(), c['grads'][k])          # every element: nothing is masked out
    print(f'head B={B} N={N}: ' + ', '.join(f'{k} {e:.2e}' for k, e in worst.items()))
    assert max(worst.values()) <= R.BAR, worst
    # the running statistics: torch's own update, from torch's own float64 modules on the CPU
    rc, rb = _head_modules(c['P'], 'cpu', torch.float64)
    h = torch.cat([torch.from_numpy(c['g']).double().unsqueeze(2).expand(-1, -1, N), torch.from_numpy(c['pf']).double().transpose(1, 2)], 1)
    for i in range(3):
        h = torch.relu(rb[i](rc[i](h)))
    for i in range(3):
        assert int(bns[i].num_batches_tracked) == int(rb[i].num_batches_tracked) == 1
        assert R.rel_err(bns[i].running_mean.cpu().numpy(), rb[i].running_mean.numpy()) <= R.BAR
        assert R.rel_err(bns[i].running_var.cpu().numpy(), rb[i].running_var.numpy()) <= R.BAR


def _models(n_out, device, seed=0):
    torch.manual_seed(seed)
    ours = pointnet2_train.PointNetSeg(6, n_out)
    # a few optimiser-free perturbations so that BatchNorm weights and biases are not at their 1 / 0 start
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in ours.named_parameters():
            if name.endswith('bn1.weight') or name.endswith('bn2.weight') or name.endswith('bn3.weight'):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            if 'bn' in name and name.endswith('bias'):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
    base = pointnet2.PointNetSeg(6, n_out)
    base.load_state_dict(ours.state_dict(), strict=True)
    return ours.to(device), base.to(device)


def _step(model, x, wl, wt):
    model.zero_grad(set_to_none=True)
    logits, trans_feat = model(x)
    ((logits * wl).sum() + (trans_feat * wt).sum()).backward()
    return logits.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


@pytest.mark.parametrize('n_out', [12, 300])
def test_model_matches_the_torch_op_path_and_float64(n_out, cuda_device, monkeypatch):
    """Training forward and every parameter gradient of pointnet2_train.PointNetSeg at (B, N) = (2, 40), against the torch-op path on the
    same device and against float64 on the CPU, under the suite's bar 1e-4 * max(1, |ref|) per element.  Where the torch-op path --
    the parent's arithmetic -- itself misses the bar against float64 on these inputs, the HIP path is allowed twice the torch-op
    path's measured error for that tensor (both are f32 chains of the same length in another order); the comparison is made on the
    spot, on the same inputs.  The real widths do NOT meet the plain bar at B = 2, in either path: STN3d's and STNkd's FC tails run
    BatchNorm over the B = 2 rows, whose gradient is a difference of nearly equal terms scaled by invstd, and float32 rounding of the
    shared encoder forward is amplified by it.  Measured on an MI355X, max over elements of |err| / max(1, |ref|):

        n_out  tensor                    HIP vs float64   torch ops vs float64   HIP vs torch ops
        12     logits                    1.40e-02         1.40e-02               8.85e-06
        12     worst (stn.conv1.weight)  9.18e+02         9.18e+02               2.17e-02
        12     head conv1..4 weights     9.34e-01 max     9.34e-01 max           3.86e-05 max
        12     head bn1..3 weight, bias  5.40e-02 max     5.40e-02 max           2.53e-06 max
        300    logits                    8.28e-02         8.28e-02               8.02e-06
        300    worst (stn.conv2.weight)  1.04e+03         1.04e+03               6.94e-04
        300    head conv1..4 weights     7.92e+00 max     7.92e+00 max           1.20e-04 max
        300    head bn1..3 weight, bias  3.73e-01 max     3.73e-01 max           1.35e-05 max

    Most of the 70 gradients are outside the plain bar in BOTH paths, by the same amount to two or three digits; the head at
    well-conditioned widths is held to the plain bar by test_head_logits_and_every_gradient_match_float64."""
    B, N = 2, 40
    ours, base = _models(n_out, cuda_device)
    sd = ours.state_dict()
    assert list(sd) == list(base.state_dict()) and all(sd[k].shape == v.shape for k, v in base.state_dict().items())
    rng = np.random.default_rng(n_out)
    x = _dev(rng.normal(0, 0.5, (B, N, 6)).astype(np.float32), cuda_device)
    wl = _dev(R.dy_for(B * N, n_out, seed=3).reshape(B, N, n_out), cuda_device)
    wt = _dev(rng.uniform(-1, 1, (B, 64, 64)).astype(np.float32) / 64, cuda_device)

    ours.eval(); base.eval()
    with torch.no_grad():
        (ya, ta), (yb, tb) = ours(x), base(x)
    assert torch.equal(ya, yb) and torch.equal(ta, tb)

    ref64 = copy.deepcopy(base).cpu().double().train()
    l64, g64 = _step(ref64, x.cpu().double(), wl.cpu().double(), wt.cpu().double())
    tor = copy.deepcopy(ours).train()
    hip = copy.deepcopy(ours).train()
    monkeypatch.setattr(pointnet2_train, 'USE_TORCH_OPS', True)
    lt, gt = _step(tor, x, wl, wt)
    monkeypatch.setattr(pointnet2_train, 'USE_TORCH_OPS', False)
    lh, gh = _step(hip, x, wl, wt)
    assert lh.shape == (B, N, n_out) and lh.is_contiguous()
    assert len(gh) == len(list(hip.parameters())) == 70 and set(gh) == set(g64) == set(gt)          # every parameter, none left out

    cpu = lambda t: t.cpu().numpy()
    rows = {'logits': (R.rel_err(cpu(lh), cpu(l64)), R.rel_err(cpu(lt), cpu(l64)), R.rel_err(cpu(lh), cpu(lt)))}
    for k in gh:
        rows[k] = (R.rel_err(cpu(gh[k]), cpu(g64[k])), R.rel_err(cpu(gt[k]), cpu(g64[k])), R.rel_err(cpu(gh[k]), cpu(gt[k])))
    for k, b in hip.named_buffers():
        want = dict(ref64.named_buffers())[k]
        rows['buffer ' + k] = (R.rel_err(cpu(b.double()), cpu(want.double())), R.rel_err(cpu(dict(tor.named_buffers())[k].double()), cpu(want.double())), 0.0)
    worst = [max(r[i] for r in rows.values()) for i in range(3)]
    print(f'n_out={n_out}: worst HIP vs float64 {worst[0]:.2e}, torch ops vs float64 {worst[1]:.2e}, HIP vs torch ops {worst[2]:.2e}')
    for k, (eh, et, ed) in rows.items():
        if eh > R.BAR or ed > R.BAR:
            print(f'  {k}: HIP {eh:.2e}, torch ops {et:.2e}, HIP vs torch ops {ed:.2e}')
    for k, (eh, et, ed) in rows.items():
        assert eh <= max(R.BAR, 2 * et), (k, eh, et)
        assert ed <= max(R.BAR, 3 * et), (k, ed, et)          # |hip - torch| <= |hip - f64| + |torch - f64|


def _train_three_steps(device, seed):
    torch.manual_seed(seed)
    model = pointnet2_train.PointNetSeg(6, 300).to(device).train()
    crit = nl.NocsMinSymmetryCELoss({'nocs_class_name': 'nut', 'ce_loss_bins': 100})
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((2, 64, 6), generator=g).mul_(0.5).to(device)
    target = torch.rand((2, 64, 3), generator=g).to(device)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        logits, _ = model(x)
        loss = crit(logits, target)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return model, torch.stack(losses), x


def test_three_adam_steps_are_bit_identical_and_the_checkpoint_loads_into_the_inference_model(cuda_device, monkeypatch):
    """Three Adam steps of the whole model with the device loss, repeated from the same seed, give the same bits.  The encoder runs on
    torch ops, whose library kernels state no summation order: the flag by which torch asks its convolution and BatchNorm library for
    deterministic kernels is set for the test (without it this test was seen to fail in one of three runs on an MI355X, and to pass
    with identical bits in every step of twelve repeated trainings in the other two; with it, in nine fresh processes out of
    nine).  The head needs no flag:
    test_three_adam_steps_of_the_head_alone_are_bit_identical."""
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    m1, l1, x = _train_three_steps(cuda_device, 5)
    m2, l2, _ = _train_three_steps(cuda_device, 5)
    assert torch.isfinite(l1).all() and torch.equal(l1, l2)
    sd1, sd2 = m1.state_dict(), m2.state_dict()
    for k in sd1:
        assert torch.equal(sd1[k], sd2[k]), k
    assert int(sd1['bn1.num_batches_tracked']) == 3
    base = pointnet2.PointNetSeg(6, 300).to(cuda_device)
    base.load_state_dict(sd1, strict=True)
    base.eval(); m1.eval()
    with torch.no_grad():
        (ya, ta), (yb, tb) = base(x), m1(x)
    assert torch.equal(ya, yb) and torch.equal(ta, tb)


def _train_head_three_steps(device):
    c = R.head_case(3, 65)
    convs, bns = _head_modules(c['P'], device)
    params = [p for m in convs + bns for p in m.parameters()]
    opt = torch.optim.Adam(params, lr=1e-2)
    crit = nl.NocsMinSymmetryCELoss({'nocs_class_name': 'nut', 'ce_loss_bins': R.HEAD_WIDTHS['n_out'] // 3})
    g, pf = _dev(c['g'], device), _dev(c['pf'], device)
    target = torch.rand((3, 65, 3), generator=torch.Generator().manual_seed(2)).to(device)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = crit(D.seg_head_train(g, pf, convs, bns), target)
        loss.backward()
        opt.step()
        losses.append(loss.detach().clone())
    return torch.stack(losses), [p.detach().clone() for p in params] + [b.running_var.clone() for b in bns]


def test_three_adam_steps_of_the_head_alone_are_bit_identical(cuda_device):
    """No torch library kernel with an unstated order is in the head's step: no flag is needed."""
    l1, p1 = _train_head_three_steps(cuda_device)
    l2, p2 = _train_head_three_steps(cuda_device)
    assert torch.isfinite(l1).all() and float(l1[2]) < float(l1[0]) and torch.equal(l1, l2)
    for a, b in zip(p1, p2):
        assert torch.equal(a, b)


def test_refusals(cuda_device):
    model = pointnet2_train.PointNetSeg(6, 12).to(cuda_device).train()
    with pytest.raises(NotImplementedError, match='HIP device'):
        model(torch.zeros(2, 8, 6))
    with pytest.raises(NotImplementedError, match='float32'):
        model(torch.zeros((2, 8, 6), device=cuda_device, dtype=torch.float64))
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        model(torch.zeros((1, 1, 6), device=cuda_device))
    c = R.head_case(2, 33)
    convs, bns = _head_modules(c['P'], cuda_device)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        D.seg_head_train(_dev(c['g'][:1], cuda_device), _dev(c['pf'][:1, :1], cuda_device), convs, bns)
    assert int(bns[0].num_batches_tracked) == 0
    logits = D.seg_head_train(_dev(c['g'], cuda_device), _dev(c['pf'], cuda_device), convs, bns)
    logits.sum().backward()
    with pytest.raises(RuntimeError, match='second time'):
        logits.sum().backward()
    g = _dev(c['g'], cuda_device).requires_grad_(True)
    out = D.seg_head_train(g, _dev(c['pf'], cuda_device), convs, bns)
    first, = torch.autograd.grad(out.sum(), g, create_graph=True)
    with pytest.raises(RuntimeError):          # once differentiable: there is no double backward
        first.sum().backward()
