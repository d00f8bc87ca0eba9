"""GPU tests of the PointGroup network in training mode (catgrasp_amd/pointgroup_train.py) at the shipped configuration, under the
seeded test weights of tests/pointgroup_ref.py.

Yardstick: tests/pointgroup_train_ref.py, float64 on the CPU, evaluated under the DEVICE's ReLU masks, so that it is the smooth function
the device evaluated (tests/test_pointgroup_train_ref_cpu.py: 0.013 % of the float64 pre-activations lie within 1e-4 of zero, where
float32 decides the sign; every disagreement between the device's masks and float64's own must lie in that band).  The masks are read
off the output of bn_relu_train: the fused function calls no BatchNorm1d or ReLU module, so a forward hook on those never fires (the
torch-op baseline is taken with forward hooks on its nn.ReLU modules).

Bars: 1e-4 * max(1, |ref|) per element, and 1e-4 * max |ref| of the tensor (the gradients are below one, where the first bar alone
would be an absolute one).  tests/test_pointgroup_train_ref_cpu.py holds float32's own noise to a quarter of both.  The bias gradients
that are zero by mathematics (pointgroup_train_ref.zero_by_mathematics) have no scale of their own and are asserted to be small."""
import functools
import os

import numpy as np
import pytest
import torch
from torch import nn

import catgrasp_amd.spconv as base_spconv
import pointgroup_ref as P
import pointgroup_train_ref as T
from catgrasp_amd import _lib, pointgroup, pointgroup_train

pytestmark = pytest.mark.gpu

BAR = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_KEPT = {}


def _cfg():
    return pointgroup.config_from_yaml(os.path.join(GOLDEN, 'config_pointgroup.yaml'))


def _model(dev):
    """The training model under the test weights, put back to them (and to training mode, without gradients) on every call."""
    if 'model' not in _KEPT:
        model = pointgroup_train.PointGroup(_cfg())
        sd = model.state_dict()
        sd.update({k: torch.from_numpy(v) for k, v in P.params().items()})
        _KEPT['state'] = {k: v.clone() for k, v in sd.items()}
        _KEPT['model'] = model.to(dev)
    model = _KEPT['model']
    model.load_state_dict(_KEPT['state'])
    model.zero_grad(set_to_none=True)
    return model.train()


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _inputs(kind, dev):
    idx = P.scene(kind)
    imap, coords, info, v2p = T.points(kind)
    tensor = base_spconv.SparseConvTensor(_dev(P.features(len(idx)), dev), _dev(idx, dev), P.SHAPE, P.BATCH)
    return tensor, _dev(imap, dev), _dev(coords, dev), _dev(info, dev), _dev(v2p, dev)


def _step(model, kind, dev, with_v2p=True):
    """One forward + loss + backward -> (loss tensor, pt_offsets, {key: grad})."""
    tensor, imap, coords, info, v2p = _inputs(kind, dev)
    ret = model(tensor, imap, coords, None, None, 0, v2p_map=v2p if with_v2p else None)
    loss, _, _ = pointgroup_train.loss_fn({'pt_offsets': (ret['pt_offsets'], coords, info, None)}, 0, model.cfg)
    loss.backward()
    return loss.detach(), ret['pt_offsets'].detach(), {k: p.grad for k, p in model.named_parameters()}


def _record_fused_masks(monkeypatch, model):
    names = {id(m): n for n, m in model.named_modules() if isinstance(m, nn.BatchNorm1d)}
    masks, real = {}, pointgroup_train.bn_relu_train

    def recorded(x, bn):
        y = real(x, bn)
        masks[names[id(bn)]] = (y.detach() > 0).cpu().numpy()
        return y
    monkeypatch.setattr(pointgroup_train, 'bn_relu_train', recorded)
    return masks


def _check_step(kind, masks, loss, pt_offsets, grads, state, what):
    """Everything a step produced against float64 under the step's own masks."""
    own = T.own(kind)
    assert sorted(masks) == sorted(own.keys)
    flipped = outside = 0
    for k in own.keys:
        differ = masks[k] != (own.pre[k] > 0)
        flipped += int(differ.sum())
        outside += int((differ & (np.abs(own.pre[k]) >= T.BAND)).sum())
    print(f'{what} {kind}: {flipped} masks differ from float64\'s own sign, {outside} of them outside the band of {T.BAND:g}')
    assert outside == 0
    want = T.Run(kind, masks=[masks[k] for k in own.keys])
    err_loss = abs(float(loss) - want.loss)
    elem, rel = T.errors(pt_offsets.cpu().numpy(), want.pt_offsets)
    print(f'{what} {kind}: loss {float(loss):.6g}, |got - ref| {err_loss:.3g}; pt_offsets {elem:.3g} per element, {rel:.3g} of the tensor (bar {BAR:g})')
    assert err_loss <= BAR * max(1.0, abs(want.loss)) and elem <= BAR and rel <= BAR
    for k, stat in want.running.items():
        e = T.errors(state[k].cpu().numpy(), stat)[0]
        assert e <= BAR, (k, e)
        assert int(state[k.rsplit('.', 1)[0] + '.num_batches_tracked']) == 1
    zero = T.zero_by_mathematics(want.grads)
    worst, worst_zero = ('', 0.0, 0.0), 0.0
    for k, g in grads.items():
        if k.startswith('score_'):
            assert g is None, k                                              # the unrun branch
            continue
        got = g.cpu().numpy()
        assert np.isfinite(got).all(), k
        if k in zero:
            worst_zero = max(worst_zero, float(np.abs(got).max()))
            assert np.abs(got).max() <= BAR, (k, float(np.abs(got).max()))   # zero by mathematics: small, and no relative bar
            continue
        elem, rel = T.errors(got, want.grads[k])
        if rel > worst[2]:
            worst = (k, elem, rel)
        assert elem <= BAR and rel <= BAR, (k, elem, rel)
    assert sum(not k.startswith('score_') for k in grads) == len(want.grads)
    print(f'{what} {kind}: worst gradient {worst[0]}: {worst[1]:.3g} per element, {worst[2]:.3g} of its tensor\'s max (bar {BAR:g}); '
          f'largest of the {len(zero)} gradients that are zero by mathematics: {worst_zero:.3g}')


@pytest.mark.parametrize('kind', ['full', 'n33'])
def test_a_step_against_float64_under_the_devices_masks(kind, cuda_device, monkeypatch):
    model = _model(cuda_device)
    masks = _record_fused_masks(monkeypatch, model)
    loss, pt_offsets, grads = _step(model, kind, cuda_device)
    assert pt_offsets.shape == (len(P.scene(kind)) + 40, 3) and pt_offsets.dtype == torch.float32
    _check_step(kind, masks, loss, pt_offsets, grads, model.state_dict(), 'fused')
    assert all(int(v) == 0 for k, v in model.state_dict().items() if k.startswith('score_') and k.endswith('num_batches_tracked'))


def test_launch_counts_of_one_training_forward(cuda_device, monkeypatch):
    """One training forward on scene n33 (33 voxels, the smallest scene whose every level keeps more than one row): 73 cg_sparse_conv
    launches (input_conv, the 70 layers of the U-Net, the two nn.Linear of the head) and 66 cg_bn_relu_train_forward calls (the 64
    BatchNorms of the U-Net, output_layer's and offset.1), never the two-source kernel.  Both figures were counted at commit 55cfb43,
    before the training forward became the inference model's walk with another `run`."""
    model = _model(cuda_device)
    lib = _lib.lib()
    counts = {}

    def counted(name):
        fn = getattr(lib, name)

        def call(*args):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args)
        monkeypatch.setattr(lib, name, call)
    for name in ('cg_sparse_conv', 'cg_sparse_conv_cat', 'cg_bn_relu_train_forward'):
        counted(name)
    tensor, imap, coords, _, v2p = _inputs('n33', cuda_device)
    model(tensor, imap, coords, None, None, 0, v2p_map=v2p)
    assert counts == {'cg_sparse_conv': 73, 'cg_bn_relu_train_forward': 66}


def test_the_torch_op_baseline_is_the_same_network(cuda_device, monkeypatch):
    """The wiring behind USE_TORCH_OPS (nn.BatchNorm1d, nn.ReLU, torch indexing, nn.Linear), which scripts/pointgroup_train_time.py
    times the fused step against: within the bars of float64 under ITS masks, and its loss and offsets within the bar of the fused
    step's."""
    model = _model(cuda_device)
    fused_loss, fused_offsets, _ = _step(model, 'full', cuda_device)
    model = _model(cuda_device)
    monkeypatch.setattr(pointgroup_train, 'USE_TORCH_OPS', True)
    masks, hooks = {}, []
    for name, seq in model.named_modules():
        if name.startswith('score_') or not isinstance(seq, (base_spconv.SparseSequential, nn.Sequential)):
            continue
        for i, (child, m) in enumerate(seq.named_children()):
            if isinstance(m, nn.ReLU):
                bn = f'{name}.{list(seq._modules)[i - 1]}'
                hooks.append(m.register_forward_hook(lambda mod, args, out, bn=bn: masks.__setitem__(bn, (out.detach() > 0).cpu().numpy())))
    try:
        loss, pt_offsets, grads = _step(model, 'full', cuda_device)
    finally:
        for h in hooks:
            h.remove()
    _check_step('full', masks, loss, pt_offsets, grads, model.state_dict(), 'torch ops')
    assert abs(float(loss) - float(fused_loss)) <= BAR * max(1.0, abs(float(fused_loss)))
    assert T.errors(pt_offsets.cpu().numpy(), fused_offsets.cpu().numpy())[0] <= BAR


def test_a_step_is_bit_reproducible_and_the_same_on_a_side_stream(cuda_device):
    def run(kind, **kw):
        loss, pt_offsets, grads = _step(_model(cuda_device), kind, cuda_device, **kw)
        return [loss, pt_offsets] + [g for k, g in sorted(grads.items()) if g is not None]
    for kind in ('full', 'n33'):
        first, again, rebuilt = run(kind), run(kind), run(kind, with_v2p=False)
        side = torch.cuda.Stream(device=cuda_device)
        side.wait_stream(torch.cuda.current_stream(cuda_device))
        with torch.cuda.stream(side):
            other = run(kind)
        side.synchronize()
        assert len(first) == 2 + 278
        for a, b, c, d in zip(first, again, other, rebuilt):
            assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d), kind


@functools.lru_cache(maxsize=None)
def _gather_case():
    """50 voxels, 400 points: about eight members per voxel, so that the order of a voxel's sum shows in its bits; voxel 7 has none."""
    rng = np.random.default_rng(21)
    imap = rng.integers(49, size=400)
    imap[imap >= 7] += 1
    grad = (rng.uniform(-1, 1, (400, 16)) * 10.0 ** rng.integers(-3, 3, (400, 1))).astype(np.float32)
    want32, descending = np.zeros((50, 16), np.float32), np.zeros((50, 16), np.float32)
    for v in range(50):
        members = np.nonzero(imap == v)[0]
        for i in members:
            want32[v] = want32[v] + grad[i]
        for i in members[::-1]:
            descending[v] = descending[v] + grad[i]
    want64 = np.zeros((50, 16))
    np.add.at(want64, imap, grad.astype(np.float64))
    assert (want32.view(np.uint32) != descending.view(np.uint32)).mean() > 0.2      # the order is there to be seen
    return imap.astype(np.int32), grad, want32, want64


def test_gather_rows_backward_is_the_ascending_chain(cuda_device):
    imap, grad, want32, want64 = _gather_case()
    d_map = _dev(imap, cuda_device)
    v2p = pointgroup_train.v2p_from_input_map(d_map, 50)
    assert v2p.shape[0] == 50 and int(v2p[7, 0]) == 0
    for given in (v2p, None):
        feats = torch.rand((50, 16), device=cuda_device).requires_grad_(True)
        out = pointgroup_train.gather_rows(feats, d_map, given)
        assert torch.equal(out.detach(), feats.detach()[d_map.long()])
        out.backward(_dev(grad, cuda_device))
        got = feats.grad.cpu().numpy()
        assert T.errors(got, want64)[0] <= BAR
        assert np.array_equal(got.view(np.uint32), want32.view(np.uint32)) and not got[7].any()


def test_refusals(cuda_device):
    model = _model(cuda_device)
    tensor, imap, coords, _, v2p = _inputs('n1', cuda_device)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        model(tensor, imap[:1] * 0, coords[:1], None, None, 0)
    tensor, imap, coords, _, v2p = _inputs('n33', cuda_device)
    with pytest.raises(NotImplementedError, match='score branch'):
        model(tensor, imap, coords, None, None, model.prepare_epochs + 1)
    inference = pointgroup.PointGroup(_cfg()).to(cuda_device).train()
    with pytest.raises(NotImplementedError, match='inference only'):
        inference(tensor, imap, coords, None, None, 0)


def test_eval_mode_is_the_inference_models_forward(cuda_device):
    model = _model(cuda_device).eval()
    inference = pointgroup.PointGroup(_cfg())
    inference.load_state_dict(model.state_dict(), strict=True)
    inference = inference.to(cuda_device).eval()
    for kind in ('full', 'n1'):
        tensor, imap, coords, _, _ = _inputs(kind, cuda_device)
        a = model(tensor, imap, coords, None, None, 0)['pt_offsets']
        tensor, imap, coords, _, _ = _inputs(kind, cuda_device)
        b = inference(tensor, imap, coords, None, None, 0)['pt_offsets']
        assert torch.equal(a, b) and not a.requires_grad


def test_twenty_sgd_steps_learn_and_the_checkpoint_deploys_on_the_inference_model(cuda_device, tmp_path):
    cfg = _cfg()
    idx = P.scene('n33')
    imap, coords, info, v2p = T.points('n33')
    item = idx[imap, 0]
    batch = {'locs': torch.from_numpy(np.concatenate([item[:, None], idx[imap, 1:]], 1).astype(np.int64)),
             'voxel_locs': torch.from_numpy(idx.astype(np.int64)), 'p2v_map': torch.from_numpy(imap), 'v2p_map': torch.from_numpy(np.array(v2p)),
             'locs_float': torch.from_numpy(np.array(coords)), 'feats': torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, (len(imap), 3)).astype(np.float32)),
             'instance_labels': torch.from_numpy(item.astype(np.int64)), 'instance_info': torch.from_numpy(np.array(info)),
             'instance_pointnum': torch.from_numpy(np.bincount(item).astype(np.int32)),
             'offsets': torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(item, minlength=P.BATCH))]).astype(np.int32)),
             'spatial_shape': list(P.SHAPE)}
    torch.manual_seed(0)
    model = pointgroup_train.PointGroup(cfg).to(cuda_device).train()
    model_fn = pointgroup_train.model_fn_decorator(cfg)
    optimiser = torch.optim.SGD([p for n, p in model.named_parameters() if not n.startswith('score_')], lr=0.02)
    losses = []
    for _ in range(20):
        optimiser.zero_grad()
        loss, preds, visual_dict, meter_dict = model_fn(batch, model, 0)
        loss.backward()
        optimiser.step()
        losses.append(visual_dict['loss'])
    print('loss over 20 SGD steps:', ' '.join(f'{v:.4g}' for v in losses))
    assert sorted(visual_dict) == ['loss', 'offset_dir_loss', 'offset_norm_loss'] and meter_dict == {} and list(preds) == ['pt_offsets']
    assert preds['pt_offsets'].shape == (len(imap), 3) and not preds['pt_offsets'].requires_grad
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    path = str(tmp_path / 'pointgroup_trained.pth')
    torch.save({'state_dict': model.state_dict()}, path)
    deployed = pointgroup.load_model(pointgroup.PointGroup(cfg), path).to(cuda_device).eval()
    test_fn = pointgroup_train.model_fn_decorator(cfg, test=True)
    a = test_fn(batch, model.eval(), 0)['pt_offsets']
    b = test_fn(batch, deployed, 0)['pt_offsets']
    assert torch.equal(a, b) and float(a.abs().max()) > 0
