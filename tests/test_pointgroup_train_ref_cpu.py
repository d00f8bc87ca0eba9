"""CPU tests of the training yardstick (tests/pointgroup_train_ref.py) and of the conditions the GPU bars of
tests/test_pointgroup_train_gpu.py rest on; and what of catgrasp_amd/pointgroup_train.py needs no device: the module tree, the
state_dict, the initial tensors, the rebuilt point lists and the loss.

Measured here, scene `full` under pointgroup_ref.params(): 639,760 pre-activations in 66 BatchNorms, 82 of them (0.013 %) within
1e-4 of zero and 7 within 1e-5.  The float32 restatement under float64's masks stays a factor of four or more below the GPU bars
(the test prints the figures)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import pointgroup_ref as P
import pointgroup_train_ref as T
import sparse_grad_ref as gref
import sparse_ref as R
from catgrasp_amd import pointgroup, pointgroup_train

BAR = 1e-4
N_BN = 66                       # 52 in the 26 residual blocks, 6 + 6 in front of the strided and inverse layers, 2 in the head
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _cfg():
    return pointgroup.config_from_yaml(os.path.join(GOLDEN, 'config_pointgroup.yaml'))


def test_conv_and_its_autograd_gradients_are_the_sparse_yardsticks():
    lv = P.scene_levels('n33')
    for nbr, n_in, cin, cout in ((lv.subm, 33, 16, 32), (lv.down_nbr, 33, 16, 32), (lv.inverse_nbr, len(lv.out_indices), 32, 16),
                                 (np.arange(33, dtype=np.int32).reshape(-1, 1), 33, 32, 16)):
        rng = np.random.default_rng(cin + nbr.shape[1])
        x, w = rng.uniform(-1, 1, (n_in, cin)), rng.uniform(-1, 1, (nbr.shape[1], cin, cout))
        b, dy = rng.uniform(-1, 1, cout), rng.uniform(-1, 1, (nbr.shape[0], cout))
        tx, tw, tb = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, b))
        out = T.conv(tx, nbr, tw, tb)
        out.backward(torch.from_numpy(dy))
        dw, dx, db = gref.grads(x, nbr, w, dy)
        for got, want in ((out.detach(), R.conv(x, nbr, w, b)), (tw.grad, dw), (tx.grad, dx), (tb.grad, db)):
            assert T.errors(got.numpy(), want)[0] <= 1e-12


def test_every_level_of_the_training_scenes_has_two_rows():
    counts = {kind: P.scene_levels(kind).counts() for kind in ('full', 'n33', 'item0_empty')}
    print(counts)
    assert all(min(c) >= 2 and len(c) == 7 for c in counts.values())
    assert counts['full'][0] == 600 and counts['n33'][0] == 33 and counts['item0_empty'][0] == 150
    assert min(P.scene_levels('n1').counts()) == 1
    with pytest.raises(ValueError, match='more than 1 value'):
        T.Run('n1')


def test_the_doubtful_band_is_thin():
    run = T.own('full')
    assert len(run.keys) == N_BN and len(set(run.keys)) == N_BN and run.keys[-2:] == ['output_layer.0', 'offset.1']
    z = np.concatenate([np.abs(run.pre[k]).ravel() for k in run.keys])
    inside, closer = int((z < T.BAND).sum()), int((z < 1e-5).sum())
    print(f'{z.size} pre-activations, {inside} ({100.0 * inside / z.size:.3f} %) within {T.BAND:g} of zero, {closer} within 1e-5')
    assert inside <= 0.0005 * z.size
    assert run.pre['offset.1'].shape == (640, 16) and run.pre['output_layer.0'].shape == (600, 16)     # the head's BatchNorm sees the points


def test_float32_under_float64s_masks_stays_within_a_quarter_of_the_gpu_bars():
    want = T.own('full')
    masks = [want.pre[k] > 0 for k in want.keys]
    again = T.Run('full', masks=masks)
    assert again.loss == want.loss and all(np.array_equal(again.grads[k], want.grads[k]) for k in want.grads)   # given masks are its own
    got = T.Run('full', dtype=torch.float32, masks=masks)
    assert abs(got.loss - want.loss) <= 0.25 * BAR * max(1.0, abs(want.loss))
    worst = {'pt_offsets': T.errors(got.pt_offsets, want.pt_offsets)}
    assert worst['pt_offsets'][0] <= 0.25 * BAR
    score = [k for k in P.params() if k.startswith('score_')]
    assert not score                                                       # the test weights hold no tensor of the unrun branch
    assert sorted(got.grads) == sorted(want.grads) and len(want.grads) == 2 * N_BN + 2 * 71 + 4
    zero = T.zero_by_mathematics(want.grads)
    print(f'{len(zero)} bias gradients are zero by mathematics:', ' '.join(zero))
    for k in sorted(want.grads):
        elem, rel = T.errors(got.grads[k], want.grads[k])
        if k in zero:
            assert np.abs(want.grads[k]).max() < 1e-12 and np.abs(got.grads[k]).max() <= 0.25 * BAR, k
            continue
        worst[k] = (elem, rel)
        assert elem <= 0.25 * BAR and rel <= 0.25 * BAR, (k, elem, rel)
    for k, stat in want.running.items():
        assert T.errors(got.running[k], stat)[0] <= 0.25 * BAR, k
    top = max(worst, key=lambda k: worst[k][1] if k != 'pt_offsets' else 0)
    print(f'float32 vs float64 under the same masks: loss {abs(got.loss - want.loss):.3g}, pt_offsets {worst["pt_offsets"][0]:.3g}, '
          f'worst gradient {top}: {worst[top][1]:.3g} of its tensor\'s max (a quarter of the bar: {0.25 * BAR:g})')


# ------------------------------------------------------------------------------------------------ the module, without a device
def test_module_tree_state_dict_and_initial_tensors_are_the_inference_models():
    cfg = _cfg()
    torch.manual_seed(11)
    train = pointgroup_train.PointGroup(cfg)
    torch.manual_seed(11)
    base = pointgroup.PointGroup(cfg)
    assert isinstance(train, pointgroup.PointGroup)
    a, b = train.state_dict(), base.state_dict()
    with open(os.path.join(GOLDEN, 'pointgroup_state_keys.json')) as f:
        golden = json.load(f)
    assert [[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in a.items()] == golden
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert [n for n, _ in train.named_modules()] == [n for n, _ in base.named_modules()]
    for (_, m), (_, o) in zip(train.named_modules(), base.named_modules()):
        assert isinstance(m, type(o)), (type(m), type(o))
    from catgrasp_amd import spconv, spconv_autograd
    convs = [m for m in train.modules() if isinstance(m, spconv.SparseConvolution)]
    assert len(convs) == 71 + 15 and all(isinstance(m, spconv_autograd._Differentiable) for m in convs)
    assert not any(isinstance(m, spconv_autograd._Differentiable) for m in base.modules())
    base.load_state_dict(train.state_dict(), strict=True)
    # the inference model still refuses training mode
    with pytest.raises(NotImplementedError, match='inference only'):
        base.train()(None, None, None, None, None, 0)
    with pytest.raises(NotImplementedError, match='score branch'):
        train.train()(None, None, None, None, None, cfg.prepare_epochs + 1)


def test_v2p_from_input_map_is_the_voxelizations_output_map():
    for kind in ('full', 'n33'):
        imap, _, _, v2p = T.points(kind)
        got = pointgroup_train.v2p_from_input_map(torch.from_numpy(imap), len(v2p))
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), v2p)
    got = pointgroup_train.v2p_from_input_map(torch.tensor([2, 0, 2, 2], dtype=torch.int32), 4)      # voxels 1 and 3 have no point
    assert got.tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [3, 0, 2, 3], [0, 0, 0, 0]]


def test_loss_fn_is_the_offset_loss():
    rng = np.random.default_rng(2)
    pt, coords, info = (torch.from_numpy(rng.uniform(-1, 1, s).astype(np.float32)) for s in ((50, 3), (50, 3), (50, 9)))
    cfg = types.SimpleNamespace(prepare_epochs=10, loss_weight=[1.0, 0.5, 2.0, 1.0])
    loss, loss_out, infos = pointgroup_train.loss_fn({'pt_offsets': (pt, coords, info, None)}, 3, cfg)
    want = 0.5 * float(((pt.double() - (info[:, :3].double() - coords.double())) ** 2).mean())
    assert abs(float(loss) - want) <= 1e-6 and infos == {}
    assert list(loss_out) == ['offset_norm_loss', 'offset_dir_loss'] and loss_out['offset_dir_loss'] == (0.0, 50)
    assert abs(loss_out['offset_norm_loss'][0] - 2 * want) <= 1e-6 and loss_out['offset_norm_loss'][1] == 50
    with pytest.raises(NotImplementedError):
        pointgroup_train.loss_fn({'pt_offsets': (pt, coords, info, None)}, 11, cfg)
