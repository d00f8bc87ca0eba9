"""GPU tests of the assembled PointGroup network (catgrasp_amd/pointgroup.py) at the shipped configuration, under the seeded test
weights of tests/pointgroup_ref.py: per element against the float64 yardstick, bit for bit against the same modules wired the plain way,
the launch and rule-book counts of one forward, and independence of row order and of the other batch item.

The bar is the suite's 1e-4 * max(1, |ref|).  tests/test_pointgroup_ref_cpu.py holds the float32 noise of these weights through the 73
dependent layers to a quarter of it (measured there: 5.4e-6)."""
import os

import numpy as np
import pytest
import torch

import catgrasp_amd.spconv as spconv
import pointgroup_ref as P
from catgrasp_amd import _lib, pointgroup

pytestmark = pytest.mark.gpu

BAR = 1e-4
_MODEL = {}


def _model(dev):
    if 'm' not in _MODEL:
        cfg = pointgroup.config_from_yaml(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'config_pointgroup.yaml'))
        model = pointgroup.PointGroup(cfg)
        sd = model.state_dict()
        sd.update({k: torch.from_numpy(v) for k, v in P.params().items()})
        model.load_state_dict(sd)
        _MODEL['m'] = model.to(dev).eval()
    return _MODEL['m']


def _tensor(idx, x, dev):
    return spconv.SparseConvTensor(torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.ascontiguousarray(idx)).to(dev), P.SHAPE, P.BATCH)


def _scene_tensor(kind, dev):
    idx = P.scene(kind)
    return _tensor(idx, P.features(len(idx)), dev)


def _err(got, want):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max(initial=0.0))


@pytest.mark.parametrize('kind', P.SCENES)
def test_offsets_and_unet_features_against_the_float64_yardstick(kind, cuda_device):
    model = _model(cuda_device)
    want_feats, want_offsets, imap = P.reference(kind)
    d_map = torch.from_numpy(imap).to(cuda_device)
    feats = model.unet_features(_scene_tensor(kind, cuda_device))
    assert torch.equal(feats.indices.cpu(), torch.from_numpy(P.scene(kind))) and list(feats.spatial_shape) == list(P.SHAPE)
    ret = model(_scene_tensor(kind, cuda_device), d_map, None, None, None, epoch=model.prepare_epochs - 1)
    assert list(ret) == ['pt_offsets'] and ret['pt_offsets'].shape == (len(imap), 3) and ret['pt_offsets'].dtype == torch.float32
    ef, eo = _err(feats.features, want_feats), _err(ret['pt_offsets'], want_offsets)
    print(f'{kind}: {len(want_feats)} voxels, max |got - ref| / max(1, |ref|): features {ef:.3g}, pt_offsets {eo:.3g} (bar {BAR:g}); '
          f'max |ref| {np.abs(want_feats).max():.3g} / {np.abs(want_offsets).max():.3g}')
    assert ef <= BAR and eo <= BAR


# The same modules wired the plain way: SparseSequential (which folds BatchNorm + ReLU into the next layer's prologue), torch.cat, +=.
def _plain_block(block, input):
    identity = spconv.SparseConvTensor(input.features, input.indices, input.spatial_shape, input.batch_size)
    output = block.conv_branch(input)
    output.features += block.i_branch(identity).features
    return output


def _plain_ublock(u, input):
    output = input
    for block in u.blocks:
        output = _plain_block(block, output)
    if len(u.nPlanes) > 1:
        decoder = u.deconv(_plain_ublock(u.u, u.conv(output)))
        output.features = torch.cat((output.features, decoder.features), dim=1)
        for block in u.blocks_tail:
            output = _plain_block(block, output)
    return output


@pytest.mark.parametrize('two_source', [False, True])
@pytest.mark.parametrize('kind', ['full', 'n1'])
def test_fused_forward_has_the_bits_of_the_plain_wiring(kind, two_source, cuda_device, monkeypatch):
    """With either form of the six skips: torch.cat + cg_sparse_conv, and cg_sparse_conv_cat."""
    monkeypatch.setattr(pointgroup, 'USE_TWO_SOURCE_KERNEL', two_source)
    model = _model(cuda_device)
    calls = []
    lib = _lib.lib()
    real = lib.cg_sparse_conv_cat
    monkeypatch.setattr(lib, 'cg_sparse_conv_cat', lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        plain = _plain_ublock(model.unet, model.input_conv(_scene_tensor(kind, cuda_device)))
        assert not calls
        fused = model.unet_features(_scene_tensor(kind, cuda_device))
        assert len(calls) == (12 if two_source else 0)
        assert plain.features.shape == (len(P.scene(kind)), 16) and torch.equal(fused.features, plain.features)
        imap = torch.from_numpy(P.reference(kind)[2]).to(cuda_device)
        want = model.offset(model.output_layer(plain).features[imap.long()])
        got = model(_scene_tensor(kind, cuda_device), imap, None, None, None, epoch=0)['pt_offsets']
        assert float((got - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))      # torch's Linear sums in another order


def test_launch_and_rule_book_counts_of_one_forward(cuda_device, monkeypatch):
    model = _model(cuda_device)
    lib = _lib.lib()
    counts = {}

    def counted(name):
        fn = getattr(lib, name)

        def call(*args):
            counts[name] = counts.get(name, 0) + 1
            return fn(*args)
        monkeypatch.setattr(lib, name, call)
    for name in ('cg_sparse_conv', 'cg_sparse_conv_cat', 'cg_sparse_rules_subm', 'cg_sparse_rules_down', 'cg_sparse_rules_inverse'):
        counted(name)
    cat = torch.cat
    monkeypatch.setattr(torch, 'cat', lambda *a, **k: (counts.__setitem__('torch.cat', counts.get('torch.cat', 0) + 1), cat(*a, **k))[1])
    x = _scene_tensor('full', cuda_device)
    feats = model.unet_features(x)
    two = 12 if pointgroup.USE_TWO_SOURCE_KERNEL else 0           # the k = 3 convolution and the i_branch of six skips
    assert counts.get('cg_sparse_conv', 0) + counts.get('cg_sparse_conv_cat', 0) == 71 and counts.get('cg_sparse_conv_cat', 0) == two
    assert counts.get('torch.cat', 0) == (0 if pointgroup.USE_TWO_SOURCE_KERNEL else 6)
    assert (counts['cg_sparse_rules_subm'], counts['cg_sparse_rules_down'], counts['cg_sparse_rules_inverse']) == (7, 6, 6)
    assert sorted(x.indice_dict) == sorted([f'subm{i}' for i in range(1, 8)] + [f'spconv{i}' for i in range(1, 7)])
    before = dict(counts)
    model.head(feats.features)
    assert counts['cg_sparse_conv'] - before['cg_sparse_conv'] == 2 and counts.get('cg_sparse_conv_cat', 0) == two
    counts.clear()
    model(_scene_tensor('full', cuda_device), torch.zeros(5, dtype=torch.int32, device=cuda_device), None, None, None, epoch=0)
    assert counts.get('cg_sparse_conv', 0) + counts.get('cg_sparse_conv_cat', 0) == 73
    assert counts['cg_sparse_rules_subm'] + counts['cg_sparse_rules_down'] + counts['cg_sparse_rules_inverse'] == 19


def test_result_does_not_depend_on_the_row_order(cuda_device):
    model = _model(cuda_device)
    idx = P.scene('full')
    x, imap = P.features(len(idx)), P.reference('full')[2]
    perm = np.random.default_rng(31).permutation(len(idx))
    where = np.argsort(perm)                                      # row of every original voxel after the permutation
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda_device)
    a = model.unet_features(_tensor(idx, x, cuda_device)).features
    b = model.unet_features(_tensor(idx[perm], x[perm], cuda_device)).features
    assert torch.equal(b, a[d(perm)])
    pa = model(_tensor(idx, x, cuda_device), d(imap), None, None, None, epoch=0)['pt_offsets']
    pb = model(_tensor(idx[perm], x[perm], cuda_device), d(where[imap].astype(np.int32)), None, None, None, epoch=0)['pt_offsets']
    assert torch.equal(pa, pb)


def test_a_batch_item_does_not_see_the_other(cuda_device):
    model = _model(cuda_device)
    idx = P.scene('full')
    x = P.features(len(idx))
    own = idx[:, 0] == 0
    other = P.scene('item0_empty')                                # another item 1
    idx2 = np.concatenate([idx[own], other])
    x2 = np.concatenate([x[own], P.features(len(other), seed=32)])
    a = model.unet_features(_tensor(idx, x, cuda_device)).features
    b = model.unet_features(_tensor(idx2, x2, cuda_device)).features
    assert own.sum() > 200 and torch.equal(a[torch.from_numpy(own).to(cuda_device)], b[:int(own.sum())])
    alone = model.unet_features(_tensor(idx[own], x[own], cuda_device)).features          # ... or its absence
    assert torch.equal(alone, b[:int(own.sum())])


def test_a_site_outside_the_spatial_shape_raises(cuda_device):
    model = _model(cuda_device)
    for bad in ([0, 150, 5, 5], [0, 5, 5, 131], [2, 5, 5, 5], [0, -1, 5, 5]):
        idx = np.concatenate([P.scene('n33'), np.array([bad], dtype=np.int32)])
        with pytest.raises(ValueError, match='outside'):
            model.unet_features(_tensor(idx, P.features(len(idx)), cuda_device))
    idx = np.concatenate([P.scene('n33'), P.scene('n33')[:1]])
    with pytest.raises(ValueError, match='twice'):
        model.unet_features(_tensor(idx, P.features(len(idx)), cuda_device))
