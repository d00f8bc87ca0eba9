"""GPU tests of the sparse 3-D convolution layers (catgrasp_amd/spconv.py, csrc/sparse_rules.hip, csrc/sparse_conv.hip).

Yardstick: tests/sparse_ref.py, the float64 dictionary-lookup restatement of the layers' rules, pinned against dense float64
torch.nn.functional.conv3d / conv_transpose3d in tests/test_sparse_ref_cpu.py.

Bounds.  Integers (rule books, output sites and their order, output shapes, dropped sites) are EQUAL.  Features are per element within
1e-4 * max(1, |ref|), the suite's standing bar; with weights uniform in +-sqrt(3/Cin) the outputs are of order one, so one lost or
misplaced neighbour is four orders above the bar, while float32 accumulation noise at Cin = 192, k = 3 is near 1e-7 * sum|a*b|.

Scenes (the smallest at which each failure shows): batch 2, spatial_shape (9, 12, 17), 299 sites holding both corners, a voxel at the
end of one row and one at the start of the next, the same position in both batch items, an isolated voxel, a full 3x3x3 block and
voxels at the odd last coordinates (dropped by the strided layer); N = 1, 33, 301 for partial 32-row tiles; one scene whose batch
item 0 is empty."""
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

import catgrasp_amd.spconv as spconv
import sparse_ref as ref
from catgrasp_amd import _lib

pytestmark = pytest.mark.gpu

BAR = 1e-4
SCENES = OrderedDict([('full299', dict(n=299)), ('n1', dict(n=1, special=False)), ('n33', dict(n=33, special=False)), ('n301', dict(n=301, seed=5)),
                      ('empty_item0', dict(n=120, special=False, only_item=1))])
_BOOKS = {}


def _books(name):
    """The restatement's rule books of a scene, computed once."""
    if name not in _BOOKS:
        idx = ref.scene(**SCENES[name])
        out_idx, down, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
        _BOOKS[name] = dict(idx=idx, subm=ref.subm_rules(idx, ref.SHAPE), out_idx=out_idx, down=down, out_shape=out_shape, dropped=dropped,
                            inv=ref.inverse_rules(idx, out_idx, ref.SHAPE))
    return _BOOKS[name]


def _tensor(idx, x, dev):
    return spconv.SparseConvTensor(torch.from_numpy(np.ascontiguousarray(x)).to(dev), torch.from_numpy(np.ascontiguousarray(idx)).to(dev), ref.SHAPE, ref.BATCH)


def _layer(cls, cin, cout, k, dev, seed=2, **kw):
    layer = cls(cin, cout, k, **kw).to(dev).eval()
    w, b = ref.weights(k, cin, cout, seed=seed)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(w)); layer.bias.copy_(torch.from_numpy(b))
    return layer, w, b


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _check(got, want, what):
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max(initial=0.0))
    print(f'{what}: rows {want.shape[0]} max |got - ref| / max(1, |ref|) = {err:.3g} (bar {BAR:g}), max |ref| = {np.abs(want).max(initial=0.0):.3g}')
    assert np.isfinite(got).all() and err <= BAR, (what, err)


def _run_three(name, cin, cout, dev, pro, res):
    """SubM k = 3, strided and inverse layer, each cin -> cout, on one scene against the restatement (the inverse layer reads fresh
    cin-channel features on the strided layer's output sites)."""
    bk = _books(name)
    idx, n, m = bk['idx'], len(bk['idx']), len(bk['out_idx'])
    x = ref.features(n, cin)
    scale, shift = ref.bn_params(cin) if pro else (None, None)
    prologue = (_dev(scale, dev), _dev(shift, dev)) if pro else None
    rng = np.random.default_rng(9)
    with torch.no_grad():
        subm, w, b = _layer(spconv.SubMConv3d, cin, cout, 3, dev, padding=1, indice_key='subm1')
        r = rng.uniform(-1, 1, (n, cout)).astype(np.float32) if res else None
        out = subm(_tensor(idx, x, dev), prologue=prologue, residual=_dev(r, dev))
        assert torch.equal(out.indices.cpu(), torch.from_numpy(idx)) and list(out.spatial_shape) == list(ref.SHAPE)
        _check(out.features, ref.conv(x, bk['subm'], w, b, scale, shift, r), f'{name} subm {cin}->{cout} pro {pro} res {res}')

        down, w, b = _layer(spconv.SparseConv3d, cin, cout, 2, dev, stride=2, indice_key='spconv1')
        r = rng.uniform(-1, 1, (m, cout)).astype(np.float32) if res else None
        t = _tensor(idx, x, dev)
        out = down(t, prologue=prologue, residual=_dev(r, dev))
        assert torch.equal(out.indices.cpu(), torch.from_numpy(bk['out_idx'])) and tuple(out.spatial_shape) == bk['out_shape']
        _check(out.features, ref.conv(x, bk['down'], w, b, scale, shift, r), f'{name} down {cin}->{cout} pro {pro} res {res}')

        inv, w, b = _layer(spconv.SparseInverseConv3d, cin, cout, 2, dev, seed=4, indice_key='spconv1')
        y = ref.features(m, cin, seed=6)
        r = rng.uniform(-1, 1, (n, cout)).astype(np.float32) if res else None
        coarse = spconv.SparseConvTensor(_dev(y, dev), out.indices, out.spatial_shape, ref.BATCH)
        coarse.indice_dict = t.indice_dict
        up = inv(coarse, prologue=prologue, residual=_dev(r, dev))
        assert torch.equal(up.indices.cpu(), torch.from_numpy(idx)) and list(up.spatial_shape) == list(ref.SHAPE)
        _check(up.features, ref.conv(y, bk['inv'], w, b, scale, shift, r), f'{name} inverse {cin}->{cout} pro {pro} res {res}')
        if not res and bk['dropped'].any():
            assert torch.equal(up.features[torch.from_numpy(bk['dropped']).to(dev)].cpu(), torch.from_numpy(b).expand(int(bk['dropped'].sum()), cout))


@pytest.mark.parametrize('name', list(SCENES))
def test_rule_books_output_sites_and_shapes_are_equal(name, cuda_device):
    bk = _books(name)
    idx = torch.from_numpy(bk['idx']).to(cuda_device)
    subm = spconv.subm_rules(idx, list(ref.SHAPE), ref.BATCH)
    assert subm.nbr.dtype == torch.int32 and np.array_equal(subm.nbr.cpu().numpy(), bk['subm'])
    down = spconv.down_rules(idx, list(ref.SHAPE), ref.BATCH)
    assert tuple(down.out_spatial_shape) == bk['out_shape'] == (4, 6, 8)
    assert down.out_indices.dtype == torch.int32 and np.array_equal(down.out_indices.cpu().numpy(), bk['out_idx'])
    assert np.array_equal(down.nbr.cpu().numpy(), bk['down'])
    inv = spconv.inverse_rules(down)
    assert np.array_equal(inv.cpu().numpy(), bk['inv'])
    dropped = (inv < 0).all(1).cpu().numpy()
    assert np.array_equal(dropped, bk['dropped'])
    print(f'{name}: {len(bk["idx"])} sites, {len(bk["out_idx"])} strided outputs, {int(dropped.sum())} dropped, '
          f'{(bk["subm"] >= 0).mean() * 27:.2f} of 27 neighbours present per site')
    if name == 'full299':
        assert dropped.sum() >= 6            # the case is populated


@pytest.mark.parametrize('cout', [3, 16, 48, 112])
@pytest.mark.parametrize('cin', [6, 16, 32, 112, 192])
def test_features_over_the_channel_grid(cin, cout, cuda_device):
    _run_three('full299', cin, cout, cuda_device, pro=False, res=False)
    _run_three('full299', cin, cout, cuda_device, pro=True, res=True)


@pytest.mark.parametrize('pro,res', [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize('name', ['n1', 'n33', 'n301', 'empty_item0'])
def test_partial_tiles_and_every_prologue_residual_combination(name, pro, res, cuda_device):
    _run_three(name, 32, 48, cuda_device, pro, res)
    _run_three(name, 6, 3, cuda_device, pro, res)


def test_subm_k1_is_a_matrix_product(cuda_device):
    bk = _books('n301')
    for cin, cout in ((32, 16), (192, 112), (6, 3)):
        x = ref.features(len(bk['idx']), cin)
        layer, w, b = _layer(spconv.SubMConv3d, cin, cout, 1, cuda_device)
        scale, shift = ref.bn_params(cin)
        with torch.no_grad():
            t = _tensor(bk['idx'], x, cuda_device)
            out = layer(t)
            assert t.indice_dict == {} and out.indices is t.indices
            _check(out.features, x.astype(np.float64) @ w.reshape(cin, cout).astype(np.float64) + b, f'k=1 {cin}->{cout}')
            out = layer(t, prologue=(_dev(scale, cuda_device), _dev(shift, cuda_device)))
            _check(out.features, ref.conv(x, np.arange(len(x))[:, None], w, b, scale, shift), f'k=1 {cin}->{cout} prologue')


def test_a_shared_indice_key_reuses_the_rule_book(cuda_device):
    bk = _books('full299')
    x = ref.features(299, 16)
    a, _, _ = _layer(spconv.SubMConv3d, 16, 32, 3, cuda_device, padding=1, indice_key='subm1')
    b, _, _ = _layer(spconv.SubMConv3d, 32, 16, 3, cuda_device, padding=1, indice_key='subm1')
    c, _, _ = _layer(spconv.SubMConv3d, 16, 16, 3, cuda_device, padding=1)                    # no key: builds its own, stores nothing
    d, _, _ = _layer(spconv.SparseConv3d, 16, 32, 2, cuda_device, stride=2, indice_key='spconv1')
    e, _, _ = _layer(spconv.SparseInverseConv3d, 32, 16, 2, cuda_device, indice_key='spconv1')
    with torch.no_grad():
        t = _tensor(bk['idx'], x, cuda_device)
        y = a(t)
        book = t.find_indice_pair('subm1')
        assert book is not None and y.indice_dict is t.indice_dict
        z = b(y)
        assert z.find_indice_pair('subm1') is book and z.find_indice_pair('subm1').nbr is book.nbr and list(t.indice_dict) == ['subm1']
        c(z)
        assert list(t.indice_dict) == ['subm1']
        lo = d(z)
        down = t.find_indice_pair('spconv1')
        assert down is not None and lo.indices is down.out_indices and 'inverse_nbr' not in down.extra
        up = e(lo)
        inv = down.extra['inverse_nbr']
        e(lo)
        assert t.find_indice_pair('spconv1') is down and down.extra['inverse_nbr'] is inv and up.indices is down.in_indices
        with pytest.raises(ValueError):
            e(_tensor(bk['idx'], ref.features(299, 32), cuda_device))           # no strided layer has run on this tensor
        with pytest.raises(ValueError):
            spconv.SparseInverseConv3d(32, 16, 2, indice_key='subm1').to(cuda_device)(lo)      # the key of another kind of layer


def _bn(c, dev, seed):
    rng = np.random.default_rng(seed)
    bn = nn.BatchNorm1d(c, eps=1e-4, momentum=0.1).to(dev).eval()
    with torch.no_grad():
        bn.weight.copy_(_dev(rng.uniform(0.5, 1.5, c) * rng.choice([-1, 1], c), dev)); bn.bias.copy_(_dev(rng.uniform(-0.5, 0.5, c), dev))
        bn.running_mean.copy_(_dev(rng.uniform(-0.3, 0.3, c), dev)); bn.running_var.copy_(_dev(rng.uniform(0.5, 2.0, c), dev))
    return bn


def _bn64(bn):
    g, b, m, v = (t.detach().cpu().numpy().astype(np.float64) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    scale = g / np.sqrt(v + bn.eps)
    return scale, b - m * scale


class _UBlock(nn.Module):
    """Wired exactly as the reference's UBlock.forward with one VGG-style block per stage."""

    def __init__(self, planes, dev, level=1):
        super().__init__()
        p = planes[0]
        self.planes = planes
        self.blocks = spconv.SparseSequential(OrderedDict([('block0', spconv.SparseSequential(
            _bn(p, dev, 10 * level), nn.ReLU(), _layer(spconv.SubMConv3d, p, p, 3, dev, seed=20 + level, padding=1, indice_key=f'subm{level}')[0]))]))
        if len(planes) > 1:
            self.conv = spconv.SparseSequential(_bn(p, dev, 10 * level + 1), nn.ReLU(),
                                                _layer(spconv.SparseConv3d, p, planes[1], 2, dev, seed=30 + level, stride=2, indice_key=f'spconv{level}')[0])
            self.u = _UBlock(planes[1:], dev, level + 1)
            self.deconv = spconv.SparseSequential(_bn(planes[1], dev, 10 * level + 2), nn.ReLU(),
                                                  _layer(spconv.SparseInverseConv3d, planes[1], p, 2, dev, seed=40 + level, indice_key=f'spconv{level}')[0])
            self.blocks_tail = spconv.SparseSequential(OrderedDict([('block0', spconv.SparseSequential(
                _bn(2 * p, dev, 10 * level + 3), nn.ReLU(), _layer(spconv.SubMConv3d, 2 * p, p, 3, dev, seed=50 + level, padding=1, indice_key=f'subm{level}')[0]))]))

    def forward(self, input):
        output = self.blocks(input)
        identity = spconv.SparseConvTensor(output.features, output.indices, output.spatial_shape, output.batch_size)
        if len(self.planes) > 1:
            output_decoder = self.conv(output)
            output_decoder = self.u(output_decoder)
            output_decoder = self.deconv(output_decoder)
            output.features = torch.cat((identity.features, output_decoder.features), dim=1)
            output = self.blocks_tail(output)
        return output

    def restated(self, idx, shape, x):
        def seq(s, x, nbr):
            bn, _, conv = s
            return ref.conv(x, nbr, conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), *_bn64(bn))
        subm = ref.subm_rules(idx, shape)
        out = seq(self.blocks[0], x, subm)
        if len(self.planes) > 1:
            out_idx, down, out_shape, _ = ref.down_rules(idx, shape)
            dec = self.u.restated(out_idx, out_shape, seq(self.conv, out, down))
            dec = seq(self.deconv, dec, ref.inverse_rules(idx, out_idx, shape))
            out = seq(self.blocks_tail[0], np.concatenate([out, dec], axis=1), subm)
        return out


def test_two_level_unet_composition(cuda_device):
    bk = _books('full299')
    x = ref.features(299, 16)
    net = _UBlock([16, 32, 48], cuda_device).eval()
    with torch.no_grad():
        t = _tensor(bk['idx'], x, cuda_device)
        out = net(t)
    assert sorted(t.indice_dict) == ['spconv1', 'spconv2', 'subm1', 'subm2', 'subm3']
    assert torch.equal(out.indices.cpu(), torch.from_numpy(bk['idx']))
    _check(out.features, net.restated(bk['idx'], ref.SHAPE, x.astype(np.float64)), 'UBlock [16, 32, 48]')


def _three_layers(cin, cout, dev):
    return (_layer(spconv.SubMConv3d, cin, cout, 3, dev, padding=1, indice_key='subm1')[0],
            _layer(spconv.SparseConv3d, cin, cout, 2, dev, stride=2, indice_key='spconv1')[0],
            _layer(spconv.SparseInverseConv3d, cout, cin, 2, dev, seed=4, indice_key='spconv1')[0])


def _forward_three(layers, idx, x, dev, prologue=None):
    subm, down, inv = layers
    with torch.no_grad():
        t = _tensor(idx, x, dev)
        a = subm(t, prologue=prologue)
        b = down(t, prologue=prologue)
        c = inv(b)
    return a, b, c


def test_run_to_run_and_row_permutation_are_bit_identical(cuda_device):
    bk = _books('full299')
    idx, x = bk['idx'], ref.features(299, 32)
    layers = _three_layers(32, 48, cuda_device)
    scale, shift = ref.bn_params(32)
    pro = (_dev(scale, cuda_device), _dev(shift, cuda_device))
    a, b, c = _forward_three(layers, idx, x, cuda_device, pro)
    a2, b2, c2 = _forward_three(layers, idx, x, cuda_device, pro)
    assert torch.equal(a.features, a2.features) and torch.equal(b.features, b2.features) and torch.equal(c.features, c2.features)
    assert torch.equal(b.indices, b2.indices)
    perm = np.random.default_rng(11).permutation(299)
    ap, bp, cp = _forward_three(layers, idx[perm], x[perm], cuda_device, pro)
    p = torch.from_numpy(perm).to(cuda_device)
    assert torch.equal(ap.features, a.features[p]) and torch.equal(cp.features, c.features[p])          # the same bits per site
    assert torch.equal(bp.indices, b.indices) and torch.equal(bp.features, b.features)                  # key order: no undoing needed


def test_a_batch_item_does_not_see_the_other(cuda_device):
    bk = _books('full299')
    idx, x = bk['idx'], ref.features(299, 32)
    keep = idx[:, 0] == 0
    other = ref.scene(n=150, seed=21, special=False, only_item=1)
    idx2 = np.concatenate([idx[keep], other])
    x2 = np.concatenate([x[keep], ref.features(150, 32, seed=22)])
    layers = _three_layers(32, 48, cuda_device)
    a, b, c = _forward_three(layers, idx, x, cuda_device)
    a2, b2, c2 = _forward_three(layers, idx2, x2, cuda_device)
    k = torch.from_numpy(keep).to(cuda_device)
    n0 = int(keep.sum())
    assert 0 < n0 < 299
    assert torch.equal(a.features[k], a2.features[:n0]) and torch.equal(c.features[k], c2.features[:n0])
    m0 = int((b.indices[:, 0] == 0).sum())
    assert m0 > 0 and torch.equal(b.indices[:m0], b2.indices[:m0]) and torch.equal(b.features[:m0], b2.features[:m0])
    assert int((b2.indices[:, 0] == 0).sum()) == m0


def test_folded_bn_relu_conv_equals_the_direct_prologue_and_the_three_steps(cuda_device):
    bk = _books('n301')
    idx, x = bk['idx'], ref.features(301, 32)
    for make, nbr_name in ((lambda: _layer(spconv.SubMConv3d, 32, 48, 3, cuda_device, padding=1)[0], 'subm'),
                           (lambda: _layer(spconv.SparseConv3d, 32, 48, 2, cuda_device, stride=2)[0], 'down')):
        conv, bn = make(), _bn(32, cuda_device, 77)
        seq = spconv.SparseSequential(bn, nn.ReLU(), conv).eval()
        with torch.no_grad():
            t = _tensor(idx, x, cuda_device)
            folded = seq(t)
            assert torch.equal(t.features.cpu(), torch.from_numpy(x))                      # folded: the input's features are not rewritten
            direct = conv(_tensor(idx, x, cuda_device), prologue=spconv.bn_relu_prologue(bn))
            assert torch.equal(folded.features, direct.features)
            s = _tensor(idx, x, cuda_device)
            s.features = torch.relu(bn(s.features))
            stepwise = conv(s)
            seq.train()                                                                     # not folded outside eval mode; the BN itself stays in eval
            bn.eval()
            unfolded = seq(_tensor(idx, x, cuda_device))
            seq.eval()
        assert torch.equal(unfolded.features, stepwise.features)
        want = ref.conv(x, bk[nbr_name], conv.weight.detach().cpu().numpy(), conv.bias.detach().cpu().numpy(), *_bn64(bn))
        _check(folded.features, want, f'folded BN, ReLU, {nbr_name}')
        _check(stepwise.features, want, f'BN, ReLU, {nbr_name} as three steps')


def test_dense_places_every_row(cuda_device):
    bk = _books('full299')
    x = ref.features(299, 6)
    t = _tensor(bk['idx'], x, cuda_device)
    assert np.array_equal(t.dense().cpu().numpy(), ref.dense(bk['idx'], x, ref.BATCH, ref.SHAPE).astype(np.float32))


def test_refusals(cuda_device):
    dev = cuda_device
    idx = ref.scene(n=33, special=False).copy()
    x = ref.features(33, 16)
    subm, _, _ = _layer(spconv.SubMConv3d, 16, 16, 3, dev, padding=1)
    down, _, _ = _layer(spconv.SparseConv3d, 16, 32, 2, dev, stride=2)
    for row, col, val in ((5, 1, 9), (5, 2, 12), (5, 3, 17), (32, 3, -1), (0, 0, 2), (0, 0, -1)):          # coordinate and batch index out of range
        bad = idx.copy(); bad[row, col] = val
        for layer in (subm, down):
            with torch.no_grad(), pytest.raises(ValueError, match='outside'):
                layer(_tensor(bad, x, dev))
    dup = idx.copy(); dup[20] = dup[3]
    for layer in (subm, down):
        with torch.no_grad(), pytest.raises(ValueError, match='twice'):
            layer(_tensor(dup, x, dev))
    with pytest.raises(ValueError):
        _tensor(idx, x[:32], dev)                                                # mismatched rows at construction
    t = _tensor(idx, x, dev)
    t.features = t.features[:32]
    with torch.no_grad(), pytest.raises(ValueError):
        subm(t)                                                                  # and after it
    with torch.no_grad(), pytest.raises(ValueError):
        subm(_tensor(idx, ref.features(33, 32), dev))                            # channels the layer does not take
    for cin, cout in ((8, 16), (240, 16), (16, 5), (16, 128)):
        with pytest.raises(ValueError):
            spconv.SubMConv3d(cin, cout, 3, padding=1)
    nbr = torch.zeros((33, 27), dtype=torch.int32, device=dev)
    with pytest.raises(_lib.CatgraspAmdError, match='-2'):
        spconv.sparse_conv(torch.zeros((33, 24), device=dev), nbr, torch.zeros((27, 24, 16), device=dev))      # the C entry point refuses too
    for make in (lambda: spconv.SubMConv3d(16, 16, 5, padding=2), lambda: spconv.SparseConv3d(16, 32, 3, stride=2, padding=1),
                 lambda: spconv.SparseConv3d(16, 32, 2, stride=1), lambda: spconv.SparseInverseConv3d(32, 16, 3, indice_key='k')):
        with pytest.raises(NotImplementedError):
            make()
    with pytest.raises(NotImplementedError):
        subm(_tensor(idx, x, dev))                                               # gradients enabled and the weights require them
    with torch.no_grad(), pytest.raises(_lib.CatgraspAmdError):
        subm(spconv.SparseConvTensor(torch.from_numpy(x), torch.from_numpy(idx), ref.SHAPE, ref.BATCH))      # host tensors
    with torch.no_grad():
        out = subm(_tensor(idx, x, dev))                                         # and the layer still runs after all of that
    assert out.features.shape == (33, 16)
