"""GPU tests of the rule-book builders (csrc/sparse_rules.hip, spconv.subm_rules / down_rules / inverse_rules) on the grids at the edges
of what they take: linear keys across 2^31 and 2^32, axes of 1, 2 and 3, a fully dense block, a strided layer that drops every site,
and one that drops most of them (rules_down_kernel's duplicate check then runs in threads beyond the table's).

Yardstick: sparse_ref.subm_rules / down_rules / inverse_rules, dictionary lookups on coordinate tuples that never form a key, so they
do not depend on the grid's size.  tests/test_sparse_ref_cpu.py asserts that each scene holds what it is here for.

Bound: integers (tables, output sites and their order, shapes, dropped masks) are EQUAL; the features of the layers that run on these
scenes have the bits of sparse_ref.conv_exact."""
import numpy as np
import pytest
import torch

import catgrasp_amd.spconv as spconv
import sparse_ref as ref

pytestmark = pytest.mark.gpu


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_books(name, dev):
    """Every rule book of one edge scene against the restatement.  -> (reference dict, the device's strided book or None)"""
    idx, shape, batch = ref.edge_scene(name)
    d_idx = _dev(idx, dev)
    want = ref.subm_rules(idx, shape)
    subm = spconv.subm_rules(d_idx, list(shape), batch)
    assert subm.nbr.dtype == torch.int32 and tuple(subm.nbr.shape) == (len(idx), 27) and np.array_equal(subm.nbr.cpu().numpy(), want)
    assert subm.out_indices is subm.in_indices and list(subm.out_spatial_shape) == list(shape)
    bk = dict(idx=idx, shape=shape, batch=batch, subm=want)
    print(f'{name}: {len(idx)} sites in {batch} x {shape}, {(want >= 0).mean() * 27:.2f} of 27 neighbours per site, subm table equal')
    if min(shape) < 2:
        with pytest.raises(ValueError, match='smaller than the kernel'):
            spconv.down_rules(d_idx, list(shape), batch)
        return bk, None
    out_idx, down_want, out_shape, dropped = ref.down_rules(idx, shape)
    down = spconv.down_rules(d_idx, list(shape), batch)
    assert tuple(down.out_spatial_shape) == out_shape
    assert down.out_indices.dtype == torch.int32 and tuple(down.out_indices.shape) == (len(out_idx), 4)
    assert down.nbr.dtype == torch.int32 and tuple(down.nbr.shape) == (len(out_idx), 8)
    assert down.extra['out_keys'].dtype == torch.int64 and tuple(down.extra['out_keys'].shape) == (len(out_idx),)
    assert np.array_equal(down.out_indices.cpu().numpy(), out_idx) and np.array_equal(down.nbr.cpu().numpy(), down_want)
    assert np.array_equal(down.extra['out_keys'].cpu().numpy(), ref.linear_key(out_idx, out_shape))
    inv_want = ref.inverse_rules(idx, out_idx, shape)
    inv = spconv.inverse_rules(down)
    assert inv.dtype == torch.int32 and tuple(inv.shape) == (len(idx), 8) and np.array_equal(inv.cpu().numpy(), inv_want)
    assert np.array_equal((inv < 0).all(1).cpu().numpy(), dropped)
    bk.update(out_idx=out_idx, down=down_want, out_shape=out_shape, dropped=dropped, inv=inv_want)
    print(f'{name}: {len(out_idx)} strided outputs in {out_shape}, {int(dropped.sum())} sites dropped, strided and inverse tables equal')
    return bk, down


@pytest.mark.parametrize('name', ref.EDGE_SCENES)
def test_rule_books_on_the_edge_grids_are_equal(name, cuda_device):
    bk, _ = _check_books(name, cuda_device)
    if name == 'dense':
        assert (bk['subm'] >= 0).all(1).sum() == 48              # the interior sites: 27 of 27 neighbours
    if name == 'large':
        keys, okeys = ref.linear_key(bk['idx'], bk['shape']), ref.linear_key(bk['out_idx'], bk['out_shape'])
        assert keys.max() > 2 ** 32 and (keys < 2 ** 31).any() and okeys.max() > 2 ** 31 and (okeys < 2 ** 31).any()
    if name == 'all_dropped':
        assert bk['out_idx'].shape == (0, 4) and bk['dropped'].all()
    if name.startswith('mostly_dropped'):
        assert len(bk['out_idx']) * 8 < len(bk['idx'])


def _bits_equal(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    assert same.all(), f'{what}: {int((~same).sum())} of {same.size} elements differ in their bits'
    print(f'{what}: rows {want.shape[0]}, channels {want.shape[1]}, {want.size} elements, bits equal')


def _layer(cls, cin, cout, k, dev, seed, **kw):
    layer = cls(cin, cout, k, **kw).to(dev).eval()
    w, b = ref.weights(k, cin, cout, seed=seed)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(w)); layer.bias.copy_(torch.from_numpy(b))
    return layer, w, b


@pytest.mark.parametrize('name', ['large', 'two', 'three_two_five', 'dense', 'all_dropped', 'mostly_dropped'])
def test_the_three_layers_on_the_edge_grids_have_the_bits_of_the_model(name, cuda_device):
    """One 16 -> 16 SubM, strided and inverse layer, with prologue and residual.  all_dropped: the strided layer returns (0, 16) and
    the inverse layer, whose input has no rows, the bias (+ residual) in every row."""
    dev = cuda_device
    idx, shape, batch = ref.edge_scene(name)
    out_idx, down_nbr, out_shape, dropped = ref.down_rules(idx, shape)
    n, m, c = len(idx), len(out_idx), 16
    x, y = ref.features(n, c), ref.features(m, c, seed=6)
    scale, shift = ref.bn_params(c)
    prologue = (_dev(scale, dev), _dev(shift, dev))
    rng = np.random.default_rng(9)
    with torch.no_grad():
        subm, w, b = _layer(spconv.SubMConv3d, c, c, 3, dev, 2, padding=1, indice_key='subm1')
        r = rng.uniform(-1, 1, (n, c)).astype(np.float32)
        fine = spconv.SparseConvTensor(_dev(x, dev), _dev(idx, dev), shape, batch)
        out = subm(fine, prologue=prologue, residual=_dev(r, dev))
        assert torch.equal(out.indices.cpu(), torch.from_numpy(idx)) and list(out.spatial_shape) == list(shape)
        _bits_equal(out.features, ref.conv_exact(x, ref.subm_rules(idx, shape), w, b, scale, shift, r), f'{name} subm')

        down, w, b = _layer(spconv.SparseConv3d, c, c, 2, dev, 3, stride=2, indice_key='spconv1')
        r = rng.uniform(-1, 1, (m, c)).astype(np.float32)
        out = down(fine, prologue=prologue, residual=_dev(r, dev))
        assert out.features.dtype == torch.float32 and tuple(out.features.shape) == (m, c) and out.features.is_cuda
        assert torch.equal(out.indices.cpu(), torch.from_numpy(out_idx)) and tuple(out.spatial_shape) == out_shape
        _bits_equal(out.features, ref.conv_exact(x, down_nbr, w, b, scale, shift, r), f'{name} strided')

        inv, w, b = _layer(spconv.SparseInverseConv3d, c, c, 2, dev, 4, indice_key='spconv1')
        coarse = spconv.SparseConvTensor(_dev(y, dev), out.indices, out.spatial_shape, batch)
        coarse.indice_dict = fine.indice_dict
        r = rng.uniform(-1, 1, (n, c)).astype(np.float32)
        up = inv(coarse, prologue=prologue, residual=_dev(r, dev))
        assert torch.equal(up.indices.cpu(), torch.from_numpy(idx)) and list(up.spatial_shape) == list(shape)
        _bits_equal(up.features, ref.conv_exact(y, ref.inverse_rules(idx, out_idx, shape), w, b, scale, shift, r), f'{name} inverse')
        plain = inv(coarse).features.cpu()
        if dropped.any():
            assert torch.equal(plain[torch.from_numpy(dropped)], torch.from_numpy(b).expand(int(dropped.sum()), c))          # the bias only
        if name == 'all_dropped':
            assert m == 0 and torch.equal(plain, torch.from_numpy(b).expand(n, c))


def test_an_axis_of_one_takes_the_submanifold_layers_and_refuses_the_strided_one(cuda_device):
    dev = cuda_device
    idx, shape, batch = ref.edge_scene('unit')
    x = ref.features(len(idx), 16)
    with torch.no_grad():
        subm, w, b = _layer(spconv.SubMConv3d, 16, 16, 3, dev, 2, padding=1)
        out = subm(spconv.SparseConvTensor(_dev(x, dev), _dev(idx, dev), shape, batch))
        _bits_equal(out.features, ref.conv_exact(x, ref.subm_rules(idx, shape), w, b), 'unit subm')
        want = (x.astype(np.float64) @ w[1, 1, 1].astype(np.float64) + b).astype(np.float32)          # only the centre offset
        assert np.abs(out.features.cpu().numpy() - want).max() <= 1e-5
        down, _, _ = _layer(spconv.SparseConv3d, 16, 16, 2, dev, 3, stride=2)
        with pytest.raises(ValueError, match='smaller than the kernel'):
            down(spconv.SparseConvTensor(_dev(x, dev), _dev(idx, dev), shape, batch))


@pytest.mark.parametrize('name', ['mostly_dropped', 'mostly_dropped_x20'])
def test_a_duplicate_among_the_dropped_sites_is_still_refused(name, cuda_device):
    """The pair sits at a sorted position >= n_out*8 (x20: in a workgroup beyond the table's), where no thread builds a table entry."""
    _, shape, batch = ref.edge_scene(name)
    dup, pos = ref.with_dropped_duplicate(name)
    assert pos >= 8 * batch
    d = _dev(dup, cuda_device)
    with pytest.raises(ValueError, match='twice'):
        spconv.subm_rules(d, list(shape), batch)
    with pytest.raises(ValueError, match='twice'):
        spconv.down_rules(d, list(shape), batch)
    _check_books(name, cuda_device)                                              # and the builders still run after it
