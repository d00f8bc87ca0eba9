"""GPU tests of the sparse convolution kernel (csrc/sparse_conv.hip) bit for bit: spconv.sparse_conv and the three layer classes against
sparse_ref.conv_exact, the float32 restatement of the kernel's chain (prologue with two roundings, k ascending, channels in the order
of the MFMA steps, (acc + bias) + residual), proved on the CPU in tests/test_sparse_ref_cpu.py.

Bound: none.  The uint32 views of the output and of the model are EQUAL, element by element.  The 1e-4 tests of
tests/test_sparse_conv_gpu.py cannot see a wrong channel order inside the MFMA step, a contracted prologue, a changed epilogue
association or the cin = 6 path meeting a clamped weight where the tile's zero padding should be; each of them changes between a
quarter and a half of the bits here (test_conv_exact_sees_each_planted_variant).

Inputs stay in the normal float32 range, plus the exact zeros that the ReLU of the prologue cuts.  No subnormals.

Shapes, the smallest at which each path can go wrong: 96 sites of sparse_ref.scene with its special sites (three 32-row tiles), every
cin in {6, 16, 32, 112, 192, 224} against every cout in {3, 16, 48, 112} (224 and 112 are CG_SPARSE_MAX_CIN and CG_SPARSE_MAX_COUT),
K = 27, 8, 8 and 1; rows 1, 31, 32, 33, 65 for the partial tiles with all eight prologue / residual / bias combinations."""
import itertools

import numpy as np
import pytest
import torch

import catgrasp_amd.spconv as spconv
import sparse_ref as ref

pytestmark = pytest.mark.gpu

_TABLES = {}


def _tables(n):
    """{kind: (nbr, rows read, rows written)} of the n-site scene and its sites, from the restatement, computed once."""
    if n not in _TABLES:
        idx = ref.scene(n=n, special=n >= 96)
        out_idx, down, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
        m = len(out_idx)
        _TABLES[n] = dict(idx=idx, out_idx=out_idx, out_shape=out_shape, dropped=dropped, subm=(ref.subm_rules(idx, ref.SHAPE), n, n), down=(down, n, m),
                          inverse=(ref.inverse_rules(idx, out_idx, ref.SHAPE), m, n), k1=(np.arange(n, dtype=np.int32).reshape(n, 1), n, n))
    return _TABLES[n]


KINDS = ('subm', 'down', 'inverse', 'k1')


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits_equal(got, want, what):
    """-> number of elements compared"""
    got = got.detach().cpu().numpy()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        i = np.unravel_index(np.argmin(same), same.shape)
        raise AssertionError(f'{what}: {int((~same).sum())} of {same.size} elements differ in their bits; first at {i}: got {got[i]!r}, model {want[i]!r}')
    assert np.isfinite(want).all(), what
    print(f'{what}: rows {want.shape[0]}, channels {want.shape[1]}, {want.size} elements, bits equal')
    return want.size


def _layer(cls, cin, cout, k, dev, seed=2, **kw):
    layer = cls(cin, cout, k, **kw).to(dev).eval()
    w, b = ref.weights(k, cin, cout, seed=seed)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(w)); layer.bias.copy_(torch.from_numpy(b))
    return layer, w, b


@pytest.mark.parametrize('cout', [3, 16, 48, 112])
@pytest.mark.parametrize('cin', [6, 16, 32, 112, 192, 224])
def test_layers_over_the_channel_grid_have_the_bits_of_the_model(cin, cout, cuda_device):
    """SubMConv3d k = 3 and k = 1, SparseConv3d and SparseInverseConv3d, each cin -> cout, with prologue + residual and with neither."""
    dev, t = cuda_device, _tables(96)
    idx, n, m = t['idx'], 96, len(t['out_idx'])
    assert 20 <= m < n and t['dropped'].sum() >= 6
    x, y = ref.features(n, cin), ref.features(m, cin, seed=6)
    rng = np.random.default_rng(9)
    total = 0
    for full in (False, True):
        scale, shift = ref.bn_params(cin) if full else (None, None)
        prologue = (_dev(scale, dev), _dev(shift, dev)) if full else None
        res = lambda rows: rng.uniform(-1, 1, (rows, cout)).astype(np.float32) if full else None
        tensor = lambda: spconv.SparseConvTensor(_dev(x, dev), _dev(idx, dev), ref.SHAPE, ref.BATCH)
        what = f'{cin}->{cout} prologue + residual {full}'
        with torch.no_grad():
            subm, w, b = _layer(spconv.SubMConv3d, cin, cout, 3, dev, padding=1, indice_key='subm1')
            r = res(n)
            out = subm(tensor(), prologue=prologue, residual=_dev(r, dev))
            assert torch.equal(out.indices.cpu(), torch.from_numpy(idx))
            total += _bits_equal(out.features, ref.conv_exact(x, t['subm'][0], w, b, scale, shift, r), f'subm K = 27 {what}')

            one, w, b = _layer(spconv.SubMConv3d, cin, cout, 1, dev, seed=3)
            r = res(n)
            out = one(tensor(), prologue=prologue, residual=_dev(r, dev))
            total += _bits_equal(out.features, ref.conv_exact(x, t['k1'][0], w, b, scale, shift, r), f'subm K = 1 {what}')

            down, w, b = _layer(spconv.SparseConv3d, cin, cout, 2, dev, stride=2, indice_key='spconv1')
            r = res(m)
            fine = tensor()
            out = down(fine, prologue=prologue, residual=_dev(r, dev))
            assert torch.equal(out.indices.cpu(), torch.from_numpy(t['out_idx'])) and tuple(out.spatial_shape) == t['out_shape']
            total += _bits_equal(out.features, ref.conv_exact(x, t['down'][0], w, b, scale, shift, r), f'strided K = 8 {what}')

            inv, w, b = _layer(spconv.SparseInverseConv3d, cin, cout, 2, dev, seed=4, indice_key='spconv1')
            r = res(n)
            coarse = spconv.SparseConvTensor(_dev(y, dev), out.indices, out.spatial_shape, ref.BATCH)
            coarse.indice_dict = fine.indice_dict
            up = inv(coarse, prologue=prologue, residual=_dev(r, dev))
            assert torch.equal(up.indices.cpu(), torch.from_numpy(idx))
            total += _bits_equal(up.features, ref.conv_exact(y, t['inverse'][0], w, b, scale, shift, r), f'inverse K = 8 {what}')
    print(f'channel grid {cin}->{cout}: {total} elements compared, all bits equal')


@pytest.mark.parametrize('cin,cout', [(32, 48), (6, 3)])
@pytest.mark.parametrize('n', [1, 31, 32, 33, 65])
def test_every_prologue_residual_bias_combination_on_partial_tiles(n, cin, cout, cuda_device):
    """spconv.sparse_conv itself, so that bias = None reaches the kernel as NULL (the layer classes always pass theirs)."""
    dev, t = cuda_device, _tables(n)
    total = 0
    for kind in KINDS:
        nbr, n_in, n_out = t[kind]
        if n_out == 0:
            print(f'n {n} {kind} {cin}->{cout}: the strided layer drops every site of this scene, nothing to compare')
            continue
        K = nbr.shape[1]
        x = ref.features(n_in, cin, seed=31)
        rng = np.random.default_rng(9)
        w = rng.uniform(-1, 1, (K, cin, cout)).astype(np.float32) * np.float32(np.sqrt(3.0 / cin))
        bias, r = rng.uniform(-1, 1, cout).astype(np.float32), rng.uniform(-1, 1, (n_out, cout)).astype(np.float32)
        scale, shift = ref.bn_params(cin)
        d_x, d_nbr, d_w = _dev(x, dev), _dev(nbr, dev), _dev(w, dev)
        for pro, res, bi in itertools.product((False, True), repeat=3):
            kw = dict(bias=bias if bi else None, scale=scale if pro else None, shift=shift if pro else None, residual=r if res else None)
            got = spconv.sparse_conv(d_x, d_nbr, d_w, **{k: _dev(v, dev) for k, v in kw.items()})
            total += _bits_equal(got, ref.conv_exact(x, nbr, w, **kw), f'n {n} {kind} {cin}->{cout} prologue {pro} residual {res} bias {bi}')
    assert total > 0
    print(f'combinations n {n} {cin}->{cout}: {total} elements compared, all bits equal')


@pytest.mark.parametrize('half,cout', [(16, 16), (112, 112)])
def test_two_sources_have_the_bits_of_the_model_on_the_concatenation(half, cout, cuda_device):
    dev, t = cuda_device, _tables(96)
    cin = 2 * half
    total = 0
    for kind in KINDS:
        nbr, n_in, n_out = t[kind]
        K = nbr.shape[1]
        xa, xb = ref.features(n_in, half, seed=21), ref.features(n_in, half, seed=22)
        rng = np.random.default_rng(9)
        w = rng.uniform(-1, 1, (K, cin, cout)).astype(np.float32) * np.float32(np.sqrt(3.0 / cin))
        bias, r = rng.uniform(-1, 1, cout).astype(np.float32), rng.uniform(-1, 1, (n_out, cout)).astype(np.float32)
        scale, shift = ref.bn_params(cin)
        for full in (False, True):
            kw = dict(bias=bias, scale=scale if full else None, shift=shift if full else None, residual=r if full else None)
            got = spconv.sparse_conv(_dev(xa, dev), _dev(nbr, dev), _dev(w, dev), features_b=_dev(xb, dev), **{k: _dev(v, dev) for k, v in kw.items()})
            total += _bits_equal(got, ref.conv_exact(np.concatenate([xa, xb], 1), nbr, w, **kw), f'{kind} {half}+{half}->{cout} prologue + residual {full}')
    print(f'two sources {half}+{half}->{cout}: {total} elements compared, all bits equal')


@pytest.mark.parametrize('cin,cout', [(32, 48), (6, 3)])
def test_a_nan_stays_in_the_rows_that_read_it(cin, cout, cuda_device):
    """One NaN in one channel of one site, no prologue: the rows that read the site are NaN in every column, every other row keeps
    the bits of the model (also the rows that share a 32-row tile, and with it an MFMA, with a reader)."""
    dev, t = cuda_device, _tables(96)
    total = 0
    for kind in ('subm', 'down', 'inverse'):
        nbr, n_in, n_out = t[kind]
        site = int(np.bincount(nbr[nbr >= 0], minlength=n_in).argmax())          # the most-read input row: the centre of the full block for subm
        reads = (nbr == site).any(1)
        assert 0 < reads.sum() < n_out and (kind != 'subm' or reads.sum() == 27)
        x = ref.features(n_in, cin, seed=41)
        x[site, cin - 1] = np.nan
        rng = np.random.default_rng(9)
        w = rng.uniform(-1, 1, (nbr.shape[1], cin, cout)).astype(np.float32) * np.float32(np.sqrt(3.0 / cin))
        bias, r = rng.uniform(-1, 1, cout).astype(np.float32), rng.uniform(-1, 1, (n_out, cout)).astype(np.float32)
        got = spconv.sparse_conv(_dev(x, dev), _dev(nbr, dev), _dev(w, dev), bias=_dev(bias, dev), residual=_dev(r, dev)).cpu().numpy()
        want = ref.conv_exact(x, nbr, w, bias, residual=r)
        assert np.isnan(want[reads]).all() and np.isnan(got[reads]).all(), kind
        total += _bits_equal(torch.from_numpy(got[~reads]), want[~reads], f'{kind} {cin}->{cout}: {int(reads.sum())} rows NaN in every column, the others')
    print(f'NaN isolation {cin}->{cout}: {total} elements compared, all bits equal')


def test_the_prologue_returns_zero_for_a_nan(cuda_device):
    """max(x*scale + shift, 0) is C's fmaxf: a NaN feature enters the sum as 0, where torch.relu would hand the NaN on.  Pinned as the
    kernel's documented behaviour (include/catgrasp_amd_sparse.h, spconv.py): no NaN in the output, and the bits of the launch with
    that feature cut by the ReLU."""
    dev, t = cuda_device, _tables(96)
    nbr, n_in, n_out = t['subm']
    cin, cout = 32, 48
    x = ref.features(n_in, cin, seed=41)
    scale, shift = ref.bn_params(cin)
    c = int(np.nonzero(scale > 0)[0][0])
    site = int(np.bincount(nbr[nbr >= 0], minlength=n_in).argmax())
    w, b = ref.weights(3, cin, cout)
    run = lambda v: spconv.sparse_conv(_dev(v, dev), _dev(nbr, dev), _dev(w.reshape(27, cin, cout), dev), bias=_dev(b, dev), scale=_dev(scale, dev), shift=_dev(shift, dev))
    clean = run(x)
    x[site, c] = np.nan
    got = run(x)
    assert not torch.isnan(got).any() and not torch.equal(got, clean)
    _bits_equal(got, ref.conv_exact(x, nbr, w, b, scale, shift), 'prologue of a NaN')
    x[site, c] = -1e6
    assert torch.equal(got, run(x))
