"""GPU tests of the two-source sparse convolution (cg_sparse_conv_cat, spconv.sparse_conv(..., features_b=)): on the layer tests' scenes
and all four kinds of rule book it has the bits of cg_sparse_conv on torch.cat((a, b), 1), and is within the suite's bar of the float64
restatement tests/sparse_ref.py."""
import numpy as np
import pytest
import torch

import catgrasp_amd.spconv as spconv
import sparse_ref as ref

pytestmark = pytest.mark.gpu

BAR = 1e-4
SCENES = {'full299': dict(n=299), 'n33': dict(n=33, special=False), 'n1': dict(n=1, special=False)}
WIDTHS = [(16, 16), (48, 48), (96, 96), (32, 16)]
COUTS = [16, 48, 96]
_TABLES = {}


def _tables(name):
    """{kind: (nbr, rows read, rows written)} of a scene from the restatement, computed once."""
    if name not in _TABLES:
        idx = ref.scene(**SCENES[name])
        out_idx, down, _, _ = ref.down_rules(idx, ref.SHAPE)
        n, m = len(idx), len(out_idx)
        _TABLES[name] = {'subm': (ref.subm_rules(idx, ref.SHAPE), n, n), 'down': (down, n, m), 'inverse': (ref.inverse_rules(idx, out_idx, ref.SHAPE), m, n),
                         'k1': (np.arange(n, dtype=np.int32).reshape(n, 1), n, n)}
    return _TABLES[name]


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _err(got, want):
    got = got.cpu().numpy().astype(np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max(initial=0.0))


@pytest.mark.parametrize('cin_a,cin_b', WIDTHS)
@pytest.mark.parametrize('name', list(SCENES))
def test_two_sources_have_the_bits_of_the_concatenated_launch(name, cin_a, cin_b, cuda_device):
    dev, cin = cuda_device, cin_a + cin_b
    worst = 0.0
    for kind, (nbr, n_in, n_out) in _tables(name).items():
        K = nbr.shape[1]
        xa, xb = ref.features(n_in, cin_a, seed=21), ref.features(n_in, cin_b, seed=22)
        cat = np.concatenate([xa, xb], 1)
        d_nbr, d_a, d_b = _dev(nbr, dev), _dev(xa, dev), _dev(xb, dev)
        d_cat = torch.cat((d_a, d_b), 1)
        scale, shift = ref.bn_params(cin)
        rng = np.random.default_rng(9)
        for cout in COUTS:
            w = rng.uniform(-1, 1, (K, cin, cout)).astype(np.float32) * np.float32(np.sqrt(3.0 / cin))
            b = rng.uniform(-1, 1, cout).astype(np.float32)
            r = rng.uniform(-1, 1, (n_out, cout)).astype(np.float32)
            d_w, d_bias = _dev(w, dev), _dev(b, dev)
            # the sources swapped together with the weight's row blocks and the prologue's halves: the same sum in another order
            swap = lambda v: np.concatenate([v[..., cin_a:, :], v[..., :cin_a, :]], -2) if v.ndim > 1 else np.concatenate([v[cin_a:], v[:cin_a]])
            for pro in (False, True):
                for res in (False, True):
                    sc, sh = (scale, shift) if pro else (None, None)
                    kw = dict(bias=d_bias, scale=_dev(sc, dev), shift=_dev(sh, dev), residual=_dev(r, dev) if res else None)
                    got = spconv.sparse_conv(d_a, d_nbr, d_w, features_b=d_b, **kw)
                    one = spconv.sparse_conv(d_cat, d_nbr, d_w, **kw)
                    what = f'{name} {kind} {cin_a}+{cin_b}->{cout} pro {pro} res {res}'
                    assert got.shape == (n_out, cout) and torch.equal(got, one), what
                    want = ref.conv(cat, nbr, w, b, sc, sh, r if res else None)
                    e = _err(got, want)
                    kw.update(scale=_dev(swap(sc), dev) if pro else None, shift=_dev(swap(sh), dev) if pro else None)
                    swapped = spconv.sparse_conv(d_b, d_nbr, _dev(swap(w), dev), features_b=d_a, **kw)
                    es = _err(swapped, want)
                    worst = max(worst, e, es)
                    assert e <= BAR and es <= BAR, (what, e, es)
    print(f'{name} {cin_a}+{cin_b}: max |got - ref| / max(1, |ref|) = {worst:.3g} (bar {BAR:g})')


def test_layers_take_a_second_source_and_refuse_what_is_not_built(cuda_device):
    dev = cuda_device
    idx = ref.scene(**SCENES['full299'])
    n = len(idx)
    xa, xb = _dev(ref.features(n, 32, seed=21), dev), _dev(ref.features(n, 16, seed=22), dev)
    layer = spconv.SubMConv3d(48, 16, 3, padding=1, indice_key='subm1').to(dev).eval()
    with torch.no_grad():
        t = spconv.SparseConvTensor(xa, _dev(idx, dev), ref.SHAPE, ref.BATCH)
        two = layer(t, features_b=xb)
        one = layer(spconv.SparseConvTensor(torch.cat((xa, xb), 1), _dev(idx, dev), ref.SHAPE, ref.BATCH))
        assert torch.equal(two.features, one.features) and two.indice_dict is t.indice_dict
        nbr = t.indice_dict['subm1'].nbr
        with pytest.raises(ValueError, match='features_b'):                                        # a host tensor never reaches the kernel
            spconv.sparse_conv(xa, nbr, torch.zeros(27, 48, 16, device=dev), features_b=xb.cpu())
        for a, b in ((8, 8), (24, 8), (16, 24)):          # each source a multiple of 16
            with pytest.raises(spconv.L.CatgraspAmdError, match='cg_sparse_conv_cat'):
                spconv.sparse_conv(torch.zeros(n, a, device=dev), nbr, torch.zeros(27, a + b, 16, device=dev), features_b=torch.zeros(n, b, device=dev))
        with pytest.raises(spconv.L.CatgraspAmdError, match='cg_sparse_conv_cat'):                 # the sum above 224
            spconv.sparse_conv(torch.zeros(n, 128, device=dev), nbr, torch.zeros(27, 240, 16, device=dev), features_b=torch.zeros(n, 112, device=dev))
