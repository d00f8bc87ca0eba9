"""GPU tests of the sparse convolution layers' gradients (catgrasp_amd/spconv_autograd.py, csrc/sparse_conv_grad.hip).

Yardstick: tests/sparse_grad_ref.py -- float64 gradients pinned against torch autograd through dense float64 convolutions, and the
float32 restatements of the two kernels' chains (tests/test_sparse_grad_ref_cpu.py).

Bounds.  dW, dx and db are per element within 1e-4 * max(1, |ref|), the suite's standing bar (BAR of tests/test_sparse_conv_gpu.py).
dy is uniform in +-sqrt(3 / n_out), so the weight gradients are of order one.  So that the bar is not an absolute one that a lost
neighbour could hide under, every compared tensor is checked from the float64 reference alone: at least half of its entries exceed
1e-2 in magnitude.  Entries that are zero by structure are left out of that count and must be EXACTLY zero in the result instead:
dW[k] of an offset that no row of the scene uses (26 of the 27 offsets of a one-site scene), dx of a row that no output reads (the
sites the strided layer drops), everything when the layer has no output row.  The bit-for-bit tests have no bound at all.

Shapes: the scenes of tests/test_sparse_conv_gpu.py and the small edge scenes of tests/sparse_ref.py (the `unit` scene has an axis of
1: no strided layer exists on it, the submanifold and 1x1x1 layers run), and one scene of 2*CG_SPARSE_GRAD_ROWS + 1 sites: the chunk
boundary, a last chunk of one row and the cross-chunk pass."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import catgrasp_amd.spconv as base
import catgrasp_amd.spconv_autograd as spconv
import sparse_grad_ref as gref
import sparse_ref as ref
from catgrasp_amd import _lib

pytestmark = pytest.mark.gpu

BAR = 1e-4
SCENE_KW = OrderedDict([('full299', dict(n=299)), ('n1', dict(n=1, special=False)), ('n33', dict(n=33, special=False)), ('n301', dict(n=301, seed=5)),
                        ('empty_item0', dict(n=120, special=False, only_item=1))])
EDGE = ('unit', 'two', 'three_two_five', 'dense', 'all_dropped', 'mostly_dropped', 'mostly_dropped_x20')
SCENES = list(SCENE_KW) + list(EDGE) + ['chunks']
# (kind, Cin, Cout): submanifold 3x3x3 four times, strided, inverse, 1x1x1, and the widest submanifold layer
PAIRS = [('subm', 6, 16), ('subm', 16, 3), ('subm', 16, 16), ('subm', 32, 16), ('down', 16, 32), ('inverse', 32, 16), ('k1', 32, 16), ('subm', 224, 112)]
KSIZE = {'subm': 3, 'down': 2, 'inverse': 2, 'k1': 1}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """-> (indices, spatial shape, batch size, books)"""
    if name in SCENE_KW:
        idx, shape, batch = ref.scene(**SCENE_KW[name]), ref.SHAPE, ref.BATCH
    elif name == 'chunks':
        idx, shape, batch = gref.big_scene()
    else:
        idx, shape, batch = ref.edge_scene(name)
    return idx, tuple(shape), batch, gref.books(idx, shape)


def _populated(want, structural_zero, what):
    """From the float64 reference alone: at least half of the entries that are not zero by structure exceed 1e-2."""
    live = np.abs(want[~structural_zero])
    assert not want[structural_zero].any(), what
    share = float((live > 1e-2).mean()) if live.size else 1.0
    assert share >= 0.5, (what, share, live.size)
    return share


@functools.lru_cache(maxsize=None)
def _reference(name, kind, cin, cout):
    """Inputs and float64 gradients of one layer on one scene, computed once: dict(x, w, b, dy, dw, dx, db, zero_w, zero_x)."""
    idx, shape, batch, books = _scene(name)
    nbr, nbr_t, flip, n_in, n_out = books[kind]
    x = ref.features(n_in, cin, seed=1 if kind != 'inverse' else 6)
    w, b = ref.weights(KSIZE[kind], cin, cout, seed=2 + list(KSIZE).index(kind))
    dy = gref.dy_for(n_out, cout)
    dw, dx, db = gref.grads(x, nbr, w, dy)
    zero_w = np.broadcast_to(~(nbr >= 0).any(0)[:, None, None], dw.shape)
    zero_x = np.broadcast_to(~(nbr_t >= 0).any(1)[:, None], dx.shape)
    what = f'{name} {kind} {cin}->{cout}'
    shares = (_populated(dw, zero_w, what + ' dW'), _populated(dx, zero_x, what + ' dx'), _populated(db, np.full(db.shape, n_out == 0), what + ' db'))
    return dict(x=x, w=w, b=b, dy=dy, dw=dw, dx=dx, db=db, zero_w=zero_w, zero_x=zero_x, nbr=nbr, nbr_t=nbr_t, flip=flip, shares=shares)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _make(mod, kind, cin, cout, dev, w=None, b=None):
    k = KSIZE[kind]
    if kind == 'subm':
        layer = mod.SubMConv3d(cin, cout, 3, padding=1, indice_key='subm1')
    elif kind == 'k1':
        layer = mod.SubMConv3d(cin, cout, 1)
    elif kind == 'down':
        layer = mod.SparseConv3d(cin, cout, 2, stride=2, indice_key='spconv1')
    else:
        layer = mod.SparseInverseConv3d(cin, cout, 2, indice_key='spconv1')
    layer = layer.to(dev)
    if w is not None:
        with torch.no_grad():
            layer.weight.copy_(torch.from_numpy(w).reshape(k, k, k, cin, cout)); layer.bias.copy_(torch.from_numpy(b))
    return layer


def _input(name, kind, x, dev, requires_grad=True):
    """The layer's input tensor on the scene; for the inverse layer, the strided layer's output sites carrying x."""
    idx, shape, batch, _ = _scene(name)
    feats = _dev(x, dev).requires_grad_(requires_grad)
    if kind != 'inverse':
        return spconv.SparseConvTensor(feats, _dev(idx, dev), shape, batch), feats
    fine = spconv.SparseConvTensor(torch.zeros((len(idx), 16), device=dev), _dev(idx, dev), shape, batch)
    with torch.no_grad():
        lo = base.SparseConv3d(16, 16, 2, stride=2, indice_key='spconv1').to(dev)(fine)
    coarse = spconv.SparseConvTensor(feats, lo.indices, lo.spatial_shape, batch)
    coarse.indice_dict = fine.indice_dict
    return coarse, feats


def _backward(name, kind, cin, cout, dev, r=None):
    """-> (dW (K, Cin, Cout), dx, db) of the layer on the device, and the reference record."""
    r = r or _reference(name, kind, cin, cout)
    layer = _make(spconv, kind, cin, cout, dev, r['w'], r['b'])
    t, feats = _input(name, kind, r['x'], dev)
    out = layer(t)
    assert out.features.shape == r['dy'].shape and out.features.requires_grad
    out.features.backward(_dev(r['dy'], dev))
    return layer.weight.grad.reshape(-1, cin, cout), feats.grad, layer.bias.grad, r


def _check(got, want, zero, what):
    got = got.detach().cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = float((np.abs(got.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))).max(initial=0.0))
    print(f'{what}: {want.size} elements, max |got - ref| / max(1, |ref|) = {err:.3g} (bar {BAR:g}), max |ref| = {np.abs(want).max(initial=0.0):.3g}')
    assert np.isfinite(got).all() and err <= BAR, (what, err)
    assert not got[zero].any(), what                                         # zero by structure: exactly zero


@pytest.mark.parametrize('name', SCENES)
def test_gradients_against_float64_per_element(name, cuda_device):
    _, shape, _, books = _scene(name)
    ran = 0
    for kind, cin, cout in PAIRS:
        if kind not in books:
            assert name == 'unit' and min(shape) < 2                          # an axis of 1: there is no strided layer on this grid
            continue
        dw, dx, db, r = _backward(name, kind, cin, cout, cuda_device)
        what = f'{name} {kind} {cin}->{cout}'
        print(f'{what}: share of entries above 1e-2 in the float64 reference: dW {r["shares"][0]:.2f}, dx {r["shares"][1]:.2f}, db {r["shares"][2]:.2f}')
        _check(dw, r['dw'], r['zero_w'], what + ' dW')
        _check(dx, r['dx'], r['zero_x'], what + ' dx')
        _check(db, r['db'], np.zeros(cout, bool) if len(r['dy']) else np.ones(cout, bool), what + ' db')
        ran += 1
    assert ran == (6 if name == 'unit' else 8)


def test_no_output_rows_give_zero_weight_and_bias_gradients(cuda_device):
    """The strided layer on `all_dropped` has n_in = 38 and n_out = 0: cg_sparse_conv_wgrad zeroes dw and db and is CG_OK with no
    workspace, and every dx row is zero."""
    r = _reference('all_dropped', 'down', 16, 32)
    assert r['dy'].shape == (0, 32) and r['x'].shape[0] == 38
    dw, dx, db, _ = _backward('all_dropped', 'down', 16, 32, cuda_device)
    assert dw.shape == (8, 16, 32) and not dw.any() and not db.any() and dx.shape == (38, 16) and not dx.any()
    dw = torch.full((8, 16, 32), 7.0, device=cuda_device)
    db = torch.full((32,), 7.0, device=cuda_device)
    p = _lib._p
    assert _lib.lib().cg_sparse_wgrad_workspace(0, 8, 16, 32) == 0
    assert _lib.lib().cg_sparse_conv_wgrad(None, 38, None, 0, 8, None, 16, 32, None, p(dw), p(db), _lib._stream()) == 0
    assert not dw.any() and not db.any()


def _bits_equal(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        i = np.unravel_index(np.argmin(same), same.shape)
        raise AssertionError(f'{what}: {int((~same).sum())} of {same.size} elements differ in their bits; first at {i}: got {got[i]!r}, model {want[i]!r}')
    assert np.isfinite(want).all(), what
    print(f'{what}: {want.size} elements, bits equal')


@pytest.mark.parametrize('name,kind,cin,cout', [('full299', 'subm', 16, 16), ('full299', 'subm', 6, 16), ('full299', 'down', 16, 32),
                                                ('full299', 'inverse', 32, 16), ('full299', 'k1', 32, 16), ('n33', 'subm', 16, 16),
                                                ('n33', 'subm', 6, 16), ('n33', 'subm', 16, 3), ('chunks', 'subm', 16, 16)])
def test_gradients_have_the_bits_of_the_stated_chains(name, kind, cin, cout, cuda_device):
    dw, dx, db, r = _backward(name, kind, cin, cout, cuda_device)
    want_w, want_b = gref.wgrad_exact(r['x'], r['nbr'], r['dy'])
    what = f'{name} {kind} {cin}->{cout}'
    _bits_equal(dw, want_w, what + ' dW')
    _bits_equal(db, want_b, what + ' db')
    _bits_equal(dx, gref.dgrad_exact(r['dy'], r['nbr_t'], r['w'], r['flip']), what + ' dx')
    if name == 'chunks':
        assert len(r['dy']) == 2 * gref.ROWS + 1 == 2 * spconv.grad_rows() + 1
        flat = gref.wgrad_exact(r['x'], r['nbr'], r['dy'], rows=len(r['dy']))[0]
        assert (flat.view(np.uint32) != want_w.view(np.uint32)).mean() > 0.05          # the chunking is there to be seen


def test_backward_is_reproducible_and_the_same_on_a_side_stream(cuda_device):
    for name, kind, cin, cout in (('chunks', 'subm', 32, 16), ('full299', 'down', 16, 32), ('full299', 'inverse', 32, 16)):
        first = _backward(name, kind, cin, cout, cuda_device)[:3]
        again = _backward(name, kind, cin, cout, cuda_device)[:3]
        side = torch.cuda.Stream(device=cuda_device)
        side.wait_stream(torch.cuda.current_stream(cuda_device))
        with torch.cuda.stream(side):
            other = _backward(name, kind, cin, cout, cuda_device)[:3]
        side.synchronize()
        for a, b, c in zip(first, again, other):
            assert torch.equal(a, b) and torch.equal(a, c), (name, kind)


def test_only_the_gradients_asked_for_are_computed(cuda_device, monkeypatch):
    calls = []
    real_w, real_d = spconv.sparse_conv_wgrad, spconv.sparse_conv_dgrad
    monkeypatch.setattr(spconv, 'sparse_conv_wgrad', lambda *a: calls.append(('w',) + tuple(a[4:])) or real_w(*a))
    monkeypatch.setattr(spconv, 'sparse_conv_dgrad', lambda *a: calls.append(('d',)) or real_d(*a))
    r = _reference('full299', 'subm', 16, 16)
    dy = _dev(r['dy'], cuda_device)

    def run(weight, bias, feats):
        del calls[:]
        layer = _make(spconv, 'subm', 16, 16, cuda_device, r['w'], r['b'])
        layer.weight.requires_grad_(weight); layer.bias.requires_grad_(bias)
        t, x = _input('full299', 'subm', r['x'], cuda_device, requires_grad=feats)
        layer(t).features.backward(dy)
        return layer.weight.grad, layer.bias.grad, x.grad, list(calls)

    dw, db, dx, seen = run(True, True, True)
    assert seen == [('d',), ('w', True, True)] and dw is not None and db is not None and dx is not None
    fw, fb, fx, seen = run(False, True, True)                                   # a frozen weight: no dW, its kernel slots are not launched
    assert seen == [('d',), ('w', False, True)] and fw is None and torch.equal(fb, db) and torch.equal(fx, dx)
    fw, fb, fx, seen = run(False, False, True)                                  # nothing of the weight pass is wanted: it does not run
    assert seen == [('d',)] and fw is None and fb is None and torch.equal(fx, dx)
    fw, fb, fx, seen = run(True, False, False)                                  # a detached input: no dx, no input pass
    assert seen == [('w', True, False)] and fx is None and fb is None and torch.equal(fw, dw)
    _check(dw.reshape(27, 16, 16), r['dw'], r['zero_w'], 'dW again')
    # a non-contiguous gradient is made contiguous; another precision is refused
    layer = _make(spconv, 'subm', 16, 16, cuda_device, r['w'], r['b'])
    t, x = _input('full299', 'subm', r['x'], cuda_device)
    wide = torch.zeros((299, 32), device=cuda_device)
    wide[:, ::2] = dy
    layer(t).features.backward(wide[:, ::2])
    assert torch.equal(layer.weight.grad, dw) and torch.equal(x.grad, dx)
    with pytest.raises(NotImplementedError, match='float32'):
        spconv.SparseConvFunction.backward(type('ctx', (), dict(saved_tensors=(None,) * 4, needs_input_grad=(True,) * 6, flip=True))(), dy.double())
    with pytest.raises(NotImplementedError, match='features_b'):
        layer(t, features_b=torch.zeros((299, 16), device=cuda_device))


def test_without_gradients_the_layers_are_the_inference_layers(cuda_device):
    dev = cuda_device
    for kind, cin, cout in (('subm', 32, 16), ('down', 16, 32), ('inverse', 32, 16), ('k1', 32, 16)):
        r = _reference('full299', kind, cin, cout)
        new, old = _make(spconv, kind, cin, cout, dev, r['w'], r['b']), _make(base, kind, cin, cout, dev, r['w'], r['b'])
        scale, shift = (_dev(a, dev) for a in ref.bn_params(cin))
        res = _dev(np.random.default_rng(9).uniform(-1, 1, r['dy'].shape).astype(np.float32), dev)
        for kw in (dict(), dict(prologue=(scale, shift)), dict(residual=res), dict(prologue=(scale, shift), residual=res)):
            with torch.no_grad():
                a = new(_input('full299', kind, r['x'], dev, requires_grad=False)[0], **kw)
                b = old(_input('full299', kind, r['x'], dev, requires_grad=False)[0], **kw)
            assert torch.equal(a.features, b.features) and torch.equal(a.indices, b.indices) and not a.features.requires_grad, (kind, list(kw))
            # with gradients enabled and nothing that asks for one, too
            for p in new.parameters():
                p.requires_grad_(False)
            c = new(_input('full299', kind, r['x'], dev, requires_grad=False)[0], **kw)
            assert torch.equal(c.features, b.features)
            for p in new.parameters():
                p.requires_grad_(True)
            # and the differentiable forward without prologue and residual has the inference layer's bits
            if not kw:
                d = new(_input('full299', kind, r['x'], dev)[0])
                assert d.features.requires_grad and torch.equal(d.features.detach(), b.features)


def test_the_eval_mode_batchnorm_relu_fold_gives_the_float64_gradients(cuda_device):
    dev = cuda_device
    idx, shape, batch, books = _scene('full299')
    nbr = books['subm'][0]
    cin, cout = 16, 32
    r = _reference('full299', 'subm', cin, cout)
    rng = np.random.default_rng(77)
    bn = nn.BatchNorm1d(cin, eps=1e-4).to(dev)
    with torch.no_grad():
        bn.weight.copy_(_dev((rng.uniform(0.5, 1.5, cin) * rng.choice([-1, 1], cin)).astype(np.float32), dev))
        bn.bias.copy_(_dev(rng.uniform(-0.5, 0.5, cin).astype(np.float32), dev))
        bn.running_mean.copy_(_dev(rng.uniform(-0.3, 0.3, cin).astype(np.float32), dev))
        bn.running_var.copy_(_dev(rng.uniform(0.5, 2.0, cin).astype(np.float32), dev))
    g, be, m, v = (a.detach().cpu().numpy().astype(np.float64) for a in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    scale = g / np.sqrt(v + bn.eps)
    shift = be - m * scale
    pre = r['x'].astype(np.float64) * scale + shift
    assert np.abs(pre).min() >= 1e-6                                     # float32 and float64 agree on every ReLU mask
    conv = _make(spconv, 'subm', cin, cout, dev, r['w'], r['b'])
    seq = spconv.SparseSequential(bn, nn.ReLU(), conv).eval()
    t, feats = _input('full299', 'subm', r['x'], dev)
    out = seq(t)
    assert torch.equal(t.features.detach().cpu(), torch.from_numpy(r['x']))   # folded: the input's features are not rewritten
    out.features.backward(_dev(r['dy'], dev))
    dw, dp, db = gref.grads(np.maximum(pre, 0.0), nbr, r['w'], r['dy'])
    none = np.zeros(1, bool)
    _check(conv.weight.grad.reshape(27, cin, cout), dw, r['zero_w'], 'fold dW')
    _check(conv.bias.grad, db, np.zeros(cout, bool), 'fold db')
    dx = dp * (pre > 0) * scale
    _populated(dx, np.broadcast_to(none, dx.shape) | (pre <= 0), 'fold dx')
    _check(feats.grad, dx, pre <= 0, 'fold dx')
    want = ref.conv(r['x'], nbr, r['w'], r['b'], scale, shift)
    assert float((np.abs(out.features.detach().cpu().numpy() - want) / np.maximum(1, np.abs(want))).max()) <= BAR


# ------------------------------------------------------------------------------------------------------------ a small network
class _Net(nn.Module):
    """The reference's wiring in small: input conv, a BatchNorm / activation / conv block, one U level with its skip, a 1x1x1 head."""

    def __init__(self, mod):
        super().__init__()
        S = mod.SparseSequential
        self.input_conv = S(mod.SubMConv3d(6, 16, kernel_size=3, padding=1, bias=True, indice_key='subm1'))
        self.block = S(nn.BatchNorm1d(16), nn.Tanh(), mod.SubMConv3d(16, 16, kernel_size=3, padding=1, bias=True, indice_key='subm1'))
        self.conv = S(mod.SparseConv3d(16, 32, kernel_size=2, stride=2, bias=True, indice_key='spconv1'))
        self.inner = S(mod.SubMConv3d(32, 32, kernel_size=3, padding=1, bias=True, indice_key='subm2'))
        self.deconv = S(mod.SparseInverseConv3d(32, 16, kernel_size=2, bias=True, indice_key='spconv1'))
        self.head = S(mod.SubMConv3d(32, 16, kernel_size=1, bias=True))

    def forward(self, x):
        skip = self.block(self.input_conv(x))
        identity = skip.features
        up = self.deconv(self.inner(self.conv(skip)))
        up.features = torch.cat((identity, up.features), dim=1)
        return self.head(up).features


def _dense_net_float64(sd, idx, x, shape, batch):
    """The same network from dense float64 torch convolutions over the densified tensor, masked to the active sites.
    -> {state_dict key: gradient} of loss = sum(out^2) / out.numel()."""
    P = {k: v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point and 'running' not in k) for k, v in sd.items()}
    i = torch.from_numpy(idx.astype(np.int64))
    out_idx = torch.from_numpy(ref.down_rules(idx, shape)[0].astype(np.int64))
    cshape = tuple((s - 2) // 2 + 1 for s in shape)

    def dense(rows, ii, shp):
        return torch.zeros((batch,) + tuple(shp) + (rows.shape[1],), dtype=torch.float64).index_put((ii[:, 0], ii[:, 1], ii[:, 2], ii[:, 3]), rows).permute(0, 4, 1, 2, 3)

    def at(d, ii):
        return d[ii[:, 0], :, ii[:, 1], ii[:, 2], ii[:, 3]]

    def conv(rows, ii, shp, key, oi=None, **kw):
        w = P[key + '.weight']
        return at(F.conv3d(dense(rows, ii, shp), w.permute(4, 3, 0, 1, 2), P[key + '.bias'], **kw), ii if oi is None else oi)

    a = conv(torch.from_numpy(x).double(), i, shape, 'input_conv.0', padding=1)
    a = F.batch_norm(a, None, None, P['block.0.weight'], P['block.0.bias'], training=True, eps=1e-5)
    skip = conv(torch.tanh(a), i, shape, 'block.2', padding=1)
    lo = conv(skip, i, shape, 'conv.0', oi=out_idx, stride=2)
    lo = conv(lo, out_idx, cshape, 'inner.0', padding=1)
    up = F.conv_transpose3d(dense(lo, out_idx, cshape), P['deconv.0.weight'].permute(3, 4, 0, 1, 2), None, stride=2)
    up = F.pad(up, (0, shape[2] - up.shape[4], 0, shape[1] - up.shape[3], 0, shape[0] - up.shape[2]))
    up = at(up, i) + P['deconv.0.bias']                                     # a site the strided layer dropped gets the bias only
    out = torch.cat((skip, up), 1) @ P['head.0.weight'].reshape(32, 16) + P['head.0.bias']
    (out.pow(2).sum() / out.numel()).backward()
    return {k: p.grad.numpy() for k, p in P.items() if p.requires_grad}, out.detach().numpy()


def test_a_small_network_trains_to_the_float64_gradients_and_deploys_on_the_inference_layers(cuda_device):
    dev = cuda_device
    idx, shape, batch, _ = _scene('full299')
    x = ref.features(299, 6)
    torch.manual_seed(5)
    net = _Net(spconv).to(dev).train()
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 5:
                p.mul_(3.0)                                                 # kaiming_uniform(a = sqrt(5)) is a third of +-sqrt(3 / fan): outputs of order one
        net.block[0].weight.copy_(torch.linspace(0.5, 1.5, 16)); net.block[0].bias.copy_(torch.linspace(-0.3, 0.3, 16))
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    out = net(spconv.SparseConvTensor(_dev(x, dev), _dev(idx, dev), shape, batch))
    loss = out.pow(2).sum() / out.numel()
    loss.backward()
    want, out64 = _dense_net_float64(sd, idx, x, shape, batch)
    assert float((np.abs(out.detach().cpu().numpy() - out64) / np.maximum(1, np.abs(out64))).max()) <= BAR
    grads = dict(net.named_parameters())
    assert sorted(want) == sorted(grads) and len(want) == 14
    for k in sorted(want):
        got = grads[k].grad.detach().cpu().numpy().astype(np.float64)
        err = float((np.abs(got - want[k]) / np.maximum(1.0, np.abs(want[k]))).max())
        top = float(np.abs(want[k]).max())
        print(f'{k}: {got.size} elements, max err {err:.3g} (bar {BAR:g}), max |ref| = {top:.3g}')
        assert np.isfinite(got).all() and err <= BAR, (k, err)
        if k == 'input_conv.0.bias':
            # a constant shift in front of a BatchNorm in batch-statistics mode changes nothing: this gradient is zero by mathematics
            # (rounding noise in both precisions), so it has no scale of its own to be held to
            assert top < 1e-12
            continue
        # the loss's 1 / size puts these gradients below one, where the bar is an absolute one: so also the same bar on the tensor's
        # own scale (float32's 6e-8 per rounding over chains of a few hundred terms and six layers stays orders below it)
        assert top > 0 and float(np.abs(got - want[k]).max()) <= BAR * top, (k, top)
    # train here, deploy on the inference layers
    deployed = _Net(base).to(dev)
    deployed.load_state_dict(net.state_dict(), strict=True)
    net.eval(); deployed.eval()
    with torch.no_grad():
        a = net(spconv.SparseConvTensor(_dev(x, dev), _dev(idx, dev), shape, batch))
        b = deployed(base.SparseConvTensor(_dev(x, dev), _dev(idx, dev), shape, batch))
    assert torch.equal(a, b)
    with pytest.raises(NotImplementedError):
        deployed(base.SparseConvTensor(_dev(x, dev), _dev(idx, dev), shape, batch))          # the inference layers still refuse gradients
