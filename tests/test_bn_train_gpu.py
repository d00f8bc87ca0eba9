"""GPU tests of BatchNorm in batch-statistics mode + ReLU (catgrasp_amd/batchnorm.py, csrc/batchnorm_train.hip).

Yardstick: tests/bn_ref.py -- the float64 formulas (pinned against torch autograd by tests/test_bn_ref_cpu.py) and the float32
restatement of the header's chains.  Every output is per element within 1e-4 * max(1, |ref|) of float64, the project's bar, and has the
bits of the restatement.  The inputs keep every float64 pre-activation at least 1e-3 from zero, so both precisions agree on every
ReLU mask and no element is left out.

Shapes: two and three rows, the widest layer, the segment boundary (63, 64, 65 rows), the chunk boundary (1023, 1024, 1025) and 2049
rows: two whole chunks, a chunk of one row and the cross-chunk pass."""
import numpy as np
import pytest
import torch
from torch import nn

import bn_ref as B
from catgrasp_amd import _lib, batchnorm

pytestmark = pytest.mark.gpu

BAR = 1e-4
SHAPES = [(2, 16), (3, 16), (2, 224), (63, 16), (64, 16), (65, 32), (1023, 16), (1024, 48), (1025, 224), (2049, 112)]
STATS = ('mean', 'var', 'invstd', 'scale', 'shift')


def _dev(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


def _run(r, dev, need_dx=True):
    """-> dict of numpy results of one forward + backward through the raw wrappers."""
    x, gamma, beta, dy = (_dev(r[k], dev) for k in ('x', 'gamma', 'beta', 'dy'))
    y, stats = batchnorm.bn_relu_forward(x, gamma, beta, B.EPS)
    assert stats.shape == (5, x.shape[1])
    mean, var, invstd, scale, shift = stats.unbind(0)
    dx, dgamma, dbeta = batchnorm.bn_relu_backward(x, dy, stats, need_dx=need_dx)
    out = dict(y=y, mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, dx=dx, dgamma=dgamma, dbeta=dbeta)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _bits_equal(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    same = got.view(np.uint32) == want.view(np.uint32)
    if not same.all():
        i = np.unravel_index(np.argmin(same), same.shape)
        raise AssertionError(f'{what}: {int((~same).sum())} of {same.size} elements differ in their bits; first at {i}: got {got[i]!r}, model {want[i]!r}')
    assert np.isfinite(want).all(), what


@pytest.mark.parametrize('n,c', SHAPES)
def test_forward_and_backward_against_float64_and_the_stated_chains(n, c, cuda_device):
    r = B.case(n, c)
    got = _run(r, cuda_device)
    want64 = dict(r['f64'], dx=r['dx64'], dgamma=r['dgamma64'], dbeta=r['dbeta64'])
    want32 = dict(r['f32'], dx=r['dx32'], dgamma=r['dgamma32'], dbeta=r['dbeta32'])
    errs = {k: B.rel_err(got[k], want64[k]) for k in ('y',) + STATS + ('dx', 'dgamma', 'dbeta')}
    print(f'({n}, {c}): max |got - ref| / max(1, |ref|): ' + ', '.join(f'{k} {v:.3g}' for k, v in errs.items()) + f' (bar {BAR:g})')
    for k, err in errs.items():
        assert np.isfinite(got[k]).all() and err <= BAR, (k, err)
    for k in errs:
        _bits_equal(got[k], want32[k], f'({n}, {c}) {k}')
    # run to run, and on a side stream
    again = _run(r, cuda_device)
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        other = _run(r, cuda_device)
    side.synchronize()
    for k in errs:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) and np.array_equal(got[k].view(np.uint32), other[k].view(np.uint32)), k


def test_the_chunking_is_there_to_be_seen(cuda_device):
    r = B.case(2049, 112)
    got = _run(r, cuda_device)
    flat = B.forward32(r['x'], r['gamma'], r['beta'], flat=True)
    assert (flat['mean'].view(np.uint32) != got['mean'].view(np.uint32)).any()
    fused = B.forward32(r['x'], r['gamma'], r['beta'], contract=True)
    assert (fused['y'].view(np.uint32) != got['y'].view(np.uint32)).mean() > 0.01


def test_a_constant_column_gives_finite_results_with_the_restatements_bits(cuda_device):
    r = B.case(65, 32, constant=True)
    got = _run(r, cuda_device)
    assert got['var'][1] < 1e-12 and got['invstd'][1] > 100
    want32 = dict(r['f32'], dx=r['dx32'], dgamma=r['dgamma32'], dbeta=r['dbeta32'])
    for k in ('y',) + STATS + ('dx', 'dgamma', 'dbeta'):
        assert np.isfinite(got[k]).all(), k
        _bits_equal(got[k], want32[k], 'constant column ' + k)


@pytest.mark.parametrize('n,c', [(65, 32), (2049, 112)])
def test_module_step_updates_the_running_statistics_as_torch_does(n, c, cuda_device):
    r = B.case(n, c)
    rng = np.random.default_rng(9)
    start_mean, start_var = rng.uniform(-1, 1, c).astype(np.float32), rng.uniform(0.5, 2, c).astype(np.float32)

    def make(dtype, dev):
        bn = nn.BatchNorm1d(c, eps=B.EPS, momentum=0.1).to(dtype)
        with torch.no_grad():
            bn.weight.copy_(torch.from_numpy(np.array(r['gamma']))); bn.bias.copy_(torch.from_numpy(np.array(r['beta'])))
            bn.running_mean.copy_(torch.from_numpy(start_mean)); bn.running_var.copy_(torch.from_numpy(start_var))
        return bn.to(dev).train()

    ours, theirs = make(torch.float32, cuda_device), make(torch.float64, 'cpu')
    x = _dev(r['x'], cuda_device).requires_grad_(True)
    y = batchnorm.bn_relu_train(x, ours)
    y.backward(_dev(r['dy'], cuda_device))
    x64 = torch.from_numpy(np.array(r['x'])).double().requires_grad_(True)
    y64 = torch.relu(theirs(x64))
    y64.backward(torch.from_numpy(np.array(r['dy'])).double())
    pairs = [('y', y, y64), ('dx', x.grad, x64.grad), ('dgamma', ours.weight.grad, theirs.weight.grad), ('dbeta', ours.bias.grad, theirs.bias.grad),
             ('running_mean', ours.running_mean, theirs.running_mean), ('running_var', ours.running_var, theirs.running_var)]
    for what, a, b in pairs:
        err = B.rel_err(a.detach().cpu().numpy(), b.detach().numpy())
        print(f'({n}, {c}) {what}: {err:.3g} (bar {BAR:g})')
        assert err <= BAR, (what, err)
    assert int(ours.num_batches_tracked) == int(theirs.num_batches_tracked) == 1
    assert ours.num_batches_tracked.dtype == torch.int64
    _bits_equal(y.detach().cpu().numpy(), r['f32']['y'], 'module y')
    _bits_equal(x.grad.cpu().numpy(), r['dx32'], 'module dx')


def test_only_the_gradients_asked_for_are_computed(cuda_device, monkeypatch):
    r = B.case(65, 32)
    lib = _lib.lib()
    real = lib.cg_bn_relu_train_backward
    calls = []

    def counted(*a):
        calls.append(bool(a[11].value))                          # whether dx is given
        return real(*a)
    monkeypatch.setattr(lib, 'cg_bn_relu_train_backward', counted)
    dy = _dev(r['dy'], cuda_device)

    def run(need_x, need_gamma, need_beta):
        del calls[:]
        bn = nn.BatchNorm1d(32, eps=B.EPS).to(cuda_device).train()
        with torch.no_grad():
            bn.weight.copy_(_dev(r['gamma'], cuda_device)); bn.bias.copy_(_dev(r['beta'], cuda_device))
        bn.weight.requires_grad_(need_gamma); bn.bias.requires_grad_(need_beta)
        x = _dev(r['x'], cuda_device).requires_grad_(need_x)
        batchnorm.bn_relu_train(x, bn).backward(dy)
        return x.grad, bn.weight.grad, bn.bias.grad, list(calls)

    dx, dgamma, dbeta, seen = run(True, True, True)
    assert seen == [True]
    _bits_equal(dx.cpu().numpy(), r['dx32'], 'dx'); _bits_equal(dgamma.cpu().numpy(), r['dgamma32'], 'dgamma'); _bits_equal(dbeta.cpu().numpy(), r['dbeta32'], 'dbeta')
    fx, fg, fb, seen = run(False, True, True)                    # a detached input: dx NULL, the statistics' gradients unchanged
    assert seen == [False] and fx is None and torch.equal(fg, dgamma) and torch.equal(fb, dbeta)
    fx, fg, fb, seen = run(True, False, False)                   # frozen gamma and beta: dx still needs both sums
    assert seen == [True] and fg is None and fb is None and torch.equal(fx, dx)
    fx, fg, fb, seen = run(False, True, False)
    assert seen == [False] and fx is None and fb is None and torch.equal(fg, dgamma)
    # a non-contiguous gradient is made contiguous; another precision is refused
    bn = nn.BatchNorm1d(32, eps=B.EPS).to(cuda_device).train()
    with torch.no_grad():
        bn.weight.copy_(_dev(r['gamma'], cuda_device)); bn.bias.copy_(_dev(r['beta'], cuda_device))
    x = _dev(r['x'], cuda_device).requires_grad_(True)
    wide = torch.zeros((65, 64), device=cuda_device)
    wide[:, ::2] = dy
    batchnorm.bn_relu_train(x, bn).backward(wide[:, ::2])
    assert torch.equal(x.grad, dx)
    with pytest.raises(NotImplementedError, match='float32'):
        batchnorm.BatchNormReLUFunction.backward(type('ctx', (), dict(saved_tensors=(None,) * 2, needs_input_grad=(True,) * 4))(), dy.double(), None)


def test_one_row_and_unbuilt_widths_raise(cuda_device):
    bn = nn.BatchNorm1d(16).to(cuda_device).train()
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        batchnorm.bn_relu_train(torch.zeros((1, 16), device=cuda_device), bn)
    assert int(bn.num_batches_tracked) == 0
    with pytest.raises(NotImplementedError, match='multiples of 16'):
        batchnorm.bn_relu_train(torch.zeros((4, 8), device=cuda_device), nn.BatchNorm1d(8).to(cuda_device).train())
    with pytest.raises(NotImplementedError):
        batchnorm.bn_relu_train(torch.zeros((4, 16), device=cuda_device, dtype=torch.float64), bn)
