"""GPU tests of the dense layers' gradients (catgrasp_amd/dense_autograd.py, csrc/dense_train.hip) and of BatchNorm + ReLU at the widths
of PointNetSeg's head: per element within 1e-4 * max(1, |ref|) of float64 AND the bits of the float32 restatements of
tests/dense_train_ref.py / tests/bn_ref.py (proved on the CPU by tests/test_dense_train_ref_cpu.py and tests/test_bn_ref_cpu.py)."""
import numpy as np
import pytest
import torch
from torch import nn

import bn_ref as B
import dense_train_ref as R
from catgrasp_amd import batchnorm, dense_autograd as D
from dense_ref import check_bitwise

pytestmark = pytest.mark.gpu

ROWS = R.ROWS
N_ROWS = [1, 2, 31, 32, 33, 63, 64, 65, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1]
SHAPES = [(8, 4), (8, 32), (64, 36), (40, 300), (128, 300), (256, 128)]      # (Cin, Cout)
WIDE = [(3, 1024, 512), (65, 512, 256)]                                        # (n, Cin, Cout)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _bar(got, want, what):
    err = R.rel_err(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, want)
    print(f'{what}: {err:.3e} of the bar {R.BAR:.0e}')
    assert err <= R.BAR, (what, err)


def _check_dense(n, cin, cout, device):
    c = R.dense_case(n, cin, cout)
    x, w, dy = (_dev(c[k], device) for k in ('x', 'w', 'dy'))
    dw, db = D.dense_wgrad(x, dy)
    dx = D.dense_dgrad(dy, w)
    tag = f'n={n} cin={cin} cout={cout}'
    for got, k in ((dw, 'dw'), (db, 'db'), (dx, 'dx')):
        _bar(got, c[k + '64'], f'{k} {tag}')
        check_bitwise(got.cpu().numpy(), c[k + '32'], f'{k} {tag}')
    only_w, none_b = D.dense_wgrad(x, dy, need_bias=False)
    none_w, only_b = D.dense_wgrad(x, dy, need_weight=False)
    assert none_b is None and none_w is None and torch.equal(only_w, dw) and torch.equal(only_b, db)


@pytest.mark.parametrize('cin,cout', SHAPES, ids=[f'{a}x{b}' for a, b in SHAPES])
@pytest.mark.parametrize('n', N_ROWS)
def test_weight_bias_and_input_gradients(n, cin, cout, cuda_device):
    _check_dense(n, cin, cout, cuda_device)


@pytest.mark.parametrize('n,cin,cout', WIDE, ids=[f'n{n}-{a}x{b}' for n, a, b in WIDE])
def test_the_widest_layers(n, cin, cout, cuda_device):
    _check_dense(n, cin, cout, cuda_device)


@pytest.mark.parametrize('groups', [1, 2, 3])
@pytest.mark.parametrize('rpg', [1, 63, 64, 65, 1025])
def test_group_sums(rpg, groups, cuda_device):
    for c in (12, 300):
        dy = R.dy_for(groups * rpg, c, seed=rpg + groups)
        got = D.group_sums(_dev(dy, cuda_device), rpg).cpu().numpy()
        _bar(got, R.group_sums64(dy, rpg), f'group sums rpg={rpg} groups={groups} c={c}')
        check_bitwise(got, R.group_sums_exact(dy, rpg), f'group sums rpg={rpg} groups={groups} c={c}')


@pytest.mark.parametrize('cin,cout,rpg,groups', [(16, 12, 33, 2), (64, 36, 65, 3), (8, 300, 1, 5)])
def test_forward_has_the_bits_of_the_mfma_chain_and_matches_float64(cin, cout, rpg, groups, cuda_device):
    """linear / linear_group_bias forward: cg_gemm_bias_act with the weight packed on the device."""
    n = rpg * groups
    c = R.dense_case(n, cin, cout)
    rng = np.random.default_rng(n)
    bias, rb = rng.uniform(-1, 1, cout).astype(np.float32), rng.uniform(-1, 1, (groups, cout)).astype(np.float32)
    x, w = _dev(c['x'], cuda_device), _dev(c['w'], cuda_device)
    y = D.linear_group_bias(x, w, _dev(bias, cuda_device), _dev(rb, cuda_device), rpg).cpu().numpy()
    want = c['x'].astype(np.float64) @ c['w'].astype(np.float64).T + bias + np.repeat(rb.astype(np.float64), rpg, 0)
    _bar(y, want, f'forward {cin}x{cout}')
    emu = R.gemm_f32_epilogue(R.fma_chain(c['x'], c['w']), np.arange(cout), np.arange(n), bias=bias, row_bias=rb, rows_per_group=rpg)
    check_bitwise(y, emu, f'forward {cin}x{cout}')
    from catgrasp_amd import folding
    assert torch.equal(D.pack_b(w).cpu(), torch.from_numpy(folding.pack_b(c['w'])))


BN_CASES = [(2, 240), (65, 256), (1025, 512), (2049, 128)]


@pytest.mark.parametrize('n,c', BN_CASES, ids=[f'n{n}-c{c}' for n, c in BN_CASES])
def test_wide_batchnorm_has_the_bits_of_the_restatement(n, c, cuda_device):
    r = B.case(n, c)
    x, gamma, beta, dy = (_dev(r[k], cuda_device) for k in ('x', 'gamma', 'beta', 'dy'))
    if c > batchnorm.MAX_C:
        assert batchnorm._entry(c, None)[1] == 'cg_bn_relu_train_forward_wide'
    y, stats = batchnorm.bn_relu_forward(x, gamma, beta, B.EPS)
    dx, dgamma, dbeta = batchnorm.bn_relu_backward(x, dy, stats)
    tag = f'bn n={n} c={c}'
    for got, k32, want64 in ((y, r['f32']['y'], r['f64']['y']), (stats[0], r['f32']['mean'], r['f64']['mean']), (stats[1], r['f32']['var'], r['f64']['var']),
                             (dx, r['dx32'], r['dx64']), (dgamma, r['dgamma32'], r['dgamma64']), (dbeta, r['dbeta32'], r['dbeta64'])):
        _bar(got, want64, tag)
        check_bitwise(got.cpu().numpy(), k32, tag)
    bn = nn.BatchNorm1d(c, eps=B.EPS).to(cuda_device).train()       # the module path takes the width too
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
    assert torch.equal(batchnorm.bn_relu_train(x, bn), y) and int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize('c', [16, 224])
def test_wide_entry_points_return_the_bits_of_the_narrow_ones(c, cuda_device):
    r = B.case(1025, c)
    x, gamma, beta, dy = (_dev(r[k], cuda_device) for k in ('x', 'gamma', 'beta', 'dy'))
    narrow = batchnorm.bn_relu_forward(x, gamma, beta, B.EPS, wide=False)
    wide = batchnorm.bn_relu_forward(x, gamma, beta, B.EPS, wide=True)
    assert torch.equal(narrow[0], wide[0]) and torch.equal(narrow[1], wide[1])
    for a, b in zip(batchnorm.bn_relu_backward(x, dy, narrow[1], wide=False), batchnorm.bn_relu_backward(x, dy, wide[1], wide=True)):
        assert torch.equal(a, b)


def _layer_grads(c, device, rpg):
    x, w, dy = (_dev(c[k], device) for k in ('x', 'w', 'dy'))
    x.requires_grad_(True); w.requires_grad_(True)
    b = torch.zeros(w.shape[0], device=device, requires_grad=True)
    rb = torch.zeros((x.shape[0] // rpg, w.shape[0]), device=device, requires_grad=True)
    D.linear_group_bias(x, w, b, rb, rpg).backward(dy)
    return x.grad, w.grad, b.grad, rb.grad


def test_autograd_is_reproducible_and_the_same_on_a_side_stream(cuda_device):
    c = R.dense_case(2 * ROWS + 1, 64, 36)
    first = _layer_grads(c, cuda_device, 683)
    again = _layer_grads(c, cuda_device, 683)
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        other = _layer_grads(c, cuda_device, 683)
    side.synchronize()
    for a, b, o in zip(first, again, other):
        assert torch.equal(a, b) and torch.equal(a, o)
    check_bitwise(first[0].cpu().numpy(), c['dx32'], 'dx through autograd')
    check_bitwise(first[1].cpu().numpy(), c['dw32'], 'dw through autograd')
    check_bitwise(first[2].cpu().numpy(), c['db32'], 'db through autograd')
    check_bitwise(first[3].cpu().numpy(), R.group_sums_exact(c['dy'], 683), 'group sums through autograd')


def test_only_the_gradients_asked_for_are_computed(cuda_device, monkeypatch):
    calls = []
    real_w, real_d, real_g = D.dense_wgrad, D.dense_dgrad, D.group_sums
    monkeypatch.setattr(D, 'dense_wgrad', lambda *a: calls.append(('w',) + tuple(a[2:])) or real_w(*a))
    monkeypatch.setattr(D, 'dense_dgrad', lambda *a: calls.append(('d',)) or real_d(*a))
    monkeypatch.setattr(D, 'group_sums', lambda *a: calls.append(('g',)) or real_g(*a))
    c = R.dense_case(65, 64, 36)
    x, w, dy = (_dev(c[k], cuda_device) for k in ('x', 'w', 'dy'))
    b = torch.zeros(36, device=cuda_device)
    rb = torch.zeros((5, 36), device=cuda_device)

    def run(**need):
        del calls[:]
        t = dict(x=x.clone().requires_grad_(need.get('x', False)), w=w.clone().requires_grad_(need.get('w', False)),
                 b=b.clone().requires_grad_(need.get('b', False)), rb=rb.clone().requires_grad_(need.get('rb', False)))
        D.linear_group_bias(t['x'], t['w'], t['b'], t['rb'], 13).backward(dy)
        for k, v in t.items():
            assert (v.grad is not None) == need.get(k, False), k
        return list(calls)

    assert run(x=True) == [('d',)]
    assert run(w=True) == [('w', True, False)]
    assert run(b=True) == [('w', False, True)]
    assert run(rb=True) == [('g',)]
    assert run(x=True, w=True, b=True, rb=True) == [('d',), ('w', True, True), ('g',)]
    assert not D.linear(x, w, b).requires_grad


def test_refusals_come_before_any_device_work(cuda_device):
    x, w = torch.zeros((4, 8), device=cuda_device), torch.zeros((4, 8), device=cuda_device)
    with pytest.raises(NotImplementedError, match='float32'):
        D.linear(x.double(), w.double())
    with pytest.raises(NotImplementedError, match='multiple of 8'):
        D.linear(torch.zeros((4, 12), device=cuda_device), torch.zeros((4, 12), device=cuda_device))
    with pytest.raises(NotImplementedError, match='multiple of 4'):
        D.linear(x, torch.zeros((6, 8), device=cuda_device))
    with pytest.raises(ValueError):
        D.linear_group_bias(x, w, None, torch.zeros((3, 4), device=cuda_device), 3)
    ctx = type('ctx', (), dict(saved_tensors=(None,) * 2, needs_input_grad=(True,) * 5, rows_per_group=1))()
    with pytest.raises(NotImplementedError, match='float32'):
        D.DenseFunction.backward(ctx, torch.zeros((4, 4), device=cuda_device, dtype=torch.float64))
