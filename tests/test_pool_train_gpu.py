"""GPU tests of the closed-form training of PointNet's pooled layer (catgrasp_amd/pool_autograd.py, csrc/pool_train.hip): the extrema are
the bits of the dense forward on the same device, every value is within dense_train_ref.BAR of float64 per element (nothing masked
out), and the layer is reproducible, sparse in memory and refuses what it does not build.  The yardstick is tests/pool_train_ref.py,
proved on the CPU by tests/test_pool_train_ref_cpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import pool_train_ref as P
from catgrasp_amd import dense_autograd as D, pool_autograd as PA
from dense_ref import check_bitwise

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 8, 32), (3, 31, 8, 32), (3, 33, 64, 96), (2, 64, 128, 128), (2, 65, 128, 1024), (1, 1025, 8, 32), (2, 1025, 8, 32)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
VALUE_CASES = [(*s, relu, 0.0) for s in SHAPES for relu in (True, False)] + [(3, 33, 64, 96, True, 8.0), (2, 1025, 8, 32, False, 8.0)]


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _modules(k, device):
    c, cin = k['w'].shape
    conv, bn = nn.Conv1d(cin, c, 1), nn.BatchNorm1d(c, eps=P.EPS)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(k['w']).unsqueeze(2)); conv.bias.copy_(torch.from_numpy(k['b']))
        bn.weight.copy_(torch.from_numpy(k['gamma'])); bn.bias.copy_(torch.from_numpy(k['beta']))
        bn.running_mean.normal_(generator=torch.Generator().manual_seed(1)); bn.running_var.uniform_(0.5, 2, generator=torch.Generator().manual_seed(2))
    return conv.to(device).train(), bn.to(device).train()


@pytest.mark.parametrize('B,N,cin,c', SHAPES, ids=IDS)
def test_extrema_are_the_bits_of_the_dense_forward_and_the_first_index(B, N, cin, c, cuda_device):
    k = P.case(B, N, cin, c, True)
    x, w, b, gamma = (_dev(k[n], cuda_device) for n in ('x', 'w', 'b', 'gamma'))
    zsel, idx = PA.pool_extrema(x, w, b, gamma)
    z = D.dense_forward(x.view(B * N, cin), w, b).view(B, N, c)
    pos = gamma >= 0
    vmax, vmin = z.max(dim=1)[0], z.min(dim=1)[0]
    want = torch.where(pos[None, :], vmax, vmin)
    assert zsel.dtype == torch.float32 and idx.dtype == torch.int32 and torch.equal(zsel, want)
    n_idx = torch.arange(N, device=cuda_device)[None, :, None].expand(B, N, c)
    first = torch.where(z == want[:, None, :], n_idx, torch.full_like(n_idx, N)).min(dim=1)[0]
    assert torch.equal(idx.long(), first)
    # all max / all min, and no sign vector (max)
    assert torch.equal(PA.pool_extrema(x, w, b, None)[0], vmax) and torch.equal(PA.pool_extrema(x, w, b, -torch.ones_like(gamma))[0], vmin)
    if k['pair']:
        assert int(idx[0, 2]) == k['pair'][1] < k['pair'][2] and torch.equal(x[0, k['pair'][1]], x[0, k['pair'][2]])      # the planted tie
    if (B, N, cin, c) in SHAPES[:2]:                                # the CPU restatement
        assert np.array_equal(zsel.cpu().numpy().view(np.uint32), k['zsel32'].view(np.uint32)) and np.array_equal(idx.cpu().numpy(), k['idx'])
    else:
        assert np.array_equal(idx.cpu().numpy(), k['idx'])        # the same z bits give the same indices


def _run(k, device, need=('x', 'w', 'b', 'gamma', 'beta')):
    conv, bn = _modules(k, device)
    for name, p in (('w', conv.weight), ('b', conv.bias), ('gamma', bn.weight), ('beta', bn.bias)):
        p.requires_grad_(name in need)
    x = _dev(k['x'], device).requires_grad_('x' in need)
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    out = PA.conv_bn_max_train(x, conv, bn, k['relu'])
    out.backward(_dev(k['dout'], device))
    return out.detach(), dict(x=x.grad, w=None if conv.weight.grad is None else conv.weight.grad.squeeze(2), b=conv.bias.grad, gamma=bn.weight.grad,
                              beta=bn.bias.grad), bn, (rm, rv)


@pytest.mark.parametrize('B,N,cin,c,relu,offset', VALUE_CASES, ids=['-'.join(map(str, v)) for v in VALUE_CASES])
def test_output_statistics_and_every_gradient_match_float64(B, N, cin, c, relu, offset, cuda_device):
    k = P.case(B, N, cin, c, relu, offset)
    out, grads, bn, (rm, rv) = _run(k, cuda_device)
    f64, m = k['f64'], B * N
    x, w, b, gamma, beta = (_dev(k[n], cuda_device) for n in ('x', 'w', 'b', 'gamma', 'beta'))
    xbar, s = PA.centred_gram(x.view(m, cin))
    zsel, idx = PA.pool_extrema(x, w, b, gamma)
    mean = PA.pool_mean(w, b, xbar, B, N)
    var = PA.pool_var(x, w, b, mean)
    stats, out2 = PA.pool_stats(w, b, xbar, None, gamma, beta, P.EPS, N, zsel, relu, var=var)
    assert torch.equal(out, out2) and np.array_equal(idx.cpu().numpy(), k['idx']) and torch.equal(stats[0], mean) and torch.equal(stats[1], var)
    gram = PA.pool_stats(w, b, xbar, s, gamma, beta, P.EPS, N, zsel, relu)[0]              # the route through S: same mean, its own var
    assert torch.equal(gram[0], mean)
    rel = lambda v: float((np.abs(v.cpu().numpy() - f64['var']) / f64['var']).max())
    print(f'  kappa up to {P.kappa(f64).max():.3g}; relative error of var: sweep {rel(var):.2e}, Gram route {rel(gram[1]):.2e}')
    assert rel(var) <= P.BAR
    mom = bn.momentum
    err = {'out': P.rel_err(out.cpu().numpy(), f64['out']), 'mean': P.rel_err(stats[0].cpu().numpy(), f64['mean']),
           'var': P.rel_err(stats[1].cpu().numpy(), f64['var']),
           'running_mean': P.rel_err(bn.running_mean.cpu().numpy(), (1 - mom) * rm.cpu().double().numpy() + mom * f64['mean']),
           'running_var': P.rel_err(bn.running_var.cpu().numpy(), (1 - mom) * rv.cpu().double().numpy() + mom * f64['var'] * m / (m - 1))}
    for name, want in k['grads'].items():
        assert grads[name] is not None and grads[name].shape == want.shape, name
        err['d' + name] = P.rel_err(grads[name].cpu().numpy(), want)         # every element: nothing is masked out
    print(f'pool {B}x{N}x{cin}x{c} relu={relu} offset={offset}: ' + ', '.join(f'{n} {e:.2e}' for n, e in err.items()))
    assert int(bn.num_batches_tracked) == 1 and not grads['b'].any()         # the conv bias gradient is exactly 0
    assert max(err.values()) <= P.BAR, err
    # gamma == 0: out = act(beta), a zero row of dW
    assert torch.equal(out[:, 1], (torch.relu(beta[1]) if relu else beta[1]).expand(B)) and not grads['w'][1].any()


@pytest.mark.parametrize('B,N,cin,c', SHAPES[:3], ids=IDS[:3])
def test_gather_and_scatter_have_the_bits_of_their_stated_chains(B, N, cin, c, cuda_device):
    """cg_pool_wgrad_gather: one fmaf chain over b ascending; cg_pool_dgrad_scatter: per row fmaf(coef, W[c], dx) in ascending c, rows
    shared by several channels of a cloud included (every case has them: N < C)."""
    k = P.case(B, N, cin, c, True)
    rng = np.random.default_rng(B * N + c)
    coef = rng.uniform(-1, 1, (B, c)).astype(np.float32)
    dx0 = rng.normal(0, 1, (B, N, cin)).astype(np.float32)
    assert any(len(set(r)) < len(r) for r in k['idx'].tolist())
    x, w, idx = _dev(k['x'], cuda_device), _dev(k['w'], cuda_device), _dev(k['idx'], cuda_device)
    t = PA.pool_wgrad_gather(x, _dev(coef, cuda_device), idx)
    check_bitwise(t.cpu().numpy(), P.gather_exact(k['x'], coef, k['idx']), 'gather')
    dx = PA.pool_dgrad_scatter(_dev(dx0, cuda_device), _dev(coef, cuda_device), idx, w)
    check_bitwise(dx.cpu().numpy(), P.scatter_exact(dx0, coef, k['idx'], k['w']), 'scatter')
    for bad in (coef[:, :-1], coef[:1]):
        with pytest.raises(ValueError):
            PA.pool_wgrad_gather(x, _dev(bad, cuda_device), idx)
    with pytest.raises(ValueError):
        PA.pool_extrema(x, w[:, :-8].contiguous())


def test_only_the_gradients_asked_for_are_computed(cuda_device):
    k = P.case(3, 33, 64, 96, True)
    full = _run(k, cuda_device)[1]
    no_x = _run(k, cuda_device, need=('w', 'b', 'gamma', 'beta'))[1]
    no_w = _run(k, cuda_device, need=('x', 'gamma'))[1]
    assert no_x['x'] is None and no_w['w'] is None and no_w['b'] is None and no_w['beta'] is None
    for name in ('w', 'b', 'gamma', 'beta'):
        assert torch.equal(no_x[name], full[name]), name
    assert torch.equal(no_w['x'], full['x']) and torch.equal(no_w['gamma'], full['gamma'])


def test_two_runs_and_a_side_stream_give_the_same_bits(cuda_device):
    k = P.case(2, 1025, 8, 32, True)
    first, again = _run(k, cuda_device), _run(k, cuda_device)
    side = torch.cuda.Stream(device=cuda_device)
    side.wait_stream(torch.cuda.current_stream(cuda_device))
    with torch.cuda.stream(side):
        other = _run(k, cuda_device)
    side.synchronize()
    for r in (again, other):
        assert torch.equal(first[0], r[0])
        for name in first[1]:
            assert torch.equal(first[1][name], r[1][name]), name


def _composite(x, conv, bn, relu):
    y = bn(conv(x.transpose(1, 2)))
    return (F.relu(y) if relu else y).max(dim=2)[0]


def test_peak_allocation_stays_below_one_dense_activation(cuda_device):
    B, N, cin, c = 4, 4096, 128, 1024
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, N, cin), generator=g).to(cuda_device).requires_grad_(True)
    conv, bn = nn.Conv1d(cin, c, 1).to(cuda_device).train(), nn.BatchNorm1d(c).to(cuda_device).train()
    dout = torch.randn((B, c), generator=g).to(cuda_device)
    peaks = {}
    for name, fn in (('closed form', lambda: PA.conv_bn_max_train(x, conv, bn, True)), ('torch composite', lambda: _composite(x, conv, bn, True))):
        for p in (x, *conv.parameters(), *bn.parameters()):
            p.grad = None
        torch.cuda.synchronize(cuda_device)
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(cuda_device)
        base = torch.cuda.memory_allocated(cuda_device)
        fn().backward(dout)
        torch.cuda.synchronize(cuda_device)
        peaks[name] = torch.cuda.max_memory_allocated(cuda_device) - base
    dense = B * N * c * 4
    print(f'peak allocation above the inputs, forward + backward at {(B, N, cin, c)}: ' + ', '.join(f'{n} {p / 2 ** 20:.1f} MiB' for n, p in peaks.items())
          + f'; one dense activation {dense / 2 ** 20:.0f} MiB')
    assert peaks['closed form'] < dense


def test_refusals(cuda_device):
    k = P.case(3, 33, 64, 96, True)
    conv, bn = _modules(k, cuda_device)
    x = _dev(k['x'], cuda_device)
    with pytest.raises(NotImplementedError, match='HIP device'):
        PA.conv_bn_max_train(x.cpu(), conv, bn, True)
    with pytest.raises(NotImplementedError, match='float32'):
        PA.conv_bn_max_train(x.double(), conv, bn, True)
    for cin, c in ((12, 96), (64, 48)):
        with pytest.raises(NotImplementedError, match='multiple of'):
            PA.conv_bn_max_train(torch.zeros((2, 5, cin), device=cuda_device), nn.Conv1d(cin, c, 1).to(cuda_device), nn.BatchNorm1d(c).to(cuda_device).train(), True)
    with pytest.raises(ValueError, match='training mode'):
        PA.conv_bn_max_train(x, conv, nn.BatchNorm1d(96).to(cuda_device).eval(), True)
    with pytest.raises(ValueError, match='Expected more than 1 value per channel when training'):
        PA.conv_bn_max_train(x[:1, :1].contiguous(), conv, bn, True)
    assert int(bn.num_batches_tracked) == 0
    out = PA.conv_bn_max_train(x, conv, bn, True)
    out.sum().backward()
    with pytest.raises(RuntimeError, match='second time'):
        out.sum().backward()
    xg = x.clone().requires_grad_(True)
    first, = torch.autograd.grad(PA.conv_bn_max_train(xg, conv, bn, True).sum(), xg, create_graph=True)
    with pytest.raises(RuntimeError):          # once differentiable: there is no double backward
        first.sum().backward()
