"""CPU proof of tests/dense_train_ref.py, the yardstick of the dense layers' gradients and of PointNetSeg's head in training mode:
  * its float64 formulas equal torch autograd (float64) through F.linear + F.batch_norm(training=True) + relu;
  * the split first layer equals the unsplit Conv1d on the concatenated (B, Cg + Cp, N) tensor;
  * every planted variant of the float32 restatements differs from the restatement on at least one case -- otherwise the bitwise GPU
    tests could not tell them apart."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_ref
import dense_train_ref as R

TIGHT = 1e-11


def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


@pytest.mark.parametrize('n,cin,cout,rpg', [(6, 8, 4, 3), (65, 40, 12, 13), (130, 16, 300, 65)])
def test_linear_and_group_bias_grads_equal_torch_autograd(n, cin, cout, rpg):
    c = R.dense_case(n, cin, cout)
    x, w = _t(c['x'], True), _t(c['w'], True)
    b, rb = _t(np.zeros(cout), True), _t(np.zeros((n // rpg, cout)), True)
    y = F.linear(x, w, b) + rb.repeat_interleave(rpg, 0)
    y.backward(_t(c['dy']))
    assert R.rel_err(x.grad.numpy(), c['dx64']) < TIGHT
    assert R.rel_err(w.grad.numpy(), c['dw64']) < TIGHT
    assert R.rel_err(b.grad.numpy(), c['db64']) < TIGHT
    assert R.rel_err(rb.grad.numpy(), R.group_sums64(c['dy'], rpg)) < TIGHT


@pytest.mark.parametrize('B,N', [(1, 2), (2, 33), (3, 65)])
def test_head_equals_torch_autograd_through_the_unsplit_conv1d(B, N):
    """The reference's form: Conv1d over the (B, Cg + Cp, N) concatenation of g repeated over the points and the per-point features,
    BatchNorm1d with batch statistics, relu -- against the split first layer and the explicit gradients of the yardstick."""
    c = R.head_case(B, N)
    P = {k: _t(v, True) for k, v in c['P'].items()}
    g, pf = _t(c['g'], True), _t(c['pf'], True)
    h = torch.cat([g.unsqueeze(2).expand(-1, -1, N), pf.transpose(1, 2)], 1)
    for i in (1, 2, 3):
        z = F.conv1d(h, P[f'w{i}'].unsqueeze(2), P[f'b{i}'])
        h = F.relu(F.batch_norm(z, None, None, P[f'gamma{i}'], P[f'beta{i}'], training=True, eps=bn_ref.EPS))
    logits = F.conv1d(h, P['w4'].unsqueeze(2), P['b4']).permute(0, 2, 1)
    assert R.rel_err(logits.detach().numpy(), c['rec']['logits']) < TIGHT
    logits.backward(_t(c['dlogits']))
    got = dict(g=g.grad, pf=pf.grad, **{k: v.grad for k, v in P.items()})
    assert set(got) == set(c['grads'])
    for k, v in got.items():
        assert R.rel_err(v.numpy(), c['grads'][k]) < 1e-9, k
    for i in (1, 2, 3):          # no pre-activation near the ReLU edge: the nudge worked
        assert np.abs(c['rec'][f'pre{i}']).min() >= bn_ref.MARGIN


def test_restatements_agree_with_float64_and_read_the_header():
    assert R.ROWS % 64 == 0 and R.ROWS >= 64
    c = R.dense_case(R.ROWS + 1, 8, 4)
    assert R.rel_err(c['dw32'], c['dw64']) < R.BAR and R.rel_err(c['db32'], c['db64']) < R.BAR and R.rel_err(c['dx32'], c['dx64']) < R.BAR
    dy = R.dy_for(3 * 65, 12)
    assert R.rel_err(R.group_sums_exact(dy, 65), R.group_sums64(dy, 65)) < R.BAR
    assert R.dgrad_order(8) == [0, 4, 1, 5, 2, 6, 3, 7]
    assert R.dgrad_order(12) == [0, 4, 1, 5, 2, 6, 3, 7, 8, 9, 10, 11]
    assert sorted(R.dgrad_order(300)) == list(range(300)) and R.dgrad_order(300)[-4:] == [296, 297, 298, 299]


def test_the_fast_chain_step_is_dense_refs_fmaf():
    """fmaf_step on float32 values held in float64 equals dense_ref.fmaf bit for bit: random values, exact float32 midpoints (where
    the double rounding would go wrong), subnormal results, and whole chains against dense_ref.fma_chain."""
    rng = np.random.default_rng(5)
    a = rng.normal(0, 1, 200000).astype(np.float32)
    b = rng.normal(0, 1, 200000).astype(np.float32)
    c = (rng.normal(0, 1, 200000) * 10.0 ** rng.integers(-8, 3, 200000)).astype(np.float32)
    # a * b + c = (1 + 2^-23) + 2^-24 - 2^-70: just below the midpoint of 1 + 2^-23 (odd) and 1 + 2^-22; float64 rounds the sum onto the
    # midpoint itself, and a second rounding to nearest even would then go up
    a[:4] = np.float32(2.0 ** -24 * (1 + 2.0 ** -23)); b[:4] = np.float32(1 - 2.0 ** -23); c[:4] = np.float32(1 + 2.0 ** -23)
    naive = (a[:4].astype(np.float64) * b[:4] + c[:4]).astype(np.float32)
    assert (naive != R.fmaf(a[:4], b[:4], c[:4])).all()
    a[4:8] = np.float32(2.0 ** -70); b[4:8] = np.float32(1.5 * 2.0 ** -70); c[4:8] = np.float32(2.0 ** -140)          # subnormal result
    for lo in (0, 8):
        sl = slice(lo, None)
        want = R.fmaf(a[sl], b[sl], c[sl])
        got = R.fmaf_step(a[sl].astype(np.float64), b[sl].astype(np.float64), c[sl].astype(np.float64)).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    x, w = rng.normal(0, 1, (9, 300)).astype(np.float32), rng.normal(0, 1, (300, 24)).astype(np.float32)
    order = R.dgrad_order(300)
    assert np.array_equal(R.dgrad_exact(x, w).view(np.uint32), R.fma_chain(x, np.ascontiguousarray(w.T), order).view(np.uint32))


def _differs(a, b):
    return not np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def test_every_planted_variant_differs_from_the_restatement():
    c = R.dense_case(2 * R.ROWS + 1, 8, 4)
    flat = R.wgrad_exact(c['x'], c['dy'], rows=2 * R.ROWS + 1)
    desc = R.wgrad_exact(c['x'], c['dy'], descending=True)
    assert _differs(flat[0], c['dw32']) and _differs(flat[1], c['db32'])
    assert _differs(desc[0], c['dw32']) and _differs(desc[1], c['db32'])
    dy = R.dy_for(3 * 65, 12)
    assert _differs(R.group_sums_exact(dy, 65, global_tree=True), R.group_sums_exact(dy, 65))
    assert not _differs(R.group_sums_exact(dy[:128], 64, global_tree=True), R.group_sums_exact(dy[:128], 64))      # aligned groups: the same tree
    c = R.dense_case(33, 40, 300)
    assert _differs(R.dgrad_exact(c['dy'], c['w'], order=list(range(300))), c['dx32'])                                # ascending columns
