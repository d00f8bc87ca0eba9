"""Pins the yardstick tests/sparse_ref.py: its rule-book restatement of the three sparse convolution layers equals dense float64
torch convolutions to 1e-12 on the scenes that tests/test_sparse_conv_gpu.py uses, with and without the BatchNorm/ReLU prologue
(applied to the sparse rows, then densified) and the residual.  No GPU, no catgrasp_amd code."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sparse_ref as ref

SCENES = [dict(n=299), dict(n=1, special=False), dict(n=33, special=False), dict(n=301, seed=5), dict(n=120, special=False, only_item=1)]
IDS = ['full299', 'n1', 'n33', 'n301', 'empty_item0']
CIN, COUT = 6, 5


def _setup(kw, k):
    idx = ref.scene(**kw)
    x = ref.features(len(idx), CIN).astype(np.float64)
    w, b = ref.weights(k, CIN, COUT)
    return idx, x, w.astype(np.float64), b.astype(np.float64)


def _variants(n_out):
    scale, shift = ref.bn_params(CIN)
    res = np.random.default_rng(9).uniform(-1, 1, (n_out, COUT))
    return [(None, None, None), (scale, shift, None), (None, None, res), (scale, shift, res)]


def _pro(x, scale, shift):
    return x if scale is None else np.maximum(x * scale.astype(np.float64) + shift.astype(np.float64), 0.0)


def _at(dense_out, idx):
    return dense_out[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]]


def test_the_full_scene_holds_every_trap():
    idx = ref.scene()
    sites = {tuple(r) for r in idx.tolist()}
    assert len(idx) == 299 and len(sites) == 299 and idx.dtype == np.int32
    assert {(0, 0, 0, 0), (1, 8, 11, 16), (0, 3, 4, 16), (0, 3, 5, 0), (0, 5, 6, 7), (1, 5, 6, 7)} <= sites
    nbr = ref.subm_rules(idx, ref.SHAPE)
    row = {tuple(r): i for i, r in enumerate(idx.tolist())}
    assert (nbr[row[(1, 2, 9, 3)]] >= 0).sum() == 1                              # isolated: only itself
    assert (nbr[row[(0, 2, 2, 11)]] >= 0).all()                                  # centre of the full block
    assert row[(0, 3, 5, 0)] not in nbr[row[(0, 3, 4, 16)]] and row[(1, 5, 6, 7)] not in nbr[row[(0, 5, 6, 7)]]
    assert (nbr[:, 13] == np.arange(299)).all()
    _, _, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
    assert out_shape == (4, 6, 8) and 6 <= dropped.sum() < 150
    assert sorted(set(idx[:, 0].tolist())) == [0, 1]
    assert not np.array_equal(idx, idx[np.argsort(ref.linear_key(idx, ref.SHAPE))])          # the rows are not in key order


@pytest.mark.parametrize('kw', SCENES, ids=IDS)
def test_subm_equals_dense_conv3d(kw):
    idx, x, w, b = _setup(kw, 3)
    nbr = ref.subm_rules(idx, ref.SHAPE)
    wt = torch.from_numpy(w).permute(4, 3, 0, 1, 2).contiguous()
    for scale, shift, res in _variants(len(idx)):
        got = ref.conv(x, nbr, w, b, scale, shift, res)
        want = _at(F.conv3d(torch.from_numpy(ref.dense(idx, _pro(x, scale, shift), ref.BATCH, ref.SHAPE)), wt, torch.from_numpy(b), padding=1).numpy(), idx)
        want = want + (0 if res is None else res)
        assert np.abs(got - want).max() <= 1e-12


def test_subm_k1_is_a_matrix_product():
    idx, x, w, b = _setup(dict(n=299), 1)
    got = ref.conv(x, np.arange(len(idx), dtype=np.int32)[:, None], w, b)
    assert np.abs(got - (x @ w.reshape(CIN, COUT) + b)).max() <= 1e-12


@pytest.mark.parametrize('kw', SCENES, ids=IDS)
def test_down_equals_dense_strided_conv3d(kw):
    idx, x, w, b = _setup(kw, 2)
    out_idx, nbr, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
    assert out_shape == (4, 6, 8)
    keys = ref.linear_key(out_idx, out_shape)
    assert (np.diff(keys) > 0).all()
    used = np.zeros(len(idx), bool); used[nbr[nbr >= 0]] = True
    assert np.array_equal(used, ~dropped) and (nbr >= 0).sum() == (~dropped).sum()
    wt = torch.from_numpy(w).permute(4, 3, 0, 1, 2).contiguous()
    for scale, shift, res in _variants(len(out_idx)):
        got = ref.conv(x, nbr, w, b, scale, shift, res)
        full = F.conv3d(torch.from_numpy(ref.dense(idx, _pro(x, scale, shift), ref.BATCH, ref.SHAPE)), wt, None, stride=2).numpy()
        assert full.shape[2:] == out_shape
        if len(out_idx):
            want = _at(full, out_idx) + b + (0 if res is None else res)
            assert np.abs(got - want).max() <= 1e-12
        active = np.zeros((ref.BATCH,) + out_shape, bool)
        active[out_idx[:, 0], out_idx[:, 1], out_idx[:, 2], out_idx[:, 3]] = True
        assert np.abs(np.moveaxis(full, 1, -1)[~active]).max(initial=0.0) == 0.0          # no output site is missing


@pytest.mark.parametrize('kw', SCENES, ids=IDS)
def test_inverse_equals_dense_conv_transpose3d(kw):
    idx, _, w, b = _setup(kw, 2)
    w = np.ascontiguousarray(np.swapaxes(w, 3, 4))          # this layer's own Cin -> Cout: COUT channels in, CIN out
    b = ref.weights(2, COUT, CIN, seed=4)[1].astype(np.float64)
    out_idx, _, out_shape, dropped = ref.down_rules(idx, ref.SHAPE)
    nbr = ref.inverse_rules(idx, out_idx, ref.SHAPE)
    assert np.array_equal((nbr >= 0).sum(1), (~dropped).astype(int))
    y = np.random.default_rng(8).uniform(-1, 1, (len(out_idx), COUT))
    wt = torch.from_numpy(w).permute(3, 4, 0, 1, 2).contiguous()
    scale, shift = ref.bn_params(COUT)
    res = np.random.default_rng(9).uniform(-1, 1, (len(idx), CIN))
    for sc, sh, r in [(None, None, None), (scale, shift, None), (None, None, res), (scale, shift, res)]:
        got = ref.conv(y, nbr, w, b, sc, sh, r)
        up = F.conv_transpose3d(torch.from_numpy(ref.dense(out_idx, _pro(y, sc, sh), ref.BATCH, out_shape)), wt, None, stride=2).numpy()
        full = np.zeros((ref.BATCH, CIN) + ref.SHAPE)
        full[:, :, :up.shape[2], :up.shape[3], :up.shape[4]] = up          # zero-padded up to the fine shape
        want = _at(full, idx) + b + (0 if r is None else r)
        assert np.abs(got - want).max() <= 1e-12
        if r is None and dropped.any():
            assert np.array_equal(got[dropped], np.broadcast_to(b, (dropped.sum(), CIN)))          # a dropped site gets the bias only
