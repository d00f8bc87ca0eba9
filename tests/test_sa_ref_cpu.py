"""CPU proofs about tests/sa_ref.py and the cases of tests/test_sa_kernels_gpu.py: the reference is the oracle's function, every
exact case is exact in float32, and the scenes are sensitive to what the GPU module is meant to catch."""
import numpy as np
import pytest
import torch

import dense_ref as dr
import sa_ref as R
import test_sa_kernels_gpu as G
from oracle import setabstraction_ref as sref

BEACON_CASES = [c for c in G.EXACT_CASES if c['lists'] == 'beacon']
RANDOM_CASES = [c for c in G.EXACT_CASES if c['lists'] == 'random']


def _ref(sc, layers=None, idx=None):
    return R.sa_ref(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'] if idx is None else idx, sc['layers'] if layers is None else layers)


@pytest.mark.parametrize('B,N,S,K,D,widths,group_all', [(2, 50, 5, 7, 6, [64, 64, 128], False), (1, 40, 3, 33, 29, [96, 32], False),
                                                         (2, 37, 1, 37, 4, [32, 64], True)])
def test_sa_ref_is_the_oracle_in_float64_and_bounds_the_float32_chain(B, N, S, K, D, widths, group_all):
    sc = R.general_scene(B, N, S, K, D, widths, seed=11 + K, group_all=group_all)
    x = torch.from_numpy(R.grouped(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx']))
    layers = [tuple(torch.from_numpy(np.asarray(t, np.float64)) for t in (w, b) + bn) for w, b, bn in sc['raw']]
    want = sref.mlp_max(x, layers, dtype=torch.float64).numpy()
    got = _ref(sc, layers=sc['folded64'])
    assert got.shape == want.shape == (B, 1 if group_all else S, widths[-1])
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the float32 torch chain on the float32 inputs and folded float32 weights, coordinates centred in float32
    x32 = torch.from_numpy(sc['xyz'])
    bi = torch.arange(B)[:, None, None]
    if group_all:
        h = torch.cat([x32[:, None], torch.from_numpy(sc['points'])[:, None]], dim=-1)
    else:
        idx = torch.from_numpy(sc['idx'])
        h = torch.cat([x32[bi, idx] - torch.from_numpy(sc['new_xyz'])[:, :, None], torch.from_numpy(sc['points'])[bi, idx]], dim=-1)
    for w, b in sc['layers']:
        h = torch.relu(h @ torch.from_numpy(w).t() + torch.from_numpy(b))
    ref, bound = R.sa_bound(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers'])
    worst = dr.check_bound(h.max(dim=2)[0].numpy(), ref, bound, 'float32 torch chain')
    assert 0 < worst <= 1
    # gamma_n of the magnitude sums, propagated through the layers: a float32 rounding bound, not a loose one
    assert float((bound / np.maximum(np.abs(ref), 1e-30)).min()) < 1e-3


def test_every_exact_case_is_exact_in_float32():
    """exactness_margin < 1 for every exact case of the GPU module: 0 cases left out."""
    worst, at = 0.0, None
    for c in G.EXACT_CASES:
        sc = G.scene_of(c)
        m = R.exactness_margin(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers'])
        assert m < 1, (c['id'], m)
        ref = _ref(sc)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), c['id']
        if m > worst:
            worst, at = m, c['id']
    print(f'{len(G.EXACT_CASES)} exact cases, 0 left out; worst exactness margin {worst:.4f} ({at})')


def test_the_margin_is_below_one_for_the_widest_network_the_kernels_accept():
    sc = R.exact_scene(1, 64, 2, 8, 589, [512, 512, 512, 1024], seed=5)
    assert R.exactness_margin(sc['xyz'], sc['points'], sc['new_xyz'], sc['idx'], sc['layers']) < 1
    with pytest.raises(AssertionError):
        R.exactness_margin(sc['xyz'] + 1.0 / 16, sc['points'], sc['new_xyz'], sc['idx'], sc['layers'])


def test_beacon_scenes_fail_when_the_beacon_row_is_lost():
    """Replacing row g mod K by the base point every other row holds (row 0, unless the beacon sits there) changes EVERY output
    channel of neighbourhood g, for every g; and over the G >= K neighbourhoods every row position is the beacon's once."""
    assert BEACON_CASES
    for c in BEACON_CASES:
        sc = G.scene_of(c)
        idx = sc['idx']
        B, S, K = idx.shape
        h = c['N'] // 2
        pos = np.arange(B * S).reshape(B, S) % K
        assert B * S >= K and set(pos.ravel()) == set(range(K)), c['id']
        is_beacon = idx >= h
        assert np.array_equal(is_beacon, np.arange(K)[None, None, :] == pos[:, :, None]), c['id']
        lost = np.where(is_beacon, idx - h, idx)
        other = (pos + 1) % K
        if K > 1:
            assert np.array_equal(lost[np.arange(B)[:, None], np.arange(S)[None, :], pos], idx[np.arange(B)[:, None], np.arange(S)[None, :], other])
        full, without = _ref(sc), _ref(sc, idx=lost)
        assert bool((full > without).all()), c['id']


def test_random_scenes_hide_little_behind_relu_and_see_the_column_order():
    assert RANDOM_CASES
    for c in RANDOM_CASES:
        sc = G.scene_of(c)
        ref = _ref(sc)
        assert (ref > 0).mean() >= 0.95, (c['id'], (ref > 0).mean())
        w0, b0 = sc['layers'][0]
        i, j = 0, w0.shape[1] - 1
        if np.array_equal(w0[:, i], w0[:, j]):
            i = 1
        sw = w0.copy()
        sw[:, [i, j]] = sw[:, [j, i]]
        assert not np.array_equal(_ref(sc, layers=[(sw, b0)] + sc['layers'][1:]), ref), c['id']


def test_case_lists_cover_what_they_claim():
    assert len(G.REG_SIG) == 39 * 3 and {tuple(c['widths']) for c in G.REG_SIG} == {tuple(s) for s in G.REG_SIGNATURES}
    hidden = sorted(w for c in G.TILE_WAVE for w in c['widths'][:-1])
    assert hidden == [32, 64, 96, 128, 160, 288, 512] and sorted(c['widths'][-1] for c in G.TILE_WAVE) == [32, 160, 288, 1024]
    assert {(3 + c['D']) % 8 for c in G.TILE_D} == set(range(8))
    for n_cu in (256, 304, 64):
        for c in G.TILE_128:
            g = c['G'](n_cu)
            use128 = (g * 2 if c['K'] == 129 else -(-g // 16)) >= 2 * n_cu
            assert use128 == c['id'].endswith('-at'), (c['id'], n_cu)
