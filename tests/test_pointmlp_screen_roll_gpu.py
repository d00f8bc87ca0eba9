"""The screened 128 -> 1024 layer as a rolling pipeline over a wave's eight 32-channel blocks: the products of block
k + 1 run beside the select of block k, on two ping-ponged accumulator pairs and one linear weight stream per wave.  What can go wrong
there is an index, not a number: a select that reads the other accumulator pair, the `wn` / `rmax` entries or the masks of the wrong
block, a weight fragment fetched across a block edge, a first block selected before its products exist, a last block never selected,
a mask or a lower bound carried from one tile into the next.  Each test makes such a slip change the listed set by orders of magnitude:

1. Per-block scales.  The rows of a pass's folded 128 -> 1024 weights, and its bias, are multiplied by a power of two per 32-channel
   block, 2^(3 (b mod 8) - 12) and the reverse order, before packing: every block of a wave then lives 2^3 away from its neighbours.
2. Only the first, or only the last, block of every wave at full scale; the others at 2^-20 (not zero: a dead block ties with itself
   and overflows the list).
3. Two screened tiles in a row (N = 192), the second the first scaled by 2^-8.

Every case compares cg_pointmlp_max_screened with cg_pointmlp_max bit for bit under force 0 and 2, with and without `stats`, for
B = 3 (the launcher takes the channel-split exact kernels) and B = 260 (the throughput kernel, which holds the screen), and the
counters of the B = 260 calls with the ones the parent of this pipeline recorded on the same inputs
(tests/golden/screen_roll_counters.json, written by tests/golden/make_golden_screen_roll_counters.py): the scales are powers of two,
so a schedule that keeps every screen value keeps every counter."""
import json
import os

import numpy as np
import pytest
import torch

import test_pointmlp_screen_layout_gpu as T
from catgrasp_amd import folding, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'screen_roll_counters.json')
SHAPES = (128, 192, 256)
_Q = {0: 'feat.stn.', 1: 'feat.fstn.', 2: 'feat.'}      # mid -> the pass's prefix in the classifier's state dict
BLOCK_SCALES = {
    'up': [2.0 ** (3 * (b % 8) - 12) for b in range(32)],
    'down': [2.0 ** (3 * (7 - b % 8) - 12) for b in range(32)],
    'first': [1.0 if b % 8 == 0 else 2.0 ** -20 for b in range(32)],
    'last': [1.0 if b % 8 == 7 else 2.0 ** -20 for b in range(32)],
}
_NET = {}


def scaled_network(gain, mid, scales):
    """the images of pass `mid` of the layout tests' classifier, the 128 -> 1024 layer's rows and bias scaled per 32-channel block"""
    k = (gain, mid, scales)
    if k not in _NET:
        sd = {n.replace('module.', ''): v for n, v in synth.make_state_dict('cls', 6, 10, seed=0, gain=gain).items()}
        w, b = folding.fold_bn(*folding._conv(sd, _Q[mid] + 'conv3'), folding._bn(sd, _Q[mid] + 'bn3'))
        s = np.repeat(np.asarray(BLOCK_SCALES[scales], np.float64), 32)
        w, b = w * s[:, None], b * s
        D = dict(T.network(gain)[mid])
        D['w3'] = T._dev(folding.pack_b(w))
        D['b3'] = T._dev(b.astype(np.float32))
        D['w3s'] = T._dev(folding.pack_b_split(w, 'bf16').view(np.int16))
        D['wn'] = T._dev(folding.screen_norms(w))
        _NET[k] = D
    return _NET[k]


def case(gain, mid, N, scales, B=T.B_BIG, repeat_tile=False):
    _, x, t3, t64 = T.shape_case(gain, mid, N, B=B)
    if repeat_tile:             # the last tile = the one before it, scaled by 2^-8
        x = x.clone()
        x[:, N - 64:] = x[:, N - 128:N - 64] * 2.0 ** -8
    return scaled_network(gain, mid, scales), x, t3, t64


def counter_cases():
    """{key: (case builder taking B, mid, relu3)} of every case; the keys are those of tests/golden/screen_roll_counters.json"""
    cases = {}
    for gain in T.GAINS:
        for mid in (0, 1, 2):
            for relu3 in (0, 1):
                for scales in ('up', 'down'):
                    for N in SHAPES:
                        cases[f'{scales}-N{N}-gain{gain}-mid{mid}-relu{relu3}'] = (
                            lambda B, g=gain, m=mid, n=N, s=scales: case(g, m, n, s, B), mid, relu3)
                for scales in ('first', 'last'):
                    cases[f'{scales}-N192-gain{gain}-mid{mid}-relu{relu3}'] = (
                        lambda B, g=gain, m=mid, s=scales: case(g, m, 192, s, B), mid, relu3)
                cases[f'repeat-N192-gain{gain}-mid{mid}-relu{relu3}'] = (
                    lambda B, g=gain, m=mid: case(g, m, 192, 'up', B, repeat_tile=True), mid, relu3)
    return cases


def measure_counters(key, B=T.B_BIG):
    """-> {'force0': counters, 'force2': counters} of one case on the loaded library (the outputs' bits are checked on the way)"""
    make, mid, relu3 = counter_cases()[key]
    D, x, t3, t64 = make(B)
    res = T.same_bits(D, x, mid, relu3, t3, t64, f'{key} B {B}')
    return {f'force{f}': res[f] for f in (0, 2)}


_GOLDEN = {}


def _golden():
    if not _GOLDEN:
        with open(GOLDEN) as f:
            _GOLDEN.update(json.load(f)['cases'])
    return _GOLDEN


def check(key):
    measure_counters(key, B=T.B_SMALL)
    got = measure_counters(key)
    print(key, got)
    want = _golden()[key]
    ntiles = int(key.split('-')[1][1:]) // 64
    assert got['force0']['ST_FIRST'] == T.B_BIG and got['force2']['ST_FIRST'] == 0, got
    for force in ('force0', 'force2'):
        r = got[force]
        assert r['ST_SCREENED'] > 0, f'{key} {force}: the screen did not run'
        assert r['ST_SCREENED'] + r['ST_OVERFLOW'] + r['ST_RANGE'] + r['ST_FIRST'] == T.B_BIG * ntiles, r
        for c in T.COUNTERS:
            assert r[c] == want[force][c], f'{key} {force} {c}: {r[c]} but the parent recorded {want[force][c]}'


def _keys(*kinds):
    return sorted(k for k in counter_cases() if k.split('-')[0] in kinds)


@pytest.mark.parametrize('key', _keys('up', 'down'))
def test_per_block_scales(key):
    check(key)


@pytest.mark.parametrize('key', _keys('first', 'last'))
def test_first_and_last_block_alone(key):
    """only block 0 (or only block 7) of every wave at full scale: the fill must not select before the first block's products, and the
    drain must select the last block"""
    check(key)


@pytest.mark.parametrize('key', _keys('repeat'))
def test_no_state_crosses_tiles(key):
    """two screened tiles in a row, the second the first scaled by 2^-8: masks or a lower bound left over from tile t would list
    nothing, or everything, in tile t + 1"""
    check(key)
