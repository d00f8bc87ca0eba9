"""The screened 128 -> 1024 layer's LDS layout: the tile's bf16 lo pieces are formed once per tile and kept in the region that
hosts hB during the front layers.  Three things are checked, each bit for bit:

1. cg_pointmlp_max_screened == cg_pointmlp_max at the smallest shapes where that image can go wrong: one and two screened tiles behind
   a workgroup's exact first tile (N = 128, 192: with two, a stale image of tile t could be read in tile t + 1), a one-point last tile
   (N = 65, 130), a workgroup whose first tile is not tile 0 (nsplit 2), N = 2048, and pointfeat of the MID == 2 pass.
2. The screen itself is what it was: the counters of `stats` (tiles screened / overflowed / out of range / first, pairs listed, and
   the bits of the worst |screen - exact| / bound) equal the ones the parent of this layout recorded on the same seeded inputs
   (tests/golden/screen_counters.json, written by tests/golden/make_golden_screen_counters.py).  Same hi, same lo, same product
   order, same listed set -- or a counter moves.
3. The reused region is dead while the image lives: consecutive tiles scaled by 2^8 and 2^-8 so that hB and the image differ
   strongly from tile to tile.

Every shape runs with B = 3 and with B = 260: three samples are few enough that the launcher takes the channel-split exact kernels
(the screened entry must still return the same bits), 260 is the smallest batch size the other screen tests use to reach the
throughput kernel, the one that holds the screen.  The counters are those of the B = 260 calls; the tests assert that it screened."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from catgrasp_amd import _lib as L
from catgrasp_amd import engine, folding, synth
from catgrasp_amd._lib import _p, _stream

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
_ci = ctypes.c_int
B_SMALL, B_BIG = 3, 260
GAINS = (1.6, 1.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'screen_counters.json')
COUNTERS = ('ST_SCREENED', 'ST_OVERFLOW', 'ST_RANGE', 'ST_FIRST', 'ST_PAIRS', 'ST_RATIO_bits')
_PASS = {0: ('stn', 'stn', None), 1: ('enc', 'fstn', 'fstn.wm'), 2: ('enc', 'enc', None)}      # mid -> (first layer, tag, mid weights)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to('cuda:0')


def call(D, x, mid, relu3, t3=None, t64=None, nsplit=1, force=None, stats=None, pointfeat=False):
    """force None: cg_pointmlp_max; else cg_pointmlp_max_screened.  -> uint32 view of the (B, 1024) output [, of pointfeat], on the host"""
    B, N, _ = x.shape
    out = torch.full((B, 1024), 777.0, dtype=torch.float32, device=x.device)
    pf = torch.full((B, N, 64), 777.0, dtype=torch.float32, device=x.device) if pointfeat else None
    head = (_p(x), _ci(B), _ci(N), _p(t3), _p(D['w1']), _p(D['b1']), _ci(mid), _p(D['wm'] if mid == 1 else None),
            _p(D['bm'] if mid == 1 else None), _p(t64 if mid == 2 else None), _p(D['w2']), _p(D['b2']), _p(D['w3']), _p(D['b3']),
            _ci(int(relu3)), _ci(nsplit), _p(out), _p(pf))
    if force is None:
        st = L.lib().cg_pointmlp_max(*head, _stream())
    else:
        st = L.lib().cg_pointmlp_max_screened(*head, _p(D['w3s']), _p(D['wn']), _p(stats), _ci(force), _stream())
    assert st == 0, st
    torch.cuda.synchronize()
    o = out.cpu().numpy().view(np.uint32)
    return (o, pf.cpu().numpy().view(np.uint32)) if pointfeat else o


def read_counters(stats):
    s = stats.cpu().numpy()
    return {'ST_SCREENED': int(s[0]), 'ST_OVERFLOW': int(s[1]), 'ST_RANGE': int(s[2]), 'ST_FIRST': int(s[3]), 'ST_PAIRS': int(s[4]),
            'ST_RATIO_bits': int(s[5])}


_NET = {}


def network(gain):
    """the bench's classifier (seeded weights) at `gain`: {mid: images of that pass}"""
    if gain not in _NET:
        W = folding.prepare_cls(synth.make_state_dict('cls', 6, 10, seed=0, gain=gain), torch.device('cuda:0'))
        _NET[gain] = {}
        for mid, (w1, tag, wm) in _PASS.items():
            _NET[gain][mid] = {'w1': W[w1 + '.w1'], 'b1': W[w1 + '.b1'], 'w2': W[tag + '.w2'], 'b2': W[tag + '.b2'], 'w3': W[tag + '.w3'],
                               'b3': W[tag + '.b3'], 'w3s': W[tag + '.w3'].screen[0], 'wn': W[tag + '.w3'].screen[1],
                               'wm': W[wm] if wm else None, 'bm': W[wm[:-3] + '.bm'] if wm else None}
        _NET[gain]['W'] = W
    return _NET[gain]


_IN = {}


def inputs():
    """seeded (260, 2048, 6) clouds with their (260, 9) input and (260, 64 x 64) feature transforms, built once"""
    if not _IN:
        rng = np.random.default_rng(20)
        f = lambda a: np.asarray(a, np.float32)
        _IN['x'] = _dev(f(rng.standard_normal((B_BIG, 2048, 6))))
        _IN['t3'] = _dev(f(np.eye(3).reshape(1, 9) + 0.1 * rng.standard_normal((B_BIG, 9))))
        _IN['t64'] = _dev(f(np.eye(64).reshape(1, 4096) + 0.05 * rng.standard_normal((B_BIG, 4096))))
    return _IN['x'], _IN['t3'], _IN['t64']


def shape_case(gain, mid, N, B=B_BIG):
    x, t3, t64 = inputs()
    return network(gain)[mid], x[:B, :N].contiguous(), (t3[:B].contiguous() if mid else None), t64[:B].contiguous()


def bench_like_case(gain, mid):
    """13 nut + 13 screw candidates x 10 (scripts/screen_survivors.py's inputs), transforms from the engine as the bench has them"""
    k = ('bench', gain)
    if 'bx' not in _IN:
        from oracle import transforms_ref as tref
        xs = []
        for kind in ('nut', 'screw'):
            objs = synth.make_scene(4, 2500, seed=0, kind=kind)
            rng = np.random.default_rng(3)
            one = []
            for i in range(13):
                ob = objs[i % 4]
                pose = synth.make_candidates(ob, 1, rng)[0]
                ids = tref.draw_ids(len(ob['xyz']), 2048, rng)
                one.append(tref.grasp_transform(ob['xyz'].copy(), ob['normal'].copy(), pose, ids)['input'])
            xs.append(np.tile(np.stack(one), (10, 1, 1)))
        _IN['bx'] = _dev(np.concatenate(xs).astype(np.float32))
    x = _IN['bx']
    if k not in _IN:
        W = network(gain)['W']
        with engine.precision('f32'):
            t3 = engine.stn3d_forward(W, x)
            g = engine._point_pass(W, x, 'enc', 'fstn', True, None, mid='fstn.wm', t3=t3, mid_mode=1)
            t64 = engine._tnet_tail(W, 'fstn', g, 64, None)
        _IN[k] = (t3, t64)
    t3, t64 = _IN[k]
    return network(gain)[mid], x, (t3 if mid else None), t64


def same_bits(D, x, mid, relu3, t3, t64, what, nsplit=1, forces=(0, 2)):
    """the screened entry returns the exact entry's bits under every force, with the counters' launch and with the production one;
    -> {force: counters}"""
    ref = call(D, x, mid, relu3, t3, t64, nsplit)
    res = {}
    for force in forces:
        st = torch.zeros(8, dtype=torch.int64, device='cuda:0')
        got = call(D, x, mid, relu3, t3, t64, nsplit, force=force, stats=st)
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f'{what} force {force}: {len(bad)} outputs differ, first (sample, channel) {bad[0].tolist()}: ' \
                              f'{got[tuple(bad[0])]:#x} vs exact {ref[tuple(bad[0])]:#x}'
        assert np.array_equal(call(D, x, mid, relu3, t3, t64, nsplit, force=force), ref), f'{what} force {force} without counters'
        res[force] = read_counters(st)
    return res


# ------------------------------------------------------------------------------------------------ the counter cases (test 2)
def counter_cases():
    """{key: (case builder, relu3)} of every recorded case; the keys are those of tests/golden/screen_counters.json"""
    cases = {}
    for gain in GAINS:
        for mid in (0, 1, 2):
            for relu3 in (0, 1):
                cases[f'N192-gain{gain}-mid{mid}-relu{relu3}'] = (lambda g=gain, m=mid: shape_case(g, m, 192), mid, relu3)
            cases[f'N2048-gain{gain}-mid{mid}'] = (lambda g=gain, m=mid: shape_case(g, m, 2048), mid, int(mid != 2))
            cases[f'bench-gain{gain}-mid{mid}'] = (lambda g=gain, m=mid: bench_like_case(g, m), mid, int(mid != 2))
    return cases


def measure_counters(key):
    """-> {'force0': counters, 'force2': counters} of one counter case on the loaded library (the outputs' bits are checked on the way)"""
    make, mid, relu3 = counter_cases()[key]
    D, x, t3, t64 = make()
    res = same_bits(D, x, mid, relu3, t3, t64, key)
    return {f'force{f}': res[f] for f in (0, 2)}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)['cases']


@pytest.mark.parametrize('key', sorted(counter_cases()))
def test_counters_equal_the_recorded_ones(key):
    want = _golden()[key]
    got = measure_counters(key)
    print(key, got)
    assert got['force2']['ST_SCREENED'] > 0 and got['force0']['ST_SCREENED'] > 0, 'the screen did not run'
    for force in ('force0', 'force2'):
        for c in COUNTERS:
            assert got[force][c] == want[force][c], f'{key} {force} {c}: {got[force][c]} but the parent recorded {want[force][c]}'


# ------------------------------------------------------------------------------------------------------------ bits (test 1)
SHAPES = [(mid, relu3, N) for mid in (0, 1, 2) for relu3 in (0, 1) for N in (65, 128, 130, 192)] + [(mid, int(mid != 2), 2048) for mid in (0, 1, 2)]


@pytest.mark.parametrize('mid,relu3,N', SHAPES, ids=[f'mid{m}-relu{r}-N{n}' for m, r, n in SHAPES])
def test_screened_equals_exact_small_shapes(mid, relu3, N):
    ntiles = (N + 63) // 64
    for gain in GAINS:
        for B in (B_SMALL, B_BIG):
            D, x, t3, t64 = shape_case(gain, mid, N, B=B)
            res = same_bits(D, x, mid, relu3, t3, t64, f'gain {gain} mid {mid} relu3 {relu3} N {N} B {B}')
            if B == B_BIG:
                for force in (0, 2):
                    r = res[force]
                    assert r['ST_SCREENED'] + r['ST_OVERFLOW'] + r['ST_RANGE'] + r['ST_FIRST'] == B * ntiles, r
                assert res[0]['ST_FIRST'] == B and res[2]['ST_FIRST'] == 0
                if ntiles > 1:
                    assert res[0]['ST_SCREENED'] > 0, res[0]              # tiles behind the first did take the screen


def test_first_tile_is_not_tile_0():
    """nsplit 2 at N = 256: the second workgroup of a sample starts at tile 2, and screens tile 3"""
    for gain in GAINS:
        for B in (B_SMALL, B_BIG):
            D, x, t3, t64 = shape_case(gain, 1, 256, B=B)
            res = same_bits(D, x, 1, 1, t3, t64, f'gain {gain} nsplit 2 B {B}', nsplit=2)
            if B == B_BIG:
                assert res[0]['ST_FIRST'] == 2 * B and res[0]['ST_SCREENED'] + res[0]['ST_OVERFLOW'] + res[0]['ST_RANGE'] == 2 * B
                assert res[0]['ST_SCREENED'] > 0


def test_pointfeat_is_not_disturbed():
    """MID == 2 with pointfeat requested: the mid layer's output leaves through registers, the image in hB's place must not show"""
    for gain in GAINS:
        for B in (B_SMALL, B_BIG):
            D, x, t3, t64 = shape_case(gain, 2, 192, B=B)
            ref, pf_ref = call(D, x, 2, 0, t3, t64, pointfeat=True)
            for force in (0, 2):
                got, pf = call(D, x, 2, 0, t3, t64, force=force, pointfeat=True)
                assert np.array_equal(got, ref), f'gain {gain} B {B} force {force}: outputs'
                assert np.array_equal(pf, pf_ref), f'gain {gain} B {B} force {force}: pointfeat'


# ------------------------------------------------------------------------------------------------ the region is dead (test 3)
@pytest.mark.parametrize('mid', [0, 1, 2])
def test_alternating_tile_scales(mid):
    """even tiles scaled by 2^8, odd tiles by 2^-8 (N = 256): whatever a tile left in the reused region differs by orders of
    magnitude from what the next one needs there"""
    for gain in GAINS:
        for B in (B_SMALL, B_BIG):
            D, x, t3, t64 = shape_case(gain, mid, 256, B=B)
            scale = torch.tensor([2.0 ** 8, 2.0 ** -8] * 2, device=x.device).repeat_interleave(64).view(1, 256, 1)
            xs = (x * scale).contiguous()
            for relu3 in (0, 1):
                res = same_bits(D, xs, mid, relu3, t3, t64, f'alternating gain {gain} mid {mid} relu3 {relu3} B {B}', forces=(0, 2, 1))
                if B == B_BIG:
                    assert res[1]['ST_SCREENED'] == 0 and res[2]['ST_SCREENED'] + res[2]['ST_OVERFLOW'] + res[2]['ST_RANGE'] == 4 * B
