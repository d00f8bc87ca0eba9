"""The five kernels of csrc/primitives.hip (square_distance_kernel, square_distance_nd_kernel, index_points_kernel, ball_query_kernel,
group_points_kernel) against the plain float64 references of tests/group_ref.py, at every edge of their own geometry, through
catgrasp_amd.primitives.

Exact scenes (coordinates k/64, features integers over 8: tests/test_group_ref_cpu.py proves exactness_margin < 1 for every case
here) are held to equality with the float64 result: the library is built without FMA contraction and every partial sum of the
-2ab + a^2 + b^2 expansion is a float32 number, so there is no rounding band -- not for a distance, and not for the membership of a
ball.  General values are held per element to group_ref.sqdist_bound; the general ball scenes carry an r^2 that every (query, point)
pair clears by more than that bound, so every row equals ball_ref and none is excused.  Gathers are compared as bit patterns.

Which case reaches which code:
  sq-B*-N*-M*        square_distance_kernel: N below / at / past SQ_ROWS = 16 and two row tiles + 1 (the `rows = min(...)` clamp, the
                     srow[r] a row reads), M below / at / past the 256-thread block and two blocks + 1 (`m >= M`), the batch offsets
  nd-C*              square_distance_nd_kernel: C = 1 (no loop trip), 2, 4, 5, 8, 64, 131; N = 17, M = 257 take the same edges
  nd-C3-is-tiled     C = 3 through cg_square_distance_nd is cg_square_distance, bit for bit
  ip-C*-*            index_points_kernel: B S C just below / at / past one 256-thread block for (B,S) and (B,S,K) indices; indices
                     0 and N - 1, heavy duplication, special bit patterns; the error flag from the first and the very last element
  n{N}               ball_query_kernel: clouds of 1 / 63 / 64 / 65 points (the clamped tail lanes of the only chunk), 511 / 512 / 513
                     (the last chunk of a BQ_U = 8 trip, a second trip of one point), 1025 (a third trip); point N - 1 is a hit and
                     must be counted once although every clamped lane reloads it
  s{S}               1, 3, 4, 5 queries: a partial workgroup, a full one, a second one (`q >= S`)
  fill-lane63 / fill-lane0 / fill-511 / fill-512
                     the nsample-th hit in the last lane of a chunk, in the first lane of the next, at the end of a trip and at the
                     start of the next (`count < nsample` in the trip loop, `count >= nsample` in the chunk loop); the hit right
                     after it must not appear
  more-than-slots    40 hits in a chunk with 10 / 6 slots free (`pos < nsample`);  all64-ns1: a full ballot with one slot
  count-past-32      40 / 50 hits in one chunk and free slots behind them: the next chunk's hits start at `count` = all of them
  last-trip          the first hit beyond point 1024;  few: only N - 1, only 0, nothing (N in every slot)
  one-hit-ns64/65/70 the padding loop `k += 64`: 63 pads (one trip, lane 63 idle), 64 pads (one full trip), 69 pads (a second trip)
  ns-gt-n            nsample = 64 > N = 50: 50 columns
  boundary-eq        points at d == r^2 exactly are members, points one lattice step further (|o|^2 = 10 against 9) are not
  radius0            r = 0: the coincident points are members (d == 0 is not > 0), a neighbour one step away is not
  nextafter-lo / -hi r = nextafter(1/8, 0) and nextafter(1/8, inf): r^2 rounds to 1/64 in float32 either way and the points at
                     d == 1/64 are members (the reference compares in float32)
  shared             two queries at one place get the same row;  nan: a point with a NaN coordinate is in every ball
  gap-*              general values: 700 and 2000 points (two and four trips), balls that fill early, late and not at all
  group-D*-K*        group_points_kernel: D = 0 (points == NULL), 1, 5, 13; K = 1, 16, 33; totals just past one block; random,
                     all-same and all-(N - 1) index arrays; grouped_xyz requested or not; feature bit patterns; idx == N and -1"""
import functools
import zlib

import numpy as np
import pytest
import torch

import group_ref as R

pytestmark = pytest.mark.gpu


def _seed(name):
    return zlib.crc32(name.encode()) & 0xffff


def _dev(a, dev, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _bits(t):
    """A float32 tensor / array as int32 bit patterns (numpy)."""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.int32)


def _poison(dev, nbytes):
    """Leave a freed block of the size the next output takes, filled with -7s: an element the kernel fails to write reads as
    0xf9f9f9f9... (a NaN, a negative index), not as whatever an earlier, correct call left there."""
    if nbytes:
        t = torch.full((nbytes,), 0xf9, dtype=torch.uint8, device=dev)
        del t


# --------------------------------------------------------------------------------------------------------------- cases
SQ_CASES = [dict(id=f'sq-B{B}-N{N}-M{M}', B=B, N=N, M=M, C=3) for B in (1, 3) for N in (1, 15, 16, 17, 33) for M in (1, 255, 256, 257, 513)]
ND_CASES = [dict(id=f'nd-C{C}', B=2, N=17, M=257, C=C) for C in (1, 2, 4, 5, 8, 64, 131)]

# (C, B, rows per cloud): B S C = 255 / 256 / 257 where C divides them, else the nearest totals on either side of 256
IP_ROWS = [(1, 3, 85), (1, 2, 128), (1, 1, 257), (3, 5, 17), (3, 2, 43), (7, 2, 18), (7, 1, 37), (64, 3, 1), (64, 2, 2), (64, 5, 1)]
IP_SPLIT = {85: (17, 5), 128: (8, 16), 257: (257, 1), 17: (17, 1), 43: (43, 1), 18: (3, 6), 37: (37, 1), 1: (1, 1), 2: (1, 2)}
IP_CASES = [dict(id=f'ip-C{C}-{B}x{S}' + ('-bsk' if bsk else ''), C=C, B=B, shape=(B,) + (IP_SPLIT[S] if bsk else (S,)))
            for C, B, S in IP_ROWS for bsk in (False, True)]
IP_N = 23

R3 = 3.0 / 64               # the planted balls' radius: r^2 = 9 / 4096, a float32 number


def _ball(name, N, ns, hits, radius=R3, **scene):
    return dict(id=name, N=N, ns=ns, hits=hits, radius=radius, scene=dict(scene, seed=_seed(name)))


def _sweep(N):
    """Three queries.  Cloud 0: {0, N - 1} / nothing / three points inside; cloud 1: four other points inside / {0} / {N - 1}."""
    last = N - 1
    mid0 = sorted({i for i in (N // 5, N // 2, 4 * N // 5) if 0 < i < last})
    mid1 = sorted({i for i in (N // 7, N // 3, 5 * N // 7, last - 1) if 0 < i < last})
    return [[sorted({0, last}), [], mid0], [mid1, [0] if N > 1 else [], [last]]]


def _queries(S):
    """S queries on 130 points: two or three hits each, N - 1 in the last query's ball (cloud 0) or the first one's (cloud 1)."""
    return [[sorted({7 * q + b, 64 + q + 5 * b} | ({129} if q == (S - 1 if b == 0 else 0) else set())) for q in range(S)] for b in (0, 1)]


_r = lambda a, b: list(range(a, b))
BALL_CASES = (
    [_ball(f'n{N}', N, 8, _sweep(N)) for N in (1, 63, 64, 65, 511, 512, 513, 1025)]
    + [_ball(f's{S}', 130, 8, _queries(S)) for S in (1, 3, 4, 5)]
    + [_ball('fill-lane63', 200, 4, [[[5, 20, 40, 63, 64, 70], [1, 2, 3, 127, 128]], [[0, 61, 62, 63, 64], [60, 100, 126, 127, 128, 199]]]),
       _ball('fill-lane0', 200, 4, [[[5, 20, 40, 64, 65], [0, 63, 100, 128, 129]], [[61, 62, 63, 64, 65, 66], [7, 8, 9, 128, 130]]]),
       _ball('fill-511', 700, 3, [[[100, 300, 511, 512, 600], [10, 510, 699]], [[448, 510, 511, 512], [0, 1, 513]]]),
       _ball('fill-512', 700, 3, [[[100, 300, 512, 513], [2, 511, 699]], [[510, 511, 512, 513], [3, 4, 640]]]),
       _ball('more-than-slots', 200, 16, [[[3, 9, 17, 33, 41, 60] + _r(64, 104), []], [_r(20, 30) + _r(130, 170), [0, 199]]]),
       _ball('count-past-32', 200, 64, [[_r(64, 104) + [130, 150, 199], [5]], [_r(0, 50) + [64, 128], _r(70, 110) + [190]]]),
       _ball('all64-ns1', 192, 1, [[_r(64, 128), _r(0, 64)], [_r(128, 192), _r(64, 128)]]),
       _ball('last-trip', 1100, 8, [[[1030, 1050, 1099], [1024]], [[1025, 1087, 1088], [1099]]]),
       _ball('few', 130, 8, [[[129], [0], []], [[], [129], [0]]])]
    + [_ball(f'one-hit-ns{ns}', 200, ns, [[[37], [199]], [[0], [64]]]) for ns in (64, 65, 70)]
    + [_ball('ns-gt-n', 50, 64, [[[3, 10, 49], []], [[49], [0, 1, 2]]]),
       _ball('boundary-eq', 100, 16, [[[10, 20, 30, 40], [50]], [[1, 98], [0, 99]]],
             place=[{10: (0, (3, 0, 0)), 20: (0, (0, -3, 0)), 30: (0, (2, 2, 1)), 40: (0, (-1, 2, -2)), 50: (1, (0, 0, 3)),
                     11: (0, (3, 1, 0)), 21: (0, (0, -3, -1)), 31: (0, (2, 2, 2)), 41: (0, (4, 0, 0)), 5: (1, (0, 1, 3))},
                    {1: (0, (0, 3, 0)), 98: (0, (-2, -1, 2)), 0: (1, (-3, 0, 0)), 99: (1, (1, -2, 2)),
                     2: (0, (1, 3, 0)), 97: (0, (-2, -1, 3)), 50: (1, (-3, 0, -1)), 51: (1, (0, 0, -4))}]),
       _ball('radius0', 70, 4, [[[5, 66], []], [[], [69]]], radius=0.0, r2_steps=0,
             place=[{6: (0, (1, 0, 0)), 4: (0, (0, 0, -1))}, {0: (1, (0, 0, -1)), 68: (1, (0, 1, 0))}])]
    + [_ball(f'nextafter-{tag}', 100, 8, [[[10, 60], [20, 30, 70]], [[99], []]], radius=float(np.nextafter(0.125, to)), r2_steps=64, centre_dx=20,
             place=[{10: (0, (8, 0, 0)), 60: (0, (0, 0, -8)), 70: (1, (0, -8, 0)), 11: (0, (8, 1, 0)), 69: (1, (1, -8, 0))},
                    {99: (0, (-8, 0, 0)), 98: (0, (-8, 0, 1)), 0: (1, (0, 8, 1))}]) for tag, to in (('lo', 0.0), ('hi', np.inf))]
    + [_ball('shared', 130, 8, [[[4, 64, 129], [5], [4, 64, 129]], [[63], [0, 129], [63]]], shared=[(0, 2)]),
       _ball('nan', 100, 8, [[[10, 60], [50], []], [[5], [], [98]]], nan_at=[[40], [0, 99]])])
assert len({c['id'] for c in BALL_CASES}) == len(BALL_CASES)

# general values: (N, S, nsample, pool): pool None: the queries are cloud points 0 .. S - 1 (group_ref.general_ball_scene)
GAP_CASES = [dict(id=f'gap-N{N}-S{S}-ns{ns}', B=2, N=N, S=S, ns=ns, pool=pool, r=0.03) for N, S, ns, pool in ((700, 40, 16, None), (700, 40, 32, None),
                                                                                                           (2000, 100, 32, 200))]

GROUP_CASES = [dict(id=f'group-D{D}-K{K}', B=2, N=37, K=K, D=D, S=-(-257 // (2 * K * (3 + D)))) for D in (0, 1, 5, 13) for K in (1, 16, 33)]
GROUP_LISTS = ('random', 'same', 'last')


def sq_scene(case, exact):
    seed = _seed(case['id'])
    if exact:
        return R.exact_clouds(case['B'], case['N'], case['M'], case['C'], seed)
    return R.general_clouds(case['B'], case['N'], case['M'], case['C'], seed + 1) + (None,)


def ball_scene_of(case):
    hits = case['hits']
    kw = {k: v for k, v in case['scene'].items() if k != 'r2_steps'}
    return R.planted_scene(case['N'], hits, r2_steps=case['scene'].get('r2_steps', 9), **kw)


@functools.lru_cache(maxsize=None)
def _gap_scene(N, S, pool, r):
    return R.general_ball_scene(2, N, S, r, seed=11 + N, pool=pool)


def gap_scene_of(case):
    return _gap_scene(case['N'], case['S'], case['pool'], case['r'])


def group_scene_of(case):
    return R.group_scene(case['B'], case['N'], case['S'], case['K'], case['D'], _seed(case['id']))


def ip_scene_of(case):
    """points (B, 23, C) with special bit patterns in rows 0, 5 and N - 1; indices drawn from {0, N - 1, 5, 5, 5, any}."""
    rng = np.random.default_rng(_seed(case['id']))
    pts = R.with_payloads(rng.normal(size=(case['B'], IP_N, case['C'])), (0, 5, IP_N - 1))
    pick = np.array([0, IP_N - 1, 5, 5, 5, -1])[rng.integers(0, 6, case['shape'])]
    idx = np.where(pick < 0, rng.integers(0, IP_N, case['shape']), pick).astype(np.int64)
    flat = idx.reshape(-1)
    flat[0], flat[-1] = IP_N - 1, 0
    return pts, idx


# ----------------------------------------------------------------------------------------------------- square_distance
def _held_to_bound(got, src, dst, what):
    ref, bound = R.sqdist_ref(src, dst), R.sqdist_bound(src, dst)
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f'{what}: worst |error| / bound = {worst:.3f}')
    assert worst <= 1.0, what


@pytest.mark.parametrize('case', SQ_CASES + ND_CASES, ids=lambda c: c['id'])
def test_square_distance_exact_scenes_equal_float64_and_general_ones_keep_the_bound(cuda_device, case):
    from catgrasp_amd import primitives as prim
    shape = (case['B'], case['N'], case['M'])
    src, dst, _ = sq_scene(case, exact=True)
    _poison(cuda_device, 4 * int(np.prod(shape)))
    got = prim.square_distance(_dev(src, cuda_device), _dev(dst, cuda_device))
    ref = R.sqdist_ref(src, dst)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape
    assert torch.equal(got.cpu(), torch.from_numpy(ref.astype(np.float32))), case['id']
    src, dst, _ = sq_scene(case, exact=False)
    _poison(cuda_device, 4 * int(np.prod(shape)))
    _held_to_bound(prim.square_distance(_dev(src, cuda_device), _dev(dst, cuda_device)), src, dst, case['id'])


def test_square_distance_of_three_channels_through_the_generic_entry_is_the_tiled_kernel(cuda_device):
    from catgrasp_amd import _lib, primitives as prim
    src, dst = R.general_clouds(2, 17, 257, 3, seed=77)
    s, d = _dev(src, cuda_device), _dev(dst, cuda_device)
    tiled = torch.full((2, 17, 257), float('nan'), device=cuda_device)
    _lib.check(_lib.lib().cg_square_distance(_lib._p(s), _lib._p(d), 2, 17, 257, _lib._p(tiled), _lib._stream()), 'cg_square_distance')
    assert np.array_equal(_bits(prim.square_distance(s, d)), _bits(tiled))
    _held_to_bound(tiled, src, dst, 'nd-C3-is-tiled')


# -------------------------------------------------------------------------------------------------------- index_points
@pytest.mark.parametrize('case', IP_CASES, ids=lambda c: c['id'])
def test_index_points_returns_the_rows_bit_for_bit(cuda_device, case):
    from catgrasp_amd import primitives as prim
    pts, idx = ip_scene_of(case)
    _poison(cuda_device, 4 * idx.size * case['C'])
    got = prim.index_points(_dev(pts, cuda_device), _dev(idx, cuda_device, np.int64))
    assert got.dtype == torch.float32 and tuple(got.shape) == idx.shape + (case['C'],)
    assert np.array_equal(_bits(got), R.index_ref(_bits(pts), idx)), case['id']


@pytest.mark.parametrize('case', [c for c in IP_CASES if c['id'] in ('ip-C1-1x257', 'ip-C3-2x43-bsk', 'ip-C64-5x1')], ids=lambda c: c['id'])
def test_index_points_refuses_an_index_outside_the_cloud(cuda_device, case):
    from catgrasp_amd import primitives as prim
    pts, idx = ip_scene_of(case)
    p = _dev(pts, cuda_device)
    for bad in (IP_N, -1):
        for where in (0, idx.size // 2, idx.size - 1):            # the last one: the last slot of the last cloud
            i = idx.copy()
            i.reshape(-1)[where] = bad
            with pytest.raises(IndexError):
                prim.index_points(p, _dev(i, cuda_device, np.int64))
    prim.index_points(p, _dev(idx, cuda_device, np.int64))          # and the flag does not stick


# ---------------------------------------------------------------------------------------------------------- ball query
def _query(dev, radius, ns, xyz, new_xyz):
    from catgrasp_amd import primitives as prim
    B, N, S = xyz.shape[0], xyz.shape[1], new_xyz.shape[1]
    _poison(dev, 8 * B * S * min(ns, N))
    got = prim.query_ball_point(radius, ns, _dev(xyz, dev), _dev(new_xyz, dev))
    assert got.dtype == torch.int64 and tuple(got.shape) == (B, S, min(ns, N))
    return got.cpu().numpy()


@pytest.mark.parametrize('case', BALL_CASES, ids=lambda c: c['id'])
def test_ball_query_planted_scenes_give_the_closed_form_rows(cuda_device, case):
    sc = ball_scene_of(case)
    got = _query(cuda_device, case['radius'], case['ns'], sc['xyz'], sc['new_xyz'])
    want = R.planted_rows(case['N'], case['hits'], case['ns'], sc['nan_at'])
    assert np.array_equal(got, want), (case['id'], np.argwhere((got != want).any(-1)).tolist())
    assert np.array_equal(got, R.ball_ref(sc['xyz'], sc['new_xyz'], R.r2_of(case['radius']), case['ns'])), case['id']


@pytest.mark.parametrize('case', GAP_CASES, ids=lambda c: c['id'])
def test_ball_query_general_scenes_equal_the_reference_in_every_row(cuda_device, case):
    sc = gap_scene_of(case)
    assert sc is not None, 'no r^2 near the nominal radius separates the pairs'
    got = _query(cuda_device, sc['radius'], case['ns'], sc['xyz'], sc['new_xyz'])
    want = R.ball_ref(sc['xyz'], sc['new_xyz'], sc['r2'], case['ns'])
    differ = (got != want).any(-1)
    print(f"{case['id']}: r^2 candidate {sc['candidate']}, clearance {sc['clearance']:.2e}, {int(differ.sum())} of {differ.size} rows differ")
    assert not differ.any(), (case['id'], np.argwhere(differ).tolist())


# -------------------------------------------------------------------------------------------------------- group_points
@pytest.mark.parametrize('case', GROUP_CASES, ids=lambda c: c['id'])
def test_group_points_is_the_gather_the_centring_and_the_concat_bit_for_bit(cuda_device, case):
    from catgrasp_amd import primitives as prim
    import sa_ref
    B, N, S, K, D = (case[k] for k in 'BNSKD')
    sc = group_scene_of(case)
    xyz, pts, new_xyz = (_dev(sc[k], cuda_device) for k in ('xyz', 'points', 'new_xyz'))
    assert 256 < B * S * K * (3 + D)
    for kind in GROUP_LISTS:
        idx = R.group_indices(kind, B, N, S, K, _seed(case['id'] + kind))
        di = _dev(idx, cuda_device, np.int64)
        _poison(cuda_device, 4 * B * S * K * (3 + D))
        plain = prim.group_points(xyz, pts, new_xyz, di)
        _poison(cuda_device, 4 * B * S * K * (3 + D))
        both, gxyz = prim.group_points(xyz, pts, new_xyz, di, return_grouped_xyz=True)
        assert plain.dtype == torch.float32 and tuple(plain.shape) == (B, S, K, 3 + D) and tuple(gxyz.shape) == (B, S, K, 3)
        with np.errstate(invalid='ignore'):                       # the signalling NaN among the payloads, widened and narrowed
            want = sa_ref.grouped(sc['xyz'], sc['points'], sc['new_xyz'], idx).astype(np.float32)
        assert np.array_equal(plain.cpu().numpy(), want, equal_nan=True), (case['id'], kind)
        assert np.array_equal(_bits(plain)[..., :3], _bits(want[..., :3])), (case['id'], kind)                 # one correctly rounded subtraction
        if D:
            assert np.array_equal(_bits(plain)[..., 3:], R.index_ref(_bits(sc['points']), idx)), (case['id'], kind)
        assert np.array_equal(_bits(gxyz), R.index_ref(_bits(sc['xyz']), idx)), (case['id'], kind)
        assert np.array_equal(_bits(both), _bits(plain)), (case['id'], kind)


@pytest.mark.parametrize('case', [c for c in GROUP_CASES if c['id'] in ('group-D0-K1', 'group-D5-K16', 'group-D13-K33')], ids=lambda c: c['id'])
def test_group_points_refuses_the_empty_ball_sentinel_and_a_negative_index(cuda_device, case):
    from catgrasp_amd import primitives as prim
    B, N, S, K, D = (case[k] for k in 'BNSKD')
    sc = group_scene_of(case)
    xyz, pts, new_xyz = (_dev(sc[k], cuda_device) for k in ('xyz', 'points', 'new_xyz'))
    idx = R.group_indices('random', B, N, S, K, 5)
    for bad in (N, -1):
        for where in (0, idx.size - 1):
            i = idx.copy()
            i.reshape(-1)[where] = bad
            with pytest.raises(IndexError):
                prim.group_points(xyz, pts, new_xyz, _dev(i, cuda_device, np.int64))
    prim.group_points(xyz, pts, new_xyz, _dev(idx, cuda_device, np.int64))
