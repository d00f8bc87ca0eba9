"""CPU proofs about tests/group_ref.py and the cases of tests/test_primitives_edges_gpu.py: the references are the oracle's functions
(oracle/pointnet_ref.py, itself pinned to the imported reference), every exact case is exact in float32, every planted row is what
its hit list says, every general ball case carries an r^2 that no float32 evaluation can be wrong about, the distance bound holds
for the float32 evaluations of the reference (it is never fitted to the kernel), the ball's comparison is made in float32, and the
C entry points of the primitives refuse bad arguments before any device work."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import group_ref as R
import sa_ref
import test_primitives_edges_gpu as G
from catgrasp_amd import _lib
from oracle import pointnet_ref as oref

INCLUDE = os.path.dirname(_lib.HEADER_PATH)


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---------------------------------------------------------------------------------------------------- square distances
def test_exact_distance_cases_are_exact_in_float32_and_the_oracle_returns_the_float64_result():
    worst = 0.0
    for c in G.SQ_CASES + G.ND_CASES:
        src, dst, step = G.sq_scene(c, exact=True)
        m = R.exactness_margin(src, dst, step)
        assert m < 1, (c['id'], m)
        worst = max(worst, m)
        ref = R.sqdist_ref(src, dst)
        assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), c['id']
        assert np.array_equal(oref.square_distance(_t(src), _t(dst)).numpy().astype(np.float64), ref), c['id']       # the float32 oracle
        assert np.array_equal(oref.square_distance(_t(src, torch.float64), _t(dst, torch.float64)).numpy(), ref), c['id']
        if c['B'] > 1:
            assert not np.array_equal(ref[0], ref[1]), c['id']                      # a wrong batch offset shows
    assert len(G.SQ_CASES) == 50 and len(G.ND_CASES) == 7
    print(f'{len(G.SQ_CASES) + len(G.ND_CASES)} exact distance cases, 0 left out; worst exactness margin {worst:.4f}')
    with pytest.raises(AssertionError):
        R.exactness_margin(src + 1.0 / 128, dst, step)


def _f32_term_by_term(src, dst):
    """The expansion in numpy float32, channel by channel, every product and sum rounded (no FMA): what the kernels do."""
    s, d = np.asarray(src, np.float32), np.asarray(dst, np.float32)
    dot = np.zeros(s.shape[:2] + d.shape[1:2], np.float32)
    s2 = np.zeros(s.shape[:2], np.float32)
    d2 = np.zeros(d.shape[:2], np.float32)
    for c in range(s.shape[2]):
        dot = dot + s[:, :, None, c] * d[:, None, :, c]
        s2 = s2 + s[:, :, c] * s[:, :, c]
        d2 = d2 + d[:, :, c] * d[:, :, c]
    v = np.float32(-2.0) * dot
    v = v + s2[:, :, None]
    return v + d2[:, None, :]


def test_the_distance_bound_holds_for_the_oracle_and_for_a_term_by_term_float32_evaluation():
    cases = [c for c in G.SQ_CASES if c['B'] == 3 and c['N'] in (17, 33) and c['M'] in (257, 513)] + G.ND_CASES
    for c in cases:
        src, dst, _ = G.sq_scene(c, exact=False)
        assert src.dtype == dst.dtype == np.float32
        ref, bound = R.sqdist_ref(src, dst), R.sqdist_bound(src, dst)
        assert np.abs(oref.square_distance(_t(src, torch.float64), _t(dst, torch.float64)).numpy() - ref).max() <= 1e-12 * max(1.0, ref.max())
        for what, v in (('oracle float32', oref.square_distance(_t(src), _t(dst)).numpy()), ('numpy float32', _f32_term_by_term(src, dst))):
            assert v.dtype == np.float32
            ratio = float((np.abs(v.astype(np.float64) - ref) / bound).max())
            assert 0 < ratio <= 1, (c['id'], what, ratio)
        # a rounding bound, not a loose one: gamma_{C+2} of the magnitude sum, a few float32 ulps of it
        C = c['C']
        assert float((bound / R.sqdist_magnitude(src, dst)).max()) <= (C + 3) * 2.0 ** -24


def test_the_gamma_of_the_bound_counts_the_roundings():
    assert R.gamma(5) == 5 * 2.0 ** -24 / (1 - 5 * 2.0 ** -24)
    one = np.ones((1, 1, 3), np.float32)
    assert R.sqdist_bound(one, one)[0, 0, 0] == (R.gamma(5) + R.gamma(5, 2.0 ** -53)) * 12.0            # 2 * 3 + 3 + 3
    assert R.sqdist_ref(one, 3 * one)[0, 0, 0] == 12.0


# -------------------------------------------------------------------------------------------------------------- gathers
def test_index_ref_is_the_oracle_and_the_cases_reach_both_ends_and_the_block_edges():
    totals = set()
    for c in G.IP_CASES:
        pts, idx = G.ip_scene_of(c)
        assert pts.shape == (c['B'], G.IP_N, c['C']) and idx.shape == c['shape']
        assert idx.min() == 0 and idx.max() == G.IP_N - 1 and (idx.size < 30 or len(np.unique(idx)) <= idx.size // 2)
        got = R.index_ref(pts.view(np.int32), idx)
        assert np.array_equal(got, oref.index_points(torch.from_numpy(pts.view(np.int32).copy()), torch.from_numpy(idx)).numpy())
        totals.add((c['C'], idx.size * c['C']))
    assert {t for C, t in totals if C == 1} == {255, 256, 257} and {t for C, t in totals if C == 64} == {192, 256, 320}
    assert {t for C, t in totals if C == 3} == {255, 258} and {t for C, t in totals if C == 7} == {252, 259}
    assert len(set(R.PAYLOADS.tolist())) == len(R.PAYLOADS) == 9
    special = R.PAYLOADS.view(np.float32)
    assert np.isnan(special).sum() == 4 and np.isinf(special).sum() == 2 and np.signbit(special[0]) and special[0] == 0


def test_group_scenes_centre_exactly_in_float64_and_grouped_is_the_oracle():
    for c in G.GROUP_CASES:
        B, N, S, K, D = (c[k] for k in 'BNSKD')
        assert 256 < B * S * K * (3 + D) <= 256 + B * K * (3 + D), c['id']            # just past one 256-thread block
        sc = G.group_scene_of(c)
        for kind in G.GROUP_LISTS:
            idx = R.group_indices(kind, B, N, S, K, G._seed(c['id'] + kind))
            assert idx.shape == (B, S, K) and 0 <= idx.min() and idx.max() < N
            x64 = sa_ref.grouped(sc['xyz'], None, sc['new_xyz'], idx)
            # [0.25, 1): both operands are multiples of 2^-26, so is their difference, below 2^27 of them: a float64 number
            q = x64 * 2.0 ** 26
            assert np.array_equal(q, np.round(q)) and np.abs(q).max() < 2.0 ** 27 and sc['xyz'].min() >= 0.25 and sc['xyz'].max() < 1.0
            bi = np.arange(B)[:, None, None]
            f32 = sc['xyz'][bi, idx] - sc['new_xyz'][:, :, None, :]                  # numpy's float32 subtraction: correctly rounded
            assert f32.dtype == np.float32 and np.array_equal(f32, x64.astype(np.float32))
        idx = R.group_indices('random', B, N, S, K, 1)
        clean = None if sc['points'] is None else np.nan_to_num(sc['points'], nan=1.5, posinf=2.5, neginf=-2.5)
        want = sa_ref.grouped(sc['xyz'], clean, sc['new_xyz'], idx).astype(np.float32)
        t = lambda a: None if a is None else torch.from_numpy(a)
        gx = oref.index_points(t(sc['xyz']), torch.from_numpy(idx)) - t(sc['new_xyz']).view(B, S, 1, 3)
        got = torch.cat([gx, oref.index_points(t(clean), torch.from_numpy(idx))], dim=-1) if D else gx
        assert np.array_equal(got.numpy(), want), c['id']
    assert {(c['D'], c['K']) for c in G.GROUP_CASES} == {(D, K) for D in (0, 1, 5, 13) for K in (1, 16, 33)}


def test_sample_and_group_of_the_oracle_is_ball_ref_then_grouped():
    """The whole chain on a general ball scene: with an r^2 that separates every pair, the float32 oracle's neighbour lists ARE
    ball_ref's, and its grouped tensor is float32(sa_ref.grouped) on them."""
    B, N, S, ns = 2, 700, 40, 16
    rng = np.random.default_rng(3)
    xyz = (rng.normal(0, 0.05, (B, N, 3)) + np.array([0.0, 0.0, 0.6])).astype(np.float32)
    feats = rng.normal(size=(B, N, 5)).astype(np.float32)
    start = torch.tensor([7, 99])
    fps = oref.farthest_point_sample(torch.from_numpy(xyz), S, start).numpy()
    new_xyz = R.index_ref(xyz, fps)
    for j in range(400):
        r2 = np.float32(0.03 ** 2 * (1 + j * 2.0 ** -12))
        if R.ball_clearance(xyz, new_xyz, r2).min() > 0:
            break
    else:
        pytest.fail('no separating r^2')
    radius = float(np.sqrt(np.float64(r2)))
    assert R.r2_of(radius) == r2
    o_new_xyz, o_new_points, o_grouped, o_fps = oref.sample_and_group(S, radius, ns, torch.from_numpy(xyz), torch.from_numpy(feats), start)
    idx = R.ball_ref(xyz, new_xyz, r2, ns)
    assert np.array_equal(o_new_xyz.numpy(), new_xyz) and np.array_equal(o_fps.numpy(), fps)
    assert np.array_equal(o_grouped.numpy(), R.index_ref(xyz, idx))
    assert np.array_equal(o_new_points.numpy(), sa_ref.grouped(xyz, feats, new_xyz, idx).astype(np.float32))


# --------------------------------------------------------------------------------------------------------- ball queries
def _oracle_rows(xyz, new_xyz, radius, ns, dtype=torch.float32):
    return oref.query_ball_point(radius, ns, _t(xyz, dtype), _t(new_xyz, dtype)).numpy()


def test_planted_rows_are_the_reference_and_the_oracle_on_every_planted_case():
    ids = [c['id'] for c in G.BALL_CASES]
    for want in ['n1', 'n63', 'n64', 'n65', 'n511', 'n512', 'n513', 'n1025', 's1', 's3', 's4', 's5', 'fill-lane63', 'fill-lane0', 'fill-511', 'fill-512',
                 'more-than-slots', 'count-past-32', 'all64-ns1', 'last-trip', 'few', 'one-hit-ns64', 'one-hit-ns65', 'one-hit-ns70', 'ns-gt-n', 'boundary-eq', 'radius0',
                 'nextafter-lo', 'nextafter-hi', 'shared', 'nan']:
        assert want in ids, want
    worst = 0.0
    for c in G.BALL_CASES:
        sc = G.ball_scene_of(c)
        B, S = len(c['hits']), len(c['hits'][0])
        assert B == 2 and c['hits'][0] != c['hits'][1], c['id']                    # different hit lists per cloud
        assert sc['xyz'].shape == (B, c['N'], 3) and sc['new_xyz'].shape == (B, S, 3)
        m = R.exactness_margin(sc['new_xyz'], sc['xyz'], R.STEP_XYZ)
        assert m < 1, (c['id'], m)
        worst = max(worst, m)
        r2 = R.r2_of(c['radius'])
        rows = R.planted_rows(c['N'], c['hits'], c['ns'], sc['nan_at'])
        assert rows.shape == (B, S, min(c['ns'], c['N']))
        assert np.array_equal(rows, R.ball_ref(sc['xyz'], sc['new_xyz'], r2, c['ns'])), c['id']
        assert np.array_equal(rows, _oracle_rows(sc['xyz'], sc['new_xyz'], c['radius'], c['ns'])), c['id']
        # what is not a hit lies at least four lattice steps beyond r, but for the near misses placed by name: one lattice value beyond r^2
        d = R.sqdist_ref(sc['new_xyz'], sc['xyz']) * 4096.0
        r2s = float(np.float64(r2)) * 4096.0
        outside = d[d > r2s]
        assert outside.size == 0 or outside.min() >= (r2s + 1 if c['scene'].get('place') else (np.sqrt(r2s) + 4) ** 2), c['id']
    print(f'{len(G.BALL_CASES)} planted cases, 0 left out; worst exactness margin {worst:.5f}')


def test_planted_cases_land_on_the_kernel_boundaries_they_name():
    by = {c['id']: c for c in G.BALL_CASES}
    for N in (63, 65, 511, 513, 1025, 1):
        c = by[f'n{N}']
        assert N % 64 != 0 and all(any(N - 1 in h for h in hb) for hb in c['hits'])           # N - 1 is a hit wherever tail lanes reload it
        assert max(len(h) for hb in c['hits'] for h in hb) < min(c['ns'], N) or N == 1        # free slots left: a second count of it would show
    for cid, at in (('fill-lane63', (63, 127)), ('fill-lane0', (64, 128)), ('fill-511', (511,)), ('fill-512', (512,))):
        c = by[cid]
        full = [sorted(h) for hb in c['hits'] for h in hb if len(h) > c['ns']]
        assert full and {h[c['ns'] - 1] for h in full} <= set(at) and at[0] in {h[c['ns'] - 1] for h in full}, cid
        assert any(h[c['ns']] == h[c['ns'] - 1] + 1 for h in full), cid                        # the hit right behind the last slot
    c = by['more-than-slots']
    for h in (c['hits'][0][0], c['hits'][1][0]):
        chunks = np.bincount(np.asarray(h) // 64)
        assert chunks.max() == 40 and 0 < c['ns'] - np.cumsum(chunks)[np.argmax(chunks) - 1] < 40
    c = by['count-past-32']
    for h in (c['hits'][0][0], c['hits'][1][0]):                                               # > 32 hits in a chunk, more behind it, slots left over
        chunks = np.bincount(np.asarray(h) // 64)
        assert chunks.max() > 32 and chunks[np.argmax(chunks) + 1:].sum() > 0 and len(h) < c['ns']
    assert all(sorted(h) == list(range(min(h), min(h) + 64)) and min(h) % 64 == 0 for hb in by['all64-ns1']['hits'] for h in hb)
    assert min(i for hb in by['last-trip']['hits'] for h in hb for i in h) >= 1024
    assert [by[f'one-hit-ns{ns}']['ns'] for ns in (64, 65, 70)] == [64, 65, 70]
    assert by['ns-gt-n']['ns'] > by['ns-gt-n']['N']
    assert {len(c['hits'][0]) for c in G.BALL_CASES if c['id'] in ('s1', 's3', 's4', 's5')} == {1, 3, 4, 5}
    # boundary cases: hits AT r^2, near misses at the next lattice value
    for cid in ('boundary-eq', 'nextafter-lo', 'nextafter-hi', 'radius0'):
        c = by[cid]
        sc = G.ball_scene_of(c)
        d = R.sqdist_ref(sc['new_xyz'], sc['xyz'])
        r2 = np.float64(R.r2_of(c['radius']))
        assert (d == r2).any(axis=(1, 2)).all() and (d * 4096 == r2 * 4096 + 1).any(axis=(1, 2)).all(), cid
    sc = G.ball_scene_of(by['shared'])
    assert np.array_equal(sc['new_xyz'][:, 0], sc['new_xyz'][:, 2]) and not np.array_equal(sc['new_xyz'][:, 0], sc['new_xyz'][:, 1])
    sc = G.ball_scene_of(by['nan'])
    assert np.isnan(sc['xyz']).any(axis=(1, 2)).all()
    rows = R.planted_rows(100, by['nan']['hits'], 8, sc['nan_at'])
    assert rows[0, 2].tolist() == [40] * 8 and rows[1, 1].tolist() == [0, 99] + [0] * 6      # the otherwise empty balls hold the NaN points


def test_the_ball_is_compared_in_float32():
    """pointnet2.py:92 compares a float32 tensor with the Python double radius ** 2; torch makes that comparison in float32.  With
    r = nextafter(1/8, 0) the double r^2 lies below 1/64 and rounds up to it: a point at d == 1/64 is a member, though 1/64 > r^2 in
    double."""
    lo, hi = float(np.nextafter(0.125, 0.0)), float(np.nextafter(0.125, np.inf))
    assert lo ** 2 < 1.0 / 64 < hi ** 2 and R.r2_of(lo) == R.r2_of(hi) == np.float32(1.0 / 64)
    d = torch.tensor([1.0 / 64], dtype=torch.float32)
    assert not bool((d > lo ** 2).any()) and bool((d.double() > lo ** 2).all())
    by = {c['id']: c for c in G.BALL_CASES}
    for cid, radius in (('nextafter-lo', lo), ('nextafter-hi', hi)):
        c = by[cid]
        assert c['radius'] == radius
        sc = G.ball_scene_of(c)
        at = R.sqdist_ref(sc['new_xyz'], sc['xyz']) == 1.0 / 64
        assert at[0, 0, [10, 60]].all() and at[0, 1, 70] and at[1, 0, 99]
        for rows in (R.ball_ref(sc['xyz'], sc['new_xyz'], R.r2_of(radius), c['ns']), _oracle_rows(sc['xyz'], sc['new_xyz'], radius, c['ns'])):
            assert rows[0, 0].tolist() == [10, 60] + [10] * 6 and rows[0, 1].tolist() == [20, 30, 70] + [20] * 5 and rows[1, 0].tolist() == [99] * 8
            assert rows[1, 1].tolist() == [100] * 8
    # made in double the comparison would lose the point for the lower radius: the float64 oracle shows the difference
    sc = G.ball_scene_of(by['nextafter-lo'])
    assert _oracle_rows(sc['xyz'], sc['new_xyz'], lo, 8, torch.float64)[1, 0].tolist() == [100] * 8


def test_every_general_ball_case_has_an_r2_that_every_pair_clears():
    for c in G.GAP_CASES:
        sc = G.gap_scene_of(c)
        assert sc is not None, c['id']
        assert sc['xyz'].shape == (2, c['N'], 3) and sc['new_xyz'].shape == (2, c['S'], 3) and sc['r2'].dtype == np.float32
        assert abs(np.sqrt(float(sc['r2'])) / c['r'] - 1) < 0.05                                   # near the nominal radius
        clear = R.ball_clearance(sc['xyz'], sc['new_xyz'], sc['r2'])                               # recomputed from the scene alone
        assert clear.shape == (2, c['S']) and clear.min() > 0, c['id']                             # zero rows excused
        assert np.array_equal(sc['new_xyz'], R.index_ref(sc['xyz'], sc['queries']))                 # the queries are cloud points
        if c['pool'] is None:
            assert np.array_equal(sc['queries'], np.tile(np.arange(c['S']), (2, 1)))
        want = R.ball_ref(sc['xyz'], sc['new_xyz'], sc['r2'], c['ns'])
        assert np.array_equal(want, _oracle_rows(sc['xyz'], sc['new_xyz'], sc['radius'], c['ns'])), c['id']
        d32 = _f32_term_by_term(sc['new_xyz'], sc['xyz'])
        assert np.array_equal(~(d32 > sc['r2']), ~(R.sqdist_ref(sc['new_xyz'], sc['xyz']) > np.float64(sc['r2']))), c['id']
        hits = (~(d32 > sc['r2'])).sum(-1)
        print(f"{c['id']}: candidate {sc['candidate']}, r^2 {float(sc['r2']):.9g}, clearance {sc['clearance']:.2e}, hits per ball {hits.min()} .. {hits.max()}")
        assert hits.min() >= 1 and hits.max() > c['ns'] and (hits < c['ns']).any(), c['id']        # balls that fill and balls that pad
    assert [(c['N'], c['S'], c['ns']) for c in G.GAP_CASES] == [(700, 40, 16), (700, 40, 32), (2000, 100, 32)]


# --------------------------------------------------------------------------------------------------------------- C ABI
def test_the_primitives_refuse_bad_arguments_before_any_device_work(tmp_path):
    """Every call below returns before a launch: the host arrays stand in for device memory and nothing reads them."""
    if shutil.which('gcc') is None:
        pytest.fail('gcc is needed to call the library from C')
    F, I, NF, NL, NI = 'f', 'l', '(float*)0', '(long long*)0', '(int*)0'
    sq = 'cg_square_distance({src}, {dst}, {B}, {N}, {M}, {out}, (void*)0)'
    nd = 'cg_square_distance_nd({src}, {dst}, {B}, {N}, {M}, {C}, {out}, (void*)0)'
    ip = 'cg_index_points({pts}, {idx}, {B}, {N}, {C}, {S}L, {out}, {err}, (void*)0)'
    bq = 'cg_query_ball_point({xyz}, {new}, {B}, {N}, {S}, 0.01f, {ns}, {oi}, (void*)0)'
    gp = 'cg_group_points({xyz}, {pts}, {new}, {idx}, {B}, {N}, {S}, {K}, {D}, {out}, {gx}, {err}, (void*)0)'
    fps = 'cg_farthest_point_sample({xyz}, {start}, {B}, {N}, {np}, {scr}, {oi}, (void*)0)'
    fpx = 'cg_farthest_point_sample_xyz({xyz}, {start}, {B}, {N}, {np}, {scr}, {oi}, {ox}, (void*)0)'
    good = {sq: dict(src=F, dst=F, B=2, N=5, M=7, out=F), nd: dict(src=F, dst=F, B=2, N=5, M=7, C=4, out=F),
            ip: dict(pts=F, idx=I, B=2, N=5, C=4, S=6, out=F, err='i'), bq: dict(xyz=F, new=F, B=2, N=5, S=3, ns=4, oi=I),
            gp: dict(xyz=F, pts=F, new=F, idx=I, B=2, N=5, S=3, K=4, D=2, out=F, gx=F, err='i'),
            fps: dict(xyz=F, start=I, B=2, N=5, np=3, scr=NF, oi=I), fpx: dict(xyz=F, start=I, B=2, N=5, np=3, scr=NF, oi=I, ox=F)}
    null_of = dict(src=NF, dst=NF, out=NF, pts=NF, idx=NL, err=NI, xyz=NF, new=NF, oi=NL, start=NL, ox=NF)
    sizes = {sq: 'BNM', nd: 'BNM', ip: 'BNS', bq: ('B', 'N', 'S', 'ns'), gp: 'BNSKD', fps: ('B', 'N', 'np'), fpx: ('B', 'N', 'np')}
    zero_ok = {sq: 'BNM', nd: 'BNM', ip: 'BS', bq: ('B', 'S', 'ns'), gp: 'BSK', fps: ('B', 'np'), fpx: ('B', 'np')}
    required = {sq: ('src', 'dst', 'out'), nd: ('src', 'dst', 'out'), ip: ('pts', 'idx', 'out', 'err'), bq: ('xyz', 'new', 'oi'),
                gp: ('xyz', 'pts', 'new', 'idx', 'out', 'err'), fps: ('xyz', 'start', 'oi'), fpx: ('xyz', 'start', 'oi', 'ox')}
    cases = []
    for call, g in good.items():
        all_null = {k: null_of[k] for k in g if k in null_of}
        cases += [(call, {**g, k: -1}, 'CG_ERR_ARG') for k in sizes[call]]                                     # a negative size
        cases += [(call, {**g, **all_null, k: -1}, 'CG_ERR_ARG') for k in sizes[call]]                          # ... whatever the pointers
        cases += [(call, {**g, **all_null, k: 0}, 'CG_OK') for k in zero_ok[call]]                              # nothing to do: no pointer is read
        cases += [(call, {**g, k: null_of[k]}, 'CG_ERR_ARG') for k in required[call]]                           # work to do and a null pointer
    cases += [(nd, {**good[nd], 'C': 0}, 'CG_ERR_ARG'), (nd, {**good[nd], 'C': -3}, 'CG_ERR_ARG'), (nd, {**good[nd], 'C': 0, 'B': 0}, 'CG_ERR_ARG'),
              (ip, {**good[ip], 'C': 0}, 'CG_ERR_ARG'), (ip, {**good[ip], 'C': -1}, 'CG_ERR_ARG'), (ip, {**good[ip], 'C': 0, 'S': 0}, 'CG_ERR_ARG'),
              (nd, {**good[nd], 'C': 3, 'src': NF}, 'CG_ERR_ARG'),                                             # the forward to the tiled entry refuses too
              (bq, {**good[bq], 'N': 0}, 'CG_ERR_ARG'), (gp, {**good[gp], 'N': 0}, 'CG_ERR_ARG'), (fps, {**good[fps], 'N': 0}, 'CG_ERR_ARG'),
              (fpx, {**good[fpx], 'N': 0}, 'CG_ERR_ARG'),
              (gp, {**good[gp], 'D': 1, 'pts': NF}, 'CG_ERR_ARG'),                                             # features promised and not given
              (gp, {**good[gp], 'D': 0, 'pts': NF, 'K': 0}, 'CG_OK'),
              (gp, {**good[gp], 'D': 0, 'pts': NF, 'gx': NF, 'out': NF}, 'CG_ERR_ARG'),                       # D == 0 passes `points` by; the output is still needed
              (fpx, {**good[fpx], 'ox': NF, 'np': 0}, 'CG_OK'), (fpx, {**good[fpx], 'ox': NF, 'B': 0}, 'CG_OK'),
              (fps, {**good[fps], 'N': 24577}, 'CG_ERR_ARG'), (fpx, {**good[fpx], 'N': 24577}, 'CG_ERR_ARG')]     # past the register kernels: scratch needed
    body = ''.join(f'  bad += check({i}, {call.format(**a)}, {want});\n' for i, (call, a, want) in enumerate(cases))
    src = ('#include "catgrasp_amd.h"\n#include <stdio.h>\n'
           'static int check(int i, int got, int want) { if (got != want) printf("case %d: %d, not %d\\n", i, got, want); return got != want; }\n'
           'int main(void) {\n  float f[4];\n  long long l[4];\n  int i[4];\n  int bad = 0;\n  f[0] = 0.f;\n  l[0] = 0;\n  i[0] = 0;\n' + body
           + f'  printf("{len(cases)} calls\\n");\n  return bad;\n}}\n')
    (tmp_path / 'main.c').write_text(src)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-pedantic', '-I', INCLUDE, 'main.c', '-L', libdir, '-lcatgrasp_amd',
                           f'-Wl,-rpath,{libdir}', '-Wl,--allow-shlib-undefined', '-o', 'main'], cwd=tmp_path)
    out = subprocess.run([str(tmp_path / 'main')], capture_output=True, text=True)
    failed = [cases[int(line.split()[1].rstrip(':'))] for line in out.stdout.splitlines() if line.startswith('case')]
    assert out.returncode == 0 and not failed, (failed, out.stdout[-2000:], out.stderr[-2000:])
    assert out.stdout.split()[-2:] == [str(len(cases)), 'calls'] and len(cases) > 100


def test_sizes_are_judged_before_pointers_through_the_binding_too():
    """That cg_group_points goes on to launch with D == 0 and points == NULL is shown on the device (group-D0-* of the GPU module pass
    points=None): a call that gets past the checks cannot be made here."""
    lib = _lib.lib()
    assert lib.cg_group_points(None, None, None, None, 2, 5, 3, 4, 0, None, None, None, None) == -1
    assert lib.cg_group_points(None, None, None, None, 2, 5, 0, 4, 7, None, None, None, None) == 0
    assert lib.cg_group_points(None, None, None, None, 2, 5, 3, 4, -1, None, None, None, None) == -1
    assert lib.cg_farthest_point_sample_xyz(None, None, 0, 5, 3, None, None, None, None) == 0
    assert lib.cg_farthest_point_sample_xyz(None, None, 2, 5, 3, None, None, None, None) == -1
