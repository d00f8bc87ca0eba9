"""GPU tests of the k-d tree searches on the grid index (include/catgrasp_amd_kdtree.h): GridIndex.nearest / .ball_point and the
cKDTree front.

Everything is exact, so every comparison is torch.equal / array_equal: index and d2 BITS against kdtree_ref's float64 brute force, index
against the brute-force kernel behind affordance.nearest_neighbor, and one index against another across three cells per cloud (one
lattice step, about ten points a cell, one cell for the whole cloud).  The clouds with exact ties (the lattices) settle the tie rule;
scipy, whose tie rule is not stated, is asked only on 'sheet'."""
import functools
import math

import numpy as np
import pytest
import torch

import kdtree_ref as KR
import neighbors_ref as NR
from catgrasp_amd import _lib as L
from catgrasp_amd import affordance, aligning, cluster, neighbors

pytestmark = pytest.mark.gpu
MAX_ROUNDS = 64                                                             # CG_KD_MAX_ROUNDS of the header
FAR = np.array([[1e3, -1e3, 5.0], [-1e6, 2e6, 1e6]])
CLOUDS = ['sheet', 'A_perm', 'mm32', 'mm64', 'pow2']
STEP = {'sheet': 0.001, 'A_perm': 0.001, 'mm32': 0.001, 'mm64': 0.001, 'pow2': 2.0 ** -10}


@functools.lru_cache(maxsize=None)
def _cloud(name):
    P = {'mm32': lambda: NR.mm_lattice(np.float32), 'mm64': lambda: NR.mm_lattice(np.float64), 'pow2': NR.pow2_lattice}.get(name, lambda: NR.cloud(name))()
    P.setflags(write=False)
    return P


def _cells(name):
    """one lattice step; about ten points a cell (default_cell aims at 4: a surface holds 2.5 times as many at 1.6 times the pitch);
    one cell for the whole cloud"""
    P = _cloud(name).astype(np.float64)
    lo, hi = P.min(axis=0), P.max(axis=0)
    return STEP[name], 1.6 * neighbors.default_cell(lo, hi, len(P)), 2.0 * float((hi - lo).max())


@functools.lru_cache(maxsize=None)
def _queries(name):
    """float64 queries off the cloud: jittered points, uniform in the enlarged box, for a lattice the midpoints and half-step offsets
    (exact 2-, 4- and 8-way ties on 'pow2'), and two far points"""
    if name == 'sheet':
        return KR.sheet_queries()
    P = _cloud(name).astype(np.float64)
    rng = np.random.default_rng(7)
    lo, hi = P.min(axis=0), P.max(axis=0)
    sets = [P[:1000] + rng.normal(0, 2e-4, (min(len(P), 1000), 3)), rng.uniform(lo - (hi - lo), hi + (hi - lo), (1000, 3))]
    if name != 'A_perm':
        h = STEP[name] / 2
        sets += [P[::3] + np.array(o) * h for o in ((1, 0, 0), (0, 0, 1), (1, 1, 0), (0, -1, 1), (1, 1, 1), (-1, 1, -1))]
    Q = np.concatenate(sets + [FAR])
    Q.setflags(write=False)
    return Q


@functools.lru_cache(maxsize=None)
def _ref(name, f32):
    Q = _queries(name)
    return KR.nearest(_cloud(name), Q.astype(np.float32) if f32 else Q)


def _first_occurrence(P):
    _, first, inv = np.unique(P, axis=0, return_index=True, return_inverse=True)
    return first[inv.reshape(-1)].astype(np.int32)


@pytest.mark.parametrize('name', CLOUDS)
def test_nearest_is_brute_force_bit_for_bit_at_every_cell(cuda_device, name):
    P, Q = _cloud(name), _queries(name)
    if name == 'pow2':                                                      # the ties are there: midpoints of 2, 4 and 8 points
        m = NR.d2_matrix(Q[-1460:-2], P)
        assert {2, 4, 8} <= set(np.unique((m == m.min(axis=1, keepdims=True)).sum(axis=1)).tolist())
    dP = torch.tensor(P, device=cuda_device)
    outs = []
    for cell in _cells(name):
        index = neighbors.GridIndex(dP, cell)
        outs.append((*index.nearest(dP), *index.nearest(Q), *index.nearest(Q.astype(np.float32))))
        for k, t in enumerate(outs[-1]):
            assert t.is_cuda and t.dtype == (torch.float64 if k % 2 else torch.int32)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)
    own_i, own_d, i64, d64, i32, d32 = (t.cpu().numpy() for t in outs[0])
    # the cloud itself: distance zero, and of duplicates the smaller index
    assert np.array_equal(own_i, _first_occurrence(P)) and not own_d.any()
    for (gi, gd), f32 in (((i64, d64), False), ((i32, d32), True)):
        want_i, want_d = _ref(name, f32)
        assert np.array_equal(gi, want_i) and np.array_equal(gd.view(np.uint64), want_d.view(np.uint64))
        q = Q.astype(np.float32) if f32 else Q
        assert np.array_equal(affordance.nearest_neighbor(q, P, cuda_device).cpu().numpy(), want_i)
    # float64 points and queries that hold float32 values: the bits of the float32 run
    wide = neighbors.GridIndex(torch.tensor(P.astype(np.float64), device=cuda_device), _cells(name)[1])
    for a, b in zip(wide.nearest(Q.astype(np.float32).astype(np.float64)), outs[0][4:]):
        assert torch.equal(a, b)


def test_both_paths_are_taken_and_the_round_count_stays_under_the_cap(cuda_device):
    P, Q = _cloud('sheet'), _queries('sheet')
    step, _, whole = _cells('sheet')
    idx, d2, rounds = neighbors.GridIndex(P, step, device=cuda_device).nearest(Q, debug=True)
    assert rounds.dtype == torch.int32 and rounds.shape == idx.shape
    r = rounds.cpu().numpy()
    print('box rounds', np.unique(r[r > 0], return_counts=True), 'linear pass after', np.unique(-r[r < 0], return_counts=True))
    assert len(np.unique(r[r > 0])) >= 3 and 0 < (r < 0).sum() < len(r) and (r != 0).all()
    assert np.abs(r).max() <= MAX_ROUNDS
    assert np.array_equal(idx.cpu().numpy(), _ref('sheet', False)[0])
    # one cell for the whole cloud: a query inside the box is done after the first round
    P64 = P.astype(np.float64)
    inside = ((Q >= P64.min(axis=0)) & (Q <= P64.max(axis=0))).all(axis=1)
    assert inside.sum() > 1000
    idx1, _, rounds1 = neighbors.GridIndex(P, whole, device=cuda_device).nearest(Q, debug=True)
    r1 = rounds1.cpu().numpy()
    assert (r1[inside] == 1).all() and np.abs(r1).max() <= MAX_ROUNDS and torch.equal(idx1, idx)
    # a query so far from a cell so small that doubling alone would take 90 rounds: the cap ends it, with the linear pass's answer
    few = P[:200]
    Qf = np.concatenate((Q[-40:], [[1e15, -1e15, 1e15]]))
    idx2, d22, rounds2 = neighbors.GridIndex(few, 1e-6, device=cuda_device).nearest(Qf, debug=True)
    want_i, want_d = KR.nearest(few, Qf)
    assert np.array_equal(idx2.cpu().numpy(), want_i) and np.array_equal(d22.cpu().numpy().view(np.uint64), want_d.view(np.uint64))
    assert int(rounds2.abs().max()) == MAX_ROUNDS and int(rounds2[-1]) == -MAX_ROUNDS


def test_degenerate_inputs(cuda_device):
    Q = np.concatenate((NR.cloud('sheet')[:50].astype(np.float64), FAR))
    one = np.array([[0.01, -0.02, 0.5]], np.float32)
    for cell in (1e-4, 0.002, 10.0):
        idx, d2 = neighbors.GridIndex(one, cell, device=cuda_device).nearest(Q)
        assert not idx.any() and np.array_equal(d2.cpu().numpy().view(np.uint64), NR.d2_matrix(Q, one)[:, 0].view(np.uint64))
        # a hundred copies of one point: the smallest index
        idx, d2 = neighbors.GridIndex(np.repeat(one, 100, axis=0), cell, device=cuda_device).nearest(Q)
        assert not idx.any() and np.array_equal(d2.cpu().numpy().view(np.uint64), NR.d2_matrix(Q, one)[:, 0].view(np.uint64))
    # points on a line along x: ext_y = ext_z = 1
    line = np.zeros((300, 3))
    line[:, 0] = np.random.default_rng(2).permutation(300) * 0.001
    line[:, 1:] = (0.25, -0.125)
    Ql = np.concatenate((line[::7] + (0.0004, 0.003, -0.002), line[::11] + (0.0005, 0, 0), FAR))
    want_i, want_d = KR.nearest(line, Ql)
    for cell in (0.001, 0.01, 1.0):
        index = neighbors.GridIndex(line, cell, device=cuda_device)
        assert index.ext[1:] == [1, 1]
        idx, d2 = index.nearest(Ql)
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(d2.cpu().numpy().view(np.uint64), want_d.view(np.uint64))
        # m = 1, as an array and through the front
        idx, d2 = index.nearest(Ql[3:4])
        assert idx.tolist() == [want_i[3]] and d2.tolist() == [want_d[3]]
    # a query exactly on the corners of the box, and just outside them
    P = NR.cloud('sheet')
    P64 = P.astype(np.float64)
    lo, hi = P64.min(axis=0), P64.max(axis=0)
    corners = np.array([[(lo, hi)[b][a] for a, b in enumerate(bits)] for bits in np.ndindex(2, 2, 2)])
    corners = np.concatenate((corners, np.nextafter(corners, np.inf), np.nextafter(corners, -np.inf)))
    want_i, want_d = KR.nearest(P, corners)
    for cell in (0.001, 0.01):
        idx, d2 = neighbors.GridIndex(P, cell, device=cuda_device).nearest(corners)
        assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(d2.cpu().numpy().view(np.uint64), want_d.view(np.uint64))
    # no data, no queries
    empty = neighbors.GridIndex(P[:0], 0.002, device=cuda_device)
    idx, d2, rounds = empty.nearest(Q, debug=True)
    assert idx.tolist() == [-1] * len(Q) and torch.isinf(d2).all() and not rounds.any()
    offsets, indices = empty.ball_point(Q, 0.002)
    assert offsets.tolist() == [0] * (len(Q) + 1) and indices.shape == (0,) and indices.dtype == torch.int32
    index = neighbors.GridIndex(P, 0.002, device=cuda_device)
    idx, d2, rounds = index.nearest(Q[:0], debug=True)
    assert idx.shape == d2.shape == rounds.shape == (0,) and idx.dtype == torch.int32 and d2.dtype == torch.float64
    offsets, indices = index.ball_point(Q[:0], 0.002)
    assert offsets.tolist() == [0] and indices.shape == (0,)
    # the ABI refuses on the device what it refuses without one, and launches nothing
    g = index._grid()
    out_i, out_d = torch.full((4,), 7, dtype=torch.int32, device=cuda_device), torch.zeros(4, dtype=torch.float64, device=cuda_device)
    q = torch.zeros((4, 3), dtype=torch.float32, device=cuda_device)
    assert L.lib().cg_grid_nearest(*g, L._p(q), 0, None, 0, L._p(out_i), L._p(out_d), None, L._stream()) == -1
    assert L.lib().cg_grid_ball_fill(*g, L._p(q), 0, None, 4, 0.0021, L._p(out_d), 4, L._p(out_i), L._stream()) == -1
    torch.cuda.synchronize()
    assert out_i.tolist() == [7] * 4


@pytest.mark.parametrize('name,radius', [('pow2', 2.0 ** -9), ('mm32', 0.002), ('mm64', 0.002), ('sheet', 0.002), ('sheet', 0.005)])
def test_ball_lists_equal_brute_force_exactly(cuda_device, name, radius):
    P = _cloud(name)
    Q = np.concatenate((P[:1500].astype(np.float64), _queries(name)[:1500]))
    if name == 'pow2':                                                      # pairs exactly at the bound are in
        assert (NR.d2_matrix(Q[:len(P)], P) == radius * radius).any()
    for q in (Q, Q.astype(np.float32)):
        want_off, want_idx = KR.ball_point(P, q, radius)
        starts = np.zeros(len(want_idx) + 1, bool)
        starts[want_off] = True
        for cell in (radius, 2.5 * radius):
            index = neighbors.GridIndex(P, cell, device=cuda_device)
            offsets, indices = index.ball_point(q, radius)
            assert offsets.dtype == torch.int64 and indices.dtype == torch.int32 and offsets.is_cuda and indices.is_cuda
            assert np.array_equal(offsets.cpu().numpy(), want_off) and np.array_equal(indices.cpu().numpy(), want_idx)
            assert torch.equal(torch.diff(offsets).to(torch.int32), index.count_within(q, radius))
            i = indices.cpu().numpy().astype(np.int64)
            assert ((np.diff(i) > 0) | starts[1:len(i)]).all()              # ascending within every list


def test_ball_lists_with_an_empty_one_in_the_middle_and_a_total_of_zero(cuda_device):
    P = NR.cloud('sheet')
    index = neighbors.GridIndex(P, 0.005, device=cuda_device)
    Q = np.stack((P[10].astype(np.float64), [0.0, 0.0, 0.7], P[11].astype(np.float64)))
    want_off, want_idx = KR.ball_point(P, Q, 0.005)
    assert want_off[1] == want_off[2] and want_off[1] > 5 and want_off[3] - want_off[2] > 5
    offsets, indices = index.ball_point(Q, 0.005)
    assert np.array_equal(offsets.cpu().numpy(), want_off) and np.array_equal(indices.cpu().numpy(), want_idx)
    offsets, indices = index.ball_point(np.array([[0.0, 0.0, 0.7], [5.0, 5.0, 5.0]]), 0.005)
    assert offsets.tolist() == [0, 0, 0] and indices.shape == (0,)
    with pytest.raises(ValueError, match='exceeds'):
        index.ball_point(Q, 0.0051)


def test_the_front_answers_as_scipy_does(cuda_device):
    from scipy.spatial import cKDTree
    P, Q = _cloud('sheet'), _queries('sheet')
    P64 = P.astype(np.float64)
    tree = neighbors.cKDTree(P, device=cuda_device)
    assert tree.n == len(P) and tree.m == 3 and np.array_equal(tree.data, P)
    lo, hi = P64.min(axis=0), P64.max(axis=0)
    assert tree.index.cell == neighbors.default_cell(lo, hi, len(P))
    dist, idx = tree.query(Q)
    assert isinstance(dist, np.ndarray) and dist.dtype == np.float64 and idx.dtype == np.int64 and dist.shape == idx.shape == (len(Q),)
    KR.assert_same_as_scipy(dist, idx, P64, Q)
    want_i, want_d = _ref('sheet', False)
    assert np.array_equal(idx, want_i) and (np.abs(dist - np.sqrt(want_d)) <= 2.3e-16 * dist).all()      # one rounding of the root
    for cell in (0.001, 0.3):                                               # the cell is a matter of speed
        d2_, i2_ = neighbors.cKDTree(torch.tensor(P, device=cuda_device), cell=cell).query(torch.tensor(Q), return_tensor=True)
        assert d2_.is_cuda and i2_.dtype == torch.int64 and np.array_equal(d2_.cpu().numpy(), dist) and np.array_equal(i2_.cpu().numpy(), idx)
    # a miss is (inf, n); a bound below the cell (the bounded kernel) and the same bound above the cell of another tree (the unbounded
    # kernel and a mask) give one answer
    ref = cKDTree(P64)
    below, above = neighbors.cKDTree(P, cell=0.06, device=cuda_device), neighbors.cKDTree(P, cell=0.0004, device=cuda_device)
    for bound in (0.0005, 0.002, 0.05):
        (db, ib), (da, ia) = below.query(Q, distance_upper_bound=bound), above.query(Q, distance_upper_bound=bound)
        assert np.array_equal(db, da) and np.array_equal(ib, ia)
        miss = ~(want_d <= bound * bound)
        assert 0 < miss.sum() < len(Q)
        assert np.isinf(db[miss]).all() and (ib[miss] == len(P)).all() and np.array_equal(ib[~miss], want_i[~miss])
        sd, si = ref.query(Q, distance_upper_bound=bound)
        clear = np.abs(np.sqrt(want_d) - bound) > 1e-12 * bound             # scipy may round a distance at the bound the other way
        assert np.array_equal(ib[clear], si[clear]) and np.array_equal(np.isinf(db[clear]), np.isinf(sd[clear]))
    # a single point gives scalars
    d, i = tree.query(Q[5])
    assert isinstance(d, float) and isinstance(i, int) and (d, i) == (dist[5], idx[5])
    d, i = tree.query(Q[5], distance_upper_bound=1e-9)
    assert d == math.inf and i == len(P)
    d, i = tree.query(torch.tensor(Q[5]), return_tensor=True)
    assert d.shape == i.shape == () and float(d) == dist[5] and int(i) == idx[5]
    # empty queries, empty data
    dist0, idx0 = tree.query(Q[:0])
    assert dist0.shape == idx0.shape == (0,) and idx0.dtype == np.int64
    none = neighbors.cKDTree(P[:0], device=cuda_device)
    dist0, idx0 = none.query(Q[:4])
    assert none.n == 0 and np.isinf(dist0).all() and idx0.tolist() == [0] * 4
    assert none.query_ball_point(Q[:2], 0.01).tolist() == [[], []] and none.query_ball_point(Q[:2], 0.01, return_length=True).tolist() == [0, 0]


def test_the_front_gives_ball_lists_and_lengths_on_either_side_of_the_cell(cuda_device):
    P, Q = _cloud('sheet'), _queries('sheet')[:1500]
    tree = neighbors.cKDTree(P, cell=0.003, device=cuda_device)
    small, large = 0.002, 0.005
    for r in (small, large, large):
        want_off, want_idx = KR.ball_point(P, Q, r)
        lens = tree.query_ball_point(Q, r, return_length=True)
        assert isinstance(lens, np.ndarray) and lens.shape == (len(Q),) and np.array_equal(lens, np.diff(want_off))
        lists = tree.query_ball_point(Q, r)
        assert lists.dtype == object and lists.shape == (len(Q),) and isinstance(lists[0], list)
        assert all(lists[i] == want_idx[want_off[i]:want_off[i + 1]].tolist() for i in range(len(Q)))
        one = tree.query_ball_point(Q[3], r)
        assert isinstance(one, list) and one == lists[3] and tree.query_ball_point(Q[3], r, return_length=True) == len(one)
    assert list(tree._wider) == [large] and tree._wider[large].cell == large            # built once, kept


def test_the_call_shapes_of_the_reference_give_the_indices_of_todays_callers(cuda_device):
    # predicter.py:260 -- the voxel centroids of a cloud at 2 mm against the cloud; run_grasp_simulation.py:120 -- the same at 0.5 mm
    for name, voxel in (('A_perm', 0.002), ('sheet', 0.0005)):
        P = torch.tensor(_cloud(name), dtype=torch.float64, device=cuda_device)
        down = aligning.voxel_down_sample_device(P, voxel)
        assert 100 < len(down) <= len(P)
        dist, idx = neighbors.cKDTree(P).query(down, return_tensor=True)
        want_i, want_d = cluster.nearest_center(down, P)
        assert torch.equal(idx, want_i)
        assert torch.equal(idx.to(torch.int32), affordance.nearest_neighbor(down.cpu().numpy(), P.cpu().numpy(), cuda_device))
        assert float((dist - want_d).abs().max()) <= 1e-15                  # two float64 square roots of nearly the same sum
