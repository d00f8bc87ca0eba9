"""The N4 ops (cg_pg_* kernels) at their edges, against the numpy restatement (oracle/pointgroup_ops_ref.py) and the reference's own
host BFS (tests/golden/pointgroup_cap_golden.npz): the ball query at its 1000-neighbour cap, on the sphere and at batch boundaries;
bfs_cluster on the one-way lists the cap leaves behind; the segmented reductions, the IoU table, the rule-book pooling and
voxelization_idx at channel counts, segment lengths and key values where a kernel takes another path.  Every comparison is integer
equality or float bit equality: the kernels accumulate in the reference's order."""
import os

import numpy as np
import pytest
import torch

from oracle import pointgroup_ops_ref as ref

pytestmark = pytest.mark.gpu

CAP = 1000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'pointgroup_cap_golden.npz')


def bits_equal(got, want):
    """Same shape and the same 32-bit patterns (+inf, -inf and signed zeros included)."""
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want, dtype=got.dtype)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def one_batch(n):
    return np.zeros(n, dtype=np.int32), np.array([0, n], dtype=np.int32)


def ball_query(pg, dev, xyz, batch_idxs, batch_offsets, radius, mean_active=300):
    idx, start_len = pg.ballquery_batch_p(torch.from_numpy(xyz).to(dev), torch.from_numpy(batch_idxs).to(dev),
                                          torch.from_numpy(batch_offsets).to(dev), radius, mean_active)
    return idx, start_len


# ---- 1. ball query at the cap ---------------------------------------------------------------------------------------------------
# 999 / 1000 / 1001: one below the cap, exactly at it (a full list that is not cut), one above; 1063 / 1064: the list fills in the
# middle of a 64-wide ballot and at its end; 1300: the scan stops five ballots early.  With the 37 far points n % 4 (four points per
# block) is 0, 1, 2, 0, 1, 1; 1002 adds 3.
@pytest.mark.parametrize('blob', [999, 1000, 1001, 1002, 1063, 1064, 1300])
def test_ballquery_at_the_1000_neighbour_cap(cuda_device, blob):
    """One tight blob (sigma 0.002, radius 0.03: all points mutually in range, nothing near the sphere) + 37 far points, shuffled.
    idx / start_len equal the restatement; no count exceeds 1000; a capped row is the first 1000 in-range indices, ascending;
    idx holds exactly counts.sum() entries."""
    from catgrasp_amd import pointgroup_ops as pg
    rng = np.random.default_rng(blob)
    xyz = np.concatenate([rng.normal(0, 0.002, (blob, 3)), rng.uniform(5, 9, (37, 3))])
    xyz = np.ascontiguousarray(xyz[rng.permutation(len(xyz))], dtype=np.float32)
    n = len(xyz)
    bi, bo = one_batch(n)
    idx, start_len = ball_query(pg, cuda_device, xyz, bi, bo, 0.03)
    idx, start_len = idx.cpu().numpy(), start_len.cpu().numpy()
    r_idx, r_sl, _ = ref.ballquery_batch_p(xyz, bi, bo, 0.03, 300)
    assert np.array_equal(start_len, r_sl) and np.array_equal(idx, r_idx)
    counts = start_len[:, 1]
    assert counts.max() == min(blob, CAP) and idx.shape[0] == int(counts.sum())
    d = np.linalg.norm(xyz[:, None].astype(np.float64) - xyz[None].astype(np.float64), axis=2)
    assert not ((d > 0.025) & (d < 0.035)).any()                         # no pair near the sphere: float64 decides the same
    in_blob = np.flatnonzero(np.abs(xyz).max(axis=1) < 1)
    assert len(in_blob) == blob and (counts[in_blob] == min(blob, CAP)).all()
    for p in in_blob[[0, 1, len(in_blob) // 2, -2, -1]]:                  # low and high indices alike: the first 1000, ascending
        assert np.array_equal(idx[start_len[p, 0]:start_len[p, 0] + counts[p]], np.flatnonzero(d[p] < 0.03)[:CAP])


# ---- 2. ball query on the sphere ------------------------------------------------------------------------------------------------
def test_ballquery_excludes_points_exactly_on_the_sphere(cuda_device):
    """12 x 12 x 12 lattice, spacing 1/16, radius 5/16: every coordinate, difference, square and sum is exact in float32, so
    d2 == r2 exactly for the 30 lattice neighbours of an interior point at squared distance 25 (6 on the axes, 24 of the
    (+-3, +-4, 0) family).  bfs_cluster.cu:38 tests d2 < r2: none of them may be listed.  Expected lists from integer arithmetic."""
    from catgrasp_amd import pointgroup_ops as pg
    rng = np.random.default_rng(12)
    grid = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing='ij'), -1).reshape(-1, 3)
    grid = grid[rng.permutation(len(grid))]
    xyz = np.ascontiguousarray(grid / 16.0, dtype=np.float32)
    assert np.array_equal(xyz.astype(np.float64) * 16, grid)
    n = len(grid)
    d2 = ((grid[:, None] - grid[None]) ** 2).sum(-1)
    interior = np.flatnonzero(((grid >= 5) & (grid <= 6)).all(axis=1))
    assert len(interior) == 8 and ((d2[interior] == 25).sum(axis=1) == 30).all()
    want = [np.flatnonzero(row < 25) for row in d2]
    counts = np.array([len(w) for w in want], dtype=np.int32)
    assert counts.max() < CAP
    bi, bo = one_batch(n)
    idx, start_len = ball_query(pg, cuda_device, xyz, bi, bo, 5 / 16)
    idx, start_len = idx.cpu().numpy(), start_len.cpu().numpy()
    assert np.array_equal(start_len[:, 1], counts) and np.array_equal(start_len[:, 0], np.cumsum(counts) - counts)
    assert np.array_equal(idx, np.concatenate(want))
    r_idx, r_sl, _ = ref.ballquery_batch_p(xyz, bi, bo, 5 / 16, 300)      # the restatement draws the same line
    assert np.array_equal(r_idx, idx) and np.array_equal(r_sl, start_len)


# ---- 3. ball query batch edges --------------------------------------------------------------------------------------------------
def test_ballquery_batch_edges(cuda_device):
    """Items of 63, 64, 65, 0, 129 and 1 points (one below / at / above the 64-wide scan step, an empty item between two others so
    that two offsets are equal, two steps + 1, a single point), all lying on top of each other: a scan that ran past its item's
    end, or started before it, would list a foreign point.  And n = 1 on its own."""
    from catgrasp_amd import pointgroup_ops as pg
    rng = np.random.default_rng(3)
    sizes = [63, 64, 65, 0, 129, 1]
    xyz = rng.normal(0, 0.02, (sum(sizes), 3)).astype(np.float32)         # every item is the same blob: partial lists, radius 0.03
    bi = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)]).astype(np.int32)
    bo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert bo[3] == bo[4]
    idx, start_len = ball_query(pg, cuda_device, xyz, bi, bo, 0.03)
    idx, start_len = idx.cpu().numpy(), start_len.cpu().numpy()
    r_idx, r_sl, _ = ref.ballquery_batch_p(xyz, bi, bo, 0.03, 300)
    assert np.array_equal(start_len, r_sl) and np.array_equal(idx, r_idx)
    owner = np.repeat(np.arange(len(xyz)), start_len[:, 1])
    assert np.array_equal(bi[idx], bi[owner]) and (start_len[:, 1] >= 1).all()
    assert 1 < start_len[:, 1].max() < 129 and start_len[-1, 1] == 1       # partial lists; the single point finds itself alone
    one = np.array([[0.25, -1.0, 3.0]], dtype=np.float32)
    idx1, sl1 = ball_query(pg, cuda_device, one, *one_batch(1), 0.03)
    assert idx1.cpu().tolist() == [0] and sl1.cpu().tolist() == [[0, 1]]


# ---- 4. bfs_cluster on truncated lists ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def cap_golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('scene', ['blob1300', 'bridged', 'bar'])
def test_bfs_cluster_on_lists_cut_by_the_cap(cuda_device, cap_golden, scene):
    """Lists from the device ball query (counts as in the fixture, capped) -> bfs_cluster vs the reference's own queue BFS:
    offsets, cluster ids, and per cluster the members as a sorted set (the reference lists them in visit order).  On blob1300 and
    bridged a point that lists a blob's first 1000 points and is listed by nobody stays outside the blob's cluster; reading the
    lists both ways returns 1300 / 400 where the reference returns 1000 / 400."""
    from catgrasp_amd import pointgroup_ops as pg
    g = cap_golden
    xyz, label = g[f'{scene}_xyz'], g[f'{scene}_label']
    idx, start_len = ball_query(pg, cuda_device, xyz, *one_batch(len(xyz)), float(g['radius']))
    assert np.array_equal(start_len[:, 1].cpu().numpy(), g[f'{scene}_counts']) and int(start_len[:, 1].max()) == CAP
    for thr in (1, 50):
        ci, co = pg.bfs_cluster(torch.from_numpy(label).to(cuda_device), idx, start_len, thr)
        ci, co = ci.cpu().numpy(), co.cpu().numpy()
        rci, rco = g[f'{scene}_thr{thr}_cluster_idxs'], g[f'{scene}_thr{thr}_cluster_offsets']
        print(f'{scene} threshold {thr}: cluster sizes >= 50 {[int(s) for s in np.diff(co) if s >= 50]}, reference {[int(s) for s in np.diff(rco) if s >= 50]}')
        assert np.array_equal(co, rco) and np.array_equal(ci[:, 0], rci[:, 0])
        for c in range(len(rco) - 1):
            assert np.array_equal(ci[rco[c]:rco[c + 1], 1], np.sort(rci[rco[c]:rco[c + 1], 1]))


# ---- 5. bfs_cluster on hand-written one-way lists -------------------------------------------------------------------------------
def _csr(n, edges):
    """edges [(from, to)]: `from` lists `to` -> (idx, start_len)."""
    rows = [[b for a, b in edges if a == p] for p in range(n)]
    counts = np.array([len(r) for r in rows], dtype=np.int32)
    idx = np.array([b for r in rows for b in r], dtype=np.int32)
    return idx, np.stack([np.cumsum(counts) - counts, counts], 1).astype(np.int32)


ONE_WAY = {     # name: (labels, edges, the clusters the reference's queue BFS returns at threshold 1)
    'a_listed_by_a_later_point': ([0, 0, 0], [(2, 0)], [[0], [1], [2]]),
    'b_lists_a_later_point': ([0, 0, 0], [(0, 2)], [[0, 2], [1]]),
    'c_later_point_lists_a_seed': ([0, 0, 0, 0], [(3, 1), (1, 2)], [[0], [1, 2], [3]]),
    'd_label_boundary': ([0, 1, 1], [(0, 1), (1, 2)], [[0], [1, 2]]),
    'e_chain_descending': ([0] * 40, [(k, k - 1) for k in range(1, 40)], [[k] for k in range(40)]),
    'f_chain_ascending': ([0] * 40, [(k, k + 1) for k in range(39)], [list(range(40))]),
}


@pytest.mark.parametrize('case', sorted(ONE_WAY))
def test_bfs_cluster_follows_lists_one_way(cuda_device, case):
    """CSR lists typed in by hand, where `p lists q` does not imply `q lists p`.  Expected from the restated queue BFS (which the
    table above must agree with); thresholds 1 and 2: a cluster of exactly `threshold` points is kept.  Read both ways, cases a, c
    and e come out merged."""
    from catgrasp_amd import pointgroup_ops as pg
    labels, edges, table = ONE_WAY[case]
    label = np.array(labels, dtype=np.int32)
    idx, start_len = _csr(len(label), edges)
    t = lambda a: torch.from_numpy(a).to(cuda_device)
    for thr in (1, 2):
        rci, rco = ref.bfs_cluster(label, idx, start_len, thr)
        kept = [c for c in table if len(c) >= thr]
        assert [sorted(rci[rco[c]:rco[c + 1], 1].tolist()) for c in range(len(rco) - 1)] == kept
        ci, co = pg.bfs_cluster(t(label), t(idx), t(start_len), thr)
        assert ci.dtype == torch.int32 and co.dtype == torch.int32 and tuple(ci.shape) == (sum(len(c) for c in kept), 2)
        ci, co = ci.cpu().numpy(), co.cpu().numpy()
        got = [ci[co[c]:co[c + 1], 1].tolist() for c in range(len(co) - 1)]
        print(f'{case} threshold {thr}: {got if len(got) < 6 else str(len(got)) + " clusters"}')
        assert np.array_equal(co, rco) and np.array_equal(ci[:, 0], rci[:, 0]) and got == kept


# ---- 6. segment reduce and RoI pool ---------------------------------------------------------------------------------------------
# 13 segments; a wavefront handles one (segment, 64-channel slab) and a block four of them: C = 1, 63, 64 -> 13 wavefronts (13 % 4 = 1),
# 65 -> 26 (2), 130 -> 39 (3), 200 -> 52 (0).
SEG_LENGTHS = [5, 0, 1, 2, 17, 64, 65, 3, 0, 0, 130, 1, 2]


@pytest.mark.parametrize('C', [1, 63, 64, 65, 130, 200])
def test_segment_reduce_and_roipool_on_ties_and_short_segments(cuda_device, C):
    """Values drawn from {-2, ..., 2}: every longer segment holds its extreme several times, so the arg-max must be the FIRST
    index of the maximum (roipool.cu compares with a strict >).  Segments of length 0 (in the middle, and two in a row), 1 and 2.
    Bit-equal to the restatement, +inf / -inf / -1 on the empty segments included."""
    from catgrasp_amd import pointgroup_ops as pg
    assert len(SEG_LENGTHS) == 13
    rng = np.random.default_rng(C)
    offsets = np.concatenate([[0], np.cumsum(SEG_LENGTHS)]).astype(np.int32)
    inp = rng.integers(-2, 3, (int(offsets[-1]), C)).astype(np.float32)
    t_in, t_off = torch.from_numpy(inp).to(cuda_device), torch.from_numpy(offsets).to(cuda_device)
    r_mean, _ = ref.segment(inp, offsets, 0); r_min, _ = ref.segment(inp, offsets, 1); r_max, r_am = ref.segment(inp, offsets, 2)
    assert np.isposinf(r_min[1]).all() and np.isneginf(r_max[8]).all() and (r_am[9] == -1).all() and not r_mean[1].any()
    first = np.array([[offsets[s] + np.flatnonzero(inp[offsets[s]:offsets[s + 1], c] == r_max[s, c])[0] if SEG_LENGTHS[s] else -1
                       for c in range(C)] for s in range(13)])
    assert np.array_equal(first, r_am) and (inp[offsets[5]:offsets[6]] == r_max[5]).sum(axis=0).min() > 1      # ties, first one wins
    assert bits_equal(pg.sec_mean(t_in, t_off).cpu().numpy(), r_mean)
    assert bits_equal(pg.sec_min(t_in, t_off).cpu().numpy(), r_min)
    assert bits_equal(pg.sec_max(t_in, t_off).cpu().numpy(), r_max)
    of, am = pg.roipool(t_in, t_off)
    assert bits_equal(of.cpu().numpy(), r_max) and np.array_equal(am.cpu().numpy(), r_am)


# ---- 7. get_iou -----------------------------------------------------------------------------------------------------------------
def test_get_iou_past_one_trip_of_the_instance_loop(cuda_device):
    """300 instances: the 256-thread loop over instances takes a second trip, with 44 threads.  Six proposals, one of them empty and
    one made of points labelled -100 only; instance 17 has no point at all (instance_pointnum == 0, so the empty proposal divides
    0 by 1e-5).  Bit-equal to the restatement."""
    from catgrasp_amd import pointgroup_ops as pg
    rng = np.random.default_rng(7)
    N, nI = 3000, 300
    labels = rng.integers(0, nI, N).astype(np.int64)
    labels[labels == 17] = 18
    labels[rng.random(N) < 0.15] = -100
    pointnum = np.bincount(labels[labels >= 0], minlength=nI).astype(np.int32)
    assert pointnum[17] == 0 and pointnum[299] > 0
    ignored = np.flatnonzero(labels == -100)
    props = [rng.integers(0, N, 400), np.zeros(0, dtype=np.int64), rng.choice(ignored, 50), np.flatnonzero(labels == 299), rng.integers(0, N, 1),
             rng.integers(0, N, 700)]
    off = np.concatenate([[0], np.cumsum([len(p) for p in props])]).astype(np.int32)
    pidx = np.concatenate(props).astype(np.int32)
    want = ref.get_iou(pidx, off, labels, pointnum)
    assert not want[1].any() and not want[2].any() and want[3, 299] > 0.99 and want[:, 256:].any()
    t = lambda a: torch.from_numpy(a).to(cuda_device)
    got = pg.get_iou(t(pidx), t(off), t(labels), t(pointnum)).cpu().numpy()
    assert bits_equal(got, want)


# ---- 8. voxel pooling -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 64, 65, 130])
@pytest.mark.parametrize('max_active', [1, 7])
def test_voxel_pooling_rule_book_edges(cuda_device, C, max_active):
    """Rule books of width 1 + 1 and 1 + 7 with empty rows (count 0, stale ids behind it), full rows, and with max_active 7 a row that
    lists one point twice (it counts twice, in the sum and in the mean's divisor).  Mean and sum, bit-equal to the restatement."""
    from catgrasp_amd import pointgroup_ops as pg
    rng = np.random.default_rng(100 * C + max_active)
    N, M = 50, 11
    feats = rng.normal(size=(N, C)).astype(np.float32)
    rules = rng.integers(0, N, (M, max_active + 1)).astype(np.int32)      # ids behind the count are never read
    rules[:, 0] = rng.integers(0, max_active + 1, M)
    rules[0, 0] = 0; rules[5, 0] = 0; rules[1, 0] = max_active; rules[M - 1, 0] = max_active
    if max_active > 1:
        rules[3, :4] = [3, 9, 4, 9]
    for mode, average in ((4, True), (3, False)):
        got = pg.voxelization(torch.from_numpy(feats).to(cuda_device), torch.from_numpy(rules).to(cuda_device), mode).cpu().numpy()
        want = ref.voxelize_fp(feats, rules, average)
        assert not want[0].any() and bits_equal(got, want)


# ---- 9. voxelization_idx at the key limits --------------------------------------------------------------------------------------
def _check_voxelization_idx(pg, dev, coords, mode):
    oc, im, om = pg.voxelization_idx(torch.from_numpy(coords).to(dev), 32768, mode)
    roc, rim, rom = ref.voxelization_idx(coords, mode)
    assert oc.dtype == torch.int64 and im.dtype == torch.int32 and om.dtype == torch.int32
    assert np.array_equal(oc.cpu().numpy(), roc) and np.array_equal(im.cpu().numpy(), rim) and np.array_equal(om.cpu().numpy(), rom)
    return om


def test_voxelization_idx_at_the_key_limits(cuda_device):
    """The 64-bit sort key packs 15 bits of batch index and 16 bits per axis: coordinates 0 and 65535 on every axis, batch indices 0
    and 32767 (all 16 corners, the top key filling 63 bits), mixed with duplicates and mid-range rows; (N,4) and (N,3) layouts; all
    five modes (mode 0 on the unique rows); n = 1; 300 points in one voxel (a 301-wide map).  One past either limit raises."""
    from catgrasp_amd import pointgroup_ops as pg
    rng = np.random.default_rng(9)
    corners = np.array([[b, x, y, z] for b in (0, 32767) for x in (0, 65535) for y in (0, 65535) for z in (0, 65535)], dtype=np.int64)
    mid = np.concatenate([rng.integers(0, 32768, (20, 1)), rng.integers(0, 65536, (20, 3))], axis=1)
    unique = np.concatenate([corners, mid])
    assert len(np.unique(unique, axis=0)) == len(unique)
    coords = unique[rng.integers(0, len(unique), 150)]                    # duplicates, random order
    coords = np.ascontiguousarray(np.concatenate([coords, corners])[rng.permutation(150 + len(corners))])
    unique = np.ascontiguousarray(unique[rng.permutation(len(unique))])
    for cols in (slice(0, 4), slice(1, 4)):
        dup, uni = np.ascontiguousarray(coords[:, cols]), np.ascontiguousarray(np.unique(unique[:, cols], axis=0)[::-1])
        for mode in (4, 3, 1, 2):
            om = _check_voxelization_idx(pg, cuda_device, dup, mode)
        assert om.shape[1] == 2 and _check_voxelization_idx(pg, cuda_device, dup, 4).shape[1] > 2
        _check_voxelization_idx(pg, cuda_device, uni, 0)
    for mode in (4, 3, 1, 2, 0):
        assert _check_voxelization_idx(pg, cuda_device, np.array([[32767, 65535, 0, 65535]], dtype=np.int64), mode).cpu().tolist() == [[1, 0]]
    crowd = np.concatenate([np.tile([[32767, 65535, 65535, 65535]], (300, 1)), corners[:3]]).astype(np.int64)
    crowd = np.ascontiguousarray(crowd[rng.permutation(len(crowd))])
    assert tuple(_check_voxelization_idx(pg, cuda_device, crowd, 4).shape) == (4, 301)
    assert tuple(_check_voxelization_idx(pg, cuda_device, crowd, 2).shape) == (4, 2)
    for bad in ([0, 65536, 0, 0], [0, 0, 0, 65536], [32768, 0, 0, 0]):
        with pytest.raises(ValueError):
            pg.voxelization_idx(torch.tensor([[0, 1, 2, 3], bad], device=cuda_device), 32768, 4)
    with pytest.raises(ValueError):
        pg.voxelization_idx(torch.tensor([[1, 65536, 2]], device=cuda_device), 1, 4)
