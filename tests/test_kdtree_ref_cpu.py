"""CPU test (no GPU) of the reference the k-d tree tests stand on: kdtree_ref's float64 brute force against scipy.spatial.cKDTree on a
cloud without exact ties ('sheet': 7,502 points, two of them lone and far out).  Lattice clouds are not compared with scipy: its tie
rule is not stated."""
import numpy as np

import kdtree_ref as KR
import neighbors_ref as NR


def test_the_brute_force_nearest_neighbour_is_scipys_on_a_cloud_without_ties():
    P = NR.cloud('sheet').astype(np.float64)
    Q = KR.sheet_queries()
    assert P.shape == (7502, 3) and Q.shape == (3002, 3)
    idx, d2 = KR.nearest(P, Q)
    assert idx.dtype == np.int32 and d2.dtype == np.float64 and idx.min() >= 0
    KR.assert_same_as_scipy(np.sqrt(d2), idx, P, Q)


def test_the_brute_force_ball_lists_are_scipys_away_from_the_bound():
    from scipy.spatial import cKDTree
    P = NR.cloud('sheet').astype(np.float64)
    Q = KR.sheet_queries()[:1500]
    r = 0.002
    offsets, indices = KR.ball_point(P, Q, r)
    assert offsets[0] == 0 and offsets[-1] == len(indices) and np.array_equal(np.diff(offsets), NR.count_within(P, Q, r))
    d = np.sqrt(NR.d2_matrix(Q, P))
    assert (np.abs(d - r) <= 1e-12 * r).sum() == 0                           # no pair at the bound: the lists cannot differ by rounding
    want = cKDTree(P).query_ball_point(Q, r)
    for i in range(len(Q)):
        assert sorted(want[i]) == indices[offsets[i]:offsets[i + 1]].tolist()
    # and without a point
    offsets, indices = KR.ball_point(P[:0], Q[:5], r)
    assert offsets.tolist() == [0] * 6 and len(indices) == 0
    assert KR.nearest(P[:0], Q[:3])[0].tolist() == [-1] * 3
