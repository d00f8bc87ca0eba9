"""Float64 numpy brute force for the k-d tree searches on the grid index (include/catgrasp_amd_kdtree.h), and the query sets its tests
share.

d2 = (dx*dx + dy*dy) + dz*dz, float64 from the given coordinates, d = p_j - q (neighbors_ref.d2_matrix); the nearest neighbour is the
first minimum of a row (np.argmin: the smaller index on an exact tie); a ball list is the row's nonzero(d2 <= r*r), ascending."""
import functools

import numpy as np

import neighbors_ref as NR


def nearest(P, Q, chunk=512):
    """-> index (M) int32, d2 (M) float64 of the nearest point of P per query; (-1, +inf) without a point."""
    idx, d2 = np.full(len(Q), -1, np.int32), np.full(len(Q), np.inf)
    if len(P) == 0:
        return idx, d2
    for a in range(0, len(Q), chunk):
        m = NR.d2_matrix(Q[a:a + chunk], P)
        j = np.argmin(m, axis=1)
        idx[a:a + chunk], d2[a:a + chunk] = j, m[np.arange(len(j)), j]
    return idx, d2


def runner_up_gap(P, Q, chunk=512):
    """-> (M) float64: (second smallest d2 - smallest d2) / smallest d2 per query (inf where the smallest is 0 and the second is not):
    how far the answer is from a tie."""
    out = np.empty(len(Q))
    for a in range(0, len(Q), chunk):
        two = np.partition(NR.d2_matrix(Q[a:a + chunk], P), 1, axis=1)[:, :2]
        with np.errstate(divide='ignore', invalid='ignore'):
            out[a:a + chunk] = np.where(two[:, 1] > two[:, 0], (two[:, 1] - two[:, 0]) / two[:, 0], 0.0)
    return out


def ball_point(P, Q, radius, chunk=512):
    """-> offsets (M + 1) int64, indices int32: the points of P within `radius` of query i are indices[offsets[i]:offsets[i + 1]],
    ascending."""
    counts, lists = np.zeros(len(Q), np.int64), []
    for a in range(0, len(Q), chunk) if len(P) else ():
        rows, cols = np.nonzero(NR.d2_matrix(Q[a:a + chunk], P) <= radius * radius)        # row-major: ascending index per query
        counts[a:a + chunk] = np.bincount(rows, minlength=len(Q[a:a + chunk]))
        lists.append(cols.astype(np.int32))
    return np.concatenate(([0], np.cumsum(counts))).astype(np.int64), np.concatenate(lists + [np.zeros(0, np.int32)])


@functools.lru_cache(maxsize=None)
def sheet_queries():
    """The queries of the scipy comparison, float64 (3,002): the first 1,500 points of 'sheet' plus N(0, 2e-4), 1,500 uniform in its
    bounding box enlarged by its own extent on every side, and two far points.  Shared: never written to."""
    P = NR.cloud('sheet').astype(np.float64)
    rng = np.random.default_rng(3)
    jitter = P[:1500] + rng.normal(0, 2e-4, (1500, 3))
    lo, hi = P.min(axis=0), P.max(axis=0)
    uniform = rng.uniform(lo - (hi - lo), hi + (hi - lo), (1500, 3))
    Q = np.concatenate((jitter, uniform, [[1e3, -1e3, 5.0], [-1e6, 2e6, 1e6]]))
    Q.setflags(write=False)
    return Q


def assert_same_as_scipy(dist, idx, P, Q):
    """(dist, idx) against scipy.spatial.cKDTree(P).query(Q): equal indices wherever the runner-up's d2 exceeds the best by more than a
    relative 1e-12 (at most 1 % of the queries may be excused), distances within a relative 1e-14: both sides are fewer than ten
    float64 roundings of 1.1e-16 and a square root."""
    from scipy.spatial import cKDTree
    sd, si = cKDTree(P).query(Q)
    clear = runner_up_gap(P, Q) > 1e-12
    print(f'near ties: {int((~clear).sum())} of {len(Q)}; unequal indices: {int((si != idx).sum())}; '
          f'largest relative distance error: {float(np.max(np.abs(dist - sd) / sd)):.3g}')
    assert (~clear).sum() <= len(Q) // 100
    assert np.array_equal(np.asarray(idx)[clear], si[clear])
    assert np.all(np.abs(dist - sd) <= 1e-14 * sd)
