"""CPU tests (no GPU) of the grid index's references: the float64 brute force of tests/neighbors_ref.py answers what scipy's cKDTree
answers, and the test clouds have the properties the bars of tests/test_neighbors_gpu.py need -- no exact tie (or all of them, on purpose),
an eigenvalue gap, a view angle away from 90 degrees, lattice pairs on both sides of the bound."""
import numpy as np
import pytest

import neighbors_ref as N
import scene_ref as R


def _outside_queries(P):
    """Points just outside and far outside the cloud's box, and one 10 m away."""
    lo, hi = P.min(axis=0).astype(np.float64), P.max(axis=0).astype(np.float64)
    mid = (lo + hi) / 2
    return np.array([[lo[0] - 0.001, mid[1], 0.6], [hi[0] + 0.0015, mid[1], 0.6], [mid[0], lo[1] - 0.004, 0.6], [mid[0], hi[1] + 0.02, 0.6],
                     [lo[0] - 0.0049, lo[1] - 0.0001, lo[2]], [10.0, 0.0, 0.6], [0.0, 0.0, -9.4]])


@pytest.mark.parametrize('radius', [0.002, 0.005])
def test_brute_force_answers_what_ckdtree_answers(radius):
    cKDTree = pytest.importorskip('scipy.spatial').cKDTree
    P = N.cloud('sheet').astype(np.float64)
    Q = np.concatenate((P[::3] + np.random.default_rng(2).normal(0, 0.001, P[::3].shape), _outside_queries(P)))
    tree = cKDTree(P)
    counts = N.count_within(P, Q, radius)
    d2 = N.d2_matrix(Q, P)
    # away from the bound by more than rounding, the two count the same points; at this cloud every pair is
    assert (np.abs(np.sqrt(d2) - radius) > 1e-12).all()
    assert np.array_equal(counts, tree.query_ball_point(Q, r=radius, return_length=True))
    idx, best = N.nearest_within(P, Q, radius)
    dist, tidx = tree.query(Q, k=1, distance_upper_bound=radius)
    found = idx >= 0
    assert np.array_equal(found, np.isfinite(dist)) and 0 < int(found.sum()) < len(Q)
    part = np.partition(d2, 1, axis=1)
    unique = found & (part[:, 1] > part[:, 0])
    assert int(unique.sum()) >= int(found.sum()) - 5 and np.array_equal(idx[unique], tidx[unique])
    assert np.allclose(np.sqrt(best[found]), dist[found], rtol=1e-12, atol=0)
    assert (counts[-2:] == 0).all() and (idx[-2:] == -1).all() and np.isinf(best[-2:]).all()


def test_brute_force_ties_go_to_the_smaller_index_and_the_keep_set_ascends():
    P = N.cloud('sheet').copy()
    P[4000] = P[7]
    idx, d2 = N.nearest_within(P, P[[7, 4000]], 0.002)
    assert idx.tolist() == [7, 7] and d2.tolist() == [0.0, 0.0]
    assert N.count_within(P, P[[7]], 0.002)[0] == N.count_within(N.cloud('sheet'), P[[7]], 0.002)[0] + 1
    sheet = P[np.abs(P[:, 2] - 0.6) < 0.01]
    patch = sheet[np.linalg.norm(sheet[:, :2] - [0.01, -0.005], axis=1) < 0.008]
    kept, keep = N.cloudA_minus_cloudB(sheet, patch, 0.005)
    assert (np.diff(keep) > 0).all() and np.array_equal(kept, sheet[keep]) and 0 < len(keep) < len(sheet) - len(patch)
    gone = np.setdiff1d(np.arange(len(sheet)), keep)
    d = np.sqrt(N.d2_matrix(sheet, patch).min(axis=1))
    assert (d[keep] > 0.005).all() and (d[gone] <= 0.005).all()


@pytest.mark.parametrize('name,radius,max_nn', [('A_perm', 0.002, 30), ('sheet', 0.002, 30), ('sheet', 0.003, 30), ('sheet', 0.002, 8)])
def test_the_clouds_without_ties_have_the_gap_and_the_view_angle_the_normal_bars_need(name, radius, max_nn):
    ref = N.normals_ref(name, radius, max_nn)
    ok = ref['count'] >= 3
    lam = ref['lam']
    assert int(ref['tie'].sum()) == 0
    assert ((lam[ok, 1] - lam[ok, 0]) / lam[ok, 2]).min() >= 1e-3
    assert np.abs((ref['view'] * ref['normals']).sum(axis=1)).min() >= 1e-6
    assert int((~ok).sum()) == (1 if name == 'A_perm' else 2)             # the lone points
    assert int((ref['count'] == max_nn).sum()) > 400 and ref['count'].min() == 1                      # capped queries, and a lone point


def test_permuted_scene_b_has_exact_ties_that_the_opposite_rule_would_break():
    lo, hi = N.normals_ref('B_perm'), N.normals_ref('B_perm', prefer='high')
    assert int(lo['tie'].sum()) == 1450
    assert int((np.abs(hi['normals'] - lo['normals']).max(axis=1) > 1e-9).sum()) == 1450
    ok = lo['count'] >= 3
    assert ok.all() and ((lo['lam'][:, 1] - lo['lam'][:, 0]) / lo['lam'][:, 2]).min() >= 1e-3
    # the permutation is one: the row-major cloud's reference, permuted, is the permuted cloud's reference in count and d2max
    perm = np.random.default_rng(12).permutation(len(ok))
    assert np.array_equal(N.cloud('B')[perm], N.cloud('B_perm'))


def test_lattice_pairs_fall_on_both_sides_of_the_bound():
    r = 0.002
    for dtype, inside in ((np.float32, 5070), (np.float64, 7098)):
        P = N.mm_lattice(dtype)
        assert len(P) == 13 ** 3 and (P[:, 0] < 0).any() and (P[:, 0] > 0).any() and (P[:, 1] < 0).any() and (P[:, 1] > 0).any()
        steps = np.round(P.astype(np.float64) / 0.001).astype(int)
        nominal = ((steps[:, None, :] - steps[None, :, :]) ** 2).sum(axis=-1)
        d2 = N.d2_matrix(P, P)
        two = nominal == 4
        assert int(two.sum()) == 11154 and int((d2[two] <= r * r).sum()) == inside
        assert np.array_equal((d2 <= r * r)[~two], (nominal < 4)[~two])
    P = N.pow2_lattice()
    r = 2.0 ** -9
    d2 = N.d2_matrix(P, P)
    assert int((d2 == r * r).sum()) == 3402 and int((d2 <= r * r).sum(axis=1).max()) == 33
    assert int(R.organized_normals(P, r, 30)['tie'].sum()) == 335
